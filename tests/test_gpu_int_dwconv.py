"""dfq_int_dwconv2d on the GPU (intmm.int_dwconv2d, utils.quantize.int_matmul_forward(conv=True,
depthwise=True), main_dfq --int_matmul_depthwise): the integer depthwise
convolution on the packed 8-bit dot instruction with zero padding as the real value 0, bit for
bit the float64 statement of tests/int_dwconv_cases.py."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import int_conv_cases as KC
from tests import int_dwconv_cases as DC

pytestmark = pytest.mark.gpu
DEV = "cuda"

#: logits SQNR (dB) of the int_matmul_forward(conv=True, depthwise=True) forward against the plain
#: quantized forward, as measured on an MI355X; the test asserts it minus 6 dB
MEASURED_LOGIT_SQNR_DB = {"mobilenetv2": 131.17}


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(DEV)   # a copy: the cases are read-only


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _same_bits(got, want, what=""):
    g, w = _bits(got), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)
    assert g.shape == w.shape, what
    bad = np.argwhere(g != w)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), got.detach().cpu().numpy()[tuple(bad[0])], want[tuple(bad[0])])


def _range_kw(config):
    bits, sym, dev, f32, b_signed, per_row, packed = DC.CONFIGS[config]
    mn, mx = DC.SYM_RANGE if sym else DC.ASYM_RANGE
    return dict(min_dev=torch.tensor([mn], device=DEV), max_dev=torch.tensor([mx], device=DEV)) if dev else \
        dict(min_value=mn, max_value=mx)


def _call(name, config, x, w, zb=True, bias=True, **kw):
    """intmm.int_dwconv2d of geometry ``name`` under configuration ``config`` of tests/int_dwconv_cases.py."""
    from data_free_quantization_amd import intmm
    g = DC.GEOMS[name]
    bits, sym, dev, f32, b_signed, per_row, packed = DC.CONFIGS[config]
    return intmm.int_dwconv2d(_dev(x), _dev(w.b_bytes), _dev(w.sb), _dev(w.zb) if zb else None, g.kernel, g.stride, g.padding,
                              g.dilation, bits=bits, symmetric=sym, scale_f32=f32, b_packed=bool(packed),
                              bias=_dev(w.bias) if bias else None, **_range_kw(config), **kw)


@pytest.mark.parametrize("config", list(DC.CONFIGS))
@pytest.mark.parametrize("name", list(DC.GEOMS))
def test_int_dwconv2d_equals_the_statement_bit_for_bit(name, config):
    """Every geometry under KC's three configurations: 8-bit asymmetric with a device range and
    per-row unsigned B; 8-bit symmetric with a host range and per-tensor signed B; 4-bit asymmetric
    with scale_f32 and packed signed B.  The asymmetric range (-1.3, 2.5) keeps 0 off the grid, so
    the code of 0.0 in place of a padding tap would show.  Packed B with an odd K is refused."""
    from data_free_quantization_amd import intmm
    g = DC.GEOMS[name]
    if DC.CONFIGS[config][6] and DC.K(g) % 2:
        w = DC.weights(g, 1, 1, 0)
        x = DC.make_x(g, DC.ASYM_RANGE, 4, False)
        packed = torch.zeros(DC.N(g) * (DC.K(g) // 2 + 1), dtype=torch.int8, device=DEV)
        with pytest.raises(ValueError, match="even K"):
            intmm.int_dwconv2d(_dev(x), packed, _dev(w.sb), _dev(w.zb), g.kernel, g.stride, g.padding, g.dilation, bits=4,
                               min_value=-1.3, max_value=2.5, b_packed=True)
        return
    x, w, want = DC.expected(name, config)
    intmm.reset_linear_calls()
    got = _call(name, config, x, w)
    assert intmm.LINEAR_CALLS == 1
    assert got.shape == (g.B, DC.N(g), *DC.out_size(g)) and got.is_contiguous()
    _same_bits(got, want, (name, config))
    if name in DC.PADDED and config == "a8-dev-rowu":
        coded = DC.expected(name, config, code_of_zero=True)[2]
        assert not np.array_equal(_bits(got), coded.view(np.uint32))   # and it is not the other rule


@pytest.mark.parametrize("config", ["a8-dev-rowu", "s8-host-tens"])
@pytest.mark.parametrize("name", ["mnv2_s1", "mult2", "dilated", "deep_pad"])
def test_each_channel_is_int_conv2d_on_that_channel(name, config):
    """An independent check on the device: both kernels implement the same statement, so channel
    c's output equals intmm.int_conv2d on x[:, c:c+1] with that channel's rows of B, bit for bit."""
    from data_free_quantization_amd import intmm
    g = DC.GEOMS[name]
    bits, sym, dev, f32, b_signed, per_row, packed = DC.CONFIGS[config]
    x, w, want = DC.expected(name, config)
    got = _call(name, config, x, w)
    xd, codes, sb, zb, bias = _dev(x), _dev(w.b_bytes).view(DC.N(g), DC.K(g)), _dev(w.sb), _dev(w.zb), _dev(w.bias)
    for c in range(g.C):
        rows = slice(c * g.mult, (c + 1) * g.mult)
        par = lambda t: t[rows].clone() if t.numel() > 1 else t   # noqa: E731
        one = intmm.int_conv2d(xd[:, c:c + 1].contiguous(), codes[rows].clone(), par(sb), par(zb), g.kernel, g.stride, g.padding,
                               g.dilation, bits=bits, symmetric=sym, scale_f32=f32, bias=bias[rows].clone(), **_range_kw(config))
        assert torch.equal(got[:, rows].contiguous().view(torch.int32), one.view(torch.int32)), (name, config, c)
    _same_bits(got, want)


@pytest.mark.parametrize("name", ["mnv2_s1", "mnv2_s2", "dilated", "deep_pad"])
def test_against_the_fp32_depthwise_convolution(name):
    """|int_dwconv2d - F.conv2d(x^, w^, b^, groups=C)| <= (K + 6) u S + u |b^| per element, u = 2^-24,
    K = KH * KW, with S the float64 CPU grouped convolution of |x^| + |za| with |w^| + |zb|
    (DESIGN.md 3.9's bound, test_against_the_fp32_convolution's).  The code-of-zero rule from the
    same codes misses it; feeding x^ instead of x changes no bit."""
    from data_free_quantization_amd import intmm
    from data_free_quantization_amd.utils.quantize import fake_quant
    g = DC.GEOMS[name]
    K, N = DC.K(g), DC.N(g)
    gen = torch.Generator(device="cpu").manual_seed(K + g.C)
    x = (torch.randn(g.B, g.C, g.H, g.W, generator=gen) * 1.2 + 0.4).to(DEV)
    w = (torch.randn(N, K, generator=gen) * 0.05).to(DEV)
    b = torch.randn(N, generator=gen).to(DEV)
    mn, mx = DC.ASYM_RANGE
    xr = fake_quant(x.reshape(1, -1), 8, min_value=mn, max_value=mx)
    wr = fake_quant(w, 8)
    xq = xr.dq.view_as(x)
    got = intmm.int_dwconv2d(x, wr.codes, wr.scale, wr.zero, g.kernel, g.stride, g.padding, g.dilation, min_value=mn, max_value=mx, bias=b)
    geo = dict(stride=g.stride, padding=g.padding, dilation=g.dilation, groups=g.C)
    ref = F.conv2d(xq, wr.dq.view(N, 1, *g.kernel), b, **geo)
    cpu = lambda t: t.detach().cpu().double()   # noqa: E731
    S = F.conv2d(cpu(xq).abs() + cpu(xr.zero).abs(), (cpu(wr.dq).abs() + cpu(wr.zero).abs()).view(N, 1, *g.kernel),
                 None, **geo).to(DEV)   # in float64 on the CPU; zero padding: the taps outside the image are out of S
    u = 2.0 ** -24
    bound = (K + 6) * u * S + u * b.double().abs().view(1, -1, 1, 1)
    err = (got.double() - ref.double()).abs()
    print("%s: worst |int_dwconv2d - F.conv2d| / bound: %.4f" % (name, float((err / bound).max())))
    assert bool((err <= bound).all())
    # feeding x^ instead of x changes nothing: the quantizer gives the fake quant's codes back
    again = intmm.int_dwconv2d(xq.contiguous(), wr.codes, wr.scale, wr.zero, g.kernel, g.stride, g.padding, g.dilation, min_value=mn,
                               max_value=mx, bias=b)
    assert torch.equal(got, again)
    # the other rule, from the same codes, is outside the bound
    g1 = DC.one_channel(g)
    v = KC.taps(g1)
    qa = xr.codes.view_as(x).float()
    q0 = int(fake_quant(torch.zeros(1, 1, device=DEV), 8, min_value=mn, max_value=mx).codes.item())
    qb = wr.codes.cpu().numpy().astype(np.int64)
    par = [t.cpu().numpy() for t in (xr.scale, xr.zero, wr.scale, wr.zero)]
    real, coded = [], []
    for c in range(g.C):
        cols = F.unfold(qa[:, c:c + 1], g.kernel, g.dilation, g.padding, g.stride)
        qa2d = np.where(v == 1, cols.transpose(1, 2).reshape(-1, K).cpu().numpy().astype(np.int64), q0)
        rows = slice(c * g.mult, (c + 1) * g.mult)
        args = (qa2d, v, qb[rows], par[0], par[1], par[2], par[3], b.cpu().numpy()[rows])
        real.append(KC.nchw(KC.statement(*args), g1))
        coded.append(KC.nchw(KC.statement(*args, code_of_zero=True), g1))
    _same_bits(got, np.concatenate(real, axis=1))
    coded = torch.from_numpy(np.concatenate(coded, axis=1)).to(DEV)
    assert bool(((coded.double() - ref.double()).abs() > bound).any())
    if name == "deep_pad":
        rows = torch.from_numpy(KC.nchw((v.sum(1) == 0)[:, None].repeat(g.mult, 1), g1)).to(DEV).expand_as(got)
        assert int(rows[0, 0].sum()) == 28 and torch.equal(got[rows], b.view(1, -1, 1, 1).expand_as(got)[rows])


@pytest.mark.parametrize("name,config", [("mnv2_s1", "a8-dev-rowu"), ("asym", "s8-host-tens"), ("even_k_pad", "a4-f32-pack")])
def test_null_zero_and_bias_skip_their_terms(name, config):
    x, w, _ = DC.expected(name, config)
    for zb, bias in ((False, True), (True, False), (False, False)):
        want = DC.expected(name, config, zb=zb, bias=bias)[2]
        _same_bits(_call(name, config, x, w, zb=zb, bias=bias), want, (zb, bias))


def test_same_bits_from_run_to_run_and_a_guard_region_stays_untouched():
    x, w, want = DC.expected("k7_s2", "a8-dev-rowu")
    first = _call("k7_s2", "a8-dev-rowu", x, w)
    pad = torch.empty(4096 + 16, dtype=torch.uint8, device=DEV)   # moves the next allocations
    again = _call("k7_s2", "a8-dev-rowu", x, w)
    assert torch.equal(first, again) and pad.numel()
    _same_bits(first, want)
    for name in ("wide", "one_pixel", "deep_pad"):
        x, w, want = DC.expected(name, "a8-dev-rowu")
        n = want.size
        buf = torch.full((n + 64,), -7.25, device=DEV)
        out = buf[31:31 + n].view(want.shape)   # 4-B aligned only: the 16-B stores are not 16-B aligned
        got = _call(name, "a8-dev-rowu", x, w, out=out)
        assert got.data_ptr() == out.data_ptr()
        _same_bits(out, want, name)
        assert (buf[:31] == -7.25).all() and (buf[31 + n:] == -7.25).all()


def test_python_argument_checks_on_the_device():
    from data_free_quantization_amd import intmm
    g = DC.GEOMS["mnv2_s1"]
    x, w, _ = DC.expected("mnv2_s1", "a8-dev-rowu")
    x, wq = _dev(x), (_dev(w.b_bytes), _dev(w.sb), _dev(w.zb))
    rng = dict(min_value=-1.0, max_value=1.0)
    with pytest.raises(ValueError):
        intmm.int_dwconv2d(x, *wq, 5, padding=2, **rng)                          # the codes hold no rows of K = 25
    with pytest.raises(ValueError, match="multiple"):
        intmm.int_dwconv2d(x[:, :3].contiguous(), *wq, 3, padding=1, **rng)      # N = 5 rows for C = 3
    with pytest.raises(ValueError):
        intmm.int_dwconv2d(x, *wq, 3, padding=1)                                 # no range
    with pytest.raises(ValueError):
        intmm.int_dwconv2d(x[0], *wq, 3, padding=1, **rng)                       # not 4-D
    with pytest.raises(ValueError):
        intmm.int_dwconv2d(x.permute(0, 1, 3, 2), *wq, 3, padding=1, **rng)      # not contiguous
    with pytest.raises(TypeError):
        intmm.int_dwconv2d(x.double(), *wq, 3, padding=1, **rng)
    with pytest.raises(ValueError):
        intmm.int_dwconv2d(x, *wq, 3, padding=1, out=torch.empty(g.B, g.C, 5, 5, device=DEV), **rng)
    with pytest.raises(ValueError):
        intmm.int_dwconv2d(x, *wq, 3, padding=1, bias=torch.zeros(g.C + 1, device=DEV), **rng)
    with pytest.raises(ValueError):
        intmm.int_dwconv2d(x, *wq, 3, padding=1, dilation=5, **rng)              # the dilated kernel does not fit
    with pytest.raises(ValueError):
        intmm.int_dwconv2d(x, *wq, 3, padding=-1, **rng)
    with pytest.raises(ValueError):
        intmm.int_dwconv2d(x, *wq, (5, 13), padding=6, **rng)                    # 65 taps


# ---- the forward scope ------------------------------------------------------------------
def _quantized(name, x):
    """The zoo's model after --relu --equalize --absorption --quantize, observers fixed."""
    from data_free_quantization_amd import pipeline, zoo
    from data_free_quantization_amd.utils import layer_transform as L
    from data_free_quantization_amd.utils.quantize import QuantConv2d, QuantLinear
    from data_free_quantization_amd.utils.tracer import TorchTransformer
    model = zoo.build(name, seed=0, relu=True).to(DEV).eval()
    tr = TorchTransformer("positional")
    model, tr = L.switch_layers(model, tr, x, {1: [(nn.Conv2d, QuantConv2d), (nn.Linear, QuantLinear)]})
    graph, bottoms = tr.log.getGraph(), tr.log.getBottoms()
    pipeline.run_dfq(model, graph, bottoms, (QuantConv2d, QuantLinear), bc_mode="fused", clip=False, correction=False)
    L.set_quant_minmax(graph, bottoms, verbose=False)
    model.eval()
    for m in graph.values():   # fixed observers, so every forward sees the same ranges
        if hasattr(m, "quant"):
            m.quant.update_stat = False
    for q in L.module_tensor_op.quants:
        q.update_stat = False
    return model


def test_quantized_mobilenetv2_is_integer_in_every_product():
    """Batch 2 at 32 x 32: conv=True, depthwise=True makes 53 calls per forward -- every Conv2d /
    Linear is routed -- and 36 with depthwise=False in the same run; two forwards, a
    frozen_weights() forward and its cached repeat are identical; the argmax is the plain
    forward's; the logit SQNR against the plain forward is asserted at the recorded value less
    6 dB (F.conv2d's accumulation order differs between library builds, and one flipped downstream
    activation code costs an 8-bit step)."""
    from data_free_quantization_amd import intmm
    from data_free_quantization_amd.utils import layer_transform as L
    from data_free_quantization_amd.utils.quantize import QuantConv2d, QuantLinear, frozen_weights, int_matmul_forward
    name = "mobilenetv2"
    x = torch.randn(2, 3, 32, 32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    try:
        model = _quantized(name, x)
        layers = [m for m in model.modules() if isinstance(m, (QuantConv2d, QuantLinear))]
        depthwise = [m for m in layers if isinstance(m, QuantConv2d) and m.groups > 1]
        assert len(layers) == 53 and len(depthwise) == 17
        L.replace_op()
        try:
            with torch.no_grad():
                plain = model(x)
                with int_matmul_forward(conv=True):
                    model(x)
                    calls_conv = intmm.LINEAR_CALLS
                    assert not any(m._int_routed() for m in depthwise)
                with int_matmul_forward(conv=True, depthwise=True):
                    routed = model(x)
                    calls = intmm.LINEAR_CALLS
                    assert all(m._int_routed() for m in layers) and all(m._int_dw_routed() for m in depthwise)
                    again = model(x)
                    with frozen_weights():
                        frozen = model(x)
                        cached = model(x)
                    assert intmm.LINEAR_CALLS == 4 * 53
                assert torch.equal(model(x), plain)   # outside the scope again: the parent's forward
        finally:
            L.restore_op()
    finally:
        L.module_tensor_op = None
    assert (calls, calls_conv) == (53, 36)
    assert torch.isfinite(routed).all() and routed.shape == plain.shape
    assert torch.equal(routed, again) and torch.equal(routed, frozen) and torch.equal(routed, cached)
    assert torch.equal(routed.argmax(1), plain.argmax(1))
    noise = (routed.double() - plain.double()).pow(2).sum()
    sqnr = 10 * np.log10(float(plain.double().pow(2).sum() / noise)) if float(noise) > 0 else float("inf")
    print("%s with every product an integer one: %d of %d layers routed, logits SQNR %.2f dB against the plain forward"
          % (name, calls, len(layers), sqnr))
    assert MEASURED_LOGIT_SQNR_DB[name] is not None, "record the measured SQNR (printed above)"
    assert sqnr >= MEASURED_LOGIT_SQNR_DB[name] - 6.0


def test_main_dfq_int_matmul_depthwise_end_to_end(tmp_path, monkeypatch):
    """main_dfq --int_matmul --int_matmul_conv --int_matmul_depthwise evaluates a four-image
    synthetic folder with 53 integer products and writes the fields it writes without the flags."""
    from PIL import Image
    from data_free_quantization_amd import intmm, main_dfq
    rng = np.random.default_rng(0)
    for c in range(2):
        d = tmp_path / "val" / f"n{c:08d}"
        d.mkdir(parents=True)
        for k in range(2):
            Image.fromarray(rng.integers(0, 256, (240, 300, 3), dtype=np.uint8)).save(d / f"{k}.png")
    monkeypatch.chdir(tmp_path)
    argv = ["--task", "cls", "--relu", "--equalize", "--absorption", "--quantize", "--val", str(tmp_path / "val"),
            "--batch_size", "4", "--workers", "0", "--log"]
    fields = []
    for extra, calls in (([], 0), (["--int_matmul", "--int_matmul_conv", "--int_matmul_depthwise"], 53)):
        (tmp_path / "dfq_result.txt").unlink(missing_ok=True)
        intmm.reset_linear_calls()
        _, _, acc = main_dfq.main(argv + extra)
        assert acc is not None and 0.0 <= acc <= 1.0
        assert intmm.LINEAR_CALLS == calls
        text = (tmp_path / "dfq_result.txt").read_text()
        assert "Accuracy: " in text
        fields.append([ln.split(":")[0] for ln in text.splitlines() if ":" in ln])
    assert fields[0] == fields[1]
