"""dfq_int_conv2d on the GPU (intmm.int_conv2d, utils.quantize.int_matmul_forward(conv=True),
main_dfq --int_matmul_conv): the integer convolution on the i8 matrix
instruction with zero padding as the real value 0, bit for bit the float64 statement of
tests/int_conv_cases.py."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import int_conv_cases as KC
from tests import mx_conv_cases as CC

pytestmark = pytest.mark.gpu
DEV = "cuda"

#: logits SQNR (dB) of the int_matmul_forward(conv=True) forward against the plain quantized
#: forward, as measured on an MI355X; the tests assert it minus 6 dB
MEASURED_LOGIT_SQNR_DB = {"mobilenetv2": 131.17, "resnet18": 131.64}


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _same_bits(got, want, what=""):
    g, w = _bits(got), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)
    assert g.shape == w.shape, what
    bad = np.argwhere(g != w)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), got.detach().cpu().numpy()[tuple(bad[0])], want[tuple(bad[0])])


def _call(name, config, x, w, zb=True, bias=True, **kw):
    """intmm.int_conv2d of geometry ``name`` under configuration ``config`` of tests/int_conv_cases.py."""
    from data_free_quantization_amd import intmm
    g = KC.GEOMS[name]
    bits, sym, dev, f32, b_signed, per_row, packed = KC.CONFIGS[config]
    mn, mx = KC.SYM_RANGE if sym else KC.ASYM_RANGE
    rng = dict(min_dev=torch.tensor([mn], device=DEV), max_dev=torch.tensor([mx], device=DEV)) if dev else \
        dict(min_value=mn, max_value=mx)
    return intmm.int_conv2d(_dev(x), _dev(w.b_bytes), _dev(w.sb), _dev(w.zb) if zb else None, g.kernel, g.stride, g.padding,
                            g.dilation, bits=bits, symmetric=sym, scale_f32=f32, b_packed=bool(packed),
                            bias=_dev(w.bias) if bias else None, **rng, **kw)


@pytest.mark.parametrize("config", list(KC.CONFIGS))
@pytest.mark.parametrize("name", list(KC.GEOMS))
def test_int_conv2d_equals_the_statement_bit_for_bit(name, config):
    """Every geometry under: 8-bit asymmetric with a device range and per-row unsigned B; 8-bit
    symmetric with a host range and per-tensor signed B; 4-bit asymmetric with scale_f32 and
    packed signed B.  x holds values outside the range, its ends, zeros and (asymmetric) ties and
    their nextafter; the asymmetric range (-1.3, 2.5) keeps 0 off the grid, so the code of 0.0
    in place of a padding tap would show.  Packed B with an odd K is refused, as the header says."""
    from data_free_quantization_amd import intmm
    g = KC.GEOMS[name]
    if KC.CONFIGS[config][6] and CC.K(g) % 2:
        w = KC.weights(g, 1, 1, 0)
        x = KC.make_x(g, KC.ASYM_RANGE, 4, False)
        packed = torch.zeros(g.N * (CC.K(g) // 2 + 1), dtype=torch.int8, device=DEV)
        with pytest.raises(ValueError, match="even K"):
            intmm.int_conv2d(_dev(x), packed, _dev(w.sb), _dev(w.zb), g.kernel, g.stride, g.padding, g.dilation, bits=4,
                             min_value=-1.3, max_value=2.5, b_packed=True)
        return
    x, w, want = KC.expected(name, config)
    intmm.reset_linear_calls()
    got = _call(name, config, x, w)
    assert intmm.LINEAR_CALLS == 1
    oh, ow = CC.out_size(g)
    assert got.shape == (g.B, g.N, oh, ow) and got.is_contiguous()
    _same_bits(got, want, (name, config))
    if name in KC.PADDED and not KC.CONFIGS[config][1]:
        _, _, coded = KC.expected(name, config, x=x, code_of_zero=True)
        assert not np.array_equal(_bits(got), coded.view(np.uint32))   # and it is not the other rule


@pytest.mark.parametrize("name", ["g", "h", "nopad"])
def test_without_padding_it_is_int_linear_on_the_unfold_matrix(name):
    """Bit for bit intmm.int_linear on the materialised F.unfold matrix, reshaped to NCHW; the
    pointwise geometries also with ``padding`` given as a tuple."""
    from data_free_quantization_amd import intmm
    g = KC.GEOMS[name]
    x, w, want = KC.expected(name, "a8-dev-rowu")
    xd = _dev(x)
    cols = F.unfold(xd, g.kernel, g.dilation, g.padding, g.stride)
    a = cols.transpose(1, 2).reshape(-1, cols.shape[1]).contiguous()
    mn, mx = (torch.tensor([t], device=DEV) for t in KC.ASYM_RANGE)
    wq = (_dev(w.b_bytes), _dev(w.sb), _dev(w.zb))
    lin = intmm.int_linear(a, *wq, CC.K(g), min_dev=mn, max_dev=mx, bias=_dev(w.bias))
    oh, ow = CC.out_size(g)
    lin = lin.view(g.B, oh, ow, g.N).permute(0, 3, 1, 2).contiguous()
    got = _call(name, "a8-dev-rowu", x, w)
    assert torch.equal(got.view(torch.int32), lin.view(torch.int32))
    _same_bits(got, want)
    if g.kernel == (1, 1):
        for pad in ((0, 0), [0, 0]):
            again = intmm.int_conv2d(xd, *wq, 1, g.stride, pad, 1, min_dev=mn, max_dev=mx, bias=_dev(w.bias))
            assert torch.equal(again.view(torch.int32), lin.view(torch.int32))


@pytest.mark.parametrize("name", ["a", "c", "d", "f"])
def test_against_the_fp32_convolution(name):
    """|int_conv2d - F.conv2d(x^, w^, b^)| <= (K + 6) u S + u |b^| per element, u = 2^-24, with S the
    convolution of (|x^| + |za|) v with |w^| + |zb| (DESIGN.md 3.9's bound for int_linear, the
    padding taps out of S as they are out of the sums).  The "code of zero" rule -- a padding tap
    standing for q0 s + min -- misses it; on ``f`` the rows wholly in padding are (float)bias."""
    from data_free_quantization_amd import intmm
    from data_free_quantization_amd.utils.quantize import fake_quant
    g = KC.GEOMS[name]
    K = CC.K(g)
    gen = torch.Generator(device="cpu").manual_seed(K)
    x = (torch.randn(g.B, g.C, g.H, g.W, generator=gen) * 1.2 + 0.4).to(DEV)
    w = (torch.randn(g.N, K, generator=gen) * 0.05).to(DEV)
    b = torch.randn(g.N, generator=gen).to(DEV)
    mn, mx = KC.ASYM_RANGE
    xr = fake_quant(x.reshape(1, -1), 8, min_value=mn, max_value=mx)
    wr = fake_quant(w, 8)
    xq = xr.dq.view_as(x)
    got = intmm.int_conv2d(x, wr.codes, wr.scale, wr.zero, g.kernel, g.stride, g.padding, g.dilation, min_value=mn, max_value=mx, bias=b)
    geo = dict(stride=g.stride, padding=g.padding, dilation=g.dilation)
    ref = F.conv2d(xq, wr.dq.view(g.N, g.C, *g.kernel), b, **geo)
    cpu = lambda t: t.detach().cpu().double()   # noqa: E731
    S = F.conv2d(cpu(xq).abs() + cpu(xr.zero).abs(), (cpu(wr.dq).abs() + cpu(wr.zero).abs()).view(g.N, g.C, *g.kernel),
                 None, **geo).to(DEV)   # in float64 on the CPU; zero padding: the taps outside the image are out of S
    u = 2.0 ** -24
    bound = (K + 6) * u * S + u * b.double().abs().view(1, -1, 1, 1)
    err = (got.double() - ref.double()).abs()
    print("%s: worst |int_conv2d - F.conv2d| / bound: %.4f" % (name, float((err / bound).max())))
    assert bool((err <= bound).all())
    # feeding x^ instead of x changes nothing: the quantizer gives the fake quant's codes back
    again = intmm.int_conv2d(xq.contiguous(), wr.codes, wr.scale, wr.zero, g.kernel, g.stride, g.padding, g.dilation, min_value=mn,
                             max_value=mx, bias=b)
    assert torch.equal(got, again)
    # the other rule, from the same codes, is outside the bound
    v = KC.taps(g)
    qa = xr.codes.view_as(x).float()
    cols = F.unfold(qa, g.kernel, g.dilation, g.padding, g.stride)
    q0 = float(fake_quant(torch.zeros(1, 1, device=DEV), 8, min_value=mn, max_value=mx).codes.item())
    qa2d = cols.transpose(1, 2).reshape(-1, K).cpu().numpy().astype(np.int64)
    qa2d = np.where(v == 1, qa2d, int(q0))
    args = (qa2d, v, wr.codes.cpu().numpy().astype(np.int64), xr.scale.cpu().numpy(), xr.zero.cpu().numpy(), wr.scale.cpu().numpy(),
            wr.zero.cpu().numpy(), b.cpu().numpy())
    _same_bits(got, KC.nchw(KC.statement(*args), g))
    coded = torch.from_numpy(KC.nchw(KC.statement(*args, code_of_zero=True), g)).to(DEV)
    assert bool(((coded.double() - ref.double()).abs() > bound).any())
    if name == "f":
        rows = torch.from_numpy(KC.nchw((v.sum(1) == 0)[:, None].repeat(g.N, 1), g)).to(DEV)
        assert bool(rows.any()) and torch.equal(got[rows], b.view(1, -1, 1, 1).expand_as(got)[rows])


@pytest.mark.parametrize("name,config", [("a", "a8-dev-rowu"), ("e", "s8-host-tens"), ("b", "a4-f32-pack")])
def test_null_zero_and_bias_skip_their_terms(name, config):
    x, w, _ = KC.expected(name, config)
    for zb, bias in ((False, True), (True, False), (False, False)):
        _, _, want = KC.expected(name, config, x=x, zb=zb, bias=bias)
        _same_bits(_call(name, config, x, w, zb=zb, bias=bias), want, (zb, bias))


def test_same_bits_from_run_to_run_and_a_guard_region_stays_untouched():
    x, w, want = KC.expected("c", "a8-dev-rowu")
    first = _call("c", "a8-dev-rowu", x, w)
    pad = torch.empty(4096 + 16, dtype=torch.uint8, device=DEV)   # moves the next allocations
    again = _call("c", "a8-dev-rowu", x, w)
    assert torch.equal(first, again) and pad.numel()
    n = first.numel()
    buf = torch.full((n + 64,), -7.25, device=DEV)
    out = buf[31:31 + n].view(first.shape)   # 4-B aligned only: the 16-B stores are not 16-B aligned
    got = _call("c", "a8-dev-rowu", x, w, out=out)
    assert got.data_ptr() == out.data_ptr()
    _same_bits(out, want)
    assert (buf[:31] == -7.25).all() and (buf[31 + n:] == -7.25).all()
    for name in ("one_pixel", "three_pixels"):   # a lane's four rows span several images
        x, w, want = KC.expected(name, "a8-dev-rowu")
        n = want.size
        buf = torch.full((n + 64,), -7.25, device=DEV)
        _same_bits(_call(name, "a8-dev-rowu", x, w, out=buf[32:32 + n].view(want.shape)), want)
        assert (buf[:32] == -7.25).all() and (buf[32 + n:] == -7.25).all()


def test_python_argument_checks_on_the_device():
    from data_free_quantization_amd import intmm
    g = KC.GEOMS["a"]
    x, w, _ = KC.expected("a", "a8-dev-rowu")
    x, wq = _dev(x), (_dev(w.b_bytes), _dev(w.sb), _dev(w.zb))
    rng = dict(min_value=-1.0, max_value=1.0)
    with pytest.raises(ValueError):
        intmm.int_conv2d(x, *wq, 5, padding=1, **rng)                           # the codes hold no rows of K = C * 25
    with pytest.raises(ValueError):
        intmm.int_conv2d(x, *wq, 3, padding=1)                                  # no range
    with pytest.raises(ValueError):
        intmm.int_conv2d(x[0], *wq, 3, padding=1, **rng)                        # not 4-D
    with pytest.raises(ValueError):
        intmm.int_conv2d(x.permute(0, 1, 3, 2), *wq, 3, padding=1, **rng)       # not contiguous
    with pytest.raises(TypeError):
        intmm.int_conv2d(x.double(), *wq, 3, padding=1, **rng)
    with pytest.raises(ValueError):
        intmm.int_conv2d(x, *wq, 3, padding=1, out=torch.empty(g.B, g.N, 5, 5, device=DEV), **rng)
    with pytest.raises(ValueError):
        intmm.int_conv2d(x, *wq, 3, padding=1, bias=torch.zeros(g.N + 1, device=DEV), **rng)
    with pytest.raises(ValueError):
        intmm.int_conv2d(x, *wq, 3, padding=1, dilation=5, **rng)               # the dilated kernel does not fit
    with pytest.raises(ValueError):
        intmm.int_conv2d(x, *wq, 3, padding=-1, **rng)
    with pytest.raises(ValueError):
        intmm.int_conv2d(torch.zeros(1, intmm.MAX_K // 9 + 1, 3, 3, device=DEV), *wq, 3, **rng)   # K > MAX_K


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


def _scope_run(name, n_layers, n_conv, n_plain):
    """Forwards of the quantized model outside the scope, with conv=False and with conv=True;
    the call counts, that the layers the scope leaves alone are bit for bit what they are outside
    it on the same input, that two forwards and a frozen_weights() forward are identical, the
    argmax, and the logit SQNR against the plain forward (asserted at the recorded value less
    6 dB: F.conv2d's accumulation order differs between library builds, and one flipped
    downstream activation code costs an 8-bit step)."""
    from data_free_quantization_amd import intmm
    from data_free_quantization_amd.utils import layer_transform as L
    from data_free_quantization_amd.utils.quantize import QuantConv2d, QuantLinear, frozen_weights, int_matmul_forward
    x = torch.randn(2, 3, 32, 32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    try:
        model = _quantized(name, x)
        layers = [m for m in model.modules() if isinstance(m, (QuantConv2d, QuantLinear))]
        others = [m for m in layers if isinstance(m, QuantConv2d) and m.groups > 1]
        assert len(layers) == n_layers and len(others) == n_layers - n_conv
        seen = {}
        hooks = [m.register_forward_hook(lambda mod, inp, out: seen.__setitem__(mod, (inp[0].detach().clone(), out.detach().clone())))
                 for m in others]
        L.replace_op()
        try:
            with torch.no_grad():
                plain = model(x)
                with int_matmul_forward():
                    model(x)
                    calls_plain_scope = intmm.LINEAR_CALLS
                with int_matmul_forward(conv=True):
                    routed = model(x)
                    calls = intmm.LINEAR_CALLS
                    inside = dict(seen)
                    assert all(not m._int_routed() for m in others)
                    assert all(m._int_routed() for m in layers if m not in others)
                    again = model(x)
                    with frozen_weights():
                        frozen = model(x)
                        cached = model(x)
                    assert intmm.LINEAR_CALLS == 4 * n_conv
                for h in hooks:
                    h.remove()
                for m, (inp, out) in inside.items():
                    assert torch.equal(m(inp), out)
                assert torch.equal(model(x), plain)   # outside the scope again: the parent's forward
        finally:
            L.restore_op()
    finally:
        L.module_tensor_op = None
    assert (calls, calls_plain_scope) == (n_conv, n_plain)
    assert torch.isfinite(routed).all() and routed.shape == plain.shape
    assert torch.equal(routed, again) and torch.equal(routed, frozen) and torch.equal(routed, cached)
    assert torch.equal(routed.argmax(1), plain.argmax(1))
    noise = (routed.double() - plain.double()).pow(2).sum()
    sqnr = 10 * np.log10(float(plain.double().pow(2).sum() / noise)) if float(noise) > 0 else float("inf")
    print("%s on the i8 matrix instruction: %d of %d layers routed, logits SQNR %.2f dB against the plain forward"
          % (name, calls, n_layers, sqnr))
    assert MEASURED_LOGIT_SQNR_DB[name] is not None, "record the measured SQNR (printed above)"
    assert sqnr >= MEASURED_LOGIT_SQNR_DB[name] - 6.0


def test_quantized_mobilenetv2_in_the_forward_scope():
    """Batch 2 at 32 x 32: conv=True makes 36 calls per forward (the stem joins), 35 with
    conv=False in the same run; the 17 depthwise layers are untouched."""
    _scope_run("mobilenetv2", 53, 36, 35)


def test_quantized_resnet18_in_the_forward_scope():
    """Batch 2 at 32 x 32: all 21 layers are routed (4 with conv=False: the three 1x1
    downsample convolutions and the classifier)."""
    _scope_run("resnet18", 21, 21, 4)


def test_main_dfq_int_matmul_conv_end_to_end(tmp_path, monkeypatch):
    """main_dfq --int_matmul --int_matmul_conv evaluates a synthetic image folder and writes the
    fields it writes without the flags."""
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
    for extra, calls in (([], 0), (["--int_matmul", "--int_matmul_conv"], 36)):
        (tmp_path / "dfq_result.txt").unlink(missing_ok=True)
        intmm.reset_linear_calls()
        _, _, acc = main_dfq.main(argv + extra)
        assert acc is not None and 0.0 <= acc <= 1.0
        assert intmm.LINEAR_CALLS == calls
        text = (tmp_path / "dfq_result.txt").read_text()
        assert "Accuracy: " in text
        fields.append([ln.split(":")[0] for ln in text.splitlines() if ":" in ln])
    assert fields[0] == fields[1]
