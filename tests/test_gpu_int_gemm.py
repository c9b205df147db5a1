"""dfq_int_gemm / dfq_int_linear on the GPU (intmm.int_gemm, intmm.int_linear,
utils.quantize.int_matmul_forward, main_dfq --int_matmul): the integer
product of the sweep's codes on the i8 matrix instruction, bit for bit the float64
statement of tests/int_gemm_cases.py."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import oracle
from tests import int_gemm_cases as IC

pytestmark = pytest.mark.gpu
DEV = "cuda"

#: logits SQNR (dB) of the int_matmul_forward MobileNetV2 forward against the plain quantized
#: forward, as measured on an MI355X; the test asserts it minus 6 dB
MEASURED_LOGIT_SQNR_DB = 131.17


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _same_bits(got, want, what=""):
    g, w = _bits(got), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)
    assert g.shape == w.shape, what
    bad = np.argwhere(g != w)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), got.detach().cpu().numpy()[tuple(bad[0])], want[tuple(bad[0])])


def _gemm(c: IC.Case, **kw):
    from data_free_quantization_amd import intmm
    args = dict(a_zero=_dev(c.za), b_zero=_dev(c.zb), bias=_dev(c.bias))
    args.update(kw)
    return intmm.int_gemm(_dev(c.a_bytes), _dev(c.sa), args.pop("a_zero"), _dev(c.b_bytes), _dev(c.sb), args.pop("b_zero"), c.K,
                          b_packed=bool(c.packed), **args)


@pytest.mark.parametrize("spec", IC.all_cases(), ids=IC.case_id)
def test_int_gemm_equals_the_statement_bit_for_bit(spec):
    c = IC.build(*spec)
    _same_bits(_gemm(c), IC.expected(c), IC.case_id(spec))


@pytest.mark.parametrize("spec", [(17, 33, 96, 0, 1, 1, 0), (3, 7, 65, 1, 0, 0, 0), (65, 130, 64, 0, 0, 1, 1)], ids=IC.case_id)
def test_null_zeros_and_bias_skip_their_terms(spec):
    c = IC.build(*spec)
    for za, zb, bias in ((None, c.zb, c.bias), (c.za, None, c.bias), (None, None, None), (c.za, c.zb, None)):
        got = _gemm(c, a_zero=_dev(za), b_zero=_dev(zb), bias=_dev(bias))
        _same_bits(got, IC.statement(c.qa, c.qb, c.sa, za, c.sb, zb, bias), (za is None, zb is None, bias is None))


@pytest.mark.parametrize("spec", [(17, 33, 96, 0, 0, 1, 1), (200, 24, 144, 1, 1, 0, 0), (3, 7, 65, 0, 1, 1, 0)], ids=IC.case_id)
def test_a_row_stride_leaves_the_gap_columns_alone(spec):
    c = IC.build(*spec)
    wide = torch.full((c.M, c.N + 3), -77.0, device=DEV)
    out = _gemm(c, out=wide[:, :c.N])
    assert out.data_ptr() == wide.data_ptr()
    _same_bits(wide[:, :c.N].contiguous(), IC.expected(c))
    assert bool((wide[:, c.N:] == -77.0).all())


def test_same_bits_from_run_to_run_and_at_another_address():
    c = IC.build(65, 130, 64, 0, 1, 1, 0)
    first = _gemm(c)
    pad = torch.empty(4096 + 16, dtype=torch.uint8, device=DEV)   # moves the next allocations
    again = _gemm(c)
    assert torch.equal(first, again) and pad.numel()


# ---- int_linear ------------------------------------------------------------------
def _two_step(x2d, mn, mx, bits, sym, scale_f32, wq, K, bias, b_packed=False):
    """fake_quant of x on the given range (codes, scale, zero), then int_gemm."""
    from data_free_quantization_amd import intmm
    from data_free_quantization_amd.utils.quantize import fake_quant
    r = fake_quant(x2d.contiguous(), bits, symmetric=sym, min_value=mn, max_value=mx, scale_f32=scale_f32)
    out = intmm.int_gemm(r.codes, r.scale, r.zero, wq[0], wq[1], wq[2], K, b_packed=b_packed, bias=bias)
    return out, r


LINEAR_CASES = [  # (M, N, K, bits, symmetric, device range, scale_f32, slice at element 3)
    (17, 33, 96, 8, False, True, False, False), (17, 33, 96, 8, True, False, False, False),
    (17, 33, 96, 4, False, False, True, False), (17, 33, 96, 4, True, True, False, False),
    (5, 40, 65, 8, False, True, False, True), (70, 24, 144, 8, False, False, False, True),
    (3, 7, 40, 2, False, False, False, False), (16, 16, 64, 8, True, True, False, True)]


@pytest.mark.parametrize("M,N,K,bits,sym,dev_range,f32,sliced", LINEAR_CASES)
def test_int_linear_equals_quantize_then_int_gemm(M, N, K, bits, sym, dev_range, f32, sliced):
    """One launch gives the bits of the two-step path, and the activation codes are the
    oracle's.  x holds values outside the range (they clamp), the range's ends and zeros."""
    from data_free_quantization_amd import intmm
    rng = np.random.default_rng(M * 1000 + K + bits)
    mn, mx = (-1.25, 2.5) if not sym else (-1.75, 1.5)
    xw = rng.uniform(mn - 0.5, mx + 0.5, size=(M, K + 7)).astype(np.float32)
    xw[0, 3:6] = (mn, mx, 0.0)
    if M > 1 and not sym:   # quotients at and next to a half-integer: the quantizer's exact-divide path
        step = np.float32((mx - mn) / (2 ** bits - 1))
        ties = (np.float32(mn) + (np.arange(8, dtype=np.float32) % (2 ** bits - 1) + np.float32(0.5)) * step).astype(np.float32)
        xw[1, 3:11], xw[1, 11:19] = ties, np.nextafter(ties, np.float32(np.inf))
    wide = _dev(xw)
    x = wide[:, 3:3 + K] if sliced else wide[:, 3:3 + K].contiguous()
    assert (x.stride(0) > K) == sliced
    c = IC.build(M, N, K, 0, int(sym), 1, 0)   # only B is used
    wq = (_dev(c.b_bytes), _dev(c.sb), _dev(c.zb))
    bias = _dev(c.bias)
    mn32, mx32 = float(np.float32(mn)), float(np.float32(mx))
    kw = dict(min_dev=torch.tensor([mn32], device=DEV), max_dev=torch.tensor([mx32], device=DEV)) if dev_range else \
        dict(min_value=mn, max_value=mx)
    gmn, gmx = (mn32, mx32) if dev_range else (mn, mx)
    intmm.reset_linear_calls()
    got = intmm.int_linear(x, *wq, K, bits=bits, symmetric=sym, scale_f32=f32, bias=bias, **kw)
    assert intmm.LINEAR_CALLS == 1
    want, r = _two_step(x, gmn, gmx, bits, sym, f32, wq, K, bias)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    o = oracle.quantize(x.contiguous().cpu().numpy(), bits, oracle.TENSOR_SYM if sym else oracle.TENSOR_ASYM, rows=1,
                        flags=oracle.F_GIVEN | (oracle.F_F32 if f32 else 0), given=(gmn, gmx))
    assert np.array_equal(r.codes.cpu().numpy(), o["codes"])
    assert r.scale.item() == o["scale"][0] and r.zero.item() == o["zero"][0]
    # and both are the statement on those codes
    _same_bits(got, IC.statement(o["codes"].astype(np.int64), c.qb, o["scale"], o["zero"], c.sb, c.zb, c.bias))


def test_int_linear_with_packed_weights():
    from data_free_quantization_amd import intmm
    c = IC.build(17, 33, 96, 0, 1, 1, 1)
    x = torch.randn(17, 96, device=DEV)
    wq = (_dev(c.b_bytes), _dev(c.sb), _dev(c.zb))
    got = intmm.int_linear(x, *wq, 96, min_value=-2.0, max_value=2.0, b_packed=True, bias=_dev(c.bias))
    want, _ = _two_step(x, -2.0, 2.0, 8, False, False, wq, 96, _dev(c.bias), b_packed=True)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ---- the sweep's own codes ---------------------------------------------------------
@pytest.mark.parametrize("bits,pack", [(8, False), (4, False), (4, True)])
@pytest.mark.parametrize("per_channel", [True, False])
@pytest.mark.parametrize("symmetric", [True, False])
def test_weights_from_the_sweep(bits, pack, per_channel, symmetric):
    """sweep.allocate's codes, scale and zero go into int_gemm as they are."""
    from data_free_quantization_amd import intmm, sweep
    N, K, M = 40, 96, 19
    w = torch.randn(N, K, device=DEV)
    it = sweep.allocate(w, bits=bits, per_channel=per_channel, symmetric=symmetric, pack_int4=pack)
    plan = sweep.SweepPlan([it])
    plan.execute()
    torch.cuda.synchronize()
    codes = it.codes.view(torch.int8) if (pack and symmetric) else it.codes
    a = IC.build(M, N, K, 0, 0, 0, 0)
    got = intmm.int_gemm(_dev(a.a_bytes), _dev(a.sa), _dev(a.za), codes, it.scale, it.zero, K, b_packed=pack)
    raw = it.codes.cpu().numpy()
    if pack:
        b = raw.view(np.uint8).reshape(N, K // 2)
        q = np.stack([b & 0xF, b >> 4], axis=-1).reshape(N, K).astype(np.int64)
        qb = np.where(q >= 8, q - 16, q) if symmetric else q
    else:
        qb = raw.reshape(N, K).astype(np.int64)
    lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if symmetric else (0, (1 << bits) - 1)
    assert qb.min() >= lo and qb.max() <= hi and qb.max() - qb.min() > (hi - lo) // 2
    zero = it.zero.cpu().numpy()
    _same_bits(got, IC.statement(a.qa, qb, a.sa, a.za, it.scale.cpu().numpy(), zero, None))
    # the codes stand for the sweep's dequantized weight
    s = it.scale.cpu().numpy().reshape(-1, 1)
    assert np.array_equal((qb.astype(np.float32) * s + zero.reshape(-1, 1)).astype(np.float32), it.dst.cpu().numpy())
    plan.destroy()


# ---- against the fp32 path -----------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(32, 1000, 1280), (98, 1280, 320)])
def test_against_the_fp32_linear(M, N, K):
    """|int_linear - F.linear(x^, w^, b^)| <= (K + 6) u S + u |b^|, S = sum_k (|x^| + |za|)(|w^| + |zb|),
    u = 2^-24: each dequantized operand is two fp32 roundings from its affine
    value (4 u S to first order), F.linear rounds each product and adds them in fp32 in some
    order (K u), adds the bias (u) and int_linear rounds its fp64 result once (u)."""
    from data_free_quantization_amd import intmm
    from data_free_quantization_amd.utils.quantize import fake_quant
    g = torch.Generator(device="cpu").manual_seed(K)
    x = (torch.randn(M, K, generator=g) * 1.5 + 0.5).to(DEV)
    w = (torch.randn(N, K, generator=g) * 0.05).to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    mn, mx = -2.0, 4.0
    xr = fake_quant(x, 8, min_value=mn, max_value=mx)
    wr = fake_quant(w, 8)
    got = intmm.int_linear(x, wr.codes, wr.scale, wr.zero, K, min_value=mn, max_value=mx, bias=b)
    ref = F.linear(xr.dq, wr.dq, b)
    S = (xr.dq.double().abs() + xr.zero.double().abs()) @ (wr.dq.double().abs() + wr.zero.double().abs()).T
    u = 2.0 ** -24
    bound = (K + 6) * u * S + u * b.double().abs()
    err = (got.double() - ref.double()).abs()
    print("worst |int_linear - F.linear| / bound: %.4f" % float((err / bound).max()))
    assert bool((err <= bound).all())
    # and the fused-quantized input is the fake quant's: feeding x^ instead of x changes nothing
    again = intmm.int_linear(xr.dq, wr.codes, wr.scale, wr.zero, K, min_value=mn, max_value=mx, bias=b)
    assert torch.equal(got, again)


# ---- the forward scope ------------------------------------------------------------------
def _quantized_mobilenetv2(x):
    from data_free_quantization_amd import pipeline, zoo
    from data_free_quantization_amd.utils import layer_transform as L
    from data_free_quantization_amd.utils.quantize import QuantConv2d, QuantLinear
    from data_free_quantization_amd.utils.tracer import TorchTransformer
    model = zoo.build("mobilenetv2", seed=0, relu=True).to(DEV).eval()
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
    return model, graph


def test_quantized_mobilenetv2_in_the_forward_scope():
    """The zoo's MobileNetV2 after --relu --equalize --absorption --quantize, batch 2 at 32 x 32:
    35 layers routed per forward, the others bit for bit what they are outside the scope on the
    same input, two forwards identical, the plain forward's argmax on both images, and the
    logits within the recorded SQNR of the plain forward (less 6 dB: F.conv2d's accumulation
    order differs between library builds, and one flipped downstream activation code costs an
    8-bit step)."""
    from data_free_quantization_amd import intmm
    from data_free_quantization_amd.utils import layer_transform as L
    from data_free_quantization_amd.utils.quantize import QuantConv2d, QuantLinear, frozen_weights, int_matmul_forward
    x = torch.randn(2, 3, 32, 32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    try:
        model, graph = _quantized_mobilenetv2(x)
        layers = [m for m in model.modules() if isinstance(m, (QuantConv2d, QuantLinear))]
        eligible = [m for m in layers if isinstance(m, QuantLinear) or
                    (tuple(m.kernel_size) == (1, 1) and m.groups == 1 and tuple(m.padding) == (0, 0))]
        others = [m for m in layers if m not in eligible]
        assert len(eligible) == 35 and len(others) > 10
        seen = {}
        hooks = [m.register_forward_hook(lambda mod, inp, out: seen.__setitem__(mod, (inp[0].detach().clone(), out.detach().clone())))
                 for m in others]
        L.replace_op()
        try:
            with torch.no_grad():
                plain = model(x)
                with int_matmul_forward():
                    routed = model(x)
                    calls = intmm.LINEAR_CALLS
                    inside = dict(seen)
                    with frozen_weights():
                        again = model(x)
                        cached = model(x)
                    assert intmm.LINEAR_CALLS == 3 * 35
                    assert all(not m._int_routed() for m in others) and all(m._int_routed() for m in eligible)
                for h in hooks:
                    h.remove()
                # a layer outside the eligible set, fed what it was fed inside the scope, gives the same bits outside
                for m, (inp, out) in inside.items():
                    assert torch.equal(m(inp), out)
                assert torch.equal(model(x), plain)   # outside the scope again: the parent's forward
                with pytest.raises(RuntimeError, match="inference path"), int_matmul_forward(), torch.enable_grad():
                    eligible[-1](torch.randn(2, eligible[-1].in_features, device=DEV, requires_grad=True))
        finally:
            L.restore_op()
    finally:
        L.module_tensor_op = None
    assert calls == 35
    assert torch.isfinite(routed).all() and routed.shape == plain.shape
    assert torch.equal(routed, again) and torch.equal(routed, cached)
    assert torch.equal(routed.argmax(1), plain.argmax(1))
    noise = (routed.double() - plain.double()).pow(2).sum()
    sqnr = 10 * np.log10(float(plain.double().pow(2).sum() / noise)) if float(noise) > 0 else float("inf")
    print("MobileNetV2 on the i8 matrix instruction: %d layers routed, logits SQNR %.2f dB against the plain forward" % (calls, sqnr))
    assert MEASURED_LOGIT_SQNR_DB is not None, "record the measured SQNR (printed above)"
    assert sqnr >= MEASURED_LOGIT_SQNR_DB - 6.0


def test_main_dfq_int_matmul_end_to_end(tmp_path, monkeypatch):
    """main_dfq --int_matmul evaluates a synthetic image folder and writes the fields it writes
    without the flag."""
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
    for extra in ([], ["--int_matmul"]):
        (tmp_path / "dfq_result.txt").unlink(missing_ok=True)
        intmm.reset_linear_calls()
        _, _, acc = main_dfq.main(argv + extra)
        assert acc is not None and 0.0 <= acc <= 1.0
        assert intmm.LINEAR_CALLS == (35 if extra else 0)
        text = (tmp_path / "dfq_result.txt").read_text()
        assert "Accuracy: " in text
        fields.append([ln.split(":")[0] for ln in text.splitlines() if ":" in ln])
    assert fields[0] == fields[1]


def test_python_argument_checks_on_the_device():
    from data_free_quantization_amd import intmm
    c = IC.build(17, 33, 96, 0, 0, 1, 0)
    a, sa, za, b, sb, zb = (_dev(v) for v in (c.a_bytes, c.sa, c.za, c.b_bytes, c.sb, c.zb))
    with pytest.raises(ValueError):
        intmm.int_gemm(a, sa, za, b, sb[:5].contiguous(), None, 96)          # neither 1 nor N scales
    with pytest.raises(ValueError):
        intmm.int_gemm(a, sa, za, b, sb, zb[:1].contiguous(), 96)            # zero and scale disagree
    with pytest.raises(ValueError):
        intmm.int_gemm(a, sa, za, b, sb, zb, 95)                             # no whole number of rows
    with pytest.raises(ValueError):
        intmm.int_gemm(a, sa, za, b.view(-1)[1:], sb, zb, 96)                # misaligned (and not whole rows)
    with pytest.raises(TypeError):
        intmm.int_gemm(a.to(torch.int32), sa, za, b, sb, zb, 96)
    with pytest.raises(ValueError):
        intmm.int_gemm(a, sa, za, b, sb, zb, 96, out=torch.empty(17, 32, device=DEV))
    with pytest.raises(ValueError):
        intmm.int_linear(torch.randn(17, 96, device=DEV), b, sb, zb, 96)     # no range
    with pytest.raises(ValueError):
        intmm.int_linear(torch.randn(17, 95, device=DEV), b, sb, zb, 96, min_value=0.0, max_value=1.0)
    with pytest.raises(ValueError):
        intmm.int_gemm(a, sa, za, torch.zeros(33, 47, dtype=torch.uint8, device=DEV), sb, zb, 95, b_packed=True)   # packed, odd K
