"""Group-wise B parameters on the GPU (intmm.int_gemm / int_linear / int_conv2d with b_group,
intmm.group_quant, quantize_targ_layer(granularity="group")): every result bit
for bit the float64 statement of tests/int_group_cases.py."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import oracle
from tests import int_conv_cases as KC
from tests import int_gemm_cases as IC
from tests import int_group_cases as GC
from tests import mx_conv_cases as CC

pytestmark = pytest.mark.gpu
DEV = "cuda"
M, N = 33, 35   # cross the 32 x 32 wave tile on both sides


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same_bits(got, want, what=""):
    g, w = got.detach().cpu().numpy().view(np.uint32), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)
    assert g.shape == w.shape, what
    bad = np.argwhere(g != w)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), got.detach().cpu().numpy()[tuple(bad[0])], want[tuple(bad[0])])


def _gemm(c, sb, zb, za, bias, g):
    from data_free_quantization_amd import intmm
    return intmm.int_gemm(_dev(c.a_bytes), _dev(c.sa), _dev(za), _dev(c.b_bytes), _dev(sb), _dev(zb), c.K,
                          b_packed=bool(c.packed), bias=_dev(bias), b_group=g)


@pytest.mark.parametrize("a_signed,b_signed", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("K,g,packed", [(K, g, 0) for K, g in GC.GEMM_KG] + [(256, 32, 1), (200, 64, 1)])
def test_int_gemm_grouped_equals_the_statement(K, g, packed, a_signed, b_signed):
    c = IC.build(M, N, K, a_signed, b_signed, 1, packed)
    sb, zb = GC.group_params(N, K, g)
    for za, z, bias in ((c.za, zb, c.bias), (None, zb, c.bias), (c.za, None, None), (None, None, None)):
        _same_bits(_gemm(c, sb, z, za, bias, g), GC.statement(c.qa, c.qb, c.sa, za, sb, z, bias, g),
                   (za is None, z is None, bias is None))


@pytest.mark.parametrize("K,g", [(40, 64), (64, 64), (96, 128)])
def test_one_group_gives_the_per_row_bits(K, g):
    from data_free_quantization_amd import intmm
    c = IC.build(M, N, K, 0, 1, 1, 0)
    args = (_dev(c.a_bytes), _dev(c.sa), _dev(c.za), _dev(c.b_bytes))
    per_row = intmm.int_gemm(*args, _dev(c.sb), _dev(c.zb), K, bias=_dev(c.bias))
    grouped = intmm.int_gemm(*args, _dev(c.sb.reshape(N, 1)), _dev(c.zb.reshape(N, 1)), K, bias=_dev(c.bias), b_group=g)
    assert torch.equal(per_row.view(torch.int32), grouped.view(torch.int32))
    # all-zero codes under a negative scale: (sa sb) * 0 = -0.0 is assigned, not added to 0.0
    zeros, neg = torch.zeros(M, K, dtype=torch.int8, device=DEV), _dev(-c.sb)
    per_row = intmm.int_gemm(zeros, args[1], None, args[3], neg, None, K)
    grouped = intmm.int_gemm(zeros, args[1], None, args[3], neg.reshape(N, 1), None, K, b_group=g)
    assert bool((per_row.view(torch.int32) == -2 ** 31).all()) and torch.equal(per_row.view(torch.int32), grouped.view(torch.int32))


@pytest.mark.parametrize("bits,sym,dev_range", [(8, False, True), (4, True, False)])
@pytest.mark.parametrize("K,g", [(168, 32), (168, 64), (166, 64)])
def test_int_linear_grouped(K, g, bits, sym, dev_range):
    """x [70, K]: K = 168 on the 16-B loads with a ragged tail, K = 166 on the 4-B loads; the
    activation codes are the oracle's on the given range."""
    from data_free_quantization_amd import intmm
    Ml, Nl = 70, 17
    mn, mx = (-1.75, 1.5) if sym else (float(np.float32(-1.25)), 2.5)
    x = np.random.default_rng(K + g + bits).uniform(mn - 0.5, mx + 0.5, size=(Ml, K)).astype(np.float32)
    c = IC.build(2, Nl, K, 0, int(sym), 1, 0)   # only B is used
    sb, zb = GC.group_params(Nl, K, g)
    kw = dict(min_dev=torch.tensor([mn], device=DEV), max_dev=torch.tensor([mx], device=DEV)) if dev_range else \
        dict(min_value=mn, max_value=mx)
    got = intmm.int_linear(_dev(x), _dev(c.b_bytes), _dev(sb), _dev(zb), K, bits=bits, symmetric=sym, bias=_dev(c.bias),
                           b_group=g, **kw)
    o = oracle.quantize(x, bits, oracle.TENSOR_SYM if sym else oracle.TENSOR_ASYM, rows=1, flags=oracle.F_GIVEN, given=(mn, mx))
    _same_bits(got, GC.statement(o["codes"].astype(np.int64), c.qb, o["scale"], o["zero"], sb, zb, c.bias, g))


CONV = {"pad1": CC._g(2, 8, 6, 6, 9, 3, 1, 1, 1), "nopad": CC._g(2, 8, 6, 6, 9, 3, 1, 0, 1),
        "stride2": CC._g(2, 8, 6, 6, 9, 3, 2, 1, 1), "dil2": CC._g(2, 8, 6, 6, 9, 3, 1, 0, 2),
        "pointwise": CC._g(2, 96, 6, 6, 9, 1, 1, 0, 1), "n33": CC._g(2, 8, 6, 6, 33, 3, 1, 1, 1)}


@pytest.mark.parametrize("name,g", [("pad1", 32), ("pad1", 64), ("nopad", 32), ("nopad", 64), ("stride2", 32), ("stride2", 64),
                                    ("dil2", 32), ("dil2", 64), ("pointwise", 32), ("n33", 32)])
def test_int_conv2d_grouped(name, g):
    """K = 72 (pointwise: 96): the groups cut through channels and taps; with padding T_j
    differs by row and by group.  8-bit asymmetric x on (-1.3, 2.5), where 0 is off the grid."""
    from data_free_quantization_amd import intmm
    geo = CONV[name]
    K = CC.K(geo)
    x = KC.make_x(geo, KC.ASYM_RANGE, 8, False)
    w = KC.weights(geo, 0, 1, 0)
    sb, zb = GC.group_params(geo.N, K, g)
    qa, sa, za = KC.quantized(x, geo, KC.ASYM_RANGE, 8, False)
    v = KC.taps(geo)
    if name in ("pad1", "n33"):   # T_j differs by row and by group
        tj = np.stack([v[:, j * g:(j + 1) * g].sum(axis=1) for j in range(-(-K // g))])
        assert len({tuple(r) for r in tj.T}) > 1 and len({tuple(r) for r in tj}) > 1
    for z, bias in ((zb, w.bias), (None, None)):
        got = intmm.int_conv2d_grouped(_dev(x), _dev(w.b_bytes), _dev(sb), _dev(z), geo.kernel, geo.stride, geo.padding, geo.dilation,
                               min_value=KC.ASYM_RANGE[0], max_value=KC.ASYM_RANGE[1], bias=_dev(bias), b_group=g)
        _same_bits(got, KC.nchw(GC.statement(qa, w.qb, sa, za, sb, z, bias, g, v=v), geo), (name, g, z is None))


def test_a_wrong_parameter_count_raises():
    from data_free_quantization_amd import intmm
    c = IC.build(M, N, 200, 0, 0, 1, 0)
    sb, zb = GC.group_params(N, 200, 64)   # [N, 4]
    with pytest.raises(ValueError, match="values"):
        _gemm(c, sb[:, :3], None, None, None, 64)     # the short last group has its own scale
    with pytest.raises(ValueError, match="values"):
        _gemm(c, sb, zb[:, :1], None, None, 64)
    with pytest.raises(ValueError, match="values"):
        intmm.int_gemm(_dev(c.a_bytes), _dev(c.sa), None, _dev(c.b_bytes), _dev(c.sb), None, 200, b_group=64)   # per-row count


@pytest.mark.parametrize("shape,g", [((24, 96), 32), ((24, 96), 64), ((16, 8, 3, 3), 32), ((16, 8, 3, 3), 64)])
@pytest.mark.parametrize("bits,sym", [(4, False), (8, True)])
def test_group_quant_and_the_pipeline_entry(shape, g, bits, sym):
    """group_quant and quantize_targ_layer(granularity="group") give fake_quant's per-channel
    result on the [N K / g, g] view; a layer whose K is no multiple of g (the convolution's 72
    at g = 32 and 64) falls back to per channel in the pipeline and is body + tail in
    group_quant; int_gemm(b_group=g) on the codes is the statement."""
    from data_free_quantization_amd import intmm
    from data_free_quantization_amd.utils.layer_transform import quantize_targ_layer
    from data_free_quantization_amd.utils.quantize import fake_quant
    w = torch.randn(*shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(sum(shape) + g))
    Nw, K = shape[0], int(np.prod(shape[1:]))
    w2d = w.reshape(Nw, K)
    codes, scale, zero = intmm.group_quant(w2d, bits, g, symmetric=sym)
    body = K - K % g
    rb = fake_quant(w2d[:, :body].contiguous().reshape(-1, g), bits, per_channel=True, symmetric=sym)
    want_codes, want_scale, want_zero, want_dq = (rb.codes.reshape(Nw, -1), rb.scale.reshape(Nw, -1), rb.zero.reshape(Nw, -1),
                                                  rb.dq.reshape(Nw, -1))
    if K > body:
        rt = fake_quant(w2d[:, body:].contiguous(), bits, per_channel=True, symmetric=sym)
        want_codes, want_dq = torch.cat([want_codes, rt.codes], 1), torch.cat([want_dq, rt.dq], 1)
        want_scale, want_zero = torch.cat([want_scale, rt.scale[:, None]], 1), torch.cat([want_zero, rt.zero[:, None]], 1)
    assert scale.shape == (Nw, -(-K // g)) and torch.equal(codes, want_codes)
    assert torch.equal(scale, want_scale) and torch.equal(zero, want_zero)
    a = IC.build(M, Nw, K, 0, 0, 0, 0)
    got = intmm.int_gemm(_dev(a.a_bytes), _dev(a.sa), _dev(a.za), codes, scale, zero, K, b_group=g)
    _same_bits(got, GC.statement(a.qa, codes.cpu().numpy().astype(np.int64), a.sa, a.za, scale.cpu().numpy(), zero.cpu().numpy(),
                                 None, g))
    # the pipeline entry on one layer
    layer = nn.Linear(K, Nw, bias=False) if len(shape) == 2 else nn.Conv2d(shape[1], Nw, shape[2], bias=False)
    layer = layer.to(DEV)
    with torch.no_grad():
        layer.weight.copy_(w)
    state = {}
    quantize_targ_layer({0: layer}, bits, 32, (type(layer),), granularity="group", group_size=g, symmetric=sym, state=state)
    torch.cuda.synchronize()
    if K % g == 0:
        assert state[0]["group_size"] == g and state[0]["scale"].shape == (Nw, K // g)
        assert torch.equal(state[0]["codes"].reshape(Nw, K), want_codes) and torch.equal(layer.weight.detach().reshape(Nw, K), want_dq)
        assert torch.equal(state[0]["scale"], want_scale) and torch.equal(state[0]["zero"], want_zero)
    else:   # the fallback rule: per channel
        rc = fake_quant(w2d.contiguous(), bits, per_channel=True, symmetric=sym)
        assert state[0]["group_size"] is None and state[0]["scale"].shape == (Nw,)
        assert torch.equal(state[0]["codes"].reshape(Nw, K), rc.codes) and torch.equal(layer.weight.detach().reshape(Nw, K), rc.dq)
