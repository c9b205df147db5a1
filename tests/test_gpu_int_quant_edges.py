"""The activation quantizer inside dfq_int_linear, dfq_int_conv2d and dfq_int_dwconv2d
(csrc/dfq_int_quant.h) at its rounding boundaries: tensors of tests/int_quant_edge_cases.py
whose every element lies on or within 3 ulps of a half-integer quotient, on ranges that put 0 on
the grid, off it, outside the range and on a tie.  Every comparison is for equal bits, and the
expectation is the CPU oracle's codes (a true division) put through the float64 statements of
tests/int_gemm_cases.py, int_conv_cases.py and int_dwconv_cases.py -- never the two-step path
alone, whose quantizer shares the screened quotient with these kernels."""
import numpy as np
import pytest
import torch

from tests import int_conv_cases as KC
from tests import int_dwconv_cases as DC
from tests import int_gemm_cases as IC
from tests import int_quant_edge_cases as E
from tests import mx_conv_cases as CC

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(DEV)


def _same_bits(got, want, what=""):
    g = got.detach().cpu().numpy().view(np.uint32)
    w = np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)
    assert g.shape == w.shape, what
    bad = np.argwhere(g != w)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), got.detach().cpu().numpy()[tuple(bad[0])], want[tuple(bad[0])])


def _range_kw(pair, dev):
    return dict(min_dev=torch.tensor([pair[0]], device=DEV), max_dev=torch.tensor([pair[1]], device=DEV)) if dev else \
        dict(min_value=pair[0], max_value=pair[1])


def _wq(w):
    return _dev(w.b_bytes), _dev(w.sb), _dev(w.zb)


# ---- int_linear --------------------------------------------------------------------------------
def _linear(rname, bits, sym, variant, x, w, pair, **kw):
    """intmm.int_linear on x under a variant of E.LIN_VARIANTS; a sliced x is read in place at
    element 3 of a tensor 7 columns wider."""
    from data_free_quantization_amd import intmm
    K, dev, f32, sliced, b_signed = E.LIN_VARIANTS[variant]
    if sliced:
        wide = np.full((x.shape[0], K + 7), np.float32(0.5), np.float32)
        wide[:, 3:3 + K] = x
        xd = _dev(wide)[:, 3:3 + K]
        assert xd.stride(0) == K + 7
    else:
        xd = _dev(x)
    got = intmm.int_linear(xd, *_wq(w), K, bits=bits, symmetric=sym, scale_f32=f32, bias=_dev(E.case_bias(rname, w)),
                           **_range_kw(pair, dev), **kw)
    return got, xd


def _two_step(xd, rname, bits, sym, f32, w, pair, K):
    """The contract's two-step statement: fake_quant of x on the range, then int_gemm of its codes."""
    from data_free_quantization_amd import intmm
    from data_free_quantization_amd.utils.quantize import fake_quant
    r = fake_quant(xd.contiguous(), bits, symmetric=sym, min_value=pair[0], max_value=pair[1], scale_f32=f32)
    return intmm.int_gemm(r.codes, r.scale, r.zero, *_wq(w), K, bias=_dev(E.case_bias(rname, w))), r


@pytest.mark.parametrize("rname,bits,sym,variant", E.LINEAR_CASES,
                         ids=["%s-b%d-%s-%s" % (r, b, "sym" if s else "asym", v) for r, b, s, v in E.LINEAR_CASES])
def test_int_linear_on_rounding_boundaries(rname, bits, sym, variant):
    """M, N = 70, 17 with K = 168 (16-B loads, a 40-element tail) or 166 (4-B loads); ties in every
    row, lane, element slot and K step; a host range, a device range with signed B, and scale_f32
    on a column slice.  The kernel, the two-step path and the statement on the oracle's codes agree
    bit for bit, and the two-step path's codes, scale and zero are the oracle's."""
    from data_free_quantization_amd import intmm
    x, w, pair, K, want = E.linear_case(rname, bits, sym, variant)
    f32 = E.LIN_VARIANTS[variant][2]
    intmm.reset_linear_calls()
    got, xd = _linear(rname, bits, sym, variant, x, w, pair)
    assert intmm.LINEAR_CALLS == 1
    _same_bits(got, want, (rname, bits, sym, variant))
    two, r = _two_step(xd, rname, bits, sym, f32, w, pair, K)
    assert torch.equal(got.view(torch.int32), two.view(torch.int32))
    qa, sa, za = E.oracle_codes(x, pair, bits, sym, f32)
    assert np.array_equal(r.codes.cpu().numpy().astype(np.int64), qa)
    assert r.scale.item() == sa[0] and r.zero.item() == za[0]


# ---- int_conv2d --------------------------------------------------------------------------------
def _conv(gname, rname, bits, sym, x, w, pair, **kw):
    from data_free_quantization_amd import intmm
    g = E.CONV_GEOMS[gname]
    dev, f32, b_signed = E.CONV_VARIANTS[bits]
    return intmm.int_conv2d(_dev(x), *_wq(w), g.kernel, g.stride, g.padding, g.dilation, bits=bits, symmetric=sym, scale_f32=f32,
                            bias=_dev(E.case_bias(rname, w)), **_range_kw(pair, dev), **kw)


@pytest.mark.parametrize("rname", list(E.RANGES))
@pytest.mark.parametrize("gname", list(E.CONV_GEOMS))
def test_int_conv2d_on_rounding_boundaries(gname, rname):
    """A 3 x 3 layer without padding, one with padding on all four borders (K = 144, M = 162:
    three row blocks and a K tail), a stride-2 and a dilated geometry; bits 8 (device range), 4
    (scale_f32) and 2, both grids.  Each x element feeds up to nine (m, k) slots, so the ties reach
    every lane and element position.  On (-1.5, 253.5) at 8 bits every padding tap and tail column
    is a 0.0 on the tie 1.5 -- it takes the exact divide before it is masked -- and the result is not
    the code-of-zero rule's."""
    for bits in E.CONV_VARIANTS:
        for sym in (False, True):
            x, w, pair, want = E.conv_case(gname, rname, bits, sym)
            got = _conv(gname, rname, bits, sym, x, w, pair)
            _same_bits(got, want, (gname, rname, bits, sym))
            if rname == "zero_tie" and bits == 8 and not sym and E.CONV_GEOMS[gname].padding != (0, 0):
                coded = E.conv_case(gname, rname, bits, sym, x=x, code_of_zero=True)[3]
                assert not np.array_equal(got.cpu().numpy().view(np.uint32), coded.view(np.uint32))


# ---- int_dwconv2d ------------------------------------------------------------------------------
def _dwconv(gname, rname, bits, sym, x, w, pair, **kw):
    from data_free_quantization_amd import intmm
    g = DC.GEOMS[gname]
    dev, f32, b_signed = E.DW_VARIANTS[bits]
    return intmm.int_dwconv2d(_dev(x), *_wq(w), g.kernel, g.stride, g.padding, g.dilation, bits=bits, symmetric=sym, scale_f32=f32,
                              bias=_dev(E.case_bias(rname, w)), **_range_kw(pair, dev), **kw)


@pytest.mark.parametrize("rname", list(E.RANGES))
@pytest.mark.parametrize("gname", E.DW_GEOMS)
def test_int_dwconv2d_on_rounding_boundaries(gname, rname):
    """Eight geometries of tests/int_dwconv_cases.py -- ``one_pixel`` with more planes than lanes and
    several planes per workgroup, ``wide`` with several tiles each way, halo cells quantized by two
    workgroups and a cell count that is no multiple of 256 -- at bits 8 (device range) and 4
    (scale_f32), both grids."""
    for bits in E.DW_VARIANTS:
        for sym in (False, True):
            x, w, pair, want = E.dw_case(gname, rname, bits, sym)
            _same_bits(_dwconv(gname, rname, bits, sym, x, w, pair), want, (gname, rname, bits, sym))


@pytest.mark.parametrize("gname", ["mnv2_s1", "mult2"])
@pytest.mark.parametrize("rname", ["asym", "zero_tie"])
def test_each_channel_is_int_conv2d_on_that_channel_on_boundary_data(gname, rname):
    """tests/test_gpu_int_dwconv.py's cross-check on the device, on the tie-dense data."""
    from data_free_quantization_amd import intmm
    g = DC.GEOMS[gname]
    bits, sym = 8, False
    dev, f32, b_signed = E.DW_VARIANTS[bits]
    x, w, pair, want = E.dw_case(gname, rname, bits, sym)
    got = _dwconv(gname, rname, bits, sym, x, w, pair)
    xd, codes, sb, zb, bias = _dev(x), _dev(w.b_bytes).view(DC.N(g), DC.K(g)), _dev(w.sb), _dev(w.zb), _dev(w.bias)
    for c in range(g.C):
        rows = slice(c * g.mult, (c + 1) * g.mult)
        one = intmm.int_conv2d(xd[:, c:c + 1].contiguous(), codes[rows].clone(), sb[rows].clone(), zb[rows].clone(), g.kernel,
                               g.stride, g.padding, g.dilation, bits=bits, symmetric=sym, scale_f32=f32, bias=bias[rows].clone(),
                               **_range_kw(pair, dev))
        assert torch.equal(got[:, rows].contiguous().view(torch.int32), one.view(torch.int32)), (gname, rname, c)
    _same_bits(got, want)


# ---- one near-tie ------------------------------------------------------------------------------
LIN_K = 168
#: (row, k): the first and last row; k = 0, 15, 16 and 63 of the first K step, the first element of
#: the second, the last valid k of the tail and the one before it
LINEAR_TIE_POSITIONS = [(0, 0), (0, 15), (0, 16), (0, 63), (0, 64), (0, LIN_K - 1), (0, LIN_K - 2), (69, 0), (69, 15), (69, 63),
                        (69, 64), (69, LIN_K - 1), (37, 100)]


@pytest.mark.parametrize("rname,bits,sym", E.SINGLE_TIE_RANGES, ids=[r for r, _, _ in E.SINGLE_TIE_RANGES])
@pytest.mark.parametrize("row,k", LINEAR_TIE_POSITIONS)
def test_int_linear_with_one_near_tie(row, k, rname, bits, sym):
    """Data at least 0.2 of a step from every half-integer and one near-tie the reciprocal quotient
    rounds to the wrong code: only one lane of one wave raises the ballot."""
    pos = row * LIN_K + k
    x = E.single_tie_x((E.LIN_M, LIN_K), E.RANGES[rname], bits, sym, pos)
    x, w, pair, K, want = E.linear_case(rname, bits, sym, "host", x=x)
    got, _ = _linear(rname, bits, sym, "host", x, w, pair)
    _same_bits(got, want, (row, k))


def _conv_tie_positions(g):
    last = (g.B - 1, g.C - 1)
    return [(0, 0, 0, 0), (0, 0, 0, g.W - 1), (0, 0, g.H - 1, 0), (0, 0, g.H - 1, g.W - 1), (*last, 0, 0), (*last, 0, g.W - 1),
            (*last, g.H - 1, 0), (*last, g.H - 1, g.W - 1), (0, g.C // 2, g.H // 2, g.W // 2), (*last, g.H // 2, g.W // 2 + 1)]


@pytest.mark.parametrize("rname,bits,sym", E.SINGLE_TIE_RANGES, ids=[r for r, _, _ in E.SINGLE_TIE_RANGES])
@pytest.mark.parametrize("where", range(10))
def test_int_conv2d_with_one_near_tie(where, rname, bits, sym):
    """The padded 3 x 3 layer: the image's four corners (a tap next to padding) in the first and
    the last (image, channel) plane, and interior pixels."""
    g = E.CONV_GEOMS["pad1"]
    pos = int(np.ravel_multi_index(_conv_tie_positions(g)[where], (g.B, g.C, g.H, g.W)))
    x = E.single_tie_x((g.B, g.C, g.H, g.W), E.case_range(rname, E.CONV_VARIANTS[bits][0]), bits, sym, pos)
    x, w, pair, want = E.conv_case("pad1", rname, bits, sym, x=x)
    _same_bits(_conv("pad1", rname, bits, sym, x, w, pair), want, where)


def _dw_tie_positions():
    wide, one, s1 = DC.GEOMS["wide"], DC.GEOMS["one_pixel"], DC.GEOMS["mnv2_s1"]
    return [("wide", (0, 0, 0, 0)), ("wide", (0, wide.C - 1, wide.H - 1, wide.W - 1)),          # the footprint's first and last cell
            ("wide", (0, 0, 15, 31)), ("wide", (0, 0, 16, 32)), ("wide", (0, 1, 31, 63)), ("wide", (0, 1, 32, 64)),   # around tile edges: halo cells
            ("wide", (0, 0, 16, 0)), ("wide", (0, 1, 0, 32)),
            ("one_pixel", (one.B - 1, one.C - 1, one.H - 1, one.W - 1)), ("one_pixel", (0, 0, 0, 0)), ("one_pixel", (1, 64, 1, 1)),
            ("mnv2_s1", (s1.B - 1, s1.C - 1, s1.H - 1, s1.W - 1)), ("mnv2_s1", (0, 0, 0, 0))]


@pytest.mark.parametrize("rname,bits,sym", E.SINGLE_TIE_RANGES, ids=[r for r, _, _ in E.SINGLE_TIE_RANGES])
@pytest.mark.parametrize("gname,at", _dw_tie_positions(), ids=["%s-%s" % (n, "_".join(map(str, a))) for n, a in _dw_tie_positions()])
def test_int_dwconv2d_with_one_near_tie(gname, at, rname, bits, sym):
    """The footprint's first and last cell, cells on both sides of every tile edge of ``wide`` (halo
    cells, whatever the tile size), and the last pixel of the last plane of ``one_pixel``."""
    g = DC.GEOMS[gname]
    pos = int(np.ravel_multi_index(at, (g.B, g.C, g.H, g.W)))
    x = E.single_tie_x((g.B, g.C, g.H, g.W), E.case_range(rname, E.DW_VARIANTS[bits][0]), bits, sym, pos)
    x, w, pair, want = E.dw_case(gname, rname, bits, sym, x=x)
    _same_bits(_dwconv(gname, rname, bits, sym, x, w, pair), want, (gname, at))


# ---- special values ----------------------------------------------------------------------------
SPECIAL_CASES = [("relu6", 8, False), ("zero_tie", 8, False), ("asym", 4, False), ("sym", 8, True), ("below0", 2, True)]


@pytest.mark.parametrize("rname,bits,sym", SPECIAL_CASES, ids=["%s-b%d" % (r, b) for r, b, _ in SPECIAL_CASES])
def test_signed_zeros_subnormals_flt_max_and_infinities(rname, bits, sym):
    """About 2 % of the boundary data replaced by -0.0, +0.0, +-1e-40, +-FLT_MAX and +-inf, all of
    which the oracle defines (an infinity clamps to an end); the signed zeros matter on (0, 6) and
    (-1.5, 253.5).  All three kernels."""
    for variant in ("host", "dev"):
        K, dev, f32, _, _ = E.LIN_VARIANTS[variant]
        x = E.with_specials(E.boundary_x((E.LIN_M, K), E.case_range(rname, dev), bits, sym, f32))
        x, w, pair, K, want = E.linear_case(rname, bits, sym, variant, x=x)
        assert np.isfinite(want).all()
        got, xd = _linear(rname, bits, sym, variant, x, w, pair)
        _same_bits(got, want, (rname, variant))
        two, _ = _two_step(xd, rname, bits, sym, f32, w, pair, K)
        assert torch.equal(got.view(torch.int32), two.view(torch.int32))
    g = E.CONV_GEOMS["pad1"]
    if bits in E.CONV_VARIANTS:
        x = E.with_specials(E.boundary_x((g.B, g.C, g.H, g.W), E.case_range(rname, E.CONV_VARIANTS[bits][0]), bits, sym, E.CONV_VARIANTS[bits][1]))
        x, w, pair, want = E.conv_case("pad1", rname, bits, sym, x=x)
        _same_bits(_conv("pad1", rname, bits, sym, x, w, pair), want, (rname, "conv"))
    if bits in E.DW_VARIANTS:
        for gname in ("mnv2_s1", "wide"):
            g = DC.GEOMS[gname]
            x = E.with_specials(E.boundary_x((g.B, g.C, g.H, g.W), E.case_range(rname, E.DW_VARIANTS[bits][0]), bits, sym, E.DW_VARIANTS[bits][1]))
            x, w, pair, want = E.dw_case(gname, rname, bits, sym, x=x)
            _same_bits(_dwconv(gname, rname, bits, sym, x, w, pair), want, (rname, gname))


@pytest.mark.parametrize("rname,sym", [("asym", False), ("above0", False), ("sym", True)])
def test_nan_takes_the_code_of_qmin_by_this_projects_own_rule(rname, sym):
    """NOT the reference's behaviour (its cast of NaN is undefined, and the oracle is never given
    one): csrc/dfq_common.h clamps with fminf(fmaxf(t, qmin), qmax), which maps NaN to qmin, and
    the integer kernels inherit that.  The output is finite, equal to the statement with qmin's code
    at the NaN positions, and equal to the two-step path."""
    bits = 8
    x = E.boundary_x((E.LIN_M, LIN_K), E.RANGES[rname], bits, sym)
    x[[0, 0, 33, 69, 69], [0, 63, 100, 64, LIN_K - 1]] = np.float32(np.nan)
    w = IC.build(E.LIN_M, E.LIN_N, LIN_K, 0, 0, 1, 0)
    pair = E.RANGES[rname]
    qa, sa, za = E.nan_expected_codes(x, pair, bits, sym)
    want = IC.statement(qa, w.qb, sa, za, w.sb, w.zb, w.bias)
    got, xd = _linear(rname, bits, sym, "host", x, w, pair)
    assert bool(torch.isfinite(got).all())
    _same_bits(got, want, rname)
    two, r = _two_step(xd, rname, bits, sym, False, w, pair, LIN_K)
    assert np.array_equal(r.codes.cpu().numpy().astype(np.int64), qa)
    assert torch.equal(got.view(torch.int32), two.view(torch.int32))
    g = E.CONV_GEOMS["pad1"]
    xc = E.boundary_x((g.B, g.C, g.H, g.W), E.case_range(rname, True), bits, sym)
    xc[0, 0, 0, 0] = xc[1, 15, 8, 8] = xc[0, 7, 4, 4] = np.float32(np.nan)
    wc = KC.weights(g, 0, 1, 0)
    pairc = E.case_range(rname, True)
    qc, sc, zc = E.nan_expected_codes(KC.unfold(np.where(np.isnan(xc), np.float32(-np.inf), xc), g), pairc, bits, sym)
    wantc = KC.nchw(KC.statement(qc, KC.taps(g), wc.qb, sc, zc, wc.sb, wc.zb, wc.bias), g)
    gotc = _conv("pad1", rname, bits, sym, xc, wc, pairc)
    assert bool(torch.isfinite(gotc).all())
    _same_bits(gotc, wantc, (rname, "conv"))
    gd = DC.GEOMS["mnv2_s1"]
    xdw = E.boundary_x((gd.B, gd.C, gd.H, gd.W), pairc, bits, sym)
    nan_at = [(0, 0, 0, 0), (1, 4, 6, 6), (0, 2, 3, 3)]
    for at in nan_at:
        xdw[at] = np.float32(np.nan)
    wd = DC.weights(gd, 0, 1, 0)
    wantd = DC.statement(np.where(np.isnan(xdw), np.float32(-np.inf), xdw), gd, wd, pairc, bits, sym, False)
    gotd = _dwconv("mnv2_s1", rname, bits, sym, xdw, wd, pairc)
    assert bool(torch.isfinite(gotd).all())
    _same_bits(gotd, wantd, (rname, "dwconv"))


# ---- reproducibility and guard words -------------------------------------------------------------
def test_same_bits_twice_and_the_guard_words_stay_untouched():
    """Each kernel twice on boundary data, into an output view at a 4-B-aligned offset with guard
    words on both sides."""
    x, w, pair, K, want = E.linear_case("asym", 8, False, "dev")
    buf = torch.full((want.size + 64,), -7.25, device=DEV)
    out = buf[31:31 + want.size].view(want.shape)
    first = _linear("asym", 8, False, "dev", x, w, pair)[0].clone()
    got, _ = _linear("asym", 8, False, "dev", x, w, pair, out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(first.view(torch.int32), out.view(torch.int32))
    _same_bits(out, want)
    assert bool((buf[:31] == -7.25).all()) and bool((buf[31 + want.size:] == -7.25).all())
    for call, case, name in ((_conv, E.conv_case, "pad1"), (_dwconv, E.dw_case, "wide"), (_dwconv, E.dw_case, "one_pixel")):
        x, w, pair, want = case(name, "zero_tie", 8, False)
        buf = torch.full((want.size + 64,), -7.25, device=DEV)
        out = buf[31:31 + want.size].view(want.shape)   # 4-B aligned only: the 16-B stores are not 16-B aligned
        first = call(name, "zero_tie", 8, False, x, w, pair).clone()
        got = call(name, "zero_tie", 8, False, x, w, pair, out=out)
        assert got.data_ptr() == out.data_ptr() and torch.equal(first.view(torch.int32), out.view(torch.int32)), name
        _same_bits(out, want, name)
        assert bool((buf[:31] == -7.25).all()) and bool((buf[31 + want.size:] == -7.25).all()), name


# ---- a scale whose reciprocal is a subnormal float -------------------------------------------------
#: 8-bit symmetric given ranges: s = max / 127 above 2^126 (1 / s subnormal), and the controls just
#: below it -- the second the range of DESIGN.md 3.9's note
HUGE_RANGES = [(-2.2e40, 2.2e40), (-1.08e40, 1.08e40), (-1e40, 1e40)]


def _tiny_b(w):
    """B's scale and zero times 2^-24 (exact): the products with s near 1e38 stay finite floats."""
    return _dev(w.b_bytes), _dev(w.sb * np.float32(2.0 ** -24)), _dev(w.zb * np.float32(2.0 ** -24))


@pytest.mark.parametrize("pair", HUGE_RANGES, ids=["%.3g" % p[1] for p in HUGE_RANGES])
def test_int_kernels_on_a_scale_whose_reciprocal_is_subnormal(pair):
    """Finite tie-dense rows (every |x| <= FLT_MAX) on a range whose scale lies above 2^126, where
    1 / s is a subnormal float the reciprocal instruction may flush to zero, and on the controls
    below it: dfq_int_linear and dfq_int_dwconv2d against the oracle's codes through the
    statements, the two-step path's codes, scale and zero against the oracle's."""
    from data_free_quantization_amd import intmm
    from data_free_quantization_amd.utils.quantize import fake_quant
    bits, sym = 8, True
    s, zero = E.qparams(pair, bits, sym)
    assert (float(s) > E.TWO_126) == (pair[1] > 2e40) and 0.9 * E.TWO_126 < float(s)
    x = E.boundary_x((E.LIN_M, LIN_K), pair, bits, sym)
    assert np.isfinite(x).all()
    w = IC.build(E.LIN_M, E.LIN_N, LIN_K, 0, 1, 1, 0)
    qa, sa, za = E.oracle_codes(x, pair, bits, sym)
    assert len(np.unique(qa)) >= 4
    want = IC.statement(qa, w.qb, sa, za, w.sb * np.float32(2.0 ** -24), w.zb * np.float32(2.0 ** -24), None)
    assert np.isfinite(want).all() and np.abs(want).max() > 1e30
    xd = _dev(x)
    got = intmm.int_linear(xd, *_tiny_b(w), LIN_K, bits=bits, symmetric=sym, min_value=pair[0], max_value=pair[1])
    _same_bits(got, want, pair)
    r = fake_quant(xd, bits, symmetric=sym, min_value=pair[0], max_value=pair[1])
    assert np.array_equal(r.codes.cpu().numpy().astype(np.int64), qa)
    assert r.scale.item() == sa[0] and r.zero.item() == za[0]
    g = DC.GEOMS["mnv2_s1"]
    xw = E.boundary_x((g.B, g.C, g.H, g.W), pair, bits, sym)
    wd = DC.weights(g, 1, 1, 0)
    wd.sb, wd.zb = wd.sb * np.float32(2.0 ** -24), wd.zb * np.float32(2.0 ** -24)
    wantd = DC.statement(xw, g, wd, pair, bits, sym, False, bias=False)
    assert np.isfinite(wantd).all()
    gotd = intmm.int_dwconv2d(_dev(xw), _dev(wd.b_bytes), _dev(wd.sb), _dev(wd.zb), g.kernel, g.stride, g.padding, g.dilation,
                              bits=bits, symmetric=sym, min_value=pair[0], max_value=pair[1])
    _same_bits(gotd, wantd, (pair, "dwconv"))
