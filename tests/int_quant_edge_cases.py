"""Activations that sit on the rounding boundaries of the quantizer the one-launch integer kernels
share (csrc/dfq_int_quant.h: dfq_int_linear, dfq_int_conv2d, dfq_int_dwconv2d), in numpy and the
CPU oracle only (tests/test_int_quant_edges_host.py imports this module on the CPU,
tests/test_gpu_int_quant_edges.py runs the cases).

The quantizer takes the reciprocal quotient a = (x + negmn) * rcp(s) and the IEEE divide only
where a lane of the wave lies within |t| 2^-20 of a half-integer (qdq_screen, csrc/dfq_common.h).
``boundary_x`` fills a whole tensor with such values -- every half-integer from one below qmin to
one above qmax, moved by -3 .. +3 fp32 ulps -- on a given range; ``single_tie_x`` holds one such
value among data far from every boundary.  ``emulate`` is that quantizer in numpy, with the exact
path switchable.  At import the module checks that the inputs discriminate (``_self_check``): the
values are finite, at least 40 % of them raise the screen, the codes cover the grid, the quantizer
without its exact path gets codes wrong and with it gets none wrong, and one activation code
changed by one changes the bits of the expected output of all three statements."""
import functools
import zlib

import numpy as np

from oracle import oracle
from tests import int_conv_cases as KC
from tests import int_dwconv_cases as DC
from tests import int_gemm_cases as IC
from tests import mx_conv_cases as CC

#: name -> (min, max)
RANGES = {
    "asym": (-1.3, 2.5),          # 0 off the 8-bit grid
    "relu6": (0.0, 6.0),          # min == 0 exactly
    "above0": (0.75, 5.5),        # 0 below the range: a dummy zero clamps to qmin
    "below0": (-4.0, -0.5),       # 0 above the range
    "sym": (-1.75, 1.5),
    "degenerate": (0.0, 0.0),     # s is the 1e-8 floor
    "zero_tie": (-1.5, 253.5),    # 8-bit asymmetric: s == 1 and 0.0 itself sits on the tie 1.5
}
BITS = tuple(range(2, 9))
FLT_MAX = float(np.finfo(np.float32).max)
TWO_126 = 2.0 ** 126   # above it 1 / s is a subnormal float
F32 = np.float32


def mode_of(sym):
    return oracle.TENSOR_SYM if sym else oracle.TENSOR_ASYM


def grid(bits, sym):
    """(qmin, qmax)"""
    return (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if sym else (0, (1 << bits) - 1)


def qparams(rng_pair, bits, sym, f32=False):
    """(s, zero) of the given range as the oracle builds them: float32 scalars."""
    o = oracle.quantize(np.zeros((1, 1), F32), bits, mode_of(sym), rows=1, flags=oracle.F_GIVEN | (oracle.F_F32 if f32 else 0),
                        given=rng_pair)
    return o["scale"][0], o["zero"][0]


def device_pair(rng_pair):
    """The range as a device range holds it: the bounds rounded to fp32."""
    return tuple(float(F32(t)) for t in rng_pair)


def oracle_codes(x, rng_pair, bits, sym, f32=False):
    """(codes int64 of x's shape, scale [1], zero [1]) of the oracle's given-range quantizer."""
    o = oracle.quantize(np.ascontiguousarray(x, dtype=F32).reshape(1, -1), bits, mode_of(sym), rows=1,
                        flags=oracle.F_GIVEN | (oracle.F_F32 if f32 else 0), given=rng_pair)
    return o["codes"].astype(np.int64).reshape(np.shape(x)), o["scale"], o["zero"]


def ulp_step(v, steps):
    """v moved by ``steps`` fp32 ulps along the float order (through zero into the subnormals)."""
    i = np.ascontiguousarray(v, dtype=F32).view(np.int32).astype(np.int64)
    o = np.where(i < 0, -(i & 0x7FFFFFFF), i) + np.asarray(steps, dtype=np.int64)
    return np.where(o < 0, (-o) | 0x80000000, o).astype(np.uint32).view(F32)


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def boundary_x(shape, rng_pair, bits, sym, f32=False, seed=0):
    """x of ``shape``: every element fl32((k + 0.5) s + zero) moved by -3 .. +3 ulps, k uniform over
    those of [qmin - 1, qmax] whose value is a finite float (all of them unless s is huge)."""
    s, zero = qparams(rng_pair, bits, sym, f32)
    qmin, qmax = grid(bits, sym)
    rng = np.random.default_rng(_seed("boundary", tuple(shape), rng_pair, bits, sym, f32, seed))
    ks = np.arange(qmin - 1, qmax + 1, dtype=np.float64)
    ks = ks[np.abs((ks + 0.5) * np.float64(s) + np.float64(zero)) <= FLT_MAX * (1 - 2.0 ** -20)]
    n = int(np.prod(shape))
    k = rng.choice(ks, size=n)
    v = ((k + 0.5) * np.float64(s) + np.float64(zero)).astype(F32)
    return ulp_step(v, rng.integers(-3, 4, size=n)).reshape(shape)


def with_specials(x, seed=0):
    """About 2 % of x replaced by -0.0, +0.0, +-1e-40, +-FLT_MAX and +-inf (every one at least once)."""
    sp = np.array([-0.0, 0.0, -1e-40, 1e-40, -FLT_MAX, FLT_MAX, -np.inf, np.inf], dtype=F32)
    rng = np.random.default_rng(_seed("specials", x.shape, seed))
    out = np.array(x, dtype=F32)
    flat = out.reshape(-1)
    pos = rng.choice(flat.size, size=max(len(sp), flat.size // 50), replace=False)
    flat[pos] = sp[np.arange(pos.size) % len(sp)]
    return out


def emulate(x, s, zero, bits, sym, r, exact=True):
    """The kernels' quantizer in numpy fp32 (qdq_screen, qdq_exact_t, rintf), 1 / s taken as ``r``:
    (codes int64, need).  ``exact=False`` removes the IEEE divide."""
    qmin, qmax = (F32(t) for t in grid(bits, sym))
    s, r = F32(s), F32(r)
    negmn = F32(-0.0) if sym else -F32(zero)
    with np.errstate(all="ignore"):
        u = (np.asarray(x, dtype=F32) + negmn).astype(F32)
        t = np.fmin(np.fmax((u * r).astype(F32), qmin), qmax)   # fminf / fmaxf: a NaN operand is ignored
        d = ((t - np.floor(t)).astype(F32) - F32(0.5)).astype(F32)
        need = ~(np.abs(d) > (np.abs(t) * F32(2.0 ** -20)).astype(F32))
        if exact:
            t = np.where(need, np.fmin(np.fmax((u / s).astype(F32), qmin), qmax), t)
    return np.rint(t).astype(np.int64), need


def reciprocals(s):
    """fl32(1 / s) and its two fp32 neighbours (v_rcp_f32 is good to one ulp)."""
    r = F32(np.float64(1.0) / np.float64(s))
    return [np.nextafter(r, F32(0)), r, np.nextafter(r, F32(np.inf))]


def single_tie_x(shape, rng_pair, bits, sym, pos, f32=False, seed=0):
    """x of ``shape`` whose quotients lie at least 0.2 from every half-integer, except the element at
    flat position ``pos``: a near-tie whose code the quantizer without its exact path gets wrong
    (for 1 / s and both its fp32 neighbours where such a value exists, else for 1 / s)."""
    s, zero = qparams(rng_pair, bits, sym, f32)
    qmin, qmax = grid(bits, sym)
    rng = np.random.default_rng(_seed("single", tuple(shape), rng_pair, bits, sym, f32, seed))
    n = int(np.prod(shape))
    k = rng.integers(qmin, qmax + 1, size=n).astype(np.float64)
    x = ((k + rng.uniform(-0.3, 0.3, size=n)) * np.float64(s) + np.float64(zero)).astype(F32)
    x[pos] = _wrong_tie(rng_pair, bits, sym, f32)
    return x.reshape(shape)


@functools.lru_cache(maxsize=None)
def _wrong_tie(rng_pair, bits, sym, f32):
    s, zero = qparams(rng_pair, bits, sym, f32)
    qmin, qmax = grid(bits, sym)
    ks = np.arange(qmin, qmax, dtype=np.float64)
    cand = np.concatenate([ulp_step(((ks + 0.5) * np.float64(s) + np.float64(zero)).astype(F32), d) for d in range(-3, 4)])
    want = oracle_codes(cand, rng_pair, bits, sym, f32)[0]
    wrong = [emulate(cand, s, zero, bits, sym, r, exact=False)[0] != want for r in reciprocals(s)]
    for sel in (wrong[0] & wrong[1] & wrong[2], wrong[1]):
        if sel.any():
            return cand[np.argmax(sel)]
    raise AssertionError("no near-tie the reciprocal quotient gets wrong on %r at %d bits" % (rng_pair, bits))


# ---- the cases -------------------------------------------------------------------------------
LIN_M, LIN_N = 70, 17   # two 64-row blocks with a 6-row tail; the wave tile is 32 x 32, the K step 64
#: variant -> (K, device range, scale_f32, x a column slice at element 3, B signed).  K = 168: 16-B
#: loads, two full steps and a 40-element tail (lanes holding 16, 16, 8 and 0); 166: the 4-B path
LIN_VARIANTS = {"host": (168, False, False, False, 0), "dev": (166, True, False, False, 1), "f32": (168, False, True, True, 1)}
#: (range, bits, symmetric, variant)
LINEAR_CASES = [(r, b, sym, v) for r in RANGES for b in (2, 3, 4, 8) for sym in (False, True) for v in LIN_VARIANTS] + \
    [("asym", 5, False, "host"), ("sym", 5, True, "dev"), ("relu6", 6, False, "f32"), ("below0", 6, True, "host"),
     ("above0", 7, False, "dev"), ("zero_tie", 7, True, "f32")]

#: three row blocks, a K tail (K = 144) and padding on all four borders
CONV_GEOMS = {"nopad": KC.GEOMS["nopad"], "pad1": CC._g(2, 16, 9, 9, 17, 3, 1, 1, 1), "b": CC.CASES["b"], "d": CC.CASES["d"]}
#: bits -> (device range, scale_f32, B signed)
CONV_VARIANTS = {8: (True, False, 0), 4: (False, True, 1), 2: (False, False, 1)}
#: (geometry, range, bits, symmetric)
CONV_CASES = [(g, r, b, sym) for g in CONV_GEOMS for r in RANGES for b in CONV_VARIANTS for sym in (False, True)]

DW_GEOMS = ["mnv2_s1", "mnv2_s2", "dilated", "deep_pad", "k7_s2", "one_pixel", "wide", "mult2"]
#: bits -> (device range, scale_f32, B signed)
DW_VARIANTS = {8: (True, False, 0), 4: (False, True, 1)}
DW_CASES = [(g, r, b, sym) for g in DW_GEOMS for r in RANGES for b in DW_VARIANTS for sym in (False, True)]

N_CASES = (174, 168, 224)   # linear, conv, depthwise


def case_range(rname, dev):
    return device_pair(RANGES[rname]) if dev else RANGES[rname]


def has_bias(rname):
    """The degenerate range runs without a bias: at s = 1e-8 one code step is far below an ulp of a
    bias of order 1, and the result would not show the codes."""
    return rname != "degenerate"


def case_bias(rname, w):
    return w.bias if has_bias(rname) else None


def linear_case(rname, bits, sym, variant, x=None):
    """(x [M, K], B's case, range, K, expected [M, N]) of a LINEAR_CASES entry; ``x`` replaces the boundary data."""
    K, dev, f32, sliced, b_signed = LIN_VARIANTS[variant]
    pair = case_range(rname, dev)
    if x is None:
        x = boundary_x((LIN_M, K), pair, bits, sym, f32)
    w = IC.build(LIN_M, LIN_N, K, 0, b_signed, 1, 0)   # only B is used
    qa, sa, za = oracle_codes(x, pair, bits, sym, f32)
    return x, w, pair, K, IC.statement(qa, w.qb, sa, za, w.sb, w.zb, case_bias(rname, w))


def conv_case(gname, rname, bits, sym, x=None, code_of_zero=False):
    """(x NCHW, B's case, range, expected NCHW) of a CONV_CASES entry."""
    g = CONV_GEOMS[gname]
    dev, f32, b_signed = CONV_VARIANTS[bits]
    pair = case_range(rname, dev)
    if x is None:
        x = boundary_x((g.B, g.C, g.H, g.W), pair, bits, sym, f32)
    w = KC.weights(g, b_signed, 1, 0)
    qa, sa, za = KC.quantized(x, g, pair, bits, sym, f32)
    return x, w, pair, KC.nchw(KC.statement(qa, KC.taps(g), w.qb, sa, za, w.sb, w.zb, case_bias(rname, w), code_of_zero), g)


def dw_case(gname, rname, bits, sym, x=None):
    """(x NCHW, B's case, range, expected NCHW) of a DW_CASES entry."""
    g = DC.GEOMS[gname]
    dev, f32, b_signed = DW_VARIANTS[bits]
    pair = case_range(rname, dev)
    if x is None:
        x = boundary_x((g.B, g.C, g.H, g.W), pair, bits, sym, f32)
    w = DC.weights(g, b_signed, 1, 0)
    return x, w, pair, DC.statement(x, g, w, pair, bits, sym, f32, bias=has_bias(rname))


def nan_expected_codes(x, rng_pair, bits, sym, f32=False):
    """The project's own rule (csrc/dfq_common.h), not the reference's: a NaN element takes qmin's
    code, fminf(fmaxf(NaN, qmin), qmax).  The oracle never sees the NaN (its cast is undefined
    there): it quantizes x with -inf in its place, which clamps to qmin."""
    nan = np.isnan(x)
    qa, sa, za = oracle_codes(np.where(nan, F32(-np.inf), x), rng_pair, bits, sym, f32)
    assert np.all(qa[nan] == grid(bits, sym)[0])
    return qa, sa, za


def integers_fit_int32():
    """P, Sa, Sb and T of every case lie inside int32 (the kernels accumulate in it)."""
    worst = 0
    for rname, bits, sym, variant in LINEAR_CASES:
        x, w, pair, K, _ = linear_case(rname, bits, sym, variant)
        qa = oracle_codes(x, pair, bits, sym, LIN_VARIANTS[variant][2])[0]
        worst = max([worst] + [int(np.abs(t).max()) for t in IC.integers(qa, w.qb)])
    for gname, rname, bits, sym in CONV_CASES:
        g = CONV_GEOMS[gname]
        x, w, pair, _ = conv_case(gname, rname, bits, sym)
        qa = KC.quantized(x, g, pair, bits, sym, CONV_VARIANTS[bits][1])[0]
        worst = max([worst] + [int(np.abs(t).max()) for t in KC.integers(qa, KC.taps(g), w.qb)])
    for gname in DW_GEOMS:   # a depthwise sum has at most 49 terms of 255 * 255
        g = DC.GEOMS[gname]
        worst = max(worst, DC.K(g) * 255 * 255)
    return worst


# ---- import-time self-checks -------------------------------------------------------------------
CHECK_SHAPE = (LIN_M, 168)
#: the smallest (b) near-tie share, (c) grid coverage and the range of (d) wrong codes seen
MEASURED = {}


def _check_inputs(emulate_fn=emulate):
    """(a) - (e) for every (range, bits, symmetric, scale_f32) the cases use, at CHECK_SHAPE."""
    share, cover, wrong_lo, wrong_hi = 1.0, 1.0, 10 ** 9, 0
    for rname, pair0 in RANGES.items():
        for pair in {pair0, device_pair(pair0)}:
            for bits in BITS:
                for sym in (False, True):
                    for f32 in (False, True):
                        what = (rname, pair, bits, sym, f32)
                        x = boundary_x(CHECK_SHAPE, pair, bits, sym, f32)
                        assert np.isfinite(x).all(), what                                       # (a)
                        s, zero = qparams(pair, bits, sym, f32)
                        want = oracle_codes(x, pair, bits, sym, f32)[0]
                        rs = reciprocals(s)
                        near = float(emulate_fn(x, s, zero, bits, sym, rs[1])[1].mean())
                        assert near >= 0.40, (what, near)                                       # (b)
                        qmin, qmax = grid(bits, sym)
                        seen = len(np.unique(want)) / (qmax - qmin + 1)
                        assert seen >= 0.90, (what, seen)                                       # (c)
                        nwrong = [int((emulate_fn(x, s, zero, bits, sym, r, exact=False)[0] != want).sum()) for r in rs]
                        assert max(nwrong) >= 1, what                                           # (d)
                        pow2 = float(np.frexp(s)[0]) == 0.5
                        if bits == 8 and not sym and not pow2:
                            assert min(nwrong) >= 1, (what, nwrong)
                        for r in rs:                                                            # (e)
                            bad = int((emulate_fn(x, s, zero, bits, sym, r)[0] != want).sum())
                            assert bad == 0, (what, float(r), bad)
                        if bits in (2, 4, 8) and not f32 and pair == pair0:
                            share, cover = min(share, near), min(cover, seen)
                            wrong_lo, wrong_hi = min(wrong_lo, max(nwrong)), max(wrong_hi, max(nwrong))
    MEASURED.update(near_tie_share=share, grid_coverage=cover, wrong_codes=(wrong_lo, wrong_hi), elements=int(np.prod(CHECK_SHAPE)))


def _bits_differ(a, b):
    return not np.array_equal(np.ascontiguousarray(a, dtype=F32).view(np.uint32), np.ascontiguousarray(b, dtype=F32).view(np.uint32))


def _check_one_code_shows():
    """(f): one activation code changed by +-1 changes the expected output's bits, at sampled
    positions of the linear, conv and depthwise statements (K <= 1024: the step stays above an
    fp32 ulp of the result; row 0 of B is all the largest code)."""
    rng = np.random.default_rng(7)

    def flip(qa, m, k, bits, sym):
        qmin, qmax = grid(bits, sym)
        q2 = qa[m:m + 1].copy()
        q2[0, k] += 1 if q2[0, k] < qmax else -1
        return q2

    for rname, bits, sym, variant in LINEAR_CASES[::7]:
        x, w, pair, K, _ = linear_case(rname, bits, sym, variant)
        assert K <= 1024
        qa, sa, za = oracle_codes(x, pair, bits, sym, LIN_VARIANTS[variant][2])
        for m, k in zip(rng.integers(0, LIN_M, 4), rng.integers(0, K, 4)):
            args = (w.qb, sa, za, w.sb, w.zb, case_bias(rname, w))
            assert _bits_differ(IC.statement(qa[m:m + 1], *args), IC.statement(flip(qa, m, k, bits, sym), *args)), (rname, bits, sym, variant)
    for gname, rname, bits, sym in CONV_CASES[::11]:
        g = CONV_GEOMS[gname]
        assert CC.K(g) <= 1024
        x, w, pair, _ = conv_case(gname, rname, bits, sym)
        qa, sa, za = KC.quantized(x, g, pair, bits, sym, CONV_VARIANTS[bits][1])
        v = KC.taps(g)
        on = np.argwhere(v == 1)
        for m, k in on[rng.integers(0, len(on), 4)]:
            args = (v[m:m + 1], w.qb, sa, za, w.sb, w.zb, case_bias(rname, w))
            assert _bits_differ(KC.statement(qa[m:m + 1], *args), KC.statement(flip(qa, m, k, bits, sym), *args)), (gname, rname, bits, sym)
    for gname, rname, bits, sym in DW_CASES[::13]:
        g = DC.GEOMS[gname]
        g1 = DC.one_channel(g)
        x, w, pair, _ = dw_case(gname, rname, bits, sym)
        c = int(rng.integers(0, g.C))
        qa, sa, za = KC.quantized(x[:, c:c + 1], g1, pair, bits, sym, DW_VARIANTS[bits][1])
        v = KC.taps(g1)
        on = np.argwhere(v == 1)
        rows = slice(c * g.mult, (c + 1) * g.mult)
        for m, k in on[rng.integers(0, len(on), 2)]:
            args = (v[m:m + 1], w.qb[rows], sa, za, w.sb[rows], w.zb[rows], w.bias[rows] if has_bias(rname) else None)
            assert _bits_differ(KC.statement(qa[m:m + 1], *args), KC.statement(flip(qa, m, k, bits, sym), *args)), (gname, rname, bits, sym)


def _check_single_tie():
    """single_tie_x raises the screen at its one position only, for 1 / s and both neighbours, and
    the quantizer without its exact path gets that element's code wrong."""
    for rname, bits, sym in SINGLE_TIE_RANGES:
        pair = RANGES[rname]
        s, zero = qparams(pair, bits, sym)
        x = single_tie_x(CHECK_SHAPE, pair, bits, sym, pos=777)
        want = oracle_codes(x, pair, bits, sym)[0]
        for r in reciprocals(s):
            assert np.flatnonzero(emulate(x, s, zero, bits, sym, r)[1]).tolist() == [777], (rname, float(r))
        got = emulate(x, s, zero, bits, sym, reciprocals(s)[1], exact=False)[0]
        assert np.flatnonzero(got != want).tolist() == [777], rname
        z = emulate(np.zeros(1, F32), s, zero, bits, sym, reciprocals(s)[1])[1]
        assert not z.any(), rname   # a dummy 0.0 does not raise the screen on these ranges


#: (range, bits, symmetric) of the single near-tie tests
SINGLE_TIE_RANGES = [("asym", 8, False), ("sym", 8, True)]


def _self_check():
    assert (len(LINEAR_CASES), len(CONV_CASES), len(DW_CASES)) == N_CASES
    g = CONV_GEOMS["pad1"]
    assert (CC.K(g), CC.M(g)) == (144, 162)
    s, zero = qparams(RANGES["zero_tie"], 8, False)
    assert (float(s), float(zero)) == (1.0, -1.5)
    assert emulate(np.zeros(1, F32), s, zero, 8, False, F32(1.0))[1].all()   # 0.0 sits on the tie 1.5
    assert float(qparams(RANGES["degenerate"], 8, False)[0]) == float(F32(1e-8))
    _check_inputs()
    _check_single_tie()
    _check_one_code_shows()


_self_check()
