"""Geometries, operands and the expected result of dfq_int_conv2d, in numpy and CPU torch only
(tests/test_int_conv_host.py walks the index arithmetic of the geometries on the CPU,
tests/test_gpu_int_conv.py runs them).

``statement()`` is the contract of include/dfq_hip.h in int64 / float64: the activation codes
come from the oracle's given-range quantizer applied to the ``F.unfold`` matrix, v from
``F.unfold`` of ones, and a padding tap (v = 0) is absent from every sum.  With
``code_of_zero=True`` it is the other rule -- what quantizing the materialised unfold matrix
computes, a padding tap standing for the code of 0.0 -- which the tests must be able to tell
apart.  At import the module checks what the tests lean on: P, Sa, Sb and T of every case fit
int32; on the asymmetric range (-1.3, 2.5), where 0 is off the 8-bit grid, the two rules differ
on every geometry with padding taps and agree on the others; and on the two smallest
geometries ``statement()`` is within 2^-23 relative of exact rational arithmetic."""
from fractions import Fraction

import numpy as np
import torch
import torch.nn.functional as F

from oracle import oracle
from tests import int_gemm_cases as IC
from tests import mx_conv_cases as CC

#: the MX convolution's eight, a k x k layer without padding, and two where OH * OW < 4 (a
#: lane's four rows span several images)
GEOMS = {**CC.CASES,
         "nopad": CC._g(2, 5, 7, 7, 9, 3, 1, 0, 1),
         "one_pixel": CC._g(7, 4, 3, 3, 5, 3, 1, 0, 1),
         "three_pixels": CC._g(5, 2, 1, 5, 33, (1, 3), 1, 0, 1)}
PADDED = [n for n, g in GEOMS.items() if g.padding != (0, 0)]
ASYM_RANGE, SYM_RANGE = (-1.3, 2.5), (-1.75, 1.5)
#: name -> (bits, symmetric, device range, scale_f32, b_signed, per_row, packed)
CONFIGS = {"a8-dev-rowu": (8, False, True, False, 0, 1, 0),
           "s8-host-tens": (8, True, False, False, 1, 0, 0),
           "a4-f32-pack": (4, False, False, True, 1, 1, 1)}


def unfold(x: np.ndarray, g) -> np.ndarray:
    """The im2col matrix [M, K] of x [B, C, H, W]: row (b, oh, ow), column (c, kh, kw), 0.0 at padding taps."""
    cols = F.unfold(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)), g.kernel, g.dilation, g.padding, g.stride)
    return cols.transpose(1, 2).reshape(-1, cols.shape[1]).contiguous().numpy()


def taps(g) -> np.ndarray:
    """v [M, K] in int64: 1 where the tap lies inside the image."""
    return unfold(np.ones((g.B, g.C, g.H, g.W), np.float32), g).astype(np.int64)


def nchw(out2d: np.ndarray, g) -> np.ndarray:
    oh, ow = CC.out_size(g)
    return np.ascontiguousarray(out2d.reshape(g.B, oh, ow, -1).transpose(0, 3, 1, 2))


def make_x(g, rng_pair, bits, sym, seed=0) -> np.ndarray:
    """x [B, C, H, W]: values outside the range (they clamp), its ends, zeros and, on asymmetric
    ranges, quotients at and next to a half-integer (the quantizer's exact-divide path)."""
    mn, mx = rng_pair
    rng = np.random.default_rng(seed + 1000 * bits + int(sym))
    x = rng.uniform(mn - 0.5, mx + 0.5, size=(g.B, g.C, g.H, g.W)).astype(np.float32)
    flat = x.reshape(-1)
    flat[0:3] = (mn, mx, 0.0)
    flat[-1] = 0.0
    if not sym and flat.size >= 19:
        step = np.float32((mx - mn) / (2 ** bits - 1))
        ties = (np.float32(mn) + (np.arange(8, dtype=np.float32) % (2 ** bits - 1) + np.float32(0.5)) * step).astype(np.float32)
        flat[3:11], flat[11:19] = ties, np.nextafter(ties, np.float32(np.inf))
    return x


def quantized(x, g, rng_pair, bits, sym, f32=False):
    """The oracle's codes of the unfold matrix on the given range: (qa [M, K] int64, scale [1], zero [1])."""
    o = oracle.quantize(unfold(x, g), bits, oracle.TENSOR_SYM if sym else oracle.TENSOR_ASYM, rows=1,
                        flags=oracle.F_GIVEN | (oracle.F_F32 if f32 else 0), given=rng_pair)
    return o["codes"].astype(np.int64), o["scale"], o["zero"]


def weights(g, b_signed, per_row, packed) -> IC.Case:
    """B [N, K] (and a bias) as tests/int_gemm_cases.py builds it; only the B side of the case is used."""
    return IC.build(2, g.N, CC.K(g), 0, b_signed, per_row, packed)


def integers(qa, v, qb):
    """(P [M, N], Sa [M], Sb [M, N], T [M]) in int64; the products run in float64, exactly."""
    a = (v * qa).astype(np.float64)
    P = (a @ qb.astype(np.float64).T).astype(np.int64)
    Sb = (v.astype(np.float64) @ qb.astype(np.float64).T).astype(np.int64)
    return P, (v * qa).sum(axis=1), Sb, v.sum(axis=1)


def statement(qa, v, qb, sa, za, sb, zb, bias, code_of_zero=False) -> np.ndarray:
    """The contract, [M, N] float32: exact integers, then the fp64 steps in its order, one
    rounding.  za is always present; zb and bias may be None."""
    if code_of_zero:
        v = np.ones_like(v)
    P, Sa, Sb, T = integers(qa, v, qb)
    d = lambda t: np.asarray(t, dtype=np.float32).astype(np.float64).reshape(-1)   # noqa: E731
    N = qb.shape[0]
    sa, za, sb = d(sa)[0], d(za)[0], np.broadcast_to(d(sb), (N,)) if d(sb).size == 1 else d(sb)
    acc = (sa * sb)[None, :] * P.astype(np.float64)
    if zb is not None:
        zb = np.broadcast_to(d(zb), (N,))
        acc = acc + (sa * zb)[None, :] * Sa.astype(np.float64)[:, None]
    acc = acc + (za * sb)[None, :] * Sb.astype(np.float64)
    if zb is not None:
        acc = acc + (za * zb)[None, :] * T.astype(np.float64)[:, None]
    if bias is not None:
        acc = acc + d(bias)[None, :]
    return acc.astype(np.float32)


def expected(name, config, x=None, zb=True, bias=True, code_of_zero=False):
    """(x, weights case, expected NCHW result) of a geometry under a configuration of CONFIGS."""
    g = GEOMS[name]
    bits, sym, dev, f32, b_signed, per_row, packed = CONFIGS[config]
    rng_pair = SYM_RANGE if sym else ASYM_RANGE
    if dev:   # a device range holds floats
        rng_pair = tuple(float(np.float32(t)) for t in rng_pair)
    if x is None:
        x = make_x(g, rng_pair, bits, sym)
    w = weights(g, b_signed, per_row, packed)
    qa, sa, za = quantized(x, g, rng_pair, bits, sym, f32)
    out = statement(qa, taps(g), w.qb, sa, za, w.sb, w.zb if zb else None, w.bias if bias else None, code_of_zero)
    return x, w, nchw(out, g)


def exact(qa, v, qb, sa, za, sb, zb, bias):
    """The real-number result as Fractions [M][N]: the affine values of the taps inside the image
    multiplied and summed element by element, nothing factored out."""
    f = lambda t: Fraction(float(t))   # noqa: E731
    N = qb.shape[0]
    sbn = [f(sb[n if len(sb) > 1 else 0]) for n in range(N)]
    zbn = [f(zb[n if len(zb) > 1 else 0]) for n in range(N)]
    A = [[int(q) * f(sa[0]) + f(za[0]) if on else None for q, on in zip(row, vrow)] for row, vrow in zip(qa, v)]
    Bm = [[int(q) * sbn[n] + zbn[n] for q in row] for n, row in enumerate(qb)]
    return [[sum((a * b for a, b in zip(A[m], Bm[n]) if a is not None), f(bias[n])) for n in range(N)] for m in range(len(A))]


def _self_check():
    smallest = sorted(GEOMS, key=lambda n: CC.M(GEOMS[n]) * GEOMS[n].N * CC.K(GEOMS[n]))[:2]
    assert set(PADDED) == {"a", "b", "c", "d", "e", "f"}
    for name, g in GEOMS.items():
        v = taps(g)
        assert v.shape == (CC.M(g), CC.K(g))
        assert (v.min() == 0) == (name in PADDED), name
        for config, (bits, sym, dev, f32, b_signed, per_row, packed) in CONFIGS.items():
            if packed and CC.K(g) % 2:
                continue   # refused by the entry point: no packed row starts on a byte
            rng_pair = SYM_RANGE if sym else ASYM_RANGE
            x = make_x(g, rng_pair, bits, sym)
            w = weights(g, b_signed, per_row, packed)
            qa, sa, za = quantized(x, g, rng_pair, bits, sym, f32)
            for t in integers(qa, v, w.qb) + integers(qa, np.ones_like(v), w.qb):
                assert -2 ** 31 <= t.min() and t.max() < 2 ** 31, (name, config)
            args = (qa, v, w.qb, sa, za, w.sb, w.zb, w.bias)
            real, coded = statement(*args), statement(*args, code_of_zero=True)
            if config == "a8-dev-rowu":
                # 0 is off the grid: the code of 0.0 stands for q0 * s + min != 0
                assert np.array_equal(real, coded) == (name not in PADDED), name
                assert float(np.float64(qa[v == 0][0]) * np.float64(sa[0]) + np.float64(za[0])) != 0.0 if name in PADDED else True
            if name in smallest and not sym:
                ex = exact(*args)
                for m in range(real.shape[0]):
                    for n in range(real.shape[1]):
                        assert abs(Fraction(float(real[m, n])) - ex[m][n]) <= Fraction(1, 2 ** 23) * abs(ex[m][n]), (name, config, m, n)
    f = GEOMS["f"]
    assert (taps(f).sum(axis=1) == 0).any()   # whole im2col rows in padding


_self_check()
