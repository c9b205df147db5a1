"""Group-wise B parameters and the expected result of dfq_int_gemm_grouped, dfq_int_linear_grouped
and dfq_int_conv2d_grouped, in numpy only: ``statement()`` is the grouped contract of
include/dfq_hip.h in int64 / float64.  The groups of a row take scales spread over six orders of
magnitude and distinct zeros, so a wrong group index, a boundary off by a step or a dropped
short group moves the result far above an ulp."""
import zlib

import numpy as np

from tests import int_gemm_cases as IC

#: (K, g): wide loads; byte loads with a last group of 8 (whole and half steps); a last group of
#: exactly half a step; one group
GEMM_KG = [(256, 32), (256, 64), (256, 128), (200, 64), (200, 32), (96, 64), (40, 64), (64, 64)]
BAD_GROUPS = [0, -1, 16, 48, 96]


def group_params(N, K, g):
    """(sb, zb) float32 [N, G]: full-mantissa scales in [1e-5, 1e2), zeros in [-3, 3]."""
    rng = np.random.default_rng(zlib.crc32(repr((N, K, g)).encode()))
    G = -(-K // g)
    sb = (IC._scales(rng, N * G).astype(np.float64) * 10.0 ** rng.integers(-3, 4, size=N * G)).astype(np.float32)
    return sb.reshape(N, G), rng.uniform(-3, 3, size=(N, G)).astype(np.float32)


def statement(qa, qb, sa, za, sb, zb, bias, g, v=None) -> np.ndarray:
    """The grouped contract: per group the exact integers, then its fp64 steps in order, groups
    ascending, the very first term assigning; one rounding to fp32.  qa [M, K], qb [N, K]
    integers; sb, zb [N, G] float32; za, zb and bias may be None; v [M, K]: the convolution's tap
    mask (the sums carry it and K_j becomes T_j[m]), None: all ones."""
    M, K = qa.shape
    v = np.ones((M, K), np.int64) if v is None else v
    d = lambda t: np.asarray(t, dtype=np.float32).astype(np.float64)   # noqa: E731
    sa, sb = d(sa).reshape(-1)[0], d(sb)
    za = None if za is None else d(za).reshape(-1)[0]
    zb = None if zb is None else d(zb)
    acc = None
    for j in range(-(-K // g)):
        k = slice(j * g, min((j + 1) * g, K))
        a, b, vj = (v * qa)[:, k].astype(np.float64), qb[:, k].astype(np.float64), v[:, k].astype(np.float64)
        P, Sa, Sb, T = a @ b.T, a.sum(axis=1), vj @ b.T, vj.sum(axis=1)   # exact: integers below 2^53
        t = (sa * sb[:, j])[None, :] * P
        acc = t if acc is None else acc + t
        if zb is not None:
            acc = acc + (sa * zb[:, j])[None, :] * Sa[:, None]
        if za is not None:
            acc = acc + (za * sb[:, j])[None, :] * Sb
        if za is not None and zb is not None:
            acc = acc + (za * zb[:, j])[None, :] * T[:, None]
    if bias is not None:
        acc = acc + d(bias).reshape(-1)[None, :]
    return acc.astype(np.float32)
