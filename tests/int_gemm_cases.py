"""Operands and the expected result of dfq_int_gemm, in numpy only: integer codes built
directly (no quantizer in the loop), their scales, zeros and bias, and ``statement()`` --
the contract of include/dfq_hip.h in int64 / float64.

Codes are uniform over the full byte (or, packed, nibble) range; row 0 of each operand is
all the largest code and row 1 all the smallest where those rows exist, so the extreme
sums occur.  Scales are full-mantissa floats in [0.01, 0.1], zeros lie in [-3, 3].  At
import the module checks what the tests lean on: P, Sa and Sb of every case fit int32, a
square case's result is not symmetric (a row / column swap of C would show), and on the
three smallest shapes ``statement()`` is within 2^-23 relative of exact rational
arithmetic."""
import zlib
from dataclasses import dataclass
from fractions import Fraction
from typing import Optional

import numpy as np

SHAPES = [(16, 16, 64), (1, 1, 1), (16, 16, 40), (3, 7, 65), (17, 33, 96), (65, 130, 64), (32, 48, 416), (200, 24, 144),
          (5, 1000, 1280), (16, 16, 32768)]   # the last: the overflow edge, 255 * 255 * 32768 < 2^31
#: (a_signed, b_signed, per_row, packed)
MODES = [(a, b, r, p) for a in (0, 1) for b in (0, 1) for r in (0, 1) for p in (0, 1)]


def all_cases():
    """Every (M, N, K, a_signed, b_signed, per_row, packed); packed skips odd K."""
    return [(m, n, k, *mode) for m, n, k in SHAPES for mode in MODES if not (mode[3] and k % 2)]


def case_id(c) -> str:
    return "%dx%dx%d-a%s-b%s%s%s" % (c[0], c[1], c[2], "su"[1 - c[3]], "su"[1 - c[4]], "-row" if c[5] else "", "-p4" if c[6] else "")


@dataclass
class Case:
    M: int
    N: int
    K: int
    a_signed: int
    b_signed: int
    per_row: int
    packed: int
    qa: np.ndarray            # int64 [M, K]: the integers the codes stand for
    qb: np.ndarray            # int64 [N, K]
    a_bytes: np.ndarray       # int8 / uint8 [M, K]
    b_bytes: np.ndarray       # int8 / uint8 [N, K], or [N, K / 2] packed
    sa: np.ndarray            # float32 [1]
    za: Optional[np.ndarray]  # float32 [1]
    sb: np.ndarray            # float32 [1] or [N]
    zb: Optional[np.ndarray]
    bias: Optional[np.ndarray]   # float32 [N]


def code_range(signed: int, packed: int = 0):
    bits = 4 if packed else 8
    return (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)


def pack4(q: np.ndarray) -> np.ndarray:
    """[rows, K] integers (K even) -> [rows, K / 2] bytes: element 2k in the low nibble,
    two's-complement nibbles (DFQ_PACK_INT4's layout)."""
    n = (q & 0xF).astype(np.uint8)
    return n[:, 0::2] | (n[:, 1::2] << 4)


def _codes(rng, rows, K, signed, packed=0):
    lo, hi = code_range(signed, packed)
    q = rng.integers(lo, hi + 1, size=(rows, K), dtype=np.int64)
    q[0, :] = hi
    if rows > 1:
        q[1, :] = lo
    return q


def _scales(rng, n):
    s = rng.uniform(0.01, 0.1, size=n).astype(np.float32)
    assert np.all(s.view(np.uint32) & 0xFFFF)   # full mantissas: the float x float products need double
    return s


def build(M, N, K, a_signed, b_signed, per_row, packed) -> Case:
    rng = np.random.default_rng(zlib.crc32(repr((M, N, K, a_signed, b_signed, per_row, packed)).encode()))
    qa, qb = _codes(rng, M, K, a_signed), _codes(rng, N, K, b_signed, packed)
    npar = N if per_row else 1
    byte = lambda q, signed: q.astype(np.int8) if signed else q.astype(np.uint8)   # noqa: E731
    b_bytes = pack4(qb) if packed else byte(qb, b_signed)
    if packed and b_signed:
        b_bytes = b_bytes.view(np.int8)
    return Case(M, N, K, a_signed, b_signed, per_row, packed, qa, qb, byte(qa, a_signed), b_bytes,
                sa=_scales(rng, 1), za=rng.uniform(-3, 3, size=1).astype(np.float32),
                sb=_scales(rng, npar), zb=rng.uniform(-3, 3, size=npar).astype(np.float32),
                bias=rng.standard_normal(N).astype(np.float32))


def integers(qa: np.ndarray, qb: np.ndarray):
    """(P [M, N], Sa [M], Sb [N]) in int64.  The product runs in float64, exactly: every
    partial sum is an integer below 2^53."""
    P = (qa.astype(np.float64) @ qb.astype(np.float64).T).astype(np.int64)
    return P, qa.sum(axis=1), qb.sum(axis=1)


def statement(qa, qb, sa, za, sb, zb, bias, K=None) -> np.ndarray:
    """The contract: exact integers, then fp64 steps in its order, one rounding to fp32.
    qa [M, K], qb [N, K] integers; sa, za one float32; sb, zb one or N float32; za, zb and
    bias may be None (their terms are skipped)."""
    K = qa.shape[1] if K is None else K
    P, Sa, Sb = integers(qa, qb)
    d = lambda v: np.asarray(v, dtype=np.float32).astype(np.float64).reshape(-1)   # noqa: E731
    sa, sb = d(sa)[0], np.broadcast_to(d(sb), (qb.shape[0],)) if d(sb).size == 1 else d(sb)
    acc = (sa * sb)[None, :] * P.astype(np.float64)
    if zb is not None:
        zb = np.broadcast_to(d(zb), sb.shape)
        acc = acc + (sa * zb)[None, :] * Sa.astype(np.float64)[:, None]
    if za is not None:
        za = d(za)[0]
        acc = acc + ((za * sb) * Sb.astype(np.float64))[None, :]
    if za is not None and zb is not None:
        acc = acc + ((za * zb) * np.float64(K))[None, :]
    if bias is not None:
        acc = acc + d(bias)[None, :]
    return acc.astype(np.float32)


def expected(c: Case) -> np.ndarray:
    return statement(c.qa, c.qb, c.sa, c.za, c.sb, c.zb, c.bias)


def exact(c: Case):
    """The real-number result as Fractions [M][N]: the affine values multiplied and summed
    element by element, nothing factored out."""
    f = lambda v: Fraction(float(v))   # noqa: E731
    sb = [f(c.sb[n if c.per_row else 0]) for n in range(c.N)]
    zb = [f(c.zb[n if c.per_row else 0]) for n in range(c.N)]
    A = [[int(q) * f(c.sa[0]) + f(c.za[0]) for q in row] for row in c.qa]
    B = [[int(q) * sb[n] + zb[n] for q in row] for n, row in enumerate(c.qb)]
    return [[sum((a * b for a, b in zip(A[m], B[n])), f(c.bias[n])) for n in range(c.N)] for m in range(c.M)]


def _self_check():
    smallest = sorted(SHAPES, key=lambda s: s[0] * s[1] * s[2])[:3]
    for spec in all_cases():
        c = build(*spec)
        P, Sa, Sb = integers(c.qa, c.qb)
        for v in (P, Sa, Sb):
            assert -2 ** 31 <= v.min() and v.max() < 2 ** 31, case_id(spec)
        if c.packed:
            assert c.b_bytes.shape == (c.N, c.K // 2)
        if spec[:3] == (16, 16, 64):
            out = expected(c)
            assert np.any(out != out.T), case_id(spec)
        if spec[:3] in smallest:
            out, ex = expected(c), exact(c)
            for m in range(c.M):
                for n in range(c.N):
                    assert abs(Fraction(float(out[m, n])) - ex[m][n]) <= Fraction(1, 2 ** 23) * abs(ex[m][n]), case_id(spec)


_self_check()
