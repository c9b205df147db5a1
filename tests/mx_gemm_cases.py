"""Operands of dfq_mx_gemm written directly as MX codes and scale bytes in numpy -- no
quantizer in the loop -- with their exact products (tests/test_gpu_mx_gemm.py).

Elements come from the magnitudes every one of the four formats holds, {0, 0.5, 1, 1.5,
2, 3, 4, 6}, with random signs, and every block of every row of both operands draws its
own scale byte from {126, 127, 128}.  A value is then a multiple of 2^-2 (0.5 * 2^-1) and
at most 12, a product a multiple of 2^-4 and at most 144, and at K <= 416 every partial
sum in any order stays below 2^16 -- 20 bits with the four fraction bits -- so it is
exact in fp32 and the product is known to the bit from integer arithmetic: 4a and 4b are
integers.  (At K = 1280 the bound is 2^17.5: still exact.)
The codes are found in tables written from the formats' definitions (the sign bit above
the index of the magnitude), and packed as include/dfq_hip.h states: FP4 element 2k in the
low nibble, FP6 32 six-bit codes dense and little-endian, FP8 a byte each."""
from functools import lru_cache

import numpy as np

BLOCK = 32
GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
SCALE_BYTES = (126, 127, 128)
#: the issue's shapes (M, N, K)
SHAPES = [(16, 16, 128), (1, 1, 32), (17, 33, 96), (32, 48, 416), (16, 16, 40), (5, 1000, 1280), (200, 24, 144)]
FMTS = ["mxfp4", "mxfp6_e2m3", "mxfp6_e3m2", "mxfp8"]
PAIRS = [(a, b) for a in FMTS for b in FMTS]

# magnitude of every code without its sign bit, from the formats' definitions
_MAGS = {
    "mxfp4": np.array([(c & 1) * 0.5 if (c >> 1) == 0 else (2 + (c & 1)) * 2.0 ** ((c >> 1) - 2) for c in range(8)]),
    "mxfp6_e2m3": np.array([(c & 7) * 2.0 ** -3 if (c >> 3) == 0 else (8 + (c & 7)) * 2.0 ** ((c >> 3) - 4)
                            for c in range(32)]),
    "mxfp6_e3m2": np.array([(c & 3) * 2.0 ** -4 if (c >> 2) == 0 else (4 + (c & 3)) * 2.0 ** ((c >> 2) - 5)
                            for c in range(32)]),
    "mxfp8": np.array([(c & 7) * 2.0 ** -9 if (c >> 3) == 0 else (8 + (c & 7)) * 2.0 ** ((c >> 3) - 10)
                       for c in range(127)]),
}
SIGN_BIT = {"mxfp4": 0x8, "mxfp6_e2m3": 0x20, "mxfp6_e3m2": 0x20, "mxfp8": 0x80}
CODE_BYTES = {"mxfp4": 16, "mxfp6_e2m3": 24, "mxfp6_e3m2": 24, "mxfp8": 32}
assert np.array_equal(_MAGS["mxfp4"], GRID)


def blocks(K: int) -> int:
    return -(-K // BLOCK)


#: Worst |acc - sum a*b| / sum |a*b| measured on the MI355X over random data at nb <= 4 (one K
#: step) with an FP8 operand: Gaussian [32, 24] x [40, 24], mxfp8 x mxfp8
#: (tests/test_gpu_mx_gemm.py's own case; 3.13e-5 on another draw, mxfp8 x mxfp6_e2m3).  There the
#: instruction's own error -- about 2^-13 of the largest product of the step, whatever K:
#: DESIGN.md 3.8 -- exceeds the derived bound, which only grows with nb.
MEASURED_ONE_STEP = 3.187e-05


def accumulation_bound(nb: int) -> float:
    """The factor c of the contract |acc - sum a*b| <= c * sum |a*b| (include/dfq_hip.h):
    the derived 32 * nb * 2^-24 -- what any-order fp32 accumulation of the exact products
    meets, and what the hardware was measured to meet at nb >= 13 -- and, for nb <= 4, where
    the hardware exceeds it, twice the worst ratio measured there if that is more."""
    derived = 32 * nb * 2.0 ** -24
    return derived if nb > 4 else max(derived, 2 * MEASURED_ONE_STEP)


def element_codes(values: np.ndarray, fmt: str) -> np.ndarray:
    """The code of every value (each on the format's grid), uint8."""
    mags = _MAGS[fmt]
    idx = np.searchsorted(mags, np.abs(values))
    assert (mags[idx] == np.abs(values)).all(), fmt
    return (idx | np.where(np.signbit(values), SIGN_BIT[fmt], 0)).astype(np.uint8)


def pack(codes: np.ndarray, fmt: str) -> np.ndarray:
    """[rows, nb, 32] element codes -> [rows, nb, 16 | 24 | 32] bytes."""
    if fmt == "mxfp4":
        return (codes[..., 0::2] | (codes[..., 1::2] << 4)).astype(np.uint8)
    if fmt == "mxfp8":
        return codes.copy()
    q = codes.astype(np.uint32).reshape(*codes.shape[:-1], 8, 4)
    w = q[..., 0] | (q[..., 1] << 6) | (q[..., 2] << 12) | (q[..., 3] << 18)
    return np.stack([w & 0xFF, (w >> 8) & 0xFF, w >> 16], axis=-1).reshape(*codes.shape[:-1], 24).astype(np.uint8)


@lru_cache(maxsize=None)
def operand(rows: int, K: int, seed: int):
    """(values on the grid [rows, nb * 32] float64 with +0 padding past K, scale bytes [rows, nb])."""
    rng = np.random.default_rng(seed)
    nb = blocks(K)
    v = GRID[rng.integers(0, 8, (rows, nb * BLOCK))] * np.where(rng.random((rows, nb * BLOCK)) < 0.5, -1.0, 1.0)
    v[:, K:] = 0.0   # the padding of a partial last block: +0 codes, as the quantizer writes them
    s = np.array(SCALE_BYTES, np.uint8)[rng.integers(0, 3, (rows, nb))]
    v.setflags(write=False)
    s.setflags(write=False)
    return v, s


def encode(values: np.ndarray, scales: np.ndarray, fmt: str):
    """(codes uint8 [rows, nb, cb], scales) of grid values [rows, nb * 32]."""
    rows, nb = scales.shape
    return pack(element_codes(values, fmt).reshape(rows, nb, BLOCK), fmt), scales.copy()


def quarter_units(values: np.ndarray, scales: np.ndarray) -> np.ndarray:
    """4 * value * 2^(scale - 127) as int64: integers for the grid and SCALE_BYTES."""
    x = values.reshape(*scales.shape, BLOCK) * np.ldexp(4.0, scales.astype(np.int64) - 127)[:, :, None]
    assert (x == np.rint(x)).all()
    return x.reshape(values.shape).astype(np.int64)


@lru_cache(maxsize=None)
def exact_case(M: int, N: int, K: int):
    """The operands of a shape and their product, exact: (a_values, a_scales, b_values,
    b_scales, out float32 [M, N]).  The same values serve every format pair."""
    av, asc = operand(M, K, 1000 + 7 * M + K)
    bv, bsc = operand(N, K, 2000 + 11 * N + K)
    qa, qb = quarter_units(av, asc), quarter_units(bv, bsc)
    p16 = qa @ qb.T   # int64, 16 * the product
    # every partial sum in any order is an integer below 2^24 in units of 2^-4: exact in fp32
    assert (np.abs(qa) @ np.abs(qb).T).max() < 2 ** 24 and np.abs(qa).max() <= 48
    out = (p16.astype(np.float64) / 16.0).astype(np.float32)
    assert (out.astype(np.float64) * 16.0 == p16).all()
    if M == N and M > 1:
        assert not np.array_equal(out, out.T)   # a transposed C write cannot pass
    out.setflags(write=False)
    return av, asc, bv, bsc, out
