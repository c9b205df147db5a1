"""The two MXFP6 element formats (E2M3, E3M2) of dfq_mx_quantize_batch restated in
numpy, and the cases their tests run: tests/test_mx6_host.py checks the statement's
preconditions without a GPU, tests/test_gpu_mx6.py runs the cases.

The statement is that of tests/mx_cases.py (32-element blocks, +0 padding,
X = clamp(floor(log2 amax) - emax, -127, 127), nearest table magnitude with ties to
the even code, saturation, the sign bit kept) with two more tables; that module is
imported and left as it is.  New here is the code layout: uint8 [rows, nb, 24], a
block's 32 six-bit codes packed densely, little-endian -- element i in bits
[6i, 6i+6) of the block's 192-bit string, byte b its bits [8b, 8b+8) -- and the codes
pointer's own alignment as a case axis (the 16-B path stores dwords, so a pointer
1 or 2 bytes past a 4-B boundary must take the byte path).
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from tests import mx_cases as MC
from tests.mx_cases import BLOCK, blocks, esum_reference, outlier_data, round_to_table, shared_exponent  # noqa: F401

# E2M3 `s ee mmm`, bias 1: subnormals m * 2^-3, normals (8 + m) * 2^(e - 4)
E2M3_MAGS = np.array([(c & 7) * 2.0 ** -3 if (c >> 3) == 0 else (8 + (c & 7)) * 2.0 ** ((c >> 3) - 4) for c in range(32)])
# E3M2 `s eee mm`, bias 3: subnormals m * 2^-4, normals (4 + m) * 2^(e - 5)
E3M2_MAGS = np.array([(c & 3) * 2.0 ** -4 if (c >> 2) == 0 else (4 + (c & 3)) * 2.0 ** ((c >> 2) - 5) for c in range(32)])
assert E2M3_MAGS[1] == 0.125 and E2M3_MAGS[-1] == 7.5 and E3M2_MAGS[1] == 0.0625 and E3M2_MAGS[-1] == 28.0
assert (np.diff(E2M3_MAGS) > 0).all() and (np.diff(E3M2_MAGS) > 0).all()
#: fmt -> (table, emax, sign bit, code bytes per block)
FORMATS = {"mxfp6_e2m3": (E2M3_MAGS, 2, 0x20, 24), "mxfp6_e3m2": (E3M2_MAGS, 4, 0x20, 24)}
#: the kernel's traits (mx_encode): fmt -> (mbits, emin, max_code)
TRAITS = {"mxfp6_e2m3": (3, 0, 0x1F), "mxfp6_e3m2": (2, -2, 0x1F)}
#: values inside the saturating band (max, 2^(emax+1)); the middle one is the tie between the
#: last code and the carry out of the table
BAND = {"mxfp6_e2m3": (7.625, 7.75, 7.875), "mxfp6_e3m2": (29.0, 30.0, 31.0)}

ROWS = [1, 3, 65]
ROW_LENS = [1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 64, 100, 255, 256, 257, 1024, 1028, 4096, 4097]
OFFSETS = [0, 1, 3]           # source: floats from a 16-B boundary
CODE_OFFSETS = [0, 1, 2]      # codes: bytes from a 4-B boundary
KHWS = [1, 9, 49]
OUTPUTS = ["all", "inplace", "nodst", "nocodes"]
EXPONENTS = [0, -7, 5, -60, 90]


def pack6(code: np.ndarray) -> np.ndarray:
    """[..., 32] six-bit codes -> [..., 24] bytes, from the bit string itself."""
    bits = (code[..., :, None].astype(np.uint8) >> np.arange(6, dtype=np.uint8)) & 1      # element i: bits 6i .. 6i+5
    bits = bits.reshape(*code.shape[:-1], code.shape[-1] * 6)
    return np.packbits(bits, axis=-1, bitorder="little")


def unpack6(b: np.ndarray) -> np.ndarray:
    bits = np.unpackbits(b, axis=-1, bitorder="little").reshape(*b.shape[:-1], -1, 6)
    return (bits << np.arange(6, dtype=np.uint8)).sum(axis=-1).astype(np.uint8)


def pack6_words(code: np.ndarray) -> np.ndarray:
    """The same layout four elements at a time: w = c0 | c1<<6 | c2<<12 | c3<<18 ->
    bytes w & 0xFF, (w>>8) & 0xFF, w>>16."""
    q = code.astype(np.uint32).reshape(*code.shape[:-1], -1, 4)
    w = q[..., 0] | (q[..., 1] << 6) | (q[..., 2] << 12) | (q[..., 3] << 18)
    return np.stack([w & 0xFF, (w >> 8) & 0xFF, w >> 16], axis=-1).astype(np.uint8).reshape(*code.shape[:-1], -1)


def statement(x: np.ndarray, fmt: str, fp32_multiply: bool = False) -> dict:
    """The contract for x (float32 [rows, row_len]); as mx_cases.statement, FP6 tables
    and packing."""
    mags, emax, sign_bit, cbytes = FORMATS[fmt]
    assert x.dtype == np.float32 and x.ndim == 2
    rows, row_len = x.shape
    nb = blocks(row_len)
    xp = np.zeros((rows, nb * BLOCK), np.float32)
    xp[:, :row_len] = x
    xb = xp.reshape(rows, nb, BLOCK)
    amax = np.abs(xb).max(axis=2)
    X = shared_exponent(amax, emax)
    if fp32_multiply:
        inv = np.ldexp(np.float32(1.0), -X).astype(np.float32)
        v32 = np.abs(xb) * inv[:, :, None]
        assert v32.dtype == np.float32
        v = v32.astype(np.float64)
    else:
        v = np.ldexp(np.abs(xb).astype(np.float64), -X[:, :, None])
    idx, tie_down, tie_up, sat = round_to_table(v, mags)
    neg = np.signbit(xb)
    code = (idx | np.where(neg, sign_bit, 0)).astype(np.uint8)
    y64 = np.copysign(np.ldexp(mags[idx], X[:, :, None]), np.where(neg, -1.0, 1.0))
    y = y64.astype(np.float32)
    assert (y.astype(np.float64) == y64).all()   # exact in fp32
    codes = pack6(code)
    assert codes.shape == (rows, nb, cbytes)
    return {"codes": codes, "scales": (X + 127).astype(np.uint8), "y": y.reshape(rows, nb * BLOCK)[:, :row_len].copy(),
            "element_codes": code, "v": v, "tie_down": tie_down, "tie_up": tie_up, "saturated": sat}


def encode(v: np.ndarray, fmt: str) -> np.ndarray:
    """mx_encode's integer rule on magnitudes v (float32 values in [0, 2^(emax+1))):
    e = max(exponent(v), emin), n = rne(v * 2^(mbits - e)), code n + ((e - emin) << mbits),
    an integer min with max_code."""
    mbits, emin, max_code = TRAITS[fmt]
    v = np.asarray(v, np.float32)
    e = (v.view(np.uint32) >> 23).astype(np.int64) - 127
    e = np.maximum(e, emin)
    n = np.rint(v.astype(np.float64) * np.exp2(mbits - e)).astype(np.int64)   # np.rint: half to even
    return np.minimum(n + ((e - emin) << mbits), max_code).astype(np.uint8)


@dataclass
class Case(MC.Case):
    code_offset: int = 0   # codes start this many bytes past a 4-B boundary


def _grid():
    """Every rows x row_len shape twice.  The first of a pair takes khw 1 (error sums for
    every element), the second khw 49 and no error sums (it divides none of these rows:
    _khw has the rows that 9 and 49 divide); formats alternate, offsets, code offsets
    and output sets walk their lists."""
    out, i = [], 0
    fmts = tuple(FORMATS)
    for ri, rows in enumerate(ROWS):
        for li, row_len in enumerate(ROW_LENS):
            for fi in range(2):
                fmt = fmts[(ri + li + fi) % 2]
                khw = 1 if fi == 0 else 49
                out.append(Case("grid_%dx%d_%s" % (rows, row_len, fmt), outlier_data(8000 + i, (rows, row_len)), fmt, khw,
                                OFFSETS[(ri + 2 * li + fi) % 3], OUTPUTS[(i // 2 + i // 8 + fi) % 4],
                                code_offset=CODE_OFFSETS[(i // 2 + i // 6) % 3]))
                i += 1
    return out


def _aligned():
    """Row lengths the 16-B path serves, source aligned, at every code offset and in both
    formats: offset 0 takes the dword stores, 1 and 2 must not."""
    out, i = [], 0
    for fmt in FORMATS:
        for rows, row_len in ((1, 4), (3, 16), (3, 32), (65, 64), (3, 100), (3, 256), (1, 1028), (3, 4096), (1, 4100)):
            for co in CODE_OFFSETS:
                out.append(Case("aligned_%dx%d_c%d_%s" % (rows, row_len, co, fmt), outlier_data(8300 + i, (rows, row_len)),
                                fmt, 1, 0, OUTPUTS[(i // 3 + i) % 3], code_offset=co))
                i += 1
    return out


def _khw():
    """Rows that khw 9 and 49 divide (among them the split rows of mx_cases._khw), with
    error sums through LDS."""
    out, i = [], 0
    for fmt in FORMATS:
        for rows, row_len, khw in ((3, 9, 9), (65, 27, 9), (3, 288, 9), (3, 49, 49), (2, 98, 49), (2, 3136, 49),
                                   (1, 4704, 49), (2, 4608, 9), (3, 2304, 9)):
            out.append(Case("khw%d_%dx%d_%s" % (khw, rows, row_len, fmt), outlier_data(8500 + i, (rows, row_len)), fmt,
                            khw, OFFSETS[i % 3], OUTPUTS[(i // 3) % 2], code_offset=CODE_OFFSETS[(i // 2) % 3]))
            i += 1
    return out


def _patterns(fmt: str):
    """Blocks of v values whose largest lies in [2^emax, 2^(emax+1)), so X = 0: every
    table entry; every midpoint (the exact ties) and the band; values at and below half
    the smallest subnormal."""
    mags = FORMATS[fmt][0]
    top = BAND[fmt][1]
    mids = (mags[:-1] + mags[1:]) / 2
    tiny = mags[1] * np.array([0.5, 0.25, 0.4375, 0.5625, 0.75])   # half the smallest subnormal ties to 0
    a = mags.copy()                                                # 32 magnitudes (the last one is >= 2^emax)
    b = np.concatenate([mids, [top]])                              # 31 midpoints + the band's tie
    c = np.concatenate([BAND[fmt], tiny, mids[:4], mags[-4:], np.full(BLOCK - 16, top)])
    for p in (a, b, c):
        assert len(p) == BLOCK and (p.astype(np.float32) == p).all() and p.max() >= mags[-1] and p.max() < 2 * 2.0 ** FORMATS[fmt][1]
    return [p.astype(np.float32) for p in (a, b, c)]


def _hand_made():
    out = []
    rng = np.random.default_rng(8900)
    for fmt, (mags, emax, _, _) in FORMATS.items():
        top = BAND[fmt][1]
        z = np.zeros((2, 40), np.float32)
        out.append(Case("zeros_" + fmt, z.copy(), fmt, 1, 0))
        out.append(Case("negzeros_" + fmt, -z, fmt, 1, 1, code_offset=1))
        one = np.zeros((3, 70), np.float32)
        one[0, 5], one[1, 33], one[2, 69] = 0.3, -1.7e-3, 12345.0
        out.append(Case("one_nonzero_" + fmt, one, fmt, 1, 0))
        p2 = np.clip(outlier_data(8901, (4, 64)), -0.125, 0.125)
        p2[:, 3], p2[:, 40] = 0.125, -0.125   # amax an exact power of two, from either sign
        out.append(Case("amax_pow2_" + fmt, p2, fmt, 1, 3))
        # every magnitude, every tie, the band and the values that round to zero, at every
        # block exponent and either sign: a row per exponent, a block per pattern
        rowsv = []
        for k, sgn in zip(EXPONENTS, (1.0, -1.0, 1.0, -1.0, 1.0)):
            rowsv.append(np.concatenate([np.ldexp(rng.permutation(p) * np.float32(sgn), k).astype(np.float32)
                                         for p in _patterns(fmt)]))
        ties = np.stack(rowsv)
        alt = ties.copy()
        alt[:, 1::2] *= -1   # mixed signs inside a block
        out.append(Case("ties_sat_" + fmt, ties, fmt, 1, 0))
        out.append(Case("ties_sat_mixed_inplace_" + fmt, alt, fmt, 1, 1, "inplace"))
        out.append(Case("ties_sat_nodst_" + fmt, alt.copy(), fmt, 1, 0, "nodst", code_offset=2))
        out.append(Case("ties_sat_nocodes_" + fmt, ties.copy(), fmt, 1, 3, "nocodes"))
        out.append(Case("ties_sat_flipped_" + fmt, -ties, fmt, 1, 0, code_offset=1))
        # negative values that round to zero keep their sign: -0 codes
        nz = np.full((2, 32), -1e-4, np.float32)
        nz[:, 7] = 5.0
        out.append(Case("neg_to_zero_" + fmt, nz, fmt, 1, 0))
        # 2^-100 and 2^+120 in neighbouring blocks of one row (and a partial third block)
        ext = np.empty((2, 75), np.float32)
        u = (rng.uniform(0.25, 1.0, ext.shape) * rng.choice([-1.0, 1.0], ext.shape))
        ext[:, :32] = np.ldexp(u[:, :32], -98)
        ext[:, 32:64] = np.ldexp(u[:, 32:64], 120)
        ext[:, 64:] = np.ldexp(u[:, 64:], -97)
        ext[0, 0] = np.ldexp(1.0, -100)
        out.append(Case("extremes_" + fmt, ext, fmt, 1, 0))
        out.append(Case("extremes_inplace_" + fmt, ext.copy(), fmt, 25, 3, "inplace", code_offset=2))
    return out


@lru_cache(maxsize=1)
def all_cases():
    """Every case, solved once per process (the tests share it and leave it unchanged)."""
    cases = _grid() + _aligned() + _khw() + _hand_made()
    for c in cases:
        c.x.setflags(write=False)
        c.ref = statement(c.x, c.fmt)
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)
