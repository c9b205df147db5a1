"""The MX block-scaled quantizer (dfq_mx_quantize_batch) restated in numpy, and the
cases the tests run: tests/test_mx_host.py checks the statement's own preconditions
without a GPU, tests/test_gpu_mx.py runs the cases.

Statement (include/dfq_hip.h): rows are cut into blocks of 32
elements (a last partial block padded with +0); per block amax = max |x_i|,
X = -127 if amax == 0 else clamp(floor(log2 amax) - emax, -127, 127), the scale byte
is X + 127; v_i = |x_i| * 2^-X as a real number (float64 here: a 24-bit significand
times a power of two is exact) is rounded to the nearest magnitude of an explicit
table, ties to the even code, saturating at the table's last entry; the code is
x_i's sign bit above the table index; y_i = +-q_i * 2^X.
"""
from dataclasses import dataclass, field
from functools import lru_cache
from typing import Optional, Tuple

import numpy as np

BLOCK = 32
FP4_MAGS = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
# E4M3 "fn": bias 7, subnormals m * 2^-9, normals (8 + m) * 2^(e - 10); code 0x7F is NaN and not in the table
FP8_MAGS = np.array([(c & 7) * 2.0 ** -9 if (c >> 3) == 0 else (8 + (c & 7)) * 2.0 ** ((c >> 3) - 10)
                     for c in range(127)])
assert FP8_MAGS[-1] == 448.0 and FP8_MAGS[1] == 2.0 ** -9 and FP8_MAGS[8] == 2.0 ** -6
assert (np.diff(FP4_MAGS) > 0).all() and (np.diff(FP8_MAGS) > 0).all()
#: fmt -> (table, emax, sign bit, code bytes per block)
FORMATS = {"mxfp4": (FP4_MAGS, 2, 0x8, 16), "mxfp8": (FP8_MAGS, 8, 0x80, 32)}

ROWS = [1, 3, 65]
ROW_LENS = [1, 9, 27, 31, 32, 33, 64, 100, 288, 1000, 4097]
OFFSETS = [0, 1, 3]     # floats from a 16-B boundary
KHWS = [1, 9, 49]
OUTPUTS = ["all", "inplace", "nodst", "nocodes"]
MIN_MAG = 2.0 ** -100   # the contract domain: non-zero magnitudes are at least this


def blocks(row_len: int) -> int:
    return -(-row_len // BLOCK)


def shared_exponent(amax: np.ndarray, emax: int) -> np.ndarray:
    """X per block from the blocks' float32 amax."""
    _, e = np.frexp(amax.astype(np.float64))   # amax = m * 2^e, 0.5 <= m < 1: floor(log2 amax) = e - 1
    return np.where(amax == 0, -127, np.clip(e - 1 - emax, -127, 127)).astype(np.int64)


def round_to_table(v: np.ndarray, mags: np.ndarray):
    """Index of the nearest table entry, ties to the even index, saturating; and which
    elements were exact ties (rounded down / up) or beyond the last entry."""
    hi = np.clip(np.searchsorted(mags, v, side="left"), 1, len(mags) - 1)
    lo = hi - 1
    dlo, dhi = v - mags[lo], mags[hi] - v
    tie = (dlo == dhi)
    idx = np.where(dlo < dhi, lo, hi)
    idx = np.where(tie, np.where(lo % 2 == 0, lo, hi), idx)
    sat = v > mags[-1]
    idx = np.where(sat, len(mags) - 1, idx)
    return idx, tie & (idx == lo), tie & (idx == hi), sat


def statement(x: np.ndarray, fmt: str, fp32_multiply: bool = False) -> dict:
    """The contract for x (float32 [rows, row_len]).  ``fp32_multiply``: v formed as
    one float32 multiply instead of exactly."""
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
    y64 = np.ldexp(mags[idx], X[:, :, None])
    y = np.copysign(y64, np.where(neg, -1.0, 1.0)).astype(np.float32)
    assert (y.astype(np.float64) == np.copysign(y64, np.where(neg, -1.0, 1.0))).all()   # step 7: exact in fp32
    if fmt == "mxfp4":
        codes = (code[:, :, 0::2] | (code[:, :, 1::2] << 4)).astype(np.uint8)
    else:
        codes = code
    assert codes.shape == (rows, nb, cbytes)
    return {"codes": codes, "scales": (X + 127).astype(np.uint8), "y": y.reshape(rows, nb * BLOCK)[:, :row_len].copy(),
            "element_codes": code, "v": v, "tie_down": tie_down, "tie_up": tie_up, "saturated": sat}


@dataclass
class Case:
    name: str
    x: np.ndarray            # float32 [rows, row_len]
    fmt: str
    khw: int = 1
    offset: int = 0
    outputs: str = "all"     # all | inplace (dst is src) | nodst (codes, scales, esum) | nocodes (dst, esum)
    ref: Optional[dict] = field(default=None, repr=False)

    @property
    def want_esum(self) -> bool:
        return self.x.shape[1] % self.khw == 0

    @property
    def want_dst(self) -> bool:
        return self.outputs != "nodst"

    @property
    def want_codes(self) -> bool:
        return self.outputs != "nocodes"


def outlier_data(seed: int, shape: Tuple[int, int]) -> np.ndarray:
    """Gaussian x 0.05 with 1 % of the elements x 6 (tests/clip_search_cases.py)."""
    rng = np.random.default_rng(seed)
    x = (0.05 * rng.standard_normal(shape)).astype(np.float32)
    x[rng.random(shape) < 0.01] *= np.float32(6.0)
    return x


def _grid():
    """Every rows x row_len shape in both formats.  One of the two takes khw 1 (error
    sums for every element), the other khw 9 where it divides the row and 49 (no
    error sums: it divides none of these rows) otherwise; offsets and output sets
    walk their lists."""
    out, i = [], 0
    for ri, rows in enumerate(ROWS):
        for li, row_len in enumerate(ROW_LENS):
            for fi in range(2):
                fmt = ("mxfp4", "mxfp8")[(ri + li + fi) % 2]
                khw = 1 if fi == 0 else (9 if row_len % 9 == 0 else 49)
                out.append(Case("grid_%dx%d_%s" % (rows, row_len, fmt), outlier_data(7000 + i, (rows, row_len)), fmt,
                                khw, OFFSETS[(ri + 2 * li + fi) % 3], OUTPUTS[(i // 2 + i // 8 + fi) % 4]))
                i += 1
    for fmt in FORMATS:   # every axis value meets both formats
        mine = [c for c in out if c.fmt == fmt]
        assert {c.offset for c in mine} == set(OFFSETS) and {c.outputs for c in mine} == set(OUTPUTS), fmt
        assert {c.khw for c in mine} == set(KHWS) and {c.x.shape[1] for c in mine if c.khw == 9} == {9, 27, 288}, fmt
    return out


def _khw():
    """Rows that khw 49 and 9 divide, short and long enough to be cut into pieces
    (whole khw groups per piece), aligned and not."""
    out, i = [], 0
    for fmt in FORMATS:
        for rows, row_len, khw in ((3, 49, 49), (2, 98, 49), (2, 3136, 49), (1, 4704, 49), (2, 4608, 9),
                                   (3, 2304, 9), (1, 6 * 25 * 32 + 25, 25), (5, 180, 9), (2, 4100, 4)):
            out.append(Case("khw%d_%dx%d_%s" % (khw, rows, row_len, fmt), outlier_data(7500 + i, (rows, row_len)),
                            fmt, khw, OFFSETS[i % 3], OUTPUTS[(i // 3) % 2]))
            i += 1
    return out


def _pattern(fmt: str) -> np.ndarray:
    """One block's worth of v values: every table entry, every midpoint between
    neighbours (the exact ties), values inside the saturating band, and values that
    round to zero; the block's largest is in [2^emax, 2^(emax+1)), so X = 0."""
    mags = FORMATS[fmt][0]
    mids = (mags[:-1] + mags[1:]) / 2
    if fmt == "mxfp4":
        v = np.concatenate([mags, mids, [6.5, 7.0, 7.5, 0.125, 0.1875]])
    else:   # a spread of the 126 midpoints, the ends of the table, the band (448, 512)
        v = np.concatenate([mags[[0, 1, 2, 7, 8, 9, 63, 64, 119, 120, 125, 126]], mids[[0, 1, 2, 7, 8, 60, 119, 124, 125]],
                            [464.0, 480.0, 500.0, 2.0 ** -11, 2.0 ** -10 * 0.75]])
    assert len(v) <= BLOCK and (v.astype(np.float32) == v).all()
    return v.astype(np.float32)


def _hand_made():
    out = []
    rng = np.random.default_rng(7900)
    for fmt, (mags, emax, _, _) in FORMATS.items():
        top = {"mxfp4": 7.5, "mxfp8": 480.0}[fmt]   # amax inside the saturating band
        z = np.zeros((2, 40), np.float32)
        out.append(Case("zeros_" + fmt, z.copy(), fmt, 1, 0))
        out.append(Case("negzeros_" + fmt, -z, fmt, 1, 1))
        one = np.zeros((3, 70), np.float32)
        one[0, 5], one[1, 33], one[2, 69] = 0.3, -1.7e-3, 12345.0
        out.append(Case("one_nonzero_" + fmt, one, fmt, 1, 0))
        p2 = outlier_data(7901, (4, 64))
        p2 = np.clip(p2, -0.125, 0.125)
        p2[:, 3], p2[:, 40] = 0.125, -0.125   # amax an exact power of two, from either sign
        out.append(Case("amax_pow2_" + fmt, p2, fmt, 1, 3))
        # ties, the saturating band and values that round to zero at several block exponents,
        # each sign; a row holds three blocks at different exponents
        pat = _pattern(fmt)
        rowsv = []
        for k, sgn in ((0, 1.0), (-7, -1.0), (5, 1.0), (-60, -1.0), (90, 1.0), (-3, 1.0)):
            b = np.zeros(BLOCK, np.float32)
            b[:len(pat)] = pat
            b[len(pat):] = top if len(pat) < BLOCK else 0
            b = rng.permutation(b)
            if not (b >= 2.0 ** emax).any():
                b[0] = top
            rowsv.append(np.ldexp(b * np.float32(sgn), k).astype(np.float32))
        ties = np.stack([np.concatenate(rowsv[:3]), np.concatenate(rowsv[3:])])
        alt = ties.copy()
        alt[:, 1::2] *= -1   # mixed signs inside a block
        out.append(Case("ties_sat_" + fmt, ties, fmt, 1, 0))
        out.append(Case("ties_sat_mixed_inplace_" + fmt, alt, fmt, 1, 1, "inplace"))
        out.append(Case("ties_sat_nodst_" + fmt, alt.copy(), fmt, 1, 0, "nodst"))
        out.append(Case("ties_sat_nocodes_" + fmt, ties.copy(), fmt, 1, 3, "nocodes"))
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
        out.append(Case("extremes_inplace_" + fmt, ext.copy(), fmt, 25, 3, "inplace"))
    return out


def mobilenetv2_shapes():
    """(rows, row_len, khw) of MobileNetV2's 53 quantized layers (torchvision layout)."""
    out = [(32, 27, 9)]
    cin = 32
    for t, c, n, s in ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2),
                       (6, 320, 1, 1)):
        for _ in range(n):
            hid = cin * t
            if t != 1:
                out.append((hid, cin, 1))
            out.append((hid, 9, 9))
            out.append((c, hid, 1))
            cin = c
    out += [(1280, 320, 1), (1000, 1280, 1)]
    assert len(out) == 53
    return out


@lru_cache(maxsize=1)
def all_cases():
    """Every case, solved once per process (the tests share it and leave it unchanged)."""
    cases = _grid() + _khw() + _hand_made()
    for c in cases:
        c.x.setflags(write=False)
        c.ref = statement(c.x, c.fmt)
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


def esum_reference(c: Case) -> np.ndarray:
    """torch.sum(e.view(O, I, khw), -1) on the CPU, e = fl32(y - x)."""
    import torch
    e = torch.from_numpy(c.ref["y"] - c.x)
    assert e.dtype == torch.float32
    return torch.sum(e.view(c.x.shape[0], -1, c.khw), -1).reshape(-1).numpy()
