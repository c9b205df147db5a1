"""The MX quantizer's scale search (dfq_mx_quantize_search_batch) restated in numpy for
the four element formats, and the cases its tests run: tests/test_mx_search_host.py
checks the statement and the case set without a GPU, tests/test_gpu_mx_search.py runs
the cases.

Statement (include/dfq_hip.h).  Everything of tests/mx_cases.py's contract
stays -- blocks of 32, +0 padding, the tables, nearest magnitude with ties to the even
code, saturation, the sign bit, the code layouts -- except the block's exponent X.  For a
block with amax != 0 let X0 = clamp(floor(log2 amax) - emax, -127, 127) (the floor rule),
X1 = X0 + 1, y0 / y1 the contract's values under X0 / X1 and
    N_d = sum_i (fl32(y_i^d - x_i) * 2^-X0)^2
The block takes X1 iff N_1 < N_0, strictly, else X0; an all-zero block keeps X = -127.
The device forms N_d in fp32 in an order of its own, which is within 33 * 2^-24 < 2^-19
relative of the real sum, so the sign of N_1 - N_0 is certain wherever the two differ by
more than 2^-18 of the larger.  Here N_d is float64, and a block is
  termwise_equal  when y0 and y1 are the same bits element for element: it keeps X0
                  (both sums run through one instruction sequence: they tie);
  undecided       when it is not termwise equal and |N_0 - N_1| <= 2^-16 max(N_0, N_1)
                  (4x the derived margin): either candidate is a correct answer, but
                  wholly one of them -- codes, scale byte, y and error sums.
The tables and round_to_table are those of mx_cases / mx6_cases, imported and left alone.
"""
from dataclasses import dataclass, field
from functools import lru_cache
from typing import Optional

import numpy as np

from tests import mx6_cases as M6
from tests import mx_cases as MC
from tests.mx_cases import BLOCK, blocks, outlier_data, round_to_table, shared_exponent

#: fmt -> (table, emax, sign bit, code bytes per block)
FORMATS = {**MC.FORMATS, **M6.FORMATS}
#: the saturating band (max, 2^(emax+1)) of v = amax * 2^-X0
BAND = {fmt: (float(mags[-1]), 2.0 ** (emax + 1)) for fmt, (mags, emax, _, _) in FORMATS.items()}
UNDECIDED_REL = 2.0 ** -16
UNDECIDED_CAP = 0.01   # of all blocks of the case set: the set is not valid above it


def pack(code: np.ndarray, fmt: str) -> np.ndarray:
    """[rows, nb, 32] element codes -> the format's ``codes`` layout."""
    if fmt == "mxfp4":
        return (code[:, :, 0::2] | (code[:, :, 1::2] << 4)).astype(np.uint8)
    if fmt == "mxfp8":
        return code
    return M6.pack6(code)


def candidate(xb: np.ndarray, X: np.ndarray, fmt: str) -> dict:
    """The contract's outputs for blocks xb (float32 [rows, nb, 32]) under the given
    exponents X (int [rows, nb]): element codes, packed codes, scale bytes, y."""
    mags, _, sign_bit, cbytes = FORMATS[fmt]
    v = np.ldexp(np.abs(xb).astype(np.float64), -X[:, :, None])   # exact: 24 bits times a power of two
    idx, _, _, sat = round_to_table(v, mags)
    neg = np.signbit(xb)
    code = (idx | np.where(neg, sign_bit, 0)).astype(np.uint8)
    y64 = np.copysign(np.ldexp(mags[idx], X[:, :, None]), np.where(neg, -1.0, 1.0))
    y = y64.astype(np.float32)
    assert (y.astype(np.float64) == y64).all()   # exact in fp32
    codes = pack(code, fmt)
    assert codes.shape == xb.shape[:2] + (cbytes,)
    return {"element_codes": code, "codes": codes, "scales": (X + 127).astype(np.uint8), "yb": y, "saturated": sat}


def noise(xb: np.ndarray, yb: np.ndarray, X0: np.ndarray) -> np.ndarray:
    """N = sum ((fl32(y - x)) * 2^-X0)^2 per block, float64."""
    e = yb - xb
    assert e.dtype == np.float32
    t = np.ldexp(e.astype(np.float64), -X0[:, :, None])
    return (t * t).sum(axis=2)


def statement(x: np.ndarray, fmt: str, search: bool = True) -> dict:
    """The searched contract for x (float32 [rows, row_len]).  ``cand``: both candidates
    (candidate()'s dicts, with ``y`` cut to the rows); ``N``: their float64 noises;
    ``termwise_equal``, ``undecided``, ``take1`` per block; ``codes`` / ``scales`` / ``y``:
    the result with the statement's own choice.  ``search=False``: the floor rule (X0)."""
    _, emax, _, _ = FORMATS[fmt]
    assert x.dtype == np.float32 and x.ndim == 2
    rows, row_len = x.shape
    nb = blocks(row_len)
    xp = np.zeros((rows, nb * BLOCK), np.float32)
    xp[:, :row_len] = x
    xb = xp.reshape(rows, nb, BLOCK)
    amax = np.abs(xb).max(axis=2)
    X0 = shared_exponent(amax, emax)
    X1 = X0 + 1
    assert (X1 <= 127).all()
    cand = [candidate(xb, X0, fmt), candidate(xb, X1, fmt)]
    N = [noise(xb, c["yb"], X0) for c in cand]
    termwise = (cand[0]["yb"].view(np.uint32) == cand[1]["yb"].view(np.uint32)).all(axis=2)
    assert termwise[amax == 0].all()
    undecided = ~termwise & (np.abs(N[0] - N[1]) <= UNDECIDED_REL * np.maximum(N[0], N[1]))
    take1 = ~termwise & (N[1] < N[0])
    if not search:
        take1 = np.zeros_like(take1)
    for c in cand:
        c["y"] = c["yb"].reshape(rows, nb * BLOCK)[:, :row_len].copy()
    pick = lambda k, sel: np.where(sel, cand[1][k], cand[0][k])   # noqa: E731
    return {"cand": cand, "N": N, "termwise_equal": termwise, "undecided": undecided, "take1": take1,
            "codes": pick("codes", take1[:, :, None]), "scales": pick("scales", take1),
            "y": pick("yb", take1[:, :, None]).reshape(rows, nb * BLOCK)[:, :row_len].copy(), "xb": xb, "X0": X0}


def sqnr_db(x: np.ndarray, y: np.ndarray) -> float:
    x, y = x.astype(np.float64), y.astype(np.float64)
    return float(10.0 * np.log10((x * x).sum() / ((y - x) ** 2).sum()))


@dataclass
class Case:
    name: str
    x: np.ndarray            # float32 [rows, row_len]
    fmt: str
    khw: int = 1
    offset: int = 0          # source: floats from a 16-B boundary
    outputs: str = "all"     # all | inplace | nodst | nocodes (mx_cases.Case)
    code_offset: int = 0     # FP6 codes: bytes from a 4-B boundary
    expect: Optional[str] = None   # hand-made: "x1" / "x0" every non-zero block, "termwise" every block
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


def requant_block(fmt: str = "mxfp8") -> np.ndarray:
    """One E4M3 block whose searched values do not survive the floor rule: 480 * 2^k
    elements (inside the band (448, 512): X0 clamps them to 448, X1 holds them exactly as
    1.875 * 2^8) over small exact neighbours.  The searched y has amax 480 * 2^k, which the
    floor rule puts back under X0 and saturates."""
    assert fmt == "mxfp8"
    b = np.zeros(BLOCK, np.float32)
    b[[0, 9, 17, 30]] = [480.0, -480.0, 480.0, 480.0]
    b[1:9] = [1.0, -2.0, 3.0, 4.0, -6.0, 8.0, 12.0, 16.0]   # on the grid under both exponents
    b[10:17] = [464.0, -470.0, 475.0, 20.0, 24.0, -40.0, 96.0]
    return b


def _hand_made():
    out = []
    for fi, (fmt, (mags, emax, _, _)) in enumerate(FORMATS.items()):
        rng = np.random.default_rng(9900 + fi)
        lo, hi = BAND[fmt]
        # every element inside the saturating band, at several exponents, either sign: X1
        band = rng.uniform(lo + (hi - lo) / 16, hi - (hi - lo) / 16, (3, 100)).astype(np.float32)
        band[:, ::16] = hi - (hi - lo) / 8   # every block, the partial one too, holds one the clamp costs
        band *= rng.choice(np.float32([-1.0, 1.0]), band.shape)
        band = np.ldexp(band, np.array([[0], [-9], [40]])).astype(np.float32)
        out.append(Case("band_" + fmt, band, fmt, 1, 0, expect="x1"))
        out.append(Case("band_unaligned_inplace_" + fmt, band.copy(), fmt, 1, 1, "inplace", code_offset=1, expect="x1"))
        # amax an exact power of two over small neighbours: X0.  Small: inside the subnormal binade
        # under X0, where X1's grid is twice as coarse (a normal element of a floating-point grid
        # rounds to the same value under both, and would leave the block's two noises a hair apart)
        sub = emax - {"mxfp4": 0, "mxfp8": -6, "mxfp6_e2m3": 0, "mxfp6_e3m2": -2}[fmt]   # emax - emin
        p2 = np.exp2(-rng.uniform(sub + 0.5, sub + 3.0, (4, 96))) * rng.choice([-1.0, 1.0], (4, 96))
        p2 = np.ldexp(p2, np.array([[0], [-5], [3], [-20]])).astype(np.float32)
        for r, k in enumerate((0, -5, 3, -20)):
            p2[r, 3::32] = np.ldexp(np.float32(1.0 if r % 2 == 0 else -1.0), k)
        out.append(Case("amax_pow2_" + fmt, p2, fmt, 1, 3, expect="x0"))
        # a single non-zero element per block that both grids hold (1 or 1.5 times a power of two)
        one = np.zeros((3, 70), np.float32)
        one[0, 5], one[0, 40], one[1, 33], one[2, 69], one[2, 0] = 0.25, -1.5, -2.0 ** -20, 3.0 * 2.0 ** 30, 1.0
        out.append(Case("one_nonzero_" + fmt, one, fmt, 1, 0, expect="termwise"))
        z = np.zeros((2, 40), np.float32)
        out.append(Case("zeros_" + fmt, z.copy(), fmt, 1, 0, expect="termwise"))
        out.append(Case("negzeros_" + fmt, -z, fmt, 1, 1, code_offset=2, expect="termwise"))
        # 2^-100 and 2^+120 in neighbouring blocks of one row (and a partial third block)
        ext = np.empty((2, 75), np.float32)
        u = (rng.uniform(0.25, 1.0, ext.shape) * rng.choice([-1.0, 1.0], ext.shape))
        ext[:, :32] = np.ldexp(u[:, :32], -98)
        ext[:, 32:64] = np.ldexp(u[:, 32:64], 120)
        ext[:, 64:] = np.ldexp(u[:, 64:], -97)
        ext[0, 0] = np.ldexp(1.0, -100)
        out.append(Case("extremes_" + fmt, ext, fmt, 1, 0))
        out.append(Case("extremes_inplace_" + fmt, ext.copy(), fmt, 25, 3, "inplace", code_offset=2))
    # the re-quantization case: 1.875-mantissa E4M3 values at several exponents, in a [3, 96] tensor
    b = requant_block()
    rq = np.stack([np.concatenate([np.ldexp(b * np.float32(s), k) for k, s in ks]).astype(np.float32)
                   for ks in (((0, 1), (-12, -1), (7, 1)), ((-30, 1), (3, -1), (0, -1)), ((20, 1), (-3, 1), (-7, -1)))])
    out.append(Case("requant_mxfp8", rq, "mxfp8", 1, 0, expect="x1"))
    return out


def _inherited():
    """The data, shapes, khw, alignment and output sets of mx_cases and mx6_cases."""
    out = []
    for c in MC.all_cases():
        out.append(Case("mx_" + c.name, c.x, c.fmt, c.khw, c.offset, c.outputs))
    for c in M6.all_cases():
        out.append(Case("mx6_" + c.name, c.x, c.fmt, c.khw, c.offset, c.outputs, code_offset=c.code_offset))
    return out


@lru_cache(maxsize=1)
def all_cases():
    """Every case, solved once per process (the tests share it and leave it unchanged)."""
    cases = _inherited() + _hand_made()
    for c in cases:
        c.x.setflags(write=False)
        c.ref = statement(c.x, c.fmt)
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


def esum_of(c: Case, y: np.ndarray) -> np.ndarray:
    """torch.sum(e.view(O, I, khw), -1) on the CPU, e = fl32(y - x) (mx_cases.esum_reference's rule)
    for the y given -- the one the device chose."""
    import torch
    e = torch.from_numpy(y - c.x)
    assert e.dtype == torch.float32
    return torch.sum(e.view(c.x.shape[0], -1, c.khw), -1).reshape(-1).numpy()
