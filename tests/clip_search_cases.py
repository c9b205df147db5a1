"""The clip-range search (dfq_clip_search_batch) restated on the CPU, and the cases
the tests run: tests/test_clip_search_host.py checks the statement's own
preconditions without a GPU, tests/test_gpu_clip_search.py runs the cases.

Statement (include/dfq_hip.h): for a unit with fp32 data range (mn, mx), candidate
k clamps to (a_k mn, a_k mx), a_k = (float)(1 - k (1 - min_frac) / (K - 1)), the
clamped unit is quantized by the C oracle (oracle.quantize in CHANNEL or TENSOR
mode: the sweep's arithmetic on the clamped array's own data range), and
noise_k = sum (double)e^2 with e = fl32(y - x) against the UNCLAMPED x -- every
term an exact double, summed by math.fsum (correctly rounded).  The choice is the
smallest noise, ties to the smallest k.
"""
import math
from dataclasses import dataclass, field
from functools import lru_cache
from typing import Optional, Tuple

import numpy as np

from data_free_quantization_amd import _lib
from oracle import oracle as O

P = _lib.DFQ_CLIP_PIECE_ELEMS

ROWS = [1, 3, 64, 65, 130]
ROW_LENS = [1, 7, 9, 27, 63, 64, 65, 1000, P - 1, P, P + 1, 2 * P + 5]
TENSOR_SHAPES = [(5, 9), (37, 300), (3, P + 1)]
BITS = [2, 4, 8, 16]
KMS = [(1, 0.5), (2, 0.0), (16, 0.5), (64, 0.9), (16, 1.0)]   # (candidates, min_frac)
OFFSETS = [0, 1, 3]   # floats into a 16-B aligned buffer
MODES = {"tensor_asym": _lib.DFQ_TENSOR_ASYM, "tensor_sym": _lib.DFQ_TENSOR_SYM,
         "channel_asym": _lib.DFQ_CHANNEL_ASYM, "channel_sym": _lib.DFQ_CHANNEL_SYM}
assert (O.TENSOR_ASYM, O.TENSOR_SYM, O.CHANNEL_ASYM, O.CHANNEL_SYM) == tuple(MODES.values())

GAP = 1e-12   # a non-tied unit's runner-up is more than this, relative, above its best


def alpha(k: int, K: int, min_frac: float) -> np.float32:
    if K <= 1:
        return np.float32(1.0)
    return np.float32(1.0 - k * (1.0 - float(np.float32(min_frac))) / (K - 1))


def units_view(x: np.ndarray, mode: int) -> np.ndarray:
    """[units, unit_len]: rows per channel, the whole tensor per tensor."""
    return x.reshape(x.shape[0], -1) if mode >= _lib.DFQ_CHANNEL_ASYM else x.reshape(1, -1)


def candidate_ranges(x: np.ndarray, mode: int, K: int, min_frac: float):
    """lo, hi: float32 [units, K] (fp32 multiplies of the unit's min and max)."""
    u = units_view(x, mode)
    a = np.array([alpha(k, K, min_frac) for k in range(K)], dtype=np.float32)
    lo = u.min(axis=1)[:, None] * a[None, :]
    hi = u.max(axis=1)[:, None] * a[None, :]
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    return lo, hi


def noise_table(x: np.ndarray, bits: int, mode: int, K: int, min_frac: float) -> np.ndarray:
    """noise [units, K], float64, each the correctly rounded sum."""
    u = units_view(x, mode)
    lo, hi = candidate_ranges(x, mode, K, min_frac)
    out = np.empty((u.shape[0], K))
    for k in range(K):
        c = np.minimum(np.maximum(u, lo[:, k:k + 1]), hi[:, k:k + 1])
        y = O.quantize(c.reshape(x.shape), bits, mode, rows=x.shape[0])["dq"].reshape(u.shape)
        e = y - u
        assert e.dtype == np.float32
        sq = e.astype(np.float64) ** 2   # exact
        for r in range(u.shape[0]):
            out[r, k] = math.fsum(sq[r].tolist())
    return out


@dataclass
class Case:
    name: str
    x: np.ndarray            # float32, shape [rows, row_len]
    bits: int
    mode: int
    K: int
    min_frac: float
    offset: int = 0
    # the choice is 0 by construction: every candidate is the same clamp (K = 1, min_frac = 1, zeros: equal
    # noise, the tie goes to the smallest k), or the unit is constant (its min-max range reproduces it)
    tied: bool = False
    outlier: bool = False    # seeded Gaussian x 0.05 with 1 % of the elements x 6
    # the statement, filled by solve()
    noise: Optional[np.ndarray] = field(default=None, repr=False)
    choice: Optional[np.ndarray] = field(default=None, repr=False)
    lo: Optional[np.ndarray] = field(default=None, repr=False)
    hi: Optional[np.ndarray] = field(default=None, repr=False)

    @property
    def per_channel(self) -> bool:
        return self.mode >= _lib.DFQ_CHANNEL_ASYM

    @property
    def symmetric(self) -> bool:
        return self.mode in (_lib.DFQ_TENSOR_SYM, _lib.DFQ_CHANNEL_SYM)

    @property
    def unit_len(self) -> int:
        return units_view(self.x, self.mode).shape[1]

    def clamped(self) -> np.ndarray:
        u = units_view(self.x, self.mode)
        return np.clip(u, self.lo[:, None], self.hi[:, None]).reshape(self.x.shape)


def solve(c: Case) -> Case:
    c.noise = noise_table(c.x, c.bits, c.mode, c.K, c.min_frac)
    c.choice = np.argmin(c.noise, axis=1).astype(np.int32)   # the first of equal minima
    lo, hi = candidate_ranges(c.x, c.mode, c.K, c.min_frac)
    idx = np.arange(lo.shape[0])
    c.lo, c.hi = lo[idx, c.choice], hi[idx, c.choice]
    return c


def outlier_data(seed: int, shape: Tuple[int, int]) -> np.ndarray:
    rng = np.random.default_rng(seed)
    x = (0.05 * rng.standard_normal(shape)).astype(np.float32)
    x[rng.random(shape) < 0.01] *= np.float32(6.0)
    return x


def _grid():
    """Every rows x row_len shape once, per channel; bits, (K, min_frac), offset
    and symmetry walk their lists so that each value meets whole-unit and split
    shapes (checked below)."""
    out = []
    for ri, rows in enumerate(ROWS):
        for li, row_len in enumerate(ROW_LENS):
            bits = BITS[(ri + li) % 4]
            K, mf = KMS[(2 * ri + li) % 5]
            off = OFFSETS[(ri + 2 * li) % 3]
            sym = (ri + li // 4) % 2
            mode = _lib.DFQ_CHANNEL_SYM if sym else _lib.DFQ_CHANNEL_ASYM
            out.append(Case("grid_%dx%d" % (rows, row_len), outlier_data(1000 + 12 * ri + li, (rows, row_len)), bits,
                            mode, K, mf, off, tied=(K == 1 or mf == 1.0 or row_len == 1), outlier=True))
    for what, pick in (("bits", lambda c: c.bits), ("km", lambda c: (c.K, c.min_frac)),
                       ("offset", lambda c: c.offset), ("mode", lambda c: c.mode)):
        for split in (False, True):
            seen = {pick(c) for c in out if (c.x.shape[1] > P) == split}
            want = {"bits": set(BITS), "km": set(KMS), "offset": set(OFFSETS),
                    "mode": {_lib.DFQ_CHANNEL_ASYM, _lib.DFQ_CHANNEL_SYM}}[what]
            assert seen == want, (what, split, seen)
    return out


def _tensor():
    out = []
    i = 0
    for shape in TENSOR_SHAPES:
        for mode in (_lib.DFQ_TENSOR_ASYM, _lib.DFQ_TENSOR_SYM):
            for bits in BITS:
                K, mf = KMS[i % 5]
                out.append(Case("tensor_%dx%d_m%d_b%d" % (*shape, mode, bits), outlier_data(2000 + i, shape), bits, mode,
                                K, mf, OFFSETS[i % 3], tied=(K == 1 or mf == 1.0), outlier=True))
                i += 1
    assert {(c.K, c.min_frac) for c in out} == set(KMS) and {c.offset for c in out} == set(OFFSETS)
    return out


def _four_bit():
    """INT4 with 16 candidates down to half the range, every mode: the rows of the
    issue's prototype on which clipping pays (long rows with outliers)."""
    out = []
    for i, (shape, mode) in enumerate([((64, 1000), "channel_asym"), ((65, 1000), "channel_sym"),
                                       ((3, 2 * P + 5), "channel_sym"), ((3, 2 * P + 1), "channel_asym"),
                                       ((37, 300), "tensor_asym"), ((3, P + 1), "tensor_sym"),
                                       ((130, 65), "channel_asym"), ((64, 288), "channel_sym")]):
        out.append(Case("int4_%dx%d_%s" % (*shape, mode), outlier_data(3000 + i, shape), 4, MODES[mode], 16, 0.5,
                        OFFSETS[i % 3], outlier=True))
    return out


def _special():
    """Constant rows, all-zero rows, single-element rows: the choice is 0 -- zeros
    tie on every candidate, and a constant unit is reproduced by its own min-max
    range (exactly when asymmetric, to rounding when symmetric) while every
    narrower clamp moves it by (1 - a_k) |x|."""
    out = []
    rng = np.random.default_rng(4000)
    const = np.repeat(rng.standard_normal((5, 1)).astype(np.float32), 33, axis=1)
    const[3] = np.float32(-0.375)
    single = rng.standard_normal((7, 1)).astype(np.float32)
    for bits in (4, 8):
        for name, mode in MODES.items():
            if mode >= _lib.DFQ_CHANNEL_ASYM:
                out.append(Case("const_%s_b%d" % (name, bits), const.copy(), bits, mode, 16, 0.5, 1, tied=True))
                out.append(Case("single_%s_b%d" % (name, bits), single.copy(), bits, mode, 16, 0.5, 3, tied=True))
            else:
                out.append(Case("const_%s_b%d" % (name, bits), const[:1].copy(), bits, mode, 16, 0.5, 1, tied=True))
                out.append(Case("single_%s_b%d" % (name, bits), single[:1].copy(), bits, mode, 16, 0.5, 3, tied=True))
            out.append(Case("zero_%s_b%d" % (name, bits), np.zeros((4, 40), np.float32), bits, mode, 16, 0.5, 0,
                            tied=True))
            out.append(Case("zero_long_%s_b%d" % (name, bits), np.zeros((1, P + 3), np.float32), bits, mode, 64, 0.9,
                            0, tied=True))
    return out


def check_preconditions(cases) -> dict:
    """What the GPU assertions rest on, checked on the CPU statement itself."""
    narrowed = units = 0
    last = []
    min_gap = math.inf
    for c in cases:
        assert np.isfinite(c.noise).all(), c.name
        if c.tied:
            assert not c.choice.any(), c.name   # argmin takes the first of equal minima
            continue
        # exact zeros as a unit's extreme would leave the sign of (a_k * 0) to the reduction order
        u = units_view(c.x, c.mode)
        assert (u.min(axis=1) != 0).all() and (u.max(axis=1) != 0).all(), c.name
        srt = np.sort(c.noise, axis=1)
        best, second = srt[:, 0], srt[:, 1]
        assert (best > 0).all(), c.name
        gap = (second - best) / best
        assert (gap > GAP).all(), (c.name, float(gap.min()))
        min_gap = min(min_gap, float(gap.min()))
        if (c.choice == c.K - 1).any():
            last.append(c.name)
        if c.name.startswith("int4_"):
            n = int((c.choice > 0).sum())
            assert 2 * n >= c.choice.size, (c.name, n, c.choice.size)
            narrowed += n
            units += c.choice.size
    assert last, "no case chooses the last candidate"
    assert units and 2 * narrowed >= units
    return {"min_gap": min_gap, "last": last, "int4_narrowed": narrowed, "int4_units": units}


@lru_cache(maxsize=1)
def all_cases():
    """Every case, solved once per process (the tests share it and leave it unchanged)."""
    cases = [solve(c) for c in _grid() + _tensor() + _four_bit() + _special()]
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)
