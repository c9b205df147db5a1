"""The bias-correction cases at the kernels' reduction edges: shapes, seeds and a
deterministic input builder.  tests/golden/make_golden.py (section ``bc_edge``)
runs the reference's own functions on them into tests/golden/bc_edge_cases.npz;
tests/test_oracle_golden.py holds the CPU oracle to that file and
tests/test_gpu_bc_edges.py the HIP kernels.

Inputs are exact fp32 values built from integer draws: a 24-bit signed integer
times a drawn power of two (numpy PCG64, whose integer streams do not change
between numpy versions).  The exponents spread over several binades, so the
fp32 sums round at almost every add and any change of the summation order
changes bits.

What the fixture stores per case (flat arrays, cut by the case lists here):
  APPLY      bias_out [o]; for the one case whose result depends on the thread
             count (ApplyCase.threaded) the rows of THREADS instead
  PROPAGATE  fb_out [F]; for cases of >= PAR_NUMEL elements (where ATen splits
             the reduction by thread) the rows of THREADS instead
  EXPECT     the expectation vector of each term list
plus a digest of every case's inputs, so a drifting builder is told from a
drifting result.
"""
from dataclasses import dataclass
from functools import lru_cache
from typing import Tuple

import numpy as np

THREADS = (1, 8, 16)
PAR_NUMEL = 32768        # at::internal::GRAIN_SIZE: reductions below it run serially

# limits of csrc/dfq_bc.hip (dfq_transform_plan.h) the cases straddle
K_BC_STAGE = 2048        # kBcStage: longest row / column the one-launch kernel stages
K_BC_MAX_EXPECT = 4096   # kBcMaxExpect
K_BC_MAX_TERMS = 8       # kBcMaxTerms
K_BC_SCRATCH = 1024      # kBcScratch: level-0 partials a wave's cascade keeps in LDS
K_GRID_CAP = 2048        # blocks of 4 waves: rows / columns past 4 * 2048 take a second trip


def values(seed: int, n: int, e_lo: int, e_hi: int) -> np.ndarray:
    """n exact fp32 values m * 2^e: m uniform in [-2^23, 2^23), e in [e_lo, e_hi)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    m = rng.integers(-(1 << 23), 1 << 23, n)
    e = rng.integers(e_lo, e_hi, n)
    x = np.ldexp(m.astype(np.float64), e)
    y = x.astype(np.float32)
    assert (y.astype(np.float64) == x).all()
    return y


@dataclass(frozen=True)
class ApplyCase:
    name: str
    o: int
    i2: int
    f: int
    seed: int

    @property
    def bcols(self) -> int:
        return self.i2 if (self.i2 == self.f or self.f == 1) else self.f

    @property
    def threaded(self) -> bool:
        """One output row of >= PAR_NUMEL values: TensorIterator reduces it in two
        passes split by thread (every other shape is split over its rows, which
        changes no row's order)."""
        return self.o == 1 and self.bcols >= PAR_NUMEL

    def inputs(self):
        """E [o, i2] (|E| < 2^-4), expect [f] (|.| < 2), bias [o] (|.| < 2^-11: below the
        row means, so the add keeps the mean's last bits and a mean one ulp off shows)."""
        return (values(self.seed, self.o * self.i2, -33, -27).reshape(self.o, self.i2),
                values(self.seed + 1, self.f, -28, -22), values(self.seed + 2, self.o, -40, -34))


@dataclass(frozen=True)
class PropCase:
    name: str
    R: int
    F: int
    seed: int

    @property
    def threaded(self) -> bool:
        return self.R * self.F >= PAR_NUMEL

    def inputs(self):
        """vec [R * F] (|.| < 2), fake_b [F] (|.| < 2^-11, below the column means)."""
        return values(self.seed, self.R * self.F, -28, -22), values(self.seed + 1, self.F, -40, -34)


APPLY_ROW_LENS = (2, 7, 8, 9, 15, 16, 31, 32, 33, 63, 64, 65, 255, 2047, 2048, 2049, 4097)


def _apply_cases():
    out = [ApplyCase(f"row{n}", 5, n, n, 1000 + 10 * k) for k, n in enumerate(APPLY_ROW_LENS)]
    for n in (16, K_BC_STAGE + 1):   # the three broadcast forms, fused and past kBcStage
        out.append(ApplyCase(f"bcast_same{n}", 5, n, n, 2000 + n))      # i2 == f
        out.append(ApplyCase(f"bcast_f1_{n}", 5, n, 1, 2100 + n))        # one expectation for every column
        out.append(ApplyCase(f"bcast_i1_{n}", 5, 1, n, 2200 + n))        # E [o, 1] (depthwise)
    out.append(ApplyCase("grid_stride_o8200", 4 * K_GRID_CAP + 8, 2, 2, 2300))
    # (a seed at which the reference's one-thread and 8-thread results differ: about
    # one seed in five rounds the two orders to the same mean)
    out.append(ApplyCase("one_row_70000", 1, 70000, 70000, 2420))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


PROP_F = (1, 2, 3, 4, 5, 7, 8, 31, 32, 33, 100, 341, 1000)
PROP_R = (1, 3, 15, 16, 17, 255, 256, 257, 2048, 2049, 4097)
PROP_MAX_NUMEL = 2_000_000


def _prop_cases():
    out, seed = [], 5000
    for F in PROP_F:
        for R in PROP_R:
            if R * F <= PROP_MAX_NUMEL:
                out.append(PropCase(f"R{R}_F{F}", R, F, seed))
            seed += 10
    named = [
        ("chunked_below", 327, 100),          # 32,700 elements: one thread takes every column
        ("chunked_at", 328, 100),             # 32,800: the columns are chunked by thread
        ("cascade_fits", 16 * K_BC_SCRATCH + 15, 2),     # 16399: R >> 4 == kBcScratch
        ("cascade_lane0", 16 * K_BC_SCRATCH + 16, 2),    # 16400: the cascade runs on lane 0
        ("row_sum_lane0", 4 * (16 * K_BC_SCRATCH + 16), 2),   # 65600: the same inside row_sum's 4 streams
        ("grid_stride_F8200", 2, 4 * K_GRID_CAP + 8),
    ]
    for name, R, F in named:
        out.append(PropCase(name, R, F, seed))
        seed += 10
    for R in (16, 100, 1000, 4099, 33000, 70000):   # one column: a contiguous reduction
        out.append(PropCase(f"onecol_R{R}", R, 1, seed))
        seed += 10
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


APPLY_CASES: Tuple[ApplyCase, ...] = _apply_cases()
PROP_CASES: Tuple[PropCase, ...] = _prop_cases()

# ---- EXPECT ---------------------------------------------------------------
EXPECT_N = K_BC_MAX_EXPECT + 1
#: term lists over the one (w, b) vector: (name, [(relu, rotation), ...]).  A
#: term's vector is the base vector rotated by ``rotation`` elements, so the sums
#: pair different elements.
EXPECT_CASES = (
    ("relu", ((True, 0),)),
    ("plain", ((False, 0),)),
    ("sum8", tuple((k % 3 != 1, 37 * k) for k in range(K_BC_MAX_TERMS))),
    ("sum9", tuple((k % 3 != 1, 37 * k) for k in range(K_BC_MAX_TERMS + 1))),
)


@lru_cache(maxsize=1)
def expect_inputs():
    """(w, b), EXPECT_N fp32 pairs: x = -b/w spread over [-40, 40] with a dense run
    through +-1 (where ndtr switches between erf and erfc: |x| / sqrt 2 around
    1 / sqrt 2), w of both signs and down to 1e-6 in magnitude, and b == 0."""
    n = EXPECT_N
    rng = np.random.Generator(np.random.PCG64(4242))
    x = np.empty(n)
    x[:1500] = np.linspace(-40.0, 40.0, 1500)
    x[1500:2300] = 1.0 + (np.arange(800) - 400) * 2.0 ** -22      # through +1 in fp32 steps
    x[2300:3100] = -1.0 + (np.arange(800) - 400) * 2.0 ** -22     # through -1
    x[3100:] = rng.integers(-(1 << 20), 1 << 20, n - 3100) * (40.0 / (1 << 20))
    mag = np.ldexp(rng.integers(1 << 22, 1 << 23, n).astype(np.float64), rng.integers(-43, -21, n))   # 1e-6 .. 4
    mag[:64] = np.ldexp(rng.integers(1 << 22, 1 << 23, 64).astype(np.float64), -42)                 # ~1e-6 .. 2e-6
    sign = np.where(rng.integers(0, 4, n) == 0, -1.0, 1.0)         # a quarter negative
    w = (mag * sign).astype(np.float32)
    b = (-(x * w.astype(np.float64))).astype(np.float32)
    b[3100:3164] = 0.0
    assert (w != 0).all() and np.abs(w).min() < 2e-6 and (w < 0).sum() > 500 and (b == 0).sum() >= 64
    w.setflags(write=False)
    b.setflags(write=False)
    return w, b


def expect_terms(case):
    """[(w, b, relu), ...] of an EXPECT case."""
    w, b = expect_inputs()
    return [(np.roll(w, rot), np.roll(b, rot), relu) for relu, rot in case[1]]
