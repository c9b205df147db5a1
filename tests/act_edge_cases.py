"""The activation-range cases at the edges of csrc/dfq_act.hip's three
set_quant_minmax kernels (dfq_act_moments, dfq_act_minmax, dfq_act_affine):
statistic builders, lengths, placements, affine shapes and tiny traced models.
tests/golden/make_golden.py (section ``act_edge``) runs the reference's own
set_quant_minmax on the models into tests/golden/act_edge_cases.npz;
tests/test_oracle_act_edges.py holds the CPU oracle to that file and
tests/test_gpu_act_edges.py the HIP kernels.  Pure numpy / torch: no GPU.

Statistics are exact fp32 values built from PCG64 integer draws (whose streams
do not change between numpy versions), as tests/bc_edge_cases.py builds its own.

The population (POP_N (w, b) pairs; w is a BN weight, so a quarter is negative
and set_quant_minmax sees |w|) by index:

  [   0,   64)  |w| ~ 1e-6 .. 2e-6
  [  64, 1064)  x0 = -b/w swept over [-40, 40]
  [1064, 1464)  x0 through +1 in fp32 steps (ndtr switches between erf and erfc)
  [1464, 1864)  x0 through -1
  [1864, 2264)  x6 = (6 - b)/w through +1
  [2264, 2664)  x6 through -1
  [2664, 2728)  b == 0
  [2728, 2792)  b == 6
  [2792, 2856)  b within 32 ulp of 6
  [2856, 3256)  "off" channels: x0 over [4.8, 5.8], |w| in [1, 8) -- where the
                reference's fp32 calculate_var cancels to -1e-6 .. -8e-5, below
                -eps, so its torch.sqrt(var + eps) is NaN (w = 1.61, b = -8.75 is one)
  [3256, 4097)  x0 drawn over [-40, 40]
"""
from dataclasses import dataclass
from functools import lru_cache
from typing import Optional, Tuple

import numpy as np

from tests.bc_edge_cases import values

EPS = 1e-6               # set_quant_minmax's eps (utils/layer_transform.py:415)
N_SIGMA = 6.0            # its default N
POP_N = 4097
K_THREADS = 256          # kThreads: act_minmax_kernel's single block
K_GRID_CAP = 2048        # blocks_for's cap: lengths past 2048 * 256 take a second grid-stride trip

#: lengths of the moments and minmax cases; the last (moments only) is the second
#: trip of the 2,048 x 256 grid-stride loop
LENGTHS = (1, 63, 64, 65, 255, 256, 257, 1031, 4097)
LEN_SECOND_TRIP = K_GRID_CAP * K_THREADS + 300
MOMENT_LENGTHS = LENGTHS + (LEN_SECOND_TRIP,)

_OFF = slice(2856, 3256)


def _mag(rng, n, e_lo, e_hi):
    """n exact values m * 2^e, m in [2^22, 2^23), e in [e_lo, e_hi)."""
    return np.ldexp(rng.integers(1 << 22, 1 << 23, n).astype(np.float64), rng.integers(e_lo, e_hi, n))


@lru_cache(maxsize=1)
def population():
    """(w, b): the POP_N fp32 pairs of the module docstring (read-only)."""
    n = POP_N
    rng = np.random.Generator(np.random.PCG64(777))
    mag = _mag(rng, n, -42, -19)                       # ~9.5e-7 .. 8
    mag[:64] = _mag(rng, 64, -42, -41)                 # ~1e-6 .. 2e-6
    mag[1864:2664] = _mag(rng, 800, -25, -19)          # 0.125 .. 8: 6 - b keeps x6's low bits
    mag[_OFF] = _mag(rng, 400, -22, -19)               # 1 .. 8
    sign = np.where(rng.integers(0, 4, n) == 0, -1.0, 1.0)   # a quarter negative
    w = (mag * sign).astype(np.float32)
    assert (w.astype(np.float64) == mag * sign).all()
    aw = np.abs(w).astype(np.float64)                  # fake_weight = |bn.weight|
    steps = (np.arange(400) - 200) * 2.0 ** -22
    x = rng.integers(-(1 << 20), 1 << 20, n) * (40.0 / (1 << 20))
    x[64:1064] = np.linspace(-40.0, 40.0, 1000)
    x[1064:1464] = 1.0 + steps
    x[1464:1864] = -1.0 + steps
    x[_OFF] = 4.8 + np.arange(400) * (1.0 / 400)
    b = (-(x * aw)).astype(np.float32)
    b[1864:2264] = (6.0 - (1.0 + steps) * aw[1864:2264]).astype(np.float32)
    b[2264:2664] = (6.0 - (-1.0 + steps) * aw[2264:2664]).astype(np.float32)
    b[2664:2728] = 0.0
    b[2728:2792] = 6.0
    k = np.arange(-32, 32)
    b[2792:2856] = (6.0 + np.where(k >= 0, k + 1, k) * 2.0 ** -21).astype(np.float32)   # ulp(6) = 2^-21
    assert np.abs(w).min() < 2e-6 and np.abs(w).max() > 4 and 800 < (w < 0).sum() < 1300
    assert (b == 0).sum() >= 64 and (b == 6).sum() == 64 and (np.abs(b[2792:2856] - 6) <= 32 * 2.0 ** -21).all()
    assert (b[2792:2856] != 6).all()
    w.setflags(write=False)
    b.setflags(write=False)
    return w, b


def stats(n: int, seed: int = 0, absolute: bool = False):
    """(w, b) of n channels: the population walked with a stride coprime to POP_N
    from an offset set by ``seed`` (every pair once up to POP_N, tiled beyond).
    ``absolute``: |w|, as merge_batchnorm stores fake_weight."""
    w, b = population()
    idx = (131 * seed + 1000 * np.arange(n, dtype=np.int64)) % POP_N
    ww = w[idx]
    return (np.abs(ww) if absolute else ww), b[idx]


def self_check():
    """The population holds what the cases rest on; needs the CPU oracle.  Returns
    the number of channels whose ReLU / ReLU6 variance is below -eps."""
    from oracle import oracle as O
    w, b = population()
    found = []
    for kind in (1, 2):
        _, var = O.act_moments(np.abs(w), b, kind)
        neg = int((var.astype(np.float64) + np.float32(EPS) < 0).sum())
        assert 3 <= neg < 0.05 * POP_N, (kind, neg)
        found.append(neg)
    return tuple(found)


# ---- dfq_act_minmax ---------------------------------------------------------
PLACE_N = 1031
#: the lane, wave and trip boundaries of the single 256-thread block
PLACEMENTS = (0, 63, 64, 255, 256, 1030)


def minmax_inputs(n: int, seed: int, w_is_var: bool):
    """(a, w) without a NaN: |a| < 16 over five binades; w >= 0 over five binades
    (a standard deviation), or as a variance: zeros and a few values between -eps
    and 0 as well, whose sqrt(w + eps) is still real."""
    a = values(seed, n, -24, -19)
    w = np.abs(values(seed + 1, n, -26, -21))
    if w_is_var:
        rng = np.random.Generator(np.random.PCG64(seed + 2))
        pick = rng.integers(0, 8, n)
        w = np.where(pick == 0, np.float32(0), np.where(pick == 1, np.float32(-5e-7), w)).astype(np.float32)
        assert (w.astype(np.float32) + np.float32(EPS) > 0).all()
    return a.copy(), w.copy()


def _big(w_is_var):
    return np.float32(2.0 ** 28 if w_is_var else 2.0 ** 14)   # sqrt(2^28 + eps) == 2^14 in fp32


@dataclass(frozen=True)
class MinMaxCase:
    name: str
    n: int
    seed: int
    what: str = "plain"          # plain | extreme | nan | nan_w | nan_var | inf_a | inf_w | inf_minus_inf
    at: int = 0

    def nan_both(self, w_is_var: bool) -> bool:
        """Some input element is (or becomes, through the square root) NaN: both
        outputs are NaN."""
        return self.what in ("nan", "nan_w") or (self.what == "nan_var" and w_is_var)

    def inputs(self, w_is_var: bool):
        a, w = minmax_inputs(self.n, self.seed, w_is_var)
        p = self.at
        if self.what == "extreme":      # both extremes in one element: 0.5 -+ 6 * 2^14
            a[p], w[p] = 0.5, _big(w_is_var)
        elif self.what == "nan":
            a[p] = np.nan
        elif self.what == "nan_w":
            w[p] = np.nan
        elif self.what == "nan_var":    # a variance below -eps: NaN only through the square root
            w[p] = -3e-6
        elif self.what == "inf_a":
            a[p], a[(p + 700) % self.n] = np.inf, -np.inf
        elif self.what == "inf_w":
            w[p] = np.inf
        elif self.what == "inf_minus_inf":   # a - N*w is NaN, a + N*w is +inf: torch.min is NaN, torch.max is not
            a[p], w[p] = np.inf, np.inf
        return a, w


def _minmax_cases():
    out = [MinMaxCase(f"len{n}", n, 300 + 10 * k) for k, n in enumerate(LENGTHS)]
    for p in PLACEMENTS:
        out.append(MinMaxCase(f"extreme_at{p}", PLACE_N, 500, "extreme", p))
    for p in PLACEMENTS:
        out.append(MinMaxCase(f"nan_at{p}", PLACE_N, 500, "nan", p))
    out += [MinMaxCase("nan_first_w", PLACE_N, 510, "nan_w", 0),
            MinMaxCase("nan_only", 1, 520, "nan", 0),
            MinMaxCase("nan_only_w", 1, 520, "nan_w", 0),
            MinMaxCase("nan_from_var", PLACE_N, 530, "nan_var", 777),
            MinMaxCase("nan_from_var_last", 257, 530, "nan_var", 256),
            MinMaxCase("inf_a", PLACE_N, 540, "inf_a", 5),
            MinMaxCase("inf_w", PLACE_N, 550, "inf_w", 300),
            MinMaxCase("inf_minus_inf", PLACE_N, 560, "inf_minus_inf", 9)]
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


MINMAX_CASES: Tuple[MinMaxCase, ...] = _minmax_cases()


# ---- dfq_act_affine ---------------------------------------------------------
@dataclass(frozen=True)
class AffineCase:
    name: str
    o: int
    i2: int
    khw: int
    groups: int
    seed: int
    bias: bool = True

    def inputs(self, form: str):
        """(x [groups * i2], W [o, i2, khw], bias [o] or None).  ``int``: integers of
        magnitude <= 8, so every partial sum in any order is exact in fp32;
        ``binade``: the multi-binade ``values`` (|W| < 0.5, |x| < 8, |bias| < 0.5)."""
        nx, nw = self.groups * self.i2, self.o * self.i2 * self.khw
        if form == "int":
            rng = np.random.Generator(np.random.PCG64(self.seed))
            x = rng.integers(-8, 9, nx).astype(np.float32)
            W = rng.integers(-8, 9, nw).astype(np.float32)
            bias = rng.integers(-8, 9, self.o).astype(np.float32)
            assert 8 * 8 * self.khw * self.i2 + 8 < 2 ** 24     # any order of any partial sum is exact
        else:
            assert form == "binade"
            x, W, bias = values(self.seed, nx, -26, -20), values(self.seed + 1, nw, -30, -24), \
                values(self.seed + 2, self.o, -30, -24)
        return x, W.reshape(self.o, self.i2, self.khw), (bias if self.bias else None)

    def exact(self, x, W, bias):
        """(out, abs): float64 out[o] = sum_i (sum_k W[o, i, k]) x[g, i] + bias[o] and
        abs[o] = sum |W| |x| + |bias|."""
        og = self.o // self.groups
        xg = x.astype(np.float64).reshape(self.groups, self.i2)[np.arange(self.o) // og]     # [o, i2]
        Wd = W.astype(np.float64)
        out = (Wd.sum(-1) * xg).sum(-1)
        ab = (np.abs(Wd).sum(-1) * np.abs(xg)).sum(-1)
        if bias is not None:
            out, ab = out + bias.astype(np.float64), ab + np.abs(bias.astype(np.float64))
        return out, ab

    @property
    def bound_ulps(self) -> int:
        """khw adds, a product, i2 adds in any order and the bias add."""
        return self.khw + self.i2 + 2


AFFINE_CASES: Tuple[AffineCase, ...] = (
    AffineCase("i2_1", 5, 1, 1, 1, 7000),
    AffineCase("i2_63", 5, 63, 1, 1, 7010),
    AffineCase("i2_64", 5, 64, 1, 1, 7020),
    AffineCase("i2_65_khw9", 5, 65, 9, 1, 7030),
    AffineCase("i2_130_khw49", 3, 130, 49, 1, 7040),           # third trip of the wave-stride loop
    AffineCase("khw9", 7, 9, 9, 1, 7050),                      # aten_inner_sum: one vector of 8 + a tail
    AffineCase("khw12", 7, 9, 12, 1, 7060),
    AffineCase("grouped", 8, 5, 9, 4, 7070),
    AffineCase("depthwise", 40, 1, 9, 40, 7080),
    AffineCase("o8200", 4 * K_GRID_CAP + 8, 2, 1, 1, 7090),    # past 2,048 blocks x 4 waves
    AffineCase("i2_65_khw9_nobias", 5, 65, 9, 1, 7030, bias=False),
)


# ---- tiny traced models -----------------------------------------------------
WIDTH = 1031
D_WIDTH, D_GROUPS = 1032, 8     # case (d.): 1,032 = 8 groups of 129 channels
#: the window of channels where every branch of a "nan" graph is almost always off
#: (or, without an activation, has |w| ~ 1e-6), so the summed variances go below -eps
_WINDOW = 96

#: name -> (branch activations, activation after the add); None: the case (d.) model
MODELS = {
    "r6_r__r6": (("relu6", "relu"), "relu6"),
    "r6_r6__r": (("relu6", "relu6"), "relu"),
    "n_r6__n": ((None, "relu6"), None),
    "r_n__n": (("relu", None), None),
    "r6_n_r__r6": (("relu6", None, "relu"), "relu6"),     # (a + b) + c: the accumulate path runs twice
    "case_d": None,
}
SETS = ("clean", "nan")
GRAPHS = tuple(f"{s}.{m}" for s in SETS for m in MODELS)


def bn_stats(stat_set: str, c: int, k: int, act: Optional[str]):
    """(weight, bias) of the k-th BatchNorm of a model of width c.

    clean: |w| in [0.25, 2), x0 in [-3, 3]: every variance is far above zero.
    nan:   the population from a per-BN offset; in the first _WINDOW channels the
           off channels (with an activation) or |w| ~ 1e-6 (without)."""
    if stat_set == "clean":
        rng = np.random.Generator(np.random.PCG64(9100 + k))
        mag = _mag(rng, c, -24, -21)
        sign = np.where(rng.integers(0, 4, c) == 0, -1.0, 1.0)
        x0 = rng.integers(-(1 << 20), 1 << 20, c) * (3.0 / (1 << 20))
        w = (mag * sign).astype(np.float32)
        return w, (-(x0 * mag)).astype(np.float32)
    assert stat_set == "nan"
    w, b = (v.copy() for v in stats(c, seed=k))
    pw, pb = population()
    # every BN takes the same off channels: the add's variance is a sum of copies
    pick = _OFF.start + (np.arange(_WINDOW) * 4 + 1) % 400
    if act is None:
        w[:_WINDOW], b[:_WINDOW] = pw[:64][np.arange(_WINDOW) % 64], pb[pick]
    else:
        w[:_WINDOW], b[:_WINDOW] = pw[pick], pb[pick]
    return w, b


def _conv1x1(c):
    import torch
    import torch.nn as nn
    conv = nn.Conv2d(c, c, 1, bias=False)
    with torch.no_grad():
        conv.weight.fill_(2.0 ** -10)       # the ranges do not depend on it
    return conv


def _act(kind):
    import torch.nn as nn
    return {"relu": nn.ReLU, "relu6": nn.ReLU6}[kind]()


def _set_bn(bn, w, b):
    import torch
    with torch.no_grad():               # running_mean / running_var stay 0 / 1
        bn.weight.copy_(torch.from_numpy(w))
        bn.bias.copy_(torch.from_numpy(b))


def build_model(graph_name: str):
    """The nn.Module of GRAPHS entry ``<set>.<model>`` with its statistics."""
    import torch
    import torch.nn as nn
    stat_set, mname = graph_name.split(".")
    spec = MODELS[mname]

    class AddNet(nn.Module):
        """stem conv-BN-ReLU; conv-BN-(act) branches, added; (act); the head conv."""

        def __init__(self, c, acts, after):
            super().__init__()
            self.stem, self.stem_bn, self.stem_act = _conv1x1(c), nn.BatchNorm2d(c), nn.ReLU()
            self.convs = nn.ModuleList([_conv1x1(c) for _ in acts])
            self.bns = nn.ModuleList([nn.BatchNorm2d(c) for _ in acts])
            self.acts = nn.ModuleDict({str(i): _act(a) for i, a in enumerate(acts) if a})
            self.after = _act(after) if after else None
            self.head = _conv1x1(c)

        def forward(self, x):
            x = self.stem_act(self.stem_bn(self.stem(x)))
            ys = []
            for i, (conv, bn) in enumerate(zip(self.convs, self.bns)):
                y = bn(conv(x))
                ys.append(self.acts[str(i)](y) if str(i) in self.acts else y)
            s = ys[0] + ys[1]
            for y in ys[2:]:
                s = s + y
            if self.after is not None:
                s = self.after(s)
            return self.head(s)

    class AffineNet(nn.Module):
        """stem conv-BN-ReLU; a grouped 3x3 conv with a bias and no BN; the head conv."""

        def __init__(self, c, groups):
            super().__init__()
            self.stem, self.stem_bn, self.stem_act = _conv1x1(c), nn.BatchNorm2d(c), nn.ReLU()
            self.mid = nn.Conv2d(c, c, 3, padding=1, groups=groups, bias=True)
            self.head = _conv1x1(c)

        def forward(self, x):
            return self.head(self.mid(self.stem_act(self.stem_bn(self.stem(x)))))

    if spec is None:
        m = AffineNet(D_WIDTH, D_GROUPS)
        _set_bn(m.stem_bn, *bn_stats(stat_set, D_WIDTH, 0, "relu"))
        with torch.no_grad():
            seed = 9300 + SETS.index(stat_set) * 10
            m.mid.weight.copy_(torch.from_numpy(values(seed, m.mid.weight.numel(), -30, -24)).view_as(m.mid.weight))
            m.mid.bias.copy_(torch.from_numpy(values(seed + 1, D_WIDTH, -30, -24)))
        return m
    acts, after = spec
    m = AddNet(WIDTH, acts, after)
    _set_bn(m.stem_bn, *bn_stats(stat_set, WIDTH, 0, "relu"))
    for i, a in enumerate(acts):
        _set_bn(m.bns[i], *bn_stats(stat_set, WIDTH, 1 + i, a))
    return m


def model_inputs(model):
    """Every BN weight and bias and, for case (d.), the grouped conv's weight and
    bias, flat: what the fixture's digest covers."""
    import torch.nn as nn
    parts = []
    for mod in model.modules():
        if isinstance(mod, nn.BatchNorm2d):
            parts += [mod.weight.detach().numpy().ravel(), mod.bias.detach().numpy().ravel()]
    if hasattr(model, "mid"):
        parts += [model.mid.weight.detach().numpy().ravel(), model.mid.bias.detach().numpy().ravel()]
    return np.concatenate(parts)


# kinds of a recorded vector (the fixture's ``kinds``)
REC_MIN, REC_MAX, REC_SQRT = 0, 1, 2


def case_d_exact(model, n_sigma: float = N_SIGMA):
    """The case (d.) quantizer of ``build_model("<set>.case_d")`` in float64: (lo,
    hi, tol).  The statistic vectors |bn.weight| and bn.bias go through the grouped
    conv (weights summed over KH*KW) with its bias; lo = min(B - N*W), hi = max(B +
    N*W).  tol bounds an fp32 evaluation's distance from either: per element the
    affine bound E = (khw + i2 + 2) 2^-24 (sum |W||x| + |bias|) of both vectors,
    E_B + N E_W, plus the product's and the add's roundings, 2 * 2^-24 of the
    magnitude; a min or max moves by at most the largest element error."""
    W = model.mid.weight.detach().numpy()
    o, i2 = W.shape[0], W.shape[1]
    case = AffineCase("case_d", o, i2, W.size // (o * i2), model.mid.groups, 0)
    Wr, bias = W.reshape(o, i2, -1), model.mid.bias.detach().numpy()
    fb, fw = model.stem_bn.bias.detach().numpy(), np.abs(model.stem_bn.weight.detach().numpy())
    u = 2.0 ** -24
    (B, aB), (Wv, aW) = case.exact(fb, Wr, bias), case.exact(fw, Wr, bias)
    err = case.bound_ulps * u * (aB + n_sigma * aW)
    tol = float((err + 2 * u * (np.abs(B) + n_sigma * np.abs(Wv) + err)).max())
    return float((B - n_sigma * Wv).min()), float((B + n_sigma * Wv).max()), tol
