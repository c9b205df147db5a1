"""Sum rounding's plain statement (include/dfq_hip.h, steps 2-6) in numpy -- float32
for the position, int64 from the perturbation on, np.lexsort for the orders -- and
the cases the host and GPU tests share.  The statement takes the grid (s, negmn) as
inputs: the GPU test feeds it the library's own scale and zero."""
from dataclasses import dataclass

import numpy as np

HALF, STEP = 1 << 23, 1 << 24
MODES = {"tensor_asym": 0, "tensor_sym": 1, "channel_asym": 2, "channel_sym": 3}
ROWS = (1, 3, 300)
GT = ((1, 1), (1, 9), (2, 4), (63, 9), (65, 1), (257, 9), (1000, 1), (3, 49), (16384, 1))
BITS = (2, 4, 8)
KINDS = ("normal", "dense", "tie", "constant", "clamp")


def grid(x, bits, mode):
    """make_qparams on the unit's data range (scale in double): s, negmn, mn, each [rows, 1]."""
    sym, per_channel = mode in (1, 3), mode >= 2
    mn = x.min(axis=1, keepdims=True) if per_channel else np.full((x.shape[0], 1), x.min(), np.float32)
    mx = x.max(axis=1, keepdims=True) if per_channel else np.full((x.shape[0], 1), x.max(), np.float32)
    mn64, mx64 = mn.astype(np.float64), mx.astype(np.float64)
    if sym:
        s = np.maximum(np.maximum(np.abs(mx64), np.abs(mn64)) / ((1 << (bits - 1)) - 1), 1e-8).astype(np.float32)
        return s, np.full_like(s, -0.0), np.zeros_like(s)
    s = np.maximum((mx64 - mn64) / ((1 << bits) - 1), 1e-8).astype(np.float32)
    return s, (-mn64).astype(np.float32), mn64.astype(np.float32)


def _rank(primary, index):
    """Position of every element of the last axis in the order (primary descending, index ascending)."""
    order = np.lexsort((np.broadcast_to(index, primary.shape), -primary), axis=-1)
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(primary.shape[-1]), primary.shape), axis=-1)
    return rank


def statement(x, s, negmn, mn, bits, sym, T):
    """x [rows, G*T] float32; s, negmn, mn [rows, 1] float32.  Returns a dict: q0 (nearest
    codes), q, dst, flips [rows, 2], P0 and P (perturbations before and after) as [rows, G, T]."""
    rows, n = x.shape
    G = n // T
    qmin, qmax = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if sym else (0, (1 << bits) - 1)
    t = np.clip(((x + negmn).astype(np.float32) / s).astype(np.float32), np.float32(qmin), np.float32(qmax))
    q0 = np.rint(t)
    P0 = np.rint(np.ldexp((q0 - t).astype(np.float32), 24)).astype(np.int64).reshape(rows, G, T)
    q0 = q0.astype(np.int64).reshape(rows, G, T)
    taps = np.arange(T)
    # kernel stage
    e = P0.sum(-1)
    k4 = (np.abs(e) + HALF - 1) >> 24
    sg = np.sign(e)[..., None]
    v = sg * P0   # the candidates are v > 0, the largest first
    assert ((v > 0).sum(-1) >= k4).all(), "kernel stage: fewer candidates than flips"
    flip4 = (v > 0) & (_rank(v, taps) < k4[..., None])
    P = P0 - sg * STEP * flip4
    q = q0 - sg * flip4
    # channel stage
    e1 = P.sum(-1)
    E = e1.sum(-1)
    k5 = (np.abs(E) + HALF - 1) >> 24
    sE = np.sign(E)[:, None]
    key = sE * e1
    assert ((key > 0).sum(-1) >= k5).all(), "channel stage: fewer candidate kernels than flips"
    chosen = (key > 0) & (_rank(key, np.arange(G)) < k5[:, None])
    w = sE[..., None] * P
    fresh = (w > 0) & ~flip4
    # a chosen kernel without a fresh candidate takes back its last flip the other way
    cand = np.where(fresh.any(-1, keepdims=True), fresh, (w > 0) & flip4)
    assert cand.any(-1)[chosen].all(), "channel stage: a chosen kernel has nothing to flip"
    flip5 = chosen[..., None] & cand & (_rank(np.where(cand, w, -1), taps) == 0)
    P = P - sE[..., None] * STEP * flip5
    q = q - sE[..., None] * flip5
    qf = q.reshape(rows, n)
    dst = (qf.astype(np.float32) * s).astype(np.float32) + mn
    return {"q0": q0.reshape(rows, n), "q": qf, "dst": dst.astype(np.float32), "P0": P0, "P": P,
            "flips": np.stack([k4.sum(-1), k5], axis=1).astype(np.int32), "undone": int((flip5 & flip4).sum())}


@dataclass
class Case:
    name: str
    x: np.ndarray   # [rows, G * T] float32
    T: int
    bits: int
    mode: int
    offset: int     # floats between a 16-B boundary and the weight's first element
    kind: str

    @property
    def G(self):
        return self.x.shape[1] // self.T


def _content(kind, rows, n, bits, rng):
    if kind == "normal":
        return rng.standard_normal((rows, n)).astype(np.float32)
    if kind == "dense":   # every element 0.49 of a step above a code of the row's own asymmetric grid
        L = (1 << bits) - 1
        s = np.float32(2.0) / np.float32(L)
        x = np.float32(-1.0) + (rng.integers(0, L, (rows, n)).astype(np.float32) + np.float32(0.49)) * s
    elif kind == "tie":   # one repeated value: equal P in every kernel, equal e' in every kernel
        x = np.full((rows, n), 0.3, np.float32)
    elif kind == "constant":
        return np.full((rows, n), 0.75, np.float32)
    else:
        # "clamp".  Odd rows: a range under the 1e-8 scale floor times the levels (s = 1e-8).  Even rows: a
        # maximum whose quotient by its own rounded scale lands above qmax, so the clamp acts on it (the
        # floor alone never pushes t off the grid: it only widens the step)
        L, lo = (1 << bits) - 1, np.float32(-0.37)
        m = rng.random(4000).astype(np.float32)
        t = ((m - lo).astype(np.float32) / ((m.astype(np.float64) - np.float64(lo)) / L).astype(np.float32)).astype(np.float32)
        top = m[np.flatnonzero(t > L)[0]]
        x = rng.random((rows, n)).astype(np.float32)
        x[0::2] = lo + x[0::2] * (top - lo)
        x[1::2] *= np.float32(1e-8)
        x[0::2, 0], x[1::2, 0] = lo, 0.0
        x[0::2, -1], x[1::2, -1] = top, 1e-8
        return np.clip(x, x[:, :1], x[:, -1:])   # (the ends stay the range, whatever the products rounded to)
    x[:, 0], x[:, -1] = (-1.0, 1.0) if kind == "dense" else (0.0, 1.0)
    return x.astype(np.float32)


def group(gi):
    """The five cases (one per kind) of (G, T) pair gi; rows, bits, mode and offset cycle so
    that the groups together hold every value of each."""
    G, T = GT[gi]
    out = []
    for ki, kind in enumerate(KINDS):
        rows = ROWS[(gi + ki) % 3]
        if rows * G * T > (1 << 18):   # the long rows stay few
            rows = 3 if 3 * G * T <= (1 << 18) else 1
        bits, mode, offset = BITS[(gi + ki) % 3], (gi + 3 * ki) % 4, (gi + ki) % 2
        rng = np.random.default_rng(1000 * gi + ki + 1)   # (+1: with +0 one normal row rounds to |E| < 2^23 by itself)
        out.append(Case("G%d_T%d_%s_r%d_b%d_m%d_o%d" % (G, T, kind, rows, bits, mode, offset),
                        _content(kind, rows, G * T, bits, rng), T, bits, mode, offset, kind))
    return out


def all_cases():
    return [c for gi in range(len(GT)) for c in group(gi)]
