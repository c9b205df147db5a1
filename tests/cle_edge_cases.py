"""The cross-layer-equalization cases at the edges of the device-resident loop's
kernels (csrc/dfq_cle_kernels.h: cle_range_body, cle_apply_body, cle_rel_scale,
cle_tiles_body, cle_chunk_sum_with, cle_tiny_chunk_sum) and of the single-relation
kernel (csrc/dfq_cle_relation.hip): small graphs of independent chains of one to
three relations, each chain named for the kernel branch it aims at.
tests/golden/make_golden.py (section ``cle_edge``) runs the reference's own
_layer_equalization and metric on them into tests/golden/cle_edge_cases.npz;
tests/test_oracle_cle_edges.py holds the CPU oracle to that file,
tests/test_gpu_cle_edges.py the HIP kernels to both, and
tests/test_cle_edge_host.py checks that every chain still reaches its branch.
Pure numpy: no torch, no GPU.

A chain is a list of layers; consecutive layers form its relations.  Every chain
carries a ``branch`` tag whose predicate (BRANCHES) restates the kernel's or the
planner's condition from the constants of csrc/dfq_cle_plan.h, over the shapes of
the relation the chain aims at (``Chain.on``).

Shape groups (graph names):
  A_rows, A_tasks  W1 row lengths (short lane-group rows, the scalar and float4
                   wave paths next to their 256 / 1,024-element strides) and row
                   counts around the range and rescale tasks' row counts
  B_dw, B_dw1mid, B_m2mid
                   depthwise second layers (i2 == 1): 1x1 .. 9x9 filters and a
                   channel multiplier of 2, each as the end of a chain
                   (kApplyW2Contig) and as the middle of pointwise -> depthwise ->
                   pointwise (kApplyDwBoth; the multiplier's middle makes the plan
                   unfused, so it has a graph of its own), a dead and an
                   all-negative filter, depthwise -> depthwise
  C_1x1            1x1 / Linear row tiles: o2 around the 16-row tile, i2 around
                   the 256-column tile
  D_pos            position-parallel tiles (2x2, 2x3, 3x3)
  E_walk           the per-column walk of 4x4, 5x5, 7x7 second layers
  F_grouped        grouped second layers with i2 > 1: 16-row range tiles and
                   4-row rescale tiles straddling group boundaries
  G_channels       per-channel vector tasks (256 channels) and range resets
                   (1,024), a relation without BN statistics, one without bias
  H_metric         rescaled layers of exact element counts around the metric's
                   8-element, 32-stream, 8,192-element tile and 32,768-element
                   chunk limits

Each graph comes in two value sets (VALUE_SETS):
  random   weights ~ normal(0, 1)
  planted  per range unit (a W1 row; a W2 input channel's column over its group's
           rows), the minimum is the unit's FIRST element and the maximum its
           LAST (for a column: the first row's first tap and the last row's last
           tap), so a dropped head or tail changes the range; every fifth unit is
           all negative, one unit is all zeros and one holds denormals only.  No
           NaN, no infinity.
"""
from __future__ import annotations

import hashlib
from collections import OrderedDict
from dataclasses import dataclass
from functools import lru_cache
from typing import Optional, Tuple

import numpy as np

# ---- constants of csrc/dfq_cle_plan.h (tests/test_cle_edge_host.py reads the header) ----
K_WAVE = 64               # kWave
K_THREADS = 256           # kThreads: columns per W2 tile, channels per kApplyChannels task
K_COL_TILE_ROWS = 16      # kColTileRows
K_POS_TILE_MAX_ROWS = 4   # kPosTileMaxRows (DFQ_CLE_POS_ROWS)
K_TILE_MAX_KHW = 9        # kTileMaxKhw
K_CLE_TILE = 8192         # kCleTile
K_CHANS_PER_TASK = 1024   # kCleChansPerTask (kRangeReset / kRangeResetW1)
K_W1_SMALL_ELEMS = 2048   # kCleW1SmallElems
PAR_NUMEL = 32768         # at::internal::GRAIN_SIZE: torch.mean splits layers from here on by thread
REF_THREADS = 8           # the reference run's torch threads (make_golden.pipeline)

VALUE_SETS = ("random", "planted")
ITERATIONS = 3
S_MIN_MAX = (1e-8, 1e8)
#: tensors up to this many elements are stored in the fixture as arrays, larger ones
#: as their digest (h) only
ARRAY_MAX = 48
SEED = 20261021


def row_group_lanes(n: int) -> int:
    if n >= 64:
        return 64
    g = 1
    while g < n:
        g <<= 1
    return g


def rows_per_task(n: int) -> int:
    return 4 * (64 // row_group_lanes(n))


def w1_apply_rows(len1: int) -> int:
    """Rows of a kApplyW1 task (dfq_cle_plan.cpp, cle_apply_tasks)."""
    k = rows_per_task(len1)
    return 2 * k if k * len1 < K_W1_SMALL_ELEMS else k


def h(a) -> str:
    """sha256 of fp32 bytes with -0 folded to +0 (make_golden.h)."""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32)) + np.float32(0.0)
    return hashlib.sha256(a.tobytes()).hexdigest()


@dataclass(frozen=True)
class L:
    """A Conv2d (o, i per group, kh x kw, groups) or, with ``linear``, a Linear."""
    o: int
    i: int
    kh: int = 1
    kw: int = 1
    groups: int = 1
    bias: bool = True
    linear: bool = False

    @property
    def shape(self):
        return (self.o, self.i) if self.linear else (self.o, self.i, self.kh, self.kw)

    @property
    def numel(self):
        return self.o * self.i * self.kh * self.kw


@dataclass(frozen=True)
class Rel:
    """One relation's shapes, as dfq_cle_rel / CleRel hold them."""
    c1: int
    len1: int
    o2: int
    i2: int
    khw2: int
    groups: int
    o2g: int
    n1: int        # elements of W1 / W2
    n2: int
    pos: int       # the relation's place in its chain, and the chain's relation count
    nrel: int
    dw_both: bool  # W2 is a depthwise filter bank that is also the next relation's W1 (kApplyDwBoth)
    unfused: bool  # the chain forces the per-step range launches (the whole plan unfused)
    bn_stats: bool
    bias: bool


@dataclass(frozen=True)
class Chain:
    name: str
    branch: str
    layers: Tuple[L, ...]
    on: int = 0                                   # the relation the branch predicate is about
    bn_stats: Tuple[bool, ...] = ()               # per relation (default: all with fake statistics)
    dead: Optional[Tuple[int, int]] = None        # (layer, output channel): an all-zero filter
    negative: Optional[Tuple[int, int]] = None    # (layer, output channel): an all-negative filter

    def rel(self, j: int) -> Rel:
        a, b = self.layers[j], self.layers[j + 1]
        c1, i2 = a.o, b.i
        groups = c1 // i2
        assert groups * i2 == c1 and b.o % groups == 0 and (b.linear or groups == b.groups), (self.name, j)
        nrel = len(self.layers) - 1

        def is_dw(x, y):   # dfq_cle_plan.cpp, cle_chains: the depthwise pairing's condition
            return y.i == 1 and y.o == x.o

        dw_both = j + 1 < nrel and is_dw(a, b) and not (j > 0 and is_dw(self.layers[j - 1], a))
        unfused = any(self.layers[k + 1].i == 1 and self.layers[k + 1].o != self.layers[k].o for k in range(nrel - 1))
        stats = self.bn_stats[j] if self.bn_stats else True
        return Rel(c1, a.i * a.kh * a.kw, b.o, i2, b.kh * b.kw, groups, b.o // groups, a.numel, b.numel, j, nrel,
                   dw_both, unfused, stats, a.bias)

    @property
    def rels(self):
        return [self.rel(j) for j in range(len(self.layers) - 1)]


def _tile(r: Rel) -> bool:      # W2 row tiles: kRangeW2Tile / kApplyW2Tile
    return r.i2 > 1


def _one_group_tiles(r: Rel, rows: int) -> bool:
    """Every ``rows``-row tile of W2 lies inside one group."""
    return all(a // r.o2g == (min(a + rows, r.o2) - 1) // r.o2g for a in range(0, r.o2, rows))


def _pos_rows(r: Rel) -> int:
    return K_POS_TILE_MAX_ROWS if 1 < r.khw2 <= K_TILE_MAX_KHW else K_COL_TILE_ROWS


#: branch tag -> the kernel's / planner's condition over the relation's shapes
BRANCHES = OrderedDict([
    # A: W1 rows
    ("w1_short", lambda r: r.len1 < K_WAVE),                                   # for_short_rows
    ("w1_wave_scalar", lambda r: r.len1 >= K_WAVE and r.len1 % 4 != 0),         # wave_* with vec1 == 0
    ("w1_wave_vec", lambda r: r.len1 >= K_WAVE and r.len1 % 4 == 0),            # float4 path
    ("w1_task_edge", lambda r: r.c1 == 1 or any(abs(r.c1 - k) <= 1 for k in (rows_per_task(r.len1),
                                                                            w1_apply_rows(r.len1)))),
    ("w1_produced_short", lambda r: r.pos > 0 and not r.unfused and r.len1 < K_WAVE),    # not w1_self
    ("w1_produced_wave", lambda r: r.pos > 0 and not r.unfused and r.len1 >= K_WAVE),    # wave_scale
    # B: depthwise second layers
    ("dw_contig_short", lambda r: r.i2 == 1 and not r.dw_both and r.o2g * r.khw2 < K_WAVE),
    ("dw_contig_wave", lambda r: r.i2 == 1 and not r.dw_both and r.o2g * r.khw2 >= K_WAVE),
    ("dw_both_short", lambda r: r.i2 == 1 and r.dw_both and r.khw2 < K_WAVE),
    ("dw_both_wave", lambda r: r.i2 == 1 and r.dw_both and r.khw2 >= K_WAVE),
    ("dw_multiplier", lambda r: r.i2 == 1 and r.o2g == 2 and not r.unfused),
    ("dw_multiplier_unfused", lambda r: r.i2 == 1 and r.o2g == 2 and r.unfused),
    ("dw_then_dw_short", lambda r: r.i2 == 1 and r.pos == 1 and r.nrel == 3 and r.khw2 < K_WAVE),   # fused contig
    ("dw_then_dw_wave", lambda r: r.i2 == 1 and r.pos == 1 and r.nrel == 3 and r.khw2 >= K_WAVE),   # wave_scale_range
    # C / D / E: W2 row tiles of one group
    ("tile_1x1", lambda r: _tile(r) and r.groups == 1 and r.khw2 == 1 and r.pos + 1 == r.nrel),
    ("tile_1x1_fused", lambda r: _tile(r) and r.groups == 1 and r.khw2 == 1 and r.pos + 1 < r.nrel),
    ("tile_position", lambda r: _tile(r) and r.groups == 1 and 1 < r.khw2 <= K_TILE_MAX_KHW and r.pos + 1 == r.nrel),
    ("tile_position_fused", lambda r: _tile(r) and r.groups == 1 and 1 < r.khw2 <= K_TILE_MAX_KHW
     and r.pos + 1 < r.nrel),
    ("tile_walk", lambda r: _tile(r) and r.groups == 1 and r.khw2 > K_TILE_MAX_KHW and r.pos + 1 == r.nrel),
    ("tile_walk_fused", lambda r: _tile(r) and r.groups == 1 and r.khw2 > K_TILE_MAX_KHW and r.pos + 1 < r.nrel),
    # F: grouped, i2 > 1
    ("grouped_straddle", lambda r: _tile(r) and r.groups > 1 and not _one_group_tiles(r, K_COL_TILE_ROWS)),
    ("grouped_aligned", lambda r: _tile(r) and r.groups > 1 and r.o2g % K_COL_TILE_ROWS == 0),
    ("grouped_straddle_fused", lambda r: _tile(r) and r.groups > 1 and not _one_group_tiles(r, _pos_rows(r))
     and r.pos + 1 < r.nrel),
    # G: per-channel vectors
    ("channels_task_edge", lambda r: any(abs(r.c1 - k) <= 1 for k in (K_THREADS, K_CHANS_PER_TASK))),
    ("no_bn_stats", lambda r: not r.bn_stats),
    ("no_bias", lambda r: not r.bias),
    ("keeps_moving", lambda r: r.nrel >= 3 and r.len1 > 1 and r.o2g * r.khw2 > 1),
    # H: the metric, over the element count of the relation's W1
    ("metric_tiny", lambda r: r.n1 < 8),                                        # cle_tiny_chunk_sum
    ("metric_tail", lambda r: 8 <= r.n1 < K_CLE_TILE),                          # the tail tile alone
    ("metric_tiles", lambda r: K_CLE_TILE <= r.n1 < PAR_NUMEL),                 # full tiles + tail, one chunk
    ("metric_chunks", lambda r: r.n1 >= PAR_NUMEL),                             # REF_THREADS chunks
])


def _pw(c1, i1=2, **kw):
    return L(c1, i1, **kw)


def _graphs():
    G = OrderedDict()

    # ---- A: W1 rows -------------------------------------------------------------------------
    def row_layer(len1, c1):
        # a row of len1 floats as i1 x kh x kw (3x3 where 9 divides it; the kernels see len1 alone)
        return L(c1, len1 // 9, 3, 3) if len1 % 9 == 0 else L(c1, len1)

    def a_chain(tag, len1, c1):
        return Chain(f"{tag}_len{len1}_c{c1}", tag, (row_layer(len1, c1), L(2, c1)))

    rows = [a_chain("w1_short", n, 3) for n in (1, 2, 3, 5, 9, 27, 33, 63)]
    # rows per wave end inside the row count: 64 / G rows per wave, c1 = 3 ends inside all of them but G = 64's
    rows += [a_chain("w1_wave_scalar", n, c) for n, c in ((65, 2), (255, 5), (257, 3), (513, 2), (1031, 2))]
    rows += [a_chain("w1_wave_vec", n, c) for n, c in ((64, 2), (68, 3), (252, 5), (256, 2), (260, 3), (508, 2),
                                                         (512, 3), (516, 2), (1020, 2), (1024, 3), (1028, 2),
                                                         (2052, 2))]
    G["A_rows"] = rows
    tasks = []
    for len1 in (9, 64, 1028):
        ks = sorted({1} | {k + d for k in (rows_per_task(len1), w1_apply_rows(len1)) for d in (-1, 0, 1)})
        tasks += [a_chain("w1_task_edge", len1, c) for c in ks]
    G["A_tasks"] = tasks

    # ---- B: depthwise second layers ---------------------------------------------------------
    def dw(c, kh, kw=None, mult=1):
        return L(c * mult, 1, kh, kw or kh, groups=c)

    dwl = []
    for kh, c1 in ((1, 33), (2, 17), (3, 16), (3, 15), (5, 17), (5, 1), (7, 15), (8, 1), (8, 17), (9, 16), (9, 33)):
        wave = kh * kh >= K_WAVE
        dwl.append(Chain(f"dw_end_{kh}x{kh}_c{c1}", "dw_contig_wave" if wave else "dw_contig_short",
                         (_pw(c1), dw(c1, kh))))
        mid = Chain(f"dw_mid_{kh}x{kh}_c{c1}", "dw_both_wave" if wave else "dw_both_short",
                    (_pw(c1), dw(c1, kh), L(3, c1)))
        if kh == 1:
            # a one-tap filter's unsigned range is 0: both of its relations scale it by 1e8 in every
            # iteration (ONE_ELEMENT_SCALE), which would drown every other chain's part of the metric
            G["B_dw1mid"] = [mid]
        else:
            dwl.append(mid)
    dwl.append(Chain("dw_end_3x3_m2_c33", "dw_multiplier", (_pw(33), dw(33, 3, mult=2))))
    dwl.append(Chain("dw_mid_3x3_dead", "dw_both_short", (_pw(17), dw(17, 3), L(3, 17)), dead=(1, 16)))
    dwl.append(Chain("dw_mid_3x3_negative", "dw_both_short", (_pw(17), dw(17, 3), L(3, 17)), negative=(1, 0)))
    dwl.append(Chain("dw_end_8x8_dead", "dw_contig_wave", (_pw(5), dw(5, 8)), dead=(1, 4)))
    dwl.append(Chain("dw_mid_9x9_negative", "dw_both_wave", (_pw(5), dw(5, 9), L(3, 5)), negative=(1, 4)))
    dwl.append(Chain("dw_dw_3x3_8x8", "dw_then_dw_wave", (_pw(17), dw(17, 3), dw(17, 8), L(3, 17)), on=1))
    dwl.append(Chain("dw_dw_8x8_3x3", "dw_then_dw_short", (_pw(15), dw(15, 8), dw(15, 3), L(3, 15)), on=1))
    G["B_dw"] = dwl
    G["B_m2mid"] = [
        Chain("dw_mid_3x3_m2_c33", "dw_multiplier_unfused", (_pw(33), dw(33, 3, mult=2), L(3, 66))),
        # beside it, under the per-step range launches the multiplier forces on the whole plan
        Chain("unfused_1x1", "tile_1x1", (_pw(257), L(17, 257))),
        Chain("unfused_3x3", "tile_position", (_pw(29), L(5, 29, 3, 3))),
        Chain("unfused_dw", "dw_contig_short", (_pw(17), dw(17, 3))),
    ]

    # ---- C: 1x1 / Linear row tiles ----------------------------------------------------------
    c = []
    for o2, i2, lin in ((1, 513, False), (1, 257, True), (1, 256, False), (1, 255, True), (17, 256, False),
                        (16, 257, True), (15, 255, False), (33, 2, False), (33, 1, False), (15, 2, True),
                        (16, 2, False), (17, 1, False), (33, 513, True)):
        c.append(Chain(f"tile_1x1_o{o2}_i{i2}" + ("_linear" if lin else ""), "tile_1x1" if i2 > 1 else "dw_contig_short",
                       (_pw(i2), L(o2, i2, linear=lin))))
    c.append(Chain("tile_1x1_fused_o17_i5", "tile_1x1_fused", (_pw(5, 3), L(17, 5), L(3, 17))))
    c.append(Chain("tile_1x1_fused_o33_i257", "tile_1x1_fused", (_pw(257), L(33, 257), L(2, 33))))
    c.append(Chain("w1_produced_short_5", "w1_produced_short", (_pw(5, 3), L(17, 5), L(3, 17)), on=1))
    G["C_1x1"] = c

    # ---- D: position-parallel tiles ---------------------------------------------------------
    d = []
    for (kh, kw), o2, i2 in (((2, 2), 1, 257), ((2, 2), 3, 28), ((2, 2), 17, 2), ((2, 2), 5, 300), ((2, 2), 4, 256),
                             ((2, 3), 4, 29), ((2, 3), 1, 255), ((2, 3), 17, 256), ((2, 3), 5, 2), ((2, 3), 3, 300),
                             ((3, 3), 3, 257), ((3, 3), 4, 28), ((3, 3), 5, 29), ((3, 3), 1, 300), ((3, 3), 17, 255),
                             ((3, 3), 4, 2)):
        d.append(Chain(f"tile_pos_{kh}x{kw}_o{o2}_i{i2}", "tile_position", (_pw(i2), L(o2, i2, kh, kw))))
    d.append(Chain("tile_pos_fused_3x3_o6_i8", "tile_position_fused", (_pw(8, 3), L(6, 8, 3, 3), L(3, 6))))
    d.append(Chain("tile_pos_fused_2x3_o5_i29", "tile_position_fused", (_pw(29), L(5, 29, 2, 3), L(3, 5))))
    d.append(Chain("w1_produced_wave_72", "w1_produced_wave", (_pw(8, 3), L(6, 8, 3, 3), L(3, 6)), on=1))
    G["D_pos"] = d

    # ---- E: the per-column walk -------------------------------------------------------------
    e = [Chain(f"tile_walk_{k}x{k}_o17_i{i2}", "tile_walk", (_pw(i2), L(17, i2, k, k)))
         for k in (4, 5, 7) for i2 in (3, 257)]
    e.append(Chain("tile_walk_fused_5x5_o6_i13", "tile_walk_fused", (_pw(13, 3), L(6, 13, 5, 5), L(3, 6))))
    e.append(Chain("w1_produced_wave_325", "w1_produced_wave", (_pw(13, 3), L(6, 13, 5, 5), L(3, 6)), on=1))
    G["E_walk"] = e

    # ---- F: grouped second layers, i2 > 1 ---------------------------------------------------
    f = []
    combos = [(1, 2, 1), (1, 3, 3), (1, 4, 5), (3, 3, 1), (3, 4, 3), (3, 2, 5), (5, 4, 1), (5, 2, 3), (5, 3, 5),
              (16, 2, 1), (16, 3, 3), (16, 2, 5), (20, 3, 1), (20, 4, 3), (20, 2, 5)]
    for n, (o2g, groups, k) in enumerate(combos):
        i2 = (2, 3, 5)[n % 3]
        tag = "grouped_aligned" if o2g % K_COL_TILE_ROWS == 0 else "grouped_straddle"
        f.append(Chain(f"grouped_o2g{o2g}_g{groups}_{k}x{k}_i{i2}", tag,
                       (_pw(groups * i2), L(o2g * groups, i2, k, k, groups=groups))))
    f.append(Chain("grouped_o2g20_g2_3x3_i300", "grouped_straddle", (_pw(600), L(40, 300, 3, 3, groups=2))))
    f.append(Chain("grouped_fused_o2g5_g2_3x3", "grouped_straddle_fused",
                   (_pw(6), L(10, 3, 3, 3, groups=2), L(3, 10))))
    f.append(Chain("grouped_fused_o2g5_g3_1x1", "grouped_straddle_fused",
                   (_pw(6), L(15, 2, 1, 1, groups=3), L(3, 15))))
    G["F_grouped"] = f

    # ---- G: per-channel vectors -------------------------------------------------------------
    g = [Chain(f"channels_c{c1}", "channels_task_edge", (_pw(c1), L(2, c1))) for c1 in (255, 256, 257, 1023, 1024, 1025)]
    g.append(Chain("channels_no_bn_stats", "no_bn_stats", (_pw(257), L(2, 257)), bn_stats=(False,)))
    g.append(Chain("channels_no_bias", "no_bias", (_pw(257, bias=False), L(2, 257))))
    G["G_channels"] = g

    # ---- H: the metric ----------------------------------------------------------------------
    hm = []
    for n in (1, 7, 8, 9, 31, 32, 33, 255, 8191, 8192, 8193, 8223, 16392, 32767, 32768, 32769, 65535, 65536, 65541,
              262147, 294913):
        tag = "metric_tiny" if n < 8 else "metric_tail" if n < K_CLE_TILE else \
            "metric_tiles" if n < PAR_NUMEL else "metric_chunks"
        # one W1 row of n elements over a tiny W2 (a one-channel 1x3 filter, then two more weights: the
        # second relation keeps the first from converging in one iteration)
        hm.append(Chain(f"metric_n{n}", tag, (L(1, n), L(1, 1, 1, 3), L(2, 1))))
    # a Linear second layer of such a count, rescaled through its 8,193 columns
    hm.append(Chain("metric_linear_n8193", "metric_tiles", (L(8193, 1), L(1, 8193, linear=True))))
    G["H_metric"] = hm
    return G


def _with_movers(G):
    """A chain of one relation converges in its first iteration; a chain of three keeps
    every graph's summed change far above the loop's threshold (2e-7) for the three
    iterations the tests run, so the stop rule cannot end a run early."""
    for name, chains in G.items():
        chains.append(Chain(f"moving_{name}", "keeps_moving", (L(6, 5), L(7, 6), L(5, 7), L(4, 5)), on=1))
    return G


GRAPHS = _with_movers(_graphs())
MAX_TARGET_LAYERS = 100   # above 128 the stop rule leaves numpy's one-leaf sum (tested elsewhere)


def graph_ids():
    return [f"{g}.{v}" for g in GRAPHS for v in VALUE_SETS]


def layer_name(chain: Chain, j: int) -> str:
    return f"{chain.name}/{j}"


def bn_name(chain: Chain, j: int) -> str:
    return f"{chain.name}/bn{j}"


def relations(graph: str):
    """[(first layer, second layer, bn, chain, relation index in the chain)], chain by chain."""
    return [(layer_name(c, j), layer_name(c, j + 1), bn_name(c, j), c, j)
            for c in GRAPHS[graph] for j in range(len(c.layers) - 1)]


# ---- values -------------------------------------------------------------------------------
#: A range unit of ONE element (a W1 row of one float, a W2 column of one row and one
#: tap) has the unsigned range 0, so the reference's scale is NaN clamped to s_max = 1e8
#: (or 0 clamped to s_min) in every iteration and the layer grows by 1e8 each time.  Such
#: layers start at this power of two: finite after three iterations, and their change
#: (~1e-6) does not drown the other layers' in the loop's float64 sum of layer means.
ONE_ELEMENT_SCALE = 2.0 ** -100


def one_element_units(chain: Chain, j: int) -> bool:
    """Layer j of the chain is a W1 of one-element rows or a W2 of one-element columns."""
    lay = chain.layers[j]
    as_w1 = j + 1 < len(chain.layers) and chain.rel(j).len1 == 1
    as_w2 = j > 0 and chain.rel(j - 1).o2g * chain.rel(j - 1).khw2 == 1
    return (as_w1 or as_w2) and lay.numel > 0


def _units(layer: L, as_columns: bool):
    """A view function pair: weight [shape] <-> [units, unit length], units being the
    W1 rows or, for a second layer, its input channels' columns over their group."""
    o, i, k = layer.o, layer.i, layer.kh * layer.kw
    if not as_columns:
        return (lambda w: w.reshape(o, i * k)), (lambda u: u.reshape(layer.shape))
    g = layer.groups
    og = o // g
    fwd = lambda w: w.reshape(g, og, i, k).transpose(0, 2, 1, 3).reshape(g * i, og * k)       # noqa: E731
    back = lambda u: u.reshape(g, i, og, k).transpose(0, 2, 1, 3).reshape(layer.shape)        # noqa: E731
    return fwd, back


def _plant(u: np.ndarray, shift: int) -> np.ndarray:
    """The planted rule on units [n, length] (a copy).  ``shift`` moves the zero and
    the denormal unit, so that a relation's W1 and W2 do not hold them at the same
    channel."""
    u = (u * np.float32(0.25)).astype(np.float32)
    n, length = u.shape
    np.clip(u, -1.5, 1.5, out=u)
    frac = (np.arange(n) % 16).astype(np.float32) / np.float32(16)
    u[:, -1] = 2 + frac
    u[:, 0] = -(2 + frac) if length > 1 else u[:, 0]
    neg = np.arange(n) % 5 == 2
    u[neg] = -np.abs(u[neg]) - np.float32(0.125)
    u[neg, -1] = -np.float32(0.0625)
    if length > 1:
        u[neg, 0] = -(3 + frac[neg])
    if n >= 4:
        u[(n // 2 + shift) % n] = 0.0
        # denormals only: m * 2^-149, min first, max last
        m = (np.arange(length) % 97 + 2).astype(np.float64)
        m[-1] = 8000.0
        m[0] = 1.0 if length > 1 else m[0]
        u[(n // 2 + 1 + shift) % n] = np.ldexp(m, -149).astype(np.float32)
    return u


@lru_cache(maxsize=4)
def tensors(graph: str, value_set: str):
    """OrderedDict name -> {"w": .., "b": .. or None} for the layers and name ->
    {"fw": .., "fb": ..} (None without fake statistics) for each relation's BN, fp32
    numpy (read-only), from PCG64 seeds."""
    assert value_set in VALUE_SETS
    gi = list(GRAPHS).index(graph)
    out = OrderedDict()
    for ci, chain in enumerate(GRAPHS[graph]):
        for j, layer in enumerate(chain.layers):
            rng = np.random.Generator(np.random.PCG64([SEED, gi, ci, j]))
            w = rng.normal(0, 1, layer.shape).astype(np.float32)
            drawn = w
            b = rng.normal(0, 0.1, layer.o).astype(np.float32) if layer.bias else None
            if value_set == "planted":
                fwd, back = _units(layer, as_columns=j > 0)
                w = np.ascontiguousarray(back(_plant(fwd(w), 2 if j > 0 else 0)))
            for what, fill in ((chain.dead, "dead"), (chain.negative, "negative")):
                if what is not None and what[0] == j:
                    w[what[1]] = 0.0 if fill == "dead" else -np.abs(drawn[what[1]]) - np.float32(0.125)
            if one_element_units(chain, j):
                w = (w * np.float32(ONE_ELEMENT_SCALE)).astype(np.float32)
            w.setflags(write=False)
            if b is not None:
                b.setflags(write=False)
            out[layer_name(chain, j)] = {"w": w, "b": b}
            if j + 1 < len(chain.layers):
                stats = chain.bn_stats[j] if chain.bn_stats else True
                fw = rng.uniform(0.5, 1.5, layer.o).astype(np.float32) if stats else None
                fb = rng.normal(0, 0.5, layer.o).astype(np.float32) if stats else None
                for a in (fw, fb):
                    if a is not None:
                        a.setflags(write=False)
                out[bn_name(chain, j)] = {"fw": fw, "fb": fb}
    return out


def input_digest(graph: str, value_set: str) -> str:
    T = tensors(graph, value_set)
    return h(np.concatenate([a.ravel() for t in T.values() for a in t.values() if a is not None]))


# ---- the fixture's layout -----------------------------------------------------------------
def pack(graph: str, W, B, BN, S):
    """A run's results in the fixture's order.  W / B: layer name -> array (B: None
    where no bias exists and none was created); BN: bn name -> (fake weight, fake
    bias) or Nones; S: one vector per relation, in relations() order.  Returns
    (index, small, digests): ``index`` lists (tensor name, start, stop) into ``small``
    (the concatenated tensors of <= ARRAY_MAX elements) or (tensor name, -1, row) into
    ``digests`` (uint8 [n, 32]: h of each larger tensor)."""
    items = []
    rels = relations(graph)
    for c in GRAPHS[graph]:
        for j in range(len(c.layers)):
            n = layer_name(c, j)
            items.append((n + ":weight", W[n]))
            if B.get(n) is not None:
                items.append((n + ":bias", B[n]))
            if j + 1 < len(c.layers):
                fw, fb = BN[bn_name(c, j)]
                if fw is not None:
                    items.append((bn_name(c, j) + ":fake_weight", fw))
                    items.append((bn_name(c, j) + ":fake_bias", fb))
    items += [(f"{a}>{b}:S", S[i]) for i, (a, b, _, _, _) in enumerate(rels)]
    index, small, digests, off = [], [], [], 0
    for name, a in items:
        a = np.asarray(a, dtype=np.float32).ravel()
        if a.size <= ARRAY_MAX:
            index.append((name, off, off + a.size))
            small.append(a)
            off += a.size
        else:
            index.append((name, -1, len(digests)))
            digests.append(np.frombuffer(bytes.fromhex(h(a)), dtype=np.uint8))
    return (index, np.concatenate(small) if small else np.zeros(0, np.float32),
            np.stack(digests) if digests else np.zeros((0, 32), np.uint8))


def first_difference(name, got, want) -> str:
    """'' when equal by value (np.array_equal), else the message of a mismatch: the
    tensor, the first differing flat index and both values."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"{name}: shape {got.shape} != {want.shape}"
    if np.array_equal(got, want):
        return ""
    g, w = got.ravel(), want.ravel()
    bad = np.flatnonzero(~((g == w) | (np.isnan(g) & np.isnan(w))))
    k = int(bad[0])
    return f"{name}: {bad.size} of {g.size} differ, first at flat index {k}: got {g[k]!r}, want {w[k]!r}"
