"""The CLE edge cases (tests/cle_edge_cases.py) on the host: every chain's shapes
satisfy the predicate of the kernel branch it is named for, the chains together
reach every branch the module lists (a case cannot silently stop reaching its
branch), the module's constants are the header's, and every graph's plan structure
passes the planner's own index checker (dfq_diag_cle_check_structure) at the 8
reference threads.  No GPU."""
import re
from pathlib import Path

import numpy as np
import pytest

from data_free_quantization_amd import _lib
from tests import cle_edge_cases as CE
from tests.test_cle_structure import _Addr, _check

CSRC = Path(__file__).resolve().parent.parent / "data_free_quantization_amd" / "csrc"


def test_constants_are_the_headers():
    text = (CSRC / "dfq_cle_plan.h").read_text()

    def const(name):
        m = re.search(r"constexpr\s+\w+\s+(?:\w+\s*=\s*[^,;]+,\s*)*?%s\s*=\s*([^,;]+)[,;]" % name, text)
        assert m, name
        v = m.group(1).strip()
        return int(re.search(r"#define %s (\d+)" % v, text).group(1)) if not v[0].isdigit() else int(v)

    assert const("kWave") == CE.K_WAVE and const("kThreads") == CE.K_THREADS
    assert const("kColTileRows") == CE.K_COL_TILE_ROWS and const("kPosTileMaxRows") == CE.K_POS_TILE_MAX_ROWS
    assert const("kTileMaxKhw") == CE.K_TILE_MAX_KHW and const("kCleTile") == CE.K_CLE_TILE
    assert const("kCleChansPerTask") == CE.K_CHANS_PER_TASK and const("kCleW1SmallElems") == CE.K_W1_SMALL_ELEMS
    assert _lib.REF_THREADS == CE.REF_THREADS
    # rows_per_task as the header states it: 4 waves x the rows a wave holds
    assert [CE.rows_per_task(n) for n in (1, 2, 3, 9, 33, 63, 64, 2052)] == [256, 128, 64, 16, 4, 4, 4, 4]


@pytest.mark.parametrize("graph", list(CE.GRAPHS))
def test_every_chain_reaches_its_branch(graph):
    chains = CE.GRAPHS[graph]
    assert sum(len(c.layers) for c in chains) <= CE.MAX_TARGET_LAYERS
    for c in chains:
        assert c.branch in CE.BRANCHES, c.name
        assert CE.BRANCHES[c.branch](c.rel(c.on)), (c.name, c.branch, c.rel(c.on))


def test_branch_tags_are_all_reached_and_names_unique():
    chains = [c for g in CE.GRAPHS.values() for c in g]
    assert {c.branch for c in chains} == set(CE.BRANCHES)
    assert len({c.name for c in chains}) == len(chains)


def test_required_shapes_are_present():
    """The shape lists the cases were asked to hold, group by group."""
    on = {g: [c.rel(c.on) for c in CE.GRAPHS[g]] for g in CE.GRAPHS}
    len1 = {r.len1 for r in on["A_rows"]}
    assert {1, 2, 3, 5, 9, 27, 33, 63, 65, 255, 257, 513, 1031, 64, 68, 252, 256, 260, 508, 512, 516, 1020, 1024,
            1028, 2052} <= len1
    for n in (9, 64, 1028):   # 1 and one less than, equal to, one more than both task row counts
        want = {1} | {k + d for k in (CE.rows_per_task(n), CE.w1_apply_rows(n)) for d in (-1, 0, 1)}
        assert want <= {r.c1 for r in on["A_tasks"] if r.len1 == n}, n
    dw = [r for g in ("B_dw", "B_dw1mid", "B_m2mid") for r in on[g] if r.i2 == 1]
    for both in (False, True):
        assert {1, 4, 9, 25, 49, 64, 81} <= {r.khw2 for r in dw if r.dw_both == both and r.o2g == 1}
    assert {r.unfused for r in dw if r.o2g == 2} == {False, True}
    assert {1, 15, 16, 17, 33} <= {r.c1 for r in dw}
    c = [r for r in on["C_1x1"] if r.khw2 == 1 and r.groups == 1]
    assert {1, 15, 16, 17, 33} <= {r.o2 for r in c} and {1, 2, 255, 256, 257, 513} <= {r.i2 for r in c}
    d = [r for r in on["D_pos"] if r.pos + 1 == r.nrel]
    assert {4, 6, 9} <= {r.khw2 for r in d} and {1, 3, 4, 5, 17} <= {r.o2 for r in d}
    assert {2, 28, 29, 255, 256, 257, 300} <= {r.i2 for r in d}
    e = on["E_walk"]
    assert {(r.khw2, r.i2) for r in e if r.o2 == 17} >= {(k, i) for k in (16, 25, 49) for i in (3, 257)}
    f = [r for r in on["F_grouped"] if r.groups > 1]
    assert {1, 3, 5, 16, 20} <= {r.o2g for r in f} and {2, 3, 4} <= {r.groups for r in f}
    assert {(r.o2g, r.khw2) for r in f} >= {(o, k) for o in (1, 3, 5, 16, 20) for k in (1, 9, 25)}
    g = [r for r in on["G_channels"] if r.nrel == 1]
    assert {255, 256, 257, 1023, 1024, 1025} <= {r.c1 for r in g}
    assert all(r.len1 == 2 and r.o2 == 2 for r in g)
    assert any(not r.bn_stats for r in g) and any(not r.bias for r in g)
    assert {1, 7, 8, 9, 31, 32, 33, 255, 8191, 8192, 8193, 8223, 16392, 32767, 32768, 32769, 65535, 65536, 65541,
            262147, 294913} <= {r.n1 for r in on["H_metric"]}


@pytest.mark.parametrize("value_set", CE.VALUE_SETS)
def test_values_follow_the_planted_rule(value_set):
    """Finite everywhere; planted: each W1 row's minimum is its first element and its
    maximum its last, with all-negative, all-zero and denormal-only rows present."""
    seen = {"negative": 0, "zero": 0, "denormal": 0}
    for graph in CE.GRAPHS:
        T = CE.tensors(graph, value_set)
        for c in CE.GRAPHS[graph]:
            for t in (T[CE.layer_name(c, j)] for j in range(len(c.layers))):
                assert np.isfinite(t["w"]).all() and (t["b"] is None or np.isfinite(t["b"]).all()), c.name
            if value_set != "planted" or c.dead or c.negative:
                continue
            rows = T[CE.layer_name(c, 0)]["w"].reshape(c.layers[0].o, -1)
            assert (rows[:, 0] == rows.min(1)).all() and (rows[:, -1] == rows.max(1)).all(), c.name
            w2 = T[CE.layer_name(c, 1)]["w"]
            lay, r = c.layers[1], c.rel(0)
            cols = w2.reshape(r.groups, r.o2g, r.i2, r.khw2).transpose(0, 2, 1, 3).reshape(r.c1, -1)
            assert (cols[:, 0] == cols.min(1)).all() and (cols[:, -1] == cols.max(1)).all(), (c.name, lay)
            for u in (rows, cols):
                seen["negative"] += int((u.max(1) < 0).sum())
                seen["zero"] += int((np.abs(u).max(1) == 0).sum())
                tiny = np.abs(u).max(1)
                seen["denormal"] += int(((tiny > 0) & (tiny < np.finfo(np.float32).tiny)
                                         & ((u != 0).all(1))).sum())
    if value_set == "planted":
        assert all(v >= 20 for v in seen.values()), seen


@pytest.mark.parametrize("graph", list(CE.GRAPHS))
def test_plan_structure_passes_the_checker(graph):
    A = _Addr()
    rows = []
    for first, second, bn, c, j in CE.relations(graph):
        r = c.rel(j)
        rows.append((A(first, "w"), A(second, "w"), A(first, "b"), A(bn, "fw") if r.bn_stats else 0,
                     A(bn, "fb") if r.bn_stats else 0, A((first, second), "S"), r.c1, r.len1, r.o2, r.i2, r.khw2, 1, 0))
    names = [CE.layer_name(c, j) for c in CE.GRAPHS[graph] for j in range(len(c.layers))]
    sizes = [lay.numel for c in CE.GRAPHS[graph] for lay in c.layers]
    rc, info, msg = _check(rows, [A(n, "w") for n in names], sizes, CE.REF_THREADS)
    assert rc == _lib.DFQ_OK, (graph, msg)
    assert msg.startswith("digest "), msg
