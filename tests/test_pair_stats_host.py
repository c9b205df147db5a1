"""dfq_pair_stats_batch without a GPU: the planner alone under sanitizers, the
entry points' argument checks, and quality.py's host arithmetic."""
import ctypes as C
import json
import math
import os
import random
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from data_free_quantization_amd import _lib, quality
from tests.pair_stats_cases import P, SHAPES, view2d

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "data_free_quantization_amd" / "libdfq_hip.so"
CXX = next((c for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"), shutil.which("c++"))
            if c and os.path.exists(c)), None)


def _zoo_shapes():
    import torch   # noqa: F401
    from data_free_quantization_amd import zoo
    return {name: [view2d(tuple(m.weight.shape)) for m in zoo.target_layers(zoo.MODELS[name]())]
            for name in zoo.MODELS}


def _random_shapes():
    rng = random.Random(20240607)
    return [(rng.randint(1, 300), rng.randint(1, 3 * P + 7)) for _ in range(50)]


def _lists():
    """(name, [(rows, row_len, want_rows_out)]): the GPU tests' shapes, the zoo's
    target weights, 50 random shapes -- and, for the alone-or-one-of-many check,
    every GPU-test and random shape alone and 20 of them as one list."""
    gpu = [view2d(s) for s in SHAPES]
    rnd = _random_shapes()
    out = [("gpu", [(r, l, 1) for r, l in gpu]), ("random", [(r, l, 1) for r, l in rnd]),
           ("gpu_no_rows", [(r, l, 0) for r, l in gpu]),
           ("mixed", [(r, l, i % 2) for i, (r, l) in enumerate(gpu + rnd)])]
    out += [("zoo:" + k, [(r, l, 1) for r, l in v]) for k, v in _zoo_shapes().items()]
    out.append(("twenty", [(r, l, 1) for r, l in (gpu + rnd)[5:25]]))
    out += [("alone:%d" % i, [(r, l, 1)]) for i, (r, l) in enumerate(gpu + rnd)]
    return out


def _run_planner(tmp_path, lists):
    text = []
    for _, shapes in lists:
        text.append(str(len(shapes)))
        text += ["%d %d %d" % s for s in shapes]
    (tmp_path / "lists.txt").write_text("\n".join(text) + "\n")
    exe = tmp_path / "stats_plan_check"
    csrc = ROOT / "data_free_quantization_amd" / "csrc"
    subprocess.run([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", str(ROOT / "include"), "-I", str(csrc),
                    str(ROOT / "tests" / "native" / "stats_plan_check.cpp"), str(csrc / "dfq_stats_plan.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe), str(tmp_path / "lists.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert not r.stderr, r.stderr[-4000:]   # no sanitizer report
    plans = []
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "list":
            plans.append({"head": {w[i]: int(w[i + 1]) for i in range(2, len(w), 2)}, "pairs": [], "tasks": []})
        elif w[0] == "pair":
            plans[-1]["pairs"].append((int(w[3]), int(w[5])))
        else:
            assert w[0] == "task", line
            plans[-1]["tasks"].append((int(w[1]), int(w[2]), int(w[3])))
    assert len(plans) == len(lists)
    return plans


def _check_plan(name, shapes, plan):
    h = plan["head"]
    assert h["rc"] == _lib.DFQ_OK, name
    assert h["tasks"] == len(plan["tasks"]) and len(plan["pairs"]) == len(shapes), name
    # the workspace holds the tables, every partial slot and every buffered row record
    assert 0 <= h["o_tasks"] and h["o_tasks"] + 16 * h["tasks"] <= h["o_slots"], name
    assert h["o_slots"] + 32 * h["slots"] <= h["o_rows"], name
    assert h["o_rows"] + 32 * h["buf_rows"] <= h["total"] <= h["ws"], name
    by_pair = {}
    for pair, nrows, first in plan["tasks"]:
        by_pair.setdefault(pair, []).append((nrows, first))
    order = [t[0] for t in plan["tasks"]]
    assert order == sorted(order), name   # list order
    slots_seen = buf_seen = 0
    for p, (rows, row_len, want) in enumerate(shapes):
        slot_base, row_base = plan["pairs"][p]
        tasks = by_pair[p]
        if want:
            assert row_base == -1, (name, p)
        else:
            assert row_base == buf_seen, (name, p)
            buf_seen += rows
        if row_len > P:
            np_ = -(-row_len // P)
            assert slot_base == slots_seen, (name, p)
            slots_seen += rows * np_
            assert slot_base + rows * np_ <= h["slots"], (name, p)
            # one task per piece; a row's pieces consecutive and in order, rows in
            # order; the pieces tile [0, row_len) of their row and never cross it
            assert [t[0] for t in tasks] == [0] * (rows * np_), (name, p)
            assert [t[1] for t in tasks] == list(range(rows * np_)), (name, p)
            covered = 0
            for _, first in tasks:
                row, piece = divmod(first, np_)
                start = piece * P
                length = min(P, row_len - start)
                assert 0 <= row < rows and 0 < length <= P and start + length <= row_len, (name, p, first)
                covered += length
            assert covered == rows * row_len, (name, p)
        else:
            assert slot_base == -1, (name, p)
            nxt = 0
            for nrows, first in tasks:   # whole rows, each exactly once, in order
                assert first == nxt and 1 <= nrows <= 64, (name, p, first)
                assert nrows == 1 or nrows * row_len <= P, (name, p, first)
                nxt += nrows
            assert nxt == rows, (name, p)
    assert slots_seen == h["slots"] and buf_seen == h["buf_rows"], name


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_planner_invariants_under_sanitizers(tmp_path):
    """dfq_stats_plan.cpp + tests/native/stats_plan_check.cpp, nothing else linked,
    under AddressSanitizer and UBSan: no report; every element of every row covered
    exactly once; no piece crosses a row; a row's pieces consecutive and in order;
    every slot inside the workspace dfq_pair_stats_ws_bytes sizes; a pair's plan
    the same alone and as one of twenty."""
    lists = _lists()
    plans = _run_planner(tmp_path, lists)
    for (name, shapes), plan in zip(lists, plans):
        _check_plan(name, shapes, plan)
    by_name = {name: (shapes, plan) for (name, shapes), plan in zip(lists, plans)}
    # [65, 128]: 64 rows would be 8192 elements -- allowed; the task rule in numbers
    gpu_tasks = [t for t in by_name["gpu"][1]["tasks"] if t[0] == SHAPES.index((65, 128))]
    assert gpu_tasks == [(SHAPES.index((65, 128)), 64, 0), (SHAPES.index((65, 128)), 1, 64)]
    big = [t for t in by_name["gpu"][1]["tasks"] if t[0] == SHAPES.index((200, 3))]
    assert [t[1] for t in big] == [64, 64, 64, 8]
    # alone or one of twenty: the same tasks (but for the pair index)
    shapes20, plan20 = by_name["twenty"]
    for p, shape in enumerate(shapes20):
        alone = by_name["alone:%d" % (p + 5)]
        assert alone[0] == [shape]
        assert [t[1:] for t in alone[1]["tasks"]] == [t[1:] for t in plan20["tasks"] if t[0] == p], shape


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        pytest.skip("libdfq_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def test_argument_validation_without_a_device(lib):
    L = lib
    assert L.dfq_pair_stats_ws_bytes(None, 1) == -1
    d = (_lib.PairDesc * 2)()
    for k in range(2):
        d[k].x, d[k].y, d[k].rows_out, d[k].total_out, d[k].rows, d[k].row_len = 0x1000, 0x2000, 0x3000, 0x4000, 4, 9
    assert L.dfq_pair_stats_ws_bytes(d, 2) > 0
    assert L.dfq_pair_stats_ws_bytes(d, -1) == -1
    for field, bad in (("rows", 0), ("row_len", 0), ("rows", -3), ("x", None), ("y", None), ("x", 0x1002)):
        keep = getattr(d[1], field)
        setattr(d[1], field, bad)
        assert L.dfq_pair_stats_ws_bytes(d, 2) == -1, field
        assert L.dfq_pair_stats_batch(d, 2, 256, 1 << 20, None) == _lib.DFQ_ERR_INVALID, field
        setattr(d[1], field, keep)
    d[1].rows_out = None
    assert L.dfq_pair_stats_ws_bytes(d, 2) > 0          # totals only: allowed
    d[1].total_out = None
    assert L.dfq_pair_stats_ws_bytes(d, 2) == -1         # both outputs NULL
    d[1].rows_out, d[1].total_out = 0x3000, 0x4000
    # a split row needs partial slots: more workspace than the same elements in short rows
    d[1].rows, d[1].row_len = 1, 3 * P + 7
    split = L.dfq_pair_stats_ws_bytes(d, 2)
    d[1].rows, d[1].row_len = 3, P
    assert split > L.dfq_pair_stats_ws_bytes(d, 2) > 0
    # nothing to do: OK without a workspace, nothing launched
    assert L.dfq_pair_stats_batch(d, 0, None, 0, None) == _lib.DFQ_OK
    assert L.dfq_pair_stats_batch(None, 0, None, 0, None) == _lib.DFQ_OK
    assert L.dfq_pair_stats_batch(None, 1, None, 0, None) == _lib.DFQ_ERR_INVALID
    # the workspace is required and checked before anything touches the device
    need = L.dfq_pair_stats_ws_bytes(d, 2)
    assert L.dfq_pair_stats_batch(d, 2, None, need, None) == _lib.DFQ_ERR_WORKSPACE
    assert L.dfq_pair_stats_batch(d, 2, 256, 16, None) == _lib.DFQ_ERR_WORKSPACE
    assert L.dfq_abi_version() == 1


def test_pair_table_matches_the_ctypes_layout():
    assert quality._PAIR.itemsize == C.sizeof(_lib.PairDesc) == 48
    assert [f for f, _ in _lib.PairDesc._fields_] == list(quality._PAIR.names)


def test_sqnr_db():
    assert quality.sqnr_db(100.0, 1.0) == 20.0
    assert quality.sqnr_db(1.0, 4.0) == 10.0 * math.log10(0.25)
    assert quality.sqnr_db(0.0, 1.0) is None
    assert quality.sqnr_db(1.0, 0.0) is None
    assert quality.sqnr_db(0.0, 0.0) is None
    assert isinstance(quality.sqnr_db(np.float64(3.0), np.float64(2.0)), float)


def test_report_arithmetic_on_hand_made_records():
    # rows: {signal, noise, max_err, max_abs}
    a = np.array([[4.0, 0.04, 0.1, 2.0],     # 20 dB
                  [1.0, 0.10, 0.3, 1.0],     # 10 dB: the worst channel
                  [9.0, 0.00, 0.0, 0.5],     # lost nothing: never the worst
                  [1.0, 0.10, 0.2, 0.25]])   # 10 dB again: the first one stays the worst
    ta = np.array([15.0, 0.24, 0.3, 2.0])
    zero = np.zeros((2, 4))                  # an all-zero layer that stayed zero
    silent = np.array([[0.0, 0.5, 0.5, 0.0], [2.0, 0.5, 0.5, 1.0]])   # a zero channel that became noise
    ts = np.array([2.0, 1.0, 0.5, 1.0])
    rep = quality.build_report([("a", "Conv2d", (4, 3, 1, 1), a, ta), (7, "Linear", (2, 5), zero, np.zeros(4)),
                                ("s", "Conv2d", (2, 1, 3, 3), silent, ts)], {"bits_weight": 8})
    assert rep["format"] == "dfq-quality/1" and rep["config"] == {"bits_weight": 8}
    la, lz, ls = rep["layers"]
    assert (la["key"], la["type"], la["shape"], la["elements"]) == ("a", "Conv2d", [4, 3, 1, 1], 12)
    assert la["signal"] == 15.0 and la["noise"] == 0.24
    assert la["sqnr_db"] == 10.0 * math.log10(15.0 / 0.24)
    assert la["worst_channel"] == 1 and la["worst_channel_sqnr_db"] == 10.0
    assert la["max_abs_err"] == 0.3 and la["max_abs_weight"] == 2.0
    assert la["channel_precision_min"] == 0.125
    assert la["channel_precision_mean"] == (1.0 + 0.5 + 0.25 + 0.125) / 4
    assert lz["key"] == "7" and lz["elements"] == 10
    for f in ("sqnr_db", "worst_channel", "worst_channel_sqnr_db", "channel_precision_mean", "channel_precision_min"):
        assert lz[f] is None, f
    assert lz["signal"] == 0.0 and lz["noise"] == 0.0 and lz["max_abs_weight"] == 0.0
    # zero signal under non-zero noise: the worst there is, with no finite figure
    assert ls["worst_channel"] == 0 and ls["worst_channel_sqnr_db"] is None
    assert ls["sqnr_db"] == 10.0 * math.log10(2.0)
    assert ls["channel_precision_min"] == 0.0 and ls["channel_precision_mean"] == 0.5
    m = rep["model"]
    assert m["signal"] == (15.0 + 0.0) + 2.0 and m["noise"] == (0.24 + 0.0) + 1.0
    assert m["sqnr_db"] == 10.0 * math.log10(m["signal"] / m["noise"])
    assert m["worst_layer"] == "s" and m["elements"] == 12 + 10 + 18
    text = json.dumps(rep, allow_nan=False)   # the standard encoder, no infinities or NaNs
    assert json.loads(text) == rep
    empty = quality.build_report([], {})
    assert empty["layers"] == [] and empty["model"]["sqnr_db"] is None and empty["model"]["worst_layer"] is None
