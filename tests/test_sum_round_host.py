"""dfq_sum_round_batch without a GPU: the statement's invariants on every case, the
precondition that makes the GPU test mean something, the planner alone under
sanitizers, and the entry points' argument checks."""
import ctypes as C
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from data_free_quantization_amd import _lib
from tests import sum_round_cases as SC

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "data_free_quantization_amd" / "libdfq_hip.so"
CXX = next((c for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"), shutil.which("c++"))
            if c and os.path.exists(c)), None)
HALF, STEP = SC.HALF, SC.STEP


@pytest.mark.parametrize("gi", range(len(SC.GT)), ids=["G%d_T%d" % gt for gt in SC.GT])
def test_statement_invariants(gi):
    """On every case: the candidates exist (the statement asserts it), |E'| <= 2^23, every
    |e''| <= 2^24 + 2^23, every code within one step of nearest and on the grid, the
    kernel-stage flips within the candidates.  On the dense and normal cases with G >= 63
    nearest rounding alone leaves some row's |E| above 2^23 -- else the GPU test could pass
    on a kernel that never flips.  The dense rows flip about G / 2 kernels at T = 1."""
    for c in SC.group(gi):
        sym = c.mode in (1, 3)
        s, negmn, mn = SC.grid(c.x, c.bits, c.mode)
        r = SC.statement(c.x, s, negmn, mn, c.bits, sym, c.T)
        qmin, qmax = (-(1 << (c.bits - 1)), (1 << (c.bits - 1)) - 1) if sym else (0, (1 << c.bits) - 1)
        e2 = r["P"].sum(-1)
        assert (np.abs(e2.sum(-1)) <= HALF).all(), c.name
        assert (np.abs(e2) <= STEP + HALF).all(), c.name
        assert (np.abs(r["q"] - r["q0"]) <= 1).all() and r["q"].min() >= qmin and r["q"].max() <= qmax, c.name
        assert (np.abs(r["P0"]) <= HALF).all(), c.name
        m = np.maximum((r["P0"] > 0).sum((1, 2)), (r["P0"] < 0).sum((1, 2)))
        assert (r["flips"][:, 0] <= m).all() and (r["flips"][:, 1] <= c.G).all(), c.name
        E0 = r["P0"].sum((1, 2))
        if c.kind in ("dense", "normal") and c.G >= 63:
            assert (np.abs(E0) > HALF).any(), c.name
        if c.kind == "dense" and c.T == 1 and c.mode == 2 and c.G >= 63:
            assert (np.abs(r["flips"][:, 1] - 0.49 * c.G) <= 0.02 * c.G + 1).all(), c.name
        if c.kind == "clamp":
            if c.mode == 2:   # the even rows' maximum is clamped, the odd rows sit on the scale floor
                t_top = ((c.x[0::2, -1:] + negmn[0::2]) / s[0::2]).astype(np.float32)
                assert (t_top > qmax).all() and (r["P0"].reshape(c.x.shape)[0::2, -1] == 0).all(), c.name
                assert (s[1::2] == np.float32(1e-8)).all(), c.name


def test_the_cases_hold_every_value_and_the_take_back_path():
    cases = SC.all_cases()
    assert {c.x.shape[0] for c in cases} == set(SC.ROWS) and {c.bits for c in cases} == set(SC.BITS)
    assert {c.mode for c in cases} == {0, 1, 2, 3} and {c.offset for c in cases} == {0, 1}
    assert {(c.G, c.T) for c in cases} == set(SC.GT) and {c.kind for c in cases} == set(SC.KINDS)
    # a kernel of nine equal P = -0.1 step flips one tap up and overshoots; the row then asks
    # those kernels for a flip down they can only make by taking the flip back
    x = np.full((1, 63 * 9), 0.3, np.float32)
    x[0, 0], x[0, -1] = -1.0, 1.0
    s, negmn, mn = SC.grid(x, 4, 3)
    assert SC.statement(x, s, negmn, mn, 4, True, 9)["undone"] > 0
    assert any(SC.statement(c.x, *SC.grid(c.x, c.bits, c.mode), c.bits, c.mode in (1, 3), c.T)["undone"] > 0
               for c in cases if c.kind == "tie" and c.T > 1)


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_planner_under_sanitizers(tmp_path):
    """dfq_round_plan.cpp + tests/native/round_plan_check.cpp, nothing else linked, under
    AddressSanitizer and UBSan: no report; the shared inline functions and every LDS layout
    pass the program's own checks; rows, grid, LDS and workspace as the shapes dictate; a
    weight's job the same wherever it stands in the list."""
    shapes = [(c.x.shape[0], c.x.shape[1], c.T, c.bits, c.mode) for c in SC.all_cases()]
    lists = [shapes, shapes[::-1], [(2, 16384, 2, 4, 2)], [(1, 16385, 1, 4, 2)], [(1, 130, 65, 4, 2)],
             [(1, 10, 3, 4, 2)], [(1, 9, 9, 9, 2)], [(1, 9, 9, 1, 0)], [(0, 9, 9, 4, 0)], [(1, 9, 0, 4, 0)], [(1, 9, 9, 4, 4)]]
    text = []
    for sh in lists:
        text.append(str(len(sh)))
        text += ["%d %d %d %d %d" % s for s in sh]
    (tmp_path / "lists.txt").write_text("\n".join(text) + "\n")
    exe = tmp_path / "round_plan_check"
    csrc = ROOT / "data_free_quantization_amd" / "csrc"
    subprocess.run([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", str(ROOT / "include"), "-I", str(csrc),
                    str(ROOT / "tests" / "native" / "round_plan_check.cpp"), str(csrc / "dfq_round_plan.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe), str(tmp_path / "lists.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert not r.stderr, r.stderr[-4000:]   # no sanitizer report
    lines = r.stdout.splitlines()
    assert lines[0] == "self 0"
    heads = [dict(zip(w[2::2], map(int, w[3::2]))) for w in (l.split() for l in lines) if w[0] == "list"]
    jobs = [[] for _ in heads]
    li = -1
    for w in (l.split() for l in lines[1:]):
        li += w[0] == "list"
        if w[0] == "job":
            jobs[li].append(tuple(int(v) for v in w[3::2]))
    assert [h["rc"] for h in heads] == [0, 0, 0, _lib.DFQ_ERR_UNSUPPORTED, _lib.DFQ_ERR_UNSUPPORTED, _lib.DFQ_ERR_SHAPE] + \
        [_lib.DFQ_ERR_INVALID] * 5
    for h, sh, jb in zip(heads[:3], lists[:3], jobs[:3]):
        assert h["total_rows"] == sum(s[0] for s in sh) and h["grid"] == min(h["total_rows"], 256)
        assert h["n_tensor"] == sum(s[4] < 2 for s in sh)
        G = [s[1] // s[2] for s in sh]
        assert h["lds"] == max(4 * g * (1 if s[2] == 1 else (s[2] | 1)) + (4 * g if s[2] > 1 else 0) + -(-s[1] // 16) * 16
                               for g, s in zip(G, sh))
        assert h["o_range"] % 256 == 0 and h["o_range"] >= h["job_bytes"] * len(sh)
        assert h["o_range"] + 8 * len(sh) <= h["total"] <= h["ws"] and h["total"] % 256 == 0
        row0 = np.concatenate([[0], np.cumsum([s[0] for s in sh])[:-1]])
        assert jb == [(int(r0), s[1], s[2], s[4] & 1, 2 * p if s[4] < 2 else -1)
                      for p, (r0, s) in enumerate(zip(row0, sh))]
    assert heads[0]["total_rows"] > heads[0]["grid"]   # the grid-stride loop over rows runs in the GPU tests
    assert heads[2]["lds"] == 147456   # the largest layout: khw 2 at the longest row
    assert [j[1:4] for j in jobs[0]] == [j[1:4] for j in jobs[1]][::-1]


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        pytest.skip("libdfq_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def test_argument_validation_without_a_device(lib):
    L = lib
    d = (_lib.SumRoundDesc * 2)()
    for k in range(2):
        d[k].src, d[k].dst, d[k].codes, d[k].scale, d[k].zero, d[k].flips = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
        d[k].rows, d[k].row_len, d[k].khw, d[k].bits, d[k].mode = 4, 18, 9, 4, _lib.DFQ_CHANNEL_SYM
    assert L.dfq_sum_round_ws_bytes(None, 1) == -1 and L.dfq_sum_round_ws_bytes(d, -1) == -1
    need = L.dfq_sum_round_ws_bytes(d, 2)
    assert need >= 256
    bad = [("bits", 1, -1), ("bits", 9, -1), ("mode", 4, -1), ("mode", -1, -1), ("rows", 0, -1), ("row_len", 0, -1),
           ("khw", 0, -1), ("reserved", 1, -1), ("src", None, -1), ("src", 0x1002, -1), ("dst", 0x2002, -1),
           ("scale", 0x4001, -1), ("zero", 0x5002, -1), ("flips", 0x6003, -1),
           ("khw", 4, _lib.DFQ_ERR_SHAPE), ("row_len", 9 * 1821, _lib.DFQ_ERR_UNSUPPORTED)]   # 16389 > DFQ_SR_MAX_ROW
    for field, value, rc in bad:
        keep = getattr(d[1], field)
        setattr(d[1], field, value)
        assert L.dfq_sum_round_ws_bytes(d, 2) == -1, (field, value)
        assert L.dfq_sum_round_batch(d, 2, 256, 1 << 20, None) == rc, (field, value)
        setattr(d[1], field, keep)
        assert L.dfq_sum_round_ws_bytes(d, 2) == need, (field, value)
    for field, value in (("bits", 2), ("bits", 8), ("khw", 1), ("khw", 18), ("row_len", 9 * 1820)):
        keep = getattr(d[1], field)
        setattr(d[1], field, value)
        assert L.dfq_sum_round_ws_bytes(d, 2) > 0, (field, value)
        setattr(d[1], field, keep)
    # any output may be NULL, but not all of them
    d[1].dst = d[1].codes = d[1].scale = d[1].zero = None
    assert L.dfq_sum_round_ws_bytes(d, 2) == need
    d[1].flips = None
    assert L.dfq_sum_round_ws_bytes(d, 2) == -1
    assert L.dfq_sum_round_batch(d, 2, 256, 1 << 20, None) == _lib.DFQ_ERR_INVALID
    d[1].codes = 0x3000
    # nothing to do: OK without a workspace, nothing launched
    assert L.dfq_sum_round_batch(d, 0, None, 0, None) == _lib.DFQ_OK
    assert L.dfq_sum_round_batch(None, 0, None, 0, None) == _lib.DFQ_OK
    assert L.dfq_sum_round_batch(None, 1, None, 0, None) == _lib.DFQ_ERR_INVALID
    assert L.dfq_sum_round_batch(d, -1, 256, 1 << 20, None) == _lib.DFQ_ERR_INVALID
    # the workspace is required and checked before anything touches the device
    assert L.dfq_sum_round_batch(d, 2, None, need, None) == _lib.DFQ_ERR_WORKSPACE
    assert L.dfq_sum_round_batch(d, 2, 256, need - 1, None) == _lib.DFQ_ERR_WORKSPACE
    assert L.dfq_sum_round_batch(d, 2, 128, need, None) == _lib.DFQ_ERR_INVALID   # misaligned workspace


def test_python_layer_without_a_device():
    import re
    import torch
    from data_free_quantization_amd import main_dfq, rounding
    from data_free_quantization_amd.utils.layer_transform import quantize_targ_layer
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        rounding.sum_round([rounding.SumRoundItem(torch.randn(4, 4))])
    assert rounding.sum_round([]) == []
    assert rounding._SR.itemsize == C.sizeof(_lib.SumRoundDesc) == 80
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "dfq_hip.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct dfq_sum_round_desc\s*\{(.*?)\}\s*dfq_sum_round_desc;", text, flags=re.S).group(1)
    assert re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*;", body) == [f for f, _ in _lib.SumRoundDesc._fields_]
    for kw in ({"weight_format": "mxfp4"}, {"clip": (-1, 1)}, {"shard": True}, {"rounding": "up"}):
        with pytest.raises(ValueError, match="rounding"):
            quantize_targ_layer({}, 4, 8, [torch.nn.Linear], **{"rounding": "sum", **kw})
    assert main_dfq.get_argument(["--quantize", "--rounding", "sum"]).rounding == "sum"
    assert main_dfq.get_argument(["--quantize"]).rounding == "nearest"
    for argv in (["--rounding", "sum"], ["--quantize", "--rounding", "sum", "--bc_mode", "fused"],
                 ["--quantize", "--rounding", "sum", "--weight_format", "mxfp4"],
                 ["--quantize", "--rounding", "sum", "--world_size", "2"]):
        with pytest.raises(SystemExit):
            main_dfq.get_argument(argv)
