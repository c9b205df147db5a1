"""dfq_mx_quantize_batch without a GPU: the numpy statement's own preconditions, the
fp32-multiply form of the scaling, an independent check of the FP8 grid, the torch
dequantizer, the planner alone under sanitizers, the entry points' argument checks
and the command-line flag."""
import ctypes as C
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from data_free_quantization_amd import _lib, mx
from tests import mx_cases as MC

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "data_free_quantization_amd" / "libdfq_hip.so"
CXX = next((c for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"), shutil.which("c++"))
            if c and os.path.exists(c)), None)
CAP, ECAP = _lib.DFQ_MX_TASK_ELEMS, _lib.DFQ_MX_ESUM_TASK_ELEMS


def test_the_case_list_meets_the_statements_preconditions():
    cases = MC.all_cases()
    for fmt, (_, _, sign_bit, _) in MC.FORMATS.items():
        mine = [c for c in cases if c.fmt == fmt]
        # a tie in each direction, a saturated element, a signed zero code, a partial block
        assert sum(int(c.ref["tie_down"].sum()) for c in mine) > 0, fmt
        assert sum(int(c.ref["tie_up"].sum()) for c in mine) > 0, fmt
        assert sum(int(c.ref["saturated"].sum()) for c in mine) > 0, fmt
        assert any((c.ref["element_codes"] == sign_bit).any() for c in mine), fmt
        assert any(c.x.shape[1] % MC.BLOCK for c in mine), fmt
        # negative values that round to zero (not only -0 inputs) are among the signed zeros
        assert any(((c.ref["y"] == 0) & (c.x < 0)).any() for c in mine), fmt
        # every axis value of the issue
        grid = [c for c in mine if c.name.startswith("grid_")]
        assert {c.x.shape for c in grid} == {(r, l) for r in MC.ROWS for l in MC.ROW_LENS}, fmt
        assert {c.offset for c in mine} == set(MC.OFFSETS) and {c.khw for c in mine} >= set(MC.KHWS), fmt
        assert {c.khw for c in mine if c.want_esum} >= set(MC.KHWS), fmt
        assert {c.outputs for c in mine} == set(MC.OUTPUTS), fmt
    for c in cases:
        a = np.abs(c.x[c.x != 0])
        assert np.isfinite(c.x).all() and (a.size == 0 or a.min() >= MC.MIN_MAG), c.name
        assert (c.ref["scales"] != 0xFF).all(), c.name
    # the extremes: magnitudes at 2^-100 and above 2^119 in one row
    ext = next(c for c in cases if c.name == "extremes_mxfp4")
    assert np.abs(ext.x[ext.x != 0]).min() == 2.0 ** -100 and np.abs(ext.x).max() > 2.0 ** 119
    # all-zero blocks take scale byte 0
    z = next(c for c in cases if c.name == "negzeros_mxfp8")
    assert (z.ref["scales"] == 0).all() and (z.ref["codes"] == 0x80)[:, 0].all() and np.signbit(z.ref["y"]).all()
    assert (z.ref["codes"][:, 1, 8:] == 0).all()   # the padding of the partial block is +0 codes


def test_fp32_multiply_gives_the_exact_forms_codes():
    """|x| * 2^-X as one float32 multiply (what the kernel does) against the exact
    product: same codes, scales and values on every case."""
    for c in MC.all_cases():
        got = MC.statement(c.x, c.fmt, fp32_multiply=True)
        for k in ("codes", "scales"):
            assert np.array_equal(got[k], c.ref[k]), (c.name, k)
        assert np.array_equal(got["y"].view(np.uint32), c.ref["y"].view(np.uint32)), c.name


def test_fp8_grid_agrees_with_torch_float8():
    """The explicit E4M3 table and its ties-to-even-code rounding against torch's
    float8_e4m3fn cast of clamp(v, -448, 448)."""
    n = 0
    for c in MC.all_cases():
        if c.fmt != "mxfp8":
            continue
        v = MC.statement(c.x, c.fmt, fp32_multiply=True)["v"].astype(np.float32)   # float32 values, widened
        neg = (c.ref["element_codes"] & 0x80) != 0
        sv = torch.from_numpy(np.where(neg, -v, v).astype(np.float32)).clamp(-448, 448)
        bits = sv.to(torch.float8_e4m3fn).view(torch.uint8).numpy()
        assert np.array_equal(bits, c.ref["element_codes"]), c.name
        n += bits.size
    assert n > 100000


def test_the_table_is_the_formats_encoding():
    # E2M1 nibble s e e m and E4M3 byte s eeee mmm decode to the tables' magnitudes
    for code in range(8):
        e, m = code >> 1, code & 1
        assert MC.FP4_MAGS[code] == (m * 0.5 if e == 0 else (1 + m * 0.5) * 2.0 ** (e - 1))
    t = mx._tables("mxfp8", "cpu").numpy()
    assert np.array_equal(t[:127].astype(np.float64), MC.FP8_MAGS) and np.isnan(t[127])
    assert np.array_equal(t[128:255], -t[:127]) and np.signbit(t[128])
    assert np.array_equal(mx._tables("mxfp4", "cpu").numpy()[:8].astype(np.float64), MC.FP4_MAGS)
    assert mx.bits_per_weight("mxfp4") == 4.25 and mx.bits_per_weight("mxfp8") == 8.25


def test_mx_dequantize_reproduces_the_statement_on_the_cpu():
    for c in MC.all_cases():
        y = mx.mx_dequantize(torch.from_numpy(c.ref["codes"]), torch.from_numpy(c.ref["scales"]), c.x.shape, c.fmt)
        assert y.dtype == torch.float32 and tuple(y.shape) == c.x.shape
        assert np.array_equal(y.numpy().view(np.uint32), c.ref["y"].view(np.uint32)), c.name
    c = MC.all_cases()[0]
    y = mx.mx_dequantize(torch.from_numpy(c.ref["codes"]), torch.from_numpy(c.ref["scales"]), (c.x.shape[0], 1, c.x.shape[1]),
                         c.fmt)
    assert tuple(y.shape) == (c.x.shape[0], 1, c.x.shape[1])
    with pytest.raises(ValueError):
        mx.mx_dequantize(torch.zeros(1, 1, 16, dtype=torch.uint8), torch.zeros(1, 1, dtype=torch.uint8), (1, 32), "mxfp6")


# ---- the planner on its own --------------------------------------------------
def _shape_list():
    """(rows, row_len, khw, esum, aligned): the cases' shapes and MobileNetV2's layers."""
    out = []
    for i, c in enumerate(MC.all_cases()):
        out.append((c.x.shape[0], c.x.shape[1], c.khw, int(c.want_esum), int(c.offset == 0)))
    out += [(r, l, k, 1, 1) for r, l, k in MC.mobilenetv2_shapes()]
    out += [(2, 5040, 63, 1, 1), (1, 1 << 20, 1, 0, 1), (70000, 3, 3, 1, 0)]
    seen, uniq = set(), []
    for s in out:
        if s not in seen:
            seen.add(s)
            uniq.append(s)
    return uniq


def _lists():
    shapes = _shape_list()
    return [("all", shapes), ("reversed", shapes[::-1]), ("twenty", shapes[20:40])] + \
        [("alone:%d" % i, [s]) for i, s in enumerate(shapes)]


def _run_planner(tmp_path, lists):
    text = []
    for _, shapes in lists:
        text.append(str(len(shapes)))
        text += ["%d %d %d %d %d" % s for s in shapes]
    (tmp_path / "lists.txt").write_text("\n".join(text) + "\n")
    exe = tmp_path / "mx_plan_check"
    csrc = ROOT / "data_free_quantization_amd" / "csrc"
    subprocess.run([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", str(ROOT / "include"), "-I", str(csrc),
                    str(ROOT / "tests" / "native" / "mx_plan_check.cpp"), str(csrc / "dfq_mx_plan.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe), str(tmp_path / "lists.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert not r.stderr, r.stderr[-4000:]   # no sanitizer report
    plans = []
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "list":
            plans.append({"head": {w[i]: int(w[i + 1]) for i in range(2, len(w), 2)}, "jobs": [], "tasks": []})
        elif w[0] == "job":
            plans[-1]["jobs"].append({w[i]: int(w[i + 1]) for i in range(2, len(w), 2)})
        else:
            assert w[0] == "task", line
            plans[-1]["tasks"].append(tuple(int(t) for t in w[1:]))
    assert len(plans) == len(lists)
    return plans


def _lcm32(k):
    return 32 * k // np.gcd(32, k)


def _check_plan(name, shapes, plan):
    h = plan["head"]
    assert h["rc"] == _lib.DFQ_OK, name
    assert h["tasks"] == len(plan["tasks"]) and len(plan["jobs"]) == len(shapes), name
    assert h["o_tasks"] >= h["job_bytes"] * len(shapes) and h["o_tasks"] % 256 == 0 and h["total"] % 256 == 0, name
    assert h["o_tasks"] + h["task_bytes"] * h["tasks"] <= h["total"] <= h["ws"], name
    assert [t[0] for t in plan["tasks"]] == sorted(t[0] for t in plan["tasks"]), name   # list order
    by_job = {}
    for job, nrows, row, col in plan["tasks"]:
        by_job.setdefault(job, []).append((nrows, row, col))
    lds = 0
    for p, ((rows, row_len, khw, esum, aligned), job) in enumerate(zip(shapes, plan["jobs"])):
        lds_e = bool(esum) and khw > 1
        lds += lds_e
        cap = ECAP if lds_e else CAP
        lp = -(-row_len // 32) * 32
        assert job["cap"] == cap and job["vec"] == int(bool(aligned) and row_len % 4 == 0), (name, p)
        if lp > cap:
            piece = job["piece"]
            unit = _lcm32(khw) if lds_e else 32
            assert 0 < piece <= cap and piece % unit == 0 and piece + unit > cap, (name, p)
            want = [(0, r, c) for r in range(rows) for c in range(0, row_len, piece)]
            assert by_job[p] == want, (name, p)   # each row's pieces in order, tiling [0, row_len) once
        else:
            per = job["rows_per_task"]
            assert per == cap // lp >= 1, (name, p)
            nxt = 0
            for nrows, row, col in by_job[p]:   # whole rows, each exactly once, in order
                assert col == 0 and row == nxt and 1 <= nrows <= per and nrows * lp <= cap, (name, p, row)
                nxt += nrows
            assert nxt == rows, (name, p)
    assert lds == h["lds_jobs"], name


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_planner_invariants_under_sanitizers(tmp_path):
    """dfq_mx_plan.cpp + tests/native/mx_plan_check.cpp, nothing else linked, under
    AddressSanitizer and UBSan: no report; the tasks tile every tensor exactly once in
    whole MX blocks and whole khw groups, no task holds more padded elements than
    its LDS copy and index arithmetic allow, the tables lie inside the workspace
    dfq_mx_quantize_ws_bytes sizes, and a tensor's plan is the same alone, in the
    reversed list and as one of twenty."""
    lists = _lists()
    plans = _run_planner(tmp_path, lists)
    for (name, shapes), plan in zip(lists, plans):
        _check_plan(name, shapes, plan)
    by_name = {name: (shapes, plan) for (name, shapes), plan in zip(lists, plans)}
    shapes_all = by_name["all"][0]
    for other in ("reversed", "twenty"):
        shapes_o, plan_o = by_name[other]
        for p, shape in enumerate(shapes_o):
            alone = by_name["alone:%d" % shapes_all.index(shape)]
            assert [t[1:] for t in alone[1]["tasks"]] == [t[1:] for t in plan_o["tasks"] if t[0] == p], (other, shape)
    # the rule in numbers: [65, 100] pads rows to 128 -> 32 rows a task; depthwise [96, 9] with
    # error sums: 2048 / 32 = 64 rows a task; [2, 3136] with khw 49: pieces of 1568
    def alone(rows, row_len, khw, esum):
        s = next(s for s in shapes_all if s[:4] == (rows, row_len, khw, esum))
        return by_name["alone:%d" % shapes_all.index(s)][1]["tasks"]

    assert alone(65, 100, 1, 1) == [(0, 32, 0, 0), (0, 32, 32, 0), (0, 1, 64, 0)]
    assert alone(96, 9, 9, 1) == [(0, 64, 0, 0), (0, 32, 64, 0)]
    assert alone(2, 3136, 49, 1) == [(0, 0, 0, 0), (0, 0, 0, 1568), (0, 0, 1, 0), (0, 0, 1, 1568)]


# ---- the entry points' argument checks ----------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        pytest.skip("libdfq_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def _good(n=2):
    d = (_lib.MxDesc * n)()
    for k in range(n):
        d[k].src, d[k].dst, d[k].codes, d[k].scales, d[k].esum = 0x1000, 0x1000, 0x2000, 0x3000, 0x4000
        d[k].rows, d[k].row_len, d[k].khw, d[k].format, d[k].flags = 4, 18, 9, _lib.DFQ_MX_FP4_E2M1, 0
    return d


def test_argument_validation_without_a_device(lib):
    L = lib
    assert L.dfq_mx_quantize_ws_bytes(None, 1) == -1
    d = _good()
    assert L.dfq_mx_quantize_ws_bytes(d, 2) > 0
    assert L.dfq_mx_quantize_ws_bytes(d, -1) == -1
    assert L.dfq_mx_quantize_batch(d, -1, 256, 1 << 20, None) == _lib.DFQ_ERR_INVALID
    bad = [("format", 2), ("format", -1), ("flags", 1), ("flags", -1), ("rows", 0), ("rows", -3), ("row_len", 0),
           ("row_len", 1 << 41), ("khw", 0), ("khw", -9), ("src", None), ("src", 0x1002), ("dst", 0x1001),
           ("esum", 0x4002)]
    for name, value in bad:
        keep = getattr(d[1], name)
        setattr(d[1], name, value)
        assert L.dfq_mx_quantize_ws_bytes(d, 2) == -1, (name, value)
        assert L.dfq_mx_quantize_batch(d, 2, 256, 1 << 20, None) == _lib.DFQ_ERR_INVALID, (name, value)
        setattr(d[1], name, keep)
        assert L.dfq_mx_quantize_ws_bytes(d, 2) > 0, (name, value)
    # every output may be NULL, but not all of them
    for name in ("dst", "codes", "scales", "esum"):
        keep = getattr(d[1], name)
        setattr(d[1], name, None)
        assert L.dfq_mx_quantize_ws_bytes(d, 2) > 0, name
        setattr(d[1], name, keep)
    d[1].dst = d[1].codes = d[1].scales = d[1].esum = None
    assert L.dfq_mx_quantize_ws_bytes(d, 2) == -1
    assert L.dfq_mx_quantize_batch(d, 2, 256, 1 << 20, None) == _lib.DFQ_ERR_INVALID
    d = _good()
    # error sums need whole khw groups per row; without esum khw is not looked at
    d[1].row_len = 20
    assert L.dfq_mx_quantize_ws_bytes(d, 2) == -1
    assert L.dfq_mx_quantize_batch(d, 2, 256, 1 << 20, None) == _lib.DFQ_ERR_SHAPE
    d[1].esum = None
    assert L.dfq_mx_quantize_ws_bytes(d, 2) > 0
    # a long row whose khw groups fit no piece (lcm(32, 65) > 2048) is refused; a short one is served
    d = _good()
    d[1].rows, d[1].row_len, d[1].khw = 2, 65 * 40, 65
    assert L.dfq_mx_quantize_batch(d, 2, 256, 1 << 20, None) == _lib.DFQ_ERR_UNSUPPORTED
    d[1].row_len = 65 * 30
    assert L.dfq_mx_quantize_ws_bytes(d, 2) > 0
    d[1].row_len, d[1].khw = 64 * 100, 64
    assert L.dfq_mx_quantize_ws_bytes(d, 2) > 0
    # nothing to do: OK without a workspace, nothing launched
    d = _good()
    assert L.dfq_mx_quantize_batch(d, 0, None, 0, None) == _lib.DFQ_OK
    assert L.dfq_mx_quantize_batch(None, 0, None, 0, None) == _lib.DFQ_OK
    assert L.dfq_mx_quantize_batch(None, 1, None, 0, None) == _lib.DFQ_ERR_INVALID
    # the workspace is required and checked before anything touches the device
    need = L.dfq_mx_quantize_ws_bytes(d, 2)
    d[1].rows = 100000
    more = L.dfq_mx_quantize_ws_bytes(d, 2)
    assert more > need >= 256
    assert L.dfq_mx_quantize_batch(d, 2, None, more, None) == _lib.DFQ_ERR_WORKSPACE
    assert L.dfq_mx_quantize_batch(d, 2, 256, 16, None) == _lib.DFQ_ERR_WORKSPACE
    assert L.dfq_mx_quantize_batch(d, 2, 256, more - 1, None) == _lib.DFQ_ERR_WORKSPACE
    assert L.dfq_mx_quantize_batch(d, 2, 128, more, None) == _lib.DFQ_ERR_INVALID   # misaligned workspace


def test_mx_table_matches_the_ctypes_layout_and_the_header():
    assert mx._MX.itemsize == C.sizeof(_lib.MxDesc) == 72
    assert [f for f, _ in _lib.MxDesc._fields_] == list(mx._MX.names)
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "dfq_hip.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct dfq_mx_desc\s*\{(.*?)\}\s*dfq_mx_desc;", text, flags=re.S).group(1)
    assert re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*;", body) == [f for f, _ in _lib.MxDesc._fields_]
    assert re.search(r"DFQ_MX_BLOCK = (\d+)", text).group(1) == str(_lib.DFQ_MX_BLOCK) == str(MC.BLOCK)
    assert re.search(r"DFQ_MX_FP4_E2M1 = (\d+), DFQ_MX_FP8_E4M3 = (\d+)", text).groups() == ("0", "1")
    assert re.search(r"DFQ_MX_TASK_ELEMS = (\d+), DFQ_MX_ESUM_TASK_ELEMS = (\d+)", text).groups() == (str(CAP), str(ECAP))
    assert _lib.load is not None and "#define DFQ_ABI_VERSION 1" in text


def test_python_rejects_cpu_tensors_and_bad_formats():
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        mx.mx_quantize([mx.MXItem(torch.randn(4, 4), dst=torch.empty(4, 4))])
    assert mx.mx_quantize([]) == []
    assert mx.is_mx("mxfp4") and mx.is_mx("mxfp8") and not mx.is_mx("int")
    with pytest.raises(ValueError):
        mx.is_mx("mxfp6")


def test_cli_flag():
    from data_free_quantization_amd import main_dfq
    assert main_dfq.get_argument(["--quantize"]).weight_format == "int"
    a = main_dfq.get_argument(["--quantize", "--weight_format", "mxfp4", "--bc_mode", "fused"])
    assert a.weight_format == "mxfp4"
    assert main_dfq.get_argument(["--quantize", "--weight_format", "mxfp8", "--clip_weight"]).weight_format == "mxfp8"
    for argv in (["--quantize", "--weight_format", "mxfp6"], ["--weight_format", "mxfp4"],
                 ["--quantize", "--weight_format", "mxfp4", "--clip_search"],
                 ["--quantize", "--weight_format", "mxfp4", "--bc_mode", "reference"],
                 ["--quantize", "--weight_format", "mxfp8", "--bc_mode", "fused", "--clip_weight"],
                 ["--quantize", "--weight_format", "mxfp4", "--world_size", "2"]):
        with pytest.raises(SystemExit):
            main_dfq.get_argument(argv)
