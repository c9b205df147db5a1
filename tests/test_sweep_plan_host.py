"""The sweep planner without a GPU (csrc/dfq_sweep_plan.cpp): built on its own as
plain C++ with tests/native/sweep_plan_check.cpp and run under AddressSanitizer and
UBSan.  The program checks, in C++, every invariant sweep_main_kernel and
sweep_reduce_kernel take on trust from the task tables (coverage, alignment, the
whole-row / block-row / row-group / slot-piece rules, the records, both workspace
layouts) for the list planner and the single-tensor planner, under every
diagnostics switch of the planner, and prints one line per plan.

Every line must equal tests/golden/sweep_plan_tables.json, recorded from the
planner as it stood inside dfq_sweep.hip before it moved: the fixture is the
definition of "the same tables" (the digest covers every DevTensor and DevTask
byte).  The fixture holds each list's distinct lines once, each with the switches
it was printed under (most single-tensor plans are the same under most switches).  `python tests/test_sweep_plan_host.py --record` rewrites it from the
current planner; a re-record needs a stated reason in the change that makes it,
since it redefines what every plan of the library is compared with.

The product library's dfq_sweep_plan_ws_bytes / dfq_quantize_ws_bytes (pure host
code, called through ctypes) must return the fixture's totals and return codes."""
import ctypes as C
import functools
import json
import os
import shutil
import subprocess
from pathlib import Path

import pytest

from data_free_quantization_amd import _lib, zoo

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "data_free_quantization_amd" / "csrc"
LIB = ROOT / "data_free_quantization_amd" / "libdfq_hip.so"
FIXTURE = Path(__file__).resolve().parent / "golden" / "sweep_plan_tables.json"
CXX = next((c for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"), shutil.which("c++"))
            if c and os.path.exists(c)), None)
SWITCHES = ("product", "group_rows", "no_blockrow", "span4096", "shuffle7", "v0", "v4", "v8", "v11")
# the checker's stand-in addresses (sweep_plan_check.cpp) and its own input flag
SRC, DST, CODES, SCALE, ZERO, ESUM, RANGE = (k << 44 for k in range(1, 8))
NULL_RANGE = 0x100   # DFQ_DEVICE_RANGE with range_enc NULL

INVALID, UNSUPPORTED, SHAPE = _lib.DFQ_ERR_INVALID, _lib.DFQ_ERR_UNSUPPORTED, _lib.DFQ_ERR_SHAPE
# Single-tensor lists: `rows row_len khw bits mode flags want_esum src_byte_offset`
# (flags: 2 given range, 8 packed, 16 device range) and what the product planner
# makes of each, counted on the planner before it moved.
SINGLES = {
    "32 9 9 8 3 0 1 0": dict(main=1, wholerow=1),                       # depthwise rows, one lane per row (scalar)
    "64 27 9 8 3 0 1 0": dict(main=2, wholerow=2),                      # short scalar rows
    "96 576 9 8 3 0 1 0": dict(main=48, wholerow=48),                   # vec4 rows
    "16 1152 9 8 3 0 1 0": dict(main=16, wholerow=16),
    "5 7 1 8 3 0 1 0": dict(main=1, wholerow=1),                        # scalar path
    "3 2880 9 8 3 0 1 0": dict(main=8, blockrow=8, padding=2),          # block-row pairs, odd row count
    "4 4608 9 8 3 0 1 0": dict(main=16, blockrow=16, padding=0),        # block-row quads
    "2 20480 1 8 3 0 1 0": dict(slotpieces=28, slots=2, reduce=4),      # rows past four pieces
    "2 9216 9 8 3 0 1 0": dict(slotpieces=14, slots=2, reduce=2),
    "3 1000 1 8 0 0 0 0": dict(main=4, blockrow=4, padding=2),          # per-tensor range, small
    "64 1000 1 8 0 0 0 0": dict(slotpieces=42, slots=1, reduce=5),      # per-tensor range, large
    "64 1000 1 8 1 2 0 0": dict(main=42, slotpieces=0, slots=0, reduce=0, blockrow=0, wholerow=0),   # given range
    "64 1000 1 8 0 16 0 0": dict(main=42, slotpieces=0, slots=0, reduce=0, blockrow=0, wholerow=0),  # device range
    "6 9 9 4 2 8 0 0": dict(main=1, wholerow=1),                        # packed, odd rows in pairs
    "2 1025 1 4 2 8 0 0": dict(rc=UNSUPPORTED),                         # packed, odd rows that cannot pair
    "1 1025 1 4 2 8 0 0": dict(rc=0),
    "2 1600 1600 8 3 0 1 0": dict(variant=6, main=2),                   # KH*KW above the small tasks
    "2 2500 2500 8 3 0 1 0": dict(rc=UNSUPPORTED),                      # KH*KW above every task
    "16 64 1 8 3 0 1 4": dict(rc=0),                                    # source off 16-byte alignment: vec4 = 0
    "0 64 1 8 3 0 0 0": dict(rc=0, main=0, reduce=0),                   # empty tensor
    "4 64 1 1 3 0 0 0": dict(rc=INVALID),                               # bits 1
    "4 64 1 17 3 0 0 0": dict(rc=INVALID),
    "4 64 1 8 4 0 0 0": dict(rc=INVALID),                               # mode 4
    "4 64 0 8 3 0 0 0": dict(rc=INVALID),                               # khw 0
    "4 64 1 8 3 2 0 0": dict(rc=INVALID),                               # channel mode with a given range
    "4 64 1 8 0 18 0 0": dict(rc=INVALID),                              # given and device range together
    "4 64 1 8 3 8 0 0": dict(rc=INVALID),                               # packed at 8 bits
    "4 64 3 8 3 0 1 0": dict(rc=SHAPE),                                 # 64 % 3 with error sums
    "2147483648 1 1 8 3 0 0 0": dict(rc=UNSUPPORTED),                   # rows above INT32_MAX
    "4 64 1 8 0 %d 0 0" % (16 | NULL_RANGE): dict(rc=INVALID),          # device range without its words
}
# (weights, main tasks, block-row entries, variant): tests/test_gpu_sweep_small.py's expectations
MODEL_LISTS = {"mobilenetv2 x1": (53, 2862, 0, 10), "mobilenetv2 x2": (106, 4476, 0, 6),
               "resnet50 x1": (54, 16721, 9216, 6), "deeplab x1": (61, 3930, 2560, 6)}


@functools.lru_cache(maxsize=None)
def _model(name):
    """Every Conv2d / Linear weight, per-channel symmetric INT8 with error sums."""
    out = []
    for m in zoo.target_layers(zoo.build(name, seed=0, relu=True)):
        s = tuple(m.weight.shape)
        khw = s[2] * s[3] if len(s) == 4 else 1
        out.append((s[0], m.weight.numel() // s[0], khw, 8, _lib.DFQ_CHANNEL_SYM, 0, 1, 0))
    return out


@functools.lru_cache(maxsize=None)
def _lists():
    """[(name, [descriptor tuples])] in the order the program sees them."""
    out = [(k, [tuple(int(v) for v in k.split())]) for k in SINGLES]
    small = ["2 1600 1600 8 3 0 1 0", "16 72 9 8 3 0 1 0", "5 7 1 8 3 0 1 0"]
    out.append(("small list that cannot be rebuilt at 1,536", [tuple(int(v) for v in k.split()) for k in small]))
    out.append(("n = 0", []))
    for name in MODEL_LISTS:
        model, copies = name.split(" x")
        out.append((name, _model(model) * int(copies)))
    return out


def _run_planner(tmp_path, planner=CSRC / "dfq_sweep_plan.cpp"):
    """{list name: the program's lines for it, list / tensor indices as the list's own}."""
    text = []
    for _, descs in _lists():
        text.append(str(len(descs)))
        text += [" ".join(map(str, d)) for d in descs]
    (tmp_path / "lists.txt").write_text("\n".join(text) + "\n")
    exe = tmp_path / "sweep_plan_check"
    subprocess.run([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-DDFQ_DIAGNOSTICS", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", str(ROOT / "include"), "-I", str(CSRC),
                    str(ROOT / "tests" / "native" / "sweep_plan_check.cpp"), str(planner), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe), str(tmp_path / "lists.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert not r.stderr, r.stderr[-4000:]   # no sanitizer report, no broken invariant
    names = [name for name, _ in _lists()]
    out = {name: {} for name in names}
    for line in r.stdout.splitlines():
        kind, idx, switch, rest = line.split(" ", 3)
        li, _, t = idx.partition(".")
        out[names[int(li)]].setdefault(" ".join(([kind, t] if t else [kind]) + [rest]), []).append(switch)
    return {name: {line: " ".join(sw) for line, sw in lines.items()} for name, lines in out.items()}


FIELDS = ("rc", "variant", "main", "reduce", "slots", "blockrow", "wholerow", "slotpieces", "padding", "o_reduce",
          "o_main", "o_slots", "total")   # then the digest; a single-tensor line's o_slots is its o_tensor


def _plans(lines):
    """{line: switches} -> [(kind, tensor or None, switch, {field: int, 'digest': str})], one per printed line."""
    out = []
    for line, switches in lines.items():
        w = line.split()
        kind, t = w[0], None
        if kind == "single":
            t = int(w[1])
            w = w[1:]
        assert len(w) == len(FIELDS) + 2, line
        f = dict(zip(FIELDS, map(int, w[1:-1])), digest=w[-1])
        out += [(kind, t, sw, f) for sw in switches.split()]
    return out


def _product(lines):
    """The product switch's plans of one list: (list fields, {tensor: single fields})."""
    head, singles = None, {}
    for kind, t, switch, f in _plans(lines):
        if switch == "product":
            if kind == "list":
                head = f
            else:
                singles[t] = f
    return head, singles


@pytest.fixture(scope="module")
def fixture():
    data = json.loads(FIXTURE.read_text())
    assert next(iter(data)) == "recorded_from" and len(data["recorded_from"]) == 40
    return data["lists"]


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_planner_alone_under_sanitizers(tmp_path, fixture):
    """No sanitizer report, no broken invariant (exit status 0, empty stderr), and
    every printed line equal to the fixture's."""
    got = _run_planner(tmp_path)
    assert list(got) == list(fixture)
    for name, lines in got.items():
        assert lines == fixture[name], name
        assert {p[2] for p in _plans(lines)} == set(SWITCHES), name


def test_fixture_holds_the_counted_plans(fixture):
    """The fixture against figures counted independently of it: the cases' return
    codes and task counts, the small-list rule's variants and the model lists' sizes."""
    for name, want in SINGLES.items():
        head, singles = _product(fixture[name])
        want = dict({"rc": 0}, **want)
        assert {k: head[k] for k in want} == want, (name, head)
        assert singles[0]["rc"] == want["rc"], name
    head, _ = _product(fixture["16 64 1 8 3 0 1 4"])
    aligned, _ = _product(fixture["96 576 9 8 3 0 1 0"])
    assert head["digest"] != aligned["digest"]
    head, _ = _product(fixture["small list that cannot be rebuilt at 1,536"])
    assert (head["rc"], head["variant"]) == (0, 6)
    head, singles = _product(fixture["n = 0"])
    assert (head["rc"], head["main"], head["reduce"], head["total"]) == (0, 0, 0, 0) and not singles
    for name, (weights, main, blockrow, variant) in MODEL_LISTS.items():
        head, _ = _product(fixture[name])
        assert len(_lists()[[n for n, _ in _lists()].index(name)][1]) == weights, name
        assert (head["rc"], head["main"], head["blockrow"], head["variant"]) == (0, main, blockrow, variant), (name, head)
    # the forced variants reach the list planner, never the single-tensor one
    for kind, _, switch, f in _plans(fixture["resnet50 x1"]):
        if switch[0] == "v":
            assert f["variant"] == (int(switch[1:]) if kind == "list" else 6), (kind, switch)


def _descs(rows):
    d = (_lib.TensorDesc * max(len(rows), 1))()
    for k, (r, row_len, khw, bits, mode, flags, esum, off) in enumerate(rows):
        d[k].src, d[k].dst, d[k].codes, d[k].scale, d[k].zero = SRC + off, DST, CODES, SCALE, ZERO
        d[k].esum = ESUM if esum else None
        d[k].rows, d[k].row_len, d[k].khw, d[k].bits, d[k].mode, d[k].flags = r, row_len, khw, bits, mode, flags & ~NULL_RANGE
        d[k].given_min, d[k].given_max = -1.0, 1.0
        d[k].range_enc = RANGE if (flags & _lib.DFQ_DEVICE_RANGE) and not (flags & NULL_RANGE) else None
    return d


def test_product_library_sizes_the_same_workspaces(fixture):
    """dfq_sweep_plan_ws_bytes and dfq_quantize_ws_bytes of libdfq_hip.so (host code,
    no device needed): the fixture's totals and return codes."""
    if not LIB.exists():
        pytest.skip("libdfq_hip.so not built (run __graft_entry__.build())")
    L = _lib.load()
    for name, rows in _lists():
        head, singles = _product(fixture[name])
        d = _descs(rows)
        assert L.dfq_sweep_plan_ws_bytes(d, len(rows)) == (head["total"] if head["rc"] == 0 else -1), name
        for t, f in singles.items():
            nbytes = C.c_size_t(0)
            assert L.dfq_quantize_ws_bytes(C.byref(d[t]), C.byref(nbytes)) == f["rc"], (name, t)
            if f["rc"] == 0:
                assert nbytes.value == f["total"], (name, t)
    assert L.dfq_sweep_plan_ws_bytes(None, 1) == -1 and L.dfq_sweep_plan_ws_bytes(None, -1) == -1


def _record(planner, commit):
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        lists = _run_planner(Path(tmp), Path(planner))
    FIXTURE.write_text(json.dumps({"recorded_from": commit, "lists": lists}, indent=0) + "\n")
    print("%d lists, %d distinct lines -> %s" % (len(lists), sum(map(len, lists.values())), FIXTURE))


if __name__ == "__main__":   # PYTHONPATH=<repository root> python tests/test_sweep_plan_host.py --record
    import sys
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: test_sweep_plan_host.py --record   (rewrites the fixture: state the reason in the change)")
    head = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    _record(CSRC / "dfq_sweep_plan.cpp", head)
