"""dfq_mx_linear without a GPU: its index arithmetic and per-lane quantizer walked on the CPU
under sanitizers (with the shared encoder tied to the MX contract's statement), the entry
point's argument checks, the descriptor's layout, the Python wrappers' checks and the CLI flag."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from data_free_quantization_amd import _lib, mx
from tests import mx6_cases as M6
from tests import mx_cases as MC
from tests import mx_gemm_cases as GC

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "data_free_quantization_amd" / "libdfq_hip.so"
CXX = next((c for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"), shutil.which("c++"))
            if c and os.path.exists(c)), None)
#: the GPU tests' shapes (tests/test_gpu_mx_linear_fused.py)
SHAPES = GC.SHAPES + [(3, 5, 30), (7, 9, 70), (32, 40, 24)]
CASE_ELEMS = 40000   # the case file holds the contract's cases up to this size


def _contract_cases():
    """(case, statement) for every case of the quantizer's tests small enough for the file."""
    out = []
    for mod in (MC, M6):
        for c in mod.all_cases():
            if c.x.size <= CASE_ELEMS:
                out.append((c, c.ref if c.ref is not None else mod.statement(c.x, c.fmt)))
    return out


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_index_arithmetic_and_encoder_under_sanitizers(tmp_path):
    """dfq_mx_linear_plan.cpp + tests/native/mx_linear_plan_check.cpp, nothing else linked, under
    AddressSanitizer and UBSan.  For every shape of the GPU tests, all 16 format pairs and both
    load paths: every fp32 read lies inside its row of x, every lane's operand registers and
    scale byte -- the FP8 exchanges emulated through the header's lane helpers -- equal byte for
    byte what dfq_mx_gemm's helpers gather from the host-quantized stored codes, and every
    output element is stored once.  The same host encoder (dfq_mx_encode.h, the one both
    kernels compile) then writes the codes and scales of the quantizer's contract cases, which
    must equal the contract's statement."""
    (tmp_path / "shapes.txt").write_text("".join("%d %d %d\n" % s for s in SHAPES))
    cases = _contract_cases()
    assert len(cases) > 100 and {c.fmt for c, _ in cases} == set(GC.FMTS)
    with open(tmp_path / "cases.bin", "wb") as f:
        for c, _ in cases:
            x = np.ascontiguousarray(c.x, dtype=np.float32)
            f.write(struct.pack("<iii", mx.FORMATS[c.fmt][0], x.shape[0], x.shape[1]))
            f.write(x.tobytes())
    exe = tmp_path / "mx_linear_plan_check"
    csrc = ROOT / "data_free_quantization_amd" / "csrc"
    subprocess.run([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", str(ROOT / "include"), "-I", str(csrc),
                    str(ROOT / "tests" / "native" / "mx_linear_plan_check.cpp"), str(csrc / "dfq_mx_linear_plan.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe), str(tmp_path / "shapes.txt"), str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert not r.stderr, r.stderr[-4000:]   # no sanitizer report
    seen = {}
    lines = r.stdout.splitlines()
    assert lines[-1] == "cases %d" % len(cases)
    for line in lines[:-1]:
        w = line.split()
        assert w[0] == "ok", line
        seen[tuple(int(t) for t in w[1:6])] = {w[i]: int(w[i + 1]) for i in range(6, len(w), 2)}
    fmts = [mx.FORMATS[f][0] for f in GC.FMTS]
    assert set(seen) == {(m, n, k, a, b) for m, n, k in SHAPES for a in fmts for b in fmts}
    for (m, n, k, a, b), got in seen.items():
        tiles = -(-m // 32) * -(-n // 32)   # working waves; each builds 2 fragments per K step, on both load paths
        assert got["stores"] == m * n
        assert got["grid"] == -(-m // 64) * -(-n // 64)
        assert got["frags"] == 2 * 2 * tiles * -(-k // 128)
        # every wave in a row of tiles reads that row's elements again, nothing else: 2 paths
        assert got["reads"] == 2 * m * k * -(-n // 32)
    blob = (tmp_path / "out.bin").read_bytes()
    at = 0
    for c, want in cases:
        rows, nb = want["scales"].shape
        cb = mx.FORMATS[c.fmt][2]
        codes = np.frombuffer(blob, np.uint8, rows * nb * cb, at).reshape(rows, nb, cb)
        at += codes.size
        scales = np.frombuffer(blob, np.uint8, rows * nb, at).reshape(rows, nb)
        at += scales.size
        assert np.array_equal(scales, want["scales"]), c.name
        assert np.array_equal(codes, want["codes"]), c.name
    assert at == len(blob)


# ---- the entry point's argument checks ----------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        pytest.skip("libdfq_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def _good():
    d = _lib.MxLinearDesc()
    d.x, d.b_codes, d.b_scales, d.bias, d.out = 0x1004, 0x3000, 0x4003, 0x5004, 0x6004
    d.ldx, d.ldo, d.M, d.N, d.K = 99, 40, 17, 33, 96
    d.x_format, d.b_format = _lib.DFQ_MX_FP8_E4M3, _lib.DFQ_MX_FP4_E2M1
    return d


def test_argument_validation_without_a_device(lib):
    """Every refusal comes back before any device call: this runs on a machine without a GPU."""
    L = lib
    assert L.dfq_mx_linear(None, None) == _lib.DFQ_ERR_INVALID
    invalid = [("x", None), ("b_codes", None), ("b_scales", None), ("out", None),
               ("x_format", 2), ("x_format", -1), ("b_format", 5), ("b_format", 0x33), ("M", 0), ("N", 0), ("K", 0),
               ("M", -4), ("N", -1), ("K", -32), ("M", (1 << 31) + 1), ("N", (1 << 31) + 1), ("K", (1 << 40) + 1),
               ("flags", 1), ("flags", -1), ("reserved", 1),
               ("x", 0x1002), ("x", 0x1001), ("b_codes", 0x3008), ("b_codes", 0x3004),
               ("out", 0x6002), ("out", 0x6001), ("bias", 0x5002)]
    for name, value in invalid:
        d = _good()
        setattr(d, name, value)
        if name == "K" and value > 0:
            d.ldx = value
        assert L.dfq_mx_linear(C.byref(d), None) == _lib.DFQ_ERR_INVALID, (name, value)
    for name, values in (("ldx", (95, 0, -99)), ("ldo", (32, 0, -40))):
        for v in values:
            d = _good()
            setattr(d, name, v)
            assert L.dfq_mx_linear(C.byref(d), None) == _lib.DFQ_ERR_SHAPE, (name, v)
    # FP6 weight codes need 8 bytes, not 16; 4 is refused.  x needs 4 bytes in every format.
    for fmt in (_lib.DFQ_MX_FP6_E2M3, _lib.DFQ_MX_FP6_E3M2):
        d = _good()
        d.b_format, d.b_codes = fmt, 0x3004
        assert L.dfq_mx_linear(C.byref(d), None) == _lib.DFQ_ERR_INVALID
        d.x_format, d.x = fmt, 0x1002
        d.b_codes = 0x3008
        assert L.dfq_mx_linear(C.byref(d), None) == _lib.DFQ_ERR_INVALID


def test_desc_matches_the_header():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "dfq_hip.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct dfq_mx_linear_desc\s*\{(.*?)\}\s*dfq_mx_linear_desc;", text, flags=re.S).group(1)
    assert re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*;", body) == [f for f, _ in _lib.MxLinearDesc._fields_]
    assert C.sizeof(_lib.MxLinearDesc) == 5 * 8 + 5 * 8 + 4 * 4
    assert _lib.MxLinearDesc.x_format.offset == 80
    assert "dfq_mx_linear" in _lib.EXPORTS and "#define DFQ_ABI_VERSION 1" in text


def test_python_rejects_cpu_tensors_and_bad_arguments():
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)   # noqa: E731
    with pytest.raises(RuntimeError, match="ROCm GPU only.*no CPU fallback"):
        mx.mx_linear_fused(torch.randn(4, 32), u8(3, 1, 32), u8(3, 1), "mxfp8", 32)
    with pytest.raises(ValueError):
        mx.mx_linear_fused(torch.randn(4, 32), u8(3, 1, 32), u8(3, 1), "mxfp8", 32, act_format="mxfp6")
    with pytest.raises(ValueError):
        mx.mx_linear_fused(torch.randn(4, 32), u8(3, 1, 32), u8(3, 1), "mxfp6", 32)
    with pytest.raises(ValueError):
        mx.mx_linear_fused(torch.randn(4, 32), u8(3, 1, 32), u8(3, 1), "mxfp8", 0)
    with pytest.raises(TypeError):
        mx.mx_linear_fused(None, u8(3, 1, 32), u8(3, 1), "mxfp8", 32)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        mx.mx_linear(torch.randn(4, 32), torch.randn(3, 32), None, "mxfp4", fused=True)
    with pytest.raises(ValueError):
        mx.mx_linear(torch.randn(4, 32), torch.randn(3, 32), None, "mxfp4", "int", fused=True)
    assert mx.LINEAR_CALLS == 0


def test_the_forward_scope_takes_the_fused_switch():
    from data_free_quantization_amd.utils import quantize as Q
    assert Q._MX_MATMUL is None and Q._MX_FUSED is False
    with Q.mx_matmul_forward("mxfp4", fused=True):
        assert (Q._MX_MATMUL, Q._MX_FUSED) == ("mxfp4", True)
        with Q.mx_matmul_forward("mxfp8"):
            assert (Q._MX_MATMUL, Q._MX_FUSED) == ("mxfp8", False)
        assert (Q._MX_MATMUL, Q._MX_FUSED) == ("mxfp4", True)
    assert Q._MX_MATMUL is None and Q._MX_FUSED is False


def test_cli_flag():
    from data_free_quantization_amd import main_dfq
    base = ["--quantize", "--weight_format", "mxfp4"]
    a = main_dfq.get_argument(base + ["--mx_matmul", "mxfp8", "--mx_matmul_fused"])
    assert a.mx_matmul == "mxfp8" and a.mx_matmul_fused is True
    assert main_dfq.get_argument(base + ["--mx_matmul", "mxfp8"]).mx_matmul_fused is False
    assert main_dfq.get_argument(["--quantize"]).mx_matmul_fused is False
    for argv in (base + ["--mx_matmul_fused"], ["--quantize", "--mx_matmul_fused"], ["--mx_matmul_fused"]):
        with pytest.raises(SystemExit):
            main_dfq.get_argument(argv)
