"""dfq_mx_gemm without a GPU: its index arithmetic walked on the CPU under sanitizers,
the entry point's argument checks, the Python wrappers' checks, and the idempotence of
the MX contract that lets mx_linear multiply exactly a stored MX weight."""
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
from tests import mx6_cases as M6
from tests import mx_cases as MC
from tests import mx_gemm_cases as GC

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "data_free_quantization_amd" / "libdfq_hip.so"
CXX = next((c for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"), shutil.which("c++"))
            if c and os.path.exists(c)), None)


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_index_arithmetic_under_sanitizers(tmp_path):
    """dfq_mx_gemm_plan.cpp + tests/native/mx_gemm_plan_check.cpp, nothing else linked,
    under AddressSanitizer and UBSan: for every shape of the GPU tests and all 16 format
    pairs, every byte a lane reads lies inside its array, every output element is stored
    exactly once, and the emulated instruction over the gathered operands equals the
    direct product -- everything but the hardware's own lane map and bit order."""
    (tmp_path / "shapes.txt").write_text("".join("%d %d %d\n" % s for s in GC.SHAPES))
    exe = tmp_path / "mx_gemm_plan_check"
    csrc = ROOT / "data_free_quantization_amd" / "csrc"
    subprocess.run([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", str(ROOT / "include"), "-I", str(csrc),
                    str(ROOT / "tests" / "native" / "mx_gemm_plan_check.cpp"), str(csrc / "dfq_mx_gemm_plan.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe), str(tmp_path / "shapes.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert not r.stderr, r.stderr[-4000:]   # no sanitizer report
    seen = {}
    for line in r.stdout.splitlines():
        w = line.split()
        assert w[0] == "ok", line
        seen[tuple(int(t) for t in w[1:6])] = {w[i]: int(w[i + 1]) for i in range(6, len(w), 2)}
    fmts = [mx.FORMATS[f][0] for f in GC.FMTS]
    assert set(seen) == {(m, n, k, a, b) for m, n, k in GC.SHAPES for a in fmts for b in fmts}
    for (m, n, k, a, b), got in seen.items():
        assert got["stores"] == m * n
        assert got["grid"] == -(-m // 64) * -(-n // 64)
        assert got["reads"] > 0


# ---- the entry point's argument checks ----------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        pytest.skip("libdfq_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def _good():
    d = _lib.MxGemmDesc()
    d.a_codes, d.a_scales, d.b_codes, d.b_scales, d.bias, d.out = 0x1000, 0x2001, 0x3000, 0x4003, 0x5004, 0x6004
    d.ldo, d.M, d.N, d.K = 40, 17, 33, 96
    d.a_format, d.b_format = _lib.DFQ_MX_FP8_E4M3, _lib.DFQ_MX_FP4_E2M1
    return d


def test_argument_validation_without_a_device(lib):
    """Every refusal comes back before any device call: this runs on a machine without a GPU."""
    L = lib
    assert L.dfq_mx_gemm(None, None) == _lib.DFQ_ERR_INVALID
    invalid = [("a_codes", None), ("a_scales", None), ("b_codes", None), ("b_scales", None), ("out", None),
               ("a_format", 2), ("a_format", -1), ("b_format", 5), ("b_format", 0x33), ("M", 0), ("N", 0), ("K", 0),
               ("M", -4), ("N", -1), ("K", -32), ("flags", 1), ("flags", -1), ("reserved", 1),
               ("a_codes", 0x1008), ("a_codes", 0x1001), ("b_codes", 0x3008), ("b_codes", 0x3004),
               ("out", 0x6002), ("out", 0x6001), ("bias", 0x5002)]
    for name, value in invalid:
        d = _good()
        setattr(d, name, value)
        assert L.dfq_mx_gemm(C.byref(d), None) == _lib.DFQ_ERR_INVALID, (name, value)
    for ldo in (32, 0, -40):
        d = _good()
        d.ldo = ldo
        assert L.dfq_mx_gemm(C.byref(d), None) == _lib.DFQ_ERR_SHAPE, ldo
    # FP6 code bases need 8 bytes, not 16; 4 is refused
    for fmt in (_lib.DFQ_MX_FP6_E2M3, _lib.DFQ_MX_FP6_E3M2):
        d = _good()
        d.a_format, d.a_codes = fmt, 0x1004
        assert L.dfq_mx_gemm(C.byref(d), None) == _lib.DFQ_ERR_INVALID
        d.b_format, d.b_codes = fmt, 0x3004
        d.a_codes = 0x1008
        assert L.dfq_mx_gemm(C.byref(d), None) == _lib.DFQ_ERR_INVALID


def test_desc_matches_the_header():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "dfq_hip.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct dfq_mx_gemm_desc\s*\{(.*?)\}\s*dfq_mx_gemm_desc;", text, flags=re.S).group(1)
    assert re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*;", body) == [f for f, _ in _lib.MxGemmDesc._fields_]
    assert C.sizeof(_lib.MxGemmDesc) == 6 * 8 + 4 * 8 + 4 * 4
    assert "dfq_mx_gemm" in _lib.EXPORTS and "#define DFQ_ABI_VERSION 1" in text


def test_python_rejects_cpu_tensors_and_bad_arguments():
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)   # noqa: E731
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        mx.mx_gemm(u8(4, 1, 16), u8(4, 1), "mxfp4", u8(3, 1, 32), u8(3, 1), "mxfp8", 32)
    with pytest.raises(ValueError):
        mx.mx_gemm(u8(4, 1, 16), u8(4, 1), "mxfp6", u8(3, 1, 32), u8(3, 1), "mxfp8", 32)
    with pytest.raises(ValueError):
        mx.mx_gemm(u8(4, 1, 16), u8(4, 1), "mxfp4", u8(3, 1, 32), u8(3, 1), "mxfp8", 0)
    with pytest.raises(TypeError):
        mx.mx_gemm(None, u8(4, 1), "mxfp4", u8(3, 1, 32), u8(3, 1), "mxfp8", 32)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        mx.mx_linear(torch.randn(4, 32), torch.randn(3, 32), None, "mxfp4")
    with pytest.raises(ValueError):
        mx.mx_linear(torch.randn(4, 32), torch.randn(3, 32), None, "mxfp4", "int")
    assert mx.LINEAR_CALLS == 0


def test_cli_flag():
    from data_free_quantization_amd import main_dfq
    a = main_dfq.get_argument(["--quantize", "--weight_format", "mxfp4", "--mx_matmul", "mxfp8"])
    assert a.mx_matmul == "mxfp8" and main_dfq.get_argument(["--quantize"]).mx_matmul is None
    for argv in (["--quantize", "--mx_matmul", "mxfp8"], ["--mx_matmul", "mxfp4"],
                 ["--quantize", "--weight_format", "mxfp4", "--mx_matmul", "int"]):
        with pytest.raises(SystemExit):
            main_dfq.get_argument(argv)


# ---- idempotence ----------------------------------------------------------------
def _statement(x, fmt):
    return (M6 if fmt in M6.FORMATS else MC).statement(x, fmt)


@pytest.mark.parametrize("fmt", GC.FMTS)
def test_the_mx_contract_is_idempotent(fmt):
    """Quantizing the quantizer's output changes nothing: after quantization a block's
    largest magnitude q_max * 2^X has q_max in [2^emax, the format's maximum], so
    floor(log2) - emax gives X again (a block rounded to all zeros takes scale byte 0 and
    +0 / -0 codes, which also stay), and every y_i * 2^-X is a table magnitude already.
    So a weight quantize_targ_layer left on an MX grid re-quantizes to its own codes and
    scales, and mx_linear on it multiplies exactly the stored values."""
    cases = [c for c in (M6 if fmt in M6.FORMATS else MC).all_cases() if c.fmt == fmt]
    assert len(cases) > 20
    n = 0
    for c in cases:
        first = c.ref if c.ref is not None else _statement(c.x, fmt)
        again = _statement(first["y"], fmt)
        assert np.array_equal(again["scales"], first["scales"]), c.name
        assert np.array_equal(again["codes"], first["codes"]), c.name
        assert np.array_equal(again["y"].view(np.uint32), first["y"].view(np.uint32)), c.name
        n += first["scales"].size
    assert n > 1000
