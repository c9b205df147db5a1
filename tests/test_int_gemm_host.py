"""dfq_int_gemm / dfq_int_linear without a GPU: the index arithmetic walked on the CPU under
sanitizers, the entry points' argument checks, the descriptors against the header, the
Python wrappers' and the CLI's refusals, and the idempotence of the given-range quantizer
that lets int_matmul_forward re-quantize a fake-quantized activation to its own codes."""
import ctypes as C
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from data_free_quantization_amd import _lib, intmm
from oracle import oracle
from tests import int_gemm_cases as IC

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "data_free_quantization_amd" / "libdfq_hip.so"
CXX = next((c for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"), shutil.which("c++"))
            if c and os.path.exists(c)), None)


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_index_arithmetic_under_sanitizers(tmp_path):
    """dfq_int_gemm_plan.cpp + tests/native/int_gemm_plan_check.cpp, nothing else linked, under
    AddressSanitizer and UBSan: for every shape of the GPU tests and every (a_signed, b_signed,
    packed) mode, every byte a lane reads lies inside its array, every output element is stored
    exactly once, and the emulated instruction over the gathered fragments folds to the
    contract's integers P, Sa and Sb -- everything but the hardware's own lane map."""
    (tmp_path / "shapes.txt").write_text("".join("%d %d %d\n" % s for s in IC.SHAPES))
    exe = tmp_path / "int_gemm_plan_check"
    csrc = ROOT / "data_free_quantization_amd" / "csrc"
    subprocess.run([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", str(ROOT / "include"), "-I", str(csrc),
                    str(ROOT / "tests" / "native" / "int_gemm_plan_check.cpp"), str(csrc / "dfq_int_gemm_plan.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe), str(tmp_path / "shapes.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert not r.stderr, r.stderr[-4000:]   # no sanitizer report
    seen = {}
    for line in r.stdout.splitlines():
        w = line.split()
        assert w[0] == "ok", line
        seen[tuple(int(t) for t in w[1:7])] = {w[i]: int(w[i + 1]) for i in range(7, len(w), 2)}
    assert set(seen) == {(m, n, k, a, b, p) for m, n, k, a, b, _, p in IC.all_cases()}
    for (m, n, k, a, b, p), got in seen.items():
        assert got["stores"] == m * n
        assert got["grid"] == -(-m // 64) * -(-n // 64)
        # every wave tile reads its 32 rows of A and of B whole (rows that exist, K elements each)
        tiles_m, tiles_n = -(-m // 32), -(-n // 32)
        assert got["reads"] == tiles_n * m * k + tiles_m * (n * k // 2 if p else n * k)


# ---- the entry points' argument checks ----------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        pytest.skip("libdfq_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def _good_gemm():
    d = _lib.IntGemmDesc()
    d.a_codes, d.a_scale, d.a_zero, d.b_codes, d.b_scale, d.b_zero = 0x1000, 0x2004, 0x2008, 0x3000, 0x4004, 0x4008
    d.bias, d.out = 0x5004, 0x6004
    d.ldo, d.M, d.N, d.K = 40, 17, 33, 96
    d.a_signed, d.b_signed, d.flags = 0, 1, _lib.DFQ_INT_B_PER_ROW
    return d


def _good_linear():
    d = _lib.IntLinearDesc()
    d.x, d.min_dev, d.max_dev, d.b_codes, d.b_scale, d.b_zero = 0x1004, 0x2004, 0x2008, 0x3000, 0x4004, 0x4008
    d.bias, d.out = 0x5004, 0x6004
    d.ldx, d.ldo, d.M, d.N, d.K = 100, 40, 17, 33, 96
    d.x_bits, d.x_symmetric, d.b_signed, d.flags = 8, 0, 1, _lib.DFQ_INT_B_PACK4 | _lib.DFQ_SCALE_F32
    return d


_SHARED_INVALID = [("b_codes", None), ("b_scale", None), ("out", None), ("M", 0), ("N", 0), ("K", 0), ("M", -4), ("N", -1),
                   ("K", -32), ("flags", 8), ("flags", -1), ("flags", 0x10), ("reserved", 1), ("b_signed", 2), ("b_signed", -1),
                   ("b_codes", 0x3008), ("b_codes", 0x3001), ("out", 0x6002), ("out", 0x6001), ("bias", 0x5002),
                   ("b_scale", 0x4002), ("b_zero", 0x4009)]


def test_gemm_argument_validation_without_a_device(lib):
    """Every refusal comes back before any device call: this runs on a machine without a GPU."""
    L = lib
    assert L.dfq_int_gemm(None, None) == _lib.DFQ_ERR_INVALID
    invalid = _SHARED_INVALID + [("a_codes", None), ("a_scale", None), ("a_codes", 0x1008), ("a_codes", 0x1001),
                                 ("a_scale", 0x2002), ("a_zero", 0x2001), ("a_signed", 2), ("flags", 4)]
    for name, value in invalid:
        d = _good_gemm()
        setattr(d, name, value)
        assert L.dfq_int_gemm(C.byref(d), None) == _lib.DFQ_ERR_INVALID, (name, value)
    for ldo in (32, 0, -40):
        d = _good_gemm()
        d.ldo = ldo
        assert L.dfq_int_gemm(C.byref(d), None) == _lib.DFQ_ERR_SHAPE, ldo
    for fields in ({"K": 32769}, {"K": 95, "flags": _lib.DFQ_INT_B_PACK4}, {"M": 1 << 38, "N": 1 << 38, "ldo": 1 << 38, "K": 1}):
        d = _good_gemm()
        for k, v in fields.items():
            setattr(d, k, v)
        rc = L.dfq_int_gemm(C.byref(d), None)
        # the last one's M * ldo leaves the offset range before its grid is looked at
        assert rc == (_lib.DFQ_ERR_INVALID if "M" in fields else _lib.DFQ_ERR_UNSUPPORTED), fields
    d = _good_gemm()
    d.M, d.N, d.ldo, d.K = 1 << 24, 1 << 24, 1 << 24, 1   # 2^36 blocks
    assert L.dfq_int_gemm(C.byref(d), None) == _lib.DFQ_ERR_UNSUPPORTED


def test_linear_argument_validation_without_a_device(lib):
    L = lib
    assert L.dfq_int_linear(None, None) == _lib.DFQ_ERR_INVALID
    invalid = _SHARED_INVALID + [("x", None), ("x", 0x1002), ("min_dev", 0x2001), ("max_dev", 0x2002), ("x_bits", 1), ("x_bits", 9),
                                 ("x_bits", 16), ("x_bits", 0), ("x_symmetric", 2), ("reserved2", 1)]
    for name, value in invalid:
        d = _good_linear()
        setattr(d, name, value)
        assert L.dfq_int_linear(C.byref(d), None) == _lib.DFQ_ERR_INVALID, (name, value)
    for name, value in (("ldo", 32), ("ldx", 95), ("ldx", 0), ("ldo", -1)):
        d = _good_linear()
        setattr(d, name, value)
        assert L.dfq_int_linear(C.byref(d), None) == _lib.DFQ_ERR_SHAPE, (name, value)
    for fields in ({"K": 32769, "ldx": 40000}, {"K": 95}):   # packed with an odd K
        d = _good_linear()
        for k, v in fields.items():
            setattr(d, k, v)
        assert L.dfq_int_linear(C.byref(d), None) == _lib.DFQ_ERR_UNSUPPORTED, fields


def _header_fields(name):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "dfq_hip.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s;" % (name, name), text, flags=re.S).group(1)
    return re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*;", body), text


def test_descs_match_the_header():
    fields, text = _header_fields("dfq_int_gemm_desc")
    assert fields == [f for f, _ in _lib.IntGemmDesc._fields_]
    assert C.sizeof(_lib.IntGemmDesc) == 8 * 8 + 4 * 8 + 4 * 4
    fields, _ = _header_fields("dfq_int_linear_desc")
    assert fields == [f for f, _ in _lib.IntLinearDesc._fields_]
    assert C.sizeof(_lib.IntLinearDesc) == 8 * 8 + 2 * 8 + 5 * 8 + 6 * 4
    assert "dfq_int_gemm" in _lib.EXPORTS and "dfq_int_linear" in _lib.EXPORTS and "#define DFQ_ABI_VERSION 1" in text
    for name, value in (("DFQ_INT_B_PACK4", _lib.DFQ_INT_B_PACK4), ("DFQ_INT_B_PER_ROW", _lib.DFQ_INT_B_PER_ROW)):
        assert re.search(r"#define %s\s+0x%x\b" % (name, value), text)
    integration = (ROOT / "INTEGRATION.md").read_text()
    assert "dfq_int_gemm" in integration and "dfq_int_linear" in integration


def test_python_rejects_cpu_tensors_and_bad_arguments():
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)   # noqa: E731
    f32 = lambda *s: torch.ones(*s)   # noqa: E731
    intmm.reset_linear_calls()
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        intmm.int_gemm(u8(4, 32), f32(1), f32(1), u8(3, 32), f32(3), f32(3), 32)
    with pytest.raises(ValueError):
        intmm.int_gemm(u8(4, 32), f32(1), f32(1), u8(3, 32), f32(3), f32(3), 0)
    with pytest.raises(ValueError):
        intmm.int_gemm(u8(4, 32), f32(1), f32(1), u8(3, 32), f32(3), f32(3), 32769)
    with pytest.raises(TypeError):
        intmm.int_gemm(None, f32(1), f32(1), u8(3, 32), f32(3), f32(3), 32)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        intmm.int_linear(torch.randn(4, 32), u8(3, 32), f32(1), None, 32, min_value=-1.0, max_value=1.0)
    with pytest.raises(ValueError):
        intmm.int_linear(torch.randn(4, 32), u8(3, 32), f32(1), None, 32, bits=9, min_value=-1.0, max_value=1.0)
    with pytest.raises(ValueError):
        intmm.int_linear(torch.randn(4, 32), u8(3, 32), f32(1), None, 32, bits=1, min_value=-1.0, max_value=1.0)
    with pytest.raises(TypeError):
        intmm.int_linear(None, u8(3, 32), f32(1), None, 32, min_value=-1.0, max_value=1.0)
    assert intmm.LINEAR_CALLS == 0


def test_cli_flag():
    from data_free_quantization_amd import main_dfq
    a = main_dfq.get_argument(["--quantize", "--int_matmul"])
    assert a.int_matmul is True and main_dfq.get_argument(["--quantize"]).int_matmul is False
    assert main_dfq.get_argument(["--quantize", "--weight_format", "int", "--int_matmul"]).int_matmul is True
    for argv in (["--int_matmul"], ["--quantize", "--weight_format", "mxfp4", "--int_matmul"],
                 ["--quantize", "--weight_format", "mxfp4", "--mx_matmul", "mxfp8", "--int_matmul"]):
        with pytest.raises(SystemExit):
            main_dfq.get_argument(argv)


def test_forward_scope_resets_the_counter_and_closes():
    from data_free_quantization_amd.utils import quantize as Q
    intmm.LINEAR_CALLS = 7
    with Q.int_matmul_forward():
        assert intmm.LINEAR_CALLS == 0 and Q._INT_MATMUL
    assert not Q._INT_MATMUL


# ---- idempotence ----------------------------------------------------------------
#: bits -> the largest max(|min|, |max|) / (max - min) the derivation of DESIGN.md 3.9 covers:
#: 0.99 * 2^23 / (2^bits - 1)
def _edge(bits):
    return 0.99 * 2 ** 23 / (2 ** bits - 1)


def _ranges(bits):
    e = _edge(bits)
    return [(-1.0, 1.0), (0.0, 6.0), (0.0, 0.37), (-5.25, -0.125), (-3.7, 0.0), (-0.013, 2.9),
            (e * 0.999 - 1.0, e * 0.999),            # the edge, positive: |max| / (max - min) just inside
            (-e * 0.999 * 0.37, -e * 0.999 * 0.37 + 0.37),   # the edge, negative-only
            (1000.0, 1001.0)]


@pytest.mark.parametrize("bits", [8, 4, 2])
@pytest.mark.parametrize("flags", [oracle.F_GIVEN, oracle.F_GIVEN | oracle.F_F32])
def test_the_given_range_quantizer_is_idempotent(bits, flags):
    """quantize(quantize(x)) has quantize(x)'s codes while max(|min|, |max|) <= 0.99 * 2^23 /
    (2^bits - 1) * (max - min): the dequantized y = fl(fl(q s) + min) is within
    2^-24 |y| + 2^-24 q s of q s + min, and (y - min) / s adds two more roundings of q, so the
    quotient stays within 1/2 of q.  Symmetric grids (min = 0 exactly) always do."""
    rng = np.random.default_rng(bits * 16 + flags)
    n = 0
    for sym in (False, True):
        for mn, mx in _ranges(bits):
            x = rng.uniform(mn - 0.1 * (mx - mn), mx + 0.1 * (mx - mn), size=4096).astype(np.float32)
            x[:2] = (mn, mx)
            mode = oracle.TENSOR_SYM if sym else oracle.TENSOR_ASYM
            first = oracle.quantize(x, bits, mode, rows=1, flags=flags, given=(mn, mx))
            again = oracle.quantize(first["dq"], bits, mode, rows=1, flags=flags, given=(mn, mx))
            assert np.array_equal(again["codes"], first["codes"]), (sym, mn, mx)
            assert np.array_equal(again["dq"].view(np.uint32), first["dq"].view(np.uint32)), (sym, mn, mx)
            assert again["scale"][0] == first["scale"][0] and again["zero"][0] == first["zero"][0]
            n += len(np.unique(first["codes"]))
    assert n > 2 * len(_ranges(bits))   # the grids were used, not one code
