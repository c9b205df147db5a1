"""The grouped integer entries without a GPU: their argument checks at the C ABI and in Python,
the group arithmetic of dfq_int_gemm_plan.h walked on the CPU under sanitizers, and the numpy
statement at one group against the per-row statement."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

from data_free_quantization_amd import _lib, intmm
from tests import int_gemm_cases as IC
from tests import int_group_cases as GC
from tests.test_int_gemm_host import CXX, LIB, ROOT, _good_gemm, _good_linear


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        pytest.skip("libdfq_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def _good_conv():
    d = _lib.IntConv2dDesc()
    d.x, d.b_codes, d.b_scale, d.out = 0x1004, 0x3000, 0x4004, 0x6004
    d.B, d.C, d.H, d.W, d.N, d.KH, d.KW = 2, 8, 6, 6, 9, 3, 3
    d.stride_h = d.stride_w = d.dil_h = d.dil_w = d.pad_h = d.pad_w = 1
    d.x_bits = 8
    return d


@pytest.mark.parametrize("entry,good", [("dfq_int_gemm_grouped", _good_gemm), ("dfq_int_linear_grouped", _good_linear),
                                        ("dfq_int_conv2d_grouped", _good_conv)])
def test_group_argument_validation_without_a_device(lib, entry, good):
    """Refused before any device call: b_group < 1 and DFQ_INT_B_PER_ROW are invalid, any size
    but 32 or a multiple of 64 is unsupported, and the old entry's checks come first."""
    fn = getattr(lib, entry)
    assert fn(None, 64, None) == _lib.DFQ_ERR_INVALID

    def call(b_group, **fields):
        d = good()
        d.flags &= ~_lib.DFQ_INT_B_PER_ROW
        for k, v in fields.items():
            setattr(d, k, v)
        return fn(C.byref(d), b_group, None)
    for g in GC.BAD_GROUPS + [63, 65, 32768 + 64]:
        assert call(g) == (_lib.DFQ_ERR_INVALID if g < 1 else _lib.DFQ_ERR_UNSUPPORTED), g
    assert call(64, flags=_lib.DFQ_INT_B_PER_ROW) == _lib.DFQ_ERR_INVALID
    assert call(64, flags=0x8) == _lib.DFQ_ERR_INVALID and call(16, reserved=1) == _lib.DFQ_ERR_INVALID
    assert call(64, b_scale=None) == _lib.DFQ_ERR_INVALID


@pytest.mark.parametrize("g", GC.BAD_GROUPS)
def test_python_refuses_a_disallowed_group(g):
    u8, f32 = torch.zeros(4, 64, dtype=torch.uint8), torch.ones(4)
    with pytest.raises(ValueError, match="b_group"):
        intmm.int_gemm(u8, f32[:1], None, u8, f32, None, 64, b_group=g)
    with pytest.raises(ValueError, match="b_group"):
        intmm.int_linear(torch.zeros(4, 64), u8, f32, None, 64, min_value=0.0, max_value=1.0, b_group=g)
    with pytest.raises(ValueError, match="b_group"):
        intmm.int_conv2d_grouped(torch.zeros(1, 64, 2, 2), u8, f32, None, 1, min_value=0.0, max_value=1.0, b_group=g)
    with pytest.raises(ValueError, match="b_group"):
        intmm.group_quant(torch.zeros(4, 64), 4, g)


def test_the_statement_at_one_group_is_the_per_row_statement():
    c = IC.build(17, 33, 96, 0, 1, 1, 0)
    one = GC.statement(c.qa, c.qb, c.sa, c.za, c.sb.reshape(-1, 1), c.zb.reshape(-1, 1), c.bias, 128)
    assert np.array_equal(one.view(np.uint32), IC.expected(c).view(np.uint32))
    sb, zb = GC.group_params(33, 96, 32)
    assert not np.array_equal(GC.statement(c.qa, c.qb, c.sa, c.za, sb, zb, c.bias, 32), one)


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_group_arithmetic_under_sanitizers(tmp_path):
    """tests/native/int_group_plan_check.cpp with dfq_int_gemm_plan.h alone, under AddressSanitizer
    and UBSan: for every (K, g) of the GPU tests and the edges of the allowed sizes, every k of a
    row falls in exactly one (step, pass, lane) and that pass adds to group k / g, a group closes
    exactly once, after its last element, and the lengths are the contract's K_j."""
    exe = tmp_path / "int_group_plan_check"
    csrc = ROOT / "data_free_quantization_amd" / "csrc"
    subprocess.run([CXX, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", str(ROOT / "include"), "-I", str(csrc), str(ROOT / "tests" / "native" / "int_group_plan_check.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, timeout=300)
    kg = GC.GEMM_KG + [(168, 32), (166, 64), (72, 32), (72, 64), (1, 32), (33, 32), (32768, 32), (32768, 32768), (1000, 448)]
    r = subprocess.run([str(exe)] + ["%d:%d" % p for p in kg], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.split() == ["ok"] * len(kg)
