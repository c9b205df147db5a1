"""Pooling on stored codes without a GPU: the two structs against the ABI, each refusal's return code of
dfq_int_mean_q and dfq_int_maxpool2d_q with made-up pointers, Python's refusals before any launch, and the mean's chunks and
pieces walked under sanitizers for the GPU test's shapes."""
import ctypes as C
import subprocess

import pytest
import torch

from data_free_quantization_amd import _lib, intmm
from tests import test_int_dwconv_host as DH
from tests.test_int_add_host import QUANT_REFUSALS, _set
from tests.test_int_dwconv_host import lib  # noqa: F401  (the fixture)

OUT_REFUSALS = [("out_quant.bits", 1), ("out_quant.bits", 9), ("out_quant.bits", 8), ("out_quant.symmetric", 2), ("out_quant.max_dev", 0x7001)]   # bits 8 without a range
COMMON = [("x", None), ("out", None), ("flags", 1), ("reserved", 1), *[("x_quant." + f, v) for f, v in QUANT_REFUSALS], *OUT_REFUSALS]
#: the GPU test's shapes (tests/test_gpu_int_pool.py), the timing script's planes, and a row of 2^23 bytes
MEAN_SHAPES = [(R, P, x16) for R, P in ((1029, 1), (1029, 7), (515, 16), (515, 17), (337, 49), (5, 4096), (5, 4097), (3, 1089), (1, 1 << 23)) for x16 in (0, 1)] + [(7, 49, 15)]


def _rc(fn, desc, good, path, value):
    d = desc()
    d.x, d.out = 0x1001, 0x6004   # code bytes at any address, an fp32 out
    d.x_quant.bits, d.x_quant.given_min, d.x_quant.given_max = 8, -1.0, 2.0
    for k, v in good.items():
        setattr(d, k, v)
    _set(d, path, value)
    return fn(C.byref(d), None)


def test_the_structs_and_the_refusals_without_a_device(lib):
    M, X = _lib.IntMeanDesc, _lib.IntMaxpool2dDesc
    assert {"dfq_int_mean_q", "dfq_int_maxpool2d_q"} <= set(_lib.EXPORTS)
    assert C.sizeof(M) == 136 and (M.x_quant.offset, M.out_quant.offset, M.rows.offset, M.plane.offset, M.flags.offset) == (16, 64, 112, 120, 128)
    assert C.sizeof(X) == 200 and (X.x_quant.offset, X.out_quant.offset, X.B.offset, X.pad_w.offset, X.flags.offset) == (16, 64, 112, 184, 192)

    mean, good = lib.dfq_int_mean_q, dict(rows=40, plane=49)
    assert mean(None, None) == _lib.DFQ_ERR_INVALID
    for path, value in [*COMMON, ("out", 0x6002), ("rows", 0), ("plane", 0), ("rows", -5), ("rows", (1 << 40) + 1), ("rows", 1 << 36)]:
        assert _rc(mean, M, good, path, value) == _lib.DFQ_ERR_INVALID, (path, value)
    assert _rc(mean, M, dict(rows=2, plane=(1 << 23) + 1), "flags", 0) == _lib.DFQ_ERR_UNSUPPORTED

    pool, good = lib.dfq_int_maxpool2d_q, dict(B=2, C=3, H=7, W=7, KH=3, KW=3, stride_h=2, stride_w=2, pad_h=1, pad_w=1)
    assert pool(None, None) == _lib.DFQ_ERR_INVALID
    extents = [(n, v) for n in ("B", "C", "H", "W", "KH", "KW", "stride_h", "stride_w") for v in (0, -3, (1 << 28) + 1)]
    for path, value in [*COMMON, *extents, ("pad_h", -1), ("pad_w", -1), ("pad_h", 2), ("pad_w", 2)]:   # pad 2 > 3 // 2
        assert _rc(pool, X, good, path, value) == _lib.DFQ_ERR_INVALID, (path, value)
    assert _rc(pool, X, dict(good, H=2, pad_h=0), "flags", 0) == _lib.DFQ_ERR_SHAPE and _rc(pool, X, dict(good, W=1, pad_w=0), "flags", 0) == _lib.DFQ_ERR_SHAPE
    assert _rc(pool, X, dict(good, H=20, W=20, KH=9, KW=8), "flags", 0) == _lib.DFQ_ERR_UNSUPPORTED   # 72 taps


def test_python_refuses_before_any_launch():
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)   # noqa: E731
    g, sym = intmm.OutQuant(min_value=-1.0, max_value=2.0), intmm.OutQuant(symmetric=True, min_value=-1.0, max_value=1.0)
    for call in (lambda: intmm.int_mean_q(u8(2, 3, 7, 7), g), lambda: intmm.int_maxpool2d_q(u8(2, 3, 7, 7), g, 3, 2, 1)):
        with pytest.raises(RuntimeError, match="ROCm GPU only.*no CPU fallback"):
            call()
    for fn, rest in ((intmm.int_mean_q, ()), (intmm.int_maxpool2d_q, (2,))):
        for x, q, err in ((u8(2, 3, 4, 4).to(torch.int8), g, TypeError), (u8(2, 3, 4, 4), sym, TypeError), (u8(2, 3, 4, 4), (-1.0, 2.0), TypeError),
                          (u8(2, 3, 4, 4), intmm.OutQuant(bits=9, min_value=0.0, max_value=1.0), ValueError)):
            with pytest.raises(err):
                fn(x, q, *rest)
    for kw, err in ((dict(kernel_size=3, padding=2), ValueError), (dict(kernel_size=0), ValueError), (dict(kernel_size=2, stride=0), ValueError),
                    (dict(kernel_size=(9, 8)), NotImplementedError)):
        with pytest.raises(err):
            intmm.int_maxpool2d_q(u8(2, 3, 7, 7), g, **kw)


@pytest.mark.skipif(DH.CXX is None, reason="no host C++ compiler")
def test_the_planner_under_sanitizers(tmp_path):
    """tests/native/int_pool_plan_check.cpp with the plan files alone: no chunk or piece of the mean leaves its tensor, the pieces
    partition every row, every row is stored once."""
    (tmp_path / "shapes.txt").write_text("".join("%d %d %d\n" % s for s in MEAN_SHAPES))
    exe = tmp_path / "int_pool_plan_check"
    subprocess.run([DH.CXX, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", str(DH.ROOT / "include"), "-I", str(DH.CSRC), str(DH.ROOT / "tests" / "native" / "int_pool_plan_check.cpp"),
                    str(DH.CSRC / "dfq_int_pool_plan.cpp"), str(DH.CSRC / "dfq_int_dwconv_plan.cpp"), "-o", str(exe)], check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe), str(tmp_path / "shapes.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr and not r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
