"""The code-in / code-out integer entries without a GPU: the 4-B access predicates under sanitizers, each new check's return code, Python's refusals."""
import ctypes as C
import subprocess

import pytest
import torch

from data_free_quantization_amd import _lib, intmm
from tests import int_io_cases as QC
from tests import test_int_conv_host as CH
from tests import test_int_dwconv_host as DH
from tests.test_int_dwconv_host import lib  # noqa: F401  (the fixture)

ROOT, CSRC = DH.ROOT, DH.CSRC
ENTRIES = {"dfq_int_gemm_q": False, "dfq_int_linear_q": False, "dfq_int_conv2d_q": True, "dfq_int_dwconv2d_q": True}   # name -> takes x_codes


@pytest.mark.skipif(DH.CXX is None, reason="no host C++ compiler")
def test_byte_addressing_under_sanitizers(tmp_path):
    """tests/native/int_io_plan_check.cpp with the plan files alone, for every geometry of the GPU tests at every address mod 4."""
    lines = ["c " + " ".join(map(str, (g.B, g.C, g.H, g.W, g.N, *g.kernel, *g.stride, *g.padding, *g.dilation))) for g in QC.CONV_GEOMS.values()]
    lines += ["d " + " ".join(map(str, DH.DC.flat(QC.dw_geom(w, p)))) for w in QC.DW_WINDOWS for p in QC.DW_PLANES]
    (tmp_path / "shapes.txt").write_text("\n".join(lines) + "\n")
    exe = tmp_path / "int_io_plan_check"
    subprocess.run([DH.CXX, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", str(ROOT / "include"), "-I", str(CSRC), str(ROOT / "tests" / "native" / "int_io_plan_check.cpp"),
                    str(CSRC / "dfq_int_dwconv_plan.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe), str(tmp_path / "shapes.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr and not r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def _good(name):
    """A descriptor the old entry's checks pass (made-up pointers: never launched) and an io struct."""
    if ENTRIES[name]:
        d = DH._good() if name == "dfq_int_dwconv2d_q" else CH._good()
        d.flags = 0
    else:
        d = _lib.IntGemmDesc() if name == "dfq_int_gemm_q" else _lib.IntLinearDesc()
        d.b_codes, d.b_scale, d.out, d.ldo, d.M, d.N, d.K = 0x3000, 0x4004, 0x6004, 8, 4, 8, 16
        if name == "dfq_int_gemm_q":
            d.a_codes, d.a_scale = 0x1000, 0x2004
        else:
            d.x, d.ldx, d.x_bits = 0x1004, 16, 8
    return d, _lib.IntIo(out_bits=8, out_given_min=0.0, out_given_max=6.0)


@pytest.mark.parametrize("name", list(ENTRIES))
def test_the_new_checks_without_a_device(lib, name):
    """The old entry's refusals come first; then DFQ_ERR_INVALID for each of io's."""
    fn = getattr(lib, name)
    assert name in _lib.EXPORTS and C.sizeof(_lib.IntIo) == 48 and _lib.IntIo.out_min_dev.offset == 16
    d, io = _good(name)
    assert fn(None, C.byref(io), None) == _lib.DFQ_ERR_INVALID and fn(C.byref(d), None, None) == _lib.DFQ_ERR_INVALID
    bad = [("out_bits", 1), ("out_bits", 9), ("out_bits", -8), ("out_symmetric", 2), ("out_flags", 1), ("out_flags", _lib.DFQ_SCALE_F32 | 8),
           ("out_min_dev", 0x7002), ("out_max_dev", 0x7001), ("x_codes", 2), ("x_codes", -1), ("out_given_max", 0.0), ("out_given_max", -1.0), ("out_given_max", float("nan"))]   # a missing range
    if not ENTRIES[name]:
        bad.append(("x_codes", 1))   # gemm takes codes already; linear on codes is gemm
    for field, value in bad:
        d, io = _good(name)
        setattr(io, field, value)
        assert fn(C.byref(d), C.byref(io), None) == _lib.DFQ_ERR_INVALID, (field, value)
    d, io = _good(name)
    d.b_signed = 2                                   # the old entry's own refusal, whatever io says
    assert fn(C.byref(d), C.byref(io), None) == _lib.DFQ_ERR_INVALID
    # a byte tensor needs no alignment: the old entry's checks get past out and refuse the shape
    for out_bits, want in ((8, _lib.DFQ_ERR_SHAPE), (0, _lib.DFQ_ERR_INVALID)):
        d, io = _good(name)
        d.out, io.out_bits = 0x6001, out_bits
        setattr(d, *(("KH", 50) if ENTRIES[name] else ("ldo", 4)))
        assert fn(C.byref(d), C.byref(io), None) == want, out_bits


def test_python_refuses_before_any_launch():
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)   # noqa: E731
    rng = dict(min_value=-1.0, max_value=1.0)
    good = intmm.OutQuant(min_value=0.0, max_value=6.0)
    for oq, err in ((intmm.OutQuant(bits=1, **rng), ValueError), (intmm.OutQuant(bits=9, **rng), ValueError), (intmm.OutQuant(), ValueError),
                    (intmm.OutQuant(min_value=1.0, max_value=1.0), ValueError), (intmm.OutQuant(min_value=0.0), ValueError), (dict(bits=8), TypeError)):
        with pytest.raises(err):
            intmm.int_gemm(u8(4, 16), torch.ones(1), None, u8(8, 16), torch.ones(1), None, 16, out_quant=oq)
        with pytest.raises(err):
            intmm.int_conv2d_q(torch.randn(1, 4, 5, 5), u8(4, 4), torch.ones(1), None, 1, out_quant=oq, **rng)
    x = torch.randn(2, 4, 5, 5)
    for fn, k in ((intmm.int_conv2d_q, 4), (intmm.int_dwconv2d_q, 1)):
        with pytest.raises(RuntimeError, match="ROCm GPU only.*no CPU fallback"):
            fn(x, u8(4, k), torch.ones(1), None, 1, out_quant=good, **rng)
        for xc, sym in ((x.to(torch.int8), False), (x.to(torch.uint8), True), (x, False)):   # bytes of the other sign; fp32 where codes are announced
            with pytest.raises(TypeError, match="stored codes are torch.%s" % ("int8" if sym else "uint8")):
                fn(xc, u8(4, k), torch.ones(1), None, 1, x_codes=True, symmetric=sym, **rng)
    with pytest.raises(TypeError, match="out must be torch.uint8"):
        intmm._code_out("t", (2, 3), torch.zeros(2, 3), good, "cpu")
