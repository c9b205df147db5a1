"""The integer inverted-residual block without a GPU: the ABI entry and its struct, each refusal's return code with made-up
pointers, Python's refusals, and the planner's addresses walked under sanitizers for the GPU test's geometries."""
import ctypes as C
import subprocess

import pytest
import torch

from data_free_quantization_amd import _lib, intmm
from tests import test_int_dwconv_host as DH
from tests.test_int_dwconv_host import lib  # noqa: F401  (the fixture)

#: the GPU test's geometries (tests/test_gpu_int_mbconv.py) and the zoo MobileNetV2's widest blocks: B Cin H W Ch Cout stride pad
SHAPES = [(2, 8, 9, 7, 24, 8, 1, 1), (1, 72, 8, 8, 96, 40, 2, 1), (1, 16, 19, 13, 130, 24, 1, 1), (2, 8, 1, 1, 200, 8, 1, 1),
          (1, 8, 9, 7, 24, 8, 2, 0), (1, 8, 8, 8, 24, 8, 2, 0), (1, 8, 9, 7, 24, 8, 2, 1), (1, 8, 8, 8, 24, 8, 1, 0),
          (1, 160, 7, 7, 960, 320, 1, 1), (1, 96, 14, 14, 576, 160, 2, 1), (1, 16, 112, 112, 96, 24, 2, 1)]


def _good():
    d = _lib.IntMbconvDesc()
    d.x, d.out = 0x1001, 0x6004
    for i, layer in enumerate((d.expand, d.depthwise, d.project)):
        layer.b_codes, layer.b_scale, layer.b_zero, layer.bias = 0x3000 + 0x100 * i, 0x4004, 0x4008, 0x5004
    for q in (d.x_quant, d.hidden1, d.hidden2):
        q.bits, q.given_min, q.given_max = 8, 0.0, 6.0
    d.B, d.Cin, d.H, d.W, d.Ch, d.Cout, d.stride, d.pad = 2, 16, 7, 7, 96, 24, 1, 1
    return d


def test_the_refusals_without_a_device(lib):
    """The siblings' codes in the siblings' order: this runs on a machine without a GPU, so nothing is launched."""
    fn = lib.dfq_int_mbconv_q
    assert "dfq_int_mbconv_q" in _lib.EXPORTS and C.sizeof(_lib.IntMbconvDesc) == 400
    assert (_lib.IntMbconvDesc.expand.offset, _lib.IntMbconvDesc.x_quant.offset, _lib.IntMbconvDesc.B.offset, _lib.IntMbconvDesc.flags.offset) == (16, 136, 328, 392)
    assert fn(None, None) == _lib.DFQ_ERR_INVALID

    def rc(path, value, **kw):
        d = _good()
        for k, v in kw.items():
            setattr(d, k, v)
        obj, names = d, path.split(".")
        for n in names[:-1]:
            obj = getattr(obj, n)
        setattr(obj, names[-1], value)
        return fn(C.byref(d), None)

    invalid = [("x", None), ("out", None), ("flags", 1), ("reserved", 1), ("out", 0x6002),
               *[(q + "." + f, v) for q in ("x_quant", "hidden1", "hidden2") for f, v in (("bits", 1), ("bits", 9), ("bits", 0), ("symmetric", 2), ("flags", 1), ("reserved", 1), ("given_max", 0.0), ("min_dev", 0x7002))],
               ("out_quant.bits", 1), ("out_quant.bits", 8), ("out_quant.symmetric", 2), ("out_quant.max_dev", 0x7001),   # bits 8 without a range
               *[(l + "." + f, v) for l in ("expand", "depthwise", "project") for f, v in (("b_codes", None), ("b_scale", None), ("b_signed", 2), ("flags", 4), ("b_codes", 0x3008), ("b_scale", 0x4002), ("b_zero", 0x4009), ("bias", 0x5002))],
               *[(n, v) for n in ("B", "Cin", "H", "W", "Ch", "Cout", "stride") for v in (0, -3, (1 << 28) + 1)], ("pad", -1), ("pad", (1 << 28) + 1)]
    for path, value in invalid:
        assert rc(path, value) == _lib.DFQ_ERR_INVALID, (path, value)
    assert rc("H", 1, pad=0) == _lib.DFQ_ERR_SHAPE and rc("W", 2, pad=0) == _lib.DFQ_ERR_SHAPE
    unsupported = [("stride", 3), ("pad", 2), ("Cin", _lib.DFQ_INT_MB_MAX_CIN + 1), ("Cout", _lib.DFQ_INT_MB_MAX_COUT + 1), ("Ch", _lib.DFQ_INT_MAX_K + 1),
                   ("expand.flags", _lib.DFQ_INT_B_PACK4), ("project.flags", _lib.DFQ_INT_B_PACK4 | _lib.DFQ_INT_B_PER_ROW)]
    for path, value in unsupported:
        assert rc(path, value) == _lib.DFQ_ERR_UNSUPPORTED, (path, value)


def test_python_refuses_before_any_launch():
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)   # noqa: E731
    layer = lambda n, k: (u8(n, k), torch.ones(1), None, None)   # noqa: E731
    h, rng = intmm.OutQuant(min_value=0.0, max_value=6.0), dict(min_value=-1.0, max_value=1.0)
    x = u8(1, 4, 5, 5)
    call = lambda x=x, e=layer(8, 4), d=layer(8, 9), p=layer(4, 8), **kw: intmm.int_mbconv_q(x, e, d, p, **{**dict(hidden1=h, hidden2=h), **rng, **kw})   # noqa: E731
    with pytest.raises(RuntimeError, match="ROCm GPU only.*no CPU fallback"):
        call()
    for kw, err in ((dict(x=x.to(torch.int8)), TypeError), (dict(x=x.float()), TypeError), (dict(x=x, symmetric=True), TypeError), (dict(bits=9), ValueError)):
        with pytest.raises(err):
            call(**kw)


@pytest.mark.skipif(DH.CXX is None, reason="no host C++ compiler")
def test_the_planner_under_sanitizers(tmp_path):
    """tests/native/int_mbconv_plan_check.cpp with the plan file alone: every LDS byte read was written, every global read lies in
    its tensor, every output is stored once, the LDS extents stay inside the declared size."""
    (tmp_path / "shapes.txt").write_text("\n".join(" ".join(map(str, s)) for s in SHAPES) + "\n")
    exe = tmp_path / "int_mbconv_plan_check"
    subprocess.run([DH.CXX, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", str(DH.ROOT / "include"), "-I", str(DH.CSRC), str(DH.ROOT / "tests" / "native" / "int_mbconv_plan_check.cpp"),
                    str(DH.CSRC / "dfq_int_mbconv_plan.cpp"), "-o", str(exe)], check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe), str(tmp_path / "shapes.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr and not r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
