"""The residual add on stored codes without a GPU: the two new structs against the ABI, each refusal's return code
of dfq_int_add_q and dfq_int_mbconv_res_q with made-up pointers, and Python's refusals before any launch."""
import ctypes as C

import pytest
import torch

from data_free_quantization_amd import _lib, intmm
from tests.test_int_dwconv_host import lib  # noqa: F401  (the fixture)
from tests.test_int_mbconv_host import _good as _good_block

QUANT_REFUSALS = [("bits", 1), ("bits", 9), ("bits", 0), ("symmetric", 2), ("flags", 2), ("reserved", 1), ("given_max", -5.0), ("min_dev", 0x7002), ("max_dev", 0x7001)]


def _set(obj, path, value):
    *names, last = path.split(".")
    for n in names:
        obj = getattr(obj, n)
    setattr(obj, last, value)


def test_the_structs_and_the_adds_refusals_without_a_device(lib):
    A, R = _lib.IntAddDesc, _lib.IntMbconvRes
    assert {"dfq_int_add_q", "dfq_int_mbconv_res_q"} <= set(_lib.EXPORTS)
    assert C.sizeof(A) == 184 and (A.a_quant.offset, A.b_quant.offset, A.out_quant.offset, A.n.offset, A.flags.offset) == (24, 72, 120, 168, 176)
    assert C.sizeof(R) == 56 and (R.proj_quant.offset, R.flags.offset, R.reserved.offset) == (0, 48, 52)
    fn = lib.dfq_int_add_q
    assert fn(None, None) == _lib.DFQ_ERR_INVALID
    invalid = [("a", None), ("b", None), ("out", None), ("flags", 1), ("reserved", 1), ("out", 0x6002), ("n", 0), ("n", -5), ("n", (1 << 40) + 1),
               *[(q + "." + f, v) for q in ("a_quant", "b_quant") for f, v in QUANT_REFUSALS],
               ("out_quant.bits", 1), ("out_quant.bits", 9), ("out_quant.bits", 8), ("out_quant.symmetric", 2), ("out_quant.max_dev", 0x7001)]   # bits 8 without a range
    for path, value in invalid:
        d = A()
        d.a, d.b, d.out, d.n = 0x1001, 0x2003, 0x6004, 1000   # code bytes at any address, an fp32 out
        for q in (d.a_quant, d.b_quant):
            q.bits, q.given_min, q.given_max = 8, -1.0, 2.0
        _set(d, path, value)
        assert fn(C.byref(d), None) == _lib.DFQ_ERR_INVALID, (path, value)


def test_the_residual_block_refuses_without_a_device(lib):
    """dfq_int_mbconv_q's own refusals come first, then the residual struct's, then the shapes; the old entry still refuses flags = 1."""
    fn = lib.dfq_int_mbconv_res_q

    def rc(block=(), res=()):
        d, r = _good_block(), _lib.IntMbconvRes()
        d.Cin = d.Cout = 24
        r.proj_quant.bits, r.proj_quant.given_min, r.proj_quant.given_max = 8, -3.0, 3.0
        for path, value in block:
            _set(d, path, value)
        for path, value in res:
            _set(r, path, value)
        return fn(C.byref(d), C.byref(r), None)

    assert fn(None, None, None) == _lib.DFQ_ERR_INVALID and fn(C.byref(_good_block()), None, None) == _lib.DFQ_ERR_INVALID
    for path, value in [("x", None), ("flags", 1), ("hidden1.bits", 9), ("B", 0)]:
        assert rc(block=[(path, value)]) == _lib.DFQ_ERR_INVALID, (path, value)
    assert rc(block=[("stride", 3)]) == _lib.DFQ_ERR_UNSUPPORTED and rc(block=[("H", 1), ("pad", 0)]) == _lib.DFQ_ERR_SHAPE
    for f, v in [("flags", 1), ("reserved", 1), *[("proj_quant." + f, v) for f, v in QUANT_REFUSALS]]:
        assert rc(res=[(f, v)]) == _lib.DFQ_ERR_INVALID, (f, v)
    for block in ([("stride", 2)], [("pad", 0)], [("Cout", 16)], [("Cin", 40)]):
        assert rc(block=block) == _lib.DFQ_ERR_SHAPE, block
    assert rc(block=[("stride", 2)], res=[("proj_quant.bits", 9)]) == _lib.DFQ_ERR_INVALID   # the struct before the shapes
    d = _good_block()
    d.flags = 1
    assert lib.dfq_int_mbconv_q(C.byref(d), None) == _lib.DFQ_ERR_INVALID


def test_python_refuses_before_any_launch():
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)   # noqa: E731
    g, sym = intmm.OutQuant(min_value=-1.0, max_value=2.0), intmm.OutQuant(symmetric=True, min_value=-1.0, max_value=1.0)
    with pytest.raises(RuntimeError, match="ROCm GPU only.*no CPU fallback"):
        intmm.int_add_q(u8(2, 3), g, u8(2, 3), g)
    with pytest.raises(ValueError, match="one shape"):
        intmm.int_add_q(u8(2, 3), g, u8(3, 2), g)
    for args, err in (((u8(4).to(torch.int8), g, u8(4), g), TypeError), ((u8(4), sym, u8(4), g), TypeError), ((u8(4), g, u8(4), (-1.0, 2.0)), TypeError),
                      ((u8(4), intmm.OutQuant(bits=9, min_value=0.0, max_value=1.0), u8(4), g), ValueError)):
        with pytest.raises(err):
            intmm.int_add_q(*args)
    layer = lambda n, k: (u8(n, k), torch.ones(1), None, None)   # noqa: E731
    h = intmm.OutQuant(min_value=0.0, max_value=6.0)
    for residual, err, text in (((0.0, 1.0), TypeError, "residual"), (g, RuntimeError, "ROCm GPU only.*no CPU fallback")):
        with pytest.raises(err, match=text):
            intmm.int_mbconv_q(u8(1, 4, 5, 5), layer(8, 4), layer(8, 9), layer(4, 8), hidden1=h, hidden2=h, min_value=-1.0, max_value=1.0, residual=residual)
