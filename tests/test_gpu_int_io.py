"""The code-in / code-out integer entries on the GPU, bit for bit the statements of tests/int_io_cases.py."""
from unittest import mock

import numpy as np
import pytest
import torch

from tests import int_io_cases as QC
from tests.test_gpu_int_dwconv import DEV, _dev

pytestmark = pytest.mark.gpu
IN = {s: dict(zip(("min_value", "max_value"), r)) for s, r in QC.IN_RANGE.items()}


def _same(got, want, what=""):   # bit for bit: bytes as they are, floats through their words
    g, w = got.detach().cpu().numpy(), np.ascontiguousarray(want)
    assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
    word = np.uint32 if g.dtype == np.float32 else g.dtype
    bad = np.argwhere(g.view(word) != w.view(word))
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def _oq(rng_pair, bits=8, sym=False, dev=False):
    from data_free_quantization_amd import intmm
    if dev:
        return intmm.OutQuant(bits, sym, min_dev=torch.tensor([rng_pair[0]], device=DEV), max_dev=torch.tensor([rng_pair[1]], device=DEV))
    return intmm.OutQuant(bits, sym, min_value=rng_pair[0], max_value=rng_pair[1])


def _guarded(want, shift):   # a byte tensor of want's shape at address `shift` mod 4 inside a buffer of 0x5A, and the buffer
    buf = torch.full((want.size + 8,), 0x5A, dtype=torch.uint8, device=DEV)
    return buf[shift:shift + want.size].view(want.shape), buf


def _b(w):
    return _dev(w.b_bytes), _dev(w.sb), _dev(w.zb)


@pytest.mark.parametrize("out_sym", [False, True])
@pytest.mark.parametrize("out_bits", [8, 4])
@pytest.mark.parametrize("shape", QC.GEMM_SHAPES)
def test_gemm_and_linear_store_the_codes_of_the_statement(shape, out_bits, out_sym):
    """(37, 45, 70) also goes through a byte row stride of N + 19 and through int_linear on an fp32 input."""
    from data_free_quantization_amd import intmm
    r = QC.gemm(*shape, out_bits, out_sym)
    c = r["case"]
    oq = _oq(r["out_range"], out_bits, out_sym, dev=out_bits == 4)
    args = (_dev(c.a_bytes), _dev(c.sa), _dev(c.za), *_b(c), c.K)
    _same(intmm.int_gemm(*args, bias=_dev(c.bias), out_quant=oq), r["codes"], shape)
    if shape == (37, 45, 70):
        buf = torch.full((c.M, c.N + 19), 0x5A, dtype=torch.int8 if out_sym else torch.uint8, device=DEV)
        out = intmm.int_gemm(*args, bias=_dev(c.bias), out_quant=oq, out=buf[:, :c.N])
        assert out.data_ptr() == buf.data_ptr() and bool((buf[:, c.N:] == 0x5A).all())
        _same(buf[:, :c.N].contiguous(), r["codes"], "strided")
        lin = QC.linear(*shape, out_bits, out_sym)
        _same(intmm.int_linear(_dev(lin["x"]), *_b(c), c.K, bias=_dev(c.bias), out_quant=_oq(lin["out_range"], out_bits, out_sym), **IN[False]), lin["codes"], "linear")


@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("name", ["pw", "k3p1", "k3s2d2"])
def test_conv_reads_stored_codes(name, sym):
    """The statement on the codes, and -- the range being idempotent -- the old int_conv2d on their dequantized values."""
    from data_free_quantization_amd import intmm
    r = QC.conv(name, True, sym)
    rest = (*_b(r["w"]), r["g"].kernel, r["g"].stride, r["g"].padding, r["g"].dilation)
    got = intmm.int_conv2d_q(_dev(r["q"]), *rest, x_codes=True, symmetric=sym, bias=_dev(r["w"].bias), **IN[sym])
    _same(got, r["y"], name)
    assert torch.equal(got.view(torch.int32), intmm.int_conv2d(_dev(r["x"]), *rest, symmetric=sym, bias=_dev(r["w"].bias), **IN[sym]).view(torch.int32))


@pytest.mark.parametrize("x_codes", [True, False])
@pytest.mark.parametrize("name,packed", [("pw", False), ("k3p1", False), ("k3s2d2", False), ("quad", False), ("quad", True)])
def test_conv_stores_codes(name, packed, x_codes):
    """Into a byte tensor at every address mod 4 (the 4-B store and the byte stores), its surroundings untouched."""
    from data_free_quantization_amd import intmm
    r = QC.conv(name, x_codes, False, packed)
    g = r["g"]
    for shift in range(4):
        out, buf = _guarded(r["codes"], shift)
        intmm.int_conv2d_q(_dev(r["q"] if x_codes else r["x"]), *_b(r["w"]), g.kernel, g.stride, g.padding, g.dilation, x_codes=x_codes, b_packed=packed, bias=_dev(r["w"].bias), out_quant=_oq(r["out_range"], dev=shift == 1), out=out, **IN[False])
        _same(out, r["codes"], (name, shift))
        assert bool((buf[:shift] == 0x5A).all()) and bool((buf[shift + out.numel():] == 0x5A).all())


@pytest.mark.parametrize("path", ["codes-fp32", "fp32-codes", "codes-codes"])
@pytest.mark.parametrize("plane", list(QC.DW_PLANES))
@pytest.mark.parametrize("window", list(QC.DW_WINDOWS))
def test_depthwise(window, plane, path):
    """Each path at 4-aligned and at odd addresses: the word and the byte forms of the copy and of the store."""
    from data_free_quantization_amd import intmm
    x_codes, out_codes = path.startswith("codes"), path.endswith("codes")
    r = QC.dwconv(window, plane, x_codes)
    g, want = r["g"], r["codes"] if out_codes else r["y"]
    for shift in (0, 1):
        x = _guarded(r["q"], shift)[0].copy_(_dev(r["q"])) if x_codes else _dev(r["x"])
        out, buf = _guarded(want, shift) if out_codes else (None, None)
        got = intmm.int_dwconv2d_q(x, *_b(r["w"]), g.kernel, g.stride, g.padding, g.dilation, x_codes=x_codes, bias=_dev(r["w"].bias), out_quant=_oq(r["out_range"]) if out_codes else None, out=out, **IN[False])
        _same(got, want, (window, plane, path, shift))
        assert not out_codes or (bool((buf[:shift] == 0x5A).all()) and bool((buf[shift + out.numel():] == 0x5A).all()))


def test_a_chain_of_three_layers_exchanges_bytes_only():
    """1x1 (8 -> 24) -> depthwise 3x3 p1 -> 1x1 (24 -> 8) through uint8 tensors on [0, 6] equals, bit for bit, int_conv2d ->
    fake_quant -> int_dwconv2d -> fake_quant -> int_conv2d; the two byte tensors are fake_quant's codes there."""
    from data_free_quantization_amd import intmm
    from data_free_quantization_amd.utils.quantize import fake_quant
    gen = torch.Generator(device="cpu").manual_seed(22)
    x = (torch.randn(2, 8, 9, 7, generator=gen) * 1.2 + 0.4).to(DEV)
    w = [fake_quant((torch.randn(n, k, generator=gen) * s).to(DEV), 8, per_channel=True) for n, k, s in ((24, 8, 0.5), (24, 9, 0.4), (8, 24, 0.2))]
    b, wq = [(torch.randn(n, generator=gen) + 2.0).to(DEV) for n in (24, 24, 8)], [(t.codes, t.scale, t.zero) for t in w]
    xr, relu6 = dict(min_value=-1.3, max_value=2.5), dict(min_value=0.0, max_value=6.0)
    y1 = intmm.int_conv2d(x, *wq[0], 1, bias=b[0], **xr)   # the existing route
    f1 = fake_quant(y1.reshape(1, -1), 8, **relu6)
    y2 = intmm.int_dwconv2d(f1.dq.view_as(y1), *wq[1], 3, padding=1, bias=b[1], **relu6)
    f2 = fake_quant(y2.reshape(1, -1), 8, **relu6)
    y3 = intmm.int_conv2d(f2.dq.view_as(y2), *wq[2], 1, bias=b[2], **relu6)
    oq = intmm.OutQuant(**relu6)                            # the chain
    c1 = intmm.int_conv2d_q(x, *wq[0], 1, bias=b[0], out_quant=oq, **xr)
    c2 = intmm.int_dwconv2d_q(c1, *wq[1], 3, padding=1, x_codes=True, bias=b[1], out_quant=oq, **relu6)
    c3 = intmm.int_conv2d_q(c2, *wq[2], 1, x_codes=True, bias=b[2], **relu6)
    assert c1.dtype == c2.dtype == torch.uint8 and torch.equal(c1, f1.codes.view_as(c1)) and torch.equal(c2, f2.codes.view_as(c2))
    assert 16 <= len(torch.unique(c1)) and 16 <= len(torch.unique(c2)) and bool((c1 == 0).any()) and bool((c1 == 255).any())
    assert torch.equal(c3.view(torch.int32), y3.view(torch.int32))


def test_both_options_off_is_the_old_entry():
    """Each _q entry with an all-zero io struct gives the old entry's bits."""
    from data_free_quantization_amd import _lib, intmm
    r, d, c = QC.conv("k3p1", False, False), QC.dwconv("s1p1", "7x7", False), QC.gemm(37, 45, 70, 8, False)["case"]
    conv_args = (_dev(r["x"]), *_b(r["w"]), r["g"].kernel, r["g"].stride, r["g"].padding, r["g"].dilation)
    assert torch.equal(intmm.int_conv2d_q(*conv_args, **IN[False]), intmm.int_conv2d(*conv_args, **IN[False]))
    dw_args = (_dev(d["x"]), *_b(d["w"]), 3, 1, 1, 1)
    assert torch.equal(intmm.int_dwconv2d_q(*dw_args, **IN[False]), intmm.int_dwconv2d(*dw_args, **IN[False]))
    calls = (lambda: intmm.int_gemm(_dev(c.a_bytes), _dev(c.sa), _dev(c.za), *_b(c), c.K), lambda: intmm.int_linear(_dev(c.a_bytes).float(), *_b(c), c.K, min_value=0.0, max_value=255.0))
    want = [f() for f in calls]
    with mock.patch.object(intmm, "_io_arg", lambda out_quant, x_codes: _lib.IntIo()):   # the _q entries, nothing set
        assert all(torch.equal(f(), t) for f, t in zip(calls, want))
