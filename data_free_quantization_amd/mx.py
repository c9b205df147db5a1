"""OCP Microscaling (MX) block-scaled weight quantization: MXFP4, MXFP6 and MXFP8.

Host wrapper of ``dfq_mx_quantize_batch`` (include/dfq_hip.h): FP4
(E2M1), FP6 (E2M3 or E3M2) or FP8 (E4M3) elements with one shared power-of-two E8M0
scale per 32 consecutive elements of a row, the operand format of CDNA4's scaled
matrix instructions.  ``mx_quantize`` takes every tensor of a list in one C call (one
launch, one HBM pass, asynchronous on the stream); ``mx_dequantize`` rebuilds the
fp32 values from codes and scales in plain torch, exactly, on CPU or GPU.  There is
no CPU fallback for the quantizer: CPU tensors raise."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib

BLOCK = _lib.DFQ_MX_BLOCK
#: weight_format name -> (library format, element bits, code bytes per block)
FORMATS = {"mxfp4": (_lib.DFQ_MX_FP4_E2M1, 4, 16), "mxfp8": (_lib.DFQ_MX_FP8_E4M3, 8, 32),
           "mxfp6_e2m3": (_lib.DFQ_MX_FP6_E2M3, 6, 24), "mxfp6_e3m2": (_lib.DFQ_MX_FP6_E3M2, 6, 24)}
_NAMES = "'mxfp4', 'mxfp6_e2m3', 'mxfp6_e3m2' or 'mxfp8'"   # there is no bare 'mxfp6': the two differ


def is_mx(weight_format: str) -> bool:
    """True for an MX format name, False for "int"; anything else raises."""
    if weight_format == "int":
        return False
    if weight_format not in FORMATS:
        raise ValueError("weight_format must be 'int', %s, got %r" % (_NAMES, weight_format))
    return True


def bits_per_weight(fmt: str) -> float:
    """Element bits plus the block's share of its 8-bit scale: 4.25, 6.25 or 8.25."""
    return FORMATS[fmt][1] + 8.0 / BLOCK


def blocks(row_len: int) -> int:
    return -(-row_len // BLOCK)


_Out = Optional[Union[torch.Tensor, int]]


@dataclass
class MXItem:
    """One fp32 tensor viewed as [rows, -1] (rows = shape[0] unless given) and what
    to write for it.  The outputs may also be raw device addresses (int) into
    memory the caller keeps alive until the call has run.  ``codes``: uint8
    [rows, nb, 16] (mxfp4, element 2k in the low nibble), [rows, nb, 32] (mxfp8) or
    [rows, nb, 24] (mxfp6_*: 32 six-bit codes packed densely, element i in bits [6i, 6i+6));
    ``scales``: uint8 [rows, nb]; ``esum``: fp32 [numel / khw]; nb = ceil(row_len / 32)."""
    src: torch.Tensor
    fmt: str = "mxfp4"
    dst: _Out = None        # dequantized output (may be src)
    codes: _Out = None
    scales: _Out = None
    esum: _Out = None
    khw: int = 1
    rows: Optional[int] = None


def allocate(src: torch.Tensor, fmt: str = "mxfp4", khw: int = 1, in_place: bool = False, want_dst: bool = True,
             want_codes: bool = True, want_esum: bool = False) -> MXItem:
    """An MXItem with freshly allocated outputs on src's device."""
    rows = src.shape[0] if src.dim() > 0 else 1
    nb = blocks(src.numel() // rows)
    dev = src.device
    return MXItem(
        src=src, fmt=fmt, khw=khw, rows=rows,
        dst=(src if in_place else torch.empty_like(src)) if want_dst else None,
        codes=torch.empty((rows, nb, FORMATS[fmt][2]), dtype=torch.uint8, device=dev) if want_codes else None,
        scales=torch.empty((rows, nb), dtype=torch.uint8, device=dev) if want_codes else None,
        esum=torch.empty(src.numel() // khw, dtype=torch.float32, device=dev) if want_esum else None)


_MX = np.dtype([("src", "<u8"), ("dst", "<u8"), ("codes", "<u8"), ("scales", "<u8"), ("esum", "<u8"),
                ("rows", "<i8"), ("row_len", "<i8"), ("khw", "<i4"), ("format", "<i4"), ("flags", "<i4"),
                ("reserved", "<i4")])
assert _MX.itemsize == C.sizeof(_lib.MxDesc)
assert all(_MX.fields[f][1] == getattr(_lib.MxDesc, f).offset for f, _ in _lib.MxDesc._fields_)


def mx_quantize(items: Sequence[MXItem], stream: Optional[torch.cuda.Stream] = None) -> List[MXItem]:
    """Quantize every item in one C call, asynchronous on ``stream`` (the current
    one by default).  Returns the items."""
    items = list(items)
    if not items:
        return items
    tab, keep = [], []
    for it in items:
        _lib.require_device(it.src, *(t for t in (it.dst, it.esum) if not isinstance(t, int)))
        if it.src.device != items[0].src.device:
            raise ValueError("every tensor of an mx_quantize call must live on one device")
        if it.fmt not in FORMATS:
            raise ValueError("fmt must be %s, got %r" % (_NAMES, it.fmt))
        if it.src.numel() == 0:
            raise ValueError("empty tensors have nothing to quantize")
        for name in ("codes", "scales"):
            t = getattr(it, name)
            if t is not None and not isinstance(t, int) and not (t.is_cuda and t.dtype == torch.uint8 and
                                                                 t.is_contiguous()):
                raise TypeError(name + ": contiguous uint8 on the GPU")
        rows = it.rows if it.rows is not None else (it.src.shape[0] if it.src.dim() > 0 else 1)
        row_len = it.src.numel() // rows
        if rows * row_len != it.src.numel():
            raise ValueError("rows does not divide the tensor")
        nb = blocks(row_len)
        for name, need in (("codes", rows * nb * FORMATS[it.fmt][2]), ("scales", rows * nb),
                           ("esum", it.src.numel() // max(it.khw, 1)), ("dst", it.src.numel())):
            t = getattr(it, name)
            if t is not None and not isinstance(t, int) and t.numel() < need:
                raise ValueError("%s holds %d elements, %d needed" % (name, t.numel(), need))
        ptr = lambda t: t if isinstance(t, int) else (t.data_ptr() if t is not None else 0)   # noqa: E731
        tab.append((it.src.data_ptr(), ptr(it.dst), ptr(it.codes), ptr(it.scales), ptr(it.esum), rows, row_len,
                    int(it.khw), FORMATS[it.fmt][0], 0, 0))
        keep += [t for t in (it.dst, it.codes, it.scales, it.esum) if isinstance(t, torch.Tensor)]
    dev = items[0].src.device
    arr = np.array(tab, dtype=_MX)
    descs = arr.ctypes.data_as(C.POINTER(_lib.MxDesc))
    L = _lib.load()
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):   # the workspace is stream-ordered (caching allocator) with the launch
        # a too-small workspace (0 for a bad list) makes the call itself report the list's error
        ws = torch.empty(max(int(L.dfq_mx_quantize_ws_bytes(descs, len(items))), 256), dtype=torch.uint8, device=dev)
    if any(it.dst is not None for it in items):
        _lib.weights_changed()
    _lib.check(L.dfq_mx_quantize_batch(descs, len(items), ws.data_ptr(), ws.numel(), C.c_void_p(s.cuda_stream)),
               "dfq_mx_quantize_batch", ValueError)
    if stream is not None and s != torch.cuda.current_stream(dev):
        for t in keep:
            t.record_stream(s)
    return items


def _tables(fmt: str, device) -> torch.Tensor:
    """Value of every code (sign included), fp32."""
    if fmt == "mxfp4":
        mag = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float32)
    elif fmt == "mxfp6_e2m3":   # s ee mmm, bias 1: m / 8, (8 + m) * 2^(e - 4)
        c = torch.arange(32, dtype=torch.int32)
        e, m = c >> 3, (c & 7).to(torch.float32)
        mag = torch.where(e == 0, m * 2.0 ** -3, (8.0 + m) * torch.pow(2.0, (e - 4).to(torch.float32)))
    elif fmt == "mxfp6_e3m2":   # s eee mm, bias 3: m / 16, (4 + m) * 2^(e - 5)
        c = torch.arange(32, dtype=torch.int32)
        e, m = c >> 2, (c & 3).to(torch.float32)
        mag = torch.where(e == 0, m * 2.0 ** -4, (4.0 + m) * torch.pow(2.0, (e - 5).to(torch.float32)))
    else:
        c = torch.arange(128, dtype=torch.int32)
        e, m = c >> 3, (c & 7).to(torch.float32)
        mag = torch.where(e == 0, m * 2.0 ** -9, (8.0 + m) * torch.pow(2.0, (e - 10).to(torch.float32)))
        mag[127] = float("nan")   # the E4M3 NaN code: never produced
    return torch.cat([mag, -mag]).to(device)


def pack6(c: torch.Tensor) -> torch.Tensor:
    """[..., 4k] six-bit codes -> [..., 3k] bytes: four codes w = c0 | c1 << 6 | c2 << 12 |
    c3 << 18 are the bytes w & 0xFF, (w >> 8) & 0xFF, w >> 16 (the FP6 ``codes`` layout)."""
    q = c.to(torch.int64).reshape(*c.shape[:-1], -1, 4)
    w = q[..., 0] | (q[..., 1] << 6) | (q[..., 2] << 12) | (q[..., 3] << 18)
    return torch.stack([w & 0xFF, (w >> 8) & 0xFF, w >> 16], dim=-1).reshape(*c.shape[:-1], -1).to(torch.uint8)


def unpack6(b: torch.Tensor) -> torch.Tensor:
    """The inverse of ``pack6``: [..., 3k] bytes -> [..., 4k] six-bit codes (int64)."""
    t = b.to(torch.int64).reshape(*b.shape[:-1], -1, 3)
    w = t[..., 0] | (t[..., 1] << 8) | (t[..., 2] << 16)
    return torch.stack([w & 0x3F, (w >> 6) & 0x3F, (w >> 12) & 0x3F, w >> 18], dim=-1).reshape(*b.shape[:-1], -1)


def mx_dequantize(codes: torch.Tensor, scales: torch.Tensor, shape, fmt: str) -> torch.Tensor:
    """The fp32 tensor of ``shape`` that ``codes`` ([rows, nb, 16 | 24 | 32] uint8) and
    ``scales`` ([rows, nb] uint8) stand for: y = +-q * 2^(scale - 127), every step
    exact in fp32 -- bit for bit the ``dst`` of ``mx_quantize``.  Pure torch, CPU or GPU."""
    if fmt not in FORMATS:
        raise ValueError("fmt must be %s, got %r" % (_NAMES, fmt))
    n = 1
    for s in shape:
        n *= int(s)
    rows, nb = scales.shape
    c = codes.reshape(rows, nb, FORMATS[fmt][2]).to(torch.int64)
    if fmt == "mxfp4":
        c = torch.stack([c & 0xF, c >> 4], dim=-1)   # element 2k low, 2k + 1 high
    elif FORMATS[fmt][1] == 6:
        c = unpack6(c)
    q = _tables(fmt, codes.device)[c.reshape(rows, nb, BLOCK)]
    # 2^(scale - 127) from its bit pattern (byte 0, only written for an all-zero block, reads as 0)
    up = (scales.to(torch.int32) << 23).view(torch.float32)
    y = (q * up.unsqueeze(-1)).reshape(rows, nb * BLOCK)
    return y[:, :n // rows].reshape(tuple(shape))
