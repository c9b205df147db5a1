"""Sum rounding (extension, no reference counterpart): nearest rounding plus the few
flips, of the elements whose rounding was closest to a tie, after which the summed
rounding error of every kernel (KH*KW taps) and of every output channel is at most
half a quantization step (``dfq_sum_round_batch``, include/dfq_hip.h; DESIGN.md
3.10; after SQuant, ICLR 2022).  Nearest rounding leaves those sums to chance: at 4
bits they are a shift of the layer's expected output.  The grid -- scale and zero --
is the sweep's, bit for bit; only codes move, each by at most one step.  Data-free,
weight-only, one C call over the layer list.  There is no CPU fallback: CPU tensors
raise."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .utils.quantize import QuantResult, _code_dtype

_SR = np.dtype([("src", "<u8"), ("dst", "<u8"), ("codes", "<u8"), ("scale", "<u8"), ("zero", "<u8"), ("flips", "<u8"),
                ("rows", "<i8"), ("row_len", "<i8"), ("khw", "<i4"), ("bits", "<i4"), ("mode", "<i4"),
                ("reserved", "<i4")])
assert _SR.itemsize == C.sizeof(_lib.SumRoundDesc)
assert all(_SR.fields[f][1] == getattr(_lib.SumRoundDesc, f).offset for f, _ in _lib.SumRoundDesc._fields_)


@dataclass
class SumRoundItem:
    """One fp32 weight viewed as [shape[0], -1], every row as kernels of ``khw``
    consecutive taps (``sweep.khw_of``; 1 for Linear and 1x1), and how it is rounded.
    ``dst`` may be ``src`` (in place); None allocates."""
    src: torch.Tensor
    dst: Optional[torch.Tensor] = None
    bits: int = 8
    per_channel: bool = False
    symmetric: bool = False
    khw: int = 1
    want_codes: bool = True
    want_flips: bool = False

    def mode(self) -> int:
        if self.per_channel:
            return _lib.DFQ_CHANNEL_SYM if self.symmetric else _lib.DFQ_CHANNEL_ASYM
        return _lib.DFQ_TENSOR_SYM if self.symmetric else _lib.DFQ_TENSOR_ASYM


@dataclass
class SumRoundResult(QuantResult):
    """``QuantResult`` (``esum`` stays None) and, when asked for, the flip counts."""
    flips: Optional[torch.Tensor] = None   # int32 [rows, 2]: kernel-stage and channel-stage flips per row


def sum_round(items: Sequence[SumRoundItem], stream: Optional[torch.cuda.Stream] = None) -> List[SumRoundResult]:
    """Sum rounding of every item in one C call, asynchronous on ``stream``.  Each
    weight at most once per call; a weight's results are the same bits whatever the
    rest of the list."""
    items = list(items)
    if not items:
        return []
    dev = items[0].src.device
    tab, out = [], []
    for it in items:
        _lib.require_device(it.src, it.dst)
        if it.src.device != dev:
            raise ValueError("every weight of a sum_round call must live on one device")
        if it.src.numel() == 0:
            raise ValueError("empty tensors have no range to round on")
        if not 2 <= int(it.bits) <= 8:
            raise ValueError("sum_round takes bits 2..8, got %r" % (it.bits,))
        rows = it.src.shape[0] if it.src.dim() > 0 else 1
        row_len = it.src.numel() // rows
        if row_len > _lib.DFQ_SR_MAX_ROW:
            raise NotImplementedError("sum_round keeps a row in LDS: row_len %d exceeds DFQ_SR_MAX_ROW = %d"
                                      % (row_len, _lib.DFQ_SR_MAX_ROW))
        if not 1 <= int(it.khw) <= _lib.DFQ_SR_MAX_KHW:
            raise NotImplementedError("sum_round gives a kernel to one lane: khw %r is outside 1..DFQ_SR_MAX_KHW = %d"
                                      % (it.khw, _lib.DFQ_SR_MAX_KHW))
        if row_len % int(it.khw):
            raise ValueError("row_len %d is not a multiple of khw %d" % (row_len, it.khw))
        if it.dst is not None and it.dst.shape != it.src.shape:
            raise ValueError("dst must have src's shape")
        npar = rows if it.per_channel else 1
        res = SumRoundResult(
            dq=it.dst if it.dst is not None else torch.empty_like(it.src),
            codes=torch.empty(it.src.shape, dtype=_code_dtype(it.bits, it.symmetric), device=dev) if it.want_codes else None,
            scale=torch.empty(npar, dtype=torch.float32, device=dev),
            zero=torch.empty(npar, dtype=torch.float32, device=dev),
            flips=torch.empty((rows, 2), dtype=torch.int32, device=dev) if it.want_flips else None)
        out.append(res)
        tab.append((it.src.data_ptr(), res.dq.data_ptr(), res.codes.data_ptr() if res.codes is not None else 0,
                    res.scale.data_ptr(), res.zero.data_ptr(), res.flips.data_ptr() if res.flips is not None else 0,
                    rows, row_len, int(it.khw), int(it.bits), it.mode(), 0))
    arr = np.array(tab, dtype=_SR)
    descs = arr.ctypes.data_as(C.POINTER(_lib.SumRoundDesc))
    L = _lib.load()
    nb = int(L.dfq_sum_round_ws_bytes(descs, len(items)))
    if nb < 0:
        raise ValueError("dfq_sum_round_ws_bytes: invalid list (bits 2..8, row_len <= %d, khw <= %d dividing row_len, "
                         "at most 65535 weights)" % (_lib.DFQ_SR_MAX_ROW, _lib.DFQ_SR_MAX_KHW))
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)   # stream-ordered (caching allocator)
    if s != torch.cuda.current_stream(dev):   # the allocations must outlive work queued on another stream
        for t in [ws] + [t for r in out for t in (r.dq, r.codes, r.scale, r.zero, r.flips) if t is not None]:
            t.record_stream(s)
    if any(it.dst is it.src for it in items):
        _lib.weights_changed()
    _lib.check(L.dfq_sum_round_batch(descs, len(items), ws.data_ptr(), ws.numel(), C.c_void_p(s.cuda_stream)),
               "dfq_sum_round_batch", ValueError)
    return out
