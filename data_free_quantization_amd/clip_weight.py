"""Weight clipping.

``clip_weight`` is the drop-in for the reference's ``clip_weight.py``
(clip_weight.py:4-33): clamp every target layer's weight to [lo, hi] in place (HIP
``dfq_clamp_batch``: one call, 64 weights per launch).  The same clamp is also
available fused into the quantize sweep (``quantize_targ_layer(..., clip=(lo, hi))``).

``search_clip`` / ``clip_search`` (extension, no reference counterpart) choose the
clamp from the weights themselves: per channel or per tensor, the one of K
candidate ranges between the min-max range and ``min_frac`` of it whose
quantization noise -- the sweep's own arithmetic, measured against the unclamped
weight -- is smallest (``dfq_clip_search_batch``, include/dfq_hip.h; DESIGN.md
3.6).  Candidate 0 is the min-max range, so the result is never noisier than
today's.  The defaults (16 candidates down to half the range) are interface
choices: with no dataset there is nothing to tune them on.  There is no CPU
fallback: CPU tensors raise."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from . import _lib


def clip_weight(graph, range_clip=None, targ_type=[nn.Conv2d, nn.Linear]):
    if range_clip is None:
        range_clip = [-15, 15]
    assert isinstance(range_clip, (list, tuple)) and len(range_clip) == 2, \
        "range_clip should be a list or tuple of two elements"
    lo, hi = float(range_clip[0]), float(range_clip[1])
    _lib.weights_changed()
    ws = []
    for idx, layer in graph.items():
        if isinstance(layer, tuple(targ_type)):
            if hasattr(layer, "weight"):
                w = layer.weight.data
                _lib.require_device(w)
                ws.append(w)
            else:
                print(f"Warning: Layer at index {idx} does not have 'weight' attribute")
        else:
            print(f"Warning: Layer at index {idx} is not in the target type list for clipping")
    if ws:   # every clamp in one call (64 weights per launch)
        ptrs = (C.c_void_p * len(ws))(*[w.data_ptr() for w in ws])
        ns = (C.c_int64 * len(ws))(*[w.numel() for w in ws])
        _lib.check(_lib.load().dfq_clamp_batch(ptrs, ns, len(ws), lo, hi, _lib.stream_of(ws[0])), "dfq_clamp_batch")


_CLIP = np.dtype([("w", "<u8"), ("rows", "<i8"), ("row_len", "<i8"), ("bits", "<i4"), ("mode", "<i4"),
                  ("candidates", "<i4"), ("flags", "<i4"), ("min_frac", "<f4"), ("reserved", "<i4"),
                  ("choice", "<u8"), ("range", "<u8"), ("noise", "<u8"), ("range_enc", "<u8")])
assert _CLIP.itemsize == C.sizeof(_lib.ClipSearchDesc)
assert all(_CLIP.fields[f][1] == getattr(_lib.ClipSearchDesc, f).offset for f, _ in _lib.ClipSearchDesc._fields_)


@dataclass
class ClipItem:
    """One fp32 weight (clamped in place unless ``dry``) viewed as [shape[0], -1],
    and how its candidates are quantized."""
    w: torch.Tensor
    bits: int = 8
    per_channel: bool = False
    symmetric: bool = False
    candidates: int = 16
    min_frac: float = 0.5
    dry: bool = False
    # per-tensor modes: 2 int32 device words that receive the (min, max) of the
    # weight as the call leaves it, in dfq_range's encoding (SweepItem.range_enc)
    range_enc: Optional[torch.Tensor] = None

    def mode(self) -> int:
        if self.per_channel:
            return _lib.DFQ_CHANNEL_SYM if self.symmetric else _lib.DFQ_CHANNEL_ASYM
        return _lib.DFQ_TENSOR_SYM if self.symmetric else _lib.DFQ_TENSOR_ASYM


class ClipSearchCall:
    """A prepared ``clip_search`` call: the descriptor table, the output
    allocations and the workspace.  ``run()`` is the one C call (asynchronous on the
    stream); it may be repeated (each run searches the weights as it finds them)."""

    def __init__(self, items: Sequence[ClipItem]):
        items = list(items)
        self.items = items
        self.results: List[Dict] = []
        self._n = len(items)
        if not items:
            return
        units = []
        for it in items:
            _lib.require_device(it.w)
            if it.w.device != items[0].w.device:
                raise ValueError("every weight of a clip_search call must live on one device")
            if it.w.numel() == 0:
                raise ValueError("empty tensors have no range to search")
            units.append(it.w.shape[0] if (it.per_channel and it.w.dim() > 0) else 1)
            r = it.range_enc
            if r is not None and not (r.is_cuda and r.dtype == torch.int32 and r.numel() >= 2 and r.is_contiguous()):
                raise TypeError("range_enc: 2 contiguous int32 words on the GPU")
        self.device = dev = items[0].w.device
        total = sum(units)
        self.choice = torch.empty(total, dtype=torch.int32, device=dev)
        self.range = torch.empty((total, 2), dtype=torch.float32, device=dev)
        self.noise = torch.empty((total, 2), dtype=torch.float64, device=dev)
        cb, rb, nb_ = self.choice.data_ptr(), self.range.data_ptr(), self.noise.data_ptr()
        tab, u0 = [], 0
        for it, u in zip(items, units):
            rows = it.w.shape[0] if it.w.dim() > 0 else 1
            tab.append((it.w.data_ptr(), rows, it.w.numel() // rows, int(it.bits), it.mode(), int(it.candidates),
                        _lib.DFQ_CLIP_SEARCH_DRY if it.dry else 0, float(it.min_frac), 0,
                        cb + 4 * u0, rb + 8 * u0, nb_ + 16 * u0,
                        it.range_enc.data_ptr() if (it.range_enc is not None and not it.per_channel) else 0))
            self.results.append({"choice": self.choice[u0:u0 + u], "range": self.range[u0:u0 + u],
                                 "noise": self.noise[u0:u0 + u]})
            u0 += u
        self._tab = np.array(tab, dtype=_CLIP)
        self._descs = self._tab.ctypes.data_as(C.POINTER(_lib.ClipSearchDesc))
        nb = int(_lib.load().dfq_clip_search_ws_bytes(self._descs, self._n))
        if nb < 0:
            raise ValueError("dfq_clip_search_ws_bytes: invalid list (bits 2..16, candidates 1..%d, min_frac in "
                             "[0, 1])" % _lib.DFQ_CLIP_MAX_CANDIDATES)
        self._ws = torch.empty(nb, dtype=torch.uint8, device=dev)   # stream-ordered (caching allocator)
        self._made_on = torch.cuda.current_stream(dev)
        self._writes = not all(it.dry for it in items)

    def run(self, stream: Optional[torch.cuda.Stream] = None) -> List[Dict]:
        if not self._n:
            return self.results
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        if s != self._made_on:   # the allocations must outlive work queued on another stream
            for t in (self._ws, self.choice, self.range, self.noise):
                t.record_stream(s)
        if self._writes:
            _lib.weights_changed()
        _lib.check(_lib.load().dfq_clip_search_batch(self._descs, self._n, self._ws.data_ptr(), self._ws.numel(),
                                                     C.c_void_p(s.cuda_stream)), "dfq_clip_search_batch", ValueError)
        return self.results


def clip_search(items: Sequence[ClipItem], stream: Optional[torch.cuda.Stream] = None) -> List[Dict]:
    """The clip-range search of every item in one C call, asynchronous on
    ``stream``.  Per item a dict of device tensors: ``choice`` int32 [units],
    ``range`` float32 [units, 2] (the chosen lo, hi) and ``noise`` float64
    [units, 2] (the min-max range's noise, the chosen range's); units = shape[0]
    per channel, 1 per tensor."""
    return ClipSearchCall(items).run(stream)


def search_clip(graph, bits, *, granularity="tensor", symmetric=False, candidates=16, min_frac=0.5,
                targ_type=[nn.Conv2d, nn.Linear], dry=False, weight_ranges: Optional[Dict] = None):
    """Clamp every target layer's weight, in place, to the candidate range that
    minimizes its own quantization noise at ``bits`` (per channel or per tensor, as
    ``quantize_targ_layer`` in the same mode will quantize it): one C call for all
    layers.  ``dry``: search and report only.  ``weight_ranges``: the dict of
    ``merge_batchnorm(ranges=...)``; in the per-tensor modes each entry is rewritten
    with the clamped weight's range, so ``quantize_targ_layer(weight_ranges=...)``
    right after stays one pass.  Returns {key: {"choice", "range", "noise"}} as
    device tensors (see ``clip_search``)."""
    if granularity not in ("tensor", "channel"):
        raise ValueError("granularity must be 'tensor' or 'channel'")
    per_channel = granularity == "channel"
    tt = tuple(targ_type)
    keys, items = [], []
    for idx, layer in graph.items():
        if type(layer) not in tt:
            continue
        w = layer._parameters["weight"].detach()
        keys.append(idx)
        items.append(ClipItem(w, bits=bits, per_channel=per_channel, symmetric=symmetric, candidates=candidates,
                              min_frac=min_frac, dry=dry,
                              range_enc=weight_ranges.get(layer) if (weight_ranges and not per_channel) else None))
    return dict(zip(keys, clip_search(items)))
