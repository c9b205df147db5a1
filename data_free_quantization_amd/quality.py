"""Data-free quantization quality report: per-channel signal, noise and range.

The DFQ paper's argument is about two quantities the weights alone give: the
per-channel range spread that cross-layer equalization evens out, and the
quantization noise of each layer.  ``pair_stats`` measures both on the GPU for
many (reference, compared) weight pairs in one call (``dfq_pair_stats_batch``,
include/dfq_hip.h); ``weight_report`` turns a model's worth of them into a JSON
document (``main_dfq --report``, ``pipeline.run_dfq(report=...)``).

There is no CPU fallback: CPU tensors raise.  Biases are out of scope (bias
correction rewrites them after the weights are final).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

FORMAT = "dfq-quality/1"
SIGNAL, NOISE, MAX_ERR, MAX_ABS = 0, 1, 2, 3   # slots of a row record / of a pair's totals

_PAIR = np.dtype([("x", "<u8"), ("y", "<u8"), ("rows_out", "<u8"), ("total_out", "<u8"), ("rows", "<i8"),
                  ("row_len", "<i8")])
assert _PAIR.itemsize == C.sizeof(_lib.PairDesc)
assert all(_PAIR.fields[f][1] == getattr(_lib.PairDesc, f).offset for f, _ in _lib.PairDesc._fields_)


@dataclass
class PairStats:
    """One pair's result: ``rows`` [rows, 4] (None without per_row) and ``total``
    [4], float64 device tensors; slots {signal, noise, max_err, max_abs}."""
    rows: Optional[torch.Tensor]
    total: torch.Tensor


class PairStatsCall:
    """A prepared ``pair_stats`` call: the descriptor table, one output allocation
    and the workspace.  ``run()`` is the one C call (two launches, asynchronous on
    the stream); it may be repeated."""

    def __init__(self, pairs: Sequence[Tuple[torch.Tensor, torch.Tensor]], per_row: bool = True):
        pairs = list(pairs)
        self._keep = pairs
        self.results: List[PairStats] = []
        self._n = len(pairs)
        if not pairs:
            return
        shapes = []
        for x, y in pairs:
            _lib.require_device(x, y)
            if x.shape != y.shape:
                raise ValueError(f"pair shapes differ: {tuple(x.shape)} and {tuple(y.shape)}")
            if x.device != y.device or x.device != pairs[0][0].device:
                raise ValueError("every tensor of a pair_stats call must live on one device")
            if x.numel() == 0:
                raise ValueError("empty tensors have no statistics")
            rows = x.shape[0] if x.dim() > 0 else 1   # the sweep's [rows, row_len] view
            shapes.append((rows, x.numel() // rows))
        self.device = pairs[0][0].device
        n_rows = sum(r for r, _ in shapes) if per_row else 0
        self.out = torch.empty(4 * (n_rows + self._n), dtype=torch.float64, device=self.device)
        base, rec = self.out.data_ptr(), 4 * 8
        tab, row0 = [], 0
        for i, ((x, y), (rows, row_len)) in enumerate(zip(pairs, shapes)):
            total = self.out[4 * (n_rows + i):4 * (n_rows + i + 1)]
            rview = self.out[4 * row0:4 * (row0 + rows)].view(rows, 4) if per_row else None
            tab.append((x.data_ptr(), y.data_ptr(), base + rec * row0 if per_row else 0, base + rec * (n_rows + i),
                        rows, row_len))
            self.results.append(PairStats(rview, total))
            if per_row:
                row0 += rows
        self._tab = np.array(tab, dtype=_PAIR)
        self._descs = self._tab.ctypes.data_as(C.POINTER(_lib.PairDesc))
        nb = int(_lib.load().dfq_pair_stats_ws_bytes(self._descs, self._n))
        if nb < 0:
            raise ValueError("dfq_pair_stats_ws_bytes: invalid pair list")
        self._ws = torch.empty(nb, dtype=torch.uint8, device=self.device)
        self._made_on = torch.cuda.current_stream(self.device)

    def run(self, stream: Optional[torch.cuda.Stream] = None) -> List[PairStats]:
        if not self._n:
            return self.results
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        if s != self._made_on:   # the allocations must outlive work queued on another stream
            self.out.record_stream(s)
            self._ws.record_stream(s)
        _lib.check(_lib.load().dfq_pair_stats_batch(self._descs, self._n, self._ws.data_ptr(), self._ws.numel(),
                                                    C.c_void_p(s.cuda_stream)), "dfq_pair_stats_batch", ValueError)
        return self.results


def pair_stats(pairs, *, per_row: bool = True, stream: Optional[torch.cuda.Stream] = None) -> List[PairStats]:
    """Signal, noise, worst error and range of every ``(x, y)`` pair of CUDA fp32
    tensors (x the reference), per row of the [shape[0], -1] view and per pair:
    one C call, one output allocation, asynchronous on ``stream``."""
    return PairStatsCall(pairs, per_row=per_row).run(stream)


def sqnr_db(signal: float, noise: float) -> Optional[float]:
    """10 log10(signal / noise); None where either is zero (no finite figure)."""
    signal, noise = float(signal), float(noise)
    if noise == 0.0 or signal == 0.0:
        return None
    return 10.0 * math.log10(signal / noise)


def _targets(graph, targ_type):
    return [k for k in graph if type(graph[k]) in tuple(targ_type)]


def snapshot(graph, targ_type) -> Dict:
    """Clones of every target layer's weight, as views (each 256-B aligned, like
    the weights themselves) of one flat device buffer: {key: view}."""
    keys = _targets(graph, targ_type)
    if not keys:
        return {}
    ws = [graph[k].weight.detach() for k in keys]
    _lib.require_device(*ws)
    offs, n = [], 0
    for w in ws:
        offs.append(n)
        n += -(-w.numel() // 64) * 64
    flat = torch.empty(n, dtype=torch.float32, device=ws[0].device)
    snap = {}
    for k, w, o in zip(keys, ws, offs):
        v = flat[o:o + w.numel()].view(w.shape)
        v.copy_(w)
        snap[k] = v
    return snap


def layer_entry(key, type_name: str, shape, rows: np.ndarray, total: np.ndarray) -> dict:
    """One layer of the report from its [rows, 4] records and [4] totals (host
    arithmetic only)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    total = np.asarray(total, dtype=np.float64).reshape(4)
    sig, noi = rows[:, SIGNAL], rows[:, NOISE]
    noisy = np.flatnonzero(noi != 0.0)
    worst = worst_db = None
    if noisy.size:   # the lowest signal / noise among the rows that lost anything (first on ties)
        worst = int(noisy[np.argmin(sig[noisy] / noi[noisy])])
        worst_db = sqnr_db(sig[worst], noi[worst])
    peak = float(rows[:, MAX_ABS].max())
    prec = rows[:, MAX_ABS] / peak if peak > 0.0 else None
    return {
        "key": str(key), "type": type_name, "shape": [int(s) for s in shape],
        "elements": int(np.prod([int(s) for s in shape], dtype=np.int64)) if len(shape) else 1,
        "signal": float(total[SIGNAL]), "noise": float(total[NOISE]),
        "sqnr_db": sqnr_db(total[SIGNAL], total[NOISE]),
        "worst_channel": worst, "worst_channel_sqnr_db": worst_db,
        "max_abs_err": float(total[MAX_ERR]), "max_abs_weight": float(total[MAX_ABS]),
        "channel_precision_mean": float(prec.mean()) if prec is not None else None,
        "channel_precision_min": float(prec.min()) if prec is not None else None,
    }


def model_entry(layers: List[dict]) -> dict:
    """The model's line: sums over the layers in list order, the worst layer."""
    signal = noise = 0.0
    for e in layers:
        signal += e["signal"]
        noise += e["noise"]
    rated = [e for e in layers if e["sqnr_db"] is not None]
    return {"signal": signal, "noise": noise, "sqnr_db": sqnr_db(signal, noise),
            "worst_layer": min(rated, key=lambda e: e["sqnr_db"])["key"] if rated else None,
            "elements": sum(e["elements"] for e in layers)}


def build_report(entries, config: dict) -> dict:
    """entries: (key, type name, shape, rows [rows, 4], total [4]) per layer."""
    layers = [layer_entry(*e) for e in entries]
    return {"format": FORMAT, "config": dict(config), "layers": layers, "model": model_entry(layers)}


def weight_report(graph, snap: Dict, *, config: dict, clip_search: Optional[Dict] = None,
                  mx_scales: Optional[Dict] = None) -> dict:
    """The report of ``graph``'s target weights against ``snap`` (``snapshot``'s
    clones, taken before the quantization): one pair_stats call over
    (snap[k], graph[k].weight) in graph order, one device-to-host copy.

    ``clip_search``: what ``clip_weight.search_clip`` returned for a search run
    between the snapshot and the quantization.  Each layer entry then also counts
    its units (``clip_units``: channels, or 1 for the tensor), those that chose a
    narrower range than min-max (``clip_narrowed``) and those that chose the narrowest candidate
    (``clip_at_edge``: many of them say min_frac should be lower); the caller
    records the search's settings in ``config``.

    ``mx_scales``: {key: stored scale bytes [rows, nb]} of a quantization with the MX scale
    search (``config["weight_format"]`` names the format).  Each of those layers then also
    gets ``scale_raised``: the blocks whose stored byte is above the floor rule's, which is
    computed here from ``snap`` (mx.floor_scale_bytes)."""
    keys = [k for k in graph if k in snap]
    call = PairStatsCall([(snap[k], graph[k].weight.detach()) for k in keys])
    call.run()
    host = call.out.cpu().numpy() if keys else np.zeros(0)
    n_rows = (host.size - 4 * len(keys)) // 4
    entries, row0 = [], 0
    for i, k in enumerate(keys):
        w = graph[k].weight
        rows = w.shape[0] if w.dim() > 0 else 1
        entries.append((k, type(graph[k]).__name__, tuple(w.shape), host[4 * row0:4 * (row0 + rows)].reshape(rows, 4),
                        host[4 * (n_rows + i):4 * (n_rows + i + 1)]))
        row0 += rows
    rep = build_report(entries, config)
    if clip_search is not None:
        last = int(config["clip_candidates"]) - 1
        found = [k for k in keys if k in clip_search]
        flat = torch.cat([clip_search[k]["choice"].reshape(-1) for k in found]).cpu().numpy() if found else None
        at = 0
        for e, k in zip(rep["layers"], keys):
            if k not in clip_search:
                continue
            c = flat[at:at + clip_search[k]["choice"].numel()]
            at += c.size
            e["clip_units"] = int(c.size)
            e["clip_narrowed"] = int((c > 0).sum())
            e["clip_at_edge"] = int(((c > 0) & (c == last)).sum())
    if mx_scales is not None:
        from .mx import floor_scale_bytes
        found = [k for k in keys if k in mx_scales]
        raised = torch.stack([(mx_scales[k] > floor_scale_bytes(snap[k], config["weight_format"])).sum()
                              for k in found]).cpu().tolist() if found else []
        by_key = dict(zip(found, raised))
        for e, k in zip(rep["layers"], keys):
            if k in by_key:
                e["scale_raised"] = int(by_key[k])
    return rep
