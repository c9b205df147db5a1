"""The DFQ weight-transform pipeline in main_dfq's stage order
(main_dfq.py:188-231), on the GPU:

  merge_batchnorm -> create_relation -> cross_layer_equalization ->
  bias_absorption -> set_layer_bits -> merge_batchnorm -> [search_clip] ->
  quantize_targ_layer -> clip_weight -> bias_correction

``bc_mode``:
  * "literal"   -- exactly the reference: BC walks with the graph's keys (a no-op
                   with opaque keys)
  * "reference" -- the reference's coded arithmetic (requires positional keys)
  * "fused"     -- extension: E comes from the quantize sweep itself (the error
                   of the quantization actually applied), clip fused in the sweep
"""
from __future__ import annotations

import time
from typing import Callable, Dict, Optional

import torch
import torch.nn as nn

from . import Cross_layer_equal as cle
from . import quality
from .bias_absorption import bias_absorption
from .bias_correction import bias_correction
from .clip_weight import clip_weight, search_clip
from .utils.layer_transform import esum_source, merge_batchnorm, quantize_targ_layer
from .utils.quantize import set_layer_bits
from .utils.relation import create_relation


def run_dfq(model: nn.Module, graph, bottoms, targ, *, relu: bool = True, equalize: bool = True,
            absorption: bool = True, quantize: bool = True, clip: bool = True, correction: bool = True,
            bits_weight: int = 8, bits_activation: int = 8, bits_bias: int = 8, granularity: str = "tensor",
            symmetric: bool = False, bc_mode: str = "literal", clip_range=(-15, 15),
            stage_hook: Optional[Callable[[str], None]] = None, timings: Optional[Dict] = None,
            report: Optional[dict] = None, clip_search: Optional[dict] = None, weight_format: str = "int",
            mx_scale_search: bool = False):
    """Run the DFQ stages on ``model`` (already on the GPU) in place; returns the
    equalization relations.  ``report``: a dict to fill with the quality report
    (quality.weight_report) of the quantized weights against their values after
    the second BN fold; needs ``quantize``.  None: no clone, no extra launch.
    ``clip_search``: None, or {"candidates": K, "min_frac": f} (either may be left
    out: 16, 0.5) to clamp every weight, before it is quantized, to the range that
    minimizes its own quantization noise (clip_weight.search_clip; stage
    "clipsearch", after the report's snapshot, so the report measures the noise
    against the unclamped weights); needs ``quantize``.  Bias correction sees the
    clamped weight as its input.
    ``weight_format``: "int" (the integer grid of ``bits_weight`` / ``granularity`` /
    ``symmetric``), or "mxfp4" / "mxfp6_e2m3" / "mxfp6_e3m2" / "mxfp8": OCP MX block-scaled
    weights (mx.py; 4.25 / 6.25 / 6.25 / 8.25 bits per weight), to which those three do
    not apply.  An MX format raises ValueError with ``clip_search`` (the
    search measures integer grids), with ``bc_mode="reference"`` (its error term is the
    integer quantizer's) and with ``clip`` under ``bc_mode="fused"`` (the MX pass has no
    fused clamp); ``clip`` as its own stage after quantization stays, in the reference's
    order.
    ``mx_scale_search``: with an MX ``weight_format`` (ValueError otherwise), every block takes
    the better of the floor rule's scale and the next one up by its own quantization noise
    (quantize_targ_layer(mx_scale_search=True)).  The report's config then
    holds ``mx_scale_search`` and each layer ``scale_raised``, the blocks that took the higher
    scale.  Off: no new key, no new launch."""
    from .mx import bits_per_weight, is_mx
    mx_fmt = is_mx(weight_format)
    if mx_scale_search and not mx_fmt:
        raise ValueError("mx_scale_search needs an MX weight_format, got %r" % (weight_format,))
    if mx_fmt:
        if clip_search is not None:
            raise ValueError("weight_format=%r conflicts with clip_search: the search minimizes an integer "
                             "grid's noise" % weight_format)
        if correction and bc_mode == "reference":
            raise ValueError("weight_format=%r conflicts with bc_mode='reference': its error term is the integer "
                             "quantizer's (use 'fused' or 'literal')" % weight_format)
        if clip and bc_mode == "fused":
            raise ValueError("weight_format=%r conflicts with clip under bc_mode='fused': the MX pass has no fused "
                             "clamp" % weight_format)
    assert relu or relu == equalize, "must replace relu6 to relu while equalization"
    assert equalize or absorption == equalize, "must use absorption with equalize"
    t = timings if timings is not None else {}
    timed = timings is not None   # per-stage times need a device sync around each stage

    def stage(name, fn, *a, **k):
        if timed:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(*a, **k)
        if timed:
            torch.cuda.synchronize()
            t[name] = time.perf_counter() - t0
        if stage_hook:
            stage_hook(name)
        return out

    stage("bn1", merge_batchnorm, model, graph, bottoms, targ)
    res = []
    if equalize:
        res = stage("relations", create_relation, graph, bottoms, targ, delete_single=False)
        # launched: the next stages' host work overlaps the device loop (their kernels
        # are ordered behind it on the current stream); wait() below joins it
        stage("cle", cle.cross_layer_equalization, graph, res, targ, Save_state=False, Treshhold=2e-7, launch=True)
    if absorption:
        stage("absorb", bias_absorption, graph, res, bottoms, N=3)
    state = {} if (correction and bc_mode == "fused") else None
    qstate = state
    if mx_scale_search and report is not None and qstate is None:
        qstate = {}   # the report counts the raised scales: keep the scale bytes
    snap = searched = None
    cs_cfg = {}
    if clip_search is not None and not quantize:
        raise ValueError("clip_search needs quantize")
    if quantize:
        set_layer_bits(graph, bits_weight, bits_activation, bits_bias, targ)
        # the second fold hands the folded weights' ranges to the quantize sweep
        fold_ranges = {} if (granularity == "tensor" and not mx_fmt) else None
        stage("bn2", merge_batchnorm, model, graph, bottoms, targ, ranges=fold_ranges)
        fused_clip = tuple(clip_range) if (clip and bc_mode == "fused") else None
        if report is not None:
            snap = quality.snapshot(graph, targ)
        if clip_search is not None:
            cs_cfg = {"clip_search": True, "clip_candidates": int(clip_search.get("candidates", 16)),
                      "clip_min_frac": float(clip_search.get("min_frac", 0.5))}
            # rewrites fold_ranges with the clamped weights' ranges: the sweep stays one pass
            searched = stage("clipsearch", search_clip, graph, bits_weight, granularity=granularity,
                             symmetric=symmetric, candidates=cs_cfg["clip_candidates"],
                             min_frac=cs_cfg["clip_min_frac"], targ_type=targ, weight_ranges=fold_ranges)
        stage("quant", quantize_targ_layer, graph, bits_weight, bits_bias, targ, granularity=granularity,
              symmetric=symmetric, clip=fused_clip, state=qstate, weight_ranges=fold_ranges,
              **({"weight_format": weight_format} if mx_fmt else {}),
              **({"mx_scale_search": True} if mx_scale_search else {}))
    if clip and not (quantize and bc_mode == "fused"):
        stage("clip", clip_weight, graph, range_clip=list(clip_range), targ_type=targ)
    if snap is not None:   # the weights are final from here (bias correction rewrites biases only)
        report.update(quality.weight_report(graph, snap, config={
            "bits_weight": bits_weight, "granularity": granularity, "symmetric": bool(symmetric),
            "equalize": bool(equalize), "absorption": bool(absorption), "clip": bool(clip),
            "clip_range": [float(c) for c in clip_range], "bc_mode": bc_mode, **cs_cfg,
            **({"weight_format": weight_format, "bits_per_weight": bits_per_weight(weight_format)} if mx_fmt else {}),
            **({"mx_scale_search": True} if mx_scale_search else {})},
            clip_search=searched,
            **({"mx_scales": {k: v["scales"] for k, v in qstate.items()}} if mx_scale_search else {})))
    if correction:
        err = None
        if bc_mode == "fused":
            err = {k: esum_source(v) for k, v in (state or {}).items()}
        stage("bc", bias_correction, graph, bottoms, targ, bits_weight=bits_weight, signed=symmetric,
              error_sums=err)
    cle.wait()   # a launched CLE loop's error surfaces here (its results are already ordered on the stream)
    return res
