"""The reference CLI driver (main_dfq.py:36-267) on the MI355X DFQ path.

Same flags and stage order; the transforms run on the GPU.  Additive flags:
  --model {mobilenetv2,resnet50,deeplab,resnet18}   (default: from --task/--resnet:
                       --resnet = ResNet-18 as in the reference, torchvision layout)
  --weights PATH       state_dict to load (torch.load(weights_only=True)); synthetic
                       random-init weights otherwise (the reference checkpoints are
                       not shipped, .MISSING_LARGE_BLOBS)
  --granularity {tensor,channel}, --symmetric   weight quantizer (reference: tensor, asym)
  --bc_mode {literal,reference,fused}          see pipeline.py (default literal = the
                       reference's effective behaviour)
  --val PATH           ImageNet-val folder (ImageFolder layout) for --task cls evaluation
  --voc PATH           VOCdevkit/VOC2012 for --task seg evaluation (mIoU)
  --batch_size, --workers   evaluation DataLoader (reference: 256 / 4 cls, 32 / 2 seg)
  --world_size N       shard quantize_targ_layer's layer list over N ranks (one
                       process per GPU under torchrun, RCCL all-gather of the
                       results; distributed.py); rank 0 evaluates / logs / exports
  --report PATH        write the data-free quality report (quality.py: per-layer and
                       per-channel SQNR of the quantized weights against their values
                       before quantization, as JSON); needs --quantize
  --clip_search        before quantizing, clamp every weight (per channel or per tensor,
                       as --granularity) to the one of --clip_candidates K ranges between
                       its min-max range and --clip_min_frac of it that minimizes its own
                       quantization noise (clip_weight.search_clip); needs --quantize.
                       The defaults (16, 0.5) are interface choices: no dataset ships
                       here to tune them on.  --report then counts, per layer, the units
                       that chose a narrower range and those at the narrowest candidate
  --weight_format {int,mxfp4,mxfp6_e2m3,mxfp6_e3m2,mxfp8}   int (default): the integer grid
                       of --bits_weight / --granularity / --symmetric.  mxfp4 / mxfp6_e2m3 /
                       mxfp6_e3m2 / mxfp8: OCP MX block-scaled weights (mx.py: FP4 E2M1 / FP6
                       E2M3 / FP6 E3M2 / FP8 E4M3 elements, one power-of-two scale per 32
                       elements of a row; 4.25 / 6.25 / 6.25 / 8.25 bits per weight), to which
                       those three flags do not apply.  There is no bare mxfp6.  Not with --clip_search, --bc_mode reference,
                       --clip_weight under --bc_mode fused, or --world_size > 1
  --mx_scale_search    with an MX --weight_format: every 32-element block takes the better of
                       the OCP floor rule's scale and the next power of two up, by its own
                       quantization noise (mx.mx_quantize(scale_search=True)): a block whose
                       largest elements the floor rule would clamp trades them for a coarser
                       grid where that pays.  --report then counts the raised blocks per layer
                       (scale_raised); --export marks the file ("mx_scale_search": true), its
                       format is unchanged.  --mx_matmul re-quantizes such weights with the search
  --mx_matmul {mxfp4,mxfp6_e2m3,mxfp6_e3m2,mxfp8}   run the evaluation's Linear and 1x1-convolution
                       products on the scaled matrix instruction (utils.quantize.mx_matmul_forward,
                       mx.mx_linear): the stored MX weight codes times the layer's input rounded
                       to this MX format in blocks of 32 along the channel dimension -- a second
                       rounding of the activations, after their integer fake quant.  Needs an MX
                       --weight_format
  --mx_matmul_fused    with --mx_matmul: round each layer's input inside the multiply's kernel
                       (mx.mx_linear_fused, dfq_mx_linear) instead of in a quantizer launch of its
                       own -- the same bits, one library launch per layer once its weight codes
                       are cached.  Needs --mx_matmul
  --mx_matmul_conv     with --mx_matmul: every convolution with groups == 1 and zero padding mode --
                       any kernel size, stride, padding and dilation -- multiplies on the scaled
                       matrix instruction too (mx.mx_conv2d_fused, dfq_mx_conv2d): one launch reads
                       the NCHW input in place, gathers each im2col row, rounds it in blocks of 32
                       along (c, kh, kw) -- the order the weight's own MX blocks run in -- and
                       stores NCHW.  Grouped and depthwise convolutions stay on fp32.  Needs
                       --mx_matmul
  --int_matmul         run the evaluation's Linear and 1x1-convolution products on the i8 matrix
                       instruction (utils.quantize.int_matmul_forward, intmm.int_linear,
                       dfq_int_linear): the layer's per-tensor integer weight codes times its
                       input's activation codes, re-derived inside the kernel from the
                       fake-quantized input and the observer's range -- what an integer
                       deployment of the quantized model computes, integer sums exact, the
                       affine terms in fp64.  k x k, grouped and depthwise convolutions stay on
                       fp32.  Needs --quantize and --weight_format int; not with --mx_matmul
  --int_matmul_conv    with --int_matmul: every convolution with groups == 1 and zero padding mode
                       -- any kernel size, stride, padding and dilation -- multiplies on the i8
                       matrix instruction too (intmm.int_conv2d, dfq_int_conv2d): one launch
                       gathers the im2col rows from the NCHW input, quantizes them and stores
                       NCHW; a padding tap is the real value 0, as in F.conv2d.  Grouped and
                       depthwise convolutions stay on fp32.  Needs --int_matmul
  --int_matmul_depthwise  with --int_matmul_conv: every depthwise convolution (groups ==
                       in_channels, zero padding mode, at most 64 taps) multiplies on the packed
                       8-bit dot instruction (intmm.int_dwconv2d, dfq_int_dwconv2d): one launch
                       quantizes each input element once, keeps the code bytes in LDS and stores
                       NCHW, so every Conv2d / Linear product of MobileNetV2 and DeepLab is an
                       integer one.  Other grouped convolutions stay on fp32.  Needs
                       --int_matmul_conv

Example (README.md:137 of the reference):
  python -m data_free_quantization_amd.main_dfq --task cls --relu --equalize --absorption \
      --quantize --correction --clip_weight --bits_weight 8 --bits_activation 8 --bits_bias 8
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import torch
import torch.nn as nn

from . import _lib, mx, zoo
from .bias_absorption import bias_absorption
from .bias_correction import bias_correction
from .clip_weight import clip_weight, search_clip
from .Cross_layer_equal import cross_layer_equalization, wait as cle_wait
from .utils.layer_transform import (esum_source, merge_batchnorm, quantize_targ_layer, replace_op, restore_op,
                                    set_quant_minmax, switch_layers)
from .utils.quantize import QuantConv2d, QuantLinear, QuantMeasure, set_layer_bits
from .utils.relation import create_relation
from .utils.tracer import TorchTransformer


def get_argument(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--gpu", action="store_true")
    p.add_argument("--sizedisp", action="store_true")
    p.add_argument("--visualize", action="store_true")
    p.add_argument("--quantize", action="store_true")
    p.add_argument("--equalize", action="store_true")
    p.add_argument("--correction", action="store_true")
    p.add_argument("--absorption", action="store_true")
    p.add_argument("--relu", action="store_true")
    p.add_argument("--clip_weight", action="store_true")
    p.add_argument("--task", default="cls", type=str, choices=["cls", "seg"])
    p.add_argument("--resnet", action="store_true")
    p.add_argument("--log", action="store_true")
    p.add_argument("--bits_weight", type=int, default=8)
    p.add_argument("--bits_activation", type=int, default=8)
    p.add_argument("--bits_bias", type=int, default=8)
    # additive
    p.add_argument("--model", default=None, choices=list(zoo.MODELS))
    p.add_argument("--weights", default=None)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--granularity", default="tensor", choices=["tensor", "channel"])
    p.add_argument("--symmetric", action="store_true")
    p.add_argument("--bc_mode", default="literal", choices=["literal", "reference", "fused"])
    p.add_argument("--val", default="./val")
    p.add_argument("--voc", default="./VOCdevkit/VOC2012/")
    p.add_argument("--batch_size", type=int, default=256)
    p.add_argument("--workers", type=int, default=4)
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--export", default=None,
                   help="write the integer weights (codes, scale, zero, bias) to this safetensors file")
    p.add_argument("--world_size", type=int, default=1,
                   help="ranks sharing quantize_targ_layer's layer list (launch with torchrun --nproc-per-node N)")
    p.add_argument("--report", default=None,
                   help="write the weight quantization quality report (per-channel SQNR, JSON) to this file")
    p.add_argument("--clip_search", action="store_true",
                   help="clamp each weight to the candidate range with the least quantization noise before quantizing")
    p.add_argument("--clip_candidates", type=int, default=16, help="candidate ranges per unit (1..64)")
    p.add_argument("--clip_min_frac", type=float, default=0.5,
                   help="the narrowest candidate as a share of the min-max range, in [0, 1]")
    p.add_argument("--weight_format", default="int", choices=["int", "mxfp4", "mxfp6_e2m3", "mxfp6_e3m2", "mxfp8"],
                   help="weight codes: the integer grid, or OCP MX block-scaled FP4 / FP6 / FP8 (32-element blocks)")
    p.add_argument("--mx_matmul", default=None, choices=["mxfp4", "mxfp6_e2m3", "mxfp6_e3m2", "mxfp8"],
                   help="evaluate with the MX layers' products on the scaled matrix instruction, activations "
                        "rounded to this MX format")
    p.add_argument("--mx_matmul_fused", action="store_true",
                   help="with --mx_matmul: quantize each layer's input inside the multiply's kernel (one launch per layer)")
    p.add_argument("--mx_matmul_conv", action="store_true",
                   help="with --mx_matmul: k x k convolutions (groups == 1) multiply on the scaled matrix instruction too, "
                        "their im2col rows gathered and rounded inside the kernel")
    p.add_argument("--int_matmul", action="store_true",
                   help="evaluate with the integer layers' Linear and 1x1-convolution products on the i8 matrix "
                        "instruction, from the weight and activation codes")
    p.add_argument("--int_matmul_conv", action="store_true",
                   help="with --int_matmul: k x k convolutions (groups == 1) multiply on the i8 matrix instruction too, "
                        "their im2col rows gathered and quantized inside the kernel")
    p.add_argument("--int_matmul_depthwise", action="store_true",
                   help="with --int_matmul_conv: depthwise convolutions multiply on the packed 8-bit dot instruction, "
                        "their input quantized once per element inside the kernel")
    p.add_argument("--mx_scale_search", action="store_true",
                   help="MX weights: per block, the better of the floor rule's scale and the next one up by "
                        "the block's own quantization noise")
    args = p.parse_args(argv)
    if args.mx_matmul is not None and args.weight_format == "int":
        p.error("--mx_matmul needs an MX --weight_format")
    if args.mx_matmul_fused and args.mx_matmul is None:
        p.error("--mx_matmul_fused needs --mx_matmul")
    if args.mx_matmul_conv and args.mx_matmul is None:
        p.error("--mx_matmul_conv needs --mx_matmul")
    if args.int_matmul_conv and not args.int_matmul:
        p.error("--int_matmul_conv needs --int_matmul")
    if args.int_matmul_depthwise and not args.int_matmul_conv:
        p.error("--int_matmul_depthwise needs --int_matmul_conv")
    if args.int_matmul and args.mx_matmul is not None:
        p.error("--int_matmul conflicts with --mx_matmul")
    if args.int_matmul and (not args.quantize or args.weight_format != "int"):
        p.error("--int_matmul needs --quantize and --weight_format int")
    if args.mx_scale_search and args.weight_format == "int":
        p.error("--mx_scale_search needs an MX --weight_format")
    if args.weight_format != "int":
        if not args.quantize:
            p.error("--weight_format needs --quantize")
        if args.clip_search:
            p.error("--weight_format %s conflicts with --clip_search (the search minimizes an integer grid's noise; "
                    "--mx_scale_search is the MX formats' search)" % args.weight_format)
        if args.bc_mode == "reference":
            p.error("--weight_format %s conflicts with --bc_mode reference (its error term is the integer "
                    "quantizer's)" % args.weight_format)
        if args.clip_weight and args.bc_mode == "fused":
            p.error("--weight_format %s conflicts with --clip_weight under --bc_mode fused (the MX pass has no fused "
                    "clamp)" % args.weight_format)
        if args.world_size > 1:
            p.error("--weight_format %s is not sharded: run it with --world_size 1" % args.weight_format)
    if args.report and not args.quantize:
        p.error("--report needs --quantize")
    if args.clip_search and not args.quantize:
        p.error("--clip_search needs --quantize")
    if args.clip_search and args.world_size > 1:
        p.error("--clip_search is not sharded: run it with --world_size 1")
    if args.clip_search and not (1 <= args.clip_candidates <= _lib.DFQ_CLIP_MAX_CANDIDATES and
                                 0.0 <= args.clip_min_frac <= 1.0):
        p.error("--clip_candidates takes 1..%d and --clip_min_frac a value in [0, 1]" % _lib.DFQ_CLIP_MAX_CANDIDATES)
    return args


def _model_name(args):
    if args.model:
        return args.model
    if args.task == "seg":
        return "deeplab"
    return "resnet18" if args.resnet else "mobilenetv2"   # main_dfq.py:126-131


def canonical_state_dict(state):
    """A reference checkpoint's state_dict in this package's module names.  The
    reference's DeepLab backbone exposes features[0:4] / features[4:] a second
    time as low_level_features / high_level_features
    (modeling/segmentation/backbone/mobilenet.py:115-116), so its checkpoints hold
    every backbone tensor twice; a slice of an nn.Sequential keeps the original
    child names, so ``low_level_features.N`` / ``high_level_features.N`` map back
    to ``backbone.features.N`` (and must agree with it)."""
    out = {}
    alias = ("backbone.low_level_features.", "backbone.high_level_features.")
    for k, v in state.items():
        for pre in alias:
            if k.startswith(pre):
                canon = "backbone.features." + k[len(pre):]
                if canon in state and not torch.equal(state[canon], v):
                    raise ValueError(f"checkpoint alias {k} disagrees with {canon}")
                out.setdefault(canon, v)
                break
        else:
            out[k] = v
    return out


def build_model(args):
    name = _model_name(args)
    model = zoo.build(name, seed=args.seed)
    if args.weights:
        state = torch.load(args.weights, map_location="cpu", weights_only=True)
        state = state.get("state_dict", state) if isinstance(state, dict) else state
        model.load_state_dict(canonical_state_dict(state))
    return model, name


def inference_all(model, task, args):
    """main_dfq.py:66-113 on the GPU: ImageNet-val top-1 (``--val``, ImageFolder
    layout) for cls, PASCAL VOC 2012 val mIoU (``--voc``) for seg, through the
    torchvision-free harness in evaluate.py.  Returns None (with a message) when
    the dataset is not there -- neither ships with the reference or this image."""
    from . import evaluate
    if task == "cls":
        if not os.path.isdir(args.val):
            print(f"Evaluation skipped: no ImageFolder at {args.val}")
            return None
        print("Start inference")
        acc = evaluate.inference_cls(model, args.val, args.device, batch_size=args.batch_size,
                                     workers=args.workers)
        print(f"Final Accuracy: {acc * 100:.2f}%")
        return acc
    if not os.path.isdir(args.voc):
        print(f"Evaluation skipped: no VOC 2012 tree at {args.voc}")
        return None
    print("Start inference")
    miou = evaluate.inference_seg(model, args.voc, args.device, batch_size=min(args.batch_size, 32),
                                  workers=args.workers)
    print(f"mIoU: {miou * 100:.2f}%")
    return miou


def main(argv=None):
    args = get_argument(argv)
    assert args.relu or args.relu == args.equalize, "must replace relu6 to relu while equalization"
    assert args.equalize or args.absorption == args.equalize, "must use absorption with equalize"
    rank = 0
    if args.world_size > 1:
        from . import distributed as D
        world, rank, dev = D.init_from_env()
        if world != args.world_size:
            raise ValueError(f"--world_size {args.world_size} but WORLD_SIZE={world} (launch with torchrun "
                             f"--nproc-per-node {args.world_size})")
        args.device = str(dev)
    model, name = build_model(args)
    if args.sizedisp:
        print("param size:", sum(p.numel() for p in model.parameters()) * 4 / 2 ** 20, "MB")
    model = model.to(args.device).eval()

    transformer = TorchTransformer(key_mode="positional" if args.bc_mode != "literal" else "opaque")
    module_dict = {}
    if args.quantize:
        module_dict[1] = [(nn.Conv2d, QuantConv2d), (nn.Linear, QuantLinear)]
    if args.relu:
        module_dict[0] = [(torch.nn.ReLU6, torch.nn.ReLU)]
    data = torch.ones(zoo.INPUT_SHAPES[name])
    model, transformer = switch_layers(model, transformer, data, module_dict, ignore_layer=[QuantMeasure],
                                       quant_op=args.quantize)
    model = model.to(args.device)
    graph = transformer.log.getGraph()
    bottoms = transformer.log.getBottoms()
    targ_layer = (QuantConv2d, QuantLinear) if args.quantize else (nn.Conv2d, nn.Linear)
    if str(args.device).startswith("cuda"):
        _lib.preload()   # library + code objects: process setup, outside the timed stages

    t0 = time.perf_counter()
    model = merge_batchnorm(model, graph, bottoms, targ_layer)
    res = []
    if args.equalize:
        res = create_relation(graph, bottoms, targ_layer, delete_single=False)
        cross_layer_equalization(graph, res, targ_layer, Save_state=False, Treshhold=2e-7, launch=True)
    if args.absorption:
        bias_absorption(graph, res, bottoms, N=3, visualize=args.visualize)
    state = {} if (args.bc_mode == "fused" or args.export or (args.report and args.mx_scale_search)) else None
    if args.quantize:
        set_layer_bits(graph, args.bits_weight, args.bits_activation, args.bits_bias, targ_layer)
        sharded = args.world_size > 1
        mx_fmt = args.weight_format != "int"
        fold_ranges = {} if (args.granularity == "tensor" and not sharded and not mx_fmt) else None
        model = merge_batchnorm(model, graph, bottoms, targ_layer, ranges=fold_ranges)
        fused_clip = [-15, 15] if (args.clip_weight and args.bc_mode == "fused") else None
        if args.report:   # the weights the quantizer is about to see (every rank: same stage order)
            from . import quality
            snap = quality.snapshot(graph, targ_layer)
        searched = None
        if args.clip_search:   # rewrites fold_ranges with the clamped weights' ranges (one-pass sweep)
            searched = search_clip(graph, args.bits_weight, granularity=args.granularity, symmetric=args.symmetric,
                                   candidates=args.clip_candidates, min_frac=args.clip_min_frac,
                                   targ_type=targ_layer, weight_ranges=fold_ranges)
        graph = quantize_targ_layer(graph, args.bits_weight, args.bits_bias, targ_layer,
                                    granularity=args.granularity, symmetric=args.symmetric, clip=fused_clip,
                                    state=state, shard=sharded, weight_ranges=fold_ranges,
                                    **({"weight_format": args.weight_format} if mx_fmt else {}),
                                    **({"mx_scale_search": True} if args.mx_scale_search else {}))
        set_quant_minmax(graph, bottoms)   # main_dfq.py:217
    if args.clip_weight and not (args.quantize and args.bc_mode == "fused"):
        clip_weight(graph, range_clip=[-15, 15], targ_type=targ_layer)
    if args.correction:
        # main_dfq.py:231 passes visualize= to a signature without it (TypeError in the
        # reference); this driver calls the documented signature.
        err = {k: esum_source(v) for k, v in state.items()} if (state and args.bc_mode == "fused") else None
        bias_correction(graph, bottoms, targ_layer, bits_weight=args.bits_weight, signed=args.symmetric,
                        error_sums=err)
    cle_wait()   # the launched CLE loop's error, if any, surfaces here
    torch.cuda.synchronize()
    print(f"DFQ weight transforms took {time.perf_counter() - t0:.3f} s on {args.device}")
    if args.export and args.quantize and state and rank == 0:
        from . import export
        clip = [-15, 15] if args.clip_weight else None   # fused in the sweep or clip_weight after it: same clamp
        export.save(args.export, graph, state, bits=args.bits_weight, granularity=args.granularity,
                    symmetric=args.symmetric, clip=clip,
                    **({"weight_format": args.weight_format} if args.weight_format != "int" else {}),
                    **({"mx_scale_search": True} if args.mx_scale_search else {}))
        print(f"Exported {len(state)} quantized layers to {args.export}")
    if args.report and rank == 0:   # sharded runs: every rank holds every result after the gather
        import json
        rep = quality.weight_report(graph, snap, config={
            "model": name, "bits_weight": args.bits_weight, "granularity": args.granularity,
            "symmetric": args.symmetric, "equalize": args.equalize, "absorption": args.absorption,
            "clip": args.clip_weight, "clip_range": [-15.0, 15.0], "bc_mode": args.bc_mode,
            "world_size": args.world_size,
            **({"clip_search": True, "clip_candidates": args.clip_candidates, "clip_min_frac": args.clip_min_frac}
               if args.clip_search else {}),
            **({"weight_format": args.weight_format, "bits_per_weight": mx.bits_per_weight(args.weight_format)}
               if args.weight_format != "int" else {}),
            **({"mx_scale_search": True} if args.mx_scale_search else {})}, clip_search=searched,
            **({"mx_scales": {k: v["scales"] for k, v in state.items()}} if args.mx_scale_search else {}))
        with open(args.report, "w") as f:
            json.dump(rep, f, indent=1, allow_nan=False)
        m = rep["model"]
        worst = next((e for e in rep["layers"] if e["key"] == m["worst_layer"]), None)
        print("Quality report: model SQNR {} dB, worst layer {} ({} dB) -> {}".format(
            "n/a" if m["sqnr_db"] is None else f"{m['sqnr_db']:.2f}", m["worst_layer"],
            "n/a" if worst is None else f"{worst['sqnr_db']:.2f}", args.report))

    # main_dfq.py:237-240: inference in eval mode -- also the observers set_layer_bits
    # created (new modules start in training mode)
    model.eval()
    accuracy = None
    if rank == 0:
        if args.quantize:
            replace_op()
        start = time.time()
        # the weights are final from here: the Quant* layers keep their weight /
        # bias fake-quant between batches (utils.quantize.frozen_weights)
        import contextlib
        from .utils.quantize import frozen_weights, int_matmul_forward, mx_matmul_forward
        scope = (mx_matmul_forward(args.mx_matmul, fused=args.mx_matmul_fused, conv=args.mx_matmul_conv) if args.mx_matmul is not None
                 else int_matmul_forward(conv=args.int_matmul_conv, depthwise=args.int_matmul_depthwise) if args.int_matmul else contextlib.nullcontext())
        with frozen_weights(), scope:
            accuracy = inference_all(model, args.task, args)
        print(f"Inference time is {time.time() - start} seconds")
        if args.quantize:
            restore_op()
    if args.world_size > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    if args.log and rank == 0:
        with open("dfq_result.txt", "a+") as ww:
            ww.write("task: {}, resnet: {}, relu: {}, equalize: {}, absorption: {}, quantize: {}, correction: {}, "
                     "clip: {}, bits_weight: {}, bits_activation: {}, bits_bias: {}\n".format(
                         args.task, args.resnet, args.relu, args.equalize, args.absorption, args.quantize,
                         args.correction, args.clip_weight, args.bits_weight, args.bits_activation, args.bits_bias))
            ww.write("Accuracy: {} %\n\n".format(accuracy * 100 if accuracy is not None else "n/a"))
    return model, graph, accuracy


if __name__ == "__main__":
    main(sys.argv[1:])
