"""Time dfq_mx_gemm (mx.mx_gemm) and mx.mx_linear beside what the Quant* layers' forward
does today, F.linear on the dequantized fp32 weight.

Shapes (M, N, K): MobileNetV2's classifier at batch 32, [32, 1280] x [1000, 1280]; its
largest pointwise layer (320 -> 1280 at 7 x 7) at batch 32, [1568, 320] x [1280, 320]; and
4096^3.  Per shape and (activation, weight) format pair three legs are alternated three
times in this process, each timed call inside a HIP event pair, median of --steps calls
after --warmup:
  gemm     mx_gemm alone on codes quantized beforehand (one launch)
  linear   mx_linear: mx_quantize of the fp32 input and weight (codes and scales only),
           then mx_gemm -- what a layer pays inside mx_matmul_forward() without a cache
  f_linear F.linear(x, w_dequantized): the fp32 product the forward runs outside the scope
TFLOP/s counts 2 M N K.  The fraction of the 8 TB/s HBM peak counts the gemm's algorithmic
bytes (both operands' codes and scale bytes once, the fp32 output once) and is given for
every shape; it means something where the shape is memory-bound (the first two).
--sqnr instead records the SQNR of the zoo MobileNetV2's logits under mx_matmul_forward
against the plain forward, for every activation format.  Data, not assertions.

  python scripts/mx_gemm_time.py          # -> profiles/r11/mx_gemm_time.jsonl
  python scripts/mx_gemm_time.py --sqnr   # -> profiles/r11/mx_forward_sqnr.jsonl
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench  # noqa: E402
from data_free_quantization_amd import _lib, mx  # noqa: E402

OUT = Path(__file__).resolve().parent.parent / "profiles" / "r11"
SHAPES = [("classifier_b32", 32, 1000, 1280), ("pointwise_320_1280_b32", 32 * 49, 1280, 320), ("4096^3", 4096, 4096, 4096)]
PAIRS = [("mxfp8", "mxfp4"), ("mxfp8", "mxfp8"), ("mxfp4", "mxfp4"), ("mxfp6_e2m3", "mxfp6_e3m2")]   # (activation, weight)


def emit(records, path):
    lines = [json.dumps(r) for r in records]
    print("\n".join(lines))
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(lines) + "\n")


def timed(run, stream, warmup, steps):
    for _ in range(warmup):
        run()
    return statistics.median(bench.steps_with_events(run, stream, steps))


def timing(args):
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    _lib.preload()
    stream = torch.cuda.current_stream(dev)
    g = torch.Generator().manual_seed(0)
    records = []
    for name, M, N, K in SHAPES:
        x = torch.randn(M, K, generator=g).to(dev)
        w = (torch.randn(N, K, generator=g) * 0.05).to(dev)
        bias = torch.randn(N, generator=g).to(dev)
        for a_fmt, w_fmt in PAIRS:
            xi, wi = mx.mx_quantize([mx.allocate(x, a_fmt), mx.allocate(w, w_fmt)])
            out = torch.empty(M, N, device=dev)
            runs = {"gemm": lambda: mx.mx_gemm(xi.codes, xi.scales, a_fmt, wi.codes, wi.scales, w_fmt, K, bias=bias, out=out),
                    "linear": lambda: mx.mx_linear(x, wi.dst, bias, w_fmt, a_fmt),
                    "f_linear": lambda: F.linear(x, wi.dst, bias)}
            legs = [{k + "_ms": round(timed(r, stream, args.warmup, args.steps), 5) for k, r in runs.items()}
                    for _ in range(3)]
            ms = {k: statistics.median(leg[k + "_ms"] for leg in legs) for k in runs}
            nbytes = xi.codes.numel() + xi.scales.numel() + wi.codes.numel() + wi.scales.numel() + 4 * M * N
            records.append({"what": "mx_gemm / mx_linear / F.linear on the dequantized weight", "shape": name, "M": M, "N": N,
                            "K": K, "act_format": a_fmt, "weight_format": w_fmt, "device": torch.cuda.get_device_name(dev),
                            "warmup": args.warmup, "steps": args.steps, "legs": legs,
                            **{k + "_ms": v for k, v in ms.items()},
                            **{k + "_tflops": round(2.0 * M * N * K / v / 1e9, 3) for k, v in ms.items()},
                            "gemm_algo_bytes": nbytes,
                            "gemm_frac_of_hbm_peak": round(nbytes / ms["gemm"] / 1e6 / bench.HBM_PEAK_GBS, 5)})
    torch.cuda.synchronize()
    emit(records, Path(args.out) if args.out else OUT / "mx_gemm_time.jsonl")


def sqnr(args):
    from data_free_quantization_amd import pipeline, zoo
    from data_free_quantization_amd.utils import layer_transform as L
    from data_free_quantization_amd.utils.quantize import QuantConv2d, QuantLinear, mx_matmul_forward
    from data_free_quantization_amd.utils.tracer import TorchTransformer
    records = []
    for w_fmt in mx.FORMATS:
        model = zoo.build("mobilenetv2", seed=0, relu=True).cuda().eval()
        x = torch.randn(4, 3, 224, 224, generator=torch.Generator().manual_seed(0)).cuda()
        tr = TorchTransformer("positional")
        model, tr = L.switch_layers(model, tr, x, {1: [(nn.Conv2d, QuantConv2d), (nn.Linear, QuantLinear)]})
        graph, bottoms = tr.log.getGraph(), tr.log.getBottoms()
        pipeline.run_dfq(model, graph, bottoms, (QuantConv2d, QuantLinear), weight_format=w_fmt, bc_mode="fused", clip=False)
        L.set_quant_minmax(graph, bottoms, verbose=False)
        model.eval()
        for m in graph.values():
            if hasattr(m, "quant"):
                m.quant.update_stat = False
        for q in L.module_tensor_op.quants:
            q.update_stat = False
        L.replace_op()
        try:
            with torch.no_grad():
                plain = model(x).double()
                for a_fmt in mx.FORMATS:
                    with mx_matmul_forward(a_fmt):
                        y = model(x).double()
                        calls = mx.LINEAR_CALLS
                    records.append({"what": "zoo MobileNetV2 logits under mx_matmul_forward against the plain forward",
                                    "weight_format": w_fmt, "act_format": a_fmt, "batch": 4, "resolution": 224,
                                    "layers_routed": calls, "finite": bool(torch.isfinite(y).all()),
                                    "logits_sqnr_db": round(10 * np.log10(float(plain.pow(2).sum() / (y - plain).pow(2).sum())), 3),
                                    "top1_agree": int((y.argmax(1) == plain.argmax(1)).sum())})
        finally:
            L.restore_op()
            L.module_tensor_op = None
    emit(records, Path(args.out) if args.out else OUT / "mx_forward_sqnr.jsonl")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sqnr", action="store_true")
    ap.add_argument("--out", default=None, help="the JSON lines' file (default: under profiles/r11)")
    a = ap.parse_args()
    sqnr(a) if a.sqnr else timing(a)
