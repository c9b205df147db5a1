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
  python scripts/mx_gemm_time.py --ab OTHER.so   # dfq_mx_gemm and dfq_mx_linear of another build of the library
                                          #   (the parent commit's) against this tree's, alternated three
                                          #   times in this process -> profiles/r14/mx_mm_parent_ab.jsonl
"""
import argparse
import ctypes as C
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


def parent_ab(args):
    """dfq_mx_gemm and dfq_mx_linear through two builds of the library in one process: --ab's
    (the parent commit's, built into a scratch directory) and this tree's, alternated three
    times on the same descriptors, so the same buffers.  dfq_mx_linear is timed on both of its
    paths: x 16-B aligned (16-B loads) and the same x one float further (4-B loads).  The bound
    of a (shape, pair, call) is the parent's own spread: the new median may exceed the parent's
    median by no more than the parent's slowest leg exceeds its fastest.  The two builds' outputs
    are compared for equality in every cell."""
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    _lib.preload()
    stream = torch.cuda.current_stream(dev)
    s = C.c_void_p(stream.cuda_stream)
    mine, other = _lib.load(), C.CDLL(str(Path(args.ab).resolve()))
    for name in ("dfq_mx_gemm", "dfq_mx_linear"):   # typed here: another commit's build need not export all this tree's binding asks for
        getattr(other, name).argtypes, getattr(other, name).restype = getattr(mine, name).argtypes, getattr(mine, name).restype
    libs = {"parent": other, "new": mine}
    g = torch.Generator().manual_seed(0)
    records = []
    for name, M, N, K in SHAPES:
        xbuf = torch.zeros(M * K + 4, device=dev)
        xs = {"linear_16B": xbuf[:M * K].view(M, K), "linear_4B": xbuf[1:M * K + 1].view(M, K)}
        for x in xs.values():
            x.copy_(torch.randn(M, K, generator=g))
        assert xs["linear_16B"].data_ptr() % 16 == 0 and xs["linear_4B"].data_ptr() % 16 == 4
        w = (torch.randn(N, K, generator=g) * 0.05).to(dev)
        bias = torch.randn(N, generator=g).to(dev)
        out = torch.empty(M, N, device=dev)
        for a_fmt, w_fmt in PAIRS:
            xi, wi = mx.mx_quantize([mx.allocate(xs["linear_16B"], a_fmt, want_dst=False), mx.allocate(w, w_fmt, want_dst=False)])
            dg = _lib.MxGemmDesc()
            dg.a_codes, dg.a_scales, dg.b_codes, dg.b_scales = (t.data_ptr() for t in (xi.codes, xi.scales, wi.codes, wi.scales))
            dg.bias, dg.out, dg.ldo, dg.M, dg.N, dg.K = bias.data_ptr(), out.data_ptr(), N, M, N, K
            dg.a_format, dg.b_format = mx.FORMATS[a_fmt][0], mx.FORMATS[w_fmt][0]
            calls = {"gemm": ("dfq_mx_gemm", dg)}
            for kind, x in xs.items():
                dl = _lib.MxLinearDesc()
                dl.x, dl.b_codes, dl.b_scales, dl.bias, dl.out = (t.data_ptr() for t in (x, wi.codes, wi.scales, bias, out))
                dl.ldx, dl.ldo, dl.M, dl.N, dl.K = K, N, M, N, K
                dl.x_format, dl.b_format = mx.FORMATS[a_fmt][0], mx.FORMATS[w_fmt][0]
                calls[kind] = ("dfq_mx_linear", dl)

            def run(who, kind):
                entry, d = calls[kind]
                _lib.check(getattr(libs[who], entry)(C.byref(d), s), entry)

            legs = []
            for _ in range(3):
                leg = {}
                for kind in calls:
                    for who in ("parent", "new"):
                        leg["%s_%s_ms" % (who, kind)] = round(timed(lambda: run(who, kind), stream, args.warmup, args.steps), 5)
                legs.append(leg)
            rec = {"what": "dfq_mx_gemm / dfq_mx_linear: the parent commit's library against this tree's, alternated in one "
                           "process on the same buffers", "shape": name, "M": M, "N": N, "K": K, "act_format": a_fmt,
                   "weight_format": w_fmt, "device": torch.cuda.get_device_name(dev), "warmup": args.warmup,
                   "steps": args.steps, "legs": legs}
            for kind in calls:
                run("parent", kind)
                want = out.clone()
                run("new", kind)
                assert torch.equal(out.view(torch.int32), want.view(torch.int32)), (name, a_fmt, w_fmt, kind)
                old = [leg["parent_%s_ms" % kind] for leg in legs]
                new = [leg["new_%s_ms" % kind] for leg in legs]
                rec[kind] = {"parent_ms": old, "new_ms": new, "parent_median": statistics.median(old),
                             "new_median": statistics.median(new), "parent_spread": round(max(old) - min(old), 5),
                             "new_within_parent_spread": statistics.median(new) <= statistics.median(old) + (max(old) - min(old))}
            records.append(rec)
    torch.cuda.synchronize()
    emit(records, Path(args.out) if args.out else OUT.parent / "r14" / "mx_mm_parent_ab.jsonl")


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
    ap.add_argument("--ab", default=None, help="another build of libdfq_hip.so to time dfq_mx_gemm / dfq_mx_linear against")
    ap.add_argument("--out", default=None, help="the JSON lines' file (default: under profiles/r11, --ab: profiles/r14)")
    a = ap.parse_args()
    sqnr(a) if a.sqnr else parent_ab(a) if a.ab else timing(a)
