"""Time the integer matrix multiply (intmm.int_linear: the input quantized inside the kernel;
intmm.int_gemm: both operands stored codes) beside the fp32 product and the MX multiply.

Shapes [M, K] x [N, K]: MobileNetV2's classifier at batch 32 ([32, 1280] x [1000, 1280]), its
last pointwise layer at batch 32 ([1568, 320] x [1280, 320]) and 4096^3.  8-bit per-tensor
asymmetric codes for both operands, as int_matmul_forward uses them.  Per shape the four legs
are alternated three times in this process, each timed call inside a HIP event pair, median of
--steps calls after --warmup:
  int_linear       intmm.int_linear on fp32 x and stored weight codes: one launch
  int_gemm         intmm.int_gemm on stored codes of both (the quantizer's launch not counted)
  f_linear         F.linear(x^, w^, b) on the dequantized fp32 tensors: what the forward runs
                   outside the scope
  mx_linear_fused  mx.mx_linear_fused, MXFP8 activations x MXFP4 weight codes: one launch
Every record also says whether int_linear and quantize-then-int_gemm gave the same bits.
Data, not assertions.

  python scripts/int_gemm_time.py          # -> profiles/r17/int_gemm_time.jsonl
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench  # noqa: E402
from data_free_quantization_amd import _lib, intmm, mx  # noqa: E402
from data_free_quantization_amd.utils.quantize import fake_quant  # noqa: E402

OUT = Path(__file__).resolve().parent.parent / "profiles" / "r17"
#: (name, M, N, K)
SHAPES = [("mobilenetv2_classifier_b32", 32, 1000, 1280), ("mobilenetv2_pw_320_1280_7_b32", 1568, 1280, 320),
          ("square_4096", 4096, 4096, 4096)]


def timed(run, stream, warmup, steps):
    for _ in range(warmup):
        run()
    return statistics.median(bench.steps_with_events(run, stream, steps))


def main(args):
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    _lib.preload()
    stream = torch.cuda.current_stream(dev)
    g = torch.Generator().manual_seed(0)
    records = []
    for name, M, N, K in SHAPES:
        x = (torch.randn(M, K, generator=g) * 1.5 + 0.5).to(dev)
        w = (torch.randn(N, K, generator=g) * 0.05).to(dev)
        bias = torch.randn(N, generator=g).to(dev)
        mn, mx_ = -2.0, 4.0
        xr, wr = fake_quant(x, 8, min_value=mn, max_value=mx_), fake_quant(w, 8)
        wi = mx.mx_quantize([mx.allocate(w, "mxfp4", want_dst=False)])[0]
        out = [torch.empty(M, N, device=dev) for _ in range(3)]
        runs = {"int_linear": lambda: intmm.int_linear(x, wr.codes, wr.scale, wr.zero, K, min_value=mn, max_value=mx_, bias=bias,
                                                       out=out[0]),
                "int_gemm": lambda: intmm.int_gemm(xr.codes, xr.scale, xr.zero, wr.codes, wr.scale, wr.zero, K, bias=bias, out=out[1]),
                "f_linear": lambda: F.linear(xr.dq, wr.dq, bias),
                "mx_linear_fused": lambda: mx.mx_linear_fused(x, wi.codes, wi.scales, "mxfp4", K, "mxfp8", bias=bias, out=out[2])}
        same = bool(torch.equal(runs["int_linear"]().view(torch.int32), runs["int_gemm"]().view(torch.int32)))
        legs = [{n + "_ms": round(timed(r, stream, args.warmup, args.steps), 5) for n, r in runs.items()} for _ in range(3)]
        ms = {n: statistics.median(leg[n + "_ms"] for leg in legs) for n in runs}
        rec = {"what": "int_linear / int_gemm / F.linear on fp32 / mx_linear_fused (MXFP8 x MXFP4)", "shape": name, "M": M, "N": N,
               "K": K, "bits": 8, "device": torch.cuda.get_device_name(dev), "warmup": args.warmup, "steps": args.steps,
               "int_linear_equals_int_gemm_bitwise": same, "legs": legs, **{n + "_ms": v for n, v in ms.items()},
               "int_linear_over_f_linear": round(ms["int_linear"] / ms["f_linear"], 4),
               "int_gemm_over_f_linear": round(ms["int_gemm"] / ms["f_linear"], 4),
               "int_linear_over_mx_linear_fused": round(ms["int_linear"] / ms["mx_linear_fused"], 4),
               "int_linear_tera_ops": round(2.0 * M * N * K / (ms["int_linear"] * 1e-3) / 1e12, 3)}
        records.append(rec)
        print(json.dumps(rec), flush=True)
    torch.cuda.synchronize()
    path = Path(args.out) if args.out else OUT / "int_gemm_time.jsonl"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(json.dumps(r) for r in records) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None, help="the JSON lines' file (default: under profiles/r17)")
    main(ap.parse_args())
