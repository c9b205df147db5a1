"""Time dfq_mx_linear (mx.mx_linear_fused: the activation quantized inside the multiply's
kernel) beside the path it replaces and beside F.linear.

Shapes and format pairs are scripts/mx_gemm_time.py's: MobileNetV2's classifier at batch 32,
[32, 1280] x [1000, 1280]; its largest pointwise layer at batch 32, [1568, 320] x [1280, 320];
and 4096^3, where the fused kernel re-quantizes every A fragment once per 32 output columns and
the unfused path is expected to win.  Per shape and (activation, weight) pair four legs are
alternated three times in this process, each timed call inside a HIP event pair, median of
--steps calls after --warmup:
  gemm     mx_gemm alone on codes quantized beforehand (one launch): the multiply's floor
  linear   mx_linear with weight_mx given: mx_quantize of the fp32 input, then mx_gemm -- what a
           layer pays inside frozen_weights() today
  fused    mx_linear(fused=True) with weight_mx given: one dfq_mx_linear launch
  f_linear F.linear(x, w_dequantized): the fp32 product the forward runs outside the scope
Every record also says whether `fused` and `linear` gave the same bits.  Data, not assertions.

  python scripts/mx_linear_fused_time.py          # -> profiles/r13/mx_linear_fused_time.jsonl
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
from data_free_quantization_amd import _lib, mx  # noqa: E402
from scripts.mx_gemm_time import PAIRS, SHAPES  # noqa: E402

OUT = Path(__file__).resolve().parent.parent / "profiles" / "r13"


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
        x = torch.randn(M, K, generator=g).to(dev)
        w = (torch.randn(N, K, generator=g) * 0.05).to(dev)
        bias = torch.randn(N, generator=g).to(dev)
        for a_fmt, w_fmt in PAIRS:
            xi, wi = mx.mx_quantize([mx.allocate(x, a_fmt), mx.allocate(w, w_fmt)])
            wmx = (wi.codes, wi.scales)
            out = torch.empty(M, N, device=dev)
            runs = {"gemm": lambda: mx.mx_gemm(xi.codes, xi.scales, a_fmt, wi.codes, wi.scales, w_fmt, K, bias=bias, out=out),
                    "linear": lambda: mx.mx_linear(x, wi.dst, bias, w_fmt, a_fmt, weight_mx=wmx),
                    "fused": lambda: mx.mx_linear(x, wi.dst, bias, w_fmt, a_fmt, weight_mx=wmx, fused=True),
                    "f_linear": lambda: F.linear(x, wi.dst, bias)}
            same = bool(torch.equal(runs["linear"]().view(torch.int32), runs["fused"]().view(torch.int32)))
            legs = [{k + "_ms": round(timed(r, stream, args.warmup, args.steps), 5) for k, r in runs.items()}
                    for _ in range(3)]
            ms = {k: statistics.median(leg[k + "_ms"] for leg in legs) for k in runs}
            records.append({"what": "mx_gemm / mx_linear (weight codes given) / fused mx_linear / F.linear", "shape": name, "M": M,
                            "N": N, "K": K, "act_format": a_fmt, "weight_format": w_fmt,
                            "device": torch.cuda.get_device_name(dev), "warmup": args.warmup, "steps": args.steps,
                            "fused_equals_linear_bitwise": same, "legs": legs, **{k + "_ms": v for k, v in ms.items()},
                            "fused_over_linear": round(ms["fused"] / ms["linear"], 4),
                            "fused_over_gemm": round(ms["fused"] / ms["gemm"], 4),
                            "fused_over_f_linear": round(ms["fused"] / ms["f_linear"], 4)})
    torch.cuda.synchronize()
    lines = [json.dumps(r) for r in records]
    print("\n".join(lines))
    path = Path(args.out) if args.out else OUT / "mx_linear_fused_time.jsonl"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None, help="the JSON lines' file (default: under profiles/r13)")
    main(ap.parse_args())
