"""Time dfq_int_dwconv2d (intmm.int_dwconv2d: the depthwise convolution on the packed 8-bit dot
instruction, every input element quantized once inside the kernel, the code bytes kept in LDS,
padding as the real value 0, the result stored NCHW) beside the fp32 F.conv2d(groups=C) these
layers ran on before -- there was no integer route for them, so it is the only comparison.

Shapes at batch 32: MobileNetV2's depthwise 3 x 3 layers at 112^2 (C = 32, stride 1), 112^2 -> 56^2
(C = 96, stride 2), 28^2 (C = 192), 14^2 (C = 576) and 7^2 (C = 960), and DeepLab's dilated one
(C = 960, dilation 2, on the 37^2 input its fixed padding makes of 33^2).  8-bit asymmetric
activations on a device range, per-tensor 8-bit weight codes (the forward scope's).  Per shape the
legs are alternated three times in this process, each timed call inside a HIP event pair, median
of --steps calls after --warmup:
  dwconv    int_dwconv2d: one launch on the NCHW input
  f_conv2d  F.conv2d(x, w_dequantized, groups=C): the fp32 product the forward runs outside the scope
`hbm_fraction` is the algorithmic bytes -- x once, out once, the weight codes -- over dwconv's
time, as a fraction of 8 TB/s.  Data, not assertions.

  python scripts/int_dwconv_time.py          # -> profiles/r19/int_dwconv_time.jsonl
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

OUT = Path(__file__).resolve().parent.parent / "profiles" / "r19"
BATCH = 32
HBM_BYTES_PER_S = 8e12
#: (name, C, H, W, stride, padding, dilation), all 3 x 3
SHAPES = [("mobilenetv2_dw_32_112_s1", 32, 112, 112, 1, 1, 1),
          ("mobilenetv2_dw_96_112_s2", 96, 112, 112, 2, 1, 1),
          ("mobilenetv2_dw_192_28_s1", 192, 28, 28, 1, 1, 1),
          ("mobilenetv2_dw_576_14_s1", 576, 14, 14, 1, 1, 1),
          ("mobilenetv2_dw_960_7_s1", 960, 7, 7, 1, 1, 1),
          ("deeplab_dw_960_37_d2", 960, 37, 37, 1, 0, 2)]


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
    for name, Cin, H, W, s, p, d in SHAPES:
        k = 3
        x = (torch.randn(BATCH, Cin, H, W, generator=g) * 1.2 + 0.4).to(dev)
        w = (torch.randn(Cin, 1, k, k, generator=g) * 0.05).to(dev)
        bias = torch.randn(Cin, generator=g).to(dev)
        OH, OW = mx.conv_out_size(H, k, s, p, d), mx.conv_out_size(W, k, s, p, d)
        mn, mxv = torch.tensor([-1.3], device=dev), torch.tensor([2.5], device=dev)
        wr = fake_quant(w.reshape(Cin, k * k).contiguous(), 8)
        wq = (wr.codes, wr.scale, wr.zero)
        wdq = wr.dq.view(Cin, 1, k, k)
        out = torch.empty(BATCH, Cin, OH, OW, device=dev)
        runs = {"dwconv": lambda: intmm.int_dwconv2d(x, *wq, k, s, p, d, min_dev=mn, max_dev=mxv, bias=bias, out=out),
                "f_conv2d": lambda: F.conv2d(x, wdq, bias, s, p, d, groups=Cin)}
        algo_bytes = 4 * x.numel() + 4 * out.numel() + wr.codes.numel()
        rec = {"what": "int_dwconv2d / F.conv2d(groups=C) on the dequantized weight", "shape": name, "batch": BATCH, "C": Cin, "H": H,
               "W": W, "kernel": k, "stride": s, "padding": p, "dilation": d, "OH": OH, "OW": OW, "bits": 8,
               "device": torch.cuda.get_device_name(dev), "warmup": args.warmup, "steps": args.steps, "algo_bytes": algo_bytes}
        legs = [{n + "_ms": round(timed(r, stream, args.warmup, args.steps), 5) for n, r in runs.items()} for _ in range(3)]
        ms = {n: statistics.median(leg[n + "_ms"] for leg in legs) for n in runs}
        rec.update(legs=legs, **{n + "_ms": v for n, v in ms.items()},
                   dwconv_over_f_conv2d=round(ms["dwconv"] / ms["f_conv2d"], 4),
                   hbm_fraction=round(algo_bytes / (ms["dwconv"] * 1e-3) / HBM_BYTES_PER_S, 4),
                   f_conv2d_hbm_fraction=round(algo_bytes / (ms["f_conv2d"] * 1e-3) / HBM_BYTES_PER_S, 4))
        records.append(rec)
        print(json.dumps(rec), flush=True)
    torch.cuda.synchronize()
    path = Path(args.out) if args.out else OUT / "int_dwconv_time.jsonl"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(json.dumps(r) for r in records) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None, help="the JSON lines' file (default: under profiles/r19)")
    main(ap.parse_args())
