"""Time dfq_int_conv2d (intmm.int_conv2d: the im2col rows gathered and quantized inside the
integer multiply's kernel, padding as the real value 0, the result stored NCHW) beside the only
integer route the entry points offered before it, beside F.conv2d and beside the MX convolution.

Shapes at batch 32, the five layers of README's MX convolution table: MobileNetV2's
[320 -> 1280, 7 x 7] and [16 -> 96, 112 x 112] pointwise layers and its stem [3 -> 32, 3 x 3 s2
p1, 224^2]; ResNet-50's [64 -> 64, 3 x 3 p1, 56^2] and its stem [3 -> 64, 7 x 7 s2 p3, 224^2].
8-bit asymmetric activations on a device range, per-tensor 8-bit weight codes (the forward
scope's).  Per shape the legs are alternated three times in this process, each timed call inside
a HIP event pair, median of --steps calls after --warmup, weight codes cached:
  conv      int_conv2d: one launch on the NCHW input
  before    1 x 1: strided slice, permute to channels last, int_linear, permute back
            (utils.quantize._int_conv1x1); k x k: F.unfold, int_linear, reshape and permute back --
            which computes the OTHER padding rule (a padding tap as the code of 0.0), so its bits
            differ from conv's wherever the geometry has padding
  f_conv2d  F.conv2d(x, w_dequantized): the fp32 product the forward runs outside the scope
  mx_conv   mx.mx_conv2d_fused, MXFP8 activations on MXFP4 weights
Every record also says whether `conv` and `before` gave the same bits.  Data, not assertions.

  python scripts/int_conv_time.py          # -> profiles/r18/int_conv_time.jsonl
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

OUT = Path(__file__).resolve().parent.parent / "profiles" / "r18"
BATCH = 32
#: (name, C, H, W, N, kernel, stride, padding)
SHAPES = [("mobilenetv2_pw_320_1280_7", 320, 7, 7, 1280, 1, 1, 0),
          ("mobilenetv2_pw_16_96_112", 16, 112, 112, 96, 1, 1, 0),
          ("mobilenetv2_stem_3x3_s2", 3, 224, 224, 32, 3, 2, 1),
          ("resnet50_3x3_64_64_56", 64, 56, 56, 64, 3, 1, 1),
          ("resnet50_stem_7x7_s2", 3, 224, 224, 64, 7, 2, 3)]


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
    for name, Cin, H, W, N, k, s, p in SHAPES:
        x = (torch.randn(BATCH, Cin, H, W, generator=g) * 1.2 + 0.4).to(dev)
        w = (torch.randn(N, Cin, k, k, generator=g) * 0.05).to(dev)
        bias = torch.randn(N, generator=g).to(dev)
        K = Cin * k * k
        OH, OW = mx.conv_out_size(H, k, s, p, 1), mx.conv_out_size(W, k, s, p, 1)
        mn, mxv = torch.tensor([-1.3], device=dev), torch.tensor([2.5], device=dev)
        wr = fake_quant(w.reshape(N, K).contiguous(), 8)
        wq = (wr.codes, wr.scale, wr.zero)
        wdq = wr.dq.view(N, Cin, k, k)
        wi = mx.mx_quantize([mx.allocate(w, "mxfp4")])[0]
        out, out_mx = torch.empty(BATCH, N, OH, OW, device=dev), torch.empty(BATCH, N, OH, OW, device=dev)
        rng = dict(min_dev=mn, max_dev=mxv, bias=bias)

        def before():
            if k == 1:
                xs = x[:, :, ::s, ::s]
                n, c, h, ww = xs.shape
                x2d = xs.permute(0, 2, 3, 1).contiguous().view(n * h * ww, c)
                y = intmm.int_linear(x2d, *wq, K, **rng)
                return y.view(n, h, ww, -1).permute(0, 3, 1, 2).contiguous()
            x2d = F.unfold(x, k, 1, p, s).transpose(1, 2).reshape(BATCH * OH * OW, K)
            y = intmm.int_linear(x2d, *wq, K, **rng)
            return y.view(BATCH, OH, OW, N).permute(0, 3, 1, 2).contiguous()

        runs = {"conv": lambda: intmm.int_conv2d(x, *wq, k, s, p, 1, out=out, **rng),
                "before": before,
                "f_conv2d": lambda: F.conv2d(x, wdq, bias, s, p),
                "mx_conv": lambda: mx.mx_conv2d_fused(x, wi.codes, wi.scales, "mxfp4", k, s, p, 1, act_format="mxfp8", bias=bias, out=out_mx)}
        same = bool(torch.equal(runs["conv"]().view(torch.int32), before().view(torch.int32)))
        rec = {"what": "int_conv2d / the integer path before (weight codes given) / F.conv2d / mx_conv2d_fused FP8xFP4", "shape": name,
               "batch": BATCH, "C": Cin, "H": H, "W": W, "N": N, "kernel": k, "stride": s, "padding": p, "M": BATCH * OH * OW, "K": K,
               "bits": 8, "device": torch.cuda.get_device_name(dev), "warmup": args.warmup, "steps": args.steps,
               "conv_equals_before_bitwise": same, "before_pads_with_the_code_of_zero": p != 0}
        legs = [{n + "_ms": round(timed(r, stream, args.warmup, args.steps), 5) for n, r in runs.items()} for _ in range(3)]
        ms = {n: statistics.median(leg[n + "_ms"] for leg in legs) for n in runs}
        rec.update(legs=legs, **{n + "_ms": v for n, v in ms.items()},
                   conv_over_before=round(ms["conv"] / ms["before"], 4), conv_over_f_conv2d=round(ms["conv"] / ms["f_conv2d"], 4),
                   conv_over_mx_conv=round(ms["conv"] / ms["mx_conv"], 4))
        records.append(rec)
        print(json.dumps(rec), flush=True)
    torch.cuda.synchronize()
    path = Path(args.out) if args.out else OUT / "int_conv_time.jsonl"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(json.dumps(r) for r in records) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None, help="the JSON lines' file (default: under profiles/r18)")
    main(ap.parse_args())
