"""Time dfq_mx_conv2d (mx.mx_conv2d_fused: the im2col rows gathered and quantized inside the
multiply's kernel, the result stored NCHW) beside what the layer paid before and beside F.conv2d.

Shapes at batch 32: MobileNetV2's [320 -> 1280, 7 x 7] and [16 -> 96, 112 x 112] pointwise layers
and its stem [3 -> 32, 3 x 3 s2 p1, 224^2]; ResNet-50's [64 -> 64, 3 x 3 p1, 56^2] and its stem
[3 -> 64, 7 x 7 s2 p3, 224^2].  Formats: MXFP8 and MXFP4 activations on MXFP4 weights.  Per shape
and pair the legs are alternated three times in this process, each timed call inside a HIP event
pair, median of --steps calls after --warmup:
  conv      mx_conv2d_fused on cached weight codes: one launch on the NCHW input
  before    what the layer did before, on cached weight codes -- 1 x 1: strided slice, permute to
            channels last, mx_linear(fused=True), permute back (utils.quantize._mx_conv1x1);
            k x k: F.unfold, mx_linear_fused, reshape and permute back, the only MX route there was
  f_conv2d  F.conv2d(x, w_dequantized): the fp32 product the forward runs outside the scope
  general   pointwise shapes only: the diagnostics library's dfq_mx_conv2d with the pointwise
            variant switched off (DFQ_MX_CONV_GENERAL), the A/B of that variant
Every record also says whether `conv` and `before` gave the same bits.  Data, not assertions.

  python scripts/mx_conv_time.py          # -> profiles/r14/mx_conv_time.jsonl
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench  # noqa: E402
from data_free_quantization_amd import _lib, mx  # noqa: E402

OUT = Path(__file__).resolve().parent.parent / "profiles" / "r14"
BATCH = 32
#: (name, C, H, W, N, kernel, stride, padding)
SHAPES = [("mobilenetv2_pw_320_1280_7", 320, 7, 7, 1280, 1, 1, 0),
          ("mobilenetv2_pw_16_96_112", 16, 112, 112, 96, 1, 1, 0),
          ("mobilenetv2_stem_3x3_s2", 3, 224, 224, 32, 3, 2, 1),
          ("resnet50_3x3_64_64_56", 64, 56, 56, 64, 3, 1, 1),
          ("resnet50_stem_7x7_s2", 3, 224, 224, 64, 7, 2, 3)]
PAIRS = [("mxfp8", "mxfp4"), ("mxfp4", "mxfp4")]


def timed(run, stream, warmup, steps):
    for _ in range(warmup):
        run()
    return statistics.median(bench.steps_with_events(run, stream, steps))


def general_call(x, codes, scales, w_fmt, k, s, p, a_fmt, bias, out):
    """dfq_mx_conv2d of the diagnostics library (the general gather where the environment says so)."""
    L = _lib.load_diag()
    d = _lib.MxConv2dDesc()
    d.x, d.b_codes, d.b_scales, d.bias, d.out = x.data_ptr(), codes.data_ptr(), scales.data_ptr(), bias.data_ptr(), out.data_ptr()
    d.B, d.C, d.H, d.W = x.shape
    d.N, d.KH, d.KW = out.shape[1], k, k
    d.stride_h = d.stride_w = s
    d.pad_h = d.pad_w = p
    d.dil_h = d.dil_w = 1
    d.x_format, d.b_format = mx.FORMATS[a_fmt][0], mx.FORMATS[w_fmt][0]
    ref = C.byref(d)
    return lambda: _lib.check(L.dfq_mx_conv2d(ref, _lib.raw_stream(x.device)), "dfq_mx_conv2d (diagnostics)")


def main(args):
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    _lib.preload()
    os.environ["DFQ_MX_CONV_GENERAL"] = "1"   # read by the diagnostics library only
    stream = torch.cuda.current_stream(dev)
    g = torch.Generator().manual_seed(0)
    records = []
    for name, Cin, H, W, N, k, s, p in SHAPES:
        x = torch.randn(BATCH, Cin, H, W, generator=g).to(dev)
        w = (torch.randn(N, Cin, k, k, generator=g) * 0.05).to(dev)
        bias = torch.randn(N, generator=g).to(dev)
        K = Cin * k * k
        OH, OW = mx.conv_out_size(H, k, s, p, 1), mx.conv_out_size(W, k, s, p, 1)
        for a_fmt, w_fmt in PAIRS:
            wi = mx.mx_quantize([mx.allocate(w, w_fmt)])[0]
            wmx = (wi.codes, wi.scales)
            w2d = wi.dst.reshape(N, K)
            out = torch.empty(BATCH, N, OH, OW, device=dev)

            def before():
                if k == 1:
                    xs = x[:, :, ::s, ::s]
                    n, c, h, ww = xs.shape
                    x2d = xs.permute(0, 2, 3, 1).contiguous().view(n * h * ww, c)
                    y = mx.mx_linear(x2d, w2d, bias, w_fmt, a_fmt, weight_mx=wmx, fused=True)
                    return y.view(n, h, ww, -1).permute(0, 3, 1, 2).contiguous()
                x2d = F.unfold(x, k, 1, p, s).transpose(1, 2).reshape(BATCH * OH * OW, K)
                y = mx.mx_linear_fused(x2d, wmx[0], wmx[1], w_fmt, K, a_fmt, bias=bias)
                return y.view(BATCH, OH, OW, N).permute(0, 3, 1, 2).contiguous()

            runs = {"conv": lambda: mx.mx_conv2d_fused(x, wmx[0], wmx[1], w_fmt, k, s, p, 1, act_format=a_fmt, bias=bias, out=out),
                    "before": before,
                    "f_conv2d": lambda: F.conv2d(x, wi.dst, bias, s, p)}
            same = bool(torch.equal(runs["conv"]().view(torch.int32), before().view(torch.int32)))
            rec = {"what": "mx_conv2d_fused / the path before (weight codes given) / F.conv2d", "shape": name, "batch": BATCH,
                   "C": Cin, "H": H, "W": W, "N": N, "kernel": k, "stride": s, "padding": p, "M": BATCH * OH * OW, "K": K,
                   "act_format": a_fmt, "weight_format": w_fmt, "device": torch.cuda.get_device_name(dev),
                   "warmup": args.warmup, "steps": args.steps, "conv_equals_before_bitwise": same}
            if k == 1 and p == 0:
                out2 = torch.empty_like(out)
                runs["general"] = general_call(x, wmx[0], wmx[1], w_fmt, k, s, p, a_fmt, bias, out2)
                runs["general"]()
                rec["general_equals_conv_bitwise"] = bool(torch.equal(out2.view(torch.int32), out.view(torch.int32)))
            legs = [{n + "_ms": round(timed(r, stream, args.warmup, args.steps), 5) for n, r in runs.items()} for _ in range(3)]
            ms = {n: statistics.median(leg[n + "_ms"] for leg in legs) for n in runs}
            rec.update(legs=legs, **{n + "_ms": v for n, v in ms.items()},
                       conv_over_before=round(ms["conv"] / ms["before"], 4), conv_over_f_conv2d=round(ms["conv"] / ms["f_conv2d"], 4))
            if "general" in ms:
                rec["conv_over_general"] = round(ms["conv"] / ms["general"], 4)
            records.append(rec)
            print(json.dumps(rec), flush=True)
    torch.cuda.synchronize()
    path = Path(args.out) if args.out else OUT / "mx_conv_time.jsonl"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(json.dumps(r) for r in records) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None, help="the JSON lines' file (default: under profiles/r14)")
    main(ap.parse_args())
