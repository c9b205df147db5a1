"""Time the code-in / code-out integer entries (intmm.int_conv2d_q, intmm.int_dwconv2d_q: stored
activation codes at either end) beside the route they replace and beside fp32.

Shapes at batch 32: the five convolution layers of README's integer convolution table
(scripts/int_conv_time.py's) and three depthwise 3 x 3 s1 p1 layers of MobileNetV2 (C = 32 at
112^2, C = 192 at 28^2, C = 960 at 7^2).  8-bit asymmetric activations on host ranges, per-tensor
8-bit weight codes; the output range of a layer is [0, 6].  Per layer four legs, alternated three
times in this process, each timed call inside a HIP event pair, median of --steps calls after
--warmup:
  codes     the new call, uint8 codes in and uint8 codes out
  fp32      the new call with neither option (must tie `old`: it is the old entry)
  old       the route `codes` replaces: the old entry, then the fake_quant_given launch that
            rounds its fp32 result for the next layer
  f_conv2d  F.conv2d on fp32
and the three-layer chain of tests/test_gpu_int_io.py at MobileNetV2's 14^2 block size
(96 -> 576 pointwise, 576 depthwise 3 x 3, 576 -> 96 pointwise): the chain on bytes, the existing
route (three old entries, two fake_quant_given launches), the three fp32 calls, and each layer of
the two routes on its own (new1..3, old1..3; old1 and old2 include their fake_quant_given).  Every record
says whether the new route gave the old route's bits.  Data, not assertions.

  python scripts/int_io_time.py          # -> profiles/r22/int_io_time.jsonl
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from data_free_quantization_amd import _lib, intmm, mx  # noqa: E402
from data_free_quantization_amd.utils.quantize import fake_quant, fake_quant_given  # noqa: E402
from scripts.int_conv_time import SHAPES as CONV_SHAPES, timed  # noqa: E402

OUT = Path(__file__).resolve().parent.parent / "profiles" / "r22"
BATCH = 32
#: (name, C, H, W): depthwise 3 x 3, stride 1, padding 1
DW_SHAPES = [("mobilenetv2_dw_32_112", 32, 112, 112), ("mobilenetv2_dw_192_28", 192, 28, 28), ("mobilenetv2_dw_960_7", 960, 7, 7)]
XR, RELU6 = dict(min_value=-1.3, max_value=2.5), dict(min_value=0.0, max_value=6.0)


def weights(g, N, K, dev, scale=0.05):
    r = fake_quant((torch.randn(N, K, generator=g) * scale).to(dev), 8)
    return (r.codes, r.scale, r.zero), r.dq


def measure(runs, stream, args):
    legs = [{n + "_ms": round(timed(r, stream, args.warmup, args.steps), 5) for n, r in runs.items()} for _ in range(3)]
    ms = {n: statistics.median(leg[n + "_ms"] for leg in legs) for n in runs}
    return legs, ms


def layer(name, depthwise, Cin, H, W, N, k, s, p, g, dev, stream, args):
    x = (torch.randn(BATCH, Cin, H, W, generator=g) * 1.2 + 0.4).to(dev)
    K = k * k if depthwise else Cin * k * k
    wq, wdq = weights(g, N, K, dev)
    bias = (torch.randn(N, generator=g) + 2.0).to(dev)
    OH, OW = mx.conv_out_size(H, k, s, p, 1), mx.conv_out_size(W, k, s, p, 1)
    xq = fake_quant(x.reshape(1, -1), 8, **XR).codes.view_as(x)
    new, old = (intmm.int_dwconv2d_q, intmm.int_dwconv2d) if depthwise else (intmm.int_conv2d_q, intmm.int_conv2d)
    oq = intmm.OutQuant(**RELU6)
    out8, out32, rounded = (torch.empty(BATCH, N, OH, OW, dtype=t, device=dev) for t in (torch.uint8, torch.float32, torch.float32))
    w4 = wdq.view(N, 1 if depthwise else Cin, k, k)

    def route():
        old(x, *wq, k, s, p, 1, bias=bias, out=out32, **XR)
        return fake_quant_given(out32, 8, out=rounded, **RELU6)

    runs = {"codes": lambda: new(xq, *wq, k, s, p, 1, x_codes=True, bias=bias, out_quant=oq, out=out8, **XR),
            "fp32": lambda: new(x, *wq, k, s, p, 1, bias=bias, out=out32, **XR),
            "old": route,
            "f_conv2d": lambda: F.conv2d(x, w4, bias, s, p, groups=Cin if depthwise else 1)}
    route()
    same = bool(torch.equal(runs["codes"](), fake_quant(out32.reshape(1, -1), 8, **RELU6).codes.view_as(out8)))
    legs, ms = measure(runs, stream, args)
    rec = {"what": "codes in / codes out beside the old entry + fake_quant_given, the old entry alone and F.conv2d", "shape": name,
           "depthwise": depthwise, "batch": BATCH, "C": Cin, "H": H, "W": W, "N": N, "kernel": k, "stride": s, "padding": p,
           "device": torch.cuda.get_device_name(dev), "warmup": args.warmup, "steps": args.steps, "codes_equal_the_old_route_bitwise": same,
           "legs": legs, **{n + "_ms": v for n, v in ms.items()}, "codes_over_old": round(ms["codes"] / ms["old"], 4),
           "fp32_over_old": round(ms["fp32"] / ms["old"], 4), "codes_over_f_conv2d": round(ms["codes"] / ms["f_conv2d"], 4)}
    print(json.dumps(rec), flush=True)
    return rec


def chain(g, dev, stream, args):
    C, E, HW = 96, 576, 14
    x = (torch.randn(BATCH, C, HW, HW, generator=g) * 1.2 + 0.4).to(dev)
    (w1, d1), (w2, d2), (w3, d3) = weights(g, E, C, dev, 0.1), weights(g, E, 9, dev, 0.3), weights(g, C, E, dev, 0.05)
    b1, b2, b3 = ((torch.randn(n, generator=g) + 1.0).to(dev) for n in (E, E, C))
    oq = intmm.OutQuant(**RELU6)

    def new():
        c1 = intmm.int_conv2d_q(x, *w1, 1, bias=b1, out_quant=oq, **XR)
        c2 = intmm.int_dwconv2d_q(c1, *w2, 3, 1, 1, x_codes=True, bias=b2, out_quant=oq, **RELU6)
        return intmm.int_conv2d_q(c2, *w3, 1, x_codes=True, bias=b3, **RELU6)

    def old():
        y = fake_quant_given(intmm.int_conv2d(x, *w1, 1, bias=b1, **XR), 8, **RELU6)
        y = fake_quant_given(intmm.int_dwconv2d(y, *w2, 3, 1, 1, bias=b2, **RELU6), 8, **RELU6)
        return intmm.int_conv2d(y, *w3, 1, bias=b3, **RELU6)

    def fp32():
        y = F.conv2d(x, d1.view(E, C, 1, 1), b1)
        y = F.conv2d(y, d2.view(E, 1, 3, 3), b2, 1, 1, groups=E)
        return F.conv2d(y, d3.view(C, E, 1, 1), b3)

    same = bool(torch.equal(new().view(torch.int32), old().view(torch.int32)))
    # each layer of the two routes on its own, on that route's own input
    c1 = intmm.int_conv2d_q(x, *w1, 1, bias=b1, out_quant=oq, **XR)
    c2 = intmm.int_dwconv2d_q(c1, *w2, 3, 1, 1, x_codes=True, bias=b2, out_quant=oq, **RELU6)
    y1 = fake_quant_given(intmm.int_conv2d(x, *w1, 1, bias=b1, **XR), 8, **RELU6)
    y2 = fake_quant_given(intmm.int_dwconv2d(y1, *w2, 3, 1, 1, bias=b2, **RELU6), 8, **RELU6)
    stages = {"new1": lambda: intmm.int_conv2d_q(x, *w1, 1, bias=b1, out_quant=oq, **XR),
              "new2": lambda: intmm.int_dwconv2d_q(c1, *w2, 3, 1, 1, x_codes=True, bias=b2, out_quant=oq, **RELU6),
              "new3": lambda: intmm.int_conv2d_q(c2, *w3, 1, x_codes=True, bias=b3, **RELU6),
              "old1": lambda: fake_quant_given(intmm.int_conv2d(x, *w1, 1, bias=b1, **XR), 8, **RELU6),
              "old2": lambda: fake_quant_given(intmm.int_dwconv2d(y1, *w2, 3, 1, 1, bias=b2, **RELU6), 8, **RELU6),
              "old3": lambda: intmm.int_conv2d(y2, *w3, 1, bias=b3, **RELU6)}
    legs, ms = measure({"chain": new, "old": old, "fp32": fp32, **stages}, stream, args)
    rec = {"what": "1x1 -> depthwise 3x3 -> 1x1 on bytes beside the old entries with fake_quant_given between them and three F.conv2d",
           "shape": "mobilenetv2_block_96_576_96_14", "batch": BATCH, "device": torch.cuda.get_device_name(dev), "warmup": args.warmup,
           "steps": args.steps, "chain_equals_the_old_route_bitwise": same, "legs": legs, **{n + "_ms": v for n, v in ms.items()},
           "chain_over_old": round(ms["chain"] / ms["old"], 4), "chain_over_fp32": round(ms["chain"] / ms["fp32"], 4)}
    print(json.dumps(rec), flush=True)
    return rec


def main(args):
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    _lib.preload()
    stream = torch.cuda.current_stream(dev)
    g = torch.Generator().manual_seed(0)
    records = [layer(name, False, C, H, W, N, k, s, p, g, dev, stream, args) for name, C, H, W, N, k, s, p in CONV_SHAPES]
    records += [layer(name, True, C, H, W, C, 3, 1, 1, g, dev, stream, args) for name, C, H, W in DW_SHAPES]
    records.append(chain(g, dev, stream, args))
    torch.cuda.synchronize()
    path = Path(args.out) if args.out else OUT / "int_io_time.jsonl"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(json.dumps(r) for r in records) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None, help="the JSON lines' file (default: under profiles/r22)")
    main(ap.parse_args())
