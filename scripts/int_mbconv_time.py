"""Time the one-launch integer inverted-residual block (intmm.int_mbconv_q) beside
the three-call chain on bytes it equals and beside three fp32 F.conv2d calls.

Four MobileNetV2 blocks at batch 32: 96 -> 576 -> 96 at 14^2 (stride 1), 16 -> 96 -> 24 at 112^2
(stride 2), 32 -> 192 -> 32 at 28^2 (stride 1), 160 -> 960 -> 320 at 7^2 (stride 1).  8-bit
asymmetric input codes on (-1.3, 2.5), per-tensor 8-bit weight codes, both hidden grids on [0, 6],
fp32 output.  Per block three legs, alternated three times in this process, each timed call inside
a HIP event pair, median of --steps calls after --warmup (scripts/int_io_time.py's method):
  fused     int_mbconv_q, one launch
  chain     int_conv2d_q -> int_dwconv2d_q -> int_conv2d_q as one timed region
  f_conv2d  three F.conv2d calls on fp32
The script asserts that the fused output equals the chain's bits; the times are data.

  python scripts/int_mbconv_time.py          # -> profiles/r23/int_mbconv_time.jsonl
"""
import argparse
import json
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from data_free_quantization_amd import _lib, intmm  # noqa: E402
from data_free_quantization_amd.utils.quantize import fake_quant  # noqa: E402
from scripts.int_io_time import BATCH, RELU6, XR, measure, weights  # noqa: E402

OUT = Path(__file__).resolve().parent.parent / "profiles" / "r23"
#: (name, Cin, Ch, Cout, H = W, stride)
BLOCKS = [("mobilenetv2_block_96_576_96_14", 96, 576, 96, 14, 1), ("mobilenetv2_block_16_96_24_112_s2", 16, 96, 24, 112, 2),
          ("mobilenetv2_block_32_192_32_28", 32, 192, 32, 28, 1), ("mobilenetv2_block_160_960_320_7", 160, 960, 320, 7, 1)]


def block(name, C, E, N, HW, s, g, dev, stream, args):
    x = (torch.randn(BATCH, C, HW, HW, generator=g) * 1.2 + 0.4).to(dev)
    xq = fake_quant(x.reshape(1, -1), 8, **XR).codes.view_as(x)
    (w1, d1), (w2, d2), (w3, d3) = weights(g, E, C, dev, 0.1), weights(g, E, 9, dev, 0.3), weights(g, N, E, dev, 0.05)
    b1, b2, b3 = ((torch.randn(n, generator=g) + 1.0).to(dev) for n in (E, E, N))
    oq = intmm.OutQuant(**RELU6)

    def fused():
        return intmm.int_mbconv_q(xq, (*w1, b1), (*w2, b2), (*w3, b3), stride=s, padding=1, hidden1=oq, hidden2=oq, **XR)

    def chain():
        c1 = intmm.int_conv2d_q(xq, *w1, 1, x_codes=True, bias=b1, out_quant=oq, **XR)
        c2 = intmm.int_dwconv2d_q(c1, *w2, 3, s, 1, x_codes=True, bias=b2, out_quant=oq, **RELU6)
        return intmm.int_conv2d_q(c2, *w3, 1, x_codes=True, bias=b3, **RELU6)

    def fp32():
        y = F.conv2d(x, d1.view(E, C, 1, 1), b1)
        y = F.conv2d(y, d2.view(E, 1, 3, 3), b2, s, 1, groups=E)
        return F.conv2d(y, d3.view(N, E, 1, 1), b3)

    assert torch.equal(fused().view(torch.int32), chain().view(torch.int32)), name
    legs, ms = measure({"fused": fused, "chain": chain, "f_conv2d": fp32}, stream, args)
    rec = {"what": "the one-launch inverted-residual block beside the three-call chain on bytes and three F.conv2d", "shape": name,
           "batch": BATCH, "Cin": C, "Ch": E, "Cout": N, "H": HW, "W": HW, "stride": s, "padding": 1,
           "device": torch.cuda.get_device_name(dev), "warmup": args.warmup, "steps": args.steps, "fused_equals_the_chain_bitwise": True,
           "legs": legs, **{n + "_ms": v for n, v in ms.items()}, "fused_over_chain": round(ms["fused"] / ms["chain"], 4),
           "fused_over_f_conv2d": round(ms["fused"] / ms["f_conv2d"], 4)}
    print(json.dumps(rec), flush=True)
    return rec


def main(args):
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    _lib.preload()
    stream = torch.cuda.current_stream(dev)
    g = torch.Generator().manual_seed(0)
    records = [block(*b, g, dev, stream, args) for b in BLOCKS]
    torch.cuda.synchronize()
    path = Path(args.out) if args.out else OUT / "int_mbconv_time.jsonl"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(json.dumps(r) for r in records) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None, help="the JSON lines' file (default: under profiles/r23)")
    main(ap.parse_args())
