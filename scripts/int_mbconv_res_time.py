"""Time the inverted-residual block with its shortcut in the epilogue (intmm.int_mbconv_q(residual=...),
DESIGN.md 3.9.3) beside the two routes it replaces, and intmm.int_add_q alone.

MobileNetV2's five residual block shapes at batch 32, uint8 codes in and out: 24 -> 144 -> 24 at
56^2, 32 -> 192 -> 32 at 28^2, 64 -> 384 -> 64 at 14^2, 96 -> 576 -> 96 at 14^2, 160 -> 960 -> 160
at 7^2.  8-bit asymmetric input codes on (-1.3, 2.5), per-tensor 8-bit weight codes, both hidden
grids on [0, 6]; the project's grid P and the output grid are the 5th and 95th percentile of the
tensors they hold.  Per block four legs, alternated three times in this process, each timed call
inside a HIP event pair, median of --steps calls after --warmup (scripts/int_io_time.py's method):
  fused   int_mbconv_q(residual=P, out_quant=O), one launch
  split   int_mbconv_q(out_quant=P), then int_add_q, two launches
  torch   int_mbconv_q to fp32, then dequantize x, add, fake_quant_given and the cast to codes in torch
  add     int_add_q alone on the block's output size -- also as a share of 8 TB/s at 3 B an element
A last record times int_add_q on 2^28 elements, which no cache holds: code output with every base
aligned, with every base 1 B off (a head before the first 16-B boundary), with only b 1 B off (its
bytes loaded one by one), and fp32 output (6 B an element).
The script asserts that the fused output equals the split route's bytes; the times are data.

  python scripts/int_mbconv_res_time.py          # -> profiles/r24/int_mbconv_res_time.jsonl
"""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from data_free_quantization_amd import _lib, intmm  # noqa: E402
from data_free_quantization_amd.utils.quantize import fake_quant, fake_quant_given  # noqa: E402
from scripts.int_io_time import BATCH, RELU6, XR, measure, weights  # noqa: E402

OUT = Path(__file__).resolve().parent.parent / "profiles" / "r24"
HBM_BYTES_PER_S = 8e12
#: (name, Cin = Cout, Ch, H = W)
BLOCKS = [("mobilenetv2_res_24_144_24_56", 24, 144, 56), ("mobilenetv2_res_32_192_32_28", 32, 192, 28), ("mobilenetv2_res_64_384_64_14", 64, 384, 14),
          ("mobilenetv2_res_96_576_96_14", 96, 576, 14), ("mobilenetv2_res_160_960_160_7", 160, 960, 7)]


def _grid(t):
    lo, hi = torch.quantile(t.float().flatten()[:1 << 22], torch.tensor([0.05, 0.95], device=t.device)).tolist()
    return dict(min_value=lo, max_value=hi)


def block(name, C, E, HW, g, dev, stream, args):
    x = (torch.randn(BATCH, C, HW, HW, generator=g) * 1.2 + 0.4).to(dev)
    xr = fake_quant(x.reshape(1, -1), 8, **XR)
    xq, s_x, z_x = xr.codes.view_as(x), xr.scale.reshape(()), xr.zero.reshape(())
    (w1, _), (w2, _), (w3, _) = weights(g, E, C, dev, 0.1), weights(g, E, 9, dev, 0.3), weights(g, C, E, dev, 0.05)
    layers = [(*w, (torch.randn(n, generator=g) + 1.0).to(dev)) for w, n in ((w1, E), (w2, E), (w3, C))]
    h, X = intmm.OutQuant(**RELU6), intmm.OutQuant(**XR)
    mb = lambda **kw: intmm.int_mbconv_q(xq, *layers, stride=1, padding=1, hidden1=h, hidden2=h, **XR, **kw)   # noqa: E731
    y = mb()
    P = _grid(y)
    O = _grid(y + (xq.float() * s_x + z_x))
    oqp, oqo = intmm.OutQuant(**P), intmm.OutQuant(**O)
    c3, out8, y32, r32 = mb(out_quant=oqp), torch.empty_like(xq), torch.empty_like(y), torch.empty_like(y)

    def split():
        mb(out_quant=oqp, out=c3)
        return intmm.int_add_q(c3, oqp, xq, X, out_quant=oqo, out=out8)

    def route():   # what a caller had before: the fp32 round trip of the block's output
        mb(out=y32)
        v = fake_quant_given(y32 + (xq.float() * s_x + z_x), 8, out=r32, **O)
        return torch.round((v - O["min_value"]) / ((O["max_value"] - O["min_value"]) / 255)).to(torch.uint8)

    runs = {"fused": lambda: mb(residual=oqp, out_quant=oqo, out=out8), "split": split, "torch": route,
            "add": lambda: intmm.int_add_q(c3, oqp, xq, X, out_quant=oqo, out=out8)}
    same = bool(torch.equal(runs["fused"]().clone(), split()))
    assert same, name
    legs, ms = measure(runs, stream, args)
    n = xq.numel()
    rec = {"what": "the residual block in one launch beside int_mbconv_q + int_add_q and beside the fp32 round trip through torch; int_add_q alone",
           "shape": name, "batch": BATCH, "Cin": C, "Ch": E, "Cout": C, "H": HW, "W": HW, "elements": n,
           "device": torch.cuda.get_device_name(dev), "warmup": args.warmup, "steps": args.steps, "fused_equals_split_bitwise": same,
           "legs": legs, **{k + "_ms": v for k, v in ms.items()}, "fused_over_split": round(ms["fused"] / ms["split"], 4),
           "fused_over_torch": round(ms["fused"] / ms["torch"], 4),
           "add_share_of_8TBps_at_3B": round(3 * n / HBM_BYTES_PER_S / (ms["add"] * 1e-3), 4)}
    print(json.dumps(rec), flush=True)
    return rec


def large_add(n, dev, stream, args):
    """int_add_q beyond every cache: n elements, uint8 and fp32 output, aligned and with every base 1 B off."""
    a, b = (torch.randint(0, 256, (n + 1,), dtype=torch.uint8, device=dev) for _ in range(2))
    o8, o32 = torch.empty(n + 1, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    X, O = intmm.OutQuant(**XR), intmm.OutQuant(min_value=-1.0, max_value=4.0)
    runs = {"codes": lambda: intmm.int_add_q(a[:n], X, b[:n], X, out_quant=O, out=o8[:n]),
            "codes_shifted": lambda: intmm.int_add_q(a[1:], X, b[1:], X, out_quant=O, out=o8[1:]),
            "codes_b_off": lambda: intmm.int_add_q(a[:n], X, b[1:], X, out_quant=O, out=o8[:n]),
            "fp32": lambda: intmm.int_add_q(a[:n], X, b[:n], X, out=o32)}
    legs, ms = measure(runs, stream, args)
    rate = lambda k, bytes_per: round(bytes_per * n / (ms[k] * 1e-3) / HBM_BYTES_PER_S, 4)   # noqa: E731
    rec = {"what": "int_add_q alone on a tensor no cache holds", "shape": "add_%d" % n, "elements": n, "device": torch.cuda.get_device_name(dev),
           "warmup": args.warmup, "steps": args.steps, "legs": legs, **{k + "_ms": v for k, v in ms.items()},
           "codes_share_of_8TBps_at_3B": rate("codes", 3), "codes_shifted_share_of_8TBps_at_3B": rate("codes_shifted", 3),
           "codes_b_off_share_of_8TBps_at_3B": rate("codes_b_off", 3), "fp32_share_of_8TBps_at_6B": rate("fp32", 6)}
    print(json.dumps(rec), flush=True)
    return rec


def main(args):
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    _lib.preload()
    stream = torch.cuda.current_stream(dev)
    g = torch.Generator().manual_seed(0)
    records = [block(*b, g, dev, stream, args) for b in BLOCKS]
    records.append(large_add(1 << 28, dev, stream, args))
    torch.cuda.synchronize()
    path = Path(args.out) if args.out else OUT / "int_mbconv_res_time.jsonl"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(json.dumps(r) for r in records) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None, help="the JSON lines' file (default: under profiles/r24)")
    main(ap.parse_args())
