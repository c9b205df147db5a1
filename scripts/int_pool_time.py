"""Time the pooling entries on stored codes (intmm.int_mean_q, intmm.int_maxpool2d_q)
beside the route a caller had before them.

Batch 32, uint8 codes on (-1.3, 2.5) in, uint8 codes out on the 5th and 95th percentile of the result:
  mean     [32, 1280, 7, 7] (MobileNetV2's head), [32, 2048, 7, 7] (ResNet-50's), [32, 256, 33, 33] (DeepLab's ASPP)
  maxpool  [32, 64, 112, 112] with 3 x 3, stride 2, padding 1 (the ResNets' stem); the output stays on the input's grid
Per shape two legs, alternated three times in this process, each timed call inside a HIP event pair,
median of --steps calls after --warmup (scripts/int_io_time.py's method):
  codes   the new entry, one launch
  torch   mean: dequantize in torch, mean, fake_quant_given, the cast to codes
          maxpool: dequantize, F.max_pool2d, fake_quant_given on the input's grid, the cast to codes
The algorithmic bytes are one per input element and one per output element; a record gives the new
call's share of 8 TB/s over them.  The script asserts that the max pool's two routes agree bit for
bit and that the mean's codes differ from the torch route's by at most one step (the routes round
differently: 3.9.4); the times are data.

  python scripts/int_pool_time.py          # -> profiles/r25/int_pool_time.jsonl
"""
import argparse
import json
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from data_free_quantization_amd import _lib, intmm  # noqa: E402
from data_free_quantization_amd.utils.quantize import fake_quant, fake_quant_given  # noqa: E402
from scripts.int_io_time import BATCH, XR, measure  # noqa: E402

OUT = Path(__file__).resolve().parent.parent / "profiles" / "r25"
HBM_BYTES_PER_S = 8e12
MEANS = [("mobilenetv2_head_1280_7", 1280, 7), ("resnet50_head_2048_7", 2048, 7), ("deeplab_aspp_256_33", 256, 33)]
MAXPOOLS = [("resnet_stem_64_112", 64, 112, 3, 2, 1)]


def _codes(C, HW, g, dev):
    """uint8 codes of a draw on XR, with the grid's scale and zero (0-d tensors)."""
    x = (torch.randn(BATCH, C, HW, HW, generator=g) * 1.2 + 0.4).to(dev)
    r = fake_quant(x.reshape(1, -1), 8, **XR)
    return r.codes.view_as(x), r.scale.reshape(()), r.zero.reshape(())


def _to_codes(v, lo, hi):   # the cast a caller writes after fake_quant_given
    return torch.round((v - lo) / ((hi - lo) / 255)).to(torch.uint8)


def _record(what, name, shape, n_in, n_out, dev, args, legs, ms, **more):
    rec = {"what": what, "shape": name, "batch": BATCH, "x": list(shape), "bytes": n_in + n_out, "device": torch.cuda.get_device_name(dev),
           "warmup": args.warmup, "steps": args.steps, "legs": legs, **{k + "_ms": v for k, v in ms.items()},
           "codes_over_torch": round(ms["codes"] / ms["torch"], 4),
           "codes_share_of_8TBps": round((n_in + n_out) / HBM_BYTES_PER_S / (ms["codes"] * 1e-3), 4), **more}
    print(json.dumps(rec), flush=True)
    return rec


def mean(name, C, HW, g, dev, stream, args):
    xq, s, z = _codes(C, HW, g, dev)
    X = intmm.OutQuant(**XR)
    y = intmm.int_mean_q(xq, X)
    lo, hi = torch.quantile(y.flatten(), torch.tensor([0.05, 0.95], device=dev)).tolist()
    O, out8, r32 = intmm.OutQuant(min_value=lo, max_value=hi), torch.empty(BATCH, C, dtype=torch.uint8, device=dev), torch.empty(BATCH, C, device=dev)

    def route():
        m = (xq.float() * s + z).view(BATCH, C, -1).mean(-1)
        return _to_codes(fake_quant_given(m, 8, out=r32, min_value=lo, max_value=hi), lo, hi)

    runs = {"codes": lambda: intmm.int_mean_q(xq, X, out_quant=O, out=out8), "torch": route}
    step = int((runs["codes"]().int() - route().int()).abs().max())
    assert step <= 1, (name, step)
    legs, ms = measure(runs, stream, args)
    return _record("the mean over H * W on stored codes beside dequantize, mean, fake_quant_given and the cast in torch", name, xq.shape,
                   xq.numel(), BATCH * C, dev, args, legs, ms, largest_code_difference=step)


def maxpool(name, C, HW, k, s_, p, g, dev, stream, args):
    xq, s, z = _codes(C, HW, g, dev)
    X = intmm.OutQuant(**XR)
    out8 = intmm.int_maxpool2d_q(xq, X, k, s_, p)
    r32 = torch.empty(out8.shape, device=dev)

    def route():
        m = F.max_pool2d(xq.float() * s + z, k, s_, p)
        return _to_codes(fake_quant_given(m, 8, out=r32, **XR), XR["min_value"], XR["max_value"])

    runs = {"codes": lambda: intmm.int_maxpool2d_q(xq, X, k, s_, p, out=out8), "torch": route}
    same = bool(torch.equal(runs["codes"](), route()))
    assert same, name
    legs, ms = measure(runs, stream, args)
    return _record("max pooling on stored codes beside dequantize, F.max_pool2d, fake_quant_given and the cast in torch", name, xq.shape,
                   xq.numel(), out8.numel(), dev, args, legs, ms, kernel=k, stride=s_, padding=p, codes_equal_torch_bitwise=same)


def main(args):
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    _lib.preload()
    stream = torch.cuda.current_stream(dev)
    g = torch.Generator().manual_seed(0)
    records = [mean(*m, g, dev, stream, args) for m in MEANS] + [maxpool(*m, g, dev, stream, args) for m in MAXPOOLS]
    torch.cuda.synchronize()
    path = Path(args.out) if args.out else OUT / "int_pool_time.jsonl"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(json.dumps(r) for r in records) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None, help="the JSON lines' file (default: under profiles/r25)")
    main(ap.parse_args())
