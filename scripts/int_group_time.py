"""Time what group-wise B parameters cost dfq_int_gemm (intmm.int_gemm(b_group=g): an fp32 scale and
zero per g elements of a weight row, the group's fp64 steps applied where the group closes)
beside the per-row call of the same process -- the kernel it grew from, one scale per row applied
after the K loop.

Shapes: the README's three, [32, 1280] x [1000, 1280] (the classifier at batch 32),
[1568, 320] x [1280, 320] (MobileNetV2's last pointwise layer at batch 32) and 4096^3.  8-bit codes
on both sides, asymmetric (every term of the statement runs), with a bias.  Per shape the legs are
alternated three times in this process, each timed call inside a HIP event pair, median of --steps
calls after --warmup:
  per_row   int_gemm, b_scale / b_zero [N]
  g128, g64, g32   int_gemm(b_group=g), b_scale / b_zero [N, ceil(K / g)]
Only the same-process ratios g*_over_per_row mean anything across machines.  Data, not assertions.

  python scripts/int_group_time.py          # -> profiles/r21/int_group_time.jsonl
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench  # noqa: E402
from data_free_quantization_amd import _lib, intmm  # noqa: E402

OUT = Path(__file__).resolve().parent.parent / "profiles" / "r21"
SHAPES = [("classifier_b32", 32, 1000, 1280), ("pointwise_320_1280_b32", 1568, 1280, 320), ("square_4096", 4096, 4096, 4096)]
GROUPS = (128, 64, 32)


def timed(run, stream, warmup, steps):
    for _ in range(warmup):
        run()
    return statistics.median(bench.steps_with_events(run, stream, steps))


def main(args):
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    _lib.preload()
    stream = torch.cuda.current_stream(dev)
    gen = torch.Generator().manual_seed(0)
    records = []
    for name, M, N, K in SHAPES:
        a = torch.randint(0, 256, (M, K), generator=gen, dtype=torch.uint8).to(dev)
        b = torch.randint(0, 256, (N, K), generator=gen, dtype=torch.uint8).to(dev)
        sa, za = torch.tensor([0.02], device=dev), torch.tensor([-1.3], device=dev)
        bias = torch.randn(N, generator=gen).to(dev)
        out = torch.empty(M, N, device=dev)
        par = {g: ((torch.rand(N, -(-K // g), generator=gen) * 0.09 + 0.01).to(dev), (torch.rand(N, -(-K // g), generator=gen) * 6 - 3).to(dev))
               for g in GROUPS}
        row = (par[GROUPS[0]][0][:, 0].contiguous(), par[GROUPS[0]][1][:, 0].contiguous())
        runs = {"per_row": lambda: intmm.int_gemm(a, sa, za, b, row[0], row[1], K, bias=bias, out=out)}
        for g in GROUPS:
            runs["g%d" % g] = lambda g=g: intmm.int_gemm(a, sa, za, b, par[g][0], par[g][1], K, bias=bias, out=out, b_group=g)
        rec = {"what": "int_gemm(b_group=g) / int_gemm per row", "shape": name, "M": M, "N": N, "K": K, "bits": 8,
               "device": torch.cuda.get_device_name(dev), "warmup": args.warmup, "steps": args.steps}
        legs = [{n + "_ms": round(timed(r, stream, args.warmup, args.steps), 5) for n, r in runs.items()} for _ in range(3)]
        ms = {n: statistics.median(leg[n + "_ms"] for leg in legs) for n in runs}
        rec.update(legs=legs, **{n + "_ms": v for n, v in ms.items()},
                   **{"g%d_over_per_row" % g: round(ms["g%d" % g] / ms["per_row"], 4) for g in GROUPS})
        records.append(rec)
        print(json.dumps(rec), flush=True)
    torch.cuda.synchronize()
    path = Path(args.out) if args.out else OUT / "int_group_time.jsonl"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(json.dumps(r) for r in records) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None, help="the JSON lines' file (default: under profiles/r21)")
    main(ap.parse_args())
