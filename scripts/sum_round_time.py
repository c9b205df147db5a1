"""Time sum rounding (rounding.sum_round) beside the nearest-rounding sweep
(SweepPlan.execute) on the zoo MobileNetV2 and ResNet-50 weight lists, 4 bits per channel
asymmetric, out of place, dequantized values and codes written by both.

Per model the two legs are alternated three times in this process, each timed call inside
a HIP event pair, median of --steps calls after --warmup.  sum_round's timed call includes
its host work (the table, the output allocations); the sweep's is the prepared plan's
execute alone.  Also recorded, informational: the flips, the per-channel |sum(dq - w)| / s
before and after (mean and max over all channels), and the SQNR of both roundings from
quality.pair_stats.  Data, not assertions.

  python scripts/sum_round_time.py          # -> profiles/r20/sum_round_time.jsonl
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch
import torch.nn as nn

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench  # noqa: E402
from data_free_quantization_amd import _lib, quality, sweep, zoo  # noqa: E402
from data_free_quantization_amd.rounding import SumRoundItem, sum_round  # noqa: E402

OUT = Path(__file__).resolve().parent.parent / "profiles" / "r20"
BITS = 4


def timed(run, stream, warmup, steps):
    for _ in range(warmup):
        run()
    return statistics.median(bench.steps_with_events(run, stream, steps))


def main(args):
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    _lib.preload()
    stream = torch.cuda.current_stream(dev)
    records = []
    for name in ("mobilenetv2", "resnet50"):
        model = zoo.build(name, seed=0).to(dev).eval()
        ws = [m.weight.detach() for m in model.modules() if isinstance(m, (nn.Conv2d, nn.Linear))]
        ws = [w for w in ws if w.numel() // w.shape[0] <= _lib.DFQ_SR_MAX_ROW]
        items = [SumRoundItem(w, bits=BITS, per_channel=True, khw=sweep.khw_of(w), want_flips=True) for w in ws]
        plan_items = [sweep.allocate(w, bits=BITS, per_channel=True, symmetric=False, khw=sweep.khw_of(w)) for w in ws]
        plan = sweep.SweepPlan(plan_items)
        runs = {"sum_round": lambda: sum_round(items), "sweep": plan.execute}
        legs = [{n + "_ms": round(timed(r, stream, args.warmup, args.steps), 5) for n, r in runs.items()} for _ in range(3)]
        ms = {n: statistics.median(leg[n + "_ms"] for leg in legs) for n in runs}
        res = sum_round(items)
        plan.execute()
        torch.cuda.synchronize()
        shift = {"nearest": [], "sum": []}   # per channel |sum(dq - w)| / s
        for w, r, p in zip(ws, res, plan_items):
            for key, dq in (("nearest", p.dst), ("sum", r.dq)):
                shift[key].append(((dq - w).double().flatten(1).sum(1).abs() / r.scale.double()).cpu())
        shift = {k: torch.cat(v) for k, v in shift.items()}
        sq = {}
        for key, dqs in (("nearest", [p.dst for p in plan_items]), ("sum", [r.dq for r in res])):
            tot = torch.stack([s.total for s in quality.pair_stats(list(zip(ws, dqs)), per_row=False)]).sum(0).cpu()
            sq[key] = quality.sqnr_db(tot[0], tot[1])
        rec = {"what": "sum_round vs SweepPlan.execute, W4 per channel asymmetric", "model": name, "weights": len(ws),
               "elements": sum(w.numel() for w in ws), "channels": int(shift["sum"].numel()), "bits": BITS,
               "device": torch.cuda.get_device_name(dev), "warmup": args.warmup, "steps": args.steps, "legs": legs,
               **{n + "_ms": v for n, v in ms.items()}, "sum_round_over_sweep": round(ms["sum_round"] / ms["sweep"], 3),
               "kernel_stage_flips": int(sum(int(r.flips[:, 0].sum()) for r in res)),
               "channel_stage_flips": int(sum(int(r.flips[:, 1].sum()) for r in res)),
               **{"channel_shift_steps_%s_%s" % (k, f): round(float(getattr(v, f)()), 4) for k, v in shift.items()
                  for f in ("mean", "max")},
               "sqnr_db_nearest": round(sq["nearest"], 3), "sqnr_db_sum": round(sq["sum"], 3)}
        records.append(rec)
        print(json.dumps(rec), flush=True)
        plan.destroy()
    torch.cuda.synchronize()
    path = Path(args.out) if args.out else OUT / "sum_round_time.jsonl"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(json.dumps(r) for r in records) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None, help="the JSON lines' file (default: under profiles/r20)")
    main(ap.parse_args())
