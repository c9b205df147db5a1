"""Time dfq_pair_stats_batch on the bench headline's list, beside the sweep.

The list is bench.py's: 155 MobileNetV2 weight sets (8,215 tensors, 2.15 GB of fp32
weights), seeded as there.  The sweep writes its dequantized output out of place,
so the pairs are (weights, dq): a call reads 4.3 GB, well past the 256 MB Infinity
Cache.  The yardstick is the sweep's own achieved bytes per second on the same
list, in the same process, alternated three times with the new call; every timed
call sits inside a HIP event pair (both launches and the table upload), 10 warm-up
and 100 timed calls per leg, median.  Algorithmic bytes of the new call: 8 B per
element + 32 B per row + 32 B per partial slot.  One JSON line on stdout.

  python scripts/pair_stats_time.py            # the timing
  python scripts/pair_stats_time.py --reports  # MobileNetV2 quality-report figures per configuration
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench  # noqa: E402
from data_free_quantization_amd import _lib, distributed as D, quality  # noqa: E402

PEAK_TBS = 8.0   # MI355X HBM3E peak


def timed(run, stream, warmup, steps):
    for _ in range(warmup):
        run()
    return statistics.median(bench.steps_with_events(run, stream, steps))


def timing(args):
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    _lib.preload()
    b = bench.parse([])
    shapes = bench.model_shapes(b.model)
    per_copy = sum(int(torch.Size(s).numel()) for s in shapes)
    copies = args.copies or max(1, -(-(2 << 30) // (4 * per_copy)))
    specs = D.uniform_specs(shapes * copies, bits=b.bits, per_channel=b.granularity == "channel",
                            symmetric=not b.asym, want_esum=not b.no_esum, clip=(-15.0, 15.0))
    items = bench.make_list(specs, range(len(specs)), dev, 1234)
    plan = bench._plan_of(items)
    stream = torch.cuda.current_stream(dev)
    plan.execute(stream)   # dq exists from here
    pairs = [(it.src, it.dst) for it in items]
    call = quality.PairStatsCall(pairs)
    one = quality.PairStatsCall(pairs[:len(shapes)])
    elems = per_copy * copies
    rows = sum(s[0] for s in shapes) * copies
    P = _lib.DFQ_PAIR_PIECE_ELEMS
    row_lens = [(s[0], int(torch.Size(s).numel()) // s[0]) for s in shapes]
    slots = sum(r * -(-rl // P) for r, rl in row_lens if rl > P) * copies
    pair_bytes = 8 * elems + 32 * rows + 32 * slots
    sweep_bytes = int(plan.stats["algo_bytes"])
    legs = []
    for _ in range(3):
        sweep_ms = timed(lambda: plan.execute(stream), stream, args.warmup, args.steps)
        pair_ms = timed(lambda: call.run(stream), stream, args.warmup, args.steps)
        legs.append({"sweep_ms": round(sweep_ms, 4), "sweep_tbs": round(sweep_bytes / sweep_ms / 1e9, 3),
                     "pair_ms": round(pair_ms, 4), "pair_tbs": round(pair_bytes / pair_ms / 1e9, 3)})
    one_us = 1e3 * timed(lambda: one.run(stream), stream, args.warmup, args.steps)
    torch.cuda.synchronize()
    total = sum(float(r.total[1]) for r in call.results[:len(shapes)])   # the outputs are real: first set's noise
    pair_ms = statistics.median(leg["pair_ms"] for leg in legs)
    sweep_ms = statistics.median(leg["sweep_ms"] for leg in legs)
    print(json.dumps({
        "what": "dfq_pair_stats_batch on the bench headline list, pairs (weights, dq)",
        "device": torch.cuda.get_device_name(dev), "model": b.model, "copies": copies, "tensors": len(items),
        "elements": elems, "rows": rows, "partial_slots": slots, "warmup": args.warmup, "steps": args.steps,
        "pair_ms": pair_ms, "pair_algo_bytes": pair_bytes, "pair_tbs": round(pair_bytes / pair_ms / 1e9, 3),
        "pair_fraction_of_8tbs": round(pair_bytes / pair_ms / 1e9 / PEAK_TBS, 4),
        "sweep_ms": sweep_ms, "sweep_algo_bytes": sweep_bytes, "sweep_tbs": round(sweep_bytes / sweep_ms / 1e9, 3),
        "legs": legs, "one_model_us": round(one_us, 2), "one_model_tensors": len(shapes),
        "one_model_algo_bytes": pair_bytes // copies, "first_set_noise": total}))


def reports():
    """Model SQNR and worst layer of MobileNetV2 (zoo weights, seed 0) per configuration."""
    import torch.nn as nn
    from data_free_quantization_amd import zoo
    from data_free_quantization_amd.pipeline import run_dfq
    from data_free_quantization_amd.utils.tracer import build_graph
    targ = (nn.Conv2d, nn.Linear)
    configs = [("per-tensor asym INT8, --equalize", dict(equalize=True, absorption=True)),
               ("per-tensor asym INT8, no --equalize", dict(equalize=False, absorption=False)),
               ("per-channel sym INT8, --equalize", dict(equalize=True, absorption=True, granularity="channel",
                                                         symmetric=True))]
    for name, kw in configs:
        model = zoo.build("mobilenetv2", seed=0, relu=True).cuda()
        g = build_graph(model, "positional")
        rep = {}
        run_dfq(model, g.getGraph(), g.getBottoms(), targ, report=rep, **kw)
        m = rep["model"]
        worst = next(e for e in rep["layers"] if e["key"] == m["worst_layer"])
        prec = [e["channel_precision_mean"] for e in rep["layers"]]
        print(json.dumps({"config": name, "model_sqnr_db": round(m["sqnr_db"], 3), "worst_layer": m["worst_layer"],
                          "worst_layer_shape": worst["shape"], "worst_layer_sqnr_db": round(worst["sqnr_db"], 3),
                          "worst_channel_sqnr_db": round(min(e["worst_channel_sqnr_db"] for e in rep["layers"]), 3),
                          "mean_channel_precision": round(sum(prec) / len(prec), 4)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=0, help="weight sets (0: the bench's, >= 2 GiB)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reports", action="store_true")
    a = ap.parse_args()
    reports() if a.reports else timing(a)
