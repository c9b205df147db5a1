"""Time dfq_clip_search_batch on the bench headline's list, beside the sweep.

The list is bench.py's: 155 MobileNetV2 weight sets (8,215 tensors, 2.15 GB of fp32
weights), seeded as there, searched in the bench's quantizer mode at INT4 and INT8
with 16 candidates down to half the range.  The timed calls are dry (the search
and its outputs, the weights left as they are, so every call does the same work);
one more call per bit width then clamps fresh copies in place, timed once.  The
yardstick is the sweep on the same list, in the same process, alternated three
times with the searches; every timed call sits inside a HIP event pair (all
launches and the table upload), median of --steps calls after --warmup.  By
operation count the search is VALU-bound (~K x 30 lane operations per element), so
the figure to read is the ratio to the sweep, not bytes per second.  The JSON lines
go to stdout and to --out.

  python scripts/clip_search_time.py             # the timing -> profiles/r08/clip_search_time.jsonl
  python scripts/clip_search_time.py --quality   # MobileNetV2 report figures with and without the search
                                                 #   -> profiles/r08/quality_clip_search.jsonl
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench  # noqa: E402
from data_free_quantization_amd import _lib, distributed as D  # noqa: E402
from data_free_quantization_amd.clip_weight import ClipItem, ClipSearchCall  # noqa: E402

K, MIN_FRAC = 16, 0.5
OUT = Path(__file__).resolve().parent.parent / "profiles" / "r08"


def emit(records, path):
    lines = [json.dumps(r) for r in records]
    print("\n".join(lines))
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(lines) + "\n")


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
    per_channel, symmetric = b.granularity == "channel", not b.asym
    specs = D.uniform_specs(shapes * copies, bits=b.bits, per_channel=per_channel, symmetric=symmetric,
                            want_esum=not b.no_esum, clip=(-15.0, 15.0))
    items = bench.make_list(specs, range(len(specs)), dev, 1234)
    plan = bench._plan_of(items)
    stream = torch.cuda.current_stream(dev)

    def call(bits, srcs, dry):
        return ClipSearchCall([ClipItem(s, bits=bits, per_channel=per_channel, symmetric=symmetric, candidates=K,
                                        min_frac=MIN_FRAC, dry=dry) for s in srcs])

    srcs = [it.src for it in items]
    calls = {bits: call(bits, srcs, True) for bits in (4, 8)}
    ones = {bits: call(bits, srcs[:len(shapes)], True) for bits in (4, 8)}
    legs = []
    for _ in range(3):
        leg = {"sweep_ms": round(timed(lambda: plan.execute(stream), stream, args.warmup, args.sweep_steps), 4)}
        for bits in (4, 8):
            leg["search_w%d_ms" % bits] = round(timed(lambda: calls[bits].run(stream), stream, args.warmup,
                                                      args.steps), 4)
        legs.append(leg)
    out = {"what": "dfq_clip_search_batch (dry) on the bench headline list, beside the sweep",
           "device": torch.cuda.get_device_name(dev), "model": b.model, "copies": copies, "tensors": len(items),
           "elements": per_copy * copies, "units": (sum(s[0] for s in shapes) if per_channel else len(shapes)) * copies,
           "granularity": b.granularity, "symmetric": symmetric, "candidates": K, "min_frac": MIN_FRAC,
           "warmup": args.warmup, "steps": args.steps, "sweep_steps": args.sweep_steps, "legs": legs}
    sweep_ms = statistics.median(leg["sweep_ms"] for leg in legs)
    out["sweep_ms"] = sweep_ms
    for bits in (4, 8):
        ms = statistics.median(leg["search_w%d_ms" % bits] for leg in legs)
        one_us = 1e3 * timed(lambda: ones[bits].run(stream), stream, args.warmup, args.steps)
        torch.cuda.synchronize()
        choice = calls[bits].choice
        out["w%d" % bits] = {"search_ms": ms, "ratio_to_sweep": round(ms / sweep_ms, 2),
                             "g_elements_per_s": round(per_copy * copies / ms / 1e6, 2),
                             "one_model_us": round(one_us, 2),
                             "narrowed_share": round(float((choice > 0).float().mean()), 4),
                             "at_edge_share": round(float((choice == K - 1).float().mean()), 4)}
    # the clamping call, once per bit width, on fresh copies of the first eight weight sets
    for bits in (4, 8):
        fresh = [s.clone() for s in srcs[:8 * len(shapes)]]
        wet, dry = call(bits, fresh, False), call(bits, fresh, True)
        dry_ms = timed(lambda: dry.run(stream), stream, 1, 3)
        wet_ms = bench.steps_with_events(lambda: wet.run(stream), stream, 1)[0]
        out["w%d" % bits]["eight_sets_dry_ms"] = round(dry_ms, 4)
        out["w%d" % bits]["eight_sets_clamping_ms"] = round(wet_ms, 4)
    emit([out], Path(args.out) if args.out else OUT / "clip_search_time.jsonl")


def quality_records(args):
    """Model SQNR, worst channel and share of narrowed units of MobileNetV2 (zoo
    weights, seed 0): per channel (symmetric) and per tensor (asymmetric), W4 and
    W8, without and with the search.  One JSON line each: data, not assertions."""
    import torch.nn as nn
    from data_free_quantization_amd import zoo
    from data_free_quantization_amd.pipeline import run_dfq
    from data_free_quantization_amd.utils.tracer import build_graph
    targ = (nn.Conv2d, nn.Linear)
    records = []
    for gran, sym in (("channel", True), ("tensor", False)):
        for bits in (4, 8):
            for search in (None, {"candidates": K, "min_frac": MIN_FRAC}):
                model = zoo.build("mobilenetv2", seed=0, relu=True).cuda()
                g = build_graph(model, "positional")
                rep = {}
                run_dfq(model, g.getGraph(), g.getBottoms(), targ, report=rep, bits_weight=bits, granularity=gran,
                        symmetric=sym, clip_search=search)
                m = rep["model"]
                rec = {"granularity": gran, "symmetric": sym, "bits_weight": bits, "clip_search": search is not None,
                       "candidates": K if search else None, "min_frac": MIN_FRAC if search else None,
                       "model_sqnr_db": round(m["sqnr_db"], 3), "worst_layer": m["worst_layer"],
                       "worst_channel_sqnr_db": round(min(e["worst_channel_sqnr_db"] for e in rep["layers"]), 3)}
                if search:
                    units = sum(e["clip_units"] for e in rep["layers"])
                    rec.update(units=units, narrowed_share=round(sum(e["clip_narrowed"] for e in rep["layers"]) / units, 4),
                               at_edge_share=round(sum(e["clip_at_edge"] for e in rep["layers"]) / units, 4))
                records.append(rec)
    emit(records, Path(args.out) if args.out else OUT / "quality_clip_search.jsonl")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=0, help="weight sets (0: the bench's, >= 2 GiB)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sweep_steps", type=int, default=100)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--out", default=None, help="the JSON lines' file (default: under profiles/r08)")
    a = ap.parse_args()
    quality_records(a) if a.quality else timing(a)
