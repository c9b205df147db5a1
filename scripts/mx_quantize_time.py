"""Time dfq_mx_quantize_batch on the bench headline's list, beside the sweep.

The list is bench.py's: 155 MobileNetV2 weight sets (8,215 tensors, 2.15 GB of fp32
weights), seeded as there.  Each MX format writes dst + codes + scales + esum for
every tensor in one call (one launch, one HBM pass); dst and esum are the sweep
items' own buffers, so both passes write the same places.  The yardstick is the
bench's sweep (per-channel INT8 with its codes and error sums) on the same list, in
the same process, alternated three times with the MX calls; every timed call sits
inside a HIP event pair (the table upload and the launch), median of --steps calls
after --warmup.  Fractions are algorithmic bytes (computed here from the shapes:
read 4, write 4 + 0.5 | 0.75 | 1 of codes + 1/32 of scales per padded element + 4/khw of
error sums) over time over the 8 TB/s HBM peak; the sweep's are its plan's
algo_bytes.  A whole call over peak is an end-to-end figure (it holds the table
upload), not the kernel's share.  One weight set alone is timed the same way, in
microseconds.  The JSON line goes to stdout and to --out.

  python scripts/mx_quantize_time.py             # -> profiles/r10/mx6_quantize_time.jsonl
  python scripts/mx_quantize_time.py --quality   # MobileNetV2 model SQNR per format, with and
                                                 #   without equalization -> profiles/r10/quality_mx6.jsonl
  python scripts/mx_quantize_time.py --ab OTHER.so   # MXFP4 / MXFP8 call times of another build of the
                                                 #   library (the parent commit's) against this tree's, alternated
                                                 #   three times in this process -> profiles/r10/mx6_parent_ab.jsonl
  python scripts/mx_quantize_time.py --search    # dfq_mx_quantize_search_batch against the floor call, per format,
                                                 #   alternated three times -> profiles/r12/mx_search_time.jsonl
  python scripts/mx_quantize_time.py --search_quality   # MobileNetV2 model SQNR per format with and without
                                                 #   --mx_scale_search, and the logits SQNR of the forward on the matrix
                                                 #   instruction with searched MXFP8 weights -> profiles/r12/quality_mx_search.jsonl
"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench  # noqa: E402
from data_free_quantization_amd import _lib, distributed as D, mx  # noqa: E402

OUT = Path(__file__).resolve().parent.parent / "profiles" / "r10"
OUT_SEARCH = Path(__file__).resolve().parent.parent / "profiles" / "r12"


def emit(records, path):
    lines = [json.dumps(r) for r in records]
    print("\n".join(lines))
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(lines) + "\n")


def timed(run, stream, warmup, steps):
    for _ in range(warmup):
        run()
    return statistics.median(bench.steps_with_events(run, stream, steps))


class MxCall:
    """A prepared dfq_mx_quantize_batch call over sweep items: the descriptor table,
    the code and scale arenas and the workspace; run() is the one C call.  ``share``:
    an MXFP8 call over the same items whose arenas and workspace this one writes too --
    where a buffer lies moves a call's time by percents, more than the formats differ."""

    def __init__(self, items, fmt, share=None):
        self._lib = _lib.load()
        dev = items[0].src.device
        cb = mx.FORMATS[fmt][2]
        geo = []
        for it in items:
            rows = it.src.shape[0]
            geo.append((rows, it.src.numel() // rows, mx.blocks(it.src.numel() // rows)))
        if share is not None:
            self.codes, self.scales = share.codes, share.scales
        else:
            self.codes = torch.empty(sum(r * nb * cb for r, _, nb in geo), dtype=torch.uint8, device=dev)
            self.scales = torch.empty(sum(-(-r * nb // 16) * 16 for r, _, nb in geo), dtype=torch.uint8, device=dev)
        assert self.codes.numel() >= sum(r * nb * cb for r, _, nb in geo)
        tab, co, so, self.algo_bytes = [], 0, 0, 0
        for it, (rows, row_len, nb) in zip(items, geo):
            tab.append((it.src.data_ptr(), it.dst.data_ptr(), self.codes.data_ptr() + co, self.scales.data_ptr() + so,
                        it.esum.data_ptr() if it.esum is not None else 0, rows, row_len, it.khw, mx.FORMATS[fmt][0], 0, 0))
            co += rows * nb * cb
            so += -(-rows * nb // 16) * 16
            self.algo_bytes += 8 * rows * row_len + rows * nb * (cb + 1) + (4 * rows * row_len // it.khw
                                                                           if it.esum is not None else 0)
        self._tab = np.array(tab, dtype=mx._MX)
        self._descs = self._tab.ctypes.data_as(C.POINTER(_lib.MxDesc))
        self._n = len(items)
        nb_ws = int(self._lib.dfq_mx_quantize_ws_bytes(self._descs, self._n))
        assert nb_ws > 0
        self._ws = share._ws if share is not None else torch.empty(nb_ws, dtype=torch.uint8, device=dev)
        assert self._ws.numel() >= nb_ws
        self.ws_bytes = nb_ws

    def run(self, stream, lib=None, search=False):
        """The call, through this process's library or another build of it (same buffers);
        ``search``: dfq_mx_quantize_search_batch on the same table."""
        name = "dfq_mx_quantize_search_batch" if search else "dfq_mx_quantize_batch"
        _lib.check(getattr(lib or self._lib, name)(self._descs, self._n, self._ws.data_ptr(), self._ws.numel(),
                                                   C.c_void_p(stream.cuda_stream)), name)


def bench_list(args):
    """The bench headline's sweep items on the GPU and what describes them."""
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
    return dev, b, shapes, per_copy, copies, symmetric, items


def timing(args):
    dev, b, shapes, per_copy, copies, symmetric, items = bench_list(args)
    plan = bench._plan_of(items)
    stream = torch.cuda.current_stream(dev)
    calls = {"mxfp8": MxCall(items, "mxfp8")}   # the largest codes: every format writes into its arenas
    calls.update({fmt: MxCall(items, fmt, share=calls["mxfp8"]) for fmt in mx.FORMATS if fmt != "mxfp8"})
    ones = {"mxfp8": MxCall(items[:len(shapes)], "mxfp8")}
    ones.update({fmt: MxCall(items[:len(shapes)], fmt, share=ones["mxfp8"]) for fmt in mx.FORMATS if fmt != "mxfp8"})
    one_plan = bench._plan_of(items[:len(shapes)])
    legs = []
    for _ in range(3):
        leg = {"sweep_ms": round(timed(lambda: plan.execute(stream), stream, args.warmup, args.steps), 4)}
        for fmt in mx.FORMATS:
            leg[fmt + "_ms"] = round(timed(lambda: calls[fmt].run(stream), stream, args.warmup, args.steps), 4)
        legs.append(leg)
    frac = lambda nbytes, ms: round(nbytes / ms / 1e6 / bench.HBM_PEAK_GBS, 4)   # noqa: E731
    sweep_ms = statistics.median(leg["sweep_ms"] for leg in legs)
    out = {"what": "dfq_mx_quantize_batch (dst + codes + scales + esum) on the bench headline list, beside the sweep",
           "device": torch.cuda.get_device_name(dev), "model": b.model, "copies": copies, "tensors": len(items),
           "elements": per_copy * copies, "warmup": args.warmup, "steps": args.steps, "legs": legs,
           "sweep": {"bits": b.bits, "granularity": b.granularity, "symmetric": symmetric, "ms": sweep_ms,
                     "algo_bytes": plan.stats["algo_bytes"], "launches": plan.stats["launches"],
                     "frac_of_peak": frac(plan.stats["algo_bytes"], sweep_ms),
                     "one_model_us": round(1e3 * timed(lambda: one_plan.execute(stream), stream, args.warmup,
                                                       args.steps), 2)}}
    for fmt in mx.FORMATS:
        ms = statistics.median(leg[fmt + "_ms"] for leg in legs)
        c = calls[fmt]
        out[fmt] = {"ms": ms, "algo_bytes": c.algo_bytes, "frac_of_peak": frac(c.algo_bytes, ms),
                    "bytes_per_element": round(c.algo_bytes / (per_copy * copies), 4),
                    "ratio_to_sweep_ms": round(ms / sweep_ms, 3), "table_bytes": c.ws_bytes,
                    "one_model_us": round(1e3 * timed(lambda: ones[fmt].run(stream), stream, args.warmup, args.steps), 2)}
    torch.cuda.synchronize()
    emit([out], Path(args.out) if args.out else OUT / "mx6_quantize_time.jsonl")


def parent_ab(args):
    """MXFP4 and MXFP8 on the bench list through two builds of the library in one
    process: --ab's (the parent commit's, built into a scratch directory) and this
    tree's, alternated three times, both on the same descriptor table, outputs and
    workspace (where the buffers lie moves a call by more than the builds differ).  The
    formats the other build lacks are not timed."""
    dev, b, shapes, per_copy, copies, symmetric, items = bench_list(args)
    stream = torch.cuda.current_stream(dev)
    # the one entry it is timed through, typed here: another commit's build need not export
    # everything this tree's binding asks for (its kernel's code object loads in the first leg's warm-up)
    other = C.CDLL(str(Path(args.ab).resolve()))
    mine = _lib.load().dfq_mx_quantize_batch
    other.dfq_mx_quantize_batch.argtypes, other.dfq_mx_quantize_batch.restype = mine.argtypes, mine.restype
    fmts = ("mxfp4", "mxfp8")
    calls = {fmt: MxCall(items, fmt) for fmt in fmts}
    libs = {"parent": other, "new": _lib.load()}
    legs = []
    for _ in range(3):
        leg = {}
        for fmt in fmts:
            for who in ("parent", "new"):
                leg["%s_%s_ms" % (who, fmt)] = round(timed(lambda: calls[fmt].run(stream, libs[who]), stream, args.warmup,
                                                           args.steps), 4)
        legs.append(leg)
    out = {"what": "dfq_mx_quantize_batch (dst + codes + scales + esum) on the bench headline list: the parent commit's "
                   "library against this tree's, alternated in one process",
           "device": torch.cuda.get_device_name(dev), "model": b.model, "copies": copies, "tensors": len(items),
           "warmup": args.warmup, "steps": args.steps, "legs": legs}
    for fmt in fmts:
        old = [leg["parent_%s_ms" % fmt] for leg in legs]
        new = [leg["new_%s_ms" % fmt] for leg in legs]
        out[fmt] = {"parent_ms": old, "new_ms": new, "parent_min": min(old), "parent_max": max(old),
                    "new_within_parent_spread": all(t <= max(old) for t in new)}
    torch.cuda.synchronize()
    emit([out], Path(args.out) if args.out else OUT / "mx6_parent_ab.jsonl")


def search_timing(args):
    """dfq_mx_quantize_search_batch against dfq_mx_quantize_batch on the bench list: the same
    descriptor table, outputs and workspace, the two calls alternated three times per format
    in one process.  The source is restored before every leg from a copy (dst is the source:
    a second call over searched values would time other data)."""
    dev, b, shapes, per_copy, copies, symmetric, items = bench_list(args)
    stream = torch.cuda.current_stream(dev)
    calls = {"mxfp8": MxCall(items, "mxfp8")}
    calls.update({fmt: MxCall(items, fmt, share=calls["mxfp8"]) for fmt in mx.FORMATS if fmt != "mxfp8"})
    aliased = all(it.dst.data_ptr() == it.src.data_ptr() for it in items)
    keep = [it.src.clone() for it in items] if aliased else None

    def restore():
        if keep is not None:
            torch._foreach_copy_([it.src for it in items], keep)

    legs = []
    for _ in range(3):
        leg = {}
        for fmt in mx.FORMATS:
            for who, search in (("floor", False), ("search", True)):
                restore()
                leg["%s_%s_ms" % (who, fmt)] = round(timed(lambda: calls[fmt].run(stream, search=search), stream,
                                                           args.warmup, args.steps), 4)
        legs.append(leg)
    out = {"what": "dfq_mx_quantize_search_batch against dfq_mx_quantize_batch (dst + codes + scales + esum) on the bench "
                   "headline list, alternated in one process",
           "device": torch.cuda.get_device_name(dev), "model": b.model, "copies": copies, "tensors": len(items),
           "elements": per_copy * copies, "dst_aliases_src": aliased, "warmup": args.warmup, "steps": args.steps,
           "legs": legs}
    frac = lambda nbytes, ms: round(nbytes / ms / 1e6 / bench.HBM_PEAK_GBS, 4)   # noqa: E731
    for fmt in mx.FORMATS:
        f = statistics.median(leg["floor_%s_ms" % fmt] for leg in legs)
        t = statistics.median(leg["search_%s_ms" % fmt] for leg in legs)
        out[fmt] = {"floor_ms": f, "search_ms": t, "ratio": round(t / f, 3), "algo_bytes": calls[fmt].algo_bytes,
                    "floor_frac_of_peak": frac(calls[fmt].algo_bytes, f), "search_frac_of_peak": frac(calls[fmt].algo_bytes, t)}
    torch.cuda.synchronize()
    emit([out], Path(args.out) if args.out else OUT_SEARCH / "mx_search_time.jsonl")


def matmul_logits_record(fmt, search):
    """Logits SQNR of the zoo's MobileNetV2 (seed 0, batch 2 at 32 x 32, fixed observers) with its
    eligible products on the matrix instruction (MXFP8 activations) against its plain forward."""
    import torch.nn as nn
    from data_free_quantization_amd import pipeline, zoo
    from data_free_quantization_amd.utils import layer_transform as L
    from data_free_quantization_amd.utils.quantize import QuantConv2d, QuantLinear, frozen_weights, mx_matmul_forward
    from data_free_quantization_amd.utils.tracer import TorchTransformer
    torch.manual_seed(0)
    model = zoo.build("mobilenetv2", seed=0, relu=True).cuda().eval()
    x = torch.randn(2, 3, 32, 32, device="cuda")
    tr = TorchTransformer("positional")
    model, tr = L.switch_layers(model, tr, x, {1: [(nn.Conv2d, QuantConv2d), (nn.Linear, QuantLinear)]})
    graph, bottoms = tr.log.getGraph(), tr.log.getBottoms()
    try:
        pipeline.run_dfq(model, graph, bottoms, (QuantConv2d, QuantLinear), weight_format=fmt, bc_mode="fused", clip=False,
                         **({"mx_scale_search": True} if search else {}))
        L.set_quant_minmax(graph, bottoms, verbose=False)
        model.eval()
        for m in graph.values():
            if hasattr(m, "quant"):
                m.quant.update_stat = False
        for q in L.module_tensor_op.quants:
            q.update_stat = False
        L.replace_op()
        try:
            with torch.no_grad(), frozen_weights():
                plain = model(x)
                with mx_matmul_forward("mxfp8"):
                    routed = model(x)
                    calls = mx.LINEAR_CALLS
        finally:
            L.restore_op()
    finally:
        L.module_tensor_op = None
    noise = float((routed.double() - plain.double()).pow(2).sum())
    return {"what": "logits of --mx_matmul mxfp8 against the plain forward", "weight_format": fmt, "mx_scale_search": search,
            "layers_routed": calls, "logits_sqnr_db": round(10 * np.log10(float(plain.double().pow(2).sum()) / noise), 3)}


def search_quality_records(args):
    """Model SQNR of the zoo's MobileNetV2 (seed 0) from main_dfq --relu --equalize --absorption
    --quantize --weight_format F --report, with and without --mx_scale_search, and the blocks
    the search raised; then matmul_logits_record for MXFP8 weights.  Data, not assertions."""
    import tempfile
    from data_free_quantization_amd import main_dfq
    records = []
    with tempfile.TemporaryDirectory() as tmp:
        for fmt in ("mxfp4", "mxfp6_e3m2", "mxfp6_e2m3", "mxfp8"):
            for search in (False, True):
                path = Path(tmp) / "report.json"
                argv = ["--relu", "--equalize", "--absorption", "--quantize", "--weight_format", fmt] + \
                    (["--mx_scale_search"] if search else []) + ["--report", str(path)]
                main_dfq.main(argv)
                rep = json.loads(path.read_text())
                m = rep["model"]
                records.append({"argv": " ".join(argv[:-2]), "weight_format": fmt, "mx_scale_search": search,
                                "model_sqnr_db": round(m["sqnr_db"], 3), "worst_layer": m["worst_layer"],
                                "worst_channel_sqnr_db": round(min(e["worst_channel_sqnr_db"] for e in rep["layers"]), 3),
                                **({"scale_raised": sum(e["scale_raised"] for e in rep["layers"]),
                                    "blocks": sum(e["shape"][0] * -(-(e["elements"] // e["shape"][0]) // 32)
                                                  for e in rep["layers"])} if search else {})})
    records += [matmul_logits_record("mxfp8", False), matmul_logits_record("mxfp8", True)]
    emit(records, Path(args.out) if args.out else OUT_SEARCH / "quality_mx_search.jsonl")


def quality_records(args):
    """Model SQNR of the zoo's MobileNetV2 (seed 0) from main_dfq --relu [--equalize
    --absorption] --quantize --report: every MX format beside per-channel symmetric
    INT4 / INT8, with and without equalization.  One JSON line each: data, not
    assertions."""
    import tempfile
    from data_free_quantization_amd import main_dfq
    records = []
    with tempfile.TemporaryDirectory() as tmp:
        for equalize in (True, False):
            for fmt, extra in (("mxfp4", []), ("mxfp6_e3m2", []), ("mxfp6_e2m3", []), ("mxfp8", []),
                               ("int", ["--bits_weight", "4", "--granularity", "channel", "--symmetric"]),
                               ("int", ["--bits_weight", "8", "--granularity", "channel", "--symmetric"])):
                path = Path(tmp) / "report.json"
                argv = ["--relu"] + (["--equalize", "--absorption"] if equalize else []) + \
                    ["--quantize", "--weight_format", fmt, "--report", str(path)] + extra
                main_dfq.main(argv)
                rep = json.loads(path.read_text())
                m, cfg = rep["model"], rep["config"]
                records.append({"argv": " ".join(argv[:-2 - len(extra)] + extra), "weight_format": fmt,
                                "bits_per_weight": cfg.get("bits_per_weight", cfg["bits_weight"]), "equalize": equalize,
                                "model_sqnr_db": round(m["sqnr_db"], 3), "worst_layer": m["worst_layer"],
                                "worst_channel_sqnr_db": round(min(e["worst_channel_sqnr_db"] for e in rep["layers"]), 3)})
    emit(records, Path(args.out) if args.out else OUT / "quality_mx6.jsonl")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=0, help="weight sets (0: the bench's, >= 2 GiB)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--ab", default=None, help="another build of libdfq_hip.so to time MXFP4 / MXFP8 against")
    ap.add_argument("--search", action="store_true", help="time the searched call against the floor call")
    ap.add_argument("--search_quality", action="store_true", help="model SQNR with and without --mx_scale_search")
    ap.add_argument("--out", default=None, help="the JSON lines' file (default: under profiles/r10 or r12)")
    a = ap.parse_args()
    if a.search or a.search_quality:
        search_quality_records(a) if a.search_quality else search_timing(a)
    else:
        quality_records(a) if a.quality else parent_ab(a) if a.ab else timing(a)
