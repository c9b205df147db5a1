"""mx.mx_quantize(scale_search=True) (dfq_mx_quantize_search_batch) on the GPU against the
numpy statement of tests/mx_search_cases.py, and the option through mx_linear, the pipeline,
the report and the forward on the matrix instruction.

Every comparison is for equality.  A block's codes, scale byte and values must be those of
one candidate, wholly: the statement's choice where the two noises differ by more than the
fp32 margin, X0 where the candidates are equal element for element, either one for the blocks
the statement calls undecided -- which the test counts, so that a block outside that set
cannot pass as one.  The error sums are those of the values the device chose.  Every output
buffer is followed (the codes also preceded) by guard words that must come back untouched."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import mx_search_cases as SC
from tests.mx_gpu_util import GB, GF, GUARD, as_bytes as _bytes, run

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _linear_calls_back_at_zero():
    """mx.LINEAR_CALLS counts since the last reset, and tests that run later read it: leave none behind."""
    yield
    from data_free_quantization_amd import mx
    mx.reset_linear_calls()


def _run(cases, scale_search=True):
    """One call over ``cases``, searched unless told otherwise; every buffer back on the host, guards included."""
    return run(cases, scale_search=scale_search)


def _check(c, out, ref=None):
    """The case against its statement (``ref``: another statement of the same data).  Returns
    (undecided blocks the device chose the other way, undecided blocks, the y the device chose)."""
    r = ref if ref is not None else c.ref
    rows, row_len = c.x.shape
    n, off = c.x.size, c.offset
    nb, cb, co = SC.blocks(row_len), SC.FORMATS[c.fmt][3], c.code_offset
    assert set(out) == {"src"} | ({"dst"} if c.want_dst else set()) | \
        ({"codes", "scales"} if c.want_codes else set()) | ({"esum"} if c.want_esum else set()), c.name
    match = [np.ones((rows, nb), bool), np.ones((rows, nb), bool)]   # the block is candidate d in every output
    if c.want_codes:
        codes = out["codes"][co:co + rows * nb * cb].reshape(rows, nb, cb)
        scales = out["scales"][:rows * nb].reshape(rows, nb)
        for d in (0, 1):
            match[d] &= (codes == r["cand"][d]["codes"]).all(axis=2) & (scales == r["cand"][d]["scales"])
        assert (out["codes"][:co] == GB).all() and (out["codes"][co + rows * nb * cb:] == GB).all(), c.name
        assert (out["scales"][rows * nb:] == GB).all(), c.name
    if c.want_dst:
        yb = np.zeros((rows, nb * SC.BLOCK), np.float32)
        yb[:, :row_len] = out["dst"][off:off + n].reshape(c.x.shape)
        pad = np.zeros((rows, nb * SC.BLOCK), bool)
        pad[:, row_len:] = True   # dst has no padding: it matches there
        for d in (0, 1):
            same = (yb.view(np.uint32) == r["cand"][d]["yb"].reshape(rows, -1).view(np.uint32)) | pad
            match[d] &= same.reshape(rows, nb, SC.BLOCK).all(axis=2)
        assert (out["dst"][:off] == GF).all() and (out["dst"][off + n:] == GF).all(), c.name
    tw, und, take1 = r["termwise_equal"], r["undecided"], r["take1"]
    # match[d] is over every output, so a block that passes is wholly one candidate.  Termwise-equal
    # candidates differ in codes and scale byte, never in y: X0 (both match where only dst is written)
    ok = np.where(tw, match[0], np.where(und, match[0] | match[1], np.where(take1, match[1], match[0])))
    assert ok.all(), (c.name, np.argwhere(~ok)[:4].tolist())
    chose1 = match[1] & ~match[0]
    y = np.where(chose1[:, :, None], r["cand"][1]["yb"], r["cand"][0]["yb"]).reshape(rows, -1)[:, :row_len].copy()
    if c.outputs != "inplace":   # the source is only read
        assert np.array_equal(out["src"][off:off + n].view(np.uint32), c.x.reshape(-1).view(np.uint32)), c.name
        assert (out["src"][:off] == GF).all() and (out["src"][off + n:] == GF).all(), c.name
    if c.want_esum:
        ne = n // c.khw
        assert np.array_equal(out["esum"][:ne], SC.esum_of(c, y)), c.name
        assert (out["esum"][ne:] == GF).all(), c.name
    return int((und & (chose1 != take1)).sum()), int(und.sum()), y


def _mixed(cases):
    """A searched list that mixes FP4, FP6 and FP8 tensors, each tensor at most once."""
    by = {fmt: [c for c in cases if c.fmt == fmt] for fmt in SC.FORMATS}
    out = []
    for i in range(30):
        out += [by[fmt][(7 * i + j) % len(by[fmt])] for j, fmt in enumerate(SC.FORMATS)]
    out = list({c.name: c for c in out}.values())
    assert {c.fmt for c in out} == set(SC.FORMATS) and any(c.khw > 1 and c.want_esum for c in out)
    return out


@pytest.fixture(scope="module")
def world():
    cases = SC.all_cases()
    mixed = _mixed(cases)
    return {"cases": cases, "together": _run(cases), "again": _run(cases), "mixed": mixed, "mixed_out": _run(mixed),
            "alone": {c.name: _run([c])[0] for c in mixed}}


def test_every_block_is_one_candidate_and_the_right_one(world):
    flipped = undecided = blocks = 0
    for c, out in zip(world["cases"], world["together"]):
        f, u, _ = _check(c, out)
        flipped, undecided, blocks = flipped + f, undecided + u, blocks + c.ref["take1"].size
    print("%d blocks, %d undecided in the statement, %d of them chosen the other way by the device"
          % (blocks, undecided, flipped))
    assert undecided <= SC.UNDECIDED_CAP * blocks and flipped <= undecided


def test_the_same_bytes_again_alone_and_in_a_mixed_list(world):
    for i, c in enumerate(world["cases"]):
        assert _bytes(world["again"][i]) == _bytes(world["together"][i]), c.name
    index = {c.name: i for i, c in enumerate(world["cases"])}
    for c, out in zip(world["mixed"], world["mixed_out"]):
        want = _bytes(world["together"][index[c.name]])
        assert _bytes(out) == want, c.name
        assert _bytes(world["alone"][c.name]) == want, c.name


def test_the_same_result_aliased_or_not_and_at_every_offset(world):
    """The data of cases of each format run again with dst aliasing src and apart, 0 / 1 / 3
    floats from a 16-B boundary (the 16-B and the 4-B path): one result, bit for bit."""
    picks = []
    for fmt in SC.FORMATS:
        mine = [c for c in world["cases"] if c.fmt == fmt and c.x.shape[1] % 4 == 0 and c.x.shape[1] >= 64]
        picks += [mine[0], mine[len(mine) // 2], next(c for c in mine if c.khw > 1 and c.want_esum),
                  next(c for c in mine if c.name.startswith("band_"))]
    variants = []
    for c in picks:
        for off in (0, 1, 3):
            for outputs in ("all", "inplace"):
                variants.append(SC.Case("%s@%d_%s" % (c.name, off, outputs), c.x, c.fmt, c.khw, off, outputs,
                                        code_offset=0, ref=c.ref))
    outs = _run(variants)
    for k in range(0, len(variants), 6):
        base = variants[k]
        n, first = base.x.size, None
        for c, out in zip(variants[k:k + 6], outs[k:k + 6]):
            _check(c, out)
            got = {"dst": out["dst"][c.offset:c.offset + n].tobytes(), "codes": out["codes"][:-GUARD].tobytes(),
                   "scales": out["scales"][:-GUARD].tobytes(), "esum": out["esum"][:-GUARD].tobytes() if c.want_esum else b""}
            first = first or got
            assert got == first, c.name


def test_the_unsearched_call_is_still_the_floor_rule(world):
    """mx_quantize(scale_search=False) beside the new entry: the floor statement, bit for bit."""
    cases = [next(c for c in world["cases"] if c.name == n)
             for n in ("band_mxfp4", "mx6_ties_sat_mxfp6_e3m2", "requant_mxfp8", "mx_khw9_2x4608_mxfp8")]
    moved = 0
    for c, out in zip(cases, _run(cases, scale_search=False)):
        floor = SC.statement(c.x, c.fmt, search=False)
        rows, nb = floor["scales"].shape
        assert np.array_equal(out["codes"][c.code_offset:-GUARD].reshape(floor["codes"].shape), floor["codes"]), c.name
        assert np.array_equal(out["scales"][:-GUARD].reshape(rows, nb), floor["scales"]), c.name
        y = out["dst"][c.offset:c.offset + c.x.size].reshape(c.x.shape)
        assert np.array_equal(y.view(np.uint32), floor["y"].view(np.uint32)), c.name
        moved += int(c.ref["take1"].sum())
    assert moved > 20   # the search would have answered otherwise


def test_requantizing_the_devices_values_with_the_search_returns_them(world):
    """mx_quantize(y, scale_search=True).dst == y in all four formats (the stored grid has
    no noise), whatever scale byte the second pass settles on."""
    again = []
    for c, out in zip(world["cases"], world["together"]):
        if c.outputs != "all" or c.khw != 1:
            continue
        y = out["dst"][c.offset:c.offset + c.x.size].reshape(c.x.shape).copy()
        again.append(SC.Case("again_" + c.name, y, c.fmt, 1, c.offset, "nocodes"))
    assert {c.fmt for c in again} == set(SC.FORMATS) and len(again) > 40
    for c, out in zip(again, _run(again)):
        got = out["dst"][c.offset:c.offset + c.x.size].reshape(c.x.shape)
        assert np.array_equal(got.view(np.uint32), c.x.view(np.uint32)), c.name
        assert not out["esum"][:c.x.size].any(), c.name


def test_mx_linear_needs_the_search_for_a_searched_mxfp8_weight():
    """A searched MXFP8 weight [40, 96] (its first rows the crafted 1.875-mantissa blocks)
    times activations [32, 96]: with weight_scale_search the product is mx_gemm's on the
    stored codes, bit for bit; without it the crafted rows' outputs differ (480 * 2^k
    saturates to 448 * 2^k under the floor rule)."""
    from data_free_quantization_amd import mx
    rng = np.random.default_rng(5)
    w = (0.05 * rng.standard_normal((40, 96))).astype(np.float32)
    crafted = next(c for c in SC.all_cases() if c.name == "requant_mxfp8")
    w[:3] = crafted.x
    x = torch.from_numpy(rng.standard_normal((32, 96)).astype(np.float32)).to(DEV)
    wi = mx.mx_quantize([mx.allocate(torch.from_numpy(w).to(DEV), "mxfp8")], scale_search=True)[0]
    ref = SC.statement(w, "mxfp8")
    assert not ref["undecided"].any() and ref["take1"][:3].all()
    assert np.array_equal(wi.dst.cpu().numpy().view(np.uint32), ref["y"].view(np.uint32))
    assert np.array_equal(wi.codes.cpu().numpy(), ref["codes"]) and np.array_equal(wi.scales.cpu().numpy(), ref["scales"])
    xi = mx.mx_quantize([mx.allocate(x, "mxfp8", want_dst=False)])[0]   # the activations keep the floor rule
    want = mx.mx_gemm(xi.codes, xi.scales, "mxfp8", wi.codes, wi.scales, "mxfp8", 96)
    got = mx.mx_linear(x, wi.dst, None, "mxfp8", "mxfp8", weight_scale_search=True)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    floor = mx.mx_linear(x, wi.dst, None, "mxfp8", "mxfp8")
    assert not torch.equal(floor[:, :3], want[:, :3])   # the finding, pinned
    kept = mx.mx_linear(x, wi.dst, None, "mxfp8", "mxfp8", weight_mx=(wi.codes, wi.scales))
    assert torch.equal(kept, want)


# ---- the pipeline ---------------------------------------------------------------
def _plain_run(**kw):
    from data_free_quantization_amd import zoo
    from data_free_quantization_amd.pipeline import run_dfq
    from data_free_quantization_amd.utils.tracer import build_graph
    targ = (nn.Conv2d, nn.Linear)
    model = zoo.build("mobilenetv2", seed=0, relu=True).cuda()
    g = build_graph(model, "positional")
    graph, bottoms = g.getGraph(), g.getBottoms()
    rep = {}
    run_dfq(model, graph, bottoms, targ, bc_mode="fused", clip=False, report=rep, **kw)
    torch.cuda.synchronize()
    return graph, rep


def test_quantize_targ_layer_marks_the_layers_and_keeps_dequantizable_codes(tmp_path):
    from data_free_quantization_amd import export, mx, zoo
    from data_free_quantization_amd.utils.layer_transform import merge_batchnorm, quantize_targ_layer
    from data_free_quantization_amd.utils.tracer import build_graph
    targ = (nn.Conv2d, nn.Linear)
    model = zoo.build("mobilenetv2", seed=0, relu=True).cuda()
    g = build_graph(model, "positional")
    graph, bottoms = g.getGraph(), g.getBottoms()
    merge_batchnorm(model, graph, bottoms, targ)
    before = {k: graph[k].weight.detach().clone() for k in graph if type(graph[k]) in targ}
    state = {}
    quantize_targ_layer(graph, 8, 8, targ, state=state, weight_format="mxfp4", mx_scale_search=True)
    torch.cuda.synchronize()
    assert len(state) == 53
    raised = 0
    for k, st in state.items():
        layer, w = graph[k], graph[k].weight.detach()
        assert layer.weight_format == "mxfp4" and layer.mx_scale_search is True, k
        assert set(st) == {"codes", "scales", "esum", "khw", "format", "scale_search"} and st["scale_search"] is True
        y = mx.mx_dequantize(st["codes"], st["scales"], w.shape, "mxfp4")
        assert torch.equal(y.view(torch.int32), w.view(torch.int32)), k
        floor = mx.floor_scale_bytes(before[k], "mxfp4")
        assert ((st["scales"] == floor) | (st["scales"] == floor + 1)).all(), k
        raised += int((st["scales"] > floor).sum())
    assert raised > 0
    # one layer against the statement
    k = next(k for k in state if before[k][0].numel() >= 64)
    x = before[k].cpu().numpy().reshape(before[k].shape[0], -1)
    ref = SC.statement(x, "mxfp4")
    sure = ~ref["undecided"]
    assert np.array_equal(state[k]["scales"].cpu().numpy()[sure], ref["scales"][sure])
    path = tmp_path / "w.safetensors"
    export.save(path, graph, state, bits=8, granularity="tensor", symmetric=False, weight_format="mxfp4",
                mx_scale_search=True)
    meta, entries = export.load(path)
    assert meta["mx_scale_search"] is True and meta["weight_format"] == "mxfp4"
    for k in state:
        y = export.dequantize(meta, str(k), entries[str(k)])
        assert torch.equal(y.view(torch.int32), graph[k].weight.detach().cpu().view(torch.int32)), k
    # a pass without the option takes the mark away and leaves no key; so does an integer pass
    state2 = {}
    quantize_targ_layer(graph, 8, 8, targ, state=state2, weight_format="mxfp4")
    assert all("mx_scale_search" not in graph[k].__dict__ and "scale_search" not in state2[k] for k in state2)
    quantize_targ_layer(graph, 8, 8, targ, weight_format="mxfp4", mx_scale_search=True)
    quantize_targ_layer(graph, 8, 8, targ)
    assert all("mx_scale_search" not in graph[k].__dict__ and "weight_format" not in graph[k].__dict__ for k in state)


def test_the_report_counts_the_raised_scales_and_no_layer_gets_noisier():
    _, plain = _plain_run(weight_format="mxfp4")
    _, searched = _plain_run(weight_format="mxfp4", mx_scale_search=True)
    assert searched["config"]["mx_scale_search"] is True and "mx_scale_search" not in plain["config"]
    assert all("scale_raised" not in e for e in plain["layers"])
    assert len(searched["layers"]) == len(plain["layers"]) == 53
    total = 0
    for a, b in zip(plain["layers"], searched["layers"]):
        assert a["key"] == b["key"] and a["shape"] == b["shape"]
        assert isinstance(b["scale_raised"], int) and 0 <= b["scale_raised"] <= b["shape"][0] * -(-(b["elements"] // b["shape"][0]) // 32)
        # undecided blocks can move a layer's noise by no more than 2^-16 relative
        assert b["sqnr_db"] >= a["sqnr_db"] - 0.01, (a["key"], a["sqnr_db"], b["sqnr_db"])
        total += b["scale_raised"]
    assert total > 0
    print("MobileNetV2 mxfp4 model SQNR %.2f dB -> %.2f dB with the scale search, %d blocks raised"
          % (plain["model"]["sqnr_db"], searched["model"]["sqnr_db"], total))
    assert searched["model"]["sqnr_db"] >= plain["model"]["sqnr_db"] - 0.01


def test_the_forward_on_the_matrix_instruction_multiplies_the_stored_values():
    """run_dfq(weight_format="mxfp8", mx_scale_search=True) on the zoo's MobileNetV2 with Quant*
    layers: inside mx_matmul_forward the marked layers re-quantize their weights with the
    search, so frozen_weights() keeps codes that stand for the stored values and the logits are
    those of the stored codes, bit for bit."""
    from data_free_quantization_amd import mx, pipeline, zoo
    from data_free_quantization_amd.utils import layer_transform as L
    from data_free_quantization_amd.utils.quantize import QuantConv2d, QuantLinear, frozen_weights, mx_matmul_forward
    from data_free_quantization_amd.utils.tracer import TorchTransformer
    fmt = "mxfp8"   # the format in which the floor rule does not give the weights back
    model = zoo.build("mobilenetv2", seed=0, relu=True).to(DEV).eval()
    x = torch.randn(2, 3, 32, 32, device=DEV)
    tr = TorchTransformer("positional")
    model, tr = L.switch_layers(model, tr, x, {1: [(nn.Conv2d, QuantConv2d), (nn.Linear, QuantLinear)]})
    graph, bottoms = tr.log.getGraph(), tr.log.getBottoms()
    targ = (QuantConv2d, QuantLinear)
    captured = {}
    real = pipeline.quantize_targ_layer

    def spy(*a, **k):
        captured["state"] = k.get("state")
        return real(*a, **k)

    pipeline.quantize_targ_layer = spy
    try:
        pipeline.run_dfq(model, graph, bottoms, targ, weight_format=fmt, mx_scale_search=True, bc_mode="fused", clip=False)
    finally:
        pipeline.quantize_targ_layer = real
    state = captured["state"]
    try:
        L.set_quant_minmax(graph, bottoms, verbose=False)
        model.eval()
        for m in graph.values():   # fixed observers, so every forward sees the same ranges
            if hasattr(m, "quant"):
                m.quant.update_stat = False
        for q in L.module_tensor_op.quants:
            q.update_stat = False
        eligible = {k: m for k, m in graph.items()
                    if isinstance(m, QuantLinear) or (isinstance(m, QuantConv2d) and tuple(m.kernel_size) == (1, 1) and
                                                      m.groups == 1 and tuple(m.padding) == (0, 0))}
        assert len(eligible) > 30 and all(m.weight_format == fmt and m.mx_scale_search for m in eligible.values())
        L.replace_op()
        try:
            with torch.no_grad(), mx_matmul_forward("mxfp8"):
                free = model(x)
                with frozen_weights():
                    first = model(x)
                    differ = 0
                    for k, m in eligible.items():
                        key, codes, scales = m.__dict__["_mx_w_cache"]
                        w = m.weight.detach().reshape(m.weight.shape[0], -1)
                        assert torch.equal(mx.mx_dequantize(codes, scales, w.shape, fmt).view(torch.int32), w.view(torch.int32)), k
                        st = state[k]
                        assert torch.equal(mx.mx_dequantize(st["codes"], st["scales"], w.shape, fmt).view(torch.int32),
                                           w.view(torch.int32)), k
                        differ += int((st["scales"] != scales).sum())
                        m.__dict__["_mx_w_cache"] = (key, st["codes"], st["scales"])   # the stored codes, same key
                    stored = model(x)
                    assert all(m.__dict__["_mx_w_cache"][1] is state[k]["codes"] for k, m in eligible.items())
                # what the floor rule would have multiplied: not the stored values
                lost = 0
                for k, m in eligible.items():
                    w = m.weight.detach().reshape(m.weight.shape[0], -1).contiguous()
                    again = mx.mx_quantize([mx.allocate(w, fmt)])[0]
                    lost += int((again.dst != w).sum())
        finally:
            L.restore_op()
    finally:
        L.module_tensor_op = None
    assert torch.isfinite(first).all()
    assert torch.equal(free, first) and torch.equal(first, stored)
    assert lost > 0
    print("%d eligible layers; %d scale bytes differ between the stored and the re-quantized codes; the floor rule "
          "would have changed %d weights" % (len(eligible), differ, lost))
