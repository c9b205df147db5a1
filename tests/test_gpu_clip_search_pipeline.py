"""The clip-range search through pipeline.run_dfq(clip_search=...) and
main_dfq --clip_search: stage order, the report's new fields, and every channel's
noise against the same run without the search (bound as in
tests/test_gpu_clip_search.py: two fp64 sums of the same n non-negative terms
differ by at most n 2^-52, relative)."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import clip_search_cases as CC

pytestmark = pytest.mark.gpu
TARG = (nn.Conv2d, nn.Linear)
GOLDEN = Path(__file__).resolve().parent / "golden" / "quality_report_mobilenetv2_w8.json"

FLAGS = ["--task", "cls", "--relu", "--equalize", "--absorption", "--quantize", "--correction", "--clip_weight",
         "--bits_weight", "8", "--bits_activation", "8", "--bits_bias", "8"]
W4 = {"bits_weight": 4, "granularity": "channel", "symmetric": True}


def _run(report, **kw):
    from data_free_quantization_amd import quality, zoo
    from data_free_quantization_amd.pipeline import run_dfq
    from data_free_quantization_amd.utils.tracer import build_graph
    model = zoo.build("mobilenetv2", seed=0, relu=True).cuda()
    g = build_graph(model, "positional")
    graph, bottoms = g.getGraph(), g.getBottoms()
    tkeys = [k for k in graph if type(graph[k]) in TARG]
    before, stages = {}, []

    def hook(stage):
        stages.append(stage)
        if stage == "bn2":
            for k in tkeys:
                before[k] = graph[k].weight.detach().clone()

    run_dfq(model, graph, bottoms, TARG, stage_hook=hook, report=report, **kw)
    stats = quality.pair_stats([(before[k], graph[k].weight.detach()) for k in tkeys])
    torch.cuda.synchronize()
    noise = {k: s.rows[:, quality.NOISE].cpu().numpy() for k, s in zip(tkeys, stats)}
    return tkeys, stages, before, noise


@pytest.fixture(scope="module")
def runs():
    rep0, rep1 = {}, {}
    tkeys, stages0, before0, noise0 = _run(rep0, **W4)
    _, stages1, before1, noise1 = _run(rep1, clip_search={"candidates": 16, "min_frac": 0.5}, **W4)
    return {"tkeys": tkeys, "rep0": rep0, "rep1": rep1, "stages0": stages0, "stages1": stages1,
            "before0": before0, "before1": before1, "noise0": noise0, "noise1": noise1}


def test_stage_order_and_report_fields(runs):
    s0, s1 = runs["stages0"], runs["stages1"]
    assert "clipsearch" not in s0
    assert s1 == s0[:s0.index("quant")] + ["clipsearch"] + s0[s0.index("quant"):]
    assert s1[s1.index("clipsearch") - 1] == "bn2" and s1[s1.index("clipsearch") + 1] == "quant"
    c0, c1 = runs["rep0"]["config"], runs["rep1"]["config"]
    assert (c1["clip_search"], c1["clip_candidates"], c1["clip_min_frac"]) == (True, 16, 0.5)
    assert {k: v for k, v in c1.items() if not k.startswith("clip_search") and k not in
            ("clip_candidates", "clip_min_frac")} == c0
    for e0, e1, k in zip(runs["rep0"]["layers"], runs["rep1"]["layers"], runs["tkeys"]):
        assert not any(f.startswith("clip_") for f in e0), e0["key"]
        assert e1["clip_units"] == e1["shape"][0]
        assert 0 <= e1["clip_at_edge"] <= e1["clip_narrowed"] <= e1["clip_units"], e1["key"]
        # a narrowed unit is a channel whose noise changed (or, rarely, one whose narrower clamp rounds the same)
        assert int((runs["noise1"][k] != runs["noise0"][k]).sum()) <= e1["clip_narrowed"], e1["key"]
    total = sum(e["clip_units"] for e in runs["rep1"]["layers"])
    narrowed = sum(e["clip_narrowed"] for e in runs["rep1"]["layers"])
    print("MobileNetV2 W4 per channel: %d of %d channels narrowed, %d at the grid edge; model SQNR %.3f -> %.3f dB"
          % (narrowed, total, sum(e["clip_at_edge"] for e in runs["rep1"]["layers"]),
             runs["rep0"]["model"]["sqnr_db"], runs["rep1"]["model"]["sqnr_db"]))
    json.loads(json.dumps(runs["rep1"], allow_nan=False))


def test_no_channel_gets_noisier(runs):
    for k in runs["tkeys"]:
        # the search starts from the same weights in both runs
        assert torch.equal(runs["before0"][k], runs["before1"][k]), k
        n = runs["before0"][k][0].numel()
        a, b = runs["noise1"][k], runs["noise0"][k]
        assert (a <= b * (1 + n * 2.0 ** -52)).all(), (k, float((a / b).max()))


def test_a_layer_the_statement_narrows_improves(runs):
    """The CPU statement on one layer's weights (the smallest layer with rows of
    at least 64 elements): where it narrows a channel, the layer's reported noise
    with the search is strictly below the run without it."""
    from data_free_quantization_amd import _lib
    sized = [(runs["before0"][k].numel(), i) for i, k in enumerate(runs["tkeys"])
             if runs["before0"][k][0].numel() >= 64]
    i = min(sized)[1]
    k = runs["tkeys"][i]
    x = runs["before0"][k].cpu().numpy()
    x2 = x.reshape(x.shape[0], -1)
    noise = CC.noise_table(x2, 4, _lib.DFQ_CHANNEL_SYM, 16, 0.5)
    choice = np.argmin(noise, axis=1)
    e0, e1 = runs["rep0"]["layers"][i], runs["rep1"]["layers"][i]
    print("layer", k, x.shape, "statement narrows %d of %d channels; reported %d" % ((choice > 0).sum(), choice.size,
                                                                                   e1["clip_narrowed"]))
    srt = np.sort(noise, axis=1)
    if ((srt[:, 1] - srt[:, 0]) > CC.GAP * srt[:, 0]).all():   # no choice hangs on a rounding
        assert e1["clip_narrowed"] == int((choice > 0).sum())
        assert e1["clip_at_edge"] == int(((choice > 0) & (choice == 15)).sum())
    if (choice > 0).any():
        assert e1["noise"] < e0["noise"], (e1["noise"], e0["noise"])
        assert runs["rep1"]["model"]["noise"] < runs["rep0"]["model"]["noise"]


def test_main_dfq_clip_search_report(tmp_path, monkeypatch, capsys):
    from data_free_quantization_amd import main_dfq
    monkeypatch.chdir(tmp_path)
    path = tmp_path / "quality.json"
    main_dfq.main(FLAGS + ["--bits_weight", "4", "--granularity", "channel", "--symmetric", "--clip_search",
                           "--clip_candidates", "8", "--clip_min_frac", "0.6", "--report", str(path)])
    rep = json.loads(path.read_text())
    cfg = rep["config"]
    assert (cfg["clip_search"], cfg["clip_candidates"], cfg["clip_min_frac"]) == (True, 8, 0.6)
    assert len(rep["layers"]) == 53
    for e in rep["layers"]:
        assert e["clip_units"] == e["shape"][0] and 0 <= e["clip_at_edge"] <= e["clip_narrowed"] <= e["clip_units"]
    assert sum(e["clip_narrowed"] for e in rep["layers"]) > 0


def test_main_dfq_report_without_the_flag_is_unchanged(tmp_path, monkeypatch):
    """Existing behaviour: the report of a run without --clip_search is, byte for
    byte, the file the commit before the search wrote for the same command
    (tests/golden/quality_report_mobilenetv2_w8.json, recorded on an MI355X)."""
    from data_free_quantization_amd import main_dfq
    monkeypatch.chdir(tmp_path)
    path = tmp_path / "quality.json"
    main_dfq.main(FLAGS + ["--report", str(path)])
    assert path.read_bytes() == GOLDEN.read_bytes()
