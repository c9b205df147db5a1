"""The quality report through pipeline.run_dfq(report=...) and main_dfq --report:
every layer's figures recomputed in numpy from the weights before and after the
quantization (tolerance and oracle as in tests/test_gpu_pair_stats.py)."""
import json
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
TARG = (nn.Conv2d, nn.Linear)

FLAGS = ["--task", "cls", "--relu", "--equalize", "--absorption", "--quantize", "--correction", "--clip_weight",
         "--bits_weight", "8", "--bits_activation", "8", "--bits_bias", "8", "--log"]


def _run(report, **kw):
    from data_free_quantization_amd import zoo
    from data_free_quantization_amd.pipeline import run_dfq
    from data_free_quantization_amd.utils.tracer import build_graph
    model = zoo.build("mobilenetv2", seed=0, relu=True).cuda()
    g = build_graph(model, "positional")
    graph, bottoms = g.getGraph(), g.getBottoms()
    tkeys = [k for k in graph if type(graph[k]) in TARG]
    before = {}

    def hook(stage):
        if stage == "bn2":
            for k in tkeys:
                before[k] = graph[k].weight.detach().clone()

    run_dfq(model, graph, bottoms, TARG, stage_hook=hook, report=report, **kw)
    torch.cuda.synchronize()
    return tkeys, {k: v.cpu().numpy() for k, v in before.items()}, \
        {k: graph[k].weight.detach().cpu().numpy() for k in tkeys}


LD = np.longdouble
# The oracle's sums here are numpy pairwise sums in x87 extended precision (64-bit
# significand): within n 2^-64 of the exact sum of the exact fp64 terms, 2^-12 of
# the tolerance -- math.fsum over MobileNetV2's 3.5 M weights, four times a run,
# would take this test past a few seconds.
assert np.finfo(LD).nmant >= 63


def _close(got, exact, n):
    return abs(LD(got) - exact) <= n * LD(2.0) ** -52 * exact


def _check_model(rep):
    signal = noise = 0.0
    for e in rep["layers"]:
        signal += e["signal"]
        noise += e["noise"]
    m = rep["model"]
    assert m["signal"] == signal and m["noise"] == noise
    assert m["sqnr_db"] == 10.0 * math.log10(signal / noise)
    assert m["elements"] == sum(e["elements"] for e in rep["layers"])
    rated = [e for e in rep["layers"] if e["sqnr_db"] is not None]
    assert m["worst_layer"] == min(rated, key=lambda e: e["sqnr_db"])["key"]


@pytest.mark.parametrize("kw", [{}, {"granularity": "channel", "symmetric": True, "bc_mode": "fused"}],
                         ids=["tensor_asym", "channel_sym_fused"])
def test_run_dfq_report_matches_numpy(kw):
    rep = {}
    tkeys, before, after = _run(rep, **kw)
    assert rep["format"] == "dfq-quality/1"
    assert rep["config"]["granularity"] == kw.get("granularity", "tensor")
    assert rep["config"]["symmetric"] == kw.get("symmetric", False) and rep["config"]["bits_weight"] == 8
    assert [e["key"] for e in rep["layers"]] == [str(k) for k in tkeys] and len(tkeys) == 53
    for k, e in zip(tkeys, rep["layers"]):
        x, y = before[k], after[k]
        rows, row_len = x.shape[0], x.size // x.shape[0]
        x2, y2 = x.reshape(rows, row_len), y.reshape(rows, row_len)
        err = y2 - x2
        assert err.dtype == np.float32
        sig, noi = x2.astype(np.float64) ** 2, err.astype(np.float64) ** 2
        assert e["type"] in ("Conv2d", "Linear") and e["shape"] == list(x.shape) and e["elements"] == x.size
        sig_l, noi_l = sig.astype(LD), noi.astype(LD)
        s, n = sig_l.sum(), noi_l.sum()
        print(k, e["sqnr_db"], "signal rel err %.3g" % float(abs(LD(e["signal"]) - s) / s))
        assert _close(e["signal"], s, x.size) and _close(e["noise"], n, x.size), (k, e["signal"], s, e["noise"], n)
        assert e["max_abs_err"] == float(np.abs(err).max()) and e["max_abs_weight"] == float(np.abs(x2).max())
        assert n > 0 and abs(e["sqnr_db"] - 10.0 * math.log10(float(s) / float(n))) < 1e-9
        rs, rn = sig_l.sum(axis=1).astype(np.float64), noi_l.sum(axis=1).astype(np.float64)
        noisy = np.flatnonzero(rn != 0)
        worst = int(noisy[np.argmin(rs[noisy] / rn[noisy])])
        assert e["worst_channel"] == worst, k
        assert abs(e["worst_channel_sqnr_db"] - 10.0 * math.log10(rs[worst] / rn[worst])) < 1e-9
        prec = np.abs(x2).max(axis=1).astype(np.float64) / float(np.abs(x2).max())
        assert e["channel_precision_min"] == prec.min() and abs(e["channel_precision_mean"] - prec.mean()) < 1e-12
    _check_model(rep)
    json.loads(json.dumps(rep, allow_nan=False))
    # the hook changes nothing: the same final weights without a report
    _, before0, after0 = _run(None, **kw)
    for k in tkeys:
        assert np.array_equal(after[k].view(np.uint32), after0[k].view(np.uint32)), k
        assert np.array_equal(before[k].view(np.uint32), before0[k].view(np.uint32)), k


def test_main_dfq_report(tmp_path, monkeypatch, capsys):
    from data_free_quantization_amd import main_dfq
    monkeypatch.chdir(tmp_path)
    path = tmp_path / "quality.json"
    main_dfq.main(FLAGS + ["--report", str(path)])
    rep = json.loads(path.read_text())
    assert rep["format"] == "dfq-quality/1" and len(rep["layers"]) == 53
    assert rep["config"]["model"] == "mobilenetv2" and rep["config"]["bits_weight"] == 8
    for e in rep["layers"]:
        assert isinstance(e["sqnr_db"], float) and math.isfinite(e["sqnr_db"]), e["key"]
        assert 0 <= e["worst_channel"] < e["shape"][0] and e["worst_channel_sqnr_db"] <= e["sqnr_db"] + 1e-9
        assert 0.0 <= e["channel_precision_min"] <= e["channel_precision_mean"] <= 1.0
    _check_model(rep)
    out = capsys.readouterr().out
    line = [ln for ln in out.splitlines() if ln.startswith("Quality report:")]
    assert len(line) == 1 and rep["model"]["worst_layer"] in line[0] and "%.2f" % rep["model"]["sqnr_db"] in line[0]


def test_report_needs_quantize(capsys):
    from data_free_quantization_amd import main_dfq
    with pytest.raises(SystemExit) as ei:
        main_dfq.main(["--task", "cls", "--relu", "--equalize", "--absorption", "--report", "x.json"])
    assert ei.value.code == 2
    assert "--report needs --quantize" in capsys.readouterr().err
