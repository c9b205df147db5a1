"""The MXFP6 weight formats through pipeline.run_dfq(weight_format=...),
quantize_targ_layer's state and the export: the weights a run leaves are the numpy
statement (tests/mx6_cases.py) of the weights the quantizer saw, bit for bit, and the
24-byte code blocks dequantize to them."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import mx6_cases as M6

pytestmark = pytest.mark.gpu
TARG = (nn.Conv2d, nn.Linear)
STORAGE = {"mxfp6_e2m3": "fp6_e2m3_packed", "mxfp6_e3m2": "fp6_e3m2_packed"}


@pytest.fixture(scope="module")
def run6():
    """run_dfq on the zoo's MobileNetV2 with the weights at the report's snapshot and
    the error sums bias correction is handed."""
    from data_free_quantization_amd import pipeline, zoo
    from data_free_quantization_amd.utils.tracer import build_graph
    model = zoo.build("mobilenetv2", seed=0, relu=True).cuda()
    g = build_graph(model, "positional")
    graph, bottoms = g.getGraph(), g.getBottoms()
    tkeys = [k for k in graph if type(graph[k]) in TARG]
    before, captured, rep = {}, {}, {}

    def hook(stage):
        if stage == "bn2":   # where run_dfq takes the report's snapshot
            for k in tkeys:
                before[k] = graph[k].weight.detach().clone()

    real = pipeline.bias_correction

    def spy(graph_, bottoms_, targ_, **k):
        captured["error_sums"] = k.get("error_sums")
        return real(graph_, bottoms_, targ_, **k)

    pipeline.bias_correction = spy
    try:
        pipeline.run_dfq(model, graph, bottoms, TARG, stage_hook=hook, weight_format="mxfp6_e2m3", bc_mode="fused",
                         clip=False, report=rep)
    finally:
        pipeline.bias_correction = real
    torch.cuda.synchronize()
    return {"graph": graph, "tkeys": tkeys, "before": before, "error_sums": captured.get("error_sums"), "report": rep}


def test_weights_are_the_statement_of_the_snapshot(run6):
    cfg = run6["report"]["config"]
    assert cfg["weight_format"] == "mxfp6_e2m3" and cfg["bits_per_weight"] == 6.25
    assert len(run6["report"]["layers"]) == len(run6["tkeys"]) == 53
    for k in run6["tkeys"]:
        layer = run6["graph"][k]
        x = run6["before"][k].cpu().numpy()
        ref = M6.statement(x.reshape(x.shape[0], -1), "mxfp6_e2m3")
        w = layer.weight.detach().cpu().numpy()
        assert np.array_equal(w.reshape(x.shape[0], -1).view(np.uint32), ref["y"].view(np.uint32)), k
        assert layer.weight_format == "mxfp6_e2m3", k
    print("MobileNetV2 mxfp6_e2m3 model SQNR %.2f dB" % run6["report"]["model"]["sqnr_db"])


def test_fused_error_sums_are_the_mx_errors(run6):
    err = run6["error_sums"]
    assert err is not None and set(err) == set(run6["tkeys"])
    for k in run6["tkeys"]:
        x = run6["before"][k]
        w = run6["graph"][k].weight.detach()
        khw = x[0, 0].numel()
        want = torch.sum((w.cpu() - x.cpu()).view(x.shape[0], -1, khw), -1).reshape(-1)
        e = err[k]
        got = e if isinstance(e, torch.Tensor) else e[0][e[1]:e[1] + e[2]]
        assert torch.equal(got.cpu(), want), k


@pytest.mark.parametrize("fmt", list(M6.FORMATS))
def test_state_codes_dequantize_to_the_weights_and_survive_the_export(fmt, tmp_path):
    from data_free_quantization_amd import export, mx, zoo
    from data_free_quantization_amd.utils.layer_transform import merge_batchnorm, quantize_targ_layer
    from data_free_quantization_amd.utils.tracer import build_graph
    model = zoo.build("mobilenetv2", seed=0, relu=True).cuda()
    g = build_graph(model, "positional")
    graph, bottoms = g.getGraph(), g.getBottoms()
    merge_batchnorm(model, graph, bottoms, TARG)
    w0 = {k: graph[k].weight.detach().clone() for k in graph if type(graph[k]) in TARG}
    state = {}
    quantize_targ_layer(graph, 8, 8, TARG, state=state, weight_format=fmt)
    torch.cuda.synchronize()
    assert len(state) == 53
    for k, st in state.items():
        w = graph[k].weight.detach()
        assert set(st) == {"codes", "scales", "esum", "khw", "format"} and st["format"] == fmt
        nb = -(-w[0].numel() // 32)
        assert st["codes"].shape == (w.shape[0], nb, 24) and st["codes"].dtype == torch.uint8
        assert st["scales"].shape == (w.shape[0], nb)
        y = mx.mx_dequantize(st["codes"], st["scales"], w.shape, fmt)
        assert torch.equal(y.view(torch.int32), w.view(torch.int32)), k
    k = max(state, key=lambda k: graph[k].weight.numel())   # the codes themselves, on the largest layer
    x = w0[k].cpu().numpy()
    ref = M6.statement(x.reshape(x.shape[0], -1), fmt)
    assert np.array_equal(state[k]["codes"].cpu().numpy(), ref["codes"])
    assert np.array_equal(state[k]["scales"].cpu().numpy(), ref["scales"])
    path = tmp_path / "w.safetensors"
    export.save(path, graph, state, bits=8, granularity="tensor", symmetric=False, weight_format=fmt)
    meta, entries = export.load(path)
    assert meta["format"] == "dfq-mi355x/1" and meta["weight_format"] == fmt and meta["mx_block"] == 32
    assert meta["code_storage"] == STORAGE[fmt] and meta["bits_per_weight"] == 6.25
    assert set(entries) == {str(k) for k in state}
    for k in state:
        e = entries[str(k)]
        assert set(e) == {"codes", "scales"} | ({"bias"} if graph[k].bias is not None else set())
        assert e["codes"].shape[-1] == 24
        y = export.dequantize(meta, str(k), e)
        assert torch.equal(y.view(torch.int32), graph[k].weight.detach().cpu().view(torch.int32)), k
