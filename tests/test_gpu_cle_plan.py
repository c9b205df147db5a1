"""Device-resident CLE loop (dfq_cle_plan) vs the oracle's sequential replay of
Cross_layer_equal.py:63-116 on hand-made graphs: several independent chains
(dense, depthwise, grouped, Linear), signed ranges, eps, custom scale limits, a
dead channel, a relation without BN stats, a layer shared by two relations in
one chain and a large layer (multi-chunk metric).  Weights, biases, BN fake
stats, Relation.S, iteration count and every per-iteration diff: bit-exact."""
import os
import time
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests.cle_replay import _BN, _conv, _replay   # the module builders and the oracle's replay (shared)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _graph(seed, dead_dw=None):
    from data_free_quantization_amd.utils.relation import Relation
    rng = np.random.default_rng(seed)
    g = OrderedDict()
    g["Data"] = "Data"
    # chain A: dense 3x3 -> 1x1 (tile path) -> grouped(2) 3x3, with a dead channel
    g["a1"] = _conv(16, 3, 3, rng=rng, dead=5)
    g["a1bn"] = _BN(16, rng)
    g["a2"] = _conv(24, 16, 1, rng=rng, bias=False)
    g["a2bn"] = _BN(24, rng)
    g["a3"] = _conv(32, 24, 3, groups=2, rng=rng)
    # chain B: pointwise -> depthwise (contiguous columns) -> pointwise
    g["b1"] = _conv(40, 8, 1, rng=rng)
    g["b1bn"] = _BN(40, rng)
    g["b2"] = _conv(40, 40, 3, groups=40, rng=rng, dead=dead_dw)
    g["b2bn"] = _BN(40, rng, with_stats=False)
    g["b3"] = _conv(20, 40, 1, rng=rng)
    # chain C: one big layer (metric over several 32768-element chunks) -> Linear
    g["c1"] = _conv(256, 64, 3, rng=rng)
    g["c1bn"] = _BN(256, rng)
    lin = nn.Linear(256, 10)
    lin.weight.data = torch.from_numpy(rng.normal(0, 0.05, (10, 256)).astype(np.float32))
    g["c2"] = lin.to(DEV)
    # a target that no relation touches
    g["d1"] = _conv(4, 4, 1, rng=rng)
    rels = [Relation("a1", "a2", "a1bn"), Relation("b1", "b2", "b1bn"), Relation("a2", "a3", "a2bn"),
            Relation("c1", "c2", "c1bn"), Relation("b2", "b3", "b2bn")]
    return g, rels


@pytest.mark.parametrize("signed,eps,smm,thr,count", [
    (False, 0.0, (1e-8, 1e8), 2e-7, 20),
    (True, 0.0, (1e-8, 1e8), 2e-7, 20),
    (False, 1e-3, (0.5, 2.0), 1e-6, 5),
    (False, 0.0, (1e-8, 1e8), 1e3, 20),     # stops after one iteration
])
def test_device_cle_matches_oracle(signed, eps, smm, thr, count, monkeypatch):
    from data_free_quantization_amd import Cross_layer_equal as cle
    monkeypatch.setenv("DFQ_CLE_MODE", "device")
    g, rels = _graph(0)
    W, B, BN, S, diffs = _replay(g, rels, smm, thr, count, signed, eps)
    cle.cross_layer_equalization(g, rels, [nn.Conv2d, nn.Linear], s_min_max=list(smm), Treshhold=thr, Count=count,
                                 signed=signed, eps=eps, Save_state=False)
    torch.cuda.synchronize()
    assert cle.LAST_RUN["chains"] == 3 and cle.LAST_RUN["steps"] == 2
    # fused schedule: 2 rescale steps + ONE launch of metric tiles with the next
    # iteration's ranges, the chunk combine and the stop rule folded in; else
    # 2 x (range + rescale) + that launch
    diag = os.environ.get("DFQ_LIB") == "diag"   # the A/B switches exist in the diagnostics library only
    fused = not (diag and os.environ.get("DFQ_CLE_FUSED") == "0")
    # fused: 2 rescale steps + the tiles/ranges/stop-rule launch; else 2 x (range +
    # rescale) + that launch
    expect = 3 if fused else 5
    assert cle.LAST_RUN["launches_per_iteration"] == expect
    assert cle.LAST_RUN["diffs"] == diffs
    for k in W:
        assert np.array_equal(g[k].weight.detach().cpu().numpy(), W[k]), k
        if B[k] is not None:
            assert np.array_equal(g[k].bias.detach().cpu().numpy(), B[k]), k
    for k, (fw, fb) in BN.items():
        if fw is not None:
            assert np.array_equal(g[k].fake_weight.cpu().numpy(), fw), k
            assert np.array_equal(g[k].fake_bias.cpu().numpy(), fb), k
    for i, r in enumerate(rels):
        assert np.array_equal(r.S.cpu().numpy(), S[i]), i


@pytest.mark.parametrize("launch", [False, True])
@pytest.mark.parametrize("cap", [1, 3])
def test_device_cle_stops_at_iteration_cap(cap, launch, monkeypatch):
    """The iteration cap (Cross_layer_equal.MAX_ITERS; the Python layer's default of
    100,000 is never reached): the loop stops after `cap` iterations with the
    warning, and weights, biases, BN fake statistics, S and diffs equal the oracle
    replay cut at the same iteration, bit for bit.  The lagged schedule has by then
    started iteration `cap` speculatively (its rescales run before the stop rule
    of iteration cap - 1 is known), so this is the rollback's test; and cap + 1 <=
    1025 keeps the history in the plan tables' own slots, not the context's buffer."""
    from data_free_quantization_amd import Cross_layer_equal as cle
    monkeypatch.setenv("DFQ_CLE_MODE", "device")
    monkeypatch.setattr(cle, "MAX_ITERS", cap)
    g, rels = _graph(0)
    W, B, BN, S, diffs = _replay(g, rels, (1e-8, 1e8), 2e-7, 20, False, 0.0, max_iters=cap)
    assert len(diffs) == cap   # the cap cut the loop short, not its stop rule
    with pytest.warns(UserWarning, match="DFQ_CLE_MAX_ITERS"):
        cle.cross_layer_equalization(g, rels, [nn.Conv2d, nn.Linear], Treshhold=2e-7, Count=20, Save_state=False,
                                     launch=launch)
        cle.wait()
    torch.cuda.synchronize()
    assert cle.LAST_RUN["launched"] == launch
    assert cle.LAST_RUN["iterations"] == cap
    assert cle.LAST_RUN["diffs"] == diffs
    for k in W:
        assert np.array_equal(g[k].weight.detach().cpu().numpy(), W[k]), k
        if B[k] is not None:
            assert np.array_equal(g[k].bias.detach().cpu().numpy(), B[k]), k
    for k, (fw, fb) in BN.items():
        if fw is not None:
            assert np.array_equal(g[k].fake_weight.cpu().numpy(), fw), k
            assert np.array_equal(g[k].fake_bias.cpu().numpy(), fb), k
    for i, r in enumerate(rels):
        assert np.array_equal(r.S.cpu().numpy(), S[i]), i


@pytest.mark.parametrize("signed", [False, True])
def test_device_cle_depthwise_pair_edges(signed, monkeypatch):
    """Chain B (pointwise -> depthwise -> pointwise) runs both relations in ONE
    launch: the second relation's W1 ranges are derived from the depthwise
    filters' ranges scaled by the first relation's 1/s (cle_rel_scale).  Dead
    depthwise filters (s = smin, then r1 = 0 -> s = smax for the next relation),
    signed ranges: weights, biases, BN stats, scales and diffs bit-exact with the
    relation-by-relation oracle replay."""
    from data_free_quantization_amd import Cross_layer_equal as cle
    monkeypatch.setenv("DFQ_CLE_MODE", "device")
    g, rels = _graph(3, dead_dw=[7, 19])
    W, B, BN, S, diffs = _replay(g, rels, (1e-8, 1e8), 2e-7, 20, signed, 0.0)
    cle.cross_layer_equalization(g, rels, [nn.Conv2d, nn.Linear], Treshhold=2e-7, signed=signed, Save_state=False)
    torch.cuda.synchronize()
    assert cle.LAST_RUN["steps"] == 2   # chain A's two relations; chain B's pair shares one step
    assert cle.LAST_RUN["diffs"] == diffs
    for k in W:
        assert np.array_equal(g[k].weight.detach().cpu().numpy(), W[k]), k
        if B[k] is not None:
            assert np.array_equal(g[k].bias.detach().cpu().numpy(), B[k]), k
    for k, (fw, fb) in BN.items():
        if fw is not None:
            assert np.array_equal(g[k].fake_weight.cpu().numpy(), fw), k
            assert np.array_equal(g[k].fake_bias.cpu().numpy(), fb), k
    for i, r in enumerate(rels):
        assert np.array_equal(r.S.cpu().numpy(), S[i]), i


def test_device_cle_accumulates_existing_scale(monkeypatch):
    """A second call multiplies into Relation.S (set_scale_vec) instead of storing."""
    from data_free_quantization_amd import Cross_layer_equal as cle
    monkeypatch.setenv("DFQ_CLE_MODE", "device")
    g, rels = _graph(1)
    cle.cross_layer_equalization(g, rels, [nn.Conv2d, nn.Linear], Treshhold=1e3, Save_state=False)
    s1 = [r.S.clone() for r in rels]
    g2, rels2 = _graph(1)
    cle.cross_layer_equalization(g2, rels2, [nn.Conv2d, nn.Linear], Treshhold=1e3, Save_state=False)
    cle.cross_layer_equalization(g2, rels2, [nn.Conv2d, nn.Linear], Treshhold=1e3, Save_state=False)
    g3, rels3 = _graph(1)
    cle.cross_layer_equalization(g3, rels3, [nn.Conv2d, nn.Linear], Treshhold=1e3, Save_state=False)
    for r in rels3:
        r.S = None
    cle.cross_layer_equalization(g3, rels3, [nn.Conv2d, nn.Linear], Treshhold=1e3, Save_state=False)
    for a, r2, r3 in zip(s1, rels2, rels3):
        assert torch.equal(r2.S, a * r3.S)


def test_device_cle_no_relations(monkeypatch):
    from data_free_quantization_amd import Cross_layer_equal as cle
    monkeypatch.setenv("DFQ_CLE_MODE", "device")
    g, _ = _graph(2)
    before = {k: g[k].weight.detach().clone() for k in g if isinstance(g[k], (nn.Conv2d, nn.Linear))}
    cle.cross_layer_equalization(g, [], [nn.Conv2d, nn.Linear], Save_state=False)
    assert cle.LAST_RUN["iterations"] == 1 and cle.LAST_RUN["diffs"] == [0.0]
    for k, w in before.items():
        assert torch.equal(g[k].weight, w)


def test_two_live_plans():
    """A plan created while another is alive takes private device tables (the
    per-device table pool is busy); both runs equal one plan at a time, bit for
    bit (models, S, iteration counts, diffs)."""
    from data_free_quantization_amd import Cross_layer_equal as cle, zoo
    from data_free_quantization_amd.utils.layer_transform import merge_batchnorm
    from data_free_quantization_amd.utils.relation import create_relation
    from data_free_quantization_amd.utils.tracer import build_graph
    T = [nn.Conv2d, nn.Linear]

    def prep(name, seed):
        m = zoo.build(name, seed=seed, relu=True).to(DEV)
        g = build_graph(m, "positional")
        G, B = g.getGraph(), g.getBottoms()
        merge_batchnorm(m, G, B, T)
        return m, G, create_relation(G, B, T)

    cases = (("mobilenetv2", 3), ("resnet50", 4))
    refs = []
    for name, seed in cases:
        m, G, rels = prep(name, seed)
        cle.cross_layer_equalization(G, rels, T, Save_state=False, Treshhold=2e-7)
        torch.cuda.synchronize()
        refs.append((m, rels, cle.LAST_RUN["iterations"], cle.LAST_RUN["diffs"]))
    live = [prep(name, seed) for name, seed in cases]
    plans = [cle._create_plan(G, rels, T, [1e-8, 1e8], False, 0) for _, G, rels in live]
    try:
        runs = [cle._run_plan(plan, dev, 2e-7, 20) for plan, _, dev in reversed(plans)][::-1]
    finally:
        for plan, _, _ in plans:
            cle._lib.load().dfq_cle_plan_destroy(plan)
    torch.cuda.synchronize()
    for (m0, r0, it0, d0), (m1, _, r1), (it1, d1, _, _) in zip(refs, live, runs):
        assert it0 == it1 and d0 == d1
        for (k, a), (_, b) in zip(m0.state_dict().items(), m1.state_dict().items()):
            assert torch.equal(a, b), k
        for a, b in zip(r0, r1):
            assert torch.equal(a.S, b.S)


def _weights(g):
    return {k: g[k].weight for k in g if type(g[k]) in (nn.Conv2d, nn.Linear)}


@pytest.mark.parametrize("producer", [False, True])
def test_async_launch_orders_the_callers_stream(producer, monkeypatch):
    """dfq_cle_plan_launch: the call returns with the loop under way; work the
    caller enqueues afterwards on its stream (here: clones of every weight, with no
    wait and no sync in between) sees the loop's final weights, and work enqueued
    before it (a producer rewriting the weights) is seen by the loop.  Results and
    LAST_RUN are bit-identical with the blocking run."""
    from data_free_quantization_amd import Cross_layer_equal as cle
    monkeypatch.setenv("DFQ_CLE_MODE", "device")
    out = {}
    for mode in (False, True):
        monkeypatch.setattr(cle, "ASYNC", mode)
        g, rels = _graph(3)
        torch.cuda.synchronize()
        if producer:   # in flight on the caller's stream when the loop is launched
            for w in _weights(g).values():
                w.data.mul_(1.25)   # (keeps the dead channel dead)
        cle.cross_layer_equalization(g, rels, [nn.Conv2d, nn.Linear], Treshhold=2e-7, Count=20, Save_state=False)
        clones = {k: w.detach().clone() for k, w in _weights(g).items()}   # enqueued behind the loop
        if mode:
            assert cle._PENDING is not None or cle.LAST_RUN._d   # launched (or already joined)
        out[mode] = ({k: v.cpu() for k, v in clones.items()}, dict(cle.LAST_RUN), [r.S.cpu() for r in rels])
    (wa, ra, sa), (wb, rb, sb) = out[False], out[True]
    assert rb["launched"] and not ra["launched"]
    assert ra["iterations"] == rb["iterations"]
    np.testing.assert_array_equal(ra["diffs"], rb["diffs"])   # (NaN == NaN here)
    for k in wa:
        assert torch.equal(wa[k].view(torch.int32), wb[k].view(torch.int32)), k
    for x, y in zip(sa, sb):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_async_launches_back_to_back(monkeypatch):
    """Two launched loops with no wait between them (the second call joins the
    first), then a third on the same graph: each equals its blocking twin."""
    from data_free_quantization_amd import Cross_layer_equal as cle
    monkeypatch.setenv("DFQ_CLE_MODE", "device")
    res = {}
    for mode in (False, True):
        monkeypatch.setattr(cle, "ASYNC", mode)
        g1, r1 = _graph(4)
        g2, r2 = _graph(5)
        cle.cross_layer_equalization(g1, r1, [nn.Conv2d, nn.Linear], Treshhold=2e-7, Count=20, Save_state=False)
        cle.cross_layer_equalization(g2, r2, [nn.Conv2d, nn.Linear], Treshhold=2e-7, Count=20, Save_state=False)
        n2 = cle.LAST_RUN["iterations"]
        cle.cross_layer_equalization(g1, r1, [nn.Conv2d, nn.Linear], Treshhold=2e-7, Count=20, Save_state=False)
        cle.wait()
        res[mode] = ({k: w.detach().cpu() for k, w in _weights(g1).items()},
                     {k: w.detach().cpu() for k, w in _weights(g2).items()}, n2, cle.LAST_RUN["diffs"])
    a, b = res[False], res[True]
    assert a[2] == b[2]
    np.testing.assert_array_equal(a[3], b[3])
    for da, db in ((a[0], b[0]), (a[1], b[1])):
        for k in da:
            assert torch.equal(da[k].view(torch.int32), db[k].view(torch.int32)), k


def test_async_join_watchdog_keeps_callers_stream_held(monkeypatch):
    """Fail-closed launched loop: when join gives up waiting (its host
    watchdog; shortened here with the diagnostics library's test switches, the
    worker's release delayed), the call raises, and the work the caller queued
    behind the loop has NOT run -- the caller's stream stays held behind the gate
    until the loop really releases it."""
    from data_free_quantization_amd import _lib
    from data_free_quantization_amd import Cross_layer_equal as cle
    monkeypatch.setattr(_lib, "_LIB", _lib.load_diag())
    monkeypatch.setenv("DFQ_CLE_MODE", "device")
    monkeypatch.setenv("DFQ_CLE_TEST_RELEASE_DELAY_MS", "2500")
    monkeypatch.setenv("DFQ_CLE_TEST_JOIN_LIMIT_MS", "200")
    monkeypatch.setenv("DFQ_CLE_HOST_RELEASE", "1")   # only the worker's (delayed) release opens the gate
    g, rels = _graph(3)
    torch.cuda.synchronize()
    marker = torch.zeros(1, device=DEV)
    torch.cuda.synchronize()
    cle.cross_layer_equalization(g, rels, [nn.Conv2d, nn.Linear], Treshhold=2e-7, Save_state=False, launch=True)
    marker.fill_(1.0)                        # a downstream stage, queued behind the loop
    with pytest.raises(RuntimeError, match="did not finish"):
        cle.wait()
    assert not torch.cuda.current_stream().query()   # still held: the downstream work has not run
    torch.cuda.synchronize()                 # the delayed release arrives, then it runs
    assert marker.item() == 1.0


def test_async_caller_released_at_convergence(monkeypatch):
    """The stop rule opens the caller's gate when the loop converges, before the
    worker's own release (delayed here by 4 s): the work queued behind the loop
    runs, sees the final weights, and LAST_RUN still comes from the join."""
    from data_free_quantization_amd import _lib
    from data_free_quantization_amd import Cross_layer_equal as cle
    monkeypatch.setattr(_lib, "_LIB", _lib.load_diag())
    monkeypatch.setenv("DFQ_CLE_MODE", "device")
    g0, r0 = _graph(3)
    cle.cross_layer_equalization(g0, r0, [nn.Conv2d, nn.Linear], Treshhold=2e-7, Save_state=False, launch=False)
    ref = {k: w.detach().clone() for k, w in _weights(g0).items()}
    monkeypatch.setenv("DFQ_CLE_TEST_RELEASE_DELAY_MS", "4000")
    g, rels = _graph(3)
    torch.cuda.synchronize()
    cle.cross_layer_equalization(g, rels, [nn.Conv2d, nn.Linear], Treshhold=2e-7, Save_state=False, launch=True)
    t0 = time.perf_counter()
    clones = {k: w.detach().clone() for k, w in _weights(g).items()}   # queued behind the loop
    torch.cuda.current_stream().synchronize()
    # released by the device (the loop takes milliseconds), not by the worker 4 s later:
    # which release it was, not a speed -- the margin is seconds
    assert time.perf_counter() - t0 < 3.0
    assert cle._PENDING is not None             # the worker has not finished
    for k in ref:
        assert torch.equal(ref[k].view(torch.int32), clones[k].view(torch.int32)), k
    cle.wait()
    assert cle.LAST_RUN["launched"]


def _many_layer_graph(n_chains, seed=5):
    """n_chains independent 3-layer 1x1 chains (8 channels, 64-weight layers):
    3 * n_chains target layers, 2 * n_chains relations."""
    from data_free_quantization_amd.utils.relation import Relation
    rng = np.random.default_rng(seed)
    g = OrderedDict()
    g["Data"] = "Data"
    rels = []
    for c in range(n_chains):
        g[f"x{c}a"] = _conv(8, 8, 1, rng=rng)
        g[f"x{c}abn"] = _BN(8, rng)
        g[f"x{c}b"] = _conv(8, 8, 1, rng=rng)
        g[f"x{c}bbn"] = _BN(8, rng)
        g[f"x{c}c"] = _conv(8, 8, 1, rng=rng)
        rels += [Relation(f"x{c}a", f"x{c}b", f"x{c}abn"), Relation(f"x{c}b", f"x{c}c", f"x{c}bbn")]
    return g, rels


@pytest.mark.parametrize("n_chains", [47, 240])
def test_device_cle_many_layers(n_chains, monkeypatch):
    """Past numpy's one-leaf pairwise sum (> 128 layer means: the stop rule's frame
    stack) and, at 720 layers, past the stop rule's LDS staging of the chunk sums,
    layer sizes and state (the per-layer loads fallback): diffs, weights, biases and
    scales bit-exact with the oracle replay."""
    from data_free_quantization_amd import Cross_layer_equal as cle
    monkeypatch.setenv("DFQ_CLE_MODE", "device")
    g, rels = _many_layer_graph(n_chains)
    W, B, BN, S, diffs = _replay(g, rels, (1e-8, 1e8), 1e-3, 20, False, 0.0)
    cle.cross_layer_equalization(g, rels, [nn.Conv2d, nn.Linear], Treshhold=1e-3, Save_state=False)
    torch.cuda.synchronize()
    assert cle.LAST_RUN["chains"] == n_chains
    assert cle.LAST_RUN["diffs"] == diffs
    for k in W:
        assert np.array_equal(g[k].weight.detach().cpu().numpy(), W[k]), k
        assert np.array_equal(g[k].bias.detach().cpu().numpy(), B[k]), k
    for i, r in enumerate(rels):
        assert np.array_equal(r.S.cpu().numpy(), S[i]), i


def test_plan_stats_bytes_and_device_time(monkeypatch):
    """dfq_cle_plan_stats (bench.py's cle_roofline): the metric tiles' bytes are
    12 B per target element, the rescales' at least 8 B per element of every
    relation's W1 and W2 (a depthwise pair's filter counted once); a timed blocking
    run reports its loop's device time, and untimed runs report none."""
    from data_free_quantization_amd import zoo, Cross_layer_equal as cle
    from data_free_quantization_amd.utils.layer_transform import merge_batchnorm
    from data_free_quantization_amd.utils.relation import create_relation
    from data_free_quantization_amd.utils.tracer import build_graph
    T = (nn.Conv2d, nn.Linear)
    m = zoo.build("mobilenetv2", seed=0, relu=True).to(DEV)
    g = build_graph(m, "positional")
    G, B = g.getGraph(), g.getBottoms()
    merge_batchnorm(m, G, B, T)
    rels = create_relation(G, B, T)
    monkeypatch.setattr(cle, "DEVICE_TIMING", True)
    cle.cross_layer_equalization(G, rels, T, Save_state=False, Treshhold=2e-7, launch=False)
    r = dict(cle.LAST_RUN)
    tw = sum(G[k].weight.numel() for k in G if type(G[k]) in T)
    by = r["bytes_per_iteration"]
    assert by["metric"] == 12 * tw
    w1 = sum(G[x.layer_first].weight.numel() for x in rels)
    assert 8 * w1 <= by["rescale"] <= 8 * 2 * sum(G[x.layer_first].weight.numel() + G[x.layer_second].weight.numel()
                                                  for x in rels)
    assert by["total"] == by["rescale"] + by["metric"] + by["ranges"]
    assert r["iterations"] == 44 and r["iterations_launched"] >= r["iterations"]
    per_it_us = r["device_ms"] * 1e3 / r["iterations_launched"]
    assert 5.0 < per_it_us < 2000.0, per_it_us
    monkeypatch.setattr(cle, "DEVICE_TIMING", False)
    m2 = zoo.build("mobilenetv2", seed=0, relu=True).to(DEV)
    g2 = build_graph(m2, "positional")
    G2, B2 = g2.getGraph(), g2.getBottoms()
    merge_batchnorm(m2, G2, B2, T)
    cle.cross_layer_equalization(G2, create_relation(G2, B2, T), T, Save_state=False, Treshhold=2e-7, launch=False)
    assert cle.LAST_RUN["device_ms"] is None and cle.LAST_RUN["bytes_per_iteration"] == by
