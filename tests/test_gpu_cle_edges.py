"""The device-resident CLE loop (dfq_cle_plan_*, csrc/dfq_cle_kernels.h) and the
single-relation kernel (dfq_cle_relation) at the edges of their range, rescale and
metric code: the graphs of tests/cle_edge_cases.py (W1 row lengths around the lane
groups and the wave strides, depthwise filters of 1x1 .. 9x9 taps, 1x1 / position /
per-column W2 tiles around the 16-row and 256-column tiles, grouped layers whose
tiles straddle groups, per-channel vector tasks, metric layers one element either
side of a tile and a chunk), random and planted values, unsigned and signed ranges.

Three iterations under the iteration cap (both range parities and the speculative
iteration's rollback; the stop rule cannot fire earlier, every graph holds a chain
that keeps moving).  Every diff, weight, bias, BN fake weight / bias and Relation.S
equals the oracle's sequential replay bit for bit AND the reference's own run
(tests/golden/cle_edge_cases.npz); a launched run (launch=True, then wait()) gives
the same bits.  A failure names the chain's tensor and the first differing flat
index with both values."""
from functools import lru_cache

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import oracle as O
from tests import cle_edge_cases as CE
from tests.cle_replay import _replay, edge_graph, edge_state
from tests.test_oracle_cle_edges import fixture_mismatches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = [nn.Conv2d, nn.Linear]


@lru_cache(maxsize=None)
def _oracle(graph, value_set, signed):
    """The oracle's replay, computed once per case and shared (read only)."""
    g, rels = edge_graph(graph, value_set, device="cpu")
    return _replay(g, rels, CE.S_MIN_MAX, 2e-7, 20, signed, 0.0, max_iters=CE.ITERATIONS)


def _mismatches(tag, got, want):
    """Messages for every tensor of a device run that differs from the oracle's."""
    (W, B, BN, S), (oW, oB, oBN, oS) = got, want
    bad = []
    for k in oW:
        bad.append(CE.first_difference(f"{tag} {k}:weight", W[k], oW[k]))
        if oB[k] is not None:
            bad.append(f"{tag} {k}:bias missing" if B[k] is None
                       else CE.first_difference(f"{tag} {k}:bias", B[k], oB[k]))
    for k, (fw, fb) in oBN.items():
        if fw is not None:
            bad.append(CE.first_difference(f"{tag} {k}:fake_weight", BN[k][0], fw))
            bad.append(CE.first_difference(f"{tag} {k}:fake_bias", BN[k][1], fb))
    for i in oS:
        bad.append(CE.first_difference(f"{tag} relation {i} ({CE.relations(tag.split('.')[0])[i][0]}):S", S[i], oS[i]))
    return [m for m in bad if m]


@pytest.mark.parametrize("launch", [False, True])
@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("value_set", CE.VALUE_SETS)
@pytest.mark.parametrize("graph", list(CE.GRAPHS))
def test_device_loop_at_the_edges(graph, value_set, signed, launch, monkeypatch):
    from data_free_quantization_amd import Cross_layer_equal as cle
    monkeypatch.setenv("DFQ_CLE_MODE", "device")
    monkeypatch.setattr(cle, "MAX_ITERS", CE.ITERATIONS)
    oW, oB, oBN, oS, diffs = _oracle(graph, value_set, signed)
    assert len(diffs) == CE.ITERATIONS   # the cap cuts the loop short, not its stop rule
    g, rels = edge_graph(graph, value_set, device=DEV)
    with pytest.warns(UserWarning, match="DFQ_CLE_MAX_ITERS"):
        cle.cross_layer_equalization(g, rels, T, s_min_max=list(CE.S_MIN_MAX), Treshhold=2e-7, Count=20,
                                     signed=signed, Save_state=False, launch=launch)
        cle.wait()
    torch.cuda.synchronize()
    assert cle.LAST_RUN["launched"] == launch
    assert cle.LAST_RUN["iterations"] == CE.ITERATIONS
    tag = f"{graph}.{value_set}.{'s' if signed else 'u'}"
    got = edge_state(g, rels)
    bad = _mismatches(tag, got, (oW, oB, oBN, oS))
    if cle.LAST_RUN["diffs"] != diffs:
        bad.append(f"{tag} diffs: got {cle.LAST_RUN['diffs']!r}, oracle {diffs!r}")
    bad += fixture_mismatches(graph, value_set, signed, *got, cle.LAST_RUN["diffs"])
    assert not bad, "%d mismatches:\n" % len(bad) + "\n".join(bad[:12])


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("value_set", CE.VALUE_SETS)
@pytest.mark.parametrize("graph", list(CE.GRAPHS))
def test_single_relation_at_the_edges(graph, value_set, signed):
    """Every relation of every graph once through Cross_layer_equal._layer_equalization
    (dfq_cle_relation.hip: the same shape classes) against oracle.cle_relation."""
    from data_free_quantization_amd import Cross_layer_equal as cle
    tens = CE.tensors(graph, value_set)
    bad = []
    runs = []
    for first, second, bn, chain, j in CE.relations(graph):
        w1, w2 = tens[first]["w"], tens[second]["w"]
        b1 = tens[first]["b"] if tens[first]["b"] is not None else np.zeros(w1.shape[0], np.float32)
        fw, fb = tens[bn]["fw"], tens[bn]["fb"]
        dev = [None if a is None else torch.from_numpy(a.copy()).to(DEV) for a in (w1, w2, b1, fw, fb)]
        _, _, _, s = cle._layer_equalization(dev[0], dev[1], dev[2], dev[3], dev[4], s_min_max=CE.S_MIN_MAX,
                                             signed=signed)
        runs.append((f"{graph}.{value_set}.{'s' if signed else 'u'} {first}>{second}", dev + [s],
                     (w1, w2, b1, fw, fb)))
    torch.cuda.synchronize()
    for name, dev, host in runs:
        want = O.cle_relation(*host, CE.S_MIN_MAX[0], CE.S_MIN_MAX[1], signed, 0.0)
        for what, a, b in zip(("W1", "W2", "B1", "fake_weight", "fake_bias", "S"), dev, want):
            if b is not None:
                bad.append(CE.first_difference(f"{name} {what}", a.cpu().numpy(), b))
    bad = [m for m in bad if m]
    assert not bad, "%d mismatches:\n" % len(bad) + "\n".join(bad[:12])
