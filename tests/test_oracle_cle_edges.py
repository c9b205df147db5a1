"""The CPU oracle's CLE replay (tests/cle_replay._replay: oracle.cle_relation,
mean_abs_diff, np_sum), cut at three iterations, against the reference's own run of
the same graphs (tests/golden/cle_edge_cases.npz, written by make_golden.py's
``cle_edge`` section from tests/cle_edge_cases.py): every small tensor element for
element, every large one by its digest, the three diffs bit for bit.  On a
mismatch the fixture decides, and oracle/dfq_oracle.c is what gets fixed.  No GPU."""
from functools import lru_cache

import numpy as np
import pytest

from tests import cle_edge_cases as CE
from tests.cle_replay import _replay, edge_graph
from tests.helpers import GOLDEN


@lru_cache(maxsize=1)
def cle_edge():
    return np.load(GOLDEN / "cle_edge_cases.npz")


def run_tag(graph, value_set, signed):
    return f"{graph}.{value_set}.{'s' if signed else 'u'}"


def fixture_mismatches(graph, value_set, signed, W, B, BN, S, diffs):
    """What of a run's results differs from the fixture's (a list of messages)."""
    F = cle_edge()
    tag = run_tag(graph, value_set, signed)
    index, small, digests = CE.pack(graph, W, B, BN, S)
    fs, fd = F[f"{tag}.small"], F[f"{tag}.digests"]
    bad = []
    if small.shape != fs.shape or digests.shape != fd.shape:
        return [f"{tag}: layout {small.shape} {digests.shape} != fixture {fs.shape} {fd.shape}"]
    for name, a, b in index:
        if a >= 0:
            msg = CE.first_difference(f"{tag} {name} (vs fixture)", small[a:b], fs[a:b])
        else:
            msg = "" if (digests[b] == fd[b]).all() else f"{tag} {name}: digest differs from the fixture's"
        if msg:
            bad.append(msg)
    want = F[f"{tag}.diffs"].tolist()
    if list(diffs) != want:
        bad.append(f"{tag} diffs: got {list(diffs)!r}, fixture {want!r}")
    return bad


def oracle_run(graph, value_set, signed):
    """(g, rels, (W, B, BN, S, diffs)) of the oracle's replay of ITERATIONS iterations on host modules."""
    g, rels = edge_graph(graph, value_set, device="cpu")
    return _replay(g, rels, CE.S_MIN_MAX, 2e-7, 20, signed, 0.0, max_iters=CE.ITERATIONS)


@pytest.mark.parametrize("value_set", CE.VALUE_SETS)
@pytest.mark.parametrize("graph", list(CE.GRAPHS))
def test_inputs_are_the_fixtures(graph, value_set):
    """A drifting value builder is told from a drifting result."""
    assert CE.input_digest(graph, value_set) == str(cle_edge()[f"{graph}.{value_set}.inputs"])


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("value_set", CE.VALUE_SETS)
@pytest.mark.parametrize("graph", list(CE.GRAPHS))
def test_oracle_replay_matches_reference(graph, value_set, signed):
    W, B, BN, S, diffs = oracle_run(graph, value_set, signed)
    assert len(diffs) == CE.ITERATIONS
    bad = fixture_mismatches(graph, value_set, signed, W, B, BN, S, diffs)
    assert not bad, "\n".join(bad[:20])
