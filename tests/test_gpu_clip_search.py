"""clip_weight.clip_search (dfq_clip_search_batch) on the GPU against the CPU
statement of tests/clip_search_cases.py (C oracle quantize on the clamped array,
math.fsum of the exact fp64 squares).

Choices, ranges and clamped weights are compared for equality; the statement
checks on the CPU that no choice hangs on a rounding (every runner-up is more than
1e-12 above its best, far beyond the sums' error).  Noise sums: every term is a
non-negative exact double, so any summation order of n terms is within
(n-1) 2^-53 / (1 - (n-1) 2^-53) of the exact sum, relative; the tolerance n 2^-52
is twice that (tests/test_gpu_pair_stats.py), and so also bounds the difference of
two such sums of the same terms (the search's and quality.pair_stats').
"""
import numpy as np
import pytest
import torch

from tests import clip_search_cases as CC

pytestmark = pytest.mark.gpu


def _place(a, dev, off):
    """``a`` on the device, starting ``off`` floats into a larger (aligned) buffer."""
    buf = torch.zeros(a.size + 8, dtype=torch.float32, device=dev)
    v = buf[off:off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * off
    return v


def _items(cases, dev, dry=False):
    from data_free_quantization_amd.clip_weight import ClipItem
    out = []
    for c in cases:
        enc = None if c.per_channel else torch.full((2,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
        out.append(ClipItem(_place(c.x, dev, c.offset), bits=c.bits, per_channel=c.per_channel, symmetric=c.symmetric,
                            candidates=c.K, min_frac=c.min_frac, dry=dry, range_enc=enc))
    return out


def _host(items, res):
    torch.cuda.synchronize()
    return [{"choice": r["choice"].cpu().numpy(), "range": r["range"].cpu().numpy(), "noise": r["noise"].cpu().numpy(),
             "w": it.w.cpu().numpy(), "enc": None if it.range_enc is None else it.range_enc.cpu().numpy()}
            for it, r in zip(items, res)]


def _decode(e):
    """dfq_range's ordered encoding -> float32."""
    e = np.uint32(e)
    u = (e & np.uint32(0x7fffffff)) if (e & np.uint32(0x80000000)) else ~e
    return np.array([u], dtype=np.uint32).view(np.float32)[0]


@pytest.fixture(scope="module")
def world():
    """Every case once: one call over the whole list, one over the reversed list,
    one per case alone and one dry call; then the sweep on the clamped and on the
    unclamped weights, and pair_stats of both against the originals."""
    from data_free_quantization_amd import quality
    from data_free_quantization_amd.clip_weight import clip_search
    from data_free_quantization_amd.sweep import SweepItem, SweepPlan
    dev = torch.device("cuda:0")
    cases = CC.all_cases()
    CC.check_preconditions(cases)
    items = _items(cases, dev)
    together = _host(items, clip_search(items))
    rev = _items(cases[::-1], dev)
    reverse = _host(rev, clip_search(rev))[::-1]
    alone = []
    for c in cases:
        it = _items([c], dev)
        alone.append(_host(it, clip_search(it))[0])
    dry_items = _items(cases, dev, dry=True)
    dry = _host(dry_items, clip_search(dry_items))

    def sweep(srcs, encs=None):
        its = [SweepItem(src=s, dst=torch.empty_like(s), bits=c.bits, per_channel=c.per_channel, symmetric=c.symmetric,
                         rows=s.shape[0] if c.per_channel else 1,
                         range_enc=None if encs is None else encs[i]) for i, (s, c) in enumerate(zip(srcs, cases))]
        plan = SweepPlan(its)
        plan.execute()
        plan.destroy()
        return [it.dst for it in its]

    orig = [_place(c.x, dev, 0) for c in cases]
    dq_clamped = sweep([it.w for it in items])
    dq_handoff = sweep([it.w for it in items], [it.range_enc for it in items])   # DFQ_DEVICE_RANGE where per tensor
    dq_plain = sweep(orig)
    st_clamped = quality.pair_stats(list(zip(orig, dq_clamped)))
    st_plain = quality.pair_stats(list(zip(orig, dq_plain)))
    torch.cuda.synchronize()

    def noise_of(stats, c):
        return (stats.rows[:, quality.NOISE] if c.per_channel else stats.total[quality.NOISE:quality.NOISE + 1]).cpu().numpy()

    return {"cases": cases, "together": together, "reverse": reverse, "alone": alone, "dry": dry,
            "dq_clamped": [t.cpu().numpy() for t in dq_clamped], "dq_handoff": [t.cpu().numpy() for t in dq_handoff],
            "noise_clamped": [noise_of(s, c) for s, c in zip(st_clamped, cases)],
            "noise_plain": [noise_of(s, c) for s, c in zip(st_plain, cases)]}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _within(got, exact, n):
    return np.abs(got - exact) <= n * 2.0 ** -52 * exact


GROUPS = ["grid_%dx" % r for r in CC.ROWS] + ["tensor_", "int4_", "const_", "single_", "zero_"]


@pytest.mark.parametrize("group", GROUPS)
def test_search_matches_the_statement(group, world):
    seen = 0
    for i, c in enumerate(world["cases"]):
        if not c.name.startswith(group):
            continue
        seen += 1
        got = world["together"][i]
        units, n = c.choice.size, c.unit_len
        assert got["choice"].shape == (units,) and got["range"].shape == (units, 2) and got["noise"].shape == (units, 2)
        # 1. the choice (0 for the tied cases)
        assert np.array_equal(got["choice"], c.choice), (c.name, got["choice"], c.choice)
        if c.tied:
            assert not got["choice"].any(), c.name
        # 2. the range, bitwise
        assert np.array_equal(_bits(got["range"][:, 0]), _bits(c.lo)), c.name
        assert np.array_equal(_bits(got["range"][:, 1]), _bits(c.hi)), c.name
        # 3. both noise figures against fsum
        first, best = c.noise[:, 0], c.noise[np.arange(units), c.choice]
        worst = max(float(np.max(np.abs(got["noise"][:, k] - w)[w > 0] / w[w > 0], initial=0.0))
                    for k, w in ((0, first), (1, best)))
        print(c.name, "bits", c.bits, "K", c.K, "narrowed %d/%d" % ((c.choice > 0).sum(), units),
              "worst relative noise error %.3g (bound %.3g)" % (worst, n * 2.0 ** -52))
        assert _within(got["noise"][:, 0], first, n).all(), c.name
        assert _within(got["noise"][:, 1], best, n).all(), c.name
        # 4. the weights: clamped in place; untouched, bitwise, by a dry call with the same outputs
        assert (got["w"] == c.clamped()).all(), c.name
        d = world["dry"][i]
        assert np.array_equal(_bits(d["w"]), _bits(c.x)), c.name
        for f in ("choice", "range", "noise"):
            assert np.array_equal(_bits(d[f]), _bits(got[f])), (c.name, f)
        if c.per_channel:
            assert got["enc"] is None
        else:
            # 5. range_enc decodes to the min and max of the tensor as the call left it
            assert _decode(~got["enc"].view(np.uint32)[0]) == got["w"].min(), c.name
            assert _decode(got["enc"].view(np.uint32)[1]) == got["w"].max(), c.name
            assert _decode(~d["enc"].view(np.uint32)[0]) == c.x.min() and _decode(d["enc"].view(np.uint32)[1]) == c.x.max()
        # 6. a sweep fed that range_enc (DFQ_DEVICE_RANGE) equals the sweep on the data range
        assert np.array_equal(_bits(world["dq_handoff"][i]), _bits(world["dq_clamped"][i])), c.name
        # 7. the existing sweep on the clamped weights is the candidate as the search evaluated it ...
        assert _within(world["noise_clamped"][i], got["noise"][:, 1], n).all(), (c.name, world["noise_clamped"][i],
                                                                              got["noise"][:, 1])
        assert _within(world["noise_plain"][i], got["noise"][:, 0], n).all(), c.name
        # ... and never noisier than the sweep on the unclamped weights
        assert (world["noise_clamped"][i] <= world["noise_plain"][i] * (1 + n * 2.0 ** -52)).all(), c.name
    assert seen >= 4


def test_results_do_not_depend_on_the_list(world):
    """8. Bit-identical outputs and weights: all weights in one call, the list
    reversed, every weight alone."""
    for i, c in enumerate(world["cases"]):
        for other in ("reverse", "alone"):
            for f in ("choice", "range", "noise", "w"):
                assert np.array_equal(_bits(world["together"][i][f]), _bits(world[other][i][f])), (c.name, other, f)
            if not c.per_channel:
                assert np.array_equal(world["together"][i]["enc"], world[other][i]["enc"]), (c.name, other)


def test_clipping_pays_at_four_bits(world):
    """The INT4 outlier cases: at least half the units narrow their range, and the
    narrowed units' noise is strictly below the min-max range's."""
    for i, c in enumerate(world["cases"]):
        if not c.name.startswith("int4_"):
            continue
        got = world["together"][i]
        k = got["choice"] > 0
        assert 2 * int(k.sum()) >= k.size, c.name
        assert (got["noise"][k, 1] < got["noise"][k, 0]).all(), c.name
        assert (got["noise"][~k, 1] == got["noise"][~k, 0]).all(), c.name


def test_python_errors():
    from data_free_quantization_amd.clip_weight import ClipItem, clip_search
    a = torch.randn(4, 6, device="cuda:0")
    for kw in ({"bits": 1}, {"bits": 17}, {"candidates": 0}, {"candidates": 65}, {"min_frac": -0.1}, {"min_frac": 1.1},
               {"min_frac": float("nan")}):
        with pytest.raises(ValueError, match="invalid list"):
            clip_search([ClipItem(a.clone(), **kw)])
    with pytest.raises(ValueError, match="contiguous"):
        clip_search([ClipItem(a.t())])
    with pytest.raises(TypeError):
        clip_search([ClipItem(a.double())])
    with pytest.raises(TypeError, match="range_enc"):
        clip_search([ClipItem(a.clone(), range_enc=torch.zeros(2, device="cuda:0"))])
    w = a.clone()
    r = clip_search([ClipItem(w, bits=4, per_channel=True, symmetric=True)])[0]
    assert r["choice"].dtype == torch.int32 and r["choice"].shape == (4,) and r["choice"].is_cuda
    assert r["range"].dtype == torch.float32 and r["range"].shape == (4, 2)
    assert r["noise"].dtype == torch.float64 and r["noise"].shape == (4, 2)
