"""set_quant_minmax's statistics on the CPU oracle (oracle/dfq_oracle.c
oracle_act_*) against the REFERENCE per channel (tests/golden/act_edge_cases.npz,
cases in tests/act_edge_cases.py): ReLU6 moments, add merges with two and three
branches, variances below -eps (NaN through torch.sqrt) and case (d.).

The fixture holds what the reference handed to torch.min / torch.max /
torch.sqrt while its set_quant_minmax ran: the per-channel mean - N*w, mean + N*w
and var + eps of every call, in call order.  The project's walk runs here on the
oracle backend of tests/test_oracle_act_range.py, and every statistic call
rebuilds the same vectors in fp32 numpy from its arguments: they equal the
recorded ones bit for bit, NaN positions included.  tests/test_gpu_act_edges.py
holds the HIP kernels to the oracle.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import oracle as O
from tests import act_edge_cases as AE
from tests.helpers import act_edge, h
from tests.test_oracle_act_range import _oracle_backend, _oracle_merge_bn

TARG = (nn.Conv2d, nn.Linear)
F32 = np.float32


def same_per_channel(got, want, what=""):
    """Equal bits in every channel; a NaN matches a NaN (its sign and payload are
    the platform's)."""
    got, want = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(want, dtype=F32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.flatnonzero((gn != wn) | (~gn & ~wn & (got.view(np.uint32) != want.view(np.uint32))))
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} channels differ, first at {bad[:5]}: " \
                          f"{got[bad[:5]]} vs {want[bad[:5]]}"


def same_scalar(got, want):
    """By value, NaN equal to NaN (a zero's sign out of torch.min / torch.max depends
    on the reduction order: make_golden.h)."""
    return (np.isnan(got) and np.isnan(want)) or got == want


class _Recorded:
    """The reference's recorded vectors, consumed in call order."""

    def __init__(self, rec):
        self.rec, self.at, self.case_d = rec, 0, False

    def take(self, kind, vec, what):
        assert self.at < len(self.rec), f"{what}: the reference made only {len(self.rec)} calls"
        k, want = self.rec[self.at]
        assert k == kind, f"call {self.at} ({what}): the reference called kind {k}, the walk kind {kind}"
        same_per_channel(vec, want, f"call {self.at} ({what})")
        self.at += 1


def _checked_backend(monkeypatch, L, rec):
    """The oracle backend with every statistic call's vectors held to ``rec``."""
    _oracle_backend(monkeypatch, L)
    moments_inplace, minmax, get_max, get_min = L._moments_inplace, L._minmax, L._get_max_value, L._get_min_value
    eps = F32(AE.EPS)

    def checked_inplace(mean, var, kind):
        arg = var.numpy() + eps
        rec.take(AE.REC_SQRT, arg, "sqrt(var + eps) for the mean")     # calculate_mean(_6)(torch.sqrt(var + eps), ..)
        rec.take(AE.REC_SQRT, arg, "sqrt(var + eps) for the variance")
        moments_inplace(mean, var, kind)

    def checked_minmax(a, w, n_sigma, w_is_var=False):
        an, wn = a.detach().numpy(), w.detach().numpy()
        if not rec.case_d:     # (case (d.)'s vectors reach torch as [1, C, 1, 1]: not recorded)
            if w_is_var:
                with np.errstate(invalid="ignore"):
                    sw = np.sqrt(wn + eps)
                rec.take(AE.REC_SQRT, wn + eps, "sqrt(var + eps) for the min")
                rec.take(AE.REC_MIN, an - F32(n_sigma) * sw, "mean - N*std")
                rec.take(AE.REC_SQRT, wn + eps, "sqrt(var + eps) for the max")
                rec.take(AE.REC_MAX, an + F32(n_sigma) * sw, "mean + N*std")
            else:
                rec.take(AE.REC_MIN, an - F32(n_sigma) * wn, "bias - N*weight")
                rec.take(AE.REC_MAX, an + F32(n_sigma) * wn, "bias + N*weight")
        return minmax(a, w, n_sigma, w_is_var)

    def in_case_d(fn):
        def wrapped(bias, weight, n):
            rec.case_d = True
            try:
                return fn(bias, weight, n)
            finally:
                rec.case_d = False
        return wrapped

    monkeypatch.setattr(L, "_moments_inplace", checked_inplace)
    monkeypatch.setattr(L, "_minmax", checked_minmax)
    monkeypatch.setattr(L, "_get_max_value", in_case_d(get_max))
    monkeypatch.setattr(L, "_get_min_value", in_case_d(get_min))


def test_population_self_check():
    neg = AE.self_check()
    print("channels with a variance below -eps (ReLU, ReLU6):", neg, "of", AE.POP_N)


@pytest.mark.parametrize("gname", AE.GRAPHS)
def test_walk_with_oracle_matches_reference_per_channel(gname, monkeypatch):
    """Every vector the reference reduced or took the root of, and every quantizer's
    (min, max), NaN equal to NaN."""
    from data_free_quantization_amd.utils import layer_transform as L
    from data_free_quantization_amd.utils.quantize import QuantMeasure
    from data_free_quantization_amd.utils.tracer import build_graph
    fx = act_edge()[gname]
    model = AE.build_model(gname)
    assert h(AE.model_inputs(model)) == fx["digest"], "the builder's statistics drifted from the fixture's"
    d_exact = AE.case_d_exact(model) if gname.endswith("case_d") else None
    g = build_graph(model, "positional")
    graph, bottoms = g.getGraph(), g.getBottoms()
    tkeys = [k for k in graph if type(graph[k]) in TARG]
    assert tkeys == fx["targets"]
    for k in tkeys:
        graph[k].quant = QuantMeasure(num_bits=8)
    monkeypatch.setattr(L, "module_tensor_op", L.CustomTensorOP(graph, bottoms))
    assert L.module_tensor_op.names == fx["op_keys"]
    rec = _Recorded(fx["rec"])
    _checked_backend(monkeypatch, L, rec)
    _oracle_merge_bn(graph, bottoms)
    L.set_quant_minmax(graph, bottoms, verbose=False)
    assert rec.at == len(rec.rec), f"the walk made {rec.at} of the reference's {len(rec.rec)} calls"
    mods = [graph[k].quant for k in tkeys] + list(L.module_tensor_op.quants)
    assert len(mods) == len(fx["min"])
    bad = []
    for i, q in enumerate(mods):
        got = (float(q.running_min), float(q.running_max))
        want = (float(fx["min"][i]), float(fx["max"][i]))
        if any(q is c for c in L.CASE_D):
            lo, hi, tol = d_exact
            # the reference's own MKL GEMV and the oracle: both inside the derived bound
            assert abs(want[0] - lo) <= tol and abs(want[1] - hi) <= tol, (want, lo, hi, tol)
            assert abs(got[0] - lo) <= tol and abs(got[1] - hi) <= tol, (got, lo, hi, tol)
        elif not (same_scalar(got[0], want[0]) and same_scalar(got[1], want[1])):
            bad.append((i, got, want))
    assert not bad, bad
    if gname.endswith("case_d"):
        assert len(L.CASE_D) == 1
    elif gname.startswith("nan."):   # the head's range: the reference's (nan, nan)
        head = len(tkeys) - 1
        assert np.isnan(fx["min"][head]) and np.isnan(fx["max"][head])


@pytest.mark.parametrize("w_is_var", [False, True], ids=["std", "var"])
@pytest.mark.parametrize("case", AE.MINMAX_CASES, ids=[c.name for c in AE.MINMAX_CASES])
def test_oracle_minmax_is_torch_min_max(case, w_is_var):
    """oracle_act_minmax against torch.min / torch.max of the vectors built in fp32
    numpy: NaN propagates as torch propagates it, infinities stay."""
    a, w = case.inputs(w_is_var)
    with np.errstate(invalid="ignore"):
        sw = np.sqrt(w + F32(AE.EPS)) if w_is_var else w
        lo, hi = a - F32(AE.N_SIGMA) * sw, a + F32(AE.N_SIGMA) * sw
    want = float(torch.min(torch.from_numpy(lo))), float(torch.max(torch.from_numpy(hi)))
    got = O.act_minmax(a, w, AE.N_SIGMA, w_is_var)
    assert same_scalar(got[0], want[0]) and same_scalar(got[1], want[1]), (got, want)
    if case.nan_both(w_is_var):
        assert np.isnan(got[0]) and np.isnan(got[1])
    elif case.what == "inf_minus_inf":
        assert np.isnan(got[0]) and got[1] == np.inf
    else:
        assert not np.isnan(got[0]) and not np.isnan(got[1])


@pytest.mark.parametrize("case", AE.AFFINE_CASES, ids=[c.name for c in AE.AFFINE_CASES])
def test_oracle_affine(case):
    """oracle_act_affine: exact on small integers, inside the derived bound of a
    float64 evaluation on the multi-binade values."""
    x, W, bias = case.inputs("int")
    ref, ab = case.exact(x, W, bias)
    assert ab.max() < 2 ** 24
    got = O.act_affine(x, W, bias, case.groups)
    assert np.array_equal(got.astype(np.float64), ref)
    x, W, bias = case.inputs("binade")
    ref, ab = case.exact(x, W, bias)
    got = O.act_affine(x, W, bias, case.groups)
    assert (np.abs(got.astype(np.float64) - ref) <= case.bound_ulps * 2.0 ** -24 * ab).all()
