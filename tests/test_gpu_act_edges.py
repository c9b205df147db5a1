"""The three kernels under set_quant_minmax (csrc/dfq_act.hip: dfq_act_moments,
dfq_act_minmax, dfq_act_affine) at their edges, per element
(cases: tests/act_edge_cases.py):

  * dfq_act_moments against the CPU oracle bit for bit: all three kinds (ReLU6
    included), sqrt_w, accumulate, the aliased in-place form, every length from
    one element to the second trip of the grid-stride loop;
  * dfq_act_minmax against the oracle (which tests/test_oracle_act_edges.py holds
    to torch.min / torch.max): every length, the extreme and a NaN at every lane /
    wave / trip boundary of its single block, NaN through the square root only,
    infinities; the result lands in one slot of a larger buffer;
  * dfq_act_affine exactly on small integers and within the derived bound of a
    float64 evaluation on multi-binade values: groups, KH*KW around
    aten_inner_sum's branches, i2 around the wave, no bias;
  * the walk itself on the device (the batched record / replay path) on the tiny
    models of tests/golden/act_edge_cases.npz: every quantizer's range equals the
    reference's, (nan, nan) included;
  * the C entry points' argument checks.

The kernel-vs-oracle comparisons rest on the device's double exp / erf / erfc and
the host libm rounding to the same fp32 value, as dfq_bc_expect's test does.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn

from data_free_quantization_amd import _lib
from oracle import oracle as O
from tests import act_edge_cases as AE
from tests.bc_edge_cases import values
from tests.helpers import act_edge, h
from tests.test_oracle_act_edges import same_per_channel, same_scalar

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TARG = (nn.Conv2d, nn.Linear)
EPS = AE.EPS
SENTINEL = np.float32(-12345.5)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.cpu().numpy()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _moments(w, b, n, kind, sqrt_w, acc, mean, var):
    rc = _lib.load().dfq_act_moments(_lib.ptr(w), _lib.ptr(b), n, kind, int(sqrt_w), EPS, int(acc), _lib.ptr(mean),
                                     _lib.ptr(var), _stream())
    _lib.check(rc, "dfq_act_moments")


# ---- dfq_act_moments ----------------------------------------------------------
def _moment_inputs(n, sqrt_w):
    """(w, b): BN statistics (a quarter of the weights negative) or, for sqrt_w, a
    (variance, mean) pair as _moments_inplace sees it: the ReLU moments of the
    statistics, whose variances go below -eps in some channels."""
    w, b = AE.stats(n, seed=n % 97)
    if not sqrt_w:
        return w, b
    mean, var = O.act_moments(np.abs(w), b, 1)
    if n >= 1031:
        assert (var.astype(np.float64) + np.float32(EPS) < 0).any()
    return var, mean


@pytest.mark.parametrize("kind", [0, 1, 2], ids=["none", "relu", "relu6"])
@pytest.mark.parametrize("n", AE.MOMENT_LENGTHS)
def test_moments_equal_oracle(n, kind):
    for sqrt_w in (False, True):
        w, b = _moment_inputs(n, sqrt_w)
        dw, db = T(w), T(b)
        for acc in (False, True):
            mean0, var0 = values(40 + kind, n, -26, -20), np.abs(values(50 + kind, n, -26, -20))
            if acc:
                want = O.act_moments(w, b, kind, sqrt_w, into=(mean0.copy(), var0.copy()))
            else:
                want = O.act_moments(w, b, kind, sqrt_w)
            mean, var = T(mean0), T(var0)
            _moments(dw, db, n, kind, sqrt_w, acc, mean, var)
            what = f"n={n} kind={kind} sqrt_w={sqrt_w} accumulate={acc}"
            same_per_channel(N(mean), want[0], "mean, " + what)
            same_per_channel(N(var), want[1], "var, " + what)


@pytest.mark.parametrize("kind", [0, 1, 2], ids=["none", "relu", "relu6"])
@pytest.mark.parametrize("n", AE.LENGTHS)
def test_moments_in_place_equal_the_separate_call(n, kind):
    """_moments_inplace's form: w = var, b = mean, the outputs written over the inputs."""
    var0, mean0 = _moment_inputs(n, True)
    dv, dm = T(var0), T(mean0)
    mean, var = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    _moments(dv, dm, n, kind, True, False, mean, var)
    _moments(dv, dm, n, kind, True, False, dm, dv)
    same_per_channel(N(dm), N(mean), "mean")
    same_per_channel(N(dv), N(var), "var")
    want = O.act_moments(var0, mean0, kind, True)
    same_per_channel(N(dm), want[0], "mean vs oracle")
    same_per_channel(N(dv), want[1], "var vs oracle")


@pytest.mark.parametrize("n", [1, 65, 257, 4097])
def test_moments_write_only_their_n_elements(n):
    guard = 7
    w, b = AE.stats(n, seed=5)
    dw, db = T(w), T(b)
    buf = torch.full((2, n + 2 * guard), float(SENTINEL), device=DEV)
    mean, var = buf[0, guard:guard + n], buf[1, guard:guard + n]
    _moments(dw, db, n, 2, False, False, mean, var)
    got = N(buf)
    want = O.act_moments(w, b, 2)
    same_per_channel(got[0, guard:guard + n], want[0], "mean")
    same_per_channel(got[1, guard:guard + n], want[1], "var")
    assert (got[:, :guard] == SENTINEL).all() and (got[:, guard + n:] == SENTINEL).all()   # element n included
    assert np.array_equal(N(dw), w) and np.array_equal(N(db), b)


# ---- dfq_act_minmax -----------------------------------------------------------
@pytest.mark.parametrize("w_is_var", [False, True], ids=["std", "var"])
@pytest.mark.parametrize("case", AE.MINMAX_CASES, ids=[c.name for c in AE.MINMAX_CASES])
def test_minmax_equals_oracle(case, w_is_var):
    a, w = case.inputs(w_is_var)
    want = O.act_minmax(a, w, AE.N_SIGMA, w_is_var)
    da, dw = T(a), T(w)
    slots, k = 8, 3
    buf = torch.full((2 * slots,), float(SENTINEL), device=DEV)     # as _MinMaxBatch: slot k of one buffer
    rc = _lib.load().dfq_act_minmax(_lib.ptr(da), _lib.ptr(dw), case.n, int(w_is_var), EPS, AE.N_SIGMA,
                                    buf.data_ptr() + 8 * k, _stream())
    _lib.check(rc, "dfq_act_minmax")
    got = N(buf)
    lo, hi = float(got[2 * k]), float(got[2 * k + 1])
    print(case.name, w_is_var, (lo, hi), want)
    assert same_scalar(lo, want[0]) and same_scalar(hi, want[1]), ((lo, hi), want)
    for g_, w_ in ((lo, want[0]), (hi, want[1])):   # the same bits, but for a zero's sign
        if not np.isnan(w_) and w_ != 0:
            assert np.float32(g_).view(np.uint32) == np.float32(w_).view(np.uint32)
    rest = np.delete(got, [2 * k, 2 * k + 1])
    assert (rest == SENTINEL).all()
    if case.nan_both(w_is_var):
        assert np.isnan(lo) and np.isnan(hi)


# ---- dfq_act_affine -----------------------------------------------------------
def _affine(x, W, bias, case, out):
    rc = _lib.load().dfq_act_affine(_lib.ptr(x), _lib.ptr(W), _lib.ptr(bias), case.o, case.i2, case.khw, case.groups,
                                    _lib.ptr(out), _stream())
    _lib.check(rc, "dfq_act_affine")


@pytest.mark.parametrize("case", AE.AFFINE_CASES, ids=[c.name for c in AE.AFFINE_CASES])
def test_affine_exact_on_small_integers(case):
    x, W, bias = case.inputs("int")
    ref, ab = case.exact(x, W, bias)
    assert ab.max() < 2 ** 24       # every partial sum, in any order, is an integer fp32 holds
    out = torch.full((case.o + 1,), float(SENTINEL), device=DEV)
    _affine(T(x), T(W), None if bias is None else T(bias), case, out)
    got = N(out)
    assert np.array_equal(got[:case.o].astype(np.float64), ref)
    assert got[case.o] == SENTINEL


@pytest.mark.parametrize("case", AE.AFFINE_CASES, ids=[c.name for c in AE.AFFINE_CASES])
def test_affine_within_bound_and_reproducible(case):
    """|got - ref| <= (khw + i2 + 2) 2^-24 (sum |W||x| + |bias|) per output: khw adds,
    a product, i2 adds in any order and the bias add.  The same bits run to run and
    with every operand at another address (4 bytes off a 16-byte boundary)."""
    x, W, bias = case.inputs("binade")
    ref, ab = case.exact(x, W, bias)
    dx, dW, db = T(x), T(W), (None if bias is None else T(bias))
    out = torch.full((case.o,), float(SENTINEL), device=DEV)
    _affine(dx, dW, db, case, out)
    got = N(out)
    err = np.abs(got.astype(np.float64) - ref)
    bound = case.bound_ulps * 2.0 ** -24 * ab
    print(case.name, "largest error / bound:", float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all(), (np.flatnonzero(err > bound)[:5], err.max())
    out2 = torch.full((case.o,), float(SENTINEL), device=DEV)
    _affine(dx, dW, db, case, out2)
    assert np.array_equal(N(out2).view(np.uint32), got.view(np.uint32))

    def moved(a):
        buf = torch.full((a.size + 5,), float(SENTINEL), device=DEV)
        buf[1:1 + a.size] = T(a.ravel())
        return buf[1:1 + a.size]

    mx, mW, mb, mo = moved(x), moved(W), (None if bias is None else moved(bias)), moved(np.zeros(case.o, np.float32))
    assert mx.data_ptr() % 16 == 4 and mx.is_contiguous()
    _affine(mx, mW, mb, case, mo)
    assert np.array_equal(N(mo).view(np.uint32), got.view(np.uint32))


# ---- the walk on the device -----------------------------------------------------
@pytest.mark.parametrize("gname", AE.GRAPHS)
def test_walk_on_device_matches_reference(gname, monkeypatch):
    """L.set_quant_minmax on the GPU (the batched record / replay walk) on each tiny
    model: every quantizer's (running_min, running_max) equals the fixture's, NaN
    equal to NaN; a NaN range survives _RangeWrites (its H2D copy and the
    dfq_bc_chain COPY) into the buffers.  The case (d.) quantizer is held within the
    derived bound of its float64 value."""
    from data_free_quantization_amd.utils import layer_transform as L
    from data_free_quantization_amd.utils.quantize import QuantMeasure
    from data_free_quantization_amd.utils.tracer import build_graph
    fx = act_edge()[gname]
    model = AE.build_model(gname)
    assert h(AE.model_inputs(model)) == fx["digest"], "the builder's statistics drifted from the fixture's"
    d_exact = AE.case_d_exact(model) if gname.endswith("case_d") else None
    model = model.cuda()
    g = build_graph(model, "positional")
    graph, bottoms = g.getGraph(), g.getBottoms()
    tkeys = [k for k in graph if type(graph[k]) in TARG]
    assert tkeys == fx["targets"]
    for k in tkeys:
        graph[k].quant = QuantMeasure(num_bits=8).cuda()
    monkeypatch.setattr(L, "module_tensor_op", L.CustomTensorOP(graph, bottoms).cuda())
    assert L.module_tensor_op.names == fx["op_keys"]
    mods = [graph[k].quant for k in tkeys] + list(L.module_tensor_op.quants)
    for q in mods:
        q.running_min.fill_(float(SENTINEL))
        q.running_max.fill_(float(SENTINEL))
    fetched = []
    fetch = L._MinMaxBatch.fetch
    monkeypatch.setattr(L._MinMaxBatch, "fetch", lambda self: (fetched.append(self.n), fetch(self))[1])
    L.merge_batchnorm(model, graph, bottoms, TARG)
    L.set_quant_minmax(graph, bottoms, verbose=False)
    torch.cuda.synchronize()
    assert len(fetched) == 1 and fetched[0] > 0, "the walk did not take the batched path"
    bad = []
    for i, q in enumerate(mods):
        got = (float(q.running_min), float(q.running_max))
        want = (float(fx["min"][i]), float(fx["max"][i]))
        if any(q is c for c in L.CASE_D):
            lo, hi, tol = d_exact
            print(gname, "case (d.):", got, "float64:", (lo, hi), "tol", tol, "reference:", want)
            assert abs(got[0] - lo) <= tol and abs(got[1] - hi) <= tol, (got, lo, hi, tol)
        elif not (same_scalar(got[0], want[0]) and same_scalar(got[1], want[1])):
            bad.append((i, got, want))
    assert not bad, bad
    if gname.endswith("case_d"):
        assert len(L.CASE_D) == 1
    elif gname.startswith("nan."):
        head = graph[tkeys[-1]].quant
        assert bool(torch.isnan(head.running_min)) and bool(torch.isnan(head.running_max))


# ---- argument checks ------------------------------------------------------------
def test_argument_checks():
    lib = _lib.load()
    INVALID, OK = _lib.DFQ_ERR_INVALID, _lib.DFQ_OK
    n = 8
    a, b = torch.ones(n, device=DEV), torch.ones(n, device=DEV)
    m, v = torch.full((n,), float(SENTINEL), device=DEV), torch.full((n,), float(SENTINEL), device=DEV)
    out2 = torch.full((2,), float(SENTINEL), device=DEV)
    p = _lib.ptr
    s = _stream()
    for args in ((None, p(b), n, 1, 0, EPS, 0, p(m), p(v)), (p(a), None, n, 1, 0, EPS, 0, p(m), p(v)),
                 (p(a), p(b), n, 1, 0, EPS, 0, None, p(v)), (p(a), p(b), n, 1, 0, EPS, 0, p(m), None),
                 (p(a), p(b), n, 3, 0, EPS, 0, p(m), p(v)), (p(a), p(b), n, -1, 0, EPS, 0, p(m), p(v)),
                 (p(a), p(b), -1, 1, 0, EPS, 0, p(m), p(v))):
        assert lib.dfq_act_moments(*args, s) == INVALID, args
    assert lib.dfq_act_moments(p(a), p(b), 0, 2, 0, EPS, 0, p(m), p(v), s) == OK     # n == 0: nothing to do
    for args in ((None, p(b), n, 0, EPS, 6.0, p(out2)), (p(a), None, n, 0, EPS, 6.0, p(out2)),
                 (p(a), p(b), n, 0, EPS, 6.0, None), (p(a), p(b), 0, 0, EPS, 6.0, p(out2)),
                 (p(a), p(b), -1, 0, EPS, 6.0, p(out2))):
        assert lib.dfq_act_minmax(*args, s) == INVALID, args
    # x [4], W [4, 2, 1] (groups 2): o, i2, khw, groups
    W, o = torch.ones(8, device=DEV), torch.full((4,), float(SENTINEL), device=DEV)
    for args in ((None, p(W), p(b), 4, 2, 1, 2, p(o)), (p(a), None, p(b), 4, 2, 1, 2, p(o)),
                 (p(a), p(W), p(b), 4, 2, 1, 2, None), (p(a), p(W), p(b), 4, 2, 1, 3, p(o)),
                 (p(a), p(W), p(b), 4, 2, 0, 2, p(o)), (p(a), p(W), p(b), 0, 2, 1, 2, p(o)),
                 (p(a), p(W), p(b), 4, 0, 1, 2, p(o)), (p(a), p(W), p(b), 4, 2, 1, 0, p(o)),
                 (p(a), p(W), p(b), -4, 2, 1, 2, p(o))):
        assert lib.dfq_act_affine(*args, s) == INVALID, args
    torch.cuda.synchronize()
    for t in (m, v, out2, o):       # no rejected call, and no n == 0 call, wrote anything
        assert (N(t) == SENTINEL).all()
