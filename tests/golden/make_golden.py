"""Generate the golden fixtures under tests/golden/ by running the REFERENCE's own
DFQ modules (KadAMRN/Data_Free_Quantization at /root/reference) on seeded inputs.

Run only in the development container (the reference never travels):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden.py

Outputs (all plain arrays, loadable with numpy allow_pickle=False):
  quant_cases.npz     quantize()/UniformQuantize on unit and edge-case tensors,
                      per-tensor (reference call shape of utils/layer_transform.py:298)
                      and per-channel (reference quantize() per W[o] slice)
  chunk_cases.npz     quantize() with min/max None and num_chunks (the chunked
                      data range, utils/quantize.py:25-37)
  transform_cases.npz merge_batchnorm, _layer_equalization, bias_absorption,
                      bias_correction helpers on small layers
  bc_edge_cases.npz   the bias-correction helpers at the HIP kernels' reduction edges
                      (cases and inputs: tests/bc_edge_cases.py; section ``bc_edge``)
  act_edge_cases.npz  set_quant_minmax on tiny add / case (d.) models, per channel, ReLU6
                      and NaN included (tests/act_edge_cases.py; section ``act_edge``)
  cle_edge_cases.npz  _layer_equalization, relation by relation, and the loop's metric for
                      three iterations on the graphs of tests/cle_edge_cases.py (section
                      ``cle_edge``)
  pipeline_<model>.npz  main_dfq stage order on the synthetic models of
                      data_free_quantization_amd.zoo (positional graph keys)
The synthetic model weights come from zoo.init_synthetic (numpy PCG64), so the
GPU box rebuilds identical inputs without the reference.
"""
from __future__ import annotations

import copy
import hashlib
import json
import os
import sys
import time
from collections import OrderedDict
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn

# The reference's torch.sqrt (BN fold, CLE) runs through MKL VML in HA mode, whose
# rounding depends on MKL's code path: on AVX-512 hosts 0.65% of results come out
# 1 ulp below the IEEE value, on the AVX2 path they are IEEE-exact.  Pin MKL's
# conditional-numerical-reproducibility mode to AVX2 so the fixtures are the
# reference's arithmetic with IEEE sqrt (checked below).
if not os.environ.get("DFQ_MKL_DEFAULT"):
    os.environ.setdefault("MKL_CBWR", "AVX2")
REF = Path(os.environ.get("DFQ_REFERENCE", "/root/reference"))
HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
# where the fixtures are written (DFQ_GOLDEN_OUT: a scratch directory, for the
# regeneration check in tests/test_golden_regen.py); the committed ones are read
# from HERE
OUT = Path(os.environ.get("DFQ_GOLDEN_OUT", str(HERE)))
sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(REF))

from utils.quantize import quantize as ref_quantize  # noqa: E402  (reference)
from utils.layer_transform import merge_batchnorm as ref_merge_bn, quantize_targ_layer as ref_qtl  # noqa: E402
from utils.relation import create_relation as ref_create_relation, Relation as RefRelation  # noqa: E402
import Cross_layer_equal as ref_cle  # noqa: E402
from bias_absorption import bias_absorption as ref_absorb  # noqa: E402
from clip_weight import clip_weight as ref_clip  # noqa: E402
import bias_correction as ref_bc  # noqa: E402

from data_free_quantization_amd import zoo  # noqa: E402
from data_free_quantization_amd.utils.tracer import build_graph  # noqa: E402

TARG = (nn.Conv2d, nn.Linear)


def _check_ieee_sqrt():
    x = np.random.default_rng(0).uniform(0.5, 4, 1 << 20).astype(np.float32)
    bad = int((torch.sqrt(torch.from_numpy(x)).numpy() != np.sqrt(x)).sum())
    assert bad == 0, f"torch.sqrt is not IEEE-exact under MKL_CBWR={os.environ.get('MKL_CBWR')} ({bad} differ)"


def h(a) -> str:
    """sha256 of fp32 bytes with -0 folded to +0 (zero signs are reduction-order
    dependent in torch.min/max)."""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32)) + np.float32(0.0)
    return hashlib.sha256(a.tobytes()).hexdigest()


def t2n(t):
    return t.detach().cpu().numpy().astype(np.float32).copy()


# ---------------------------------------------------------------------------
# quantize() cases
# ---------------------------------------------------------------------------
def quant_cases():
    rng = np.random.Generator(np.random.PCG64(1234))
    arrays, meta, inputs = {}, [], {}

    def add(name, x, bits, mode, **kw):
        x = np.ascontiguousarray(x, dtype=np.float32)
        xt = torch.from_numpy(x.copy())
        sym = mode in ("tensor_sym", "channel_sym")
        given = kw.get("given")
        default_range = kw.get("default_range", False)
        clip = kw.get("clip")
        if mode.startswith("tensor"):
            if given is not None:
                out = ref_quantize(xt, bits, given[0], given[1], symmetric=sym)
            elif default_range:
                out = ref_quantize(xt, bits, symmetric=sym)
            else:
                out = ref_quantize(xt, bits, float(xt.min()), float(xt.max()), symmetric=sym)
        else:
            out = torch.empty_like(xt)
            for o in range(xt.shape[0]):
                sl = xt[o].clone()
                out[o] = ref_quantize(sl, bits, float(sl.min()), float(sl.max()), symmetric=sym)
        if clip is not None:   # clip_weight after quantize (main_dfq.py:214-227)
            out = out.clamp_(clip[0], clip[1])
        khw = kw.get("khw", 1)
        idx = len(meta)
        xi = inputs.setdefault(h(x) + str(x.shape), len(inputs))
        if f"in{xi}" not in arrays:
            arrays[f"in{xi}"] = x
        dq = t2n(out)
        if dq.size <= 2048:
            arrays[f"dq{idx}"] = dq
        arrays[f"dqh{idx}"] = np.array(h(dq))
        if kw.get("esum"):
            eps = out - xt   # bias_correction.py:128-131 on the fused output
            o = x.shape[0]
            arrays[f"esum{idx}"] = t2n(torch.sum(eps.view(o, -1, khw), -1)).reshape(-1)
        meta.append(dict(name=name, input=xi, bits=bits, mode=mode, given=given, default_range=default_range,
                         clip=clip, khw=khw, esum=bool(kw.get("esum")), shape=list(x.shape)))

    shapes = [(32, 3, 3, 3), (96, 16, 1, 1), (64, 1, 3, 3), (10, 7), (1000,), (24, 144, 1, 1), (3, 4100)]
    for shp in shapes:
        x = rng.normal(0, 0.3, shp)
        khw = shp[2] * shp[3] if len(shp) == 4 else 1
        for bits in (8, 4):
            for mode in ("tensor_asym", "tensor_sym", "channel_asym", "channel_sym"):
                if mode.startswith("channel") and len(shp) == 1:
                    continue
                add(f"rand{shp}", x, bits, mode, khw=khw, esum=len(shp) > 1)
    x = rng.normal(0, 1, (16, 32, 3, 3))
    for bits in (2, 5, 16):
        add("bits", x, bits, "tensor_asym", khw=9, esum=True)
        add("bits", x, bits, "channel_sym", khw=9, esum=True)
    # edge cases
    add("const", np.full((8, 9), 0.3), 8, "tensor_asym")
    add("const_ch", np.full((8, 9), -1.7), 8, "channel_asym")
    add("zeros", np.zeros((4, 16)), 8, "tensor_sym")
    add("zeros_asym", np.zeros((4, 16)), 8, "channel_asym")
    add("tiny_range", (1.0 + np.arange(64) * 1e-9).reshape(8, 8), 8, "tensor_asym")
    add("huge", rng.normal(0, 1e30, (4, 64)), 8, "tensor_asym")
    add("denorm", rng.normal(0, 1e-39, (4, 64)), 8, "tensor_sym")
    sz = np.array([0.0, -0.0, 1.0, -1.0, 0.5, -0.5] * 4, dtype=np.float32).reshape(4, 6)
    add("signed_zero", sz, 8, "tensor_asym")
    add("signed_zero_sym", sz, 8, "tensor_sym")
    # exact ties: x = mn + (k + 1/2) * s with s a power of two
    s = 2.0 ** -6
    ties = (-1.0 + (np.arange(256) + 0.5) * s).astype(np.float32)
    ties[0], ties[-1] = -1.0, -1.0 + 255 * s
    add("ties", ties.reshape(16, 16), 8, "tensor_asym")
    add("ties_sym", (np.arange(-127, 128) * 0.5 * 2.0 ** -5).astype(np.float32).reshape(15, 17), 8, "tensor_sym")
    # given (Python double) ranges, default ranges (0-d fp32 tensors)
    x = rng.normal(0, 0.5, (32, 50))
    add("given", x, 8, "tensor_asym", given=(-0.123456789012345, 0.987654321098765))
    add("given_sym", x, 8, "tensor_sym", given=(-1.3, 0.7))
    add("default_range", x, 8, "tensor_asym", default_range=True)
    add("default_range_sym", x, 8, "tensor_sym", default_range=True)
    add("default_range_b16", x, 16, "tensor_asym", default_range=True)
    # clip after quantize
    x = rng.normal(0, 0.2, (48, 24, 3, 3))
    add("clip", x, 8, "tensor_asym", clip=(-0.1, 0.1), khw=9, esum=True)
    add("clip_ch", x, 4, "channel_sym", clip=(-0.25, 0.3), khw=9, esum=True)
    arrays["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(OUT / "quant_cases.npz", **arrays)
    print("quant cases:", len(meta))


def chunk_cases():
    """quantize() with min/max None and num_chunks (utils/quantize.py:25-37): the
    range is the mean over x.view(B // num_chunks, -1)'s rows of each row's min /
    max (0-d fp32 tensors); one bound may be given as a Python float."""
    rng = np.random.Generator(np.random.PCG64(4321))
    arrays, meta = {}, []
    specs = [((32, 3, 5, 5), 16), ((32, 3, 5, 5), 8), ((32, 3, 5, 5), 4), ((32, 3, 5, 5), 1), ((32, 3, 5, 5), 32),
             ((1000, 7), 1), ((64, 40), 2), ((48, 33), 3), ((20, 6), 40), ((18, 5), 4)]
    for k, (shp, nc) in enumerate(specs):
        x = np.ascontiguousarray(rng.normal(0, 0.4, shp), dtype=np.float32)
        arrays[f"in{k}"] = x
        for bits in (8, 4):
            for sym in (False, True):
                for given in (None, ("min", -0.25), ("max", 0.3), ("max", 3.3000015069999997), ("min", -3.3000015069999997)):
                    if given is not None and (bits != 8 or k % 3):
                        continue
                    xt = torch.from_numpy(x.copy())
                    kw = {} if given is None else {f"{given[0]}_value": given[1]}
                    idx = len(meta)
                    entry = dict(input=k, shape=list(shp), num_chunks=nc, bits=bits, sym=sym,
                                 given=None if given is None else list(given), error=None)
                    try:
                        out = ref_quantize(xt, bits, symmetric=sym, num_chunks=nc, **kw)
                    except Exception as e:   # the reference's own error (e.g. view(0, -1))
                        entry["error"] = type(e).__name__
                        meta.append(entry)
                        continue
                    y = xt.view(shp[0] // nc, -1)
                    arrays[f"range{idx}"] = np.array([float(y.min(-1)[0].mean(-1)), float(y.max(-1)[0].mean(-1))],
                                                     dtype=np.float32)
                    dq = t2n(out)
                    arrays[f"dq{idx}"] = dq
                    arrays[f"dqh{idx}"] = np.array(h(dq))
                    meta.append(entry)
    arrays["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(OUT / "chunk_cases.npz", **arrays)
    print("chunk cases:", len(meta), "errors:", sum(m["error"] is not None for m in meta))


# ---------------------------------------------------------------------------
# transform cases
# ---------------------------------------------------------------------------
def _bn(c, rng):
    bn = nn.BatchNorm2d(c)
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, c).astype(np.float32)))
        bn.bias.copy_(torch.from_numpy(rng.normal(0, 0.5, c).astype(np.float32)))
        bn.running_mean.copy_(torch.from_numpy(rng.normal(0, 0.1, c).astype(np.float32)))
        bn.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 2.0, c).astype(np.float32)))
    return bn


def _conv(o, i, k, rng, groups=1, bias=False):
    c = nn.Conv2d(i, o, k, padding=k // 2, groups=groups, bias=bias)
    with torch.no_grad():
        c.weight.copy_(torch.from_numpy(rng.normal(0, 0.3, c.weight.shape).astype(np.float32)))
        if bias:
            c.bias.copy_(torch.from_numpy(rng.normal(0, 0.1, o).astype(np.float32)))
    return c


def transform_cases():
    rng = np.random.Generator(np.random.PCG64(99))
    A, meta = {}, {}

    # merge_batchnorm on conv(no bias)->bn, conv(bias)->bn, linear->? (linear has no BN)
    for tag, (o, i, k, bias) in {"bnfold_a": (24, 16, 3, False), "bnfold_b": (40, 8, 1, True)}.items():
        conv, bn = _conv(o, i, k, rng, bias=bias), _bn(o, rng)
        A[f"{tag}_w"], A[f"{tag}_b"] = t2n(conv.weight), (t2n(conv.bias) if bias else np.zeros(o, np.float32))
        A[f"{tag}_g"], A[f"{tag}_beta"] = t2n(bn.weight), t2n(bn.bias)
        A[f"{tag}_m"], A[f"{tag}_v"] = t2n(bn.running_mean), t2n(bn.running_var)
        graph = OrderedDict([("Data", "Data"), (1, conv), (2, bn)])
        bottoms = OrderedDict([("Data", None), (1, ["Data"]), (2, [1])])
        ref_merge_bn(None, graph, bottoms, TARG)
        A[f"{tag}_w_out"], A[f"{tag}_b_out"] = t2n(conv.weight), t2n(conv.bias)
        A[f"{tag}_fw"], A[f"{tag}_fb"] = t2n(bn.fake_weight), t2n(bn.fake_bias)
        A[f"{tag}_bn_after"] = np.stack([t2n(bn.weight), t2n(bn.bias), t2n(bn.running_mean), t2n(bn.running_var)])
        meta[tag] = dict(eps=1e-5)

    # _layer_equalization
    cle = {
        "cle_dense": ((16, 8, 3), (24, 16, 1), 1, False),
        "cle_pw_dw": ((32, 16, 1), (32, 1, 3), 32, False),
        "cle_dw_pw": ((32, 1, 3), (24, 32, 1), 1, False),
        "cle_signed": ((16, 8, 3), (12, 16, 3), 1, True),
        "cle_dead": ((8, 4, 1), (6, 8, 1), 1, False),
        "cle_linear": ((20, 12, 1), (10, 20, 0), 1, False),
        "cle_grouped2": ((16, 8, 1), (8, 8, 1), 2, False),
    }
    for tag, ((o1, i1, k1), (o2, i2, k2), g2, signed) in cle.items():
        if k2 == 0:
            w1 = torch.from_numpy(rng.normal(0, 0.3, (o1, i1)).astype(np.float32))
            w2 = torch.from_numpy(rng.normal(0, 0.3, (o2, i2)).astype(np.float32))
        else:
            w1 = torch.from_numpy(rng.normal(0, 0.3, (o1, i1, k1, k1)).astype(np.float32))
            w2 = torch.from_numpy(rng.normal(0, 0.3, (o2, i2 if g2 == 1 else o1 // g2, k2, k2)).astype(np.float32))
        if tag == "cle_dead":
            w1[3].zero_()
            w2[:, 5].zero_()
        if tag == "cle_grouped2":   # conv(16)->conv(groups=2: W2 [8, 8, 1, 1])
            w2 = torch.from_numpy(rng.normal(0, 0.3, (8, 8, 1, 1)).astype(np.float32))
        b1 = torch.from_numpy(rng.normal(0, 0.1, o1).astype(np.float32))
        bnw = torch.from_numpy(rng.uniform(0.5, 1.5, o1).astype(np.float32))
        bnb = torch.from_numpy(rng.normal(0, 0.5, o1).astype(np.float32))
        A[f"{tag}_in"] = np.concatenate([t2n(w1).ravel(), t2n(w2).ravel()])
        A[f"{tag}_w1"], A[f"{tag}_w2"] = t2n(w1), t2n(w2)
        A[f"{tag}_b1"], A[f"{tag}_bnw"], A[f"{tag}_bnb"] = t2n(b1), t2n(bnw), t2n(bnb)
        W1, W2, B1, S = ref_cle._layer_equalization(w1, w2, b1, bnw, bnb, s_min_max=[1e-8, 1e8], signed=signed)
        A[f"{tag}_w1_out"], A[f"{tag}_w2_out"], A[f"{tag}_b1_out"] = t2n(W1), t2n(W2), t2n(B1)
        A[f"{tag}_bnw_out"], A[f"{tag}_bnb_out"], A[f"{tag}_S"] = t2n(bnw), t2n(bnb), t2n(S)
        meta[tag] = dict(signed=signed)

    # bias_absorption: conv1 -> bn -> relu -> conv2 (dense and depthwise second layer)
    for tag, (c1, w2shape, groups) in {"absorb_dense": (24, (16, 24, 3, 3), 1),
                                       "absorb_dw": (32, (32, 1, 3, 3), 32)}.items():
        conv1 = _conv(c1, 8, 1, rng, bias=True)
        conv2 = nn.Conv2d(c1, w2shape[0], 3, padding=1, groups=groups, bias=True)
        with torch.no_grad():
            conv2.weight.copy_(torch.from_numpy(rng.normal(0, 0.3, w2shape).astype(np.float32)))
            conv2.bias.copy_(torch.from_numpy(rng.normal(0, 0.1, w2shape[0]).astype(np.float32)))
        bn = _bn(c1, rng)
        bn.register_buffer("fake_weight", torch.from_numpy(rng.uniform(0.1, 0.6, c1).astype(np.float32)))
        bn.register_buffer("fake_bias", torch.from_numpy(rng.normal(0.8, 0.7, c1).astype(np.float32)))
        relu = nn.ReLU()
        graph = OrderedDict([("Data", "Data"), (1, conv1), (2, bn), (3, relu), (4, conv2)])
        bottoms = OrderedDict([("Data", None), (1, ["Data"]), (2, [1]), (3, [2]), (4, [3])])
        A[f"{tag}_w2"] = t2n(conv2.weight)
        A[f"{tag}_b1"], A[f"{tag}_b2"] = t2n(conv1.bias), t2n(conv2.bias)
        A[f"{tag}_fw"], A[f"{tag}_fb"] = t2n(bn.fake_weight), t2n(bn.fake_bias)
        ref_absorb(graph, [RefRelation(1, 4, 2)], bottoms, N=3)
        A[f"{tag}_b1_out"], A[f"{tag}_b2_out"] = t2n(conv1.bias), t2n(conv2.bias)
        A[f"{tag}_fb_out"] = t2n(bn.fake_bias)
        meta[tag] = dict(c1=c1)

    # bias-correction helpers
    w = torch.from_numpy(rng.uniform(0.2, 1.5, 64).astype(np.float32))
    b = torch.from_numpy(rng.normal(0, 1.0, 64).astype(np.float32))
    cm = lambda weight, bias: weight * torch.from_numpy(ref_bc.norm(0, 1).pdf(-bias / weight)).float() + \
        bias * (1 - torch.from_numpy(ref_bc.norm.cdf(-bias / weight)).float())   # bias_correction.py:170-172
    class _L:  # noqa: N801
        pass
    l1, l2 = _L(), _L()
    l1.fake_weight, l1.fake_bias = w, b
    l2.fake_weight, l2.fake_bias = w.flip(0).clone(), b.flip(0).clone()
    res = ref_bc._calculate_bias_correction_for_branches({"0": [(l1, True, "one")], "1": [(l1, True, "add"), (l2, False, "add")],
                                                           "2": [(l2, True, "add")]}, cm)
    A["bc_w"], A["bc_b"] = t2n(w), t2n(b)
    A["bc_expect_relu"] = t2n(res["0"][1])
    A["bc_expect_add"] = t2n(res["1"][1])
    E = torch.from_numpy(rng.normal(0, 0.01, (32, 64)).astype(np.float32))
    bias = torch.from_numpy(rng.normal(0, 0.1, 32).astype(np.float32))
    A["bc_E"], A["bc_bias"] = t2n(E), t2n(bias)
    bv = ref_bc._compute_final_bias_correction(E, ("one", res["0"][1]))
    layer = nn.Conv2d(64, 32, 1, bias=True)
    with torch.no_grad():
        layer.bias.copy_(bias)
    ref_bc._apply_bias_correction(layer, bv)
    A["bc_bias_out"] = t2n(layer.bias)
    A["bc_vec"] = t2n(bv).ravel()
    fb = torch.from_numpy(rng.normal(0, 0.3, 32).astype(np.float32))
    A["bc_fb"] = t2n(fb)
    prev = -bv
    A["bc_fb_out"] = t2n(fb + prev.view(-1, 32).mean(0))
    # depthwise-style E [C, 1] + expect [C] -> [C, C]
    Ed = torch.from_numpy(rng.normal(0, 0.01, (64, 1)).astype(np.float32))
    bvd = ref_bc._compute_final_bias_correction(Ed, ("one", res["0"][1]))
    layer = nn.Conv2d(64, 64, 3, groups=64, bias=True)
    with torch.no_grad():
        layer.bias.copy_(torch.zeros(64))
    ref_bc._apply_bias_correction(layer, bvd)
    A["bc_Ed"], A["bc_dw_bias_out"] = t2n(Ed), t2n(layer.bias)

    A["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(OUT / "transform_cases.npz", **A)
    print("transform cases:", len(meta))


def bc_edge_cases():
    """The bias-correction helpers at the reduction edges of the HIP kernels
    (tests/bc_edge_cases.py: shapes, seeds, input builder) -> bc_edge_cases.npz.
    Outputs only, as flat arrays in case order, plus one digest per case of its
    inputs.  Results that ATen's thread split can change are taken at every thread
    count of the case list; every other case is checked to be the same at all of
    them and stored once."""
    from tests import bc_edge_cases as BE

    class _L:  # noqa: N801
        pass

    cm = lambda weight, bias: weight * torch.from_numpy(ref_bc.norm(0, 1).pdf(-bias / weight)).float() + \
        bias * (1 - torch.from_numpy(ref_bc.norm.cdf(-bias / weight)).float())   # bias_correction.py:170-172
    A, digests = {}, []

    def at_threads(fn, threaded, what):
        res = []
        for t in BE.THREADS:
            torch.set_num_threads(t)
            res.append(fn())
        torch.set_num_threads(8)
        if threaded:
            return np.stack(res).ravel()
        assert all(r.tobytes() == res[0].tobytes() for r in res), f"{what}: depends on the thread count"
        return res[0]

    out = []
    for c in BE.APPLY_CASES:
        E, expect, bias = c.inputs()
        digests.append(h(np.concatenate([E.ravel(), expect, bias])))

        def run():
            layer = _L()
            layer.bias = nn.Parameter(torch.from_numpy(bias.copy()), requires_grad=False)
            bv = ref_bc._compute_final_bias_correction(torch.from_numpy(E.copy()), ("one", torch.from_numpy(expect.copy())))
            assert tuple(bv.shape) == (c.o, c.bcols)
            ref_bc._apply_bias_correction(layer, bv)
            return t2n(layer.bias)
        out.append(at_threads(run, c.threaded, c.name))
    A["apply_bias_out"] = np.concatenate(out)

    out = []
    for c in BE.PROP_CASES:
        vec, fb = c.inputs()
        digests.append(h(np.concatenate([vec, fb])))

        def run():
            prev = -torch.from_numpy(vec.copy())             # bias_prev = -bias (:251)
            fbt = torch.from_numpy(fb.copy())
            if prev.numel() != c.F:                          # :206-213
                prev = prev.view(-1, c.F).mean(dim=0)
            fbt.add_(prev)
            return t2n(fbt)
        out.append(at_threads(run, c.threaded, c.name))
    A["prop_fb_out"] = np.concatenate(out)

    out = []
    for case in BE.EXPECT_CASES:
        branch = []
        for w, b, relu in BE.expect_terms(case):
            layer = _L()
            layer.fake_weight, layer.fake_bias = torch.from_numpy(w.copy()), torch.from_numpy(b.copy())
            branch.append((layer, relu, "add"))
        res = ref_bc._calculate_bias_correction_for_branches({"0": branch}, cm)
        out.append(t2n(res["0"][1]))
    w, b = BE.expect_inputs()
    digests.append(h(np.concatenate([w, b])))
    A["expect"] = np.concatenate(out)
    A["digests"] = np.array(digests)
    np.savez_compressed(OUT / "bc_edge_cases.npz", **A)
    print("bc edge cases:", len(BE.APPLY_CASES), "apply,", len(BE.PROP_CASES), "propagate,", len(BE.EXPECT_CASES),
          "expect")


# ---------------------------------------------------------------------------
# model pipelines (main_dfq.py:188-231 stage order)
# ---------------------------------------------------------------------------
class _NpSpy:
    """Stands in for Cross_layer_equal's module-global ``np`` to record diff_tmp."""

    def __init__(self):
        self.diffs = []

    def sum(self, x, *a, **k):
        v = np.sum(x, *a, **k)
        self.diffs.append(float(v))
        return v

    def __getattr__(self, name):
        return getattr(np, name)


def pipeline(name: str, seed: int = 0, per_channel: bool = False, threads: int = 8, out: Path = None,
             bits_weight: int = 8, bits_bias: int = 8):
    """``threads``: torch's intra-op thread count for the run.  ATen splits two of the
    reference's fp32 reductions by it -- the CLE metric's torch.mean
    (Cross_layer_equal.py:107) and bias correction's view(-1, F).mean(0)
    (bias_correction.py:98-104,206-213) -- so the results depend on it;
    pipeline_<name>.npz is the 8-thread run, pipeline_<name>_t<T>.npz the others.
    ``bits_weight`` != 8 (BASELINE configs[4], ResNet-50 W4): main_dfq.py:209-231 with
    --bits_weight 4 -- set_layer_bits(graph, 4, 8, bits_bias), quantize_targ_layer(graph,
    4, bits_bias), clip_weight([-15, 15]), bias_correction(bits_weight=4);
    pipeline_<name>_w<bits>.npz."""
    t0 = time.time()
    torch.set_num_threads(threads)
    model = zoo.build(name, seed=seed, relu=True)
    g = build_graph(model, "positional")
    graph, bottoms = g.getGraph(), g.getBottoms()
    tkeys = [k for k in graph if type(graph[k]) in TARG]
    P = {"targets": np.array(tkeys, dtype=np.int64)}
    stats = {}

    def hb(a):   # 32-byte digest as uint8 (compact)
        return np.frombuffer(bytes.fromhex(h(a)), dtype=np.uint8)

    def snap(stage, full_bias=False):
        P[f"{stage}_wh"] = np.stack([hb(t2n(graph[k].weight)) for k in tkeys])
        bias = [t2n(graph[k].bias) if graph[k].bias is not None else np.zeros(0, np.float32) for k in tkeys]
        P[f"{stage}_bias_len"] = np.array([b.size for b in bias], dtype=np.int64)
        if full_bias:
            P[f"{stage}_bias"] = np.concatenate(bias) if bias else np.zeros(0, np.float32)
        P[f"{stage}_bh"] = np.stack([hb(b) for b in bias])

    def snap_bn(stage, full=False):
        bnk = [k for k in graph if type(graph[k]) == nn.BatchNorm2d and hasattr(graph[k], "fake_bias")]
        P[f"{stage}_bnkeys"] = np.array(bnk, dtype=np.int64)
        fw = np.concatenate([t2n(graph[k].fake_weight) for k in bnk])
        fb = np.concatenate([t2n(graph[k].fake_bias) for k in bnk])
        P[f"{stage}_fake_wh"], P[f"{stage}_fake_bh"] = hb(fw), hb(fb)
        if full:
            P[f"{stage}_fake_b"] = fb

    ref_merge_bn(model, graph, bottoms, TARG)
    snap("bn1"); snap_bn("bn1")
    res = ref_create_relation(graph, bottoms, TARG, delete_single=False)
    P["relations"] = np.array([[r.layer_first, r.layer_second, r.bn_idx] for r in res], dtype=np.int64)
    spy = _NpSpy()
    real_np = ref_cle.np
    ref_cle.np = spy
    try:
        tc = time.time()
        ref_cle.cross_layer_equalization(graph, res, TARG, Save_state=False, Treshhold=2e-7)
        stats["cle_seconds"] = time.time() - tc
    finally:
        ref_cle.np = real_np
    P["cle_diffs"] = np.array(spy.diffs, dtype=np.float64)
    P["cle_Sh"] = np.stack([hb(t2n(r.S)) for r in res])
    snap("cle"); snap_bn("cle")
    ref_absorb(graph, res, bottoms, N=3)
    snap("absorb", full_bias=True); snap_bn("absorb", full=True)
    # per-channel extension reference: quantize() per output-channel slice of the
    # post-absorption weights (what quantize_targ_layer would see after the 2nd merge)
    if per_channel:
        for mode, sym in (("chsym", True), ("chasym", False)):
            hs = []
            for k in tkeys:
                W = graph[k].weight.detach().clone()
                qw = torch.empty_like(W)   # (not `out`: that is the fixture path, saved below)
                for o in range(W.shape[0]):
                    sl = W[o].clone()
                    qw[o] = ref_quantize(sl, 8, float(sl.min()), float(sl.max()), symmetric=sym)
                hs.append(h(t2n(qw)))
            P[f"{mode}8_wh"] = np.stack([np.frombuffer(bytes.fromhex(x), dtype=np.uint8) for x in hs])
    if bits_weight != 8:   # main_dfq.py:209 (a host config step; no tensor changes on plain modules)
        from utils.quantize import set_layer_bits as ref_slb
        ref_slb(graph, bits_weight, 8, bits_bias, TARG)
    ref_merge_bn(model, graph, bottoms, TARG)
    snap("bn2", full_bias=True); snap_bn("bn2")
    ref_qtl(graph, bits_weight, bits_bias, TARG)
    snap("quant", full_bias=True)
    ref_clip(graph, [-15, 15], TARG)
    snap("clip", full_bias=True)
    try:
        ref_bc.bias_correction(graph, bottoms, TARG, bits_weight=bits_weight)
        P["bc_error"] = np.array("")
    except Exception as e:  # DeepLab: torch.cat of 2-D eps with 1-D expect (bias_correction.py:75)
        P["bc_error"] = np.array(f"{type(e).__name__}")
    snap("bc", full_bias=True); snap_bn("bc", full=True)
    stats["seconds"] = time.time() - t0
    stats["threads"] = threads
    stats["bits_weight"], stats["bits_bias"] = bits_weight, bits_bias
    P["stats"] = np.array(json.dumps(stats))
    P["bits"] = np.array([bits_weight, 8, bits_bias], dtype=np.int64)   # weight, activation, bias
    if out is None:
        out = OUT / (f"pipeline_{name}.npz" if threads == 8 else f"pipeline_{name}_t{threads}.npz")
        if bits_weight != 8:
            out = OUT / f"pipeline_{name}_w{bits_weight}.npz"
    np.savez_compressed(out, **P)
    torch.set_num_threads(8)
    print(name, "relations", len(res), "cle iters", len(spy.diffs), "bc", str(P["bc_error"]), stats)


def mkl_gap(name: str):
    """How much the reference itself moves when MKL is NOT pinned to its AVX2 code
    path (run with MKL_CBWR unset: torch.sqrt is then MKL VML's HA path, 1 ulp low
    on 0.65 % of inputs on AVX-512 hosts).  Compares a fresh run against the
    committed (pinned) pipeline_<name>.npz stage by stage; prints a JSON line."""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        out = Path(d) / "p.npz"
        pipeline(name, out=out)
        A, B = np.load(out), np.load(HERE / f"pipeline_{name}.npz")
        rep = {"model": name, "MKL_CBWR": os.environ.get("MKL_CBWR"),
               "cle_iterations": [int(len(A["cle_diffs"])), int(len(B["cle_diffs"]))]}
        for st in ("bn1", "cle", "absorb", "bn2", "quant", "clip", "bc"):
            rep[f"{st}_weight_layers_differ"] = int((A[f"{st}_wh"] != B[f"{st}_wh"]).any(1).sum())
            if f"{st}_bias" in A.files and A[f"{st}_bias"].shape == B[f"{st}_bias"].shape:
                rep[f"{st}_bias_elems_differ"] = int((A[f"{st}_bias"] != B[f"{st}_bias"]).sum())
        rep["layers"] = int(len(B["targets"]))
        print("MKLGAP", json.dumps(rep))


def act_ranges(name: str, seed: int = 0):
    """set_quant_minmax (utils/layer_transform.py:356-618) on the graph after the
    first merge_batchnorm (random BN statistics) and after the second one (the
    main_dfq order: fake stats reset to 1 / 0).  Every target layer carries a
    QuantMeasure (as QuantConv2d / QuantLinear would); every add / cat / mean /
    interpolate node one per tensor input (the reference's CustomTensorOP, in graph
    order -- PyTransformer, which would record them, is absent)."""
    import utils.layer_transform as ref_lt
    from utils.quantize import QuantMeasure as RefQM
    from data_free_quantization_amd.utils.layer_transform import CustomTensorOP as OurCTO
    model = zoo.build(name, seed=seed, relu=True)
    g = build_graph(model, "positional")
    graph, bottoms = g.getGraph(), g.getBottoms()
    tkeys = [k for k in graph if type(graph[k]) in TARG]
    for k in tkeys:
        graph[k].quant = RefQM(num_bits=8)
    ops = OurCTO(graph, bottoms)
    A = {"targets": np.array(tkeys, dtype=np.int64), "op_keys": np.array(ops.names),
         "op_counts": np.array([ops.offsets[k][1] for k in ops.names], dtype=np.int64)}

    def run(tag):
        qms = [RefQM(num_bits=8) for _ in range(len(ops.quants))]
        ref_lt.module_tensor_op = ref_lt.CustomTensorOP(qms, [(k, f"{k}_{ops.offsets[k][1]}") for k in ops.names])
        try:
            ref_lt.set_quant_minmax(graph, bottoms, verbose=False)
            A[f"{tag}_error"] = np.array("")
        except Exception as e:
            A[f"{tag}_error"] = np.array(f"{type(e).__name__}: {e}")
        mods = [graph[k].quant for k in tkeys] + qms
        A[f"{tag}_min"] = np.array([float(q.running_min) for q in mods], dtype=np.float32)
        A[f"{tag}_max"] = np.array([float(q.running_max) for q in mods], dtype=np.float32)

    ref_merge_bn(model, graph, bottoms, TARG)
    run("bn1")
    ref_merge_bn(model, graph, bottoms, TARG)
    run("bn2")
    np.savez_compressed(OUT / f"act_ranges_{name}.npz", **A)
    print(name, "act ranges:", len(tkeys), "layer quantizers,", len(ops.quants), "op quantizers",
          str(A["bn1_error"]), str(A["bn2_error"]))


def act_edge_cases():
    """set_quant_minmax on the tiny traced models of tests/act_edge_cases.py ->
    act_edge_cases.npz.  While it runs, torch.min / torch.max / torch.sqrt are
    wrapped and their one-dimensional tensor arguments recorded: the reference's
    per-channel mean - N*w, mean + N*w and var + eps (its lambdas are closures,
    so what they compute is taken where it reaches torch).  Per graph: the
    recorded vectors in call order (``seq`` indexes the file's pool of distinct
    vectors, ``kinds`` says which function took each), every quantizer's
    (min, max) and a digest of the inputs."""
    from unittest import mock
    import utils.layer_transform as ref_lt
    from utils.quantize import QuantMeasure as RefQM
    from data_free_quantization_amd.utils.layer_transform import CustomTensorOP as OurCTO
    from tests import act_edge_cases as AE
    AE.self_check()
    A, pool, flat = {}, {}, []
    for gname in AE.GRAPHS:
        model = AE.build_model(gname)
        A[f"{gname}.digest"] = np.array(h(AE.model_inputs(model)))
        g = build_graph(model, "positional")
        graph, bottoms = g.getGraph(), g.getBottoms()
        tkeys = [k for k in graph if type(graph[k]) in TARG]
        for k in tkeys:
            graph[k].quant = RefQM(num_bits=8)
        ops = OurCTO(graph, bottoms)
        qms = [RefQM(num_bits=8) for _ in range(len(ops.quants))]
        ref_lt.module_tensor_op = ref_lt.CustomTensorOP(qms, [(k, f"{k}_{ops.offsets[k][1]}") for k in ops.names])
        ref_merge_bn(model, graph, bottoms, TARG)
        rec = []

        def spy(kind, real):
            def wrapped(*a, **kw):
                if len(a) == 1 and not kw and torch.is_tensor(a[0]) and a[0].dim() == 1:
                    rec.append((kind, t2n(a[0])))
                return real(*a, **kw)
            return wrapped

        with mock.patch.object(torch, "min", spy(AE.REC_MIN, torch.min)), \
                mock.patch.object(torch, "max", spy(AE.REC_MAX, torch.max)), \
                mock.patch.object(torch, "sqrt", spy(AE.REC_SQRT, torch.sqrt)):
            ref_lt.set_quant_minmax(graph, bottoms, verbose=False)
        seq = []
        for _, v in rec:
            key = v.tobytes()
            if key not in pool:
                pool[key] = len(flat)
                flat.append(v)
            seq.append(pool[key])
        mods = [graph[k].quant for k in tkeys] + qms
        A[f"{gname}.targets"] = np.array(tkeys, dtype=np.int64)
        A[f"{gname}.op_keys"] = np.array(ops.names, dtype=np.str_)
        A[f"{gname}.seq"] = np.array(seq, dtype=np.int32)
        A[f"{gname}.kinds"] = np.array([k for k, _ in rec], dtype=np.uint8)
        A[f"{gname}.min"] = np.array([float(q.running_min) for q in mods], dtype=np.float32)
        A[f"{gname}.max"] = np.array([float(q.running_max) for q in mods], dtype=np.float32)
        nans = sum(int(np.isnan(v).sum()) for _, v in rec)
        if gname.startswith("clean."):
            assert nans == 0 and np.isfinite(A[f"{gname}.min"]).all() and np.isfinite(A[f"{gname}.max"]).all(), gname
        elif not gname.endswith("case_d"):   # the head's variance goes below -eps in >= 3 channels
            assert int(np.isnan(rec[-1][1]).sum()) >= 3 and np.isnan(A[f"{gname}.min"][len(tkeys) - 1]), gname
        print(gname, len(rec), "vectors recorded,", nans, "NaN elements")
    ref_lt.module_tensor_op = None
    A["pool_len"] = np.array([v.size for v in flat], dtype=np.int64)
    A["pool"] = np.concatenate(flat)
    np.savez_compressed(OUT / "act_edge_cases.npz", **A)
    print("act edge cases:", len(AE.GRAPHS), "graphs,", len(flat), "distinct vectors")


def cle_edge_cases():
    """The reference's own _layer_equalization, relation by relation as its
    cross_layer_equalization calls it (Cross_layer_equal.py:81-108), and its metric
    expression (:107-108) at 8 torch threads, for exactly three iterations on every
    graph and value set of tests/cle_edge_cases.py, unsigned and signed ->
    cle_edge_cases.npz.  Per run ``<graph>.<values>.<u|s>``: ``.diffs`` (float64 [3]),
    ``.small`` (every tensor of at most CE.ARRAY_MAX elements, concatenated in
    CE.pack's order: weights, created or existing first-layer biases, BN fake
    weight / bias, S) and ``.digests`` (h of each larger tensor, -0 folded); per
    graph and value set ``.inputs``, the digest of its generated inputs."""
    from tests import cle_edge_cases as CE
    from tests.cle_replay import edge_graph, edge_state
    torch.set_num_threads(CE.REF_THREADS)
    A, t0 = {}, time.time()
    for gname in CE.GRAPHS:
        assert sum(len(c.layers) for c in CE.GRAPHS[gname]) <= CE.MAX_TARGET_LAYERS, gname
        for vs in CE.VALUE_SETS:
            A[f"{gname}.{vs}.inputs"] = np.array(CE.input_digest(gname, vs))
            for signed in (False, True):
                graph, rels = edge_graph(gname, vs, device="cpu", relation_cls=RefRelation)
                diffs = []
                with torch.no_grad():
                    for _ in range(CE.ITERATIONS):
                        old_graph = copy.deepcopy(graph)
                        for rel in rels:
                            first, second, bn_idx = rel.get_idxs()
                            if graph[first].bias is None:   # :93-94
                                graph[first].bias = nn.Parameter(
                                    data=torch.zeros((graph[first].weight.size(0)), dtype=torch.float32),
                                    requires_grad=False)
                            graph[first].weight, graph[second].weight, graph[first].bias, S = \
                                ref_cle._layer_equalization(graph[first].weight, graph[second].weight,
                                                            graph[first].bias, graph[bn_idx].fake_weight,
                                                            graph[bn_idx].fake_bias, s_min_max=list(CE.S_MIN_MAX),
                                                            signed=signed, eps=0)
                            rel.set_scale_vec(S)
                        diff_list = [float(torch.mean(torch.abs(graph[k].weight - old_graph[k].weight)))
                                     for k in graph if type(graph[k]) in TARG]
                        diffs.append(float(np.sum(diff_list)))
                W, B, BN, S = edge_state(graph, rels)
                for d in (W, B):
                    for a in d.values():
                        assert a is None or np.isfinite(a).all(), (gname, vs, signed)
                _, small, digests = CE.pack(gname, W, B, BN, S)
                tag = f"{gname}.{vs}.{'s' if signed else 'u'}"
                A[f"{tag}.diffs"] = np.array(diffs, dtype=np.float64)
                A[f"{tag}.small"], A[f"{tag}.digests"] = small, digests
        print(gname, f"{time.time() - t0:.1f} s")
    np.savez_compressed(OUT / "cle_edge_cases.npz", **A)
    print("cle edge cases:", len(CE.GRAPHS), "graphs x", len(CE.VALUE_SETS), "value sets x 2 range kinds,",
          (OUT / "cle_edge_cases.npz").stat().st_size, "bytes")


FWD_INPUT = {"mobilenetv2": (16, 3, 224, 224), "resnet50": (16, 3, 224, 224), "deeplab": (2, 3, 129, 129),
             "resnet18": (16, 3, 224, 224)}
FWD_SEED = 2024


def forward_input(name):
    """The synthetic batch of the forward fixtures (numpy PCG64: the GPU test
    rebuilds it without the fixture carrying it)."""
    rng = np.random.Generator(np.random.PCG64(FWD_SEED))
    return rng.standard_normal(FWD_INPUT[name], dtype=np.float32)


def _record_op_calls(model, x):
    """The tensor-op calls a forward makes from a ``forward`` frame, in execution
    order, as the reference's op wrappers name them (utils/layer_transform.py:18-124:
    ``add_<line>_2``, ``torch_cat_<line>_<n>``, ``torch_mean_<line>_1``,
    ``F_interpolate_<line>_1``) -- what PyTransformer's recorder (absent) would
    have logged for ``switch_layers`` (:172-191)."""
    import torch.nn.functional as F
    rec = []

    def wrap(owner, attr, fmt):
        raw = getattr(owner, attr)

        def op(*a, **k):
            f = sys._getframe(1)
            if f.f_code.co_name == "forward":
                n = len(a[0]) if fmt.startswith("torch_cat") else 0
                rec.append(fmt.format(line=f.f_lineno, n=n))
            return raw(*a, **k)
        setattr(owner, attr, op)
        return owner, attr, raw

    saved = [wrap(torch.Tensor, "__add__", "add_{line}_2"), wrap(torch.Tensor, "__iadd__", "iadd_{line}_2"),
             wrap(torch, "cat", "torch_cat_{line}_{n}"), wrap(torch, "mean", "torch_mean_{line}_1"),
             wrap(F, "interpolate", "F_interpolate_{line}_1")]
    try:
        with torch.no_grad():
            model(x)
    finally:
        for owner, attr, raw in saved:
            setattr(owner, attr, raw)
    return rec


def forward_logits(name: str, seed: int = 0, bits_weight: int = 8):
    """The top-1 proxy: the reference's quantized forward after the
    main_dfq stage order (main_dfq.py:149-258) on a seeded synthetic batch.

    Conv2d / Linear become the REFERENCE's QuantConv2d / QuantLinear
    (utils/quantize.py:213-238,326-348), ReLU6 -> ReLU; merge_batchnorm,
    create_relation, cross_layer_equalization, bias_absorption, set_layer_bits,
    merge_batchnorm, quantize_targ_layer, set_quant_minmax, clip_weight and (MBv2,
    ResNet-50) bias_correction run as the reference's functions on positional keys;
    then model.eval() and the forward under torch.no_grad():
      * ``plain``: without replace_op (layer quantizers only), on a copy of the model;
      * ``ops``:   with the reference's replace_op (tensor-op inputs quantized by its
                   CustomTensorOP, one QuantMeasure per input, names as its wrappers
                   build them from the call site).
    Which ops carry quantizers was PyTransformer's choice (absent): here every
    add / cat / mean / interpolate node, as this package's CustomTensorOP does.
    ``*_nomkldnn``: the same forward with torch.backends.mkldnn disabled -- the
    reference's own sensitivity to the convolution's summation order, the noise
    floor a GPU convolution is compared against."""
    import utils.layer_transform as ref_lt
    from utils.quantize import QuantConv2d as RQC, QuantLinear as RQL, set_layer_bits as ref_slb
    from utils.quantize import QuantMeasure as RefQM
    from data_free_quantization_amd.utils.tracer import TorchTransformer
    from data_free_quantization_amd.utils.layer_transform import switch_layers
    t0 = time.time()
    model = zoo.build(name, seed=seed).eval()
    tr = TorchTransformer("positional")
    model, tr = switch_layers(model, tr, torch.ones(zoo.INPUT_SHAPES[name]),
                              {1: [(nn.Conv2d, RQC), (nn.Linear, RQL)], 0: [(nn.ReLU6, nn.ReLU)]}, quant_op=False)
    graph, bottoms = tr.log.getGraph(), tr.log.getBottoms()
    x = torch.from_numpy(forward_input(name))
    # the reference's CustomTensorOP for the graph's op nodes (graph order ==
    # execution order), named from the call sites
    op_nodes = [(k, len(bottoms[k])) for k, v in graph.items() if type(v) == str and bottoms[k] is not None
                and "pad" not in k and k.split("_")[0] in ("add", "torch.cat", "torch.mean", "F.interpolate")]
    calls = _record_op_calls(model, x[:1])
    assert len(calls) == len(op_nodes), (len(calls), len(op_nodes))
    names = []
    for (k, n), c in zip(op_nodes, calls):
        assert int(c.split("_")[-1]) == n and (k.split("_")[0].split(".")[-1] in c), (k, c)
        names.append((k, c))
    qms = [RefQM(num_bits=8, momentum=0.1) for _, n in op_nodes for _ in range(n)]
    cto = ref_lt.CustomTensorOP(qms, names)
    ref_lt.module_tensor_op = cto
    model.add_module("custom_tensor_op", cto)
    targ = (RQC, RQL)
    ref_merge_bn(model, graph, bottoms, targ)
    res = ref_create_relation(graph, bottoms, targ, delete_single=False)
    ref_cle.cross_layer_equalization(graph, res, targ, Save_state=False, Treshhold=2e-7)
    ref_absorb(graph, res, bottoms, N=3)
    ref_slb(graph, bits_weight, 8, 8, targ)
    ref_merge_bn(model, graph, bottoms, targ)
    ref_qtl(graph, bits_weight, 8, targ)
    ref_lt.set_quant_minmax(graph, bottoms, verbose=False)
    ref_clip(graph, [-15, 15], targ)
    correction = name != "deeplab"    # DeepLab: the reference's BC crashes on cat (bias_correction.py:75)
    if correction:
        ref_bc.bias_correction(graph, bottoms, targ, bits_weight=bits_weight)
    model.eval()
    # merge_batchnorm left every folded BN an identity with eps = 0 (:277-281), which
    # torch >= 2 rejects in F.batch_norm (torch 1.1, the reference's pin, accepted it).
    # The smallest normal fp32 eps keeps it an exact identity (1 + eps == 1 in fp32),
    # as this package's merge_batchnorm does around the forward.
    for mod in model.modules():
        if type(mod) == nn.BatchNorm2d and mod.eps == 0:
            mod.eps = float(torch.finfo(torch.float32).tiny)
    A = {"input_shape": np.array(FWD_INPUT[name], dtype=np.int64), "seed": np.array(FWD_SEED),
         "bits": np.array([bits_weight, 8, 8], dtype=np.int64),   # weight, activation, bias
         "correction": np.array(correction), "op_names": np.array([c for _, c in names]),
         "op_keys": np.array([str(k) for k, _ in names])}
    name_of = {id(mod): n for n, mod in model.named_modules()}
    tnames = [name_of[id(graph[k])] for k in graph if type(graph[k]) in targ]
    A["layer_names"] = np.array(tnames)

    def keep(y):   # DeepLab: every 4th pixel of the 21-class map (the full map is ~3 MB)
        y = y.detach()
        return t2n(y[:, :, ::4, ::4] if y.dim() == 4 else y)

    base = copy.deepcopy(model)     # every forward starts from this state (update_stat moves the ranges)
    for tag, mkl in (("", True), ("_nomkldnn", False)):
        torch.backends.mkldnn.enabled = mkl
        try:
            m = copy.deepcopy(base)
            with torch.no_grad():
                A[f"plain{tag}"] = keep(m(x))
            m = copy.deepcopy(base)
            ref_lt.module_tensor_op = m.custom_tensor_op
            ref_lt.replace_op()
            try:
                with torch.no_grad():
                    y = m(x)
            finally:
                ref_lt.restore_op()
            A[f"ops{tag}"] = keep(y)
            if y.dim() == 4:
                A[f"ops{tag}_argmax"] = t2n(y.argmax(1)).astype(np.uint8)
        finally:
            torch.backends.mkldnn.enabled = True
        # the ranges after the forward (update_stat, set_layer_bits quirk)
        mods = dict(m.named_modules())
        lq = [mods[n].quant for n in tnames]
        oq = [m.custom_tensor_op._modules[str(i)] for i in range(len(qms))]
        A[f"ops_layer_min{tag}"] = np.array([float(q.running_min) for q in lq], dtype=np.float32)
        A[f"ops_layer_max{tag}"] = np.array([float(q.running_max) for q in lq], dtype=np.float32)
        A[f"ops_op_min{tag}"] = np.array([float(q.running_min) for q in oq], dtype=np.float32)
        A[f"ops_op_max{tag}"] = np.array([float(q.running_max) for q in oq], dtype=np.float32)
    np.savez_compressed(OUT / (f"forward_{name}.npz" if bits_weight == 8 else f"forward_{name}_w{bits_weight}a8.npz"),
                        **A)
    d = lambda a, b: float(np.abs(A[a].astype(np.float64) - A[b]).max())   # noqa: E731
    print(name, "forward fixture:", len(names), "op nodes,", f"{time.time() - t0:.1f} s;",
          "mkldnn on/off max|d|: plain", d("plain", "plain_nomkldnn"), "ops", d("ops", "ops_nomkldnn"))


def literal_bc(name="mobilenetv2"):
    """Opaque (PyTransformer-like) keys: bias_correction skips every layer (Q2)."""
    model = zoo.build(name, seed=0, relu=True)
    g = build_graph(model, "opaque")
    graph, bottoms = g.getGraph(), g.getBottoms()
    before = [t2n(m.bias) if m.bias is not None else None for m in graph.values() if type(m) in TARG]
    ref_bc.bias_correction(graph, bottoms, TARG, bits_weight=8)
    after = [t2n(m.bias) if m.bias is not None else None for m in graph.values() if type(m) in TARG]
    same = all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(before, after))
    return same


def state_dict_keys():
    """The reference models' state_dict key names and shapes (checkpoint format),
    so tests can check that reference checkpoints load into the zoo models."""
    from modeling.classification.MobileNetV2 import MobileNetV2 as RefMBv2
    from modeling.segmentation.deeplab import DeepLab as RefDeepLab
    from modeling.segmentation.backbone.resnet import ResNet as RefResNet, Bottleneck
    out = {"mobilenetv2": RefMBv2(), "deeplab": RefDeepLab(sync_bn=False),
           "resnet50_backbone": RefResNet(Bottleneck, [3, 4, 6, 3], 16, nn.BatchNorm2d, pretrained=False)}
    res = {k: [[n, list(t.shape)] for n, t in m.state_dict().items()] for k, m in out.items()}
    (OUT / "state_dict_keys.json").write_text(json.dumps(res))
    print("state_dict keys:", {k: len(v) for k, v in res.items()})


def seg_transforms():
    """The reference's segmentation validation transform (dataset_utils/segmentation/
    pascal.py:108-112: FixScaleCrop -> Normalize -> ToTensor, custom_transforms.py)
    on seeded PIL images and masks of landscape, portrait, square and
    non-integer-scale shapes: inputs and outputs of every case, for
    tests/test_evaluate.py (data_free_quantization_amd.evaluate)."""
    from PIL import Image
    from dataset_utils.segmentation import custom_transforms as tr
    rng = np.random.default_rng(2024)
    cases = [((53, 37), 32), ((37, 53), 32), ((40, 40), 32), ((97, 61), 45), ((61, 97), 45), ((33, 100), 31),
             ((64, 48), 64), ((29, 30), 45)]   # (w, h), crop; the last two upscale
    out, meta = {}, []
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    comp = [tr.FixScaleCrop(crop_size=0), tr.Normalize(mean=mean, std=std), tr.ToTensor()]
    for i, ((w, h), crop) in enumerate(cases):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        mask = rng.integers(0, 21, (h, w), dtype=np.uint8)
        mask[rng.random((h, w)) < 0.05] = 255
        comp[0].crop_size = crop
        sample = {"image": Image.fromarray(img), "label": Image.fromarray(mask)}
        for t in comp:
            sample = t(sample)
        out[f"img{i}"], out[f"mask{i}"] = img, mask
        out[f"out_img{i}"] = sample["image"].numpy()
        out[f"out_label{i}"] = sample["label"].numpy()
        meta.append({"w": w, "h": h, "crop": crop})
    out["meta"] = np.array(json.dumps({"cases": meta, "mean": mean, "std": std}))
    np.savez_compressed(OUT / "seg_transforms.npz", **out)
    print("seg_transforms:", len(cases), "cases")


if __name__ == "__main__":
    which = sys.argv[1:] or ["quant", "transform", "mobilenetv2", "resnet50", "deeplab"]
    if any(w.startswith("mklgap_") for w in which):
        # run as: env -u MKL_CBWR DFQ_MKL_DEFAULT=1 python make_golden.py mklgap_<model>
        for w in which:
            if w.startswith("mklgap_"):
                mkl_gap(w[len("mklgap_"):])
        sys.exit(0)
    _check_ieee_sqrt()
    if "quant" in which:
        quant_cases()
    if "quant" in which or "chunks" in which:
        chunk_cases()
    if "transform" in which:
        transform_cases()
    if "bc_edge" in which:
        bc_edge_cases()
    if "act_edge" in which:
        act_edge_cases()
    if "cle_edge" in which:
        cle_edge_cases()
    for m in ("mobilenetv2", "resnet50", "deeplab", "resnet18"):
        if m in which:
            pipeline(m, per_channel=(m == "mobilenetv2"))
        if f"{m}_ch" in which:   # + the per-channel reference hashes (tests/test_golden_regen.py: a fast
            pipeline(m, per_channel=True)   # model through the per-channel block)
        for t in (1, 16):
            if f"{m}_t{t}" in which:
                pipeline(m, threads=t)
    if "resnet50_w4" in which:     # BASELINE configs[4]: ResNet-50 INT4 weights / INT8 acts, clip
        pipeline("resnet50", bits_weight=4)
    if "forward_resnet50_w4a8" in which:
        forward_logits("resnet50", bits_weight=4)
    for m in ("mobilenetv2", "resnet50", "deeplab"):
        if "act" in which or f"act_{m}" in which:
            act_ranges(m)
    for m in ("mobilenetv2", "resnet50", "deeplab", "resnet18"):
        if "forward" in which or f"forward_{m}" in which:
            forward_logits(m)
    if "keys" in which:
        state_dict_keys()
    if "seg" in which:
        seg_transforms()
    if "literal" in which:
        print("literal bias_correction is a no-op:", literal_bc())
