"""Pooling on stored codes on the GPU.  ``intmm.int_mean_q`` is, as an equality, the numpy statement
``S = sum q``, ``m = (float64(s) * S) / P + float64(z)``, ``y = float32(m)``, then the oracle's given-range codes of ``y``;
``intmm.int_maxpool2d_q`` is ``F.max_pool2d`` on the CPU of the codes cast to float32, then (``out_quant``) the oracle's codes of the
maximum's fp32 value.  A code output's range is the 5th and 95th percentile of the fp32 result."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import int_io_cases as QC
from tests.test_gpu_int_add import _at
from tests.test_gpu_int_io import _oq, _same

pytestmark = pytest.mark.gpu
#: name -> (bits, symmetric) of the output, None for fp32
OUTPUTS = {"fp32": None, "u8": (8, False), "s8": (8, True)}
#: (P, R, offset of x and out in elements, symmetric, input bits, output).  A workgroup owns 1024 rows of P = 1 and 7, 512 of 16,
#: 481 of 17, 167 of 49 and 2 of 4096, the largest small plane: every R leaves the last one ragged, and its last quad of rows too.
#: P = 4097 is the large regime, a workgroup a row.
MEAN_CASES = [(1, 1029, 0, False, 8, "fp32"), (1, 1029, 1, True, 8, "u8"), (7, 1029, 0, False, 4, "u8"), (7, 1029, 1, True, 8, "fp32"),
              (16, 515, 0, True, 8, "s8"), (16, 515, 1, False, 8, "fp32"), (17, 515, 1, False, 8, "u8"), (17, 515, 0, True, 4, "fp32"),
              (49, 337, 0, False, 8, "u8"), (49, 337, 1, False, 8, "fp32"), (49, 337, 1, True, 8, "s8"),
              (4096, 5, 1, False, 8, "u8"), (4096, 5, 0, True, 8, "fp32"),
              (4097, 5, 0, False, 8, "fp32"), (4097, 5, 1, True, 4, "u8"), (4097, 5, 1, False, 8, "s8")]


def _grid(sym, bits=8):
    """The input grid: its least and largest code, and the fp32 step and offset of its range."""
    o = QC._quantize(np.array([-1e30, 1e30]), QC.IN_RANGE[sym], bits, sym)
    lo, hi = (int(t) for t in o["codes"].reshape(-1))
    return lo, hi, np.float32(o["scale"][0]), np.float32(o["zero"][0])


def _value(q, s, z):   # the fp32 value of a code on its grid: two operations, each rounded once
    return (q.astype(np.float32) * s + z).astype(np.float32)


def _mean_statement(q, s, z):
    S = q.astype(np.int64).sum(-1)
    return ((np.float64(s) * S.astype(np.float64)) / np.float64(q.shape[-1]) + np.float64(z)).astype(np.float32)


def _coded(y, output):
    """The expected result and its range: ``y``, or its codes on the 5th .. 95th percentile of ``y``."""
    if OUTPUTS[output] is None:
        return y, None
    rng_pair = tuple(float(np.float32(t)) for t in np.percentile(y.astype(np.float64), [5, 95]))
    return QC._quantize(y, rng_pair, *OUTPUTS[output])["codes"].reshape(y.shape), rng_pair


@functools.lru_cache(maxsize=None)
def mean_reference(P, R, sym, bits, output, full=False):
    """Codes [R, P] whose rows reach different ceilings, so that the means spread over the grid; the statement of them."""
    lo, hi, s, z = _grid(sym, bits)
    g = np.random.default_rng(P * 1000 + R)
    q = g.integers(lo, g.integers(lo + 1, hi + 1, size=(R, 1)) + 1, size=(R, P))
    if full:
        q[:] = hi
    y = _mean_statement(q, s, z)
    want, rng_pair = _coded(y, output)
    assert full or len(np.unique(want)) >= 3, want
    r = dict(q=q.astype(np.int8 if sym else np.uint8), y=y, want=want, out_range=rng_pair, s=s, z=z)
    [a.setflags(write=False) for a in r.values() if isinstance(a, np.ndarray)]   # shared among the tests
    return r


def _run_mean(r, off, sym, bits, output):
    from data_free_quantization_amd import intmm
    (x, _), (out, buf) = _at(r["q"].reshape(-1), off), _at(np.zeros_like(r["want"]), off)
    before = buf.clone()
    assert x.data_ptr() % 16 == off
    oq = None if OUTPUTS[output] is None else _oq(r["out_range"], *OUTPUTS[output])
    got = intmm.int_mean_q(x.view(1, *r["q"].shape), _oq(QC.IN_RANGE[sym], bits, sym), out_quant=oq, out=out.view(1, -1))
    assert torch.equal(buf[:off], before[:off]) and torch.equal(buf[off + out.numel():], before[off + out.numel():])   # nothing outside out
    return got.view(-1)


@pytest.mark.parametrize("P,R,off,sym,bits,output", MEAN_CASES)
def test_the_mean_is_the_statement(P, R, off, sym, bits, output):
    r = mean_reference(P, R, sym, bits, output)
    _same(_run_mean(r, off, sym, bits, output), r["want"], (P, R, off, sym, bits, output))


def test_the_mean_of_the_largest_codes():
    """Every byte 255 at the largest tested P: S = 255 * 4097 is past 2^20, a partial sum kept too narrow fails."""
    r = mean_reference(4097, 3, False, 8, "fp32", full=True)
    assert (r["q"] == 255).all()
    _same(_run_mean(r, 0, False, 8, "fp32"), r["want"], "all 255")


def test_the_mean_is_near_the_mean_of_the_values():
    """|y - float64 mean of the per-element fp32 values| <= 2^-23 (3 D + 2 |z|), D = (2^bits - 1) s: DESIGN.md 3.9.4's bound,
    doubled for the second-order terms."""
    from data_free_quantization_amd import intmm
    r = mean_reference(49, 337, False, 8, "fp32")
    s, z = np.float64(r["s"]), np.float64(r["z"])
    x = torch.from_numpy(np.array(r["q"])).cuda().view(1, 337, 7, 7)
    y = intmm.int_mean_q(x, _oq(QC.IN_RANGE[False])).cpu().numpy().reshape(-1).astype(np.float64)
    err = np.abs(y - _value(r["q"], r["s"], r["z"]).astype(np.float64).mean(-1)).max()
    bound = 2.0 ** -23 * (3 * 255 * s + 2 * abs(z))
    print("error %.3e, bound %.3e" % (err, bound))
    assert err <= bound


#: B, C, H, W, kernel, stride, padding.  On 7 x 7 the last window is half padding and the 70 planes are a workgroup of 64 and one of 6;
#: on 8 x 8 the last window is dropped; 2 x 2 on 5 x 5 drops a row and a column; 33 x 65 is one more than a tile of 32 x 64 each way
POOL_GEOMS = {"k3s2p1_7": (2, 35, 7, 7, 3, 2, 1), "k3s2p1_8": (1, 3, 8, 8, 3, 2, 1), "k2s2_5": (1, 3, 5, 5, 2, 2, 0),
              "k3s1p1_big": (1, 2, 33, 65, 3, 1, 1), "k32_s21": (2, 3, 9, 17, (3, 2), (2, 1), (1, 1))}
#: negative: int8 with every code below 0 (a padding tap taken for the byte 0 wins); requant: out_quant on the 5th .. 95th percentile of
#: the values; shifted: x and out 1 B off alignment inside guard buffers
POOL_CASES = [("k3s2p1_7", False, "plain"), ("k3s2p1_7", True, "negative"), ("k3s2p1_7", True, "requant"), ("k3s2p1_8", True, "plain"),
              ("k3s2p1_8", False, "shifted"), ("k2s2_5", False, "plain"), ("k3s1p1_big", False, "plain"), ("k3s1p1_big", True, "shifted"),
              ("k32_s21", True, "plain"), ("k32_s21", False, "requant")]


@functools.lru_cache(maxsize=None)
def pool_reference(geom, sym, variant):
    B, C, H, W, k, s, p = POOL_GEOMS[geom]
    q, _ = QC.in_codes((B, C, H, W), sym, len(geom) + 7 * sym)
    if variant == "negative":
        q = (-(np.abs(q.astype(np.int64)) % 127) - 1).astype(np.int8)
        assert q.max() < 0
    c = F.max_pool2d(torch.from_numpy(q.astype(np.float32)), k, s, p).numpy()
    assert np.array_equal(c, c.astype(q.dtype).astype(np.float32))
    r = dict(q=q, want=c.astype(q.dtype), out_range=None)
    if variant == "requant":
        _, _, sx, zx = _grid(sym)
        r["want"], r["out_range"] = _coded(_value(c, sx, zx), "u8")
        assert len(np.unique(r["want"])) >= 16
    [a.setflags(write=False) for a in r.values() if isinstance(a, np.ndarray)]
    return r


@pytest.mark.parametrize("geom,sym,variant", POOL_CASES)
def test_the_max_pool_is_torchs_on_the_codes(geom, sym, variant):
    from data_free_quantization_amd import intmm
    r, (k, s, p), off = pool_reference(geom, sym, variant), POOL_GEOMS[geom][4:], int(variant == "shifted")
    (x, _), (out, buf) = _at(r["q"].reshape(-1), off), _at(np.zeros_like(r["want"]).reshape(-1), off)
    before = buf.clone()
    oq = None if r["out_range"] is None else _oq(r["out_range"])
    got = intmm.int_maxpool2d_q(x.view(r["q"].shape), _oq(QC.IN_RANGE[sym], 8, sym), k, s, p, out_quant=oq, out=out.view(r["want"].shape))
    _same(got, r["want"], (geom, sym, variant))
    assert torch.equal(buf[:off], before[:off]) and torch.equal(buf[off + out.numel():], before[off + out.numel():])   # nothing outside out
    if variant == "plain" and s == k:   # stride None is the kernel size, and an output the call allocates
        _same(intmm.int_maxpool2d_q(x.view(r["q"].shape), _oq(QC.IN_RANGE[sym], 8, sym), k), r["want"], "allocated")
