"""The one-launch integer inverted-residual block on the GPU: ``intmm.int_mbconv_q`` is, bit for bit, the numpy
float64 statement chain (``int_conv_cases.statement`` -> ``int_io_cases._quantize`` -> ``int_dwconv_cases.statement`` -> ``_quantize``
-> ``int_conv_cases.statement``) and the three existing ``_q`` calls.  The draws are the existing chain test's: x from N(0.4, 1.2^2)
on (-1.3, 2.5), weight scales 0.5 / 0.4 / 0.2, biases + 2.0, the hidden grids on [0, 6]."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import oracle
from tests import int_conv_cases as KC
from tests import int_dwconv_cases as DC
from tests import int_io_cases as QC
from tests import mx_conv_cases as CC
from tests.test_gpu_int_dwconv import DEV, _dev
from tests.test_gpu_int_io import _oq, _same

pytestmark = pytest.mark.gpu
RELU6 = (0.0, 6.0)
_BASE = dict(B=1, dims=(8, 24, 8), plane=(9, 7), stride=1, pad=1, x_sym=False, w_signed=0, per_row=1, zb=True, bias_p=True,
             out_codes=False, h2_bits=8)
#: what each pins is in the comment; the configurations are crossed sparingly, as int_conv_cases.CONFIGS does
CASES = {
    "chain": dict(B=2),                                                 # one ragged tile, one ragged chunk; batch 2
    # two K steps in expand, a ragged second chunk, Cout past two column tiles and no multiple of 16; stride 2 on an even plane
    "k2-chunks2": dict(dims=(72, 96, 40), plane=(8, 8), stride=2, x_sym=True, w_signed=1, per_row=0, zb=False, out_codes=True),
    # several tiles ragged on both axes, three chunks, hidden2 at 4 bits
    "tiles-chunks3": dict(dims=(16, 130, 24), plane=(19, 13), per_row=0, bias_p=False, out_codes=True, h2_bits=4),
    "pixel": dict(B=2, dims=(8, 200, 8), plane=(1, 1)),         # every tap but one in padding
    "s2p0-odd": dict(plane=(9, 7), stride=2, pad=0, w_signed=1, zb=False),
    "s2p0-even": dict(plane=(8, 8), stride=2, pad=0, out_codes=True),
    "s2p1-odd": dict(plane=(9, 7), stride=2),
    "s1p0": dict(plane=(8, 8), pad=0, x_sym=True),
}


def _weights(rng, N, K, scale, c, bias=True):
    """A layer's codes, scale, zero and bias: the oracle's 8-bit quantization of N(0, scale^2) weights."""
    mode = (oracle.CHANNEL_SYM if c["w_signed"] else oracle.CHANNEL_ASYM) if c["per_row"] else (oracle.TENSOR_SYM if c["w_signed"] else oracle.TENSOR_ASYM)
    o = oracle.quantize((rng.standard_normal((N, K)) * scale).astype(np.float32), 8, mode, rows=N)
    return SimpleNamespace(qb=o["codes"].astype(np.int64), b_bytes=o["codes"], sb=o["scale"], zb=o["zero"] if c["zb"] else None,
                           bias=(rng.standard_normal(N) + 2.0).astype(np.float32) if bias else None)


def _codes(y, rng_pair, bits=8, sym=False):
    """The quantizer's codes of ``y`` on a grid and the fp32 values they stand for (which quantize back to them)."""
    o = QC._quantize(y, rng_pair, bits, sym)
    q = o["codes"].reshape(y.shape)
    xq = (q.astype(np.float32) * o["scale"][0] + o["zero"][0]).astype(np.float32)
    assert np.array_equal(QC._quantize(xq, rng_pair, bits, sym)["codes"].reshape(y.shape), q)
    return q, xq


def _pointwise(xq, rng_pair, bits, sym, w, N):
    g = CC._g(*xq.shape, N, 1, 1, 0, 1)
    qa, sa, za = KC.quantized(xq, g, rng_pair, bits, sym)
    return KC.nchw(KC.statement(qa, KC.taps(g), w.qb, sa, za, w.sb, w.zb, w.bias), g)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The statement chain of a case, computed once: the operands, c1, c2 and the result (fp32, and its codes under out_codes)."""
    c = dict(_BASE, **CASES[name])
    (Cin, Ch, Cout), (H, W), rng = c["dims"], c["plane"], np.random.default_rng(0)
    in_range = QC.IN_RANGE[c["x_sym"]]
    q, xq = _codes((rng.standard_normal((c["B"], Cin, H, W)) * 1.2 + 0.4).astype(np.float32), in_range, 8, c["x_sym"])
    w = [_weights(rng, Ch, Cin, 0.5, c), _weights(rng, Ch, 9, 0.4, c), _weights(rng, Cout, Ch, 0.2, c, c["bias_p"])]
    c1, x1 = _codes(_pointwise(xq, in_range, 8, c["x_sym"], w[0], Ch), RELU6)
    gd = DC._g(c["B"], Ch, 1, H, W, 3, c["stride"], c["pad"], 1)
    c2, x2 = _codes(DC.statement(x1, gd, w[1], RELU6, 8, False, False, zb=c["zb"]), RELU6, c["h2_bits"])
    y = _pointwise(x2, RELU6, c["h2_bits"], False, w[2], Cout)
    for h, top in ((c1, 255), (c2, 2 ** c["h2_bits"] - 1)):
        assert len(np.unique(h)) >= 16 and (h == 0).any() and (h == top).any(), (name, len(np.unique(h)), h.min(), h.max())
    assert len(np.unique(y)) > 1   # a comparison of constant or saturated tensors would hide failures
    r = dict(c, q=q, w=w, c1=c1, c2=c2, y=y, in_range=in_range)
    if c["out_codes"]:
        r["out_range"] = tuple(float(np.float32(t)) for t in np.percentile(y.astype(np.float64), [5, 95]))
        r["codes"] = _codes(y, r["out_range"])[0]
    return r


@pytest.mark.parametrize("name", list(CASES))
def test_the_block_is_the_statement_chain_and_the_three_calls(name):
    from data_free_quantization_amd import intmm
    r = reference(name)
    layers = [(_dev(w.b_bytes), _dev(w.sb), _dev(w.zb), _dev(w.bias)) for w in r["w"]]
    xr = dict(zip(("min_value", "max_value"), r["in_range"]), symmetric=r["x_sym"])
    h1, h2 = _oq(RELU6), _oq(RELU6, r["h2_bits"])
    oq = _oq(r["out_range"], dev=True) if r["out_codes"] else None
    x = _dev(r["q"])
    got = intmm.int_mbconv_q(x, *layers, stride=r["stride"], padding=r["pad"], hidden1=h1, hidden2=h2, out_quant=oq, **xr)
    _same(got, r["codes"] if r["out_codes"] else r["y"], name)
    c1 = intmm.int_conv2d_q(x, *layers[0][:3], 1, x_codes=True, bias=layers[0][3], out_quant=h1, **xr)
    c2 = intmm.int_dwconv2d_q(c1, *layers[1][:3], 3, r["stride"], r["pad"], x_codes=True, bias=layers[1][3], out_quant=h2, min_value=0.0, max_value=6.0)
    c3 = intmm.int_conv2d_q(c2, *layers[2][:3], 1, x_codes=True, bias=layers[2][3], out_quant=oq, bits=r["h2_bits"], min_value=0.0, max_value=6.0)
    _same(c1, r["c1"], "c1")
    _same(c2, r["c2"], "c2")
    _same(got, c3.cpu().numpy(), "three calls")
