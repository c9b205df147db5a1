"""Operands and expected results of the code-in / code-out integer entries (dfq_int_*_q), in numpy and CPU torch only.
Nothing here restates a contract: the fp32 result is ``statement()`` of tests/int_gemm_cases.py, int_conv_cases.py or
int_dwconv_cases.py, and the only step added is the output one -- float32 of the statement, then the oracle's given-range
quantizer that ``int_conv_cases.quantized`` uses for inputs.  Stored input codes are random over the whole grid; the statements
take them through ``x^ = q * s + z``, which the oracle's quantizer maps back to q (asserted).  The output range of a case is the
5th and 95th percentile of the reference's own fp32 output; ``_case`` asserts at most a quarter saturating and 16 codes or more."""
import functools
import zlib

import numpy as np

from oracle import oracle
from tests import int_conv_cases as KC
from tests import int_dwconv_cases as DC
from tests import int_gemm_cases as IC
from tests import mx_conv_cases as CC

#: (M, N, K): the byte paths with ragged tiles, the wide paths with full tiles, one row
GEMM_SHAPES = [(37, 45, 70), (64, 64, 128), (1, 130, 16)]
#: batch 2.  pw: pointwise; k3p1: K = 27, takes the tap mask, OH * OW = 30 is no multiple of 4 and a
#: lane's rows m .. m + 3 cross an image boundary; k3s2d2: no mask, OH * OW = 12; quad: OH * OW = 16,
#: every aligned group goes out as one 4-B store, and K = 8 is even (the packed-INT4 B runs here)
CONV_GEOMS = {"pw": CC._g(2, 16, 5, 7, 24, 1, 1, 0, 1), "k3p1": CC._g(2, 3, 6, 5, 5, 3, 1, 1, 1),
              "k3s2d2": CC._g(2, 8, 11, 9, 6, 3, 2, 0, 2), "quad": CC._g(2, 8, 4, 4, 6, 1, 1, 0, 1)}
DW_PLANES = {"7x7": (7, 7), "40x70": (40, 70)}   # several planes per workgroup; several tiles per plane
DW_WINDOWS = {"s1p1": (2, 5, 1, 3, 1, 1, 1), "s2p1": (1, 3, 1, 3, 2, 1, 1), "dil2": (1, 4, 1, 3, 1, 0, 2), "mult2": (1, 3, 2, 3, 1, 1, 1)}
IN_RANGE = {False: KC.ASYM_RANGE, True: KC.SYM_RANGE}


def dw_geom(window, plane):
    B, C, mult, k, s, p, d = DW_WINDOWS[window]
    return DC._g(B, C, mult, *DW_PLANES[plane], k, s, p, d)


def _quantize(a, rng_pair, bits, sym):   # the oracle's given-range quantizer on a flat view (KC.quantized's call)
    return oracle.quantize(np.ascontiguousarray(a, dtype=np.float32).reshape(1, -1), bits, oracle.TENSOR_SYM if sym else oracle.TENSOR_ASYM,
                           rows=1, flags=oracle.F_GIVEN, given=rng_pair)


def _case(y, bits=8, sym=False, **kw):
    """A case's record: the fp32 statement ``y``, its output range and output codes, and ``kw``; read-only."""
    rng_pair = tuple(float(np.float32(t)) for t in np.percentile(y.astype(np.float64), [5, 95]))
    codes = _quantize(y, rng_pair, bits, sym)["codes"].reshape(y.shape)
    saturated = np.count_nonzero((y < np.float32(rng_pair[0])) | (y > np.float32(rng_pair[1])))
    assert 4 * saturated <= y.size and len(np.unique(codes)) >= 16, (saturated, y.size, len(np.unique(codes)))
    d = dict(kw, y=y, out_range=rng_pair, codes=codes)
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)   # shared among the tests
    return d


def in_codes(shape, sym, seed):
    """Stored 8-bit input codes over the whole grid (both ends present) and their dequantized fp32 values."""
    probe = _quantize(np.array([-1e30, 1e30]), IN_RANGE[sym], 8, sym)
    lo, hi = (int(t) for t in probe["codes"].reshape(-1))
    q = np.random.default_rng(seed).integers(lo, hi + 1, size=shape, dtype=np.int64)
    q.reshape(-1)[:2] = (lo, hi)
    xq = (q.astype(np.float32) * probe["scale"][0] + probe["zero"][0]).astype(np.float32)
    assert np.array_equal(_quantize(xq, IN_RANGE[sym], 8, sym)["codes"].reshape(shape).astype(np.int64), q)   # the range is idempotent
    return q.astype(np.int8 if sym else np.uint8), xq


@functools.lru_cache(maxsize=None)
def gemm(M, N, K, out_bits, out_sym):
    c = IC.build(M, N, K, 0, 1, 1, 0)
    return _case(IC.expected(c), out_bits, out_sym, case=c)


@functools.lru_cache(maxsize=None)
def linear(M, N, K, out_bits, out_sym):   # gemm()'s B with an fp32 input quantized to 8 bits on the asymmetric input range
    c = IC.build(M, N, K, 0, 1, 1, 0)
    x = np.random.default_rng(K).uniform(-1.8, 3.0, size=(M, K)).astype(np.float32)
    o = _quantize(x, IN_RANGE[False], 8, False)
    return _case(IC.statement(o["codes"].reshape(M, K).astype(np.int64), c.qb, o["scale"], o["zero"], c.sb, c.zb, c.bias), out_bits, out_sym, x=x)


@functools.lru_cache(maxsize=None)
def conv(name, x_codes, sym, packed=False):
    """A convolution on stored codes (or, x_codes False, on fp32 x), 8-bit inputs, 8-bit asymmetric output."""
    g = CONV_GEOMS[name]
    seed = zlib.crc32(repr((name, sym)).encode())
    q, x = in_codes((g.B, g.C, g.H, g.W), sym, seed) if x_codes else (None, KC.make_x(g, IN_RANGE[sym], 8, sym, seed % 1000))
    w = KC.weights(g, 1, 1, int(packed))
    qa, sa, za = KC.quantized(x, g, IN_RANGE[sym], 8, sym)
    return _case(KC.nchw(KC.statement(qa, KC.taps(g), w.qb, sa, za, w.sb, w.zb, w.bias), g), g=g, q=q, x=x, w=w)


@functools.lru_cache(maxsize=None)
def dwconv(window, plane, x_codes):
    g = dw_geom(window, plane)
    q, x = in_codes((g.B, g.C, g.H, g.W), False, zlib.crc32(repr((window, plane)).encode())) if x_codes else (None, DC.make_x(g, IN_RANGE[False], 8, False))
    w = DC.weights(g, 1, 1, 0)
    return _case(DC.statement(x, g, w, IN_RANGE[False], 8, False, False), g=g, q=q, x=x, w=w)
