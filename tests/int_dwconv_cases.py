"""Geometries, operands and the expected result of dfq_int_dwconv2d, in numpy and CPU torch only
(tests/test_int_dwconv_host.py walks the index arithmetic of the geometries on the CPU,
tests/test_gpu_int_dwconv.py runs them).

The statement is dfq_int_conv2d's, per channel: channel c is ``KC.statement`` on ``x[:, c:c+1]``
with the one-channel geometry and rows ``c * mult .. (c + 1) * mult - 1`` of B, scale, zero and
bias; the channels are concatenated.  At import the module checks what the tests lean on: every
result is within 2^-23 max|ref| of a float64 ``F.conv2d(groups=C)`` of the affine values; on the
asymmetric range (-1.3, 2.5), where 0 is off the 8-bit grid, the statement differs from the
code-of-zero rule on every geometry with padding and equals it on every one without."""
import functools
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import oracle
from tests import int_conv_cases as KC
from tests import int_gemm_cases as IC
from tests import mx_conv_cases as CC

Geom = namedtuple("Geom", "B C mult H W kernel stride padding dilation")


def _g(B, C, mult, H, W, k, s, p, d):
    pair = lambda v: tuple(v) if isinstance(v, tuple) else (v, v)   # noqa: E731
    return Geom(B, C, mult, H, W, pair(k), pair(s), pair(p), pair(d))


#: the smallest at which each path can go wrong
GEOMS = {
    "mnv2_s1": _g(2, 5, 1, 7, 7, 3, 1, 1, 1),               # all four borders; a 49-element plane, no multiple of 4 or 64
    "mnv2_s2": _g(1, 3, 1, 9, 8, 3, 2, 1, 1),               # stride 2, non-square; right and bottom borders differ
    "dilated": _g(1, 4, 1, 9, 9, 3, 1, 2, 2),               # DeepLab
    "deep_pad": _g(1, 2, 1, 4, 4, 3, 1, 3, 1),              # 28 of 64 outputs per channel wholly in padding: stores bias
    "asym": _g(2, 6, 1, 5, 9, (1, 3), (2, 1), (0, 1), 1),   # every parameter differs by axis
    "mult2": _g(1, 3, 2, 6, 5, 3, 1, 1, 1),                 # c = n / mult
    "k5": _g(1, 2, 1, 8, 8, 5, 1, 2, 1),                    # 25 taps: several dot words, K % 4 != 0
    "k7_s2": _g(1, 2, 1, 15, 15, 7, 2, 3, 1),               # 49 taps
    "even_k": _g(2, 3, 1, 6, 7, (2, 3), 1, 0, 1),           # K = 6: the packed-nibble configuration runs
    "even_k_pad": _g(2, 3, 1, 6, 7, (3, 2), 1, 1, 1),       # packed nibbles together with the mask
    "one_pixel": _g(3, 70, 1, 3, 3, 3, 1, 0, 1),            # OH * OW = 1; more planes than lanes in a wave
    "wide": _g(1, 2, 1, 37, 69, 3, 1, 1, 1),                # more than one tile each way, partial last tiles, halos across tile edges
    "pointwise": _g(1, 5, 1, 4, 4, 1, 1, 0, 1),             # K = 1
}
PADDED = [n for n, g in GEOMS.items() if g.padding != (0, 0)]
CONFIGS = KC.CONFIGS
ASYM_RANGE, SYM_RANGE = KC.ASYM_RANGE, KC.SYM_RANGE


def N(g) -> int:
    return g.C * g.mult


def K(g) -> int:
    return g.kernel[0] * g.kernel[1]


def one_channel(g):
    """The geometry of one channel as tests/mx_conv_cases.py names it: C = 1, N = mult."""
    return CC._g(g.B, 1, g.H, g.W, g.mult, g.kernel, g.stride, g.padding, g.dilation)


def whole(g):
    """The same with all channels (only B, C, H, W and the window are meaningful)."""
    return CC._g(g.B, g.C, g.H, g.W, N(g), g.kernel, g.stride, g.padding, g.dilation)


def out_size(g):
    return CC.out_size(one_channel(g))


def flat(g):
    """The 13 numbers of a line of the host check's shape file."""
    return (g.B, g.C, g.H, g.W, g.mult, *g.kernel, *g.stride, *g.padding, *g.dilation)


def make_x(g, rng_pair, bits, sym) -> np.ndarray:
    return KC.make_x(whole(g), rng_pair, bits, sym)


def weights(g, b_signed, per_row, packed) -> IC.Case:
    """B [N, K] (and a bias) as tests/int_gemm_cases.py builds it; only the B side of the case is used."""
    return IC.build(2, N(g), K(g), 0, b_signed, per_row, packed)


def _rows(t, c, mult):
    t = np.asarray(t)
    return t if t.size == 1 else t[c * mult:(c + 1) * mult]


def statement(x, g, w, rng_pair, bits, sym, f32, zb=True, bias=True, code_of_zero=False) -> np.ndarray:
    """The contract, NCHW float32: KC.statement per channel, concatenated."""
    g1 = one_channel(g)
    v = KC.taps(g1)
    outs = []
    for c in range(g.C):
        qa, sa, za = KC.quantized(x[:, c:c + 1], g1, rng_pair, bits, sym, f32)
        out = KC.statement(qa, v, w.qb[c * g.mult:(c + 1) * g.mult], sa, za, _rows(w.sb, c, g.mult),
                           _rows(w.zb, c, g.mult) if zb else None, w.bias[c * g.mult:(c + 1) * g.mult] if bias else None, code_of_zero)
        outs.append(KC.nchw(out, g1))
    return np.ascontiguousarray(np.concatenate(outs, axis=1))


def _range(config):
    bits, sym, dev, f32, b_signed, per_row, packed = CONFIGS[config]
    rng_pair = SYM_RANGE if sym else ASYM_RANGE
    if dev:   # a device range holds floats
        rng_pair = tuple(float(np.float32(t)) for t in rng_pair)
    return rng_pair


@functools.lru_cache(maxsize=None)
def _expected(name, config, zb, bias, code_of_zero):
    g = GEOMS[name]
    bits, sym, dev, f32, b_signed, per_row, packed = CONFIGS[config]
    x = make_x(g, _range(config), bits, sym)
    w = weights(g, b_signed, per_row, packed)
    want = statement(x, g, w, _range(config), bits, sym, f32, zb, bias, code_of_zero)
    for a in (x, want):
        a.setflags(write=False)   # shared among the tests
    return x, w, want


def expected(name, config, zb=True, bias=True, code_of_zero=False):
    """(x, weights case, expected NCHW result) of a geometry under a configuration of CONFIGS,
    computed once."""
    return _expected(name, config, zb, bias, code_of_zero)


def affine_reference(x, g, w, rng_pair, bits, sym, f32) -> np.ndarray:
    """float64 F.conv2d(groups=C) of the affine values the codes stand for."""
    o = oracle.quantize(np.ascontiguousarray(x.reshape(1, -1)), bits, oracle.TENSOR_SYM if sym else oracle.TENSOR_ASYM, rows=1,
                        flags=oracle.F_GIVEN | (oracle.F_F32 if f32 else 0), given=rng_pair)
    d = lambda t: np.asarray(t, dtype=np.float32).astype(np.float64).reshape(-1)   # noqa: E731
    xh = o["codes"].astype(np.float64).reshape(x.shape) * d(o["scale"])[0] + d(o["zero"])[0]
    col = lambda t: np.broadcast_to(d(t), (N(g),))[:, None]   # noqa: E731
    wh = w.qb.astype(np.float64) * col(w.sb) + col(w.zb)
    ref = F.conv2d(torch.from_numpy(xh), torch.from_numpy(wh).view(N(g), 1, *g.kernel), torch.from_numpy(d(w.bias)),
                   g.stride, g.padding, g.dilation, groups=g.C)
    return ref.numpy()


def _self_check():
    assert set(GEOMS) - set(PADDED) == {"even_k", "one_pixel", "pointwise"}
    worst = 0.0
    for name, g in GEOMS.items():
        v = KC.taps(one_channel(g))
        assert (v.min() == 0) == (name in PADDED), name
        for config, (bits, sym, dev, f32, b_signed, per_row, packed) in CONFIGS.items():
            if packed and K(g) % 2:
                continue   # refused by the entry point: no packed row starts on a byte
            x, w, real = expected(name, config)
            assert real.shape == (g.B, N(g), *out_size(g))
            ref = affine_reference(x, g, w, _range(config), bits, sym, f32)
            err = float(np.abs(real.astype(np.float64) - ref).max() / np.abs(ref).max())
            worst = max(worst, err)
            assert err <= 2.0 ** -23, (name, config, err)
            if config == "a8-dev-rowu":   # 0 is off the grid: the code of 0.0 stands for q0 * s + min != 0
                coded = expected(name, config, code_of_zero=True)[2]
                assert np.array_equal(real, coded) == (name not in PADDED), name
    dp = GEOMS["deep_pad"]
    assert int((KC.taps(one_channel(dp)).sum(axis=1) == 0).sum()) == 28 and out_size(dp) == (8, 8)   # whole outputs in padding
    return worst


WORST_RELATIVE_ERROR = _self_check()
