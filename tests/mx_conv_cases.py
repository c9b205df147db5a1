"""The geometries of dfq_mx_conv2d's tests (tests/test_mx_conv_host.py walks their index
arithmetic on the CPU, tests/test_gpu_mx_conv.py runs them): the smallest at which each index
path can go wrong.  (B, C, H, W, N, kernel, stride, padding, dilation), each of the last four as
an (h, w) pair."""
from collections import namedtuple

Geom = namedtuple("Geom", "B C H W N kernel stride padding dilation")


def _g(B, C, H, W, N, k, s, p, d):
    pair = lambda v: tuple(v) if isinstance(v, tuple) else (v, v)   # noqa: E731
    return Geom(B, C, H, W, N, pair(k), pair(s), pair(p), pair(d))


CASES = {
    # K = 45: blocks straddle channel and kernel-row boundaries, a partial last block.  M = 98: a
    # partial 64-row tile, and a four-row store group straddling the image boundary at m = 49
    "a": _g(2, 5, 7, 7, 9, 3, 1, 1, 1),
    "b": _g(1, 8, 7, 6, 40, 3, 2, 1, 1),          # non-square, stride 2, two wave tiles in N
    "c": _g(2, 3, 15, 15, 40, 7, 2, 3, 1),        # ResNet stem: K = 147, two K steps, the second partial
    "d": _g(1, 16, 9, 9, 9, 3, 1, 2, 2),          # dilated (DeepLab)
    "e": _g(2, 6, 5, 9, 9, (1, 3), (2, 1), (0, 1), 1),   # asymmetric everything
    "f": _g(1, 8, 4, 4, 9, 3, 1, 3, 1),           # padding wider than the kernel's reach: all-zero rows and blocks
    "g": _g(2, 24, 7, 7, 40, 1, 2, 0, 1),         # K < 32, pointwise, stride 2
    "h": _g(2, 130, 7, 7, 40, 1, 1, 0, 1),        # pointwise, K past one step
}


def out_size(g: Geom):
    return tuple((n + 2 * p - d * (k - 1) - 1) // s + 1
                 for n, k, s, p, d in zip((g.H, g.W), g.kernel, g.stride, g.padding, g.dilation))


def K(g: Geom) -> int:
    return g.C * g.kernel[0] * g.kernel[1]


def M(g: Geom) -> int:
    oh, ow = out_size(g)
    return g.B * oh * ow


def flat(g: Geom):
    """The 13 numbers of a line of the host check's shape file."""
    return (g.B, g.C, g.H, g.W, g.N, *g.kernel, *g.stride, *g.padding, *g.dilation)
