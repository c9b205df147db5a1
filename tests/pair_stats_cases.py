"""Shapes shared by the pair-statistics tests (tests/test_pair_stats_host.py plans
them, tests/test_gpu_pair_stats.py runs them): the smallest at which each path of
dfq_pair_stats_batch can go wrong."""
from data_free_quantization_amd import _lib

P = _lib.DFQ_PAIR_PIECE_ELEMS

SHAPES = [
    (1, 1), (1, 3), (3, 1), (5, 4), (7, 5), (2, 17),      # no full vector; rows starting off a 16-B boundary
    (32, 1, 3, 3), (16, 24, 1, 1),                        # depthwise (row_len 9), 1x1
    (200, 3),                                             # more than 64 rows per task
    (65, 128),                                            # a whole-row task that would exceed P elements
    (1, P - 1), (1, P), (1, P + 1), (2, 2 * P + 5), (3, 3 * P + 7),   # pieces, a short last piece, several split rows
]


def view2d(shape):
    """The [rows, row_len] view of the sweep (and of pair_stats)."""
    rows = shape[0]
    n = 1
    for s in shape:
        n *= s
    return rows, n // rows
