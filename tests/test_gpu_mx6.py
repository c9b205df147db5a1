"""mx.mx_quantize (dfq_mx_quantize_batch) in the two MXFP6 formats on the GPU against
the numpy statement of tests/mx6_cases.py.  Every comparison is for equality: the
packed codes, scales, the dequantized values as uint32 bit patterns, and the error
sums against torch.sum(e.view(O, I, khw), -1) on the CPU.  Every output buffer is
followed (the codes, which start 0, 1 or 2 bytes past a 4-B boundary, also preceded)
by guard words that must come back untouched: a dword store past the last quad of a
task, or one on the byte path's addresses, lands there."""
import numpy as np
import pytest
import torch

from tests import mx6_cases as M6
from tests import mx_cases as MC
from tests.mx_gpu_util import as_bytes as _bytes, check as _check, run as _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world():
    cases = M6.all_cases()
    return {"cases": cases, "together": _run(cases), "again": _run(cases), "reversed": _run(cases[::-1])[::-1],
            "alone": [_run([c])[0] for c in cases]}


def test_codes_scales_values_and_error_sums_equal_the_statement(world):
    for c, out in zip(world["cases"], world["together"]):
        _check(c, out)


def test_the_same_bytes_reversed_alone_and_again(world):
    for i, c in enumerate(world["cases"]):
        want = _bytes(world["together"][i])
        assert _bytes(world["again"][i]) == want, c.name
        assert _bytes(world["reversed"][i]) == want, c.name
        assert _bytes(world["alone"][i]) == want, c.name


def test_dequantize_on_the_gpu_rebuilds_dst_from_codes(world):
    from data_free_quantization_amd import mx
    dev = torch.device("cuda:0")
    for c, out in zip(world["cases"], world["together"]):
        if c.outputs != "all":
            continue
        rows, row_len = c.x.shape
        nb, cb, co = MC.blocks(row_len), M6.FORMATS[c.fmt][3], c.code_offset
        codes = torch.from_numpy(out["codes"][co:co + rows * nb * cb].reshape(rows, nb, cb).copy()).to(dev)
        scales = torch.from_numpy(out["scales"][:rows * nb].reshape(rows, nb).copy()).to(dev)
        y = mx.mx_dequantize(codes, scales, c.x.shape, c.fmt).cpu().numpy()
        assert np.array_equal(y.view(np.uint32), c.ref["y"].view(np.uint32)), c.name


def test_a_list_that_mixes_all_four_formats():
    """FP4 and FP8 cases of tests/mx_cases.py interleaved with both FP6 formats in one
    call: each tensor equals its own statement, whatever its neighbours' format."""
    old, new = MC.all_cases(), M6.all_cases()
    mixed = []
    for i in range(40):
        mixed += [old[(7 * i) % len(old)], new[(11 * i) % len(new)], new[(11 * i + 1) % len(new)], old[(7 * i + 1) % len(old)]]
    mixed = list({c.name: c for c in mixed}.values())   # each tensor at most once per call
    assert {c.fmt for c in mixed} == set(MC.FORMATS) | set(M6.FORMATS)
    assert any(c.khw > 1 and c.want_esum for c in mixed if c.fmt in M6.FORMATS)
    assert any(c.khw > 1 and c.want_esum for c in mixed if c.fmt in MC.FORMATS)
    for c, out in zip(mixed, _run(mixed)):
        _check(c, out)
