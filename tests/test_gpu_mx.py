"""mx.mx_quantize (dfq_mx_quantize_batch) on the GPU against the numpy statement of
tests/mx_cases.py.  Every comparison is for equality: codes, scales, the
dequantized values as uint32 bit patterns, and the error sums against
torch.sum(e.view(O, I, khw), -1) on the CPU.  Every output buffer is followed by
guard words that must come back untouched."""
import numpy as np
import pytest
import torch

from tests import mx_cases as MC
from tests.mx_gpu_util import as_bytes as _bytes, check as _check, run as _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world():
    cases = MC.all_cases()
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
        nb, cb = MC.blocks(row_len), MC.FORMATS[c.fmt][3]
        codes = torch.from_numpy(out["codes"][:rows * nb * cb].reshape(rows, nb, cb)).to(dev)
        scales = torch.from_numpy(out["scales"][:rows * nb].reshape(rows, nb)).to(dev)
        y = mx.mx_dequantize(codes, scales, c.x.shape, c.fmt).cpu().numpy()
        assert np.array_equal(y.view(np.uint32), c.ref["y"].view(np.uint32)), c.name
