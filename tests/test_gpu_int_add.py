"""The residual add on stored codes on the GPU: ``intmm.int_add_q`` is, as an equality, the numpy statement
``va = q_a * s_A + mn_A``, ``vb`` likewise, ``y = va + vb`` (each fp32 operation rounded once), then the oracle's given-range codes of
``y``.  The operands are the existing input draws, N(0.4, 1.2^2) quantized on ``QC.IN_RANGE``; a code output's range is the 5th and
95th percentile of ``y``."""
import functools

import numpy as np
import pytest
import torch

from tests import int_io_cases as QC
from tests.test_gpu_int_dwconv import DEV
from tests.test_gpu_int_io import _oq, _same

pytestmark = pytest.mark.gpu
#: 105 elements: under one wave's run of chunks, ragged tail.  3024: many chunks and a tail
SHAPES = {"small": (1, 3, 5, 7), "chunks": (2, 24, 9, 7)}
#: the byte offsets of a, b and out (in elements) from an aligned base: every base aligned; all three 1 B off (a head before the
#: first 16-B boundary); only b off (its bytes go one by one); b and out off by words (the 4-B path)
LAYOUTS = {"aligned": (0, 0, 0), "shifted": (1, 1, 1), "b-off": (0, 1, 0), "words": (0, 4, 8)}
#: name -> (bits, symmetric) of the output, None for fp32
OUTPUTS = {"fp32": None, "u8": (8, False), "u4": (4, False), "s8": (8, True)}
#: (shape, layout, a symmetric, output), crossed sparingly
CASES = [("small", "aligned", False, "fp32"), ("small", "aligned", True, "u8"), ("small", "aligned", False, "u4"), ("small", "shifted", False, "s8"),
         ("chunks", "aligned", False, "u8"), ("chunks", "aligned", True, "fp32"), ("chunks", "aligned", True, "s8"),
         ("chunks", "shifted", False, "u8"), ("chunks", "shifted", True, "fp32"), ("chunks", "shifted", False, "u4"),
         ("chunks", "b-off", False, "u8"), ("chunks", "b-off", True, "s8"), ("chunks", "b-off", False, "fp32"),
         ("chunks", "words", True, "u8"), ("chunks", "words", False, "fp32")]


def _operand(shape, sym, seed):
    """Stored codes of a draw on the input grid, and the grid's fp32 value of each (the statement's dq)."""
    x = (np.random.default_rng(seed).standard_normal(shape) * 1.2 + 0.4).astype(np.float32)
    o = QC._quantize(x, QC.IN_RANGE[sym], 8, sym)
    q = o["codes"].reshape(-1)
    v = (q.astype(np.float32) * np.float32(o["scale"][0]) + np.float32(o["zero"][0])).astype(np.float32)
    return q, v


@functools.lru_cache(maxsize=None)
def reference(shape, a_sym, output):
    """The statement of a case, computed once: the operands' codes (flat), y, and under a code output its range and codes."""
    (qa, va), (qb, vb) = _operand(SHAPES[shape], a_sym, 1), _operand(SHAPES[shape], False, 2)
    y = (va + vb).astype(np.float32)
    assert len(np.unique(y)) > 1
    r = dict(qa=qa, qb=qb, y=y, want=y)
    if OUTPUTS[output] is not None:
        bits, sym = OUTPUTS[output]
        r["out_range"] = tuple(float(np.float32(t)) for t in np.percentile(y.astype(np.float64), [5, 95]))
        c = r["want"] = QC._quantize(y, r["out_range"], bits, sym)["codes"].reshape(-1)
        lo, hi = (-2 ** (bits - 1), 2 ** (bits - 1) - 1) if sym else (0, 2 ** bits - 1)
        assert len(np.unique(c)) >= 16 and (c == hi).any(), (len(np.unique(c)), c.min(), c.max())
        # a symmetric grid clamps at -hi - 1 only and y leans to the positive side: that end lies beyond the data
        assert c.min() < 0 if sym else c.min() == lo, (c.min(), lo)
    [a.setflags(write=False) for a in r.values() if isinstance(a, np.ndarray)]   # shared among the tests
    return r


def _at(a, off, fill=0x5A):
    """``a`` (flat) on the GPU at ``off`` elements past an aligned base, inside a buffer of ``fill`` with 16 elements of guard behind."""
    buf = torch.full((a.size + off + 16,), fill, dtype=torch.from_numpy(np.empty(0, a.dtype)).dtype, device=DEV)
    view = buf[off:off + a.size]
    view.copy_(torch.from_numpy(np.array(a)))
    return view, buf


@pytest.mark.parametrize("shape,layout,a_sym,output", CASES)
def test_the_add_is_the_statement(shape, layout, a_sym, output):
    from data_free_quantization_amd import intmm
    r = reference(shape, a_sym, output)
    oa, ob, oo = LAYOUTS[layout]
    (a, _), (b, _) = _at(r["qa"], oa), _at(r["qb"], ob)
    out, buf = _at(np.zeros_like(r["want"]), oo)
    before, args = buf.clone(), lambda a, b: (a, _oq(QC.IN_RANGE[a_sym], 8, a_sym), b, _oq(QC.IN_RANGE[False]))   # noqa: E731
    assert (a.data_ptr() % 16, b.data_ptr() % 16, out.data_ptr() % 16) == (oa, ob, oo * out.element_size() % 16)
    oq = None if OUTPUTS[output] is None else _oq(r["out_range"], *OUTPUTS[output], dev=output == "u4")
    _same(intmm.int_add_q(*args(a, b), out_quant=oq, out=out), r["want"], (shape, layout, a_sym, output))
    assert torch.equal(buf[:oo], before[:oo]) and torch.equal(buf[oo + out.numel():], before[oo + out.numel():])   # nothing outside out
    if layout == "aligned":   # the tensor's own shape, and an output the call allocates
        _same(intmm.int_add_q(*args(a.view(SHAPES[shape]), b.view(SHAPES[shape])), out_quant=oq), r["want"].reshape(SHAPES[shape]), "allocated")
