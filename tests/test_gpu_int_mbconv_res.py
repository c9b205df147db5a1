"""The inverted-residual block with its shortcut in the epilogue.  The un-fused block is pinned against numpy in
tests/test_gpu_int_mbconv.py, so the ground here is the epilogue: with P the 5th and 95th percentile of the block's fp32 output and
c3 the block's codes on P, ``int_mbconv_q(residual=P)`` is, as an equality, the numpy add statement of tests/test_gpu_int_add.py on
(c3, x) and the two-launch route ``int_add_q(c3, P, x, X)``.  The draws are tests/test_gpu_int_mbconv.py's."""
import numpy as np
import pytest

from tests import int_io_cases as QC
from tests.test_gpu_int_dwconv import _dev
from tests.test_gpu_int_io import _oq, _same
from tests.test_gpu_int_mbconv import RELU6, _codes, _weights

pytestmark = pytest.mark.gpu
_BASE = dict(B=1, dims=(8, 24, 8), plane=(9, 7), x_sym=False, w_signed=0, per_row=1, zb=True, p_bits=8, out=None)
#: stride 1, pad 1, Cin == Cout; out: (bits, symmetric) of a code output
CASES = {
    "chain": dict(B=2),                                                       # one ragged tile, batch 2
    # tiles ragged on both axes, the second column tile ragged, three chunks
    "tiles-chunks3": dict(dims=(24, 130, 24), plane=(19, 13), out=(8, False)),
    # two K steps, xs' pitch beyond 64; symmetric x: the signed-domain byte comes back as an int8 code
    "k2-sym": dict(dims=(72, 96, 72), plane=(8, 8), x_sym=True, w_signed=1, per_row=0, zb=False, out=(8, False)),
    "ct5": dict(dims=(136, 64, 136), plane=(3, 3)),                           # nine column tiles (CT = 5), three K steps
    "pixel": dict(B=2, dims=(8, 200, 8), plane=(1, 1)),                       # the centre is the only tap inside the image
    "p4": dict(p_bits=4),
    "out4": dict(out=(4, False)),
}


def _value(q, rng_pair, bits, sym):
    """The grid's fp32 value of each code: the statement's dq, with the oracle's scale and zero of the grid."""
    o = QC._quantize(np.zeros(1, np.float32), rng_pair, bits, sym)
    return (q.astype(np.float32) * np.float32(o["scale"][0]) + np.float32(o["zero"][0])).astype(np.float32)


def _pct(y):
    return tuple(float(np.float32(t)) for t in np.percentile(y.astype(np.float64), [5, 95]))


@pytest.mark.parametrize("name", list(CASES))
def test_the_residual_epilogue_is_the_add_of_the_blocks_codes_and_x(name):
    from data_free_quantization_amd import intmm
    c = dict(_BASE, **CASES[name])
    (Cin, Ch, Cout), (H, W), rng = c["dims"], c["plane"], np.random.default_rng(0)
    in_range = QC.IN_RANGE[c["x_sym"]]
    q = _codes((rng.standard_normal((c["B"], Cin, H, W)) * 1.2 + 0.4).astype(np.float32), in_range, 8, c["x_sym"])[0]
    w = [_weights(rng, Ch, Cin, 0.5, c), _weights(rng, Ch, 9, 0.4, c), _weights(rng, Cout, Ch, 0.2, c)]
    layers = [(_dev(t.b_bytes), _dev(t.sb), _dev(t.zb), _dev(t.bias)) for t in w]
    x, X = _dev(q), _oq(in_range, 8, c["x_sym"])
    block = lambda **kw: intmm.int_mbconv_q(x, *layers, hidden1=_oq(RELU6), hidden2=_oq(RELU6), symmetric=c["x_sym"],   # noqa: E731
                                            min_value=in_range[0], max_value=in_range[1], **kw)
    p_range = _pct(block().cpu().numpy())
    P = _oq(p_range, c["p_bits"])
    c3 = block(out_quant=P)
    c3n = c3.cpu().numpy()   # the codes the fused call never stores
    assert c3n.min() == 0 and c3n.max() == 2 ** c["p_bits"] - 1, (c3n.min(), c3n.max())
    want = y = (_value(c3n, p_range, c["p_bits"], False) + _value(q, in_range, 8, c["x_sym"])).astype(np.float32)
    oq = None
    if c["out"] is not None:
        out_range = _pct(y)
        oq, want = _oq(out_range, *c["out"], dev=True), QC._quantize(y, out_range, *c["out"])["codes"].reshape(y.shape)
    assert (want != block(out_quant=oq).cpu().numpy()).any()   # the shortcut changes the result
    got = block(residual=P, out_quant=oq)
    _same(got, want, name)
    _same(intmm.int_add_q(c3, P, x, X, out_quant=oq), want, "two launches")
