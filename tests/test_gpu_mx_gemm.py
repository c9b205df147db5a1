"""dfq_mx_gemm on the GPU (mx.mx_gemm / mx.mx_linear).

The layout proof: operands written directly as codes and scale bytes (tests/mx_gemm_cases.py:
grid values every format holds, an independent scale byte per block) whose product is exact
in fp32 in any summation order, so the kernel's output must equal integer arithmetic bit
for bit -- on all 16 format pairs.  Per-block scales catch a lane <-> block or scale-byte
mismatch, mixed pairs a bit or nibble order that differs from the stored one (a permutation
common to both operands cancels only between equal formats), the random signs a
transposed C write.  Random data then checks the accumulation against the contract's
bound, measured and printed."""
import numpy as np
import pytest
import torch

from tests import mx_gemm_cases as GC

pytestmark = pytest.mark.gpu
RANDOM_SHAPES = [(32, 48, 416), (5, 1000, 1280)]
# added after the measurement: one K step (nb <= 4), where the instruction's own error shows
ONE_STEP_SHAPES = [(32, 40, 24), (32, 40, 128)]
RANDOM_PAIRS = [("mxfp8", "mxfp4"), ("mxfp8", "mxfp8"), ("mxfp6_e2m3", "mxfp6_e3m2"), ("mxfp4", "mxfp4")]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _operands(shape, a_fmt, b_fmt):
    av, asc, bv, bsc, out = GC.exact_case(*shape)
    ac, as_ = GC.encode(av, asc, a_fmt)
    bc, bs = GC.encode(bv, bsc, b_fmt)
    return _dev(ac), _dev(as_), _dev(bc), _dev(bs), out


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("shape", GC.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("a_fmt,b_fmt", GC.PAIRS)
def test_exact_products_on_every_format_pair(a_fmt, b_fmt, shape):
    from data_free_quantization_amd import mx
    ac, as_, bc, bs, want = _operands(shape, a_fmt, b_fmt)
    got = mx.mx_gemm(ac, as_, a_fmt, bc, bs, b_fmt, shape[2])
    torch.cuda.synchronize()
    assert got.shape == want.shape and got.dtype == torch.float32
    bad = np.argwhere(_bits(got) != want.view(np.uint32))
    assert bad.size == 0, (len(bad), bad[:4].tolist(), got.cpu().numpy()[tuple(bad[0])], want[tuple(bad[0])])


def test_the_cases_decode_as_mx_dequantize_reads_them():
    """The hand-written codes stand for the intended values under the project's own reader."""
    from data_free_quantization_amd import mx
    av, asc, _, _, _ = GC.exact_case(17, 33, 96)
    for fmt in GC.FMTS:
        c, s = GC.encode(av, asc, fmt)
        y = mx.mx_dequantize(_dev(c), _dev(s), (17, 96), fmt).cpu().numpy().astype(np.float64)
        assert np.array_equal(y * 4, GC.quarter_units(av, asc)[:, :96]), fmt


@pytest.mark.parametrize("shape", RANDOM_SHAPES + ONE_STEP_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("a_fmt,b_fmt", RANDOM_PAIRS + [("mxfp8", "mxfp6_e2m3")])
def test_random_data_within_the_accumulation_bound(a_fmt, b_fmt, shape):
    """Gaussian operands through mx_quantize against the float64 product of
    mx_dequantize's outputs.  The contract (include/dfq_hip.h): every product is exact in
    fp32, and |acc - sum a*b| <= 32 * nb * 2^-24 * sum |a*b| -- what any-order fp32
    accumulation of exact products meets -- is asserted as derived on (32, 48, 416) and
    (5, 1000, 1280); measured worst ratio there 4.3e-6 (mxfp8 x mxfp8, 0.17 of the bound).
    On the one-step shapes the hardware exceeds the derived bound with an FP8 operand (a
    finding about the instruction, DESIGN.md 3.8: measured worst 3.1e-5 at K = 24 against
    1.9e-6), so there the assertion is twice the worst measured ratio
    (mx_gemm_cases.accumulation_bound)."""
    from data_free_quantization_amd import mx
    M, N, K = shape
    g = torch.Generator().manual_seed(M * 131 + N * 17 + K)
    a = (torch.randn(M, K, generator=g) * 0.7).cuda()
    b = (torch.randn(N, K, generator=g) * 0.05).cuda()
    ai, bi = mx.mx_quantize([mx.allocate(a, a_fmt), mx.allocate(b, b_fmt)])
    got = mx.mx_gemm(ai.codes, ai.scales, a_fmt, bi.codes, bi.scales, b_fmt, K)
    ad = mx.mx_dequantize(ai.codes, ai.scales, (M, K), a_fmt).double().cpu().numpy()
    bd = mx.mx_dequantize(bi.codes, bi.scales, (N, K), b_fmt).double().cpu().numpy()
    assert np.array_equal(ad, ai.dst.double().cpu().numpy())
    exact, mass = ad @ bd.T, np.abs(ad) @ np.abs(bd).T
    err = np.abs(got.double().cpu().numpy() - exact)
    ratio = float((err / mass).max())
    bound = GC.accumulation_bound(mx.blocks(K))
    if shape in RANDOM_SHAPES:
        assert bound == 32 * mx.blocks(K) * 2.0 ** -24   # the issue's cases: the derived bound itself
    print("mx_gemm %s x %s %s: worst |acc - exact| / sum|a*b| = %.3e (asserted %.3e, %.4f of it; derived %.3e)"
          % (a_fmt, b_fmt, shape, ratio, bound, ratio / bound, 32 * mx.blocks(K) * 2.0 ** -24))
    assert (err <= bound * mass).all(), (ratio, bound)


def test_an_all_zero_block_contributes_nothing():
    from data_free_quantization_amd import mx
    shape = (17, 33, 96)
    av, asc, bv, bsc, _ = GC.exact_case(*shape)
    av, asc = av.copy(), asc.copy()
    av[3, 32:64] = 0.0
    asc[3, 1] = 0   # what the quantizer writes for a block of zeros: +0 codes, scale byte 0
    want = (GC.quarter_units(av, np.where(asc == 0, 127, asc).astype(np.uint8)) @ GC.quarter_units(bv, bsc).T) / 16.0
    for a_fmt, b_fmt in (("mxfp4", "mxfp8"), ("mxfp8", "mxfp6_e2m3"), ("mxfp6_e3m2", "mxfp4")):
        ac, as_ = GC.encode(av, asc, a_fmt)
        bc, bs = GC.encode(bv, bsc, b_fmt)
        assert (ac[3, 1] == 0).all() and as_[3, 1] == 0
        got = mx.mx_gemm(_dev(ac), _dev(as_), a_fmt, _dev(bc), _dev(bs), b_fmt, shape[2])
        assert np.array_equal(_bits(got), want.astype(np.float32).view(np.uint32)), (a_fmt, b_fmt)
        # and as the B operand
        got = mx.mx_gemm(_dev(bc), _dev(bs), b_fmt, _dev(ac), _dev(as_), a_fmt, shape[2])
        assert np.array_equal(_bits(got), want.T.astype(np.float32).view(np.uint32)), (a_fmt, b_fmt)


@pytest.mark.parametrize("shape", [(17, 33, 96), (200, 24, 144)], ids=lambda s: "x".join(map(str, s)))
def test_bias_and_a_row_stride(shape):
    """One fp32 add of bias[n] after the accumulation; with ldo > N the columns past N of
    every row keep what they held."""
    from data_free_quantization_amd import mx
    M, N, K = shape
    ac, as_, bc, bs, want = _operands(shape, "mxfp8", "mxfp4")
    bias = np.random.default_rng(5).integers(-64, 64, N).astype(np.float32) / 4   # exact sums
    wide = torch.full((M, N + 5), -7.25, dtype=torch.float32, device="cuda")
    got = mx.mx_gemm(ac, as_, "mxfp8", bc, bs, "mxfp4", K, bias=_dev(bias), out=wide[:, :N])
    assert got.data_ptr() == wide.data_ptr()
    assert np.array_equal(_bits(wide[:, :N]), (want + bias[None, :]).view(np.uint32))
    assert (wide[:, N:] == -7.25).all()
    # a bias that rounds: still one fp32 add
    bias = np.random.default_rng(6).standard_normal(N).astype(np.float32)
    got = mx.mx_gemm(ac, as_, "mxfp8", bc, bs, "mxfp4", K, bias=_dev(bias))
    assert np.array_equal(_bits(got), (want + bias[None, :]).astype(np.float32).view(np.uint32))


def test_same_bits_from_run_to_run_and_at_another_address():
    from data_free_quantization_amd import mx
    M, N, K = 32, 48, 416
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(M, K, generator=g).cuda(), torch.randn(N, K, generator=g).cuda()
    ai, bi = mx.mx_quantize([mx.allocate(a, "mxfp6_e2m3"), mx.allocate(b, "mxfp4")])
    run = lambda ac, as_, bc, bs, **k: mx.mx_gemm(ac, as_, "mxfp6_e2m3", bc, bs, "mxfp4", K, **k)   # noqa: E731
    first = run(ai.codes, ai.scales, bi.codes, bi.scales)
    again = run(ai.codes, ai.scales, bi.codes, bi.scales)
    assert np.array_equal(_bits(first), _bits(again))

    def moved(t, off):   # the same bytes `off` bytes into another allocation
        buf = torch.empty(t.numel() + off, dtype=torch.uint8, device="cuda")
        buf[off:].copy_(t.reshape(-1))
        return buf[off:].view(t.shape)

    wide = torch.zeros(M, N + 16, dtype=torch.float32, device="cuda")
    other = run(moved(ai.codes, 8), moved(ai.scales, 3), moved(bi.codes, 48), moved(bi.scales, 1), out=wide[:, 11:11 + N])
    assert np.array_equal(_bits(first), _bits(other))


@pytest.mark.parametrize("fmt", GC.FMTS)
def test_mx_linear_on_a_stored_mx_weight_multiplies_its_own_codes(fmt):
    """Idempotence on the device: mx_linear re-quantizes a weight quantize_targ_layer left
    on the MX grid and must land on that call's own codes and scales."""
    from data_free_quantization_amd import mx
    from data_free_quantization_amd.utils.layer_transform import quantize_targ_layer
    torch.manual_seed(11)
    layer = torch.nn.Linear(200, 37).cuda()
    graph, state = {0: layer}, {}
    quantize_targ_layer(graph, 8, 8, (torch.nn.Linear,), state=state, weight_format=fmt)
    x = torch.randn(9, 200, device="cuda")
    with torch.no_grad():
        got = mx.mx_linear(x, layer.weight, layer.bias, fmt, "mxfp8")
        xi = mx.mx_quantize([mx.allocate(x, "mxfp8", want_dst=False)])[0]
        want = mx.mx_gemm(xi.codes, xi.scales, "mxfp8", state[0]["codes"], state[0]["scales"], fmt, 200, bias=layer.bias)
        wi = mx.mx_quantize([mx.allocate(layer.weight.detach(), fmt, want_dst=False)])[0]
    assert torch.equal(wi.codes, state[0]["codes"]) and torch.equal(wi.scales, state[0]["scales"])
    assert got.shape == (9, 37) and np.array_equal(_bits(got), _bits(want))


def test_python_argument_checks_on_the_device():
    from data_free_quantization_amd import mx
    ac, as_, bc, bs, _ = _operands((17, 33, 96), "mxfp4", "mxfp8")
    with pytest.raises(ValueError):
        mx.mx_gemm(ac, as_, "mxfp4", bc, bs, "mxfp8", 128)          # nb does not match K
    with pytest.raises(ValueError):
        mx.mx_gemm(ac, as_, "mxfp8", bc, bs, "mxfp8", 96)           # code bytes do not match the format
    with pytest.raises(ValueError):
        mx.mx_gemm(ac.view(-1)[1:], as_, "mxfp4", bc, bs, "mxfp8", 96)
    with pytest.raises(TypeError):
        mx.mx_gemm(ac.float(), as_, "mxfp4", bc, bs, "mxfp8", 96)
    with pytest.raises(ValueError):
        mx.mx_gemm(ac, as_, "mxfp4", bc, bs, "mxfp8", 96, out=torch.empty(17, 32, device="cuda"))
    with pytest.raises(ValueError):
        mx.mx_gemm(ac, as_, "mxfp4", bc, bs, "mxfp8", 96, bias=torch.zeros(32, device="cuda"))
    with pytest.raises(TypeError):
        mx.mx_gemm(ac, as_, "mxfp4", bc, bs, "mxfp8", 96, out=torch.empty(17, 33, device="cuda", dtype=torch.float64))
