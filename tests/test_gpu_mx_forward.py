"""utils.quantize.mx_matmul_forward: inside the scope a Quant* layer marked with an MX
weight format multiplies through mx.mx_linear (the scaled matrix instruction) instead of
F.linear / F.conv2d; everything else is what it was."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import mx_gemm_cases as GC

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _marked(layer, fmt="mxfp4"):
    """The layer with its weight on the MX grid and marked, as quantize_targ_layer leaves it; fixed observer."""
    from data_free_quantization_amd.utils.layer_transform import quantize_targ_layer
    layer = layer.to(DEV).eval()
    quantize_targ_layer({0: layer}, 8, 8, (type(layer),), weight_format=fmt)
    assert layer.weight_format == fmt
    return layer


def _observed(layer, x):
    """Fix the activation observer's range on x (one training-mode call), then freeze it."""
    layer.quant.train()
    with torch.no_grad():
        layer.quant(x)
    layer.eval()
    return layer


def _reference(layer, x2d_of, back):
    """float64 product of the dequantized MXFP8 input and the dequantized MXFP4 weight, both
    through mx_quantize / mx_dequantize here, plus the layer's fake-quantized bias; and the
    contract's bound on the accumulation (include/dfq_hip.h; at these K, one K step, the
    measured allowance of mx_gemm_cases.accumulation_bound: with the derived 32 nb 2^-24 the
    linear layer passes at 0.003 of the allowance and the K = 24 convolution misses it at
    1.39 times -- the instruction's own error)."""
    from data_free_quantization_amd import mx
    with torch.no_grad():
        xq = layer.quant(x2d_of[0])
        _, qbias = layer._qparams(layer.weight, layer.bias)
    x2d = x2d_of[1](xq).contiguous()
    w2d = layer.weight.detach().reshape(layer.weight.shape[0], -1).contiguous()
    xi, wi = mx.mx_quantize([mx.allocate(x2d, "mxfp8"), mx.allocate(w2d, "mxfp4")])
    xd = mx.mx_dequantize(xi.codes, xi.scales, x2d.shape, "mxfp8").double()
    wd = mx.mx_dequantize(wi.codes, wi.scales, w2d.shape, "mxfp4").double()
    assert torch.equal(wd.float(), w2d)   # the stored weight is on its grid
    exact, mass = xd @ wd.T, xd.abs() @ wd.abs().T
    bound = GC.accumulation_bound(mx.blocks(x2d.shape[1])) * mass
    # the bias is one fp32 add of the fp32 accumulator: half an ulp of the result on top
    return back(exact), back(bound), qbias


def _check(got, exact, bound, qbias, bias_shape):
    b = qbias.double().view(bias_shape)
    want = exact + b
    slack = bound + 2.0 ** -24 * (want.abs() + bound)
    err = (got.double() - want).abs()
    print("worst error / allowance: %.3f" % float((err / slack.clamp_min(1e-300)).max()))
    assert (err <= slack).all()


def test_linear_layer_inside_and_outside_the_scope():
    from data_free_quantization_amd import mx
    from data_free_quantization_amd.utils.quantize import QuantLinear, mx_matmul_forward
    torch.manual_seed(0)
    x = torch.randn(7, 96, device=DEV)
    layer = _observed(_marked(QuantLinear(96, 40)), x)
    plain = _observed(QuantLinear(96, 40).to(DEV), x)   # unmarked
    with torch.no_grad():
        def parent(m):   # the parent commit's forward
            return F.linear(m.quant(x), *m._qparams(m.weight, m.bias))
        want_outside, want_plain = parent(layer), parent(plain)
        assert torch.equal(layer(x), want_outside)
        with mx_matmul_forward("mxfp8"):
            got = layer(x)
            assert mx.LINEAR_CALLS == 1
            assert torch.equal(plain(x), want_plain) and mx.LINEAR_CALLS == 1
        assert torch.equal(layer(x), want_outside) and mx.LINEAR_CALLS == 1
    exact, bound, qbias = _reference(layer, (x, lambda t: t), lambda t: t)
    _check(got, exact, bound, qbias, (1, -1))
    assert not torch.equal(got, want_outside)   # the activations were rounded to MXFP8


def test_pointwise_conv_with_a_stride():
    from data_free_quantization_amd import mx
    from data_free_quantization_amd.utils.quantize import QuantConv2d, mx_matmul_forward
    torch.manual_seed(1)
    x = torch.randn(2, 24, 7, 7, device=DEV)
    layer = _observed(_marked(QuantConv2d(24, 40, 1, stride=2)), x)
    plain = _observed(QuantConv2d(24, 40, 1, stride=2).to(DEV), x)
    spatial = _observed(_marked(QuantConv2d(24, 40, 3, padding=1)), x)   # marked, not eligible
    with torch.no_grad():
        def parent(m):
            return F.conv2d(m.quant(x), *m._qparams(m.weight, m.bias), m.stride, m.padding, m.dilation, m.groups)
        want_outside, want_plain, want_spatial = parent(layer), parent(plain), parent(spatial)
        assert torch.equal(layer(x), want_outside)
        with mx_matmul_forward("mxfp8"):
            got = layer(x)
            assert mx.LINEAR_CALLS == 1
            assert torch.equal(plain(x), want_plain) and torch.equal(spatial(x), want_spatial)
            assert mx.LINEAR_CALLS == 1
        assert torch.equal(layer(x), want_outside)
    assert got.shape == want_outside.shape == (2, 40, 4, 4) and got.is_contiguous()
    to2d = lambda t: t[:, :, ::2, ::2].permute(0, 2, 3, 1).reshape(-1, 24)   # noqa: E731
    back = lambda t: t.view(2, 4, 4, 40).permute(0, 3, 1, 2)                 # noqa: E731
    exact, bound, qbias = _reference(layer, (x, to2d), back)
    _check(got, exact, bound, qbias, (1, -1, 1, 1))


def test_frozen_weights_keeps_the_codes_and_sees_new_weights():
    from data_free_quantization_amd import mx
    from data_free_quantization_amd.utils.quantize import (QuantLinear, frozen_weights, invalidate_weight_cache,
                                                           mx_matmul_forward)
    torch.manual_seed(2)
    x = torch.randn(5, 96, device=DEV)
    layer = _observed(_marked(QuantLinear(96, 40)), x)
    with torch.no_grad(), mx_matmul_forward("mxfp8"):
        free = layer(x)
        with frozen_weights():
            first = layer(x)
            codes = layer.__dict__["_mx_w_cache"][1]
            again = layer(x)
            assert layer.__dict__["_mx_w_cache"][1] is codes
            layer.weight.data.mul_(2.0)   # stays on the MX grid: every scale byte moves by one
            invalidate_weight_cache()
            doubled = layer(x)
            assert layer.__dict__["_mx_w_cache"][1] is not codes
    assert torch.equal(free, first) and torch.equal(first, again)
    assert not torch.equal(doubled, first)


def test_quantized_mobilenetv2_routes_every_eligible_layer():
    """The zoo's MobileNetV2 after run_dfq(weight_format="mxfp4"), batch 2 at 32 x 32 (the
    smallest input its stride of 32 supports): finite inside the scope, every eligible
    module routed once.  The logits' SQNR against the plain forward is printed, not asserted."""
    from data_free_quantization_amd import mx, pipeline, zoo
    from data_free_quantization_amd.utils import layer_transform as L
    from data_free_quantization_amd.utils.quantize import QuantConv2d, QuantLinear, mx_matmul_forward
    from data_free_quantization_amd.utils.tracer import TorchTransformer
    model = zoo.build("mobilenetv2", seed=0, relu=True).to(DEV).eval()
    x = torch.randn(2, 3, 32, 32, device=DEV)
    tr = TorchTransformer("positional")
    model, tr = L.switch_layers(model, tr, x, {1: [(nn.Conv2d, QuantConv2d), (nn.Linear, QuantLinear)]})
    graph, bottoms = tr.log.getGraph(), tr.log.getBottoms()
    targ = (QuantConv2d, QuantLinear)
    try:
        pipeline.run_dfq(model, graph, bottoms, targ, weight_format="mxfp4", bc_mode="fused", clip=False)
        L.set_quant_minmax(graph, bottoms, verbose=False)
        model.eval()
        for m in graph.values():   # fixed observers, so every forward sees the same ranges
            if hasattr(m, "quant"):
                m.quant.update_stat = False
        for q in L.module_tensor_op.quants:
            q.update_stat = False
        eligible = [m for m in model.modules()
                    if isinstance(m, QuantLinear) or (isinstance(m, QuantConv2d) and tuple(m.kernel_size) == (1, 1) and
                                                      m.groups == 1 and tuple(m.padding) == (0, 0))]
        assert len(eligible) > 30 and all(m.weight_format == "mxfp4" for m in eligible)
        L.replace_op()
        try:
            with torch.no_grad():
                plain = model(x)
                with mx_matmul_forward("mxfp8"):
                    routed = model(x)
                    calls = mx.LINEAR_CALLS
                assert torch.equal(model(x), plain)   # outside the scope again: the parent's forward
        finally:
            L.restore_op()
    finally:
        L.module_tensor_op = None
    assert torch.isfinite(routed).all() and routed.shape == plain.shape
    assert calls == len(eligible)
    noise = (routed.double() - plain.double()).pow(2).sum()
    print("MobileNetV2 mxfp4 weights, mxfp8 activations on the matrix instruction: %d layers routed, logits SQNR "
          "%.2f dB against the plain forward" % (calls, 10 * np.log10(float(plain.double().pow(2).sum() / noise))))


def test_main_dfq_refuses_mx_matmul_without_an_mx_weight_format():
    from data_free_quantization_amd import main_dfq
    with pytest.raises(SystemExit):
        main_dfq.get_argument(["--quantize", "--mx_matmul", "mxfp8"])
