"""Integer matrix multiply on the i8 matrix instruction for the sweep's integer codes.

Host wrappers of ``dfq_int_gemm``, ``dfq_int_linear``, ``dfq_int_conv2d`` and ``dfq_int_dwconv2d`` (include/dfq_hip.h;
DESIGN.md 3.9): ``int_gemm`` multiplies two operands given as the integer codes, scales and
zeros the sweep (or ``utils.quantize.fake_quant``) writes -- uint8 / int8 bytes, or packed INT4
nibbles for B -- ``int_linear`` multiplies an fp32 input, quantized inside the kernel by
``fake_quant_given``'s quantizer, with such a B in one launch, and ``int_conv2d`` does that on
the im2col rows of an NCHW input, gathered inside the kernel, with zero padding standing for
the real value 0; ``int_dwconv2d`` is the depthwise convolution (groups == C) on the packed
8-bit dot instruction, each input element quantized once.  The integer sums are exact
and the affine terms are applied in fp64 in a fixed order, so every output is bit for bit a
numpy float64 statement (tests/int_gemm_cases.py).  ``b_group`` (``int_gemm``, ``int_linear``)
and ``int_conv2d_grouped`` take group-wise weight parameters, a scale and zero per 32, 64, 128, ...
elements of a weight row (``group_quant`` writes them; tests/int_group_cases.py).  ``out_quant``
(``int_gemm``, ``int_linear``) and ``int_conv2d_q`` / ``int_dwconv2d_q`` store the next layer's
activation codes instead of fp32, and the two convolutions read such codes (``x_codes``), so a
run of layers exchanges uint8 tensors (tests/int_io_cases.py); ``int_mbconv_q`` runs MobileNetV2's
expand -> depthwise -> project block on such codes in one launch, the hidden tensors in LDS, with the block's residual add in its
epilogue under ``residual``; ``int_add_q`` adds two code tensors; ``int_mean_q`` and ``int_maxpool2d_q`` are the classifiers'
global average pool and max pool on such codes.
There is no CPU fallback: CPU tensors raise."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib, mx

MAX_K = _lib.DFQ_INT_MAX_K
DW_MAX_TAPS = _lib.DFQ_INT_DW_MAX_TAPS
_CODE_DTYPES = (torch.uint8, torch.int8)


def _on_gpu(name: str, t, what: str) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: %s on the GPU" % (name, what))
    if not t.is_cuda:
        raise RuntimeError("data_free_quantization_amd multiplies integer codes on a ROCm GPU only; "
                           "%s is on %s (there is no CPU fallback)" % (name, t.device))


def _codes_arg(name: str, codes, K: int, packed: bool = False) -> int:
    """The checks of a code operand; its row count."""
    _on_gpu(name, codes, "a uint8 or int8 tensor")
    if codes.dtype not in _CODE_DTYPES or not codes.is_contiguous():
        raise TypeError(name + ": contiguous uint8 or int8 on the GPU")
    if packed and K % 2:
        raise ValueError("packed codes need an even K (every row starts on a byte), got %d" % K)
    row_bytes = K // 2 if packed else K
    if codes.numel() < row_bytes or codes.numel() % row_bytes:
        raise ValueError("%s holds %d bytes, no whole number of rows of %d" % (name, codes.numel(), row_bytes))
    if codes.data_ptr() % 16:
        raise ValueError(name + " must be 16-byte aligned")
    return codes.numel() // row_bytes


def _param_arg(name: str, t, counts, optional: bool = False):
    """A scale or zero: fp32 on the GPU with one of ``counts`` elements."""
    if t is None and optional:
        return None
    _on_gpu(name, t, "a float32 tensor")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise TypeError(name + ": contiguous float32 on the GPU")
    if t.numel() not in counts:
        raise ValueError("%s holds %d values, %s needed" % (name, t.numel(), " or ".join(str(c) for c in counts)))
    return t


def _k_arg(K) -> int:
    K = int(K)
    if K < 1:
        raise ValueError("K must be >= 1")
    if K > MAX_K:
        raise ValueError("K must be <= %d (the integer sums stay inside int32), got %d" % (MAX_K, K))
    return K


def group_allowed(b_group: int) -> bool:
    """The group sizes the kernels take: 32 (half a K step), or a multiple of 64 up to MAX_K."""
    return b_group == 32 or (64 <= b_group <= MAX_K and b_group % 64 == 0)


def _group_arg(b_group) -> Optional[int]:
    if b_group is None:
        return None
    b_group = int(b_group)
    if not group_allowed(b_group):
        raise ValueError("b_group must be 32 or a multiple of 64 up to %d, got %d" % (MAX_K, b_group))
    return b_group


def _b_args(d, b_codes, b_scale, b_zero, K: int, b_packed: bool, b_group: Optional[int] = None) -> int:
    """B's checks and descriptor fields (shared by the descriptors); N.  ``b_group``: the
    parameters are [N, ceil(K / b_group)] and DFQ_INT_B_PER_ROW stays clear."""
    N = _codes_arg("b_codes", b_codes, K, b_packed)
    if b_group is not None:
        _param_arg("b_scale", b_scale, (N * -(-K // b_group),))
        _param_arg("b_zero", b_zero, (b_scale.numel(),), optional=True)
        d.b_codes, d.b_scale = b_codes.data_ptr(), b_scale.data_ptr()
        d.b_zero = b_zero.data_ptr() if b_zero is not None else None
        d.b_signed = int(b_codes.dtype == torch.int8)
        d.flags |= _lib.DFQ_INT_B_PACK4 if b_packed else 0
        return N
    _param_arg("b_scale", b_scale, (1, N) if N > 1 else (1,))
    _param_arg("b_zero", b_zero, (b_scale.numel(),), optional=True)
    d.b_codes, d.b_scale = b_codes.data_ptr(), b_scale.data_ptr()
    d.b_zero = b_zero.data_ptr() if b_zero is not None else None
    d.b_signed = int(b_codes.dtype == torch.int8)
    # N == 1: one value either way
    d.flags |= (_lib.DFQ_INT_B_PACK4 if b_packed else 0) | (_lib.DFQ_INT_B_PER_ROW if b_scale.numel() > 1 else 0)
    return N


def _range_fields(min_dev, max_dev, min_value, max_value, scale_f32: bool):
    """A quantizer's range: its checks; (min_dev, max_dev, given_min, given_max, flags) as a descriptor or io struct takes them."""
    for name, dev_v, host_v in (("min", min_dev, min_value), ("max", max_dev, max_value)):
        if dev_v is not None:
            _param_arg(name + "_dev", dev_v, (1,))
        elif host_v is None:
            raise ValueError("the range's %s is missing: pass %s_dev or %s_value" % (name, name, name))
    return (min_dev.data_ptr() if min_dev is not None else None, max_dev.data_ptr() if max_dev is not None else None,
            float(min_value) if min_value is not None else 0.0, float(max_value) if max_value is not None else 0.0,
            _lib.DFQ_SCALE_F32 if scale_f32 else 0)


def _range_args(d, min_dev, max_dev, min_value, max_value, scale_f32: bool) -> None:
    """The input quantizer's range (int_linear's and the convolutions')."""
    d.min_dev, d.max_dev, d.given_min, d.given_max, d.flags = _range_fields(min_dev, max_dev, min_value, max_value, scale_f32)


@dataclass
class OutQuant:
    """The grid a call stores its result on as codes (dfq_int_io): ``fake_quant_given``'s
    arguments -- ``bits`` 2..8, ``symmetric`` (int8 bytes, else uint8), the range from the device
    scalars ``min_dev`` / ``max_dev`` or the Python floats ``min_value`` / ``max_value``,
    ``scale_f32`` as there.  On a range with min = 0 (and max <= 6) the clamp is the ReLU (ReLU6)."""
    bits: int = 8
    symmetric: bool = False
    min_dev: Optional[torch.Tensor] = None
    max_dev: Optional[torch.Tensor] = None
    min_value: Optional[float] = None
    max_value: Optional[float] = None
    scale_f32: bool = False


def _code_dtype(symmetric) -> torch.dtype:
    return torch.int8 if symmetric else torch.uint8


def _io_arg(out_quant: Optional[OutQuant], x_codes: bool) -> Optional[_lib.IntIo]:
    """The io struct of a call, None when the call is the old entry's; ``out_quant``'s checks."""
    if out_quant is None and not x_codes:
        return None
    io = _lib.IntIo()
    io.x_codes = int(bool(x_codes))
    if out_quant is None:
        return io
    if not isinstance(out_quant, OutQuant):
        raise TypeError("out_quant: an intmm.OutQuant")
    if not 2 <= int(out_quant.bits) <= 8:
        raise ValueError("out_quant.bits must be 2..8, got %d" % out_quant.bits)
    io.out_min_dev, io.out_max_dev, io.out_given_min, io.out_given_max, io.out_flags = _range_fields(
        out_quant.min_dev, out_quant.max_dev, out_quant.min_value, out_quant.max_value, out_quant.scale_f32)
    if out_quant.min_dev is None and out_quant.max_dev is None and not io.out_given_max > io.out_given_min:
        raise ValueError("out_quant: max_value must be above min_value")
    io.out_bits, io.out_symmetric = int(out_quant.bits), int(bool(out_quant.symmetric))
    return io


def _code_out(what: str, shape, out, out_quant: OutQuant, dev, rows_strided: bool = False) -> torch.Tensor:
    """The byte tensor a call with ``out_quant`` stores into: ``out``'s checks, or a new one."""
    dtype = _code_dtype(out_quant.symmetric)
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != dtype:
        raise TypeError("%s: out must be %s on the GPU under this out_quant" % (what, dtype))
    ok = out.stride(-1) == 1 and (out.shape[0] == 1 or out.stride(0) >= shape[1]) if rows_strided and out.dim() == 2 else out.is_contiguous()
    if tuple(out.shape) != tuple(shape) or not ok:
        raise ValueError("%s: out must be a %s tensor%s" % (what, list(shape), " with unit column stride" if rows_strided else ", contiguous"))
    return out


def _bias_dev_args(what: str, N: int, dev, bias, tensors) -> None:
    """``bias``'s checks and every tensor on one device (the convolutions', and a code output's)."""
    if bias is not None:
        _lib.require_device(bias)
        if bias.numel() != N:
            raise ValueError("bias holds %d elements, %d needed" % (bias.numel(), N))
    for t in (*tensors, bias):
        if t is not None and t.device != dev:
            raise ValueError("every tensor of an %s call must live on one device" % what)


def _launch(name: str, d, b_group: Optional[int], dev, io=None) -> None:
    """The entry point ``name``, its ``_grouped`` form under a group size, or its ``_q`` form with an io struct."""
    L = _lib.load()
    if io is not None:
        if b_group is not None:
            raise ValueError("stored activation codes and group-wise B do not combine")
        name += "_q"
        rc = getattr(L, name)(C.byref(d), C.byref(io), _lib.raw_stream(dev))
    elif b_group is None:
        rc = getattr(L, name)(C.byref(d), _lib.raw_stream(dev))
    else:
        name += "_grouped"
        rc = getattr(L, name)(C.byref(d), b_group, _lib.raw_stream(dev))
    _lib.check(rc, name, ValueError)


def _bias_out_args(what: str, d, M: int, N: int, K: int, dev, bias, out, others, out_quant=None) -> torch.Tensor:
    """mx.py's checks of ``bias``, ``out`` and the tensors' device; the descriptor fields both entries share.
    Under ``out_quant`` ``out`` is a byte tensor and its row stride counts bytes."""
    if out_quant is None:
        out = mx._bias_out_args(what, M, N, dev, bias, out, others)
    else:
        out = _code_out(what, (M, N), out, out_quant, dev, rows_strided=True)
        _bias_dev_args(what, N, dev, bias, (*others, out_quant.min_dev, out_quant.max_dev, out))
    d.bias = bias.data_ptr() if bias is not None else None
    d.out, d.ldo = out.data_ptr(), (out.stride(0) if M > 1 else max(out.stride(0), N))
    d.M, d.N, d.K = M, N, K
    return out


def int_gemm(a_codes: torch.Tensor, a_scale: torch.Tensor, a_zero: Optional[torch.Tensor], b_codes: torch.Tensor,
             b_scale: torch.Tensor, b_zero: Optional[torch.Tensor], K: int, *, b_packed: bool = False,
             bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
             b_group: Optional[int] = None, out_quant: Optional[OutQuant] = None) -> torch.Tensor:
    """out[m, n] = sum_k (qa[m, k] * sa + za) * (qb[n, k] * sb[n] + zb[n]) (+ bias[n]) on the
    i8 matrix instruction (dfq_int_gemm).  ``a_codes``: M * K bytes, ``b_codes``:
    N * K bytes -- or N * K / 2 packed bytes with ``b_packed`` (the sweep's ``pack_int4`` layout,
    K even) -- contiguous, rows of K elements; uint8 codes are unsigned and int8 codes signed
    (packed nibbles are two's complement when the tensor is int8: view the sweep's packed
    symmetric codes as int8).  ``a_scale`` / ``a_zero``: one fp32 value each; ``b_scale`` /
    ``b_zero``: one value each, or N (per output channel); a zero may be None (0).  ``out``:
    fp32 [M, N] whose rows may be strided; allocated when None.  The result is the contract's
    fp64 statement bit for bit.  One launch, asynchronous on the current stream.

    ``b_group`` (32, or a multiple of 64): group-wise B -- ``b_scale`` / ``b_zero`` hold
    [N, ceil(K / b_group)] values, one per ``b_group`` consecutive elements of a row (the last
    group may be short; ``group_quant`` writes them), and the result is the grouped statement
    (dfq_int_gemm_grouped): the groups' fp64 terms in ascending order.  One group (b_group >= K)
    gives the per-row call's bits.  A disallowed size or a wrong count raises ValueError.

    ``out_quant`` (an ``OutQuant``; dfq_int_gemm_q): the result is stored as codes -- byte [m, n]
    is ``fake_quant``'s code of the fp32 statement above on ``out_quant``'s range, uint8, or int8
    when symmetric -- and ``out``, if passed, is such a [M, N] byte tensor (rows may be strided).
    Not with ``b_group``."""
    K = _k_arg(K)
    b_group = _group_arg(b_group)
    io = _io_arg(out_quant, False)
    M = _codes_arg("a_codes", a_codes, K)
    _param_arg("a_scale", a_scale, (1,))
    _param_arg("a_zero", a_zero, (1,), optional=True)
    d = _lib.IntGemmDesc()
    N = _b_args(d, b_codes, b_scale, b_zero, K, bool(b_packed), b_group)
    dev = a_codes.device
    out = _bias_out_args("int_gemm", d, M, N, K, dev, bias, out, (a_scale, a_zero, b_codes, b_scale, b_zero), out_quant)
    d.a_codes, d.a_scale = a_codes.data_ptr(), a_scale.data_ptr()
    d.a_zero = a_zero.data_ptr() if a_zero is not None else None
    d.a_signed = int(a_codes.dtype == torch.int8)
    _launch("dfq_int_gemm", d, b_group, dev, io)
    return out


#: int_linear calls since the last reset (utils.quantize.int_matmul_forward resets it on entry)
LINEAR_CALLS = 0


def reset_linear_calls() -> None:
    global LINEAR_CALLS
    LINEAR_CALLS = 0


def int_linear(x: torch.Tensor, b_codes: torch.Tensor, b_scale: torch.Tensor, b_zero: Optional[torch.Tensor], K: int, *,
               bits: int = 8, symmetric: bool = False, min_dev: Optional[torch.Tensor] = None,
               max_dev: Optional[torch.Tensor] = None, min_value=None, max_value=None, scale_f32: bool = False,
               b_packed: bool = False, bias: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None, b_group: Optional[int] = None,
               out_quant: Optional[OutQuant] = None) -> torch.Tensor:
    """``int_gemm`` with A given as fp32 ``x`` [M, K] and quantized to ``bits`` (2..8) inside the
    kernel (dfq_int_linear): the quantizer is ``fake_quant_given``'s -- the range from the
    device scalars ``min_dev`` / ``max_dev`` (no host synchronisation) or the Python floats
    ``min_value`` / ``max_value``, ``scale_f32`` as there -- and the codes of x never reach
    memory.  Bit for bit ``fake_quant`` of x on that range (codes, scale, zero) followed by
    ``int_gemm``.  ``x`` needs unit column stride; any row stride >= K is passed on (a column
    slice of a wider tensor is read in place).  B, ``bias``, ``out``, ``b_group`` and ``out_quant``
    (dfq_int_linear_q: the result stored as codes) as for ``int_gemm``."""
    global LINEAR_CALLS
    K = _k_arg(K)
    b_group = _group_arg(b_group)
    io = _io_arg(out_quant, False)
    bits = int(bits)
    if not 2 <= bits <= 8:
        raise ValueError("bits must be 2..8, got %d" % bits)
    _on_gpu("x", x, "a float32 tensor")
    if x.dtype != torch.float32:
        raise TypeError("x: float32 on the GPU")
    if x.dim() != 2 or x.shape[1] != K or x.shape[0] < 1 or x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < K):
        raise ValueError("x must be [M, %d] with unit column stride and a row stride >= %d, got %s with strides %s"
                         % (K, K, tuple(x.shape), tuple(x.stride())))
    d = _lib.IntLinearDesc()
    _range_args(d, min_dev, max_dev, min_value, max_value, scale_f32)
    N = _b_args(d, b_codes, b_scale, b_zero, K, bool(b_packed), b_group)
    M, dev = x.shape[0], x.device
    out = _bias_out_args("int_linear", d, M, N, K, dev, bias, out, (min_dev, max_dev, b_codes, b_scale, b_zero), out_quant)
    d.x, d.ldx = x.data_ptr(), (x.stride(0) if M > 1 else max(x.stride(0), K))
    d.x_bits, d.x_symmetric = bits, int(bool(symmetric))
    _launch("dfq_int_linear", d, b_group, dev, io)
    LINEAR_CALLS += 1
    return out


def int_conv2d(x: torch.Tensor, b_codes: torch.Tensor, b_scale: torch.Tensor, b_zero: Optional[torch.Tensor], kernel_size,
               stride=1, padding=0, dilation=1, *, bits: int = 8, symmetric: bool = False,
               min_dev: Optional[torch.Tensor] = None, max_dev: Optional[torch.Tensor] = None, min_value=None,
               max_value=None, scale_f32: bool = False, b_packed: bool = False, bias: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The convolution (groups == 1, zero padding) of the affine values the codes stand for, in
    one launch (dfq_int_conv2d): ``x`` fp32 contiguous NCHW [B, C, H, W], read in
    place and quantized to ``bits`` inside the kernel as ``int_linear`` quantizes its input; B the
    weight [N, C, KH, KW] as codes with rows of K = C * KH * KW elements along (c, kh, kw) --
    ``fake_quant(weight.reshape(N, -1))``'s -- with ``b_scale`` / ``b_zero`` / ``b_packed`` as for
    ``int_gemm``.  A padding tap has the real value 0, as in ``F.conv2d`` of the fake-quantized
    input: it is absent from every sum, not the code of 0.0 (which ``int_linear`` on ``F.unfold``'s
    matrix would use).  Where the geometry has no padding the result is bit for bit ``int_linear``
    on that matrix, reshaped to NCHW.  ``kernel_size``, ``stride``, ``padding``, ``dilation``: ints
    or (h, w) pairs.  ``out``: fp32 contiguous [B, N, OH, OW]; allocated when None.  Counts in
    ``LINEAR_CALLS``.  Asynchronous on the current stream."""
    return _conv2d(x, b_codes, b_scale, b_zero, kernel_size, stride, padding, dilation, None, bits, symmetric, min_dev, max_dev,
                   min_value, max_value, scale_f32, b_packed, bias, out)


def int_conv2d_grouped(x: torch.Tensor, b_codes: torch.Tensor, b_scale: torch.Tensor, b_zero: Optional[torch.Tensor], kernel_size,
                       stride=1, padding=0, dilation=1, *, b_group: int, bits: int = 8, symmetric: bool = False,
                       min_dev: Optional[torch.Tensor] = None, max_dev: Optional[torch.Tensor] = None, min_value=None,
                       max_value=None, scale_f32: bool = False, b_packed: bool = False,
                       bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``int_conv2d`` with group-wise B (dfq_int_conv2d_grouped): ``b_group`` as for ``int_gemm``,
    ``b_scale`` / ``b_zero`` [N, ceil(K / b_group)], the groups running along (c, kh, kw), the
    order the weight is stored in; a group's constant term counts its taps inside the image.
    (Its own function: ``int_conv2d`` and ``int_dwconv2d`` keep one signature.)"""
    if b_group is None:
        raise ValueError("b_group must be 32 or a multiple of 64")
    return _conv2d(x, b_codes, b_scale, b_zero, kernel_size, stride, padding, dilation, _group_arg(b_group), bits, symmetric,
                   min_dev, max_dev, min_value, max_value, scale_f32, b_packed, bias, out)


def _x_arg(x, bits, symmetric, x_codes: bool) -> int:
    """The checks of a convolution's ``bits`` and of ``x``'s type: fp32, or under ``x_codes`` the bytes ``symmetric`` names."""
    bits = int(bits)
    if not 2 <= bits <= 8:
        raise ValueError("bits must be 2..8, got %d" % bits)
    if x_codes and isinstance(x, torch.Tensor) and x.dtype != _code_dtype(symmetric):
        raise TypeError("x: stored codes are %s when symmetric=%s, got %s" % (_code_dtype(symmetric), bool(symmetric), x.dtype))
    _on_gpu("x", x, "a uint8 or int8 tensor" if x_codes else "a float32 tensor")
    if not x_codes and x.dtype != torch.float32:
        raise TypeError("x: float32 on the GPU")
    return bits


def _conv_out(what: str, shape, out, out_quant, dev) -> torch.Tensor:
    if out_quant is not None:
        return _code_out(what, shape, out, out_quant, dev)
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=dev)
    if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float32:
        raise TypeError("out: float32 on the GPU")
    if tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise ValueError("out must be a contiguous [%d, %d, %d, %d] tensor" % tuple(shape))
    return out


def _conv2d(x, b_codes, b_scale, b_zero, kernel_size, stride, padding, dilation, b_group, bits, symmetric, min_dev, max_dev,
            min_value, max_value, scale_f32, b_packed, bias, out, io=None, out_quant=None) -> torch.Tensor:
    """int_conv2d's, int_conv2d_grouped's and int_conv2d_q's checks and launch."""
    global LINEAR_CALLS
    bits = _x_arg(x, bits, symmetric, io is not None and io.x_codes)
    (KH, KW), (sh, sw) = mx._pair(kernel_size, "kernel_size"), mx._pair(stride, "stride")
    (ph, pw), (dh, dw) = mx._pair(padding, "padding"), mx._pair(dilation, "dilation")
    if min(KH, KW, sh, sw, dh, dw) < 1 or min(ph, pw) < 0:
        raise ValueError("kernel_size, stride and dilation must be >= 1 and padding >= 0")
    if x.dim() != 4 or not x.is_contiguous() or x.numel() == 0:
        raise ValueError("x must be a contiguous [B, C, H, W] tensor, got %s with strides %s" % (tuple(x.shape), tuple(x.stride())))
    B, Cin, H, W = x.shape
    K = _k_arg(Cin * KH * KW)
    d = _lib.IntConv2dDesc()
    _range_args(d, min_dev, max_dev, min_value, max_value, scale_f32)
    N = _b_args(d, b_codes, b_scale, b_zero, K, bool(b_packed), b_group)
    OH, OW = mx.conv_out_size(H, KH, sh, ph, dh), mx.conv_out_size(W, KW, sw, pw, dw)
    if OH < 1 or OW < 1:
        raise ValueError("the kernel %s (dilation %s) does not fit the padded input %s" % ((KH, KW), (dh, dw), (H + 2 * ph, W + 2 * pw)))
    dev = x.device
    out = _conv_out("int_conv2d", (B, N, OH, OW), out, out_quant, dev)
    _bias_dev_args("int_conv2d", N, dev, bias, (min_dev, max_dev, b_codes, b_scale, b_zero, out, getattr(out_quant, "min_dev", None),
                                              getattr(out_quant, "max_dev", None)))
    d.x, d.out = x.data_ptr(), out.data_ptr()
    d.bias = bias.data_ptr() if bias is not None else None
    d.B, d.C, d.H, d.W, d.N, d.KH, d.KW = B, Cin, H, W, N, KH, KW
    d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w = sh, sw, ph, pw, dh, dw
    d.x_bits, d.x_symmetric = bits, int(bool(symmetric))
    _launch("dfq_int_conv2d", d, b_group, dev, io)
    LINEAR_CALLS += 1
    return out


def int_dwconv2d(x: torch.Tensor, b_codes: torch.Tensor, b_scale: torch.Tensor, b_zero: Optional[torch.Tensor], kernel_size,
                 stride=1, padding=0, dilation=1, *, bits: int = 8, symmetric: bool = False,
                 min_dev: Optional[torch.Tensor] = None, max_dev: Optional[torch.Tensor] = None, min_value=None,
                 max_value=None, scale_f32: bool = False, b_packed: bool = False, bias: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The depthwise convolution (groups == C, zero padding) of the affine values the codes stand
    for, in one launch on the packed 8-bit dot instruction (dfq_int_dwconv2d):
    ``x`` fp32 contiguous NCHW [B, C, H, W], read in place, every element quantized once to
    ``bits`` inside the kernel as ``int_linear`` quantizes its input; B the weight [N, 1, KH, KW] as
    codes with rows of K = KH * KW elements -- ``fake_quant(weight.reshape(N, -1))``'s -- N a
    multiple of C (output channel n reads input channel n // (N // C)), with ``b_scale`` /
    ``b_zero`` / ``b_packed`` as for ``int_gemm`` (packed needs an even K: a 3 x 3 kernel is
    refused).  K is at most ``DW_MAX_TAPS``.  A padding tap has the real value 0, as in
    ``int_conv2d``, and every channel's result is bit for bit ``int_conv2d`` on that channel alone.
    ``kernel_size``, ``stride``, ``padding``, ``dilation``: ints or (h, w) pairs.  ``out``: fp32
    contiguous [B, N, OH, OW]; allocated when None.  Counts in ``LINEAR_CALLS``.  Asynchronous on
    the current stream; there is no CPU fallback."""
    return _dwconv2d(x, b_codes, b_scale, b_zero, kernel_size, stride, padding, dilation, bits, symmetric, min_dev, max_dev,
                     min_value, max_value, scale_f32, b_packed, bias, out)


def _dwconv2d(x, b_codes, b_scale, b_zero, kernel_size, stride, padding, dilation, bits, symmetric, min_dev, max_dev,
              min_value, max_value, scale_f32, b_packed, bias, out, io=None, out_quant=None) -> torch.Tensor:
    """int_dwconv2d's and int_dwconv2d_q's checks and launch."""
    global LINEAR_CALLS
    bits = _x_arg(x, bits, symmetric, io is not None and io.x_codes)
    (KH, KW), (sh, sw) = mx._pair(kernel_size, "kernel_size"), mx._pair(stride, "stride")
    (ph, pw), (dh, dw) = mx._pair(padding, "padding"), mx._pair(dilation, "dilation")
    if min(KH, KW, sh, sw, dh, dw) < 1 or min(ph, pw) < 0:
        raise ValueError("kernel_size, stride and dilation must be >= 1 and padding >= 0")
    if x.dim() != 4 or not x.is_contiguous() or x.numel() == 0:
        raise ValueError("x must be a contiguous [B, C, H, W] tensor, got %s with strides %s" % (tuple(x.shape), tuple(x.stride())))
    B, Cin, H, W = x.shape
    K = KH * KW
    if K > DW_MAX_TAPS:
        raise ValueError("KH * KW must be <= %d (a tap mask is one 64-bit word), got %d" % (DW_MAX_TAPS, K))
    d = _lib.IntDwConv2dDesc()
    _range_args(d, min_dev, max_dev, min_value, max_value, scale_f32)
    N = _b_args(d, b_codes, b_scale, b_zero, K, bool(b_packed))
    if N % Cin:
        raise ValueError("b_codes holds %d rows of %d, no multiple of the %d input channels" % (N, K, Cin))
    OH, OW = mx.conv_out_size(H, KH, sh, ph, dh), mx.conv_out_size(W, KW, sw, pw, dw)
    if OH < 1 or OW < 1:
        raise ValueError("the kernel %s (dilation %s) does not fit the padded input %s" % ((KH, KW), (dh, dw), (H + 2 * ph, W + 2 * pw)))
    dev = x.device
    out = _conv_out("int_dwconv2d", (B, N, OH, OW), out, out_quant, dev)
    _bias_dev_args("int_dwconv2d", N, dev, bias, (min_dev, max_dev, b_codes, b_scale, b_zero, out, getattr(out_quant, "min_dev", None),
                                              getattr(out_quant, "max_dev", None)))
    d.x, d.out = x.data_ptr(), out.data_ptr()
    d.bias = bias.data_ptr() if bias is not None else None
    d.B, d.C, d.H, d.W, d.mult, d.KH, d.KW = B, Cin, H, W, N // Cin, KH, KW
    d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w = sh, sw, ph, pw, dh, dw
    d.x_bits, d.x_symmetric = bits, int(bool(symmetric))
    _launch("dfq_int_dwconv2d", d, None, dev, io)
    LINEAR_CALLS += 1
    return out


def int_conv2d_q(x: torch.Tensor, b_codes: torch.Tensor, b_scale: torch.Tensor, b_zero: Optional[torch.Tensor], kernel_size,
                 stride=1, padding=0, dilation=1, *, x_codes: bool = False, out_quant: Optional[OutQuant] = None, bits: int = 8,
                 symmetric: bool = False, min_dev: Optional[torch.Tensor] = None, max_dev: Optional[torch.Tensor] = None,
                 min_value=None, max_value=None, scale_f32: bool = False, b_packed: bool = False,
                 bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``int_conv2d`` with stored activation codes at either end (dfq_int_conv2d_q).

    ``x_codes``: ``x`` is a contiguous NCHW tensor of codes -- uint8, or int8 when ``symmetric``,
    else TypeError -- and the range keywords and ``bits`` name the grid they are on: with (s, z)
    ``fake_quant``'s scale and zero of that range, element q stands for q * s + z, exactly what the
    in-kernel quantizer of ``int_conv2d`` would have derived from the fp32 values; nothing is
    quantized on the way.  ``out_quant`` (an ``OutQuant``): byte [b, n, oh, ow] of the result is
    ``fake_quant``'s code of ``int_conv2d``'s fp32 value there -- the same integers and fp64 steps,
    bias included -- on ``out_quant``'s range, and ``out``, if passed, is a contiguous byte tensor.
    So ``int_conv2d_q(x, ..., out_quant=r)`` followed by ``int_conv2d_q(codes, ..., x_codes=True,
    **r's range)`` is bit for bit ``int_conv2d`` -> ``fake_quant_given`` -> ``int_conv2d`` with no
    fp32 activation in memory.  With neither option the result is ``int_conv2d``'s."""
    return _conv2d(x, b_codes, b_scale, b_zero, kernel_size, stride, padding, dilation, None, bits, symmetric, min_dev, max_dev,
                   min_value, max_value, scale_f32, b_packed, bias, out, _io_arg(out_quant, x_codes) or _lib.IntIo(), out_quant)


def int_dwconv2d_q(x: torch.Tensor, b_codes: torch.Tensor, b_scale: torch.Tensor, b_zero: Optional[torch.Tensor], kernel_size,
                   stride=1, padding=0, dilation=1, *, x_codes: bool = False, out_quant: Optional[OutQuant] = None, bits: int = 8,
                   symmetric: bool = False, min_dev: Optional[torch.Tensor] = None, max_dev: Optional[torch.Tensor] = None,
                   min_value=None, max_value=None, scale_f32: bool = False, b_packed: bool = False,
                   bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``int_dwconv2d`` with stored activation codes at either end (dfq_int_dwconv2d_q): ``x_codes``
    and ``out_quant`` as for ``int_conv2d_q`` -- the footprint's bytes are copied to LDS instead of
    quantized, and a lane's four outputs go out as one word of codes.  With neither option the
    result is ``int_dwconv2d``'s."""
    return _dwconv2d(x, b_codes, b_scale, b_zero, kernel_size, stride, padding, dilation, bits, symmetric, min_dev, max_dev,
                     min_value, max_value, scale_f32, b_packed, bias, out, _io_arg(out_quant, x_codes) or _lib.IntIo(), out_quant)


MB_MAX_CIN, MB_MAX_COUT = _lib.DFQ_INT_MB_MAX_CIN, _lib.DFQ_INT_MB_MAX_COUT


def _mb_quant(q, name: str, oq: OutQuant, tensors: list) -> None:
    """A grid of ``int_mbconv_q`` as the descriptor takes it: ``_io_arg``'s checks of an ``OutQuant``."""
    io = _io_arg(oq, False)
    q.min_dev, q.max_dev, q.given_min, q.given_max, q.flags = io.out_min_dev, io.out_max_dev, io.out_given_min, io.out_given_max, io.out_flags
    q.bits, q.symmetric = io.out_bits, io.out_symmetric
    tensors += [oq.min_dev, oq.max_dev]


def int_mbconv_q(x_codes: torch.Tensor, expand, depthwise, project, *, stride: int = 1, padding: int = 1, bits: int = 8,
                 symmetric: bool = False, min_dev: Optional[torch.Tensor] = None, max_dev: Optional[torch.Tensor] = None,
                 min_value=None, max_value=None, scale_f32: bool = False, hidden1: OutQuant, hidden2: OutQuant,
                 out_quant: Optional[OutQuant] = None, out: Optional[torch.Tensor] = None,
                 residual: Optional[OutQuant] = None) -> torch.Tensor:
    """MobileNetV2's inverted-residual block -- 1 x 1 expand -> depthwise 3 x 3 -> 1 x 1 project -- on
    stored codes in one launch, the two hidden tensors kept in LDS (dfq_int_mbconv_q).

    ``x_codes``: a contiguous NCHW tensor of codes -- uint8, or int8 when ``symmetric``, else
    TypeError -- on the grid the range keywords and ``bits`` name, as ``int_conv2d_q(x_codes=True)``
    takes it.  ``expand``, ``depthwise``, ``project``: each a ``(b_codes, b_scale, b_zero, bias)``
    tuple as the other entries take them, of shapes [Ch, Cin], [Ch, 9] and [Cout, Ch]; uint8 or int8
    bytes, scale / zero per tensor or per row, ``b_zero`` and ``bias`` may be None.  ``hidden1`` /
    ``hidden2`` (``OutQuant``): the grids of the expand's and the depthwise's outputs; on [0, 6] the
    clamp is the ReLU6.  ``stride`` 1 or 2, ``padding`` 0 or 1, both axes.  The result is bit for bit
    ``int_conv2d_q(x, *expand, 1, x_codes=True, out_quant=hidden1)`` -> ``int_dwconv2d_q(c1,
    *depthwise, 3, stride, padding, x_codes=True, out_quant=hidden2, <hidden1's grid>)`` ->
    ``int_conv2d_q(c2, *project, 1, x_codes=True, out_quant=out_quant, <hidden2's grid>)``: fp32
    [B, Cout, OH, OW], or under ``out_quant`` its code bytes; ``out``, if passed, is such a tensor.
    Cin <= ``MB_MAX_CIN``, Cout <= ``MB_MAX_COUT`` and Ch <= ``MAX_K``, else NotImplementedError.

    ``residual`` (an ``OutQuant``; dfq_int_mbconv_res_q): the block's ``x +
    project(...)`` in the same launch.  ``residual`` is the grid of the project's output, and the
    result is bit for bit ``int_add_q(int_mbconv_q(..., out_quant=residual), residual, x_codes,
    <x's grid>, out_quant=out_quant)``: the shortcut's codes come from the footprint the kernel
    already holds in LDS, the project's codes never reach memory.  Needs ``stride`` 1, ``padding`` 1
    and Cin == Cout, else ValueError.  With None the call is dfq_int_mbconv_q's.

    Counts 1 in ``LINEAR_CALLS``.  Asynchronous on the current stream; there is no CPU fallback."""
    global LINEAR_CALLS
    if residual is not None and not isinstance(residual, OutQuant):
        raise TypeError("residual: an intmm.OutQuant, the grid of the project's output")
    bits = _x_arg(x_codes, bits, symmetric, True)
    stride, padding = int(stride), int(padding)
    if stride < 1 or padding < 0:
        raise ValueError("stride must be >= 1 and padding >= 0")
    if x_codes.dim() != 4 or not x_codes.is_contiguous() or x_codes.numel() == 0:
        raise ValueError("x_codes must be a contiguous [B, C, H, W] tensor, got %s with strides %s" % (tuple(x_codes.shape), tuple(x_codes.stride())))
    B, Cin, H, W = x_codes.shape
    d = _lib.IntMbconvDesc()
    dev, tensors, rows = x_codes.device, [min_dev, max_dev], []
    d.x_quant.min_dev, d.x_quant.max_dev, d.x_quant.given_min, d.x_quant.given_max, d.x_quant.flags = _range_fields(min_dev, max_dev, min_value, max_value, scale_f32)
    d.x_quant.bits, d.x_quant.symmetric = bits, int(bool(symmetric))
    for name, layer, K in (("expand", expand, Cin), ("depthwise", depthwise, 9), ("project", project, None)):
        if not isinstance(layer, (tuple, list)) or len(layer) != 4:
            raise TypeError("%s: a (b_codes, b_scale, b_zero, bias) tuple" % name)
        b_codes, b_scale, b_zero, bias = layer
        N = _b_args(getattr(d, name), b_codes, b_scale, b_zero, _k_arg(K if K is not None else rows[0]), False)
        if name == "depthwise" and N != rows[0]:
            raise ValueError("depthwise holds %d rows of 9, the expand layer %d channels" % (N, rows[0]))
        _bias_dev_args("int_mbconv_q", N, dev, bias, (b_codes, b_scale, b_zero))
        getattr(d, name).bias = bias.data_ptr() if bias is not None else None
        rows.append(N)
    Ch, _, Cout = rows
    for name, oq in (("hidden1", hidden1), ("hidden2", hidden2)):
        if not isinstance(oq, OutQuant):
            raise TypeError(name + ": an intmm.OutQuant")
        _mb_quant(getattr(d, name), name, oq, tensors)
    if out_quant is not None:
        _mb_quant(d.out_quant, "out_quant", out_quant, tensors)
    res = None
    if residual is not None:
        res = _lib.IntMbconvRes()
        _mb_quant(res.proj_quant, "residual", residual, tensors)
    OH, OW = mx.conv_out_size(H, 3, stride, padding, 1), mx.conv_out_size(W, 3, stride, padding, 1)
    if OH < 1 or OW < 1:
        raise ValueError("the 3 x 3 kernel does not fit the padded input %s" % ((H + 2 * padding, W + 2 * padding),))
    out = _conv_out("int_mbconv_q", (B, Cout, OH, OW), out, out_quant, dev)
    _bias_dev_args("int_mbconv_q", Cout, dev, None, (*tensors, out))
    d.x, d.out = x_codes.data_ptr(), out.data_ptr()
    d.B, d.Cin, d.H, d.W, d.Ch, d.Cout, d.stride, d.pad = B, Cin, H, W, Ch, Cout, stride, padding
    if res is None:
        _lib.check(_lib.load().dfq_int_mbconv_q(C.byref(d), _lib.raw_stream(dev)), "dfq_int_mbconv_q", ValueError)
    else:
        _lib.check(_lib.load().dfq_int_mbconv_res_q(C.byref(d), C.byref(res), _lib.raw_stream(dev)), "dfq_int_mbconv_res_q", ValueError)
    LINEAR_CALLS += 1
    return out


def _add_operand(name: str, codes, quant, q, tensors: list) -> None:
    """An operand of ``int_add_q`` before its device is looked at: its grid's checks (``_mb_quant``) and, as ``_x_arg``, the dtype
    the grid's ``symmetric`` names."""
    if not isinstance(quant, OutQuant):
        raise TypeError(name + "_quant: an intmm.OutQuant")
    _mb_quant(q, name + "_quant", quant, tensors)
    if not isinstance(codes, torch.Tensor):
        raise TypeError("%s_codes: a uint8 or int8 tensor on the GPU" % name)
    if codes.dtype != _code_dtype(quant.symmetric):
        raise TypeError("%s_codes: stored codes are %s when symmetric=%s, got %s" % (name, _code_dtype(quant.symmetric), bool(quant.symmetric), codes.dtype))


def int_add_q(a_codes: torch.Tensor, a_quant: OutQuant, b_codes: torch.Tensor, b_quant: OutQuant, *,
              out_quant: Optional[OutQuant] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The sum of two tensors of stored codes in one launch (dfq_int_add_q): a
    residual add that stays on bytes.  ``a_codes`` / ``b_codes``: contiguous tensors of one shape
    on the GPU, uint8, or int8 when their grid (``a_quant`` / ``b_quant``, each an ``OutQuant``) is
    symmetric, else TypeError; any byte address is taken (a slice such as ``flat[1:]`` gives the
    same bits, more slowly).  With v the fp32 value ``fake_quant_given`` returns for a code on its
    grid, the result is ``va + vb`` in fp32 -- or, under ``out_quant``, ``fake_quant_given``'s code
    byte of that sum on ``out_quant``'s range; on a range with min = 0 the clamp is the ReLU of an
    ``add_relu``.  No operand is requantized onto a second grid.  ``out``, if passed, is a
    contiguous tensor of that shape and type.  Asynchronous on the current stream; there is no CPU
    fallback."""
    d = _lib.IntAddDesc()
    tensors: list = []
    _add_operand("a", a_codes, a_quant, d.a_quant, tensors)
    _add_operand("b", b_codes, b_quant, d.b_quant, tensors)
    if a_codes.shape != b_codes.shape:
        raise ValueError("a_codes %s and b_codes %s must have one shape" % (tuple(a_codes.shape), tuple(b_codes.shape)))
    for name, codes in (("a_codes", a_codes), ("b_codes", b_codes)):
        _on_gpu(name, codes, "a uint8 or int8 tensor")
        if not codes.is_contiguous() or codes.numel() == 0:
            raise ValueError("%s must be a non-empty contiguous tensor, got %s with strides %s" % (name, tuple(codes.shape), tuple(codes.stride())))
    if out_quant is not None:
        _mb_quant(d.out_quant, "out_quant", out_quant, tensors)
    dev, shape = a_codes.device, tuple(a_codes.shape)
    if out_quant is not None:
        out = _code_out("int_add_q", shape, out, out_quant, dev)
    elif out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float32:
        raise TypeError("out: float32 on the GPU")
    elif tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError("out must be a contiguous %s tensor" % (list(shape),))
    _bias_dev_args("int_add_q", 0, dev, None, (*tensors, b_codes, out))
    d.a, d.b, d.out, d.n = a_codes.data_ptr(), b_codes.data_ptr(), out.data_ptr(), a_codes.numel()
    _lib.check(_lib.load().dfq_int_add_q(C.byref(d), _lib.raw_stream(dev)), "dfq_int_add_q", ValueError)
    return out


def _pool_operand(what: str, d, x_codes, x_quant, out_quant, min_dims: int) -> list:
    """``x_codes`` of a pooling call and its two grids before any device is looked at: ``_add_operand``'s checks, then the
    tensor's; the grids' tensors."""
    tensors: list = []
    _add_operand("x", x_codes, x_quant, d.x_quant, tensors)
    if out_quant is not None:
        _mb_quant(d.out_quant, "out_quant", out_quant, tensors)
    _on_gpu("x_codes", x_codes, "a uint8 or int8 tensor")
    if x_codes.dim() < min_dims or not x_codes.is_contiguous() or x_codes.numel() == 0:
        raise ValueError("%s: x_codes must be a non-empty contiguous tensor of %d dimensions%s, got %s with strides %s"
                         % (what, min_dims, " or more" if min_dims == 3 else "", tuple(x_codes.shape), tuple(x_codes.stride())))
    return tensors


def int_mean_q(x_codes: torch.Tensor, x_quant: OutQuant, *, out_quant: Optional[OutQuant] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The mean over H * W of a tensor of stored codes in one launch (dfq_int_mean_q; DESIGN.md
    3.9.4): the classifiers' global average pool, staying on bytes.  ``x_codes``: a contiguous
    [B, C, H, W] or [B, C, P] tensor (any trailing dimensions) on the GPU, uint8, or int8 when its
    grid ``x_quant`` (an ``OutQuant``) is symmetric, else TypeError; any byte address is taken.
    With S the integer sum of a plane's codes and (s, z) ``fake_quant``'s scale and zero of the
    grid, the result [B, C] is ``float32((float64(s) * S) / P + float64(z))`` -- or, under
    ``out_quant``, ``fake_quant_given``'s code byte of that value.  The sum is an integer, so the
    bits do not depend on how the kernel splits the work.  P is at most 2^23, else
    NotImplementedError.  ``out``, if passed, is a contiguous [B, C] tensor of the result's type.
    Asynchronous on the current stream; there is no CPU fallback."""
    d = _lib.IntMeanDesc()
    tensors = _pool_operand("int_mean_q", d, x_codes, x_quant, out_quant, 3)
    dev, shape = x_codes.device, tuple(x_codes.shape[:2])
    if out_quant is not None:
        out = _code_out("int_mean_q", shape, out, out_quant, dev)
    elif out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float32:
        raise TypeError("out: float32 on the GPU")
    elif tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError("out must be a contiguous %s tensor" % (list(shape),))
    _bias_dev_args("int_mean_q", 0, dev, None, (*tensors, out))
    d.x, d.out, d.rows = x_codes.data_ptr(), out.data_ptr(), shape[0] * shape[1]
    d.plane = x_codes.numel() // d.rows
    _lib.check(_lib.load().dfq_int_mean_q(C.byref(d), _lib.raw_stream(dev)), "dfq_int_mean_q", ValueError)
    return out


def int_maxpool2d_q(x_codes: torch.Tensor, x_quant: OutQuant, kernel_size, stride=None, padding=0, *,
                    out_quant: Optional[OutQuant] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``F.max_pool2d`` (dilation 1, ceil mode off) on stored codes in one launch
    (dfq_int_maxpool2d_q).  ``x_codes``: a contiguous [B, C, H, W] tensor on the
    GPU, uint8, or int8 when its grid ``x_quant`` (an ``OutQuant``) is symmetric, else TypeError.
    The result [B, C, OH, OW] holds the largest code -- as the grid's integers -- among each
    window's taps inside the image: with a positive scale that is ``F.max_pool2d`` of the
    dequantized tensor, on the same grid, with no arithmetic at all.  A padding tap is absent, not
    a zero byte.  Under ``out_quant`` the maximum's fp32 value on ``x_quant`` is requantized to
    ``fake_quant_given``'s code byte on that grid.  ``kernel_size``, ``stride``, ``padding``: ints
    or (h, w) pairs; ``stride=None`` is the kernel size and ``padding`` is at most half the kernel,
    as in torch, else ValueError.  KH * KW is at most ``DW_MAX_TAPS``.  ``out``, if passed, is a
    contiguous byte tensor of the result's shape and type.  Asynchronous on the current stream;
    there is no CPU fallback."""
    (KH, KW), (ph, pw) = mx._pair(kernel_size, "kernel_size"), mx._pair(padding, "padding")
    sh, sw = (KH, KW) if stride is None else mx._pair(stride, "stride")
    if min(KH, KW, sh, sw) < 1 or min(ph, pw) < 0:
        raise ValueError("kernel_size and stride must be >= 1 and padding >= 0")
    if ph > KH // 2 or pw > KW // 2:
        raise ValueError("padding %s must be at most half the kernel %s" % ((ph, pw), (KH, KW)))
    if KH * KW > DW_MAX_TAPS:
        raise NotImplementedError("KH * KW must be <= %d, got %d" % (DW_MAX_TAPS, KH * KW))
    d = _lib.IntMaxpool2dDesc()
    tensors = _pool_operand("int_maxpool2d_q", d, x_codes, x_quant, out_quant, 4)
    if x_codes.dim() != 4:
        raise ValueError("int_maxpool2d_q: x_codes must be [B, C, H, W], got %s" % (tuple(x_codes.shape),))
    B, Cn, H, W = x_codes.shape
    OH, OW = mx.conv_out_size(H, KH, sh, ph, 1), mx.conv_out_size(W, KW, sw, pw, 1)
    if OH < 1 or OW < 1:
        raise ValueError("the kernel %s does not fit the padded input %s" % ((KH, KW), (H + 2 * ph, W + 2 * pw)))
    dev = x_codes.device
    out = _code_out("int_maxpool2d_q", (B, Cn, OH, OW), out, out_quant if out_quant is not None else x_quant, dev)
    _bias_dev_args("int_maxpool2d_q", 0, dev, None, (*tensors, out))
    d.x, d.out = x_codes.data_ptr(), out.data_ptr()
    d.B, d.C, d.H, d.W, d.KH, d.KW = B, Cn, H, W, KH, KW
    d.stride_h, d.stride_w, d.pad_h, d.pad_w = sh, sw, ph, pw
    _lib.check(_lib.load().dfq_int_maxpool2d_q(C.byref(d), _lib.raw_stream(dev)), "dfq_int_maxpool2d_q", ValueError)
    return out


def group_quant(w2d: torch.Tensor, bits: int, group: int, *, symmetric: bool = False, packed: bool = False):
    """Group-wise codes of a weight for ``int_gemm(b_group=group)``: (codes [N, K] -- or packed
    [N, K / 2] nibbles, int8 when symmetric -- scale [N, G], zero [N, G]), G = ceil(K / group).
    The sweep's per-channel mode on the [N * K / group, group] view of ``w2d`` [N, K]; a ragged
    K is the body ``w2d[:, :K - K % group]`` swept that way and the tail ``w2d[:, K - K % group:]``
    swept per row, joined column-wise.  No arithmetic of its own."""
    from . import sweep
    from .utils.quantize import fake_quant
    group = _group_arg(group)
    if group is None or w2d.dim() != 2 or w2d.numel() == 0:
        raise ValueError("group_quant takes a non-empty [N, K] weight and a group size")
    N, K = w2d.shape
    if packed and (bits > 4 or K % 2):
        raise ValueError("packed codes need bits <= 4 and an even K")

    def rows_of(part: torch.Tensor, row_len: int):
        view = part.contiguous().reshape(-1, row_len)
        if not packed:
            r = fake_quant(view, bits, per_channel=True, symmetric=symmetric)
            return r.codes.reshape(N, -1), r.scale.reshape(N, -1), r.zero.reshape(N, -1)
        it = sweep.allocate(view, bits=bits, per_channel=True, symmetric=symmetric, pack_int4=True)
        plan = sweep.SweepPlan([it])
        plan.execute()
        plan.destroy()
        codes = it.codes.view(torch.int8) if symmetric else it.codes
        return codes.reshape(N, -1), it.scale.reshape(N, -1), it.zero.reshape(N, -1)

    body = K - K % group
    parts = ([rows_of(w2d[:, :body], group)] if body else []) + ([rows_of(w2d[:, body:], K - body)] if K > body else [])
    codes, scale, zero = (torch.cat([p[i] for p in parts], dim=1).contiguous() for i in range(3))
    return codes, scale, zero
