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
numpy float64 statement (tests/int_gemm_cases.py).  There is no CPU fallback: CPU tensors
raise."""
from __future__ import annotations

import ctypes as C
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


def _b_args(d, b_codes, b_scale, b_zero, K: int, b_packed: bool) -> int:
    """B's checks and descriptor fields (shared by the two descriptors); N."""
    N = _codes_arg("b_codes", b_codes, K, b_packed)
    _param_arg("b_scale", b_scale, (1, N) if N > 1 else (1,))
    _param_arg("b_zero", b_zero, (b_scale.numel(),), optional=True)
    d.b_codes, d.b_scale = b_codes.data_ptr(), b_scale.data_ptr()
    d.b_zero = b_zero.data_ptr() if b_zero is not None else None
    d.b_signed = int(b_codes.dtype == torch.int8)
    # N == 1: one value either way
    d.flags |= (_lib.DFQ_INT_B_PACK4 if b_packed else 0) | (_lib.DFQ_INT_B_PER_ROW if b_scale.numel() > 1 else 0)
    return N


def _range_args(d, min_dev, max_dev, min_value, max_value, scale_f32: bool) -> None:
    """The quantizer's range: its checks and descriptor fields (int_linear's and int_conv2d's)."""
    for name, dev_v, host_v in (("min", min_dev, min_value), ("max", max_dev, max_value)):
        if dev_v is not None:
            _param_arg(name + "_dev", dev_v, (1,))
        elif host_v is None:
            raise ValueError("the range's %s is missing: pass %s_dev or %s_value" % (name, name, name))
    d.min_dev = min_dev.data_ptr() if min_dev is not None else None
    d.max_dev = max_dev.data_ptr() if max_dev is not None else None
    d.given_min = float(min_value) if min_value is not None else 0.0
    d.given_max = float(max_value) if max_value is not None else 0.0
    d.flags = _lib.DFQ_SCALE_F32 if scale_f32 else 0


def _bias_out_args(what: str, d, M: int, N: int, K: int, dev, bias, out, others) -> torch.Tensor:
    """mx.py's checks of ``bias``, ``out`` and the tensors' device; the descriptor fields both entries share."""
    out = mx._bias_out_args(what, M, N, dev, bias, out, others)
    d.bias = bias.data_ptr() if bias is not None else None
    d.out, d.ldo = out.data_ptr(), (out.stride(0) if M > 1 else max(out.stride(0), N))
    d.M, d.N, d.K = M, N, K
    return out


def int_gemm(a_codes: torch.Tensor, a_scale: torch.Tensor, a_zero: Optional[torch.Tensor], b_codes: torch.Tensor,
             b_scale: torch.Tensor, b_zero: Optional[torch.Tensor], K: int, *, b_packed: bool = False,
             bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[m, n] = sum_k (qa[m, k] * sa + za) * (qb[n, k] * sb[n] + zb[n]) (+ bias[n]) on the
    i8 matrix instruction (dfq_int_gemm).  ``a_codes``: M * K bytes, ``b_codes``:
    N * K bytes -- or N * K / 2 packed bytes with ``b_packed`` (the sweep's ``pack_int4`` layout,
    K even) -- contiguous, rows of K elements; uint8 codes are unsigned and int8 codes signed
    (packed nibbles are two's complement when the tensor is int8: view the sweep's packed
    symmetric codes as int8).  ``a_scale`` / ``a_zero``: one fp32 value each; ``b_scale`` /
    ``b_zero``: one value each, or N (per output channel); a zero may be None (0).  ``out``:
    fp32 [M, N] whose rows may be strided; allocated when None.  The result is the contract's
    fp64 statement bit for bit.  One launch, asynchronous on the current stream."""
    K = _k_arg(K)
    M = _codes_arg("a_codes", a_codes, K)
    _param_arg("a_scale", a_scale, (1,))
    _param_arg("a_zero", a_zero, (1,), optional=True)
    d = _lib.IntGemmDesc()
    N = _b_args(d, b_codes, b_scale, b_zero, K, bool(b_packed))
    dev = a_codes.device
    out = _bias_out_args("int_gemm", d, M, N, K, dev, bias, out, (a_scale, a_zero, b_codes, b_scale, b_zero))
    d.a_codes, d.a_scale = a_codes.data_ptr(), a_scale.data_ptr()
    d.a_zero = a_zero.data_ptr() if a_zero is not None else None
    d.a_signed = int(a_codes.dtype == torch.int8)
    _lib.check(_lib.load().dfq_int_gemm(C.byref(d), _lib.raw_stream(dev)), "dfq_int_gemm", ValueError)
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
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``int_gemm`` with A given as fp32 ``x`` [M, K] and quantized to ``bits`` (2..8) inside the
    kernel (dfq_int_linear): the quantizer is ``fake_quant_given``'s -- the range from the
    device scalars ``min_dev`` / ``max_dev`` (no host synchronisation) or the Python floats
    ``min_value`` / ``max_value``, ``scale_f32`` as there -- and the codes of x never reach
    memory.  Bit for bit ``fake_quant`` of x on that range (codes, scale, zero) followed by
    ``int_gemm``.  ``x`` needs unit column stride; any row stride >= K is passed on (a column
    slice of a wider tensor is read in place).  B, ``bias`` and ``out`` as for ``int_gemm``."""
    global LINEAR_CALLS
    K = _k_arg(K)
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
    N = _b_args(d, b_codes, b_scale, b_zero, K, bool(b_packed))
    M, dev = x.shape[0], x.device
    out = _bias_out_args("int_linear", d, M, N, K, dev, bias, out, (min_dev, max_dev, b_codes, b_scale, b_zero))
    d.x, d.ldx = x.data_ptr(), (x.stride(0) if M > 1 else max(x.stride(0), K))
    d.x_bits, d.x_symmetric = bits, int(bool(symmetric))
    _lib.check(_lib.load().dfq_int_linear(C.byref(d), _lib.raw_stream(dev)), "dfq_int_linear", ValueError)
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
    global LINEAR_CALLS
    bits = int(bits)
    if not 2 <= bits <= 8:
        raise ValueError("bits must be 2..8, got %d" % bits)
    _on_gpu("x", x, "a float32 tensor")
    if x.dtype != torch.float32:
        raise TypeError("x: float32 on the GPU")
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
    N = _b_args(d, b_codes, b_scale, b_zero, K, bool(b_packed))
    OH, OW = mx.conv_out_size(H, KH, sh, ph, dh), mx.conv_out_size(W, KW, sw, pw, dw)
    if OH < 1 or OW < 1:
        raise ValueError("the kernel %s (dilation %s) does not fit the padded input %s" % ((KH, KW), (dh, dw), (H + 2 * ph, W + 2 * pw)))
    dev = x.device
    if bias is not None:
        _lib.require_device(bias)
        if bias.numel() != N:
            raise ValueError("bias holds %d elements, %d needed" % (bias.numel(), N))
    if out is None:
        out = torch.empty((B, N, OH, OW), dtype=torch.float32, device=dev)
    else:
        if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float32:
            raise TypeError("out: float32 on the GPU")
        if tuple(out.shape) != (B, N, OH, OW) or not out.is_contiguous():
            raise ValueError("out must be a contiguous [%d, %d, %d, %d] tensor" % (B, N, OH, OW))
    for t in (min_dev, max_dev, b_codes, b_scale, b_zero, bias, out):
        if t is not None and t.device != dev:
            raise ValueError("every tensor of an int_conv2d call must live on one device")
    d.x, d.out = x.data_ptr(), out.data_ptr()
    d.bias = bias.data_ptr() if bias is not None else None
    d.B, d.C, d.H, d.W, d.N, d.KH, d.KW = B, Cin, H, W, N, KH, KW
    d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w = sh, sw, ph, pw, dh, dw
    d.x_bits, d.x_symmetric = bits, int(bool(symmetric))
    _lib.check(_lib.load().dfq_int_conv2d(C.byref(d), _lib.raw_stream(dev)), "dfq_int_conv2d", ValueError)
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
    global LINEAR_CALLS
    bits = int(bits)
    if not 2 <= bits <= 8:
        raise ValueError("bits must be 2..8, got %d" % bits)
    _on_gpu("x", x, "a float32 tensor")
    if x.dtype != torch.float32:
        raise TypeError("x: float32 on the GPU")
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
    if bias is not None:
        _lib.require_device(bias)
        if bias.numel() != N:
            raise ValueError("bias holds %d elements, %d needed" % (bias.numel(), N))
    if out is None:
        out = torch.empty((B, N, OH, OW), dtype=torch.float32, device=dev)
    else:
        if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float32:
            raise TypeError("out: float32 on the GPU")
        if tuple(out.shape) != (B, N, OH, OW) or not out.is_contiguous():
            raise ValueError("out must be a contiguous [%d, %d, %d, %d] tensor" % (B, N, OH, OW))
    for t in (min_dev, max_dev, b_codes, b_scale, b_zero, bias, out):
        if t is not None and t.device != dev:
            raise ValueError("every tensor of an int_dwconv2d call must live on one device")
    d.x, d.out = x.data_ptr(), out.data_ptr()
    d.bias = bias.data_ptr() if bias is not None else None
    d.B, d.C, d.H, d.W, d.mult, d.KH, d.KW = B, Cin, H, W, N // Cin, KH, KW
    d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w = sh, sw, ph, pw, dh, dw
    d.x_bits, d.x_symmetric = bits, int(bool(symmetric))
    _lib.check(_lib.load().dfq_int_dwconv2d(C.byref(d), _lib.raw_stream(dev)), "dfq_int_dwconv2d", ValueError)
    LINEAR_CALLS += 1
    return out
