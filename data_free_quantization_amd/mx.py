"""OCP Microscaling (MX) block-scaled weight quantization: MXFP4, MXFP6 and MXFP8.

Host wrapper of ``dfq_mx_quantize_batch`` (include/dfq_hip.h): FP4
(E2M1), FP6 (E2M3 or E3M2) or FP8 (E4M3) elements with one shared power-of-two E8M0
scale per 32 consecutive elements of a row, the operand format of CDNA4's scaled
matrix instructions.  ``mx_quantize`` takes every tensor of a list in one C call (one
launch, one HBM pass, asynchronous on the stream); ``mx_dequantize`` rebuilds the
fp32 values from codes and scales in plain torch, exactly, on CPU or GPU.
``mx_gemm`` multiplies two operands given as codes and scales on the scaled matrix
instruction (``dfq_mx_gemm``), ``mx_linear`` quantizes an fp32 input and
weight and multiplies them, and ``mx_linear_fused`` multiplies an fp32 input with stored
weight codes in one launch, quantizing the input inside the kernel (``dfq_mx_linear``).
There is no CPU fallback for the quantizer or the
multiply: CPU tensors raise."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib

BLOCK = _lib.DFQ_MX_BLOCK
#: weight_format name -> (library format, element bits, code bytes per block)
FORMATS = {"mxfp4": (_lib.DFQ_MX_FP4_E2M1, 4, 16), "mxfp8": (_lib.DFQ_MX_FP8_E4M3, 8, 32),
           "mxfp6_e2m3": (_lib.DFQ_MX_FP6_E2M3, 6, 24), "mxfp6_e3m2": (_lib.DFQ_MX_FP6_E3M2, 6, 24)}
_NAMES = "'mxfp4', 'mxfp6_e2m3', 'mxfp6_e3m2' or 'mxfp8'"   # there is no bare 'mxfp6': the two differ
#: the exponent of each element format's largest binade (the floor rule: X = floor(log2 amax) - emax)
EMAX = {"mxfp4": 2, "mxfp8": 8, "mxfp6_e2m3": 2, "mxfp6_e3m2": 4}


def is_mx(weight_format: str) -> bool:
    """True for an MX format name, False for "int"; anything else raises."""
    if weight_format == "int":
        return False
    if weight_format not in FORMATS:
        raise ValueError("weight_format must be 'int', %s, got %r" % (_NAMES, weight_format))
    return True


def bits_per_weight(fmt: str) -> float:
    """Element bits plus the block's share of its 8-bit scale: 4.25, 6.25 or 8.25."""
    return FORMATS[fmt][1] + 8.0 / BLOCK


def blocks(row_len: int) -> int:
    return -(-row_len // BLOCK)


_Out = Optional[Union[torch.Tensor, int]]


@dataclass
class MXItem:
    """One fp32 tensor viewed as [rows, -1] (rows = shape[0] unless given) and what
    to write for it.  The outputs may also be raw device addresses (int) into
    memory the caller keeps alive until the call has run.  ``codes``: uint8
    [rows, nb, 16] (mxfp4, element 2k in the low nibble), [rows, nb, 32] (mxfp8) or
    [rows, nb, 24] (mxfp6_*: 32 six-bit codes packed densely, element i in bits [6i, 6i+6));
    ``scales``: uint8 [rows, nb]; ``esum``: fp32 [numel / khw]; nb = ceil(row_len / 32)."""
    src: torch.Tensor
    fmt: str = "mxfp4"
    dst: _Out = None        # dequantized output (may be src)
    codes: _Out = None
    scales: _Out = None
    esum: _Out = None
    khw: int = 1
    rows: Optional[int] = None


def allocate(src: torch.Tensor, fmt: str = "mxfp4", khw: int = 1, in_place: bool = False, want_dst: bool = True,
             want_codes: bool = True, want_esum: bool = False) -> MXItem:
    """An MXItem with freshly allocated outputs on src's device."""
    rows = src.shape[0] if src.dim() > 0 else 1
    nb = blocks(src.numel() // rows)
    dev = src.device
    return MXItem(
        src=src, fmt=fmt, khw=khw, rows=rows,
        dst=(src if in_place else torch.empty_like(src)) if want_dst else None,
        codes=torch.empty((rows, nb, FORMATS[fmt][2]), dtype=torch.uint8, device=dev) if want_codes else None,
        scales=torch.empty((rows, nb), dtype=torch.uint8, device=dev) if want_codes else None,
        esum=torch.empty(src.numel() // khw, dtype=torch.float32, device=dev) if want_esum else None)


def floor_scale_bytes(w: torch.Tensor, fmt: str, rows: Optional[int] = None) -> torch.Tensor:
    """The scale bytes the floor rule gives fp32 ``w`` viewed as [rows, -1] (rows = shape[0]
    unless given): uint8 [rows, nb], X + 127 with X = floor(log2 amax) - emax clamped at -127,
    0 for an all-zero block.  Pure torch, CPU or GPU: what ``scale_raised`` (the quality
    report's count of blocks the scale search moved) compares the stored bytes with."""
    if fmt not in FORMATS:
        raise ValueError("fmt must be %s, got %r" % (_NAMES, fmt))
    rows = rows if rows is not None else (w.shape[0] if w.dim() > 0 else 1)
    x = w.detach().reshape(rows, -1).abs()
    nb = blocks(x.shape[1])
    x = torch.nn.functional.pad(x, (0, nb * BLOCK - x.shape[1]))
    amax = x.reshape(rows, nb, BLOCK).amax(dim=-1).contiguous()
    e = (amax.view(torch.int32) >> 23) & 0xFF   # the fp32 exponent field is floor(log2 amax) + 127
    return torch.where(amax == 0, torch.zeros_like(e), (e - EMAX[fmt]).clamp(min=0)).to(torch.uint8)


_MX = np.dtype([("src", "<u8"), ("dst", "<u8"), ("codes", "<u8"), ("scales", "<u8"), ("esum", "<u8"),
                ("rows", "<i8"), ("row_len", "<i8"), ("khw", "<i4"), ("format", "<i4"), ("flags", "<i4"),
                ("reserved", "<i4")])
assert _MX.itemsize == C.sizeof(_lib.MxDesc)
assert all(_MX.fields[f][1] == getattr(_lib.MxDesc, f).offset for f, _ in _lib.MxDesc._fields_)


def mx_quantize(items: Sequence[MXItem], stream: Optional[torch.cuda.Stream] = None,
                scale_search: bool = False) -> List[MXItem]:
    """Quantize every item in one C call, asynchronous on ``stream`` (the current
    one by default).  Returns the items.  ``scale_search``: every block takes the
    better of the floor rule's exponent and the next one up by its own quantization
    noise (``dfq_mx_quantize_search_batch``) -- same outputs, same layouts."""
    items = list(items)
    if not items:
        return items
    tab, keep = [], []
    for it in items:
        _lib.require_device(it.src, *(t for t in (it.dst, it.esum) if not isinstance(t, int)))
        if it.src.device != items[0].src.device:
            raise ValueError("every tensor of an mx_quantize call must live on one device")
        if it.fmt not in FORMATS:
            raise ValueError("fmt must be %s, got %r" % (_NAMES, it.fmt))
        if it.src.numel() == 0:
            raise ValueError("empty tensors have nothing to quantize")
        for name in ("codes", "scales"):
            t = getattr(it, name)
            if t is not None and not isinstance(t, int) and not (t.is_cuda and t.dtype == torch.uint8 and
                                                                 t.is_contiguous()):
                raise TypeError(name + ": contiguous uint8 on the GPU")
        rows = it.rows if it.rows is not None else (it.src.shape[0] if it.src.dim() > 0 else 1)
        row_len = it.src.numel() // rows
        if rows * row_len != it.src.numel():
            raise ValueError("rows does not divide the tensor")
        nb = blocks(row_len)
        for name, need in (("codes", rows * nb * FORMATS[it.fmt][2]), ("scales", rows * nb),
                           ("esum", it.src.numel() // max(it.khw, 1)), ("dst", it.src.numel())):
            t = getattr(it, name)
            if t is not None and not isinstance(t, int) and t.numel() < need:
                raise ValueError("%s holds %d elements, %d needed" % (name, t.numel(), need))
        ptr = lambda t: t if isinstance(t, int) else (t.data_ptr() if t is not None else 0)   # noqa: E731
        tab.append((it.src.data_ptr(), ptr(it.dst), ptr(it.codes), ptr(it.scales), ptr(it.esum), rows, row_len,
                    int(it.khw), FORMATS[it.fmt][0], 0, 0))
        keep += [t for t in (it.dst, it.codes, it.scales, it.esum) if isinstance(t, torch.Tensor)]
    dev = items[0].src.device
    arr = np.array(tab, dtype=_MX)
    descs = arr.ctypes.data_as(C.POINTER(_lib.MxDesc))
    L = _lib.load()
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):   # the workspace is stream-ordered (caching allocator) with the launch
        # a too-small workspace (0 for a bad list) makes the call itself report the list's error
        ws = torch.empty(max(int(L.dfq_mx_quantize_ws_bytes(descs, len(items))), 256), dtype=torch.uint8, device=dev)
    if any(it.dst is not None for it in items):
        _lib.weights_changed()
    name = "dfq_mx_quantize_search_batch" if scale_search else "dfq_mx_quantize_batch"
    _lib.check(getattr(L, name)(descs, len(items), ws.data_ptr(), ws.numel(), C.c_void_p(s.cuda_stream)), name, ValueError)
    if stream is not None and s != torch.cuda.current_stream(dev):
        for t in keep:
            t.record_stream(s)
    return items


def _codes_arg(name: str, codes, scales, fmt: str, K: int):
    """The checks of one mx_gemm operand; its row count."""
    if fmt not in FORMATS:
        raise ValueError("%s_fmt must be %s, got %r" % (name, _NAMES, fmt))
    for what, t in ((name + "_codes", codes), (name + "_scales", scales)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(what + ": a uint8 tensor on the GPU")
        if not t.is_cuda:
            raise RuntimeError("data_free_quantization_amd multiplies MX codes on a ROCm GPU only; "
                               "%s is on %s (there is no CPU fallback)" % (what, t.device))
        if t.dtype != torch.uint8 or not t.is_contiguous():
            raise TypeError(what + ": contiguous uint8 on the GPU")
    nb, cb = blocks(K), FORMATS[fmt][2]
    if scales.dim() != 2 or scales.shape[1] != nb or scales.shape[0] < 1:
        raise ValueError("%s_scales must be [rows, %d] for K = %d, got %s" % (name, nb, K, tuple(scales.shape)))
    rows = scales.shape[0]
    if codes.numel() != rows * nb * cb:
        raise ValueError("%s_codes holds %d bytes, [%d, %d, %d] needed" % (name, codes.numel(), rows, nb, cb))
    if codes.data_ptr() % (8 if cb == 24 else 16):
        raise ValueError("%s_codes must be %d-byte aligned" % (name, 8 if cb == 24 else 16))
    return rows


def _k_arg(K) -> int:
    K = int(K)
    if K < 1:
        raise ValueError("K must be >= 1")
    return K


def _bias_out_args(what: str, M: int, N: int, dev, bias, out, others):
    """The checks of ``bias`` and ``out`` of an mx_gemm / mx_linear_fused call (``what``) and of
    every tensor's device (``others``: the operands besides the one ``dev`` is taken from);
    ``out``, allocated when None."""
    if bias is not None:
        _lib.require_device(bias)
        if bias.numel() != N:
            raise ValueError("bias holds %d elements, %d needed" % (bias.numel(), N))
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=dev)
    else:
        if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float32:
            raise TypeError("out: float32 on the GPU")
        if out.dim() != 2 or tuple(out.shape) != (M, N) or out.stride(1) != 1 or (M > 1 and out.stride(0) < N):
            raise ValueError("out must be [%d, %d] with unit column stride and a row stride >= %d" % (M, N, N))
    for t in (*others, bias, out):
        if t is not None and t.device != dev:
            raise ValueError("every tensor of an %s call must live on one device" % what)
    return out


def _multiply(entry: str, d, M: int, N: int, K: int, b_fmt: str, bias, out, stream, dev, tensors) -> torch.Tensor:
    """What the two descriptors share filled in, the C call ``entry`` on ``stream`` (the
    device's current one when None), and ``tensors`` kept alive for a stream of the caller's."""
    d.bias = bias.data_ptr() if bias is not None else None
    d.out, d.ldo = out.data_ptr(), (out.stride(0) if M > 1 else max(out.stride(0), N))
    d.M, d.N, d.K, d.b_format = M, N, K, FORMATS[b_fmt][0]
    s = C.c_void_p(stream.cuda_stream) if stream is not None else _lib.raw_stream(dev)
    _lib.check(getattr(_lib.load(), entry)(C.byref(d), s), entry, ValueError)
    if stream is not None and stream != torch.cuda.current_stream(dev):
        for t in (*tensors, bias, out):
            if t is not None:
                t.record_stream(stream)
    return out


def mx_gemm(a_codes: torch.Tensor, a_scales: torch.Tensor, a_fmt: str, b_codes: torch.Tensor, b_scales: torch.Tensor,
            b_fmt: str, K: int, bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
            stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """out[m, n] = sum_k A[m, k] * B[n, k] (+ bias[n]) on the scaled matrix instruction
    (dfq_mx_gemm): A and B as the ``codes`` ([rows, nb, 16 | 24 | 32]
    uint8) and ``scales`` ([rows, nb] uint8) ``mx_quantize`` writes for rows of K elements,
    in any two formats.  ``out``: fp32 [M, N] whose rows may be strided (a column slice of
    a wider tensor); allocated when None.  One launch, asynchronous on ``stream``."""
    K = _k_arg(K)
    M = _codes_arg("a", a_codes, a_scales, a_fmt, K)
    N = _codes_arg("b", b_codes, b_scales, b_fmt, K)
    dev = a_codes.device
    out = _bias_out_args("mx_gemm", M, N, dev, bias, out, (a_scales, b_codes, b_scales))
    d = _lib.MxGemmDesc()
    d.a_codes, d.a_scales, d.b_codes, d.b_scales = (t.data_ptr() for t in (a_codes, a_scales, b_codes, b_scales))
    d.a_format = FORMATS[a_fmt][0]
    return _multiply("dfq_mx_gemm", d, M, N, K, b_fmt, bias, out, stream, dev, (a_codes, a_scales, b_codes, b_scales))


def mx_linear_fused(x: torch.Tensor, b_codes: torch.Tensor, b_scales: torch.Tensor, b_fmt: str, K: int,
                    act_format: str = "mxfp8", bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                    stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """out[m, n] = sum_k Q(x)[m, k] * B[n, k] (+ bias[n]) in one launch (dfq_mx_linear; DESIGN.md
    3.8): ``x`` fp32 [M, K] rounded to ``act_format`` inside the kernel -- blocks of 32 along K,
    the floor rule, no scale search -- times B given as ``mx_gemm``'s B.  Bit for bit
    ``mx_quantize`` of x followed by ``mx_gemm``; the input's codes never reach memory.
    ``x`` needs unit column stride; any row stride >= K is passed on (a column slice of a wider
    tensor is read in place, no copy).  ``out`` as for ``mx_gemm``."""
    K = _k_arg(K)
    if act_format not in FORMATS:
        raise ValueError("act_format must be %s, got %r" % (_NAMES, act_format))
    if b_fmt not in FORMATS:
        raise ValueError("b_fmt must be %s, got %r" % (_NAMES, b_fmt))
    if not isinstance(x, torch.Tensor):
        raise TypeError("x: a float32 tensor on the GPU")
    if not x.is_cuda:
        raise RuntimeError("data_free_quantization_amd multiplies MX codes on a ROCm GPU only; "
                           "x is on %s (there is no CPU fallback)" % (x.device,))
    if x.dtype != torch.float32:
        raise TypeError("x: float32 on the GPU")
    N = _codes_arg("b", b_codes, b_scales, b_fmt, K)
    if x.dim() != 2 or x.shape[1] != K or x.shape[0] < 1 or x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < K):
        raise ValueError("x must be [M, %d] with unit column stride and a row stride >= %d, got %s with strides %s"
                         % (K, K, tuple(x.shape), tuple(x.stride())))
    M = x.shape[0]
    dev = x.device
    out = _bias_out_args("mx_linear_fused", M, N, dev, bias, out, (b_codes, b_scales))
    d = _lib.MxLinearDesc()
    d.x, d.b_codes, d.b_scales = x.data_ptr(), b_codes.data_ptr(), b_scales.data_ptr()
    d.ldx = x.stride(0) if M > 1 else max(x.stride(0), K)
    d.x_format = FORMATS[act_format][0]
    return _multiply("dfq_mx_linear", d, M, N, K, b_fmt, bias, out, stream, dev, (x, b_codes, b_scales))


def _pair(v, name: str):
    """An int or a pair of ints as (h, w)."""
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError("%s: an int or a pair of ints, got %r" % (name, v))
        return int(v[0]), int(v[1])
    return int(v), int(v)


def conv_out_size(size: int, k: int, stride: int, padding: int, dilation: int) -> int:
    """Output extent of a convolution along one axis (< 1: the kernel does not fit)."""
    span = size + 2 * padding - dilation * (k - 1) - 1
    return span // stride + 1 if span >= 0 else 0


def mx_conv2d_fused(x: torch.Tensor, b_codes: torch.Tensor, b_scales: torch.Tensor, b_fmt: str, kernel_size, stride=1,
                    padding=0, dilation=1, act_format: str = "mxfp8", bias: Optional[torch.Tensor] = None,
                    out: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """conv2d(Q(x), B) (+ bias) in one launch (dfq_mx_conv2d), groups == 1 and zero
    padding: ``x`` fp32 contiguous NCHW [B, C, H, W], read in place; B the weight [N, C, KH, KW] as
    the ``codes`` / ``scales`` ``mx_quantize`` writes for it -- rows of K = C * KH * KW elements,
    blocks of 32 along (c, kh, kw).  The kernel gathers each im2col row, rounds it to ``act_format``
    in blocks of 32 along the same (c, kh, kw) order (padding taps are +0 elements; the floor rule,
    no scale search) and stores NCHW: bit for bit ``mx_linear_fused`` of the materialised
    ``F.unfold`` matrix, without the matrix.  ``kernel_size``, ``stride``, ``padding``,
    ``dilation``: ints or (h, w) pairs.  ``out``: fp32 contiguous [B, N, OH, OW]; allocated when
    None.  Asynchronous on ``stream``."""
    if act_format not in FORMATS:
        raise ValueError("act_format must be %s, got %r" % (_NAMES, act_format))
    if b_fmt not in FORMATS:
        raise ValueError("b_fmt must be %s, got %r" % (_NAMES, b_fmt))
    if not isinstance(x, torch.Tensor):
        raise TypeError("x: a float32 tensor on the GPU")
    if not x.is_cuda:
        raise RuntimeError("data_free_quantization_amd multiplies MX codes on a ROCm GPU only; "
                           "x is on %s (there is no CPU fallback)" % (x.device,))
    if x.dtype != torch.float32:
        raise TypeError("x: float32 on the GPU")
    (KH, KW), (sh, sw) = _pair(kernel_size, "kernel_size"), _pair(stride, "stride")
    (ph, pw), (dh, dw) = _pair(padding, "padding"), _pair(dilation, "dilation")
    if min(KH, KW, sh, sw, dh, dw) < 1 or min(ph, pw) < 0:
        raise ValueError("kernel_size, stride and dilation must be >= 1 and padding >= 0")
    if x.dim() != 4 or not x.is_contiguous() or x.numel() == 0:
        raise ValueError("x must be a contiguous [B, C, H, W] tensor, got %s with strides %s" % (tuple(x.shape), tuple(x.stride())))
    B, Cin, H, W = x.shape
    K = Cin * KH * KW
    N = _codes_arg("b", b_codes, b_scales, b_fmt, K)
    OH, OW = conv_out_size(H, KH, sh, ph, dh), conv_out_size(W, KW, sw, pw, dw)
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
    for t in (b_codes, b_scales, bias, out):
        if t is not None and t.device != dev:
            raise ValueError("every tensor of an mx_conv2d_fused call must live on one device")
    d = _lib.MxConv2dDesc()
    d.x, d.b_codes, d.b_scales, d.out = x.data_ptr(), b_codes.data_ptr(), b_scales.data_ptr(), out.data_ptr()
    d.bias = bias.data_ptr() if bias is not None else None
    d.B, d.C, d.H, d.W, d.N, d.KH, d.KW = B, Cin, H, W, N, KH, KW
    d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w = sh, sw, ph, pw, dh, dw
    d.x_format, d.b_format = FORMATS[act_format][0], FORMATS[b_fmt][0]
    s = C.c_void_p(stream.cuda_stream) if stream is not None else _lib.raw_stream(dev)
    _lib.check(_lib.load().dfq_mx_conv2d(C.byref(d), s), "dfq_mx_conv2d", ValueError)
    if stream is not None and stream != torch.cuda.current_stream(dev):
        for t in (x, b_codes, b_scales, bias, out):
            if t is not None:
                t.record_stream(stream)
    return out


#: mx_linear calls since the last reset (utils.quantize.mx_matmul_forward resets it on entry)
LINEAR_CALLS = 0


def reset_linear_calls() -> None:
    global LINEAR_CALLS
    LINEAR_CALLS = 0


def mx_linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], weight_format: str,
              act_format: str = "mxfp8", weight_mx=None, weight_scale_search: bool = False, fused: bool = False) -> torch.Tensor:
    """x @ weight.T (+ bias) on the scaled matrix instruction: x (fp32 [M, K], contiguous)
    rounded to ``act_format`` and weight (fp32 [N, K]) to ``weight_format`` by
    ``mx_quantize`` -- blocks of 32 along K for both, codes and scales only -- then one
    ``mx_gemm``.  A weight that already lies on its MX grid (quantize_targ_layer's) re-quantizes
    to its own codes, so the product is of exactly the stored values.
    ``weight_scale_search``: quantize the weight with ``mx_quantize(scale_search=True)`` -- what a
    weight that lies on a searched grid needs to come back as its stored values (the floor rule
    saturates a searched MXFP8 block's 1.875 * 2^k).  The input keeps the floor rule.
    ``weight_mx``: the weight's (codes, scales) from an earlier call, instead of
    quantizing it again.  ``fused``: the input is quantized inside the multiply's kernel
    (``mx_linear_fused``: one launch once the weight's codes exist, the same bits); the weight,
    when ``weight_mx`` is None, still goes through ``mx_quantize``.  Returns fp32 [M, N]."""
    global LINEAR_CALLS
    for fmt in (weight_format, act_format):
        if fmt not in FORMATS:
            raise ValueError("format must be %s, got %r" % (_NAMES, fmt))
    _lib.require_device(x, weight, bias)
    if x.dim() != 2 or weight.dim() != 2 or x.shape[1] != weight.shape[1] or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("x must be [M, K] and weight [N, K], got %s and %s" % (tuple(x.shape), tuple(weight.shape)))
    # the weight's codes: given, or one mx_quantize call -- shared with the input's where both take
    # the floor rule through the same entry point (not fused, no search)
    xi = None if fused else allocate(x.detach(), act_format, want_dst=False)
    if weight_mx is None:
        wi = allocate(weight.detach(), weight_format, want_dst=False)
        if fused or weight_scale_search:
            if xi is not None:
                mx_quantize([xi])
            mx_quantize([wi], scale_search=weight_scale_search)
        else:
            mx_quantize([xi, wi])
        weight_mx = (wi.codes, wi.scales)
    elif xi is not None:
        mx_quantize([xi])
    LINEAR_CALLS += 1
    if fused:
        return mx_linear_fused(x.detach(), weight_mx[0], weight_mx[1], weight_format, x.shape[1], act_format, bias=bias)
    return mx_gemm(xi.codes, xi.scales, act_format, weight_mx[0], weight_mx[1], weight_format, x.shape[1], bias=bias)


def _tables(fmt: str, device) -> torch.Tensor:
    """Value of every code (sign included), fp32."""
    if fmt == "mxfp4":
        mag = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float32)
    elif fmt == "mxfp6_e2m3":   # s ee mmm, bias 1: m / 8, (8 + m) * 2^(e - 4)
        c = torch.arange(32, dtype=torch.int32)
        e, m = c >> 3, (c & 7).to(torch.float32)
        mag = torch.where(e == 0, m * 2.0 ** -3, (8.0 + m) * torch.pow(2.0, (e - 4).to(torch.float32)))
    elif fmt == "mxfp6_e3m2":   # s eee mm, bias 3: m / 16, (4 + m) * 2^(e - 5)
        c = torch.arange(32, dtype=torch.int32)
        e, m = c >> 2, (c & 3).to(torch.float32)
        mag = torch.where(e == 0, m * 2.0 ** -4, (4.0 + m) * torch.pow(2.0, (e - 5).to(torch.float32)))
    else:
        c = torch.arange(128, dtype=torch.int32)
        e, m = c >> 3, (c & 7).to(torch.float32)
        mag = torch.where(e == 0, m * 2.0 ** -9, (8.0 + m) * torch.pow(2.0, (e - 10).to(torch.float32)))
        mag[127] = float("nan")   # the E4M3 NaN code: never produced
    return torch.cat([mag, -mag]).to(device)


def pack6(c: torch.Tensor) -> torch.Tensor:
    """[..., 4k] six-bit codes -> [..., 3k] bytes: four codes w = c0 | c1 << 6 | c2 << 12 |
    c3 << 18 are the bytes w & 0xFF, (w >> 8) & 0xFF, w >> 16 (the FP6 ``codes`` layout)."""
    q = c.to(torch.int64).reshape(*c.shape[:-1], -1, 4)
    w = q[..., 0] | (q[..., 1] << 6) | (q[..., 2] << 12) | (q[..., 3] << 18)
    return torch.stack([w & 0xFF, (w >> 8) & 0xFF, w >> 16], dim=-1).reshape(*c.shape[:-1], -1).to(torch.uint8)


def unpack6(b: torch.Tensor) -> torch.Tensor:
    """The inverse of ``pack6``: [..., 3k] bytes -> [..., 4k] six-bit codes (int64)."""
    t = b.to(torch.int64).reshape(*b.shape[:-1], -1, 3)
    w = t[..., 0] | (t[..., 1] << 8) | (t[..., 2] << 16)
    return torch.stack([w & 0x3F, (w >> 6) & 0x3F, (w >> 12) & 0x3F, w >> 18], dim=-1).reshape(*b.shape[:-1], -1)


def mx_dequantize(codes: torch.Tensor, scales: torch.Tensor, shape, fmt: str) -> torch.Tensor:
    """The fp32 tensor of ``shape`` that ``codes`` ([rows, nb, 16 | 24 | 32] uint8) and
    ``scales`` ([rows, nb] uint8) stand for: y = +-q * 2^(scale - 127), every step
    exact in fp32 -- bit for bit the ``dst`` of ``mx_quantize``.  Pure torch, CPU or GPU."""
    if fmt not in FORMATS:
        raise ValueError("fmt must be %s, got %r" % (_NAMES, fmt))
    n = 1
    for s in shape:
        n *= int(s)
    rows, nb = scales.shape
    c = codes.reshape(rows, nb, FORMATS[fmt][2]).to(torch.int64)
    if fmt == "mxfp4":
        c = torch.stack([c & 0xF, c >> 4], dim=-1)   # element 2k low, 2k + 1 high
    elif FORMATS[fmt][1] == 6:
        c = unpack6(c)
    q = _tables(fmt, codes.device)[c.reshape(rows, nb, BLOCK)]
    # 2^(scale - 127) from its bit pattern (byte 0, only written for an all-zero block, reads as 0)
    up = (scales.to(torch.int32) << 23).view(torch.float32)
    y = (q * up.unsqueeze(-1)).reshape(rows, nb * BLOCK)
    return y[:, :n // rows].reshape(tuple(shape))
