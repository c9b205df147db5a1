"""dfq_int_conv2d without a GPU: its index arithmetic, mask and folds walked on the CPU under
sanitizers, the entry point's argument checks, the descriptor's layout, the Python wrapper's
checks, the forward scope's switch, which layers route, and the CLI flag."""
import ctypes as C
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from data_free_quantization_amd import _lib, intmm
from tests import int_conv_cases as KC
from tests import mx_conv_cases as CC

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "data_free_quantization_amd" / "libdfq_hip.so"
CXX = next((c for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"), shutil.which("c++"))
            if c and os.path.exists(c)), None)
GEOMS = KC.GEOMS


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_index_arithmetic_under_sanitizers(tmp_path):
    """The plan .cpp files + tests/native/int_conv_plan_check.cpp, nothing else linked, under
    AddressSanitizer and UBSan.  For every geometry of the GPU tests, every kernel variant that may
    run it (the mask operand on and, where unpadded, off; the pointwise variant where pointwise)
    and both signs of either operand, walked with the plan headers' helpers alone: every read lies
    inside x, the gathered element and its mask bit are the im2col definition's, T is the mask's
    row sum, the folds give P, Sa and Sb back from signed-domain sums of random codes, and every
    output element is stored exactly once at its NCHW offset.  The counts the program reports are
    compared with F.unfold's."""
    (tmp_path / "shapes.txt").write_text("".join(" ".join(map(str, CC.flat(g))) + "\n" for g in GEOMS.values()))
    exe = tmp_path / "int_conv_plan_check"
    csrc = ROOT / "data_free_quantization_amd" / "csrc"
    subprocess.run([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", str(ROOT / "include"), "-I", str(csrc),
                    str(ROOT / "tests" / "native" / "int_conv_plan_check.cpp"), str(csrc / "dfq_int_conv_plan.cpp"),
                    str(csrc / "dfq_mx_conv_plan.cpp"), "-o", str(exe)], check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe), str(tmp_path / "shapes.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert not r.stderr, r.stderr[-4000:]   # no sanitizer report
    seen = {}
    for line in r.stdout.splitlines():
        w = line.split()
        assert w[0] == "ok", line
        rest = {w[i]: int(w[i + 1]) for i in range(14, len(w), 2)}
        seen[(tuple(int(t) for t in w[1:14]), rest["pw"], rest["mask"], rest["xs"], rest["bs"])] = rest
    want = set()
    for g in GEOMS.values():
        pointwise = g.kernel == (1, 1) and g.padding == (0, 0) and g.dilation == (1, 1)
        variants = [(0, 1)] + ([(0, 0)] if g.padding == (0, 0) else []) + ([(1, 0)] if pointwise else [])
        want |= {(CC.flat(g), pw, mask, xs, bs) for pw, mask in variants for xs in (0, 1) for bs in (0, 1)}
    assert set(seen) == want
    assert {len([k for k in seen if k[0] == CC.flat(g)]) for g in GEOMS.values()} == {4, 8, 12}   # padded, unpadded, pointwise
    for g in GEOMS.values():
        m, k = CC.M(g), CC.K(g)
        oh, ow = CC.out_size(g)
        inside = int(F.unfold(torch.ones(g.B, g.C, g.H, g.W), g.kernel, g.dilation, g.padding, g.stride).sum().item())
        waves = -(-m // 32) * -(-g.N // 32)
        quads = sum(1 for m4 in range(0, m, 4) if m4 + 3 < m and m4 % (oh * ow) + 3 < oh * ow)
        for key, got in seen.items():
            if key[0] != CC.flat(g):
                continue
            assert (got["M"], got["K"]) == (m, k)
            assert got["grid"] == -(-m // 64) * -(-g.N // 64)
            assert got["stores"] == m * g.N
            assert got["quads"] == quads * g.N
            assert got["taps"] == inside
            # every wave in a row of tiles gathers that row's elements again, nothing else
            assert got["reads"] == inside * -(-g.N // 32)
            assert got["reads"] + got["zeros"] == waves * 2 * 64 * 16 * -(-k // 64)
    # the cases do what they are there for
    f = GEOMS["f"]
    assert (KC.taps(f).sum(1) == 0).any()                                    # whole im2col rows in padding
    assert all(CC.out_size(GEOMS[n])[0] * CC.out_size(GEOMS[n])[1] < 4 for n in ("one_pixel", "three_pixels"))
    assert GEOMS["nopad"].kernel == (3, 3) and GEOMS["nopad"].padding == (0, 0)


# ---- the entry point's argument checks ----------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        pytest.skip("libdfq_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def _good():
    d = _lib.IntConv2dDesc()
    d.x, d.min_dev, d.max_dev, d.b_codes, d.b_scale, d.b_zero = 0x1004, 0x2004, 0x2008, 0x3000, 0x4004, 0x4008
    d.bias, d.out = 0x5004, 0x6004
    d.B, d.C, d.H, d.W, d.N, d.KH, d.KW = 2, 6, 7, 7, 9, 3, 3
    d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w = 1, 2, 1, 0, 1, 2
    d.x_bits, d.x_symmetric, d.b_signed, d.flags = 8, 0, 1, _lib.DFQ_INT_B_PACK4 | _lib.DFQ_SCALE_F32
    return d


def test_argument_validation_without_a_device(lib):
    """Every refusal the header lists comes back before any device call: this runs on a machine
    without a GPU."""
    L = lib
    assert L.dfq_int_conv2d(None, None) == _lib.DFQ_ERR_INVALID
    extents = ("B", "C", "H", "W", "N", "KH", "KW", "stride_h", "stride_w", "dil_h", "dil_w")
    invalid = [("x", None), ("b_codes", None), ("b_scale", None), ("out", None),
               ("flags", 8), ("flags", -1), ("flags", 0x10), ("reserved", 1), ("reserved2", 1),
               ("b_signed", 2), ("b_signed", -1), ("x_symmetric", 2), ("x_symmetric", -1),
               ("x_bits", 1), ("x_bits", 9), ("x_bits", 16), ("x_bits", 0),
               *[(n, v) for n in extents for v in (0, -3, (1 << 28) + 1)],
               ("pad_h", -1), ("pad_w", -2), ("pad_h", (1 << 28) + 1), ("pad_w", (1 << 28) + 1),
               ("x", 0x1002), ("x", 0x1001), ("out", 0x6002), ("out", 0x6001), ("bias", 0x5002),
               ("min_dev", 0x2001), ("max_dev", 0x2002), ("b_scale", 0x4002), ("b_zero", 0x4009),
               ("b_codes", 0x3008), ("b_codes", 0x3001)]
    for name, value in invalid:
        d = _good()
        setattr(d, name, value)
        assert L.dfq_int_conv2d(C.byref(d), None) == _lib.DFQ_ERR_INVALID, (name, value)

    def sized(**kw):
        d = _good()
        d.KH = d.KW = d.stride_w = d.dil_w = 1
        d.pad_h = 0
        d.flags = 0
        for k, v in kw.items():
            setattr(d, k, v)
        return L.dfq_int_conv2d(C.byref(d), None)

    # the limits: C * H * W, K and N * OH * OW below 2^31, M at most 2^31, N * K at most 2^50
    assert sized(C=1 << 11, H=1 << 10, W=1 << 10) == _lib.DFQ_ERR_INVALID
    assert sized(C=1 << 11, H=1, W=1, KH=1 << 10, KW=1 << 10, pad_h=1 << 10, pad_w=1 << 10) == _lib.DFQ_ERR_INVALID
    assert sized(C=1, N=1 << 11, H=1 << 10, W=1 << 10) == _lib.DFQ_ERR_INVALID
    assert sized(B=(1 << 21) + 1, C=1, N=1, H=1 << 5, W=1 << 5) == _lib.DFQ_ERR_INVALID
    assert sized(B=1, C=1 << 25, N=(1 << 25) + 1, H=1, W=1) == _lib.DFQ_ERR_INVALID
    # the dilated kernel does not fit the padded image
    for kw in ({"H": 2, "pad_h": 0}, {"W": 4}, {"dil_h": 5}, {"KW": 5}):
        d = _good()
        for k, v in kw.items():
            setattr(d, k, v)
        assert L.dfq_int_conv2d(C.byref(d), None) == _lib.DFQ_ERR_SHAPE, kw
    # K beyond DFQ_INT_MAX_K, packed B with an odd K, a grid beyond int32
    assert sized(C=_lib.DFQ_INT_MAX_K + 1) == _lib.DFQ_ERR_UNSUPPORTED
    assert sized(C=_lib.DFQ_INT_MAX_K // 9 + 1, KH=3, KW=3, H=3, W=3) == _lib.DFQ_ERR_UNSUPPORTED
    assert sized(C=5, flags=_lib.DFQ_INT_B_PACK4) == _lib.DFQ_ERR_UNSUPPORTED
    d = _good()
    d.C = 5   # K = 45 with the packed flag of _good()
    assert L.dfq_int_conv2d(C.byref(d), None) == _lib.DFQ_ERR_UNSUPPORTED
    assert sized(B=1 << 28, C=1, N=1 << 28, H=8, W=1, stride_h=1) == _lib.DFQ_ERR_INVALID   # N * OH * OW
    assert sized(B=1 << 28, C=1, N=1 << 28, H=1, W=1) == _lib.DFQ_ERR_UNSUPPORTED            # 2^22 x 2^22 blocks


def test_the_mx_convolution_refuses_what_it_refused(lib):
    """The geometry checks are shared with dfq_mx_conv2d; its answers did not move."""
    def mx(**kw):
        d = _lib.MxConv2dDesc()
        d.x, d.b_codes, d.b_scales, d.bias, d.out = 0x1004, 0x3000, 0x4003, 0x5004, 0x6004
        d.B, d.C, d.H, d.W, d.N, d.KH, d.KW = 2, 5, 7, 7, 9, 3, 3
        d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w = 1, 2, 1, 0, 1, 2
        d.x_format, d.b_format = _lib.DFQ_MX_FP8_E4M3, _lib.DFQ_MX_FP4_E2M1
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.dfq_mx_conv2d(C.byref(d), None)

    assert mx(H=2, pad_h=0) == _lib.DFQ_ERR_SHAPE
    assert mx(H=2, pad_h=0, x=0x1002) == _lib.DFQ_ERR_INVALID      # alignment is looked at before the output extent
    assert mx(H=0, x=0x1002) == _lib.DFQ_ERR_INVALID
    assert mx(pad_w=-1) == _lib.DFQ_ERR_INVALID
    assert mx(B=1 << 28, C=1, N=1 << 28, H=1, W=1, KH=1, KW=1, stride_w=1, dil_w=1, pad_h=0) == _lib.DFQ_ERR_UNSUPPORTED


def test_desc_matches_the_header():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "dfq_hip.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct dfq_int_conv2d_desc\s*\{(.*?)\}\s*dfq_int_conv2d_desc;", text, flags=re.S).group(1)
    assert re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*;", body) == [f for f, _ in _lib.IntConv2dDesc._fields_]
    assert C.sizeof(_lib.IntConv2dDesc) == 8 * 8 + 2 * 8 + 13 * 8 + 6 * 4
    assert _lib.IntConv2dDesc.B.offset == 80 and _lib.IntConv2dDesc.x_bits.offset == 184
    assert "dfq_int_conv2d" in _lib.EXPORTS and "#define DFQ_ABI_VERSION 1" in text
    assert re.search(r"int dfq_int_conv2d\(const dfq_int_conv2d_desc\* d, void\* stream\);", text)
    assert "dfq_int_conv_plan.cpp" in (ROOT / "data_free_quantization_amd" / "build.py").read_text()
    assert "dfq_int_conv2d" in (ROOT / "INTEGRATION.md").read_text()


def test_python_rejects_cpu_tensors_and_bad_arguments():
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)   # noqa: E731
    f32 = lambda *s: torch.ones(*s)   # noqa: E731
    x = torch.randn(2, 4, 5, 5)
    rng = dict(min_value=-1.0, max_value=1.0)
    intmm.reset_linear_calls()
    with pytest.raises(RuntimeError, match="ROCm GPU only.*no CPU fallback"):
        intmm.int_conv2d(x, u8(3, 36), f32(1), None, 3, padding=1, **rng)
    with pytest.raises(TypeError):
        intmm.int_conv2d(None, u8(3, 36), f32(1), None, 3, **rng)
    for bits in (1, 9, 16):
        with pytest.raises(ValueError):
            intmm.int_conv2d(x, u8(3, 36), f32(1), None, 3, bits=bits, **rng)
    assert intmm.LINEAR_CALLS == 0
    import inspect
    sig = inspect.signature(intmm.int_conv2d)
    assert list(sig.parameters) == ["x", "b_codes", "b_scale", "b_zero", "kernel_size", "stride", "padding", "dilation", "bits",
                                    "symmetric", "min_dev", "max_dev", "min_value", "max_value", "scale_f32", "b_packed", "bias", "out"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[8:])


def test_the_forward_scope_takes_the_conv_switch():
    from data_free_quantization_amd.utils import quantize as Q
    assert Q._INT_MATMUL is False and Q._INT_CONV is False
    intmm.LINEAR_CALLS = 7
    with Q.int_matmul_forward(conv=True):
        assert intmm.LINEAR_CALLS == 0
        assert (Q._INT_MATMUL, Q._INT_CONV) == (True, True)
        with Q.int_matmul_forward():
            assert (Q._INT_MATMUL, Q._INT_CONV) == (True, False)
            with Q.int_matmul_forward(conv=True):
                assert (Q._INT_MATMUL, Q._INT_CONV) == (True, True)
            assert (Q._INT_MATMUL, Q._INT_CONV) == (True, False)
        assert (Q._INT_MATMUL, Q._INT_CONV) == (True, True)
    assert Q._INT_MATMUL is False and Q._INT_CONV is False
    with pytest.raises(KeyError):
        with Q.int_matmul_forward(conv=True):
            raise KeyError("restored on the way out of an exception too")
    assert Q._INT_MATMUL is False and Q._INT_CONV is False


def test_which_layers_route():
    """groups == 1, padding_mode "zeros", a tuple or int padding, grids of at most 8 bits and
    K <= MAX_K route under conv=True; nothing routes beyond the 1x1 rule without it."""
    from data_free_quantization_amd.utils import quantize as Q
    layer = Q.QuantConv2d
    k3, dw, same, circ, pw, wide, big = (layer(8, 8, 3, padding=1), layer(8, 8, 3, padding=1, groups=8), layer(8, 8, 3, padding="same"),
                                         layer(8, 8, 3, padding=1), layer(8, 8, 1, stride=2), layer(8, 8, 3, padding=1, num_bits=16),
                                         layer(intmm.MAX_K // 9 + 1, 1, 3))
    act16 = layer(8, 8, 3, padding=1, num_bits_act=16)
    mxl = layer(8, 8, 3, padding=1)
    mxl.weight_format = "mxfp4"
    circ.padding_mode = "circular"   # QuantConv2d's constructor takes no padding_mode; a converted layer may carry one
    every = (k3, dw, same, circ, pw, wide, act16, big, mxl)
    assert not any(m._int_routed() for m in every)
    with Q.int_matmul_forward(conv=True):
        assert [m._int_routed() for m in every] == [True, False, False, False, True, False, False, False, False]
        assert [m._int_conv_routed() for m in (k3, dw, same, circ, pw, big)] == [True, False, False, False, True, False]
    with Q.int_matmul_forward():
        assert [m._int_routed() for m in every] == [False, False, False, False, True, False, False, False, False]
        assert not pw._int_conv_routed() and not k3._int_conv_routed()
    q = Q.QConv2d(8, 8, 3, padding=1)
    with Q.int_matmul_forward(conv=True):
        assert q._int_routed() and q._int_conv_routed()


def test_cli_flag():
    from data_free_quantization_amd import main_dfq
    a = main_dfq.get_argument(["--quantize", "--int_matmul", "--int_matmul_conv"])
    assert a.int_matmul is True and a.int_matmul_conv is True
    assert main_dfq.get_argument(["--quantize", "--int_matmul"]).int_matmul_conv is False
    assert main_dfq.get_argument(["--quantize"]).int_matmul_conv is False
    for argv in (["--quantize", "--int_matmul_conv"], ["--int_matmul_conv"],
                 ["--quantize", "--weight_format", "mxfp4", "--mx_matmul", "mxfp8", "--int_matmul_conv"],
                 ["--quantize", "--weight_format", "mxfp4", "--int_matmul", "--int_matmul_conv"]):
        with pytest.raises(SystemExit):
            main_dfq.get_argument(argv)
    assert "--int_matmul_conv" in main_dfq.__doc__
