"""dfq_mx_conv2d without a GPU: its index arithmetic walked on the CPU under sanitizers, the
entry point's argument checks, the descriptor's layout, the Python wrappers' checks and the CLI
flag."""
import ctypes as C
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from data_free_quantization_amd import _lib, mx
from tests import mx_conv_cases as CC

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "data_free_quantization_amd" / "libdfq_hip.so"
CXX = next((c for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"), shutil.which("c++"))
            if c and os.path.exists(c)), None)
#: the GPU tests' geometries, and two where OH * OW < 4 (a lane's four rows span several images)
EXTRA = {"one_pixel": CC._g(7, 4, 3, 3, 5, 3, 1, 0, 1), "three_pixels": CC._g(5, 2, 1, 5, 33, (1, 3), 1, 0, 1)}
GEOMS = {**CC.CASES, **EXTRA}


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_index_arithmetic_under_sanitizers(tmp_path):
    """dfq_mx_conv_plan.cpp + tests/native/mx_conv_plan_check.cpp, nothing else linked, under
    AddressSanitizer and UBSan.  For every geometry of the GPU tests and all four activation
    formats (pointwise geometries: both kernel variants), walked with the plan header's helpers
    alone: every read lies inside x, the gathered (m, k) element is the im2col definition's, and
    every output element is stored exactly once at its NCHW offset.  The counts the program
    reports are compared with F.unfold's."""
    (tmp_path / "shapes.txt").write_text("".join(" ".join(map(str, CC.flat(g))) + "\n" for g in GEOMS.values()))
    exe = tmp_path / "mx_conv_plan_check"
    csrc = ROOT / "data_free_quantization_amd" / "csrc"
    subprocess.run([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", str(ROOT / "include"), "-I", str(csrc),
                    str(ROOT / "tests" / "native" / "mx_conv_plan_check.cpp"), str(csrc / "dfq_mx_conv_plan.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe), str(tmp_path / "shapes.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert not r.stderr, r.stderr[-4000:]   # no sanitizer report
    seen = {}
    for line in r.stdout.splitlines():
        w = line.split()
        assert w[0] == "ok", line
        rest = {w[i]: int(w[i + 1]) for i in range(14, len(w), 2)}
        seen[(tuple(int(t) for t in w[1:14]), rest["fmt"], rest["pw"])] = rest
    fmts = [mx.FORMATS[f][0] for f in ("mxfp4", "mxfp6_e2m3", "mxfp6_e3m2", "mxfp8")]
    want = set()
    for g in GEOMS.values():
        pointwise = g.kernel == (1, 1) and g.padding == (0, 0) and g.dilation == (1, 1)
        want |= {(CC.flat(g), f, pw) for f in fmts for pw in ((0, 1) if pointwise else (0,))}
    assert set(seen) == want
    assert {g.kernel == (1, 1) for g in GEOMS.values()} == {True, False}
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
            # every wave in a row of tiles gathers that row's elements again, nothing else
            assert got["reads"] == inside * -(-g.N // 32)
            assert got["reads"] + got["zeros"] == waves * 2 * 64 * 32 * -(-k // 128)
    # the cases do what they are there for
    a, f = CC.CASES["a"], CC.CASES["f"]
    assert CC.K(a) == 45 and CC.M(a) == 98 and (CC.M(a) // 2) % 4 != 0       # a store group straddles m = 49
    cols = F.unfold(torch.ones(f.B, f.C, f.H, f.W), f.kernel, f.dilation, f.padding, f.stride)[0].t()   # [M, K]
    assert (cols.sum(1) == 0).any()                                           # whole im2col rows in padding
    assert (cols[:, :64].reshape(-1, 2, 32).sum(-1) == 0).any()               # and whole blocks


# ---- the entry point's argument checks ----------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        pytest.skip("libdfq_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def _good():
    d = _lib.MxConv2dDesc()
    d.x, d.b_codes, d.b_scales, d.bias, d.out = 0x1004, 0x3000, 0x4003, 0x5004, 0x6004
    d.B, d.C, d.H, d.W, d.N, d.KH, d.KW = 2, 5, 7, 7, 9, 3, 3
    d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w = 1, 2, 1, 0, 1, 2
    d.x_format, d.b_format = _lib.DFQ_MX_FP8_E4M3, _lib.DFQ_MX_FP4_E2M1
    return d


def test_argument_validation_without_a_device(lib):
    """Every refusal comes back before any device call: this runs on a machine without a GPU."""
    L = lib
    assert L.dfq_mx_conv2d(None, None) == _lib.DFQ_ERR_INVALID
    extents = ("B", "C", "H", "W", "N", "KH", "KW", "stride_h", "stride_w", "dil_h", "dil_w")
    invalid = [("x", None), ("b_codes", None), ("b_scales", None), ("out", None),
               ("x_format", 2), ("x_format", -1), ("b_format", 5), ("b_format", 0x33),
               ("flags", 1), ("flags", -1), ("reserved", 1),
               *[(n, v) for n in extents for v in (0, -3, (1 << 28) + 1)],
               ("pad_h", -1), ("pad_w", -2), ("pad_h", (1 << 28) + 1), ("pad_w", (1 << 28) + 1),
               ("x", 0x1002), ("x", 0x1001), ("b_codes", 0x3008), ("b_codes", 0x3004),
               ("out", 0x6002), ("out", 0x6001), ("bias", 0x5002)]
    for name, value in invalid:
        d = _good()
        setattr(d, name, value)
        assert L.dfq_mx_conv2d(C.byref(d), None) == _lib.DFQ_ERR_INVALID, (name, value)

    def sized(**kw):
        d = _good()
        d.KH = d.KW = d.stride_w = d.dil_w = 1
        d.pad_h = 0
        for k, v in kw.items():
            setattr(d, k, v)
        return L.dfq_mx_conv2d(C.byref(d), None)

    # the limits: C * H * W, K and N * OH * OW below 2^31, M at most 2^31, N * K at most 2^50
    assert sized(C=1 << 11, H=1 << 10, W=1 << 10) == _lib.DFQ_ERR_INVALID
    assert sized(C=1 << 11, H=1, W=1, KH=1 << 10, KW=1 << 10, pad_h=1 << 10, pad_w=1 << 10) == _lib.DFQ_ERR_INVALID
    assert sized(C=1, N=1 << 11, H=1 << 10, W=1 << 10) == _lib.DFQ_ERR_INVALID
    assert sized(B=(1 << 21) + 1, C=1, N=1, H=1 << 5, W=1 << 5) == _lib.DFQ_ERR_INVALID
    assert sized(B=1, C=1 << 25, N=(1 << 25) + 1, H=1, W=1) == _lib.DFQ_ERR_INVALID
    # FP6 weight codes need 8 bytes, not 16; 4 is refused
    for fmt in (_lib.DFQ_MX_FP6_E2M3, _lib.DFQ_MX_FP6_E3M2):
        d = _good()
        d.b_format, d.b_codes = fmt, 0x3004
        assert L.dfq_mx_conv2d(C.byref(d), None) == _lib.DFQ_ERR_INVALID
    # the dilated kernel does not fit the padded image
    for kw in ({"H": 2, "pad_h": 0}, {"W": 4}, {"dil_h": 5}, {"KW": 5}):
        d = _good()
        for k, v in kw.items():
            setattr(d, k, v)
        assert L.dfq_mx_conv2d(C.byref(d), None) == _lib.DFQ_ERR_SHAPE, kw
    # inside every limit, but 2^22 x 2^22 blocks
    assert sized(B=1 << 28, C=1, N=1 << 28, H=8, W=1, stride_h=1) == _lib.DFQ_ERR_INVALID   # N * OH * OW
    assert sized(B=1 << 28, C=1, N=1 << 28, H=1, W=1) == _lib.DFQ_ERR_UNSUPPORTED


def test_desc_matches_the_header():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "dfq_hip.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct dfq_mx_conv2d_desc\s*\{(.*?)\}\s*dfq_mx_conv2d_desc;", text, flags=re.S).group(1)
    assert re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*;", body) == [f for f, _ in _lib.MxConv2dDesc._fields_]
    assert C.sizeof(_lib.MxConv2dDesc) == 5 * 8 + 13 * 8 + 4 * 4
    assert _lib.MxConv2dDesc.B.offset == 40 and _lib.MxConv2dDesc.x_format.offset == 144
    assert "dfq_mx_conv2d" in _lib.EXPORTS and "#define DFQ_ABI_VERSION 1" in text
    assert "dfq_mx_conv_plan.cpp" in (ROOT / "data_free_quantization_amd" / "build.py").read_text()


def test_python_rejects_cpu_tensors_and_bad_arguments():
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)   # noqa: E731
    x = torch.randn(2, 4, 5, 5)
    with pytest.raises(RuntimeError, match="ROCm GPU only.*no CPU fallback"):
        mx.mx_conv2d_fused(x, u8(3, 2, 32), u8(3, 2), "mxfp8", 3, padding=1)
    with pytest.raises(ValueError):
        mx.mx_conv2d_fused(x, u8(3, 2, 32), u8(3, 2), "mxfp8", 3, act_format="mxfp6")
    with pytest.raises(ValueError):
        mx.mx_conv2d_fused(x, u8(3, 2, 32), u8(3, 2), "mxfp6", 3)
    with pytest.raises(TypeError):
        mx.mx_conv2d_fused(None, u8(3, 2, 32), u8(3, 2), "mxfp8", 3)
    assert mx.conv_out_size(224, 7, 2, 3, 1) == 112 and mx.conv_out_size(4, 3, 1, 0, 2) == 0
    assert mx.LINEAR_CALLS == 0


def test_the_forward_scope_takes_the_conv_switch():
    from data_free_quantization_amd.utils import quantize as Q
    assert Q._MX_MATMUL is None and Q._MX_CONV is False
    with pytest.raises(ValueError):
        with Q.mx_matmul_forward("mxfp6", conv=True):
            pass
    assert Q._MX_MATMUL is None and Q._MX_CONV is False
    with Q.mx_matmul_forward("mxfp4", conv=True):
        assert (Q._MX_MATMUL, Q._MX_FUSED, Q._MX_CONV) == ("mxfp4", False, True)
        with Q.mx_matmul_forward("mxfp8", fused=True):
            assert (Q._MX_MATMUL, Q._MX_FUSED, Q._MX_CONV) == ("mxfp8", True, False)
        assert (Q._MX_MATMUL, Q._MX_FUSED, Q._MX_CONV) == ("mxfp4", False, True)
    assert Q._MX_MATMUL is None and Q._MX_CONV is False


def test_which_layers_route():
    """groups == 1, padding_mode "zeros" and a tuple or int padding route under conv=True; nothing
    routes beyond the 1x1 rule without it."""
    from data_free_quantization_amd.utils import quantize as Q

    def layer(*a, **k):
        m = Q.QuantConv2d(*a, **k)
        m.weight_format = "mxfp4"
        return m

    k3, dw, same, circ, pw = (layer(8, 8, 3, padding=1), layer(8, 8, 3, padding=1, groups=8), layer(8, 8, 3, padding="same"),
                              layer(8, 8, 3, padding=1), layer(8, 8, 1, stride=2))
    circ.padding_mode = "circular"   # QuantConv2d's constructor takes no padding_mode; a converted layer may carry one
    with Q.mx_matmul_forward("mxfp8", conv=True):
        assert [m._mx_format() for m in (k3, dw, same, circ, pw)] == ["mxfp4", None, None, None, "mxfp4"]
        assert [m._mx_conv_routed() for m in (k3, dw, same, circ)] == [True, False, False, False]
    with Q.mx_matmul_forward("mxfp8"):
        assert [m._mx_format() for m in (k3, dw, same, circ, pw)] == [None, None, None, None, "mxfp4"]
        assert not pw._mx_conv_routed()


def test_cli_flag():
    from data_free_quantization_amd import main_dfq
    base = ["--quantize", "--weight_format", "mxfp4"]
    a = main_dfq.get_argument(base + ["--mx_matmul", "mxfp8", "--mx_matmul_conv"])
    assert a.mx_matmul == "mxfp8" and a.mx_matmul_conv is True and a.mx_matmul_fused is False
    assert main_dfq.get_argument(base + ["--mx_matmul", "mxfp8"]).mx_matmul_conv is False
    assert main_dfq.get_argument(["--quantize"]).mx_matmul_conv is False
    for argv in (base + ["--mx_matmul_conv"], ["--quantize", "--mx_matmul_conv"], ["--mx_matmul_conv"]):
        with pytest.raises(SystemExit):
            main_dfq.get_argument(argv)
    assert "--mx_matmul_conv" in main_dfq.__doc__
