"""dfq_int_dwconv2d without a GPU: its index arithmetic, masks and folds walked on the CPU under
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
from tests import int_dwconv_cases as DC

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "data_free_quantization_amd" / "libdfq_hip.so"
CSRC = ROOT / "data_free_quantization_amd" / "csrc"
CXX = next((c for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"), shutil.which("c++"))
            if c and os.path.exists(c)), None)
GEOMS = DC.GEOMS


def _plan_constants():
    text = (CSRC / "dfq_int_dwconv_plan.h").read_text()
    head = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "dfq_hip.h").read_text(), flags=re.S)
    defs = {k: int(v) for k, v in re.findall(r"#define (DFQ_INT_DW_[A-Z_]+)\s+(\d+)", head)}
    out = {}
    for name in ("kDwTileH", "kDwTileW", "kDwMaxTaps", "kDwCodeBytes", "kDwWeightWords", "kDwMaxPlanes", "kDwTargetQuads"):
        expr = re.search(name + r" = ([^;,]+)[;,]", text).group(1).strip()
        out[name] = defs[expr] if expr in defs else eval(expr, {})   # a DFQ_INT_DW_* name or a product of literals
    return out


def _plan(g, k):
    """The tile decomposition dwc_check makes, for geometries whose footprint fits at the first try."""
    oh, ow = DC.out_size(g)
    th, tw = -(-oh // -(-oh // k["kDwTileH"])), -(-ow // -(-ow // k["kDwTileW"]))   # split evenly over the fewest tiles
    tw = tw if tw == ow else -(-tw // 4) * 4
    fh = (th - 1) * g.stride[0] + (g.kernel[0] - 1) * g.dilation[0] + 1
    fw = (tw - 1) * g.stride[1] + (g.kernel[1] - 1) * g.dilation[1] + 1
    fwp = -(-fw // 4) * 4
    assert fh * fwp <= k["kDwCodeBytes"]
    tiles = -(-oh // th) * -(-ow // tw)
    planes = g.B * g.C
    pp = 1
    if tiles == 1:
        pp = max(1, min(k["kDwTargetQuads"] // (th * -(-tw // 4)), k["kDwMaxPlanes"], k["kDwCodeBytes"] // (fh * fwp), planes))
    return dict(th=th, tw=tw, pp=pp, grid=-(-planes // pp) * tiles, cells=-(-planes // pp) * tiles * pp * fh * fwp // 4,
                mc=min(g.mult, k["kDwWeightWords"] // (pp * -(-DC.K(g) // 4))), tiles=tiles)


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_index_arithmetic_under_sanitizers(tmp_path):
    """The plan .cpp file + tests/native/int_dwconv_plan_check.cpp, nothing else linked, under
    AddressSanitizer and UBSan.  For every geometry of the GPU tests, both signs of either operand
    and, where K is even, packed B too, walked with the plan header's helpers alone: every global
    read lies inside x, every LDS byte read was written and written once, the element and mask bit
    at each (output, tap) are the im2col definition's, T is the mask's sum, the folds give P, Sa
    and Sb back from signed-domain sums of random codes, every output is stored exactly once at its
    NCHW offset, and no LDS extent exceeds what the kernel declares.  The counts the program
    reports are compared with F.unfold's."""
    (tmp_path / "shapes.txt").write_text("".join(" ".join(map(str, DC.flat(g))) + "\n" for g in GEOMS.values()))
    exe = tmp_path / "int_dwconv_plan_check"
    subprocess.run([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", str(ROOT / "include"), "-I", str(CSRC),
                    str(ROOT / "tests" / "native" / "int_dwconv_plan_check.cpp"), str(CSRC / "dfq_int_dwconv_plan.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe), str(tmp_path / "shapes.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert not r.stderr, r.stderr[-4000:]   # no sanitizer report
    seen = {}
    for line in r.stdout.splitlines():
        w = line.split()
        assert w[0] == "ok", line
        rest = {w[i]: int(w[i + 1]) for i in range(14, len(w), 2)}
        seen[(tuple(int(t) for t in w[1:14]), rest["xs"], rest["bs"], rest["packed"])] = rest
    want = {(DC.flat(g), xs, bs, packed) for g in GEOMS.values() for xs in (0, 1) for bs in (0, 1)
            for packed in ((0, 1) if DC.K(g) % 2 == 0 else (0,))}
    assert set(seen) == want
    k = _plan_constants()
    assert k["kDwMaxTaps"] == _lib.DFQ_INT_DW_MAX_TAPS >= 49
    for name, g in GEOMS.items():
        oh, ow = DC.out_size(g)
        ones = torch.ones(g.B, g.C, g.H, g.W)
        cols = F.unfold(ones, g.kernel, g.dilation, g.padding, g.stride)
        inside = int(cols.sum().item())
        used = int((F.fold(cols, (g.H, g.W), g.kernel, g.dilation, g.padding, g.stride) > 0).sum().item())
        plan = _plan(g, k)
        for key, got in seen.items():
            if key[0] != DC.flat(g):
                continue
            assert (got["K"], got["OH"], got["OW"]) == (DC.K(g), oh, ow)
            assert {n: got[n] for n in ("th", "tw", "pp", "mc", "grid", "cells")} == {n: plan[n] for n in ("th", "tw", "pp", "mc", "grid", "cells")}, name
            assert got["stores"] == g.B * DC.N(g) * oh * ow
            assert got["taps"] == inside                       # every tap inside the image, once per (b, c, oh, ow)
            assert used <= got["distinct"] <= ones.numel()     # every element some tap reads is loaded
            assert got["reads"] >= got["distinct"]
            if plan["tiles"] == 1:
                assert got["reads"] == got["distinct"]         # a plane of one tile is read once
            full_quads = sum(1 for c0 in range(0, ow, 4) if c0 + 3 < ow and c0 % plan["tw"] + 3 < plan["tw"])
            assert got["quads"] == full_quads * oh * g.B * DC.N(g)
    # the cases do what they are there for
    wide, kw = GEOMS["wide"], _plan(GEOMS["wide"], k)
    oh, ow = DC.out_size(wide)
    assert oh > k["kDwTileH"] and oh % k["kDwTileH"] and ow > k["kDwTileW"] and ow % k["kDwTileW"]   # several tiles, the last partial
    assert (kw["th"], kw["tw"], kw["tiles"]) == (19, 36, 4) and oh % kw["th"] and ow % kw["tw"]
    assert _plan(GEOMS["one_pixel"], k)["pp"] == k["kDwMaxPlanes"] == 64 and DC.out_size(GEOMS["one_pixel"]) == (1, 1)
    assert _plan(GEOMS["mnv2_s1"], k)["pp"] > 1 and GEOMS["mult2"].mult == 2 and DC.K(GEOMS["k7_s2"]) == 49
    assert DC.K(GEOMS["even_k"]) % 2 == 0 and DC.K(GEOMS["even_k_pad"]) % 2 == 0 and DC.K(GEOMS["pointwise"]) == 1


# ---- the entry point's argument checks ----------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        pytest.skip("libdfq_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def _good():
    d = _lib.IntDwConv2dDesc()
    d.x, d.min_dev, d.max_dev, d.b_codes, d.b_scale, d.b_zero = 0x1004, 0x2004, 0x2008, 0x3000, 0x4004, 0x4008
    d.bias, d.out = 0x5004, 0x6004
    d.B, d.C, d.H, d.W, d.mult, d.KH, d.KW = 2, 6, 7, 7, 2, 3, 2
    d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w = 1, 2, 1, 0, 1, 2
    d.x_bits, d.x_symmetric, d.b_signed, d.flags = 8, 0, 1, _lib.DFQ_INT_B_PACK4 | _lib.DFQ_SCALE_F32
    return d


def test_argument_validation_without_a_device(lib):
    """Every refusal the header lists comes back before any device call: this runs on a machine
    without a GPU."""
    L = lib
    assert L.dfq_int_dwconv2d(None, None) == _lib.DFQ_ERR_INVALID
    extents = ("B", "C", "H", "W", "mult", "KH", "KW", "stride_h", "stride_w", "dil_h", "dil_w")
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
        assert L.dfq_int_dwconv2d(C.byref(d), None) == _lib.DFQ_ERR_INVALID, (name, value)

    def call(**kw):
        d = _good()
        for k, v in kw.items():
            setattr(d, k, v)
        return L.dfq_int_dwconv2d(C.byref(d), None)

    def sized(**kw):
        return call(**{**dict(KH=1, KW=1, stride_w=1, dil_w=1, pad_h=0, flags=0), **kw})

    # (a descriptor that passes every check is never sent from here: its pointers are made up)
    # the limits: C * mult at most 2^28, C * H * W and N * OH * OW below 2^31, B * OH * OW at most 2^31
    assert sized(C=1 << 20, mult=(1 << 8) + 1, H=1, W=1) == _lib.DFQ_ERR_INVALID
    assert sized(C=1 << 11, H=1 << 10, W=1 << 10) == _lib.DFQ_ERR_INVALID
    assert sized(C=1, mult=1 << 11, H=1 << 10, W=1 << 10) == _lib.DFQ_ERR_INVALID
    assert sized(B=(1 << 21) + 1, C=1, H=1 << 5, W=1 << 5) == _lib.DFQ_ERR_INVALID
    # the dilated kernel does not fit the padded image
    for kw in ({"H": 2, "pad_h": 0}, {"W": 2}, {"dil_h": 5}, {"KW": 5}):
        assert call(**kw) == _lib.DFQ_ERR_SHAPE, kw
    assert call(H=2, pad_h=0, x=0x1002) == _lib.DFQ_ERR_INVALID      # alignment is looked at before the output extent
    # too many taps, packed B with an odd K, one output's footprint beyond the code bytes, a grid beyond int32
    taps = _lib.DFQ_INT_DW_MAX_TAPS
    assert taps == 64
    assert call(KH=5, KW=13, H=16, W=64, flags=0) == _lib.DFQ_ERR_UNSUPPORTED                 # taps + 1
    assert call(KH=1, KW=taps + 1, H=16, W=2 * taps + 4, flags=0) == _lib.DFQ_ERR_UNSUPPORTED
    assert call(KH=3, KW=3, W=9) == _lib.DFQ_ERR_UNSUPPORTED                                   # K = 9 packed
    assert call(KH=3, KW=3, dil_h=200, dil_w=100, H=512, W=512, pad_h=0, flags=0) == _lib.DFQ_ERR_UNSUPPORTED   # 401 x 201 bytes
    assert sized(B=1 << 28, C=1 << 28, mult=1, H=1, W=1) == _lib.DFQ_ERR_UNSUPPORTED          # 2^56 planes, 64 a block


def test_desc_matches_the_header(tmp_path):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "dfq_hip.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct dfq_int_dwconv2d_desc\s*\{(.*?)\}\s*dfq_int_dwconv2d_desc;", text, flags=re.S).group(1)
    fields = re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*;", body)
    assert fields == [f for f, _ in _lib.IntDwConv2dDesc._fields_]
    assert [f if f != "mult" else "N" for f in fields] == [f for f, _ in _lib.IntConv2dDesc._fields_]   # N replaced by mult, nothing else
    assert "dfq_int_dwconv2d" in _lib.EXPORTS and "#define DFQ_ABI_VERSION 1" in text
    assert re.search(r"int dfq_int_dwconv2d\(const dfq_int_dwconv2d_desc\* d, void\* stream\);", text)
    build = (ROOT / "data_free_quantization_amd" / "build.py").read_text()
    assert "dfq_int_dwconv.hip" in build and "dfq_int_dwconv_plan.cpp" in build
    assert "dfq_int_dwconv2d" in (ROOT / "INTEGRATION.md").read_text()
    if CXX is None:
        pytest.skip("no host C++ compiler for the layout probe")
    # the compiler's layout against ctypes'
    probe = tmp_path / "probe.cpp"
    probe.write_text('#include <cstddef>\n#include <cstdio>\n#include "dfq_hip.h"\nint main() {\n'
                     '  printf("sizeof %zu\\n", sizeof(dfq_int_dwconv2d_desc));\n' +
                     "".join('  printf("%s %%zu\\n", offsetof(dfq_int_dwconv2d_desc, %s));\n' % (f, f) for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run([CXX, "-std=c++17", "-I", str(ROOT / "include"), str(probe), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines())
    assert int(got.pop("sizeof")) == C.sizeof(_lib.IntDwConv2dDesc) == 8 * 8 + 2 * 8 + 13 * 8 + 6 * 4
    assert {f: int(v) for f, v in got.items()} == {f: getattr(_lib.IntDwConv2dDesc, f).offset for f in fields}


def test_python_rejects_cpu_tensors_and_bad_arguments():
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)   # noqa: E731
    f32 = lambda *s: torch.ones(*s)   # noqa: E731
    x = torch.randn(2, 4, 5, 5)
    rng = dict(min_value=-1.0, max_value=1.0)
    intmm.reset_linear_calls()
    with pytest.raises(RuntimeError, match="ROCm GPU only.*no CPU fallback"):
        intmm.int_dwconv2d(x, u8(4, 9), f32(1), None, 3, padding=1, **rng)
    with pytest.raises(TypeError):
        intmm.int_dwconv2d(None, u8(4, 9), f32(1), None, 3, **rng)
    for bits in (1, 9, 16):
        with pytest.raises(ValueError):
            intmm.int_dwconv2d(x, u8(4, 9), f32(1), None, 3, bits=bits, **rng)
    assert intmm.LINEAR_CALLS == 0 and intmm.DW_MAX_TAPS == _lib.DFQ_INT_DW_MAX_TAPS
    import inspect
    sig = inspect.signature(intmm.int_dwconv2d)
    assert list(sig.parameters) == list(inspect.signature(intmm.int_conv2d).parameters)
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[8:])


def test_the_forward_scope_takes_the_depthwise_switch():
    from data_free_quantization_amd.utils import quantize as Q
    state = lambda: (Q._INT_MATMUL, Q._INT_CONV, Q._INT_DW)   # noqa: E731
    assert state() == (False, False, False)
    with pytest.raises(ValueError, match="needs conv=True"):
        with Q.int_matmul_forward(depthwise=True):
            pass
    assert state() == (False, False, False)
    intmm.LINEAR_CALLS = 7
    with Q.int_matmul_forward(conv=True, depthwise=True):
        assert intmm.LINEAR_CALLS == 0 and state() == (True, True, True)
        with Q.int_matmul_forward(conv=True):
            assert state() == (True, True, False)
            with Q.int_matmul_forward():
                assert state() == (True, False, False)
            assert state() == (True, True, False)
        assert state() == (True, True, True)
    assert state() == (False, False, False)
    with pytest.raises(KeyError):
        with Q.int_matmul_forward(conv=True, depthwise=True):
            raise KeyError("restored on the way out of an exception too")
    assert state() == (False, False, False)


def test_which_layers_route():
    """groups == in_channels > 1, out_channels a multiple of it, padding_mode "zeros", a tuple or int
    padding, grids of at most 8 bits and at most DW_MAX_TAPS taps route under depthwise=True;
    nothing changes without it."""
    from data_free_quantization_amd.utils import quantize as Q
    layer = Q.QuantConv2d
    dw, dw2, grouped, same, circ, wide, act16, big, k3 = (
        layer(8, 8, 3, padding=1, groups=8), layer(8, 16, 3, stride=2, padding=2, dilation=2, groups=8), layer(8, 8, 3, padding=1, groups=4),
        layer(8, 8, 3, padding="same", groups=8), layer(8, 8, 3, padding=1, groups=8), layer(8, 8, 3, padding=1, groups=8, num_bits=16),
        layer(8, 8, 3, padding=1, groups=8, num_bits_act=16), layer(8, 8, (5, 13), padding=6, groups=8), layer(8, 8, 3, padding=1))
    mxl = layer(8, 8, 3, padding=1, groups=8)
    mxl.weight_format = "mxfp4"
    circ.padding_mode = "circular"
    every = (dw, dw2, grouped, same, circ, wide, act16, big, mxl, k3)
    assert not any(m._int_routed() for m in every)
    with Q.int_matmul_forward(conv=True, depthwise=True):
        assert [m._int_routed() for m in every] == [True, True, False, False, False, False, False, False, False, True]
        assert [m._int_dw_routed() for m in (dw, dw2, grouped, same, circ, big, k3)] == [True, True, False, False, False, False, False]
        q = Q.QConv2d(8, 8, 3, padding=1, groups=8)
        assert q._int_routed() and q._int_dw_routed() and not q._int_conv_routed()
    with Q.int_matmul_forward(conv=True):
        assert [m._int_routed() for m in every] == [False] * 9 + [True]
        assert not dw._int_dw_routed()


@pytest.mark.parametrize("name,total,depthwise", [("mobilenetv2", 53, 17), ("deeplab", 61, 17)])
def test_every_layer_of_the_depthwise_models_routes(name, total, depthwise):
    """On the CPU-constructed zoo model with its Conv2d / Linear layers switched to Quant* ones:
    conv=True routes all but the depthwise layers, depthwise=True every one."""
    import torch.nn as nn
    from data_free_quantization_amd import zoo
    from data_free_quantization_amd.utils import quantize as Q
    model = zoo.build(name, seed=0, relu=True).eval()

    def quant_twin(m):
        if isinstance(m, nn.Conv2d):
            q = Q.QuantConv2d(m.in_channels, m.out_channels, m.kernel_size, m.stride, m.padding, m.dilation, m.groups, m.bias is not None)
            q.padding_mode = m.padding_mode
            return q
        return Q.QuantLinear(m.in_features, m.out_features, m.bias is not None)

    layers = [quant_twin(m) for m in model.modules() if isinstance(m, (nn.Conv2d, nn.Linear))]
    dws = [m for m in layers if isinstance(m, nn.Conv2d) and m.groups > 1]
    assert (len(layers), len(dws)) == (total, depthwise)
    assert all(m.groups == m.in_channels == m.out_channels and tuple(m.kernel_size) == (3, 3) for m in dws)
    with Q.int_matmul_forward(conv=True):
        assert sum(m._int_routed() for m in layers) == total - depthwise and not any(m._int_routed() for m in dws)
    with Q.int_matmul_forward(conv=True, depthwise=True):
        assert all(m._int_routed() for m in layers) and [m for m in layers if isinstance(m, nn.Conv2d) and m._int_dw_routed()] == dws
    if name == "deeplab":
        assert any(m.dilation != (1, 1) for m in dws)


def test_cli_flag():
    from data_free_quantization_amd import main_dfq
    a = main_dfq.get_argument(["--quantize", "--int_matmul", "--int_matmul_conv", "--int_matmul_depthwise"])
    assert a.int_matmul is True and a.int_matmul_conv is True and a.int_matmul_depthwise is True
    assert main_dfq.get_argument(["--quantize", "--int_matmul", "--int_matmul_conv"]).int_matmul_depthwise is False
    assert main_dfq.get_argument(["--quantize"]).int_matmul_depthwise is False
    for argv in (["--quantize", "--int_matmul", "--int_matmul_depthwise"], ["--quantize", "--int_matmul_depthwise"],
                 ["--int_matmul_depthwise"], ["--quantize", "--int_matmul_conv", "--int_matmul_depthwise"],
                 ["--quantize", "--weight_format", "mxfp4", "--mx_matmul", "mxfp8", "--mx_matmul_conv", "--int_matmul_depthwise"]):
        with pytest.raises(SystemExit):
            main_dfq.get_argument(argv)
    assert "--int_matmul_depthwise" in main_dfq.__doc__
