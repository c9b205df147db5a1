"""The MX scale search (dfq_mx_quantize_search_batch) without a GPU: the numpy statement
against the floor statements it extends, the figures that motivated it, the case set's own
validity (hand-made expectations, the cap on undecided blocks), the re-quantization finding
(a searched MXFP8 weight does not survive the floor rule), the dequantizers, the new entry
point's argument checks and binding, and the Python-side errors."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from data_free_quantization_amd import _lib, export, mx
from tests import mx6_cases as M6
from tests import mx_cases as MC
from tests import mx_search_cases as SC

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "data_free_quantization_amd" / "libdfq_hip.so"


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_the_floor_candidate_is_the_floor_statement():
    """Candidate 0 is mx_cases' / mx6_cases' contract, bit for bit, on their own cases."""
    cases = {c.name: c for c in SC.all_cases()}
    n = 0
    for prefix, mod in (("mx_", MC), ("mx6_", M6)):
        for c in mod.all_cases():
            s = cases[prefix + c.name]
            assert s.x is c.x
            c0 = s.ref["cand"][0]
            for k in ("codes", "scales", "element_codes"):
                assert np.array_equal(c0[k], c.ref[k]), (c.name, k)
            assert np.array_equal(_bits(c0["y"]), _bits(c.ref["y"])), c.name
            floor = SC.statement(c.x, c.fmt, search=False)
            assert np.array_equal(floor["codes"], c.ref["codes"]) and np.array_equal(_bits(floor["y"]), _bits(c.ref["y"]))
            n += s.ref["take1"].size
    assert n == 84666   # the blocks the issue's counts are about


def test_the_search_never_makes_a_block_noisier():
    took = 0
    for c in SC.all_cases():
        r = c.ref
        chosen = np.where(r["take1"], r["N"][1], r["N"][0])
        assert (chosen <= r["N"][0]).all(), c.name
        assert (r["N"][1][r["take1"]] < r["N"][0][r["take1"]]).all(), c.name
        assert not (r["take1"] & r["termwise_equal"]).any(), c.name
        # the block's noise is its y's: the whole tensor is no noisier either
        e1, e0 = (r["y"].astype(np.float64) - c.x) ** 2, (r["cand"][0]["y"].astype(np.float64) - c.x) ** 2
        assert e1.sum() <= e0.sum() * (1 + 1e-12), c.name
        assert (r["scales"] != 0xFF).all(), c.name
        took += int(r["take1"].sum())
    assert took > 5000


#: (floor dB, searched dB) on Gaussian x 0.05 and on outlier_data(0, (64, 1024)), and the share of the Gaussian tensor's blocks that take X0 + 1
TABLE = {"mxfp4": ((18.56, 18.96), (17.25, 17.56), 0.21), "mxfp6_e3m2": ((25.31, 25.63), (25.12, 25.61), 0.13),
         "mxfp6_e2m3": ((30.90, 30.99), (29.60, 29.66), 0.05), "mxfp8": ((30.08, 31.54), (29.41, 31.46), 0.21)}


@pytest.mark.parametrize("fmt", list(TABLE))
def test_the_measured_gain_is_reproduced(fmt):
    gauss = (0.05 * np.random.default_rng(0).standard_normal((4096, 32))).astype(np.float32)
    for x, want in ((gauss, TABLE[fmt][0]), (SC.outlier_data(0, (64, 1024)), TABLE[fmt][1])):
        r = SC.statement(x, fmt)
        got = (SC.sqnr_db(x, r["cand"][0]["y"]), SC.sqnr_db(x, r["y"]))
        print(fmt, got, float(r["take1"].mean()))
        assert abs(got[0] - want[0]) <= 0.05 and abs(got[1] - want[1]) <= 0.05, (fmt, got, want)
        assert got[1] > got[0]
        if x is gauss:   # the share is the Gaussian tensor's, in whole per cent
            assert round(100 * float(r["take1"].mean())) == round(100 * TABLE[fmt][2]), fmt
        # X0 - 1 and X0 + 2 never win a block: the search is two candidates
        xb, X0 = r["xb"], r["X0"]
        best = np.minimum(r["N"][0], r["N"][1])
        for d in (-1, 2):
            assert (SC.noise(xb, SC.candidate(xb, X0 + d, fmt)["yb"], X0) >= best).all(), (fmt, d)


def test_the_case_set_is_valid():
    cases = SC.all_cases()
    n_blocks = sum(c.ref["take1"].size for c in cases)
    undecided = sum(int(c.ref["undecided"].sum()) for c in cases)
    termwise = sum(int(c.ref["termwise_equal"].sum()) for c in cases)
    print("blocks", n_blocks, "undecided", undecided, "termwise equal", termwise)
    assert undecided <= SC.UNDECIDED_CAP * n_blocks   # the cap: a condition on the set, not a measurement
    inherited = [c for c in cases if c.name.startswith(("mx_", "mx6_"))]
    assert sum(int(c.ref["undecided"].sum()) for c in inherited) == 343
    assert sum(int(c.ref["termwise_equal"].sum()) for c in inherited) == 23413
    for fmt in SC.FORMATS:
        mine = {c.name: c for c in cases if c.fmt == fmt}
        for stem in ("band_", "band_unaligned_inplace_", "amax_pow2_", "one_nonzero_", "zeros_", "negzeros_", "extremes_",
                     "extremes_inplace_"):
            assert stem + fmt in mine, stem + fmt
        # the inherited axes: both alignment paths, partial blocks, every khw, every output set, decided both ways
        assert {c.offset for c in mine.values()} == {0, 1, 3} and {c.khw for c in mine.values()} >= {1, 9, 25, 49}, fmt
        assert {c.outputs for c in mine.values()} == {"all", "inplace", "nodst", "nocodes"}, fmt
        assert any(c.x.shape[1] % SC.BLOCK for c in mine.values()), fmt
        dec = [(c.ref["take1"] & ~c.ref["undecided"]).sum() for c in mine.values()]
        keep = [(~c.ref["take1"] & ~c.ref["undecided"] & ~c.ref["termwise_equal"]).sum() for c in mine.values()]
        # (E4M3's normal elements round alike under both exponents: few of its blocks keep X0 by a margin)
        assert sum(dec) > 500 and sum(keep) > (10 if fmt == "mxfp8" else 500), fmt
        ext = mine["extremes_" + fmt]
        assert np.abs(ext.x[ext.x != 0]).min() == 2.0 ** -100 and np.abs(ext.x).max() > 2.0 ** 119
        assert np.isfinite(ext.ref["N"][0]).all() and (ext.ref["N"][0] > 0).all()   # the common factor: no underflow
    for c in cases:
        a = np.abs(c.x[c.x != 0])
        assert np.isfinite(c.x).all() and (a.size == 0 or a.min() >= MC.MIN_MAG), c.name
        if c.expect is None:
            continue
        r = c.ref
        nonzero = np.abs(r["xb"]).max(axis=2) != 0
        assert not r["undecided"].any(), c.name   # what a hand-made block must do is beyond the margin
        if c.expect == "x1":
            assert nonzero.all() and r["take1"].all(), c.name
            assert r["cand"][0]["saturated"].any(axis=2).all(), c.name
        elif c.expect == "x0":
            assert nonzero.all() and not r["take1"].any() and not r["termwise_equal"].any(), c.name
            _, e = np.frexp(np.abs(r["xb"]).max(axis=2))
            assert (np.abs(r["xb"]).max(axis=2) == np.ldexp(0.5, e)).all(), c.name   # amax a power of two
        else:
            assert c.expect == "termwise" and r["termwise_equal"].all() and not r["take1"].any(), c.name
            assert (r["scales"] == r["cand"][0]["scales"]).all(), c.name
    z = next(c for c in cases if c.name == "negzeros_mxfp8")
    assert (z.ref["scales"] == 0).all() and np.signbit(z.ref["y"]).all() and (z.ref["codes"][:, 0] == 0x80).all()
    one = next(c for c in cases if c.name == "one_nonzero_mxfp4")
    assert (np.count_nonzero(one.ref["xb"], axis=2) <= 1).all() and np.count_nonzero(one.x) == 5


def _searched_values():
    """(case, searched y) for the cases whose rows are whole blocks' worth of interest: all of them."""
    return [(c, c.ref["y"]) for c in SC.all_cases()]


def test_requantizing_a_searched_weight():
    """Floor-rule re-quantization gives a searched y back bit for bit in MXFP4 and both MXFP6
    formats, not in MXFP8 (1.875 * 2^k under X1 is 480 under X0 and saturates to 448);
    re-quantization with the search gives it back in all four."""
    moved = {fmt: 0 for fmt in SC.FORMATS}
    for c, y in _searched_values():
        floor = SC.statement(y, c.fmt, search=False)
        again = SC.statement(y, c.fmt)
        assert np.array_equal(_bits(again["y"]), _bits(y)), c.name
        # the stored grid has no noise; a block not on the floor grid must therefore have moved up
        chosen = np.where(again["take1"], again["N"][1], again["N"][0])
        assert (chosen == 0).all(), c.name
        same = (_bits(floor["y"]) == _bits(y)).all()
        if c.fmt != "mxfp8":
            assert same, c.name
        else:
            moved[c.fmt] += int((_bits(floor["y"]) != _bits(y)).sum())
    crafted = next(c for c in SC.all_cases() if c.name == "requant_mxfp8")
    y = crafted.ref["y"]
    assert (np.abs(y).reshape(3, 3, 32).max(axis=2) == np.abs(crafted.x).reshape(3, 3, 32).max(axis=2)).all()   # 480 * 2^k kept
    floor = SC.statement(y, "mxfp8", search=False)
    diff = (_bits(floor["y"]) != _bits(y)).reshape(3, 3, 32)
    assert diff.any(axis=2).all()   # every crafted block
    assert (np.abs(floor["y"][diff.reshape(3, 96)] / y[diff.reshape(3, 96)]) == 448.0 / 480.0).all()
    assert moved["mxfp8"] > 0


def test_the_dequantizers_give_the_searched_values():
    for c in SC.all_cases():
        r = c.ref
        shape = list(c.x.shape)
        got = mx.mx_dequantize(torch.from_numpy(r["codes"]), torch.from_numpy(r["scales"]), shape, c.fmt)
        assert np.array_equal(_bits(got.numpy()), _bits(r["y"])), c.name
        meta = {"weight_format": c.fmt, "layers": {"w": {"shape": shape}}, "clip": None, "mx_scale_search": True}
        got = export.dequantize(meta, "w", {"codes": torch.from_numpy(r["codes"]), "scales": torch.from_numpy(r["scales"])})
        assert np.array_equal(_bits(got.numpy()), _bits(r["y"])), c.name


def test_floor_scale_bytes_is_the_floor_rule():
    raised = 0
    for c in SC.all_cases():
        got = mx.floor_scale_bytes(torch.from_numpy(c.x), c.fmt).numpy()
        assert got.dtype == np.uint8 and np.array_equal(got, c.ref["cand"][0]["scales"]), c.name
        assert np.array_equal(c.ref["scales"] > got, c.ref["take1"]), c.name
        raised += int((c.ref["scales"] > got).sum())
    assert raised > 5000
    w = torch.from_numpy(SC.all_cases()[0].x)
    assert np.array_equal(mx.floor_scale_bytes(w.reshape(w.shape[0], 1, -1), SC.all_cases()[0].fmt).numpy(),
                          SC.all_cases()[0].ref["cand"][0]["scales"])
    with pytest.raises(ValueError):
        mx.floor_scale_bytes(w, "mxfp6")


# ---- the entry point ----------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        pytest.skip("libdfq_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def _good(n=2):
    d = (_lib.MxDesc * n)()
    for k in range(n):
        d[k].src, d[k].dst, d[k].codes, d[k].scales, d[k].esum = 0x1000, 0x1000, 0x2000, 0x3000, 0x4000
        d[k].rows, d[k].row_len, d[k].khw, d[k].format, d[k].flags = 4, 18, 9, _lib.DFQ_MX_FP4_E2M1, 0
    return d


def test_search_entry_validates_its_arguments_without_a_device(lib):
    """dfq_mx_quantize_search_batch: the descriptors, workspace and error codes of
    dfq_mx_quantize_batch, checked before anything touches the device."""
    L = lib
    both = (L.dfq_mx_quantize_search_batch, L.dfq_mx_quantize_batch)
    d = _good()
    assert L.dfq_mx_quantize_search_batch(d, -1, 256, 1 << 20, None) == _lib.DFQ_ERR_INVALID
    bad = [("format", 2), ("format", -1), ("flags", 1), ("flags", -1), ("rows", 0), ("rows", -3), ("row_len", 0),
           ("row_len", 1 << 41), ("khw", 0), ("khw", -9), ("src", None), ("src", 0x1002), ("dst", 0x1001),
           ("esum", 0x4002)]
    for name, value in bad:
        keep = getattr(d[1], name)
        setattr(d[1], name, value)
        for fn in both:
            assert fn(d, 2, 256, 1 << 20, None) == _lib.DFQ_ERR_INVALID, (name, value)
        setattr(d[1], name, keep)
    d[1].dst = d[1].codes = d[1].scales = d[1].esum = None
    assert L.dfq_mx_quantize_search_batch(d, 2, 256, 1 << 20, None) == _lib.DFQ_ERR_INVALID
    d = _good()
    d[1].row_len = 20   # error sums need whole khw groups per row
    assert L.dfq_mx_quantize_search_batch(d, 2, 256, 1 << 20, None) == _lib.DFQ_ERR_SHAPE
    d = _good()
    d[1].rows, d[1].row_len, d[1].khw = 2, 65 * 40, 65
    assert L.dfq_mx_quantize_search_batch(d, 2, 256, 1 << 20, None) == _lib.DFQ_ERR_UNSUPPORTED
    d = _good()
    assert L.dfq_mx_quantize_search_batch(d, 0, None, 0, None) == _lib.DFQ_OK
    assert L.dfq_mx_quantize_search_batch(None, 0, None, 0, None) == _lib.DFQ_OK
    assert L.dfq_mx_quantize_search_batch(None, 1, None, 0, None) == _lib.DFQ_ERR_INVALID
    # the same workspace rule, and every format (a mixed list) is taken
    d = _good(4)
    for k, fmt in enumerate((_lib.DFQ_MX_FP4_E2M1, _lib.DFQ_MX_FP6_E2M3, _lib.DFQ_MX_FP8_E4M3, _lib.DFQ_MX_FP6_E3M2)):
        d[k].format = fmt
    d[1].rows = 100000
    need = L.dfq_mx_quantize_ws_bytes(d, 4)
    assert need >= 256
    for fn in both:
        assert fn(d, 4, None, need, None) == _lib.DFQ_ERR_WORKSPACE
        assert fn(d, 4, 256, 16, None) == _lib.DFQ_ERR_WORKSPACE
        assert fn(d, 4, 256, need - 1, None) == _lib.DFQ_ERR_WORKSPACE
        assert fn(d, 4, 128, need, None) == _lib.DFQ_ERR_INVALID   # misaligned workspace


def test_the_binding_matches_the_header():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "dfq_hip.h").read_text(), flags=re.S)
    proto = r"int %s\(const dfq_mx_desc\* descs, int32_t n, void\* ws, int64_t ws_bytes, void\* stream\);"
    assert re.search(proto % "dfq_mx_quantize_search_batch", text) and re.search(proto % "dfq_mx_quantize_batch", text)
    assert "dfq_mx_quantize_search_batch" in _lib.EXPORTS
    assert "#define DFQ_ABI_VERSION 1" in text
    assert mx._MX.itemsize == 72   # the descriptor is unchanged: flags stays "must be 0"
    if LIB.exists():
        L = _lib.load()
        assert L.dfq_mx_quantize_search_batch.argtypes == L.dfq_mx_quantize_batch.argtypes
        assert L.dfq_mx_quantize_search_batch.restype == L.dfq_mx_quantize_batch.restype


# ---- Python-side errors ---------------------------------------------------------
def test_cli_flag():
    from data_free_quantization_amd import main_dfq
    a = main_dfq.get_argument(["--quantize", "--weight_format", "mxfp4", "--mx_scale_search"])
    assert a.mx_scale_search and a.weight_format == "mxfp4"
    assert not main_dfq.get_argument(["--quantize", "--weight_format", "mxfp8"]).mx_scale_search
    for argv in (["--quantize", "--mx_scale_search"], ["--quantize", "--weight_format", "int", "--mx_scale_search"],
                 ["--quantize", "--weight_format", "mxfp4", "--mx_scale_search", "--clip_search"],
                 ["--weight_format", "mxfp4", "--mx_scale_search"]):
        with pytest.raises(SystemExit):
            main_dfq.get_argument(argv)


def test_python_rejects_cpu_tensors_and_integer_formats():
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        mx.mx_quantize([mx.MXItem(torch.randn(4, 4), dst=torch.empty(4, 4))], scale_search=True)
    assert mx.mx_quantize([], scale_search=True) == []
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        mx.mx_linear(torch.randn(4, 32), torch.randn(8, 32), None, "mxfp8", weight_scale_search=True)
    from data_free_quantization_amd.pipeline import run_dfq
    from data_free_quantization_amd.utils.layer_transform import quantize_targ_layer
    with pytest.raises(ValueError, match="mx_scale_search"):
        quantize_targ_layer({}, 8, 8, [torch.nn.Linear], weight_format="int", mx_scale_search=True)
    with pytest.raises(ValueError, match="mx_scale_search"):
        run_dfq(torch.nn.Linear(2, 2), {}, {}, [torch.nn.Linear], weight_format="int", mx_scale_search=True)
    with pytest.raises(ValueError, match="mx_scale_search"):
        export.save("unused", {}, {}, bits=8, granularity="tensor", symmetric=False, mx_scale_search=True)
