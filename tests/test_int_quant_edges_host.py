"""tests/int_quant_edge_cases.py on the CPU: importing it runs its self-checks (the boundary data is
finite, dense in near-ties, covers the grid, is quantized wrongly without the exact path and rightly
with it; one code step shows in the expected bits)."""
import numpy as np
import pytest

from tests import int_quant_edge_cases as E


def test_case_lists_and_measured_shares():
    assert (len(E.LINEAR_CASES), len(E.CONV_CASES), len(E.DW_CASES)) == (174, 168, 224)
    assert len(set(E.LINEAR_CASES)) == 174 and len(set(E.CONV_CASES)) == 168 and len(set(E.DW_CASES)) == 224
    assert set(E.RANGES.values()) == {(-1.3, 2.5), (0.0, 6.0), (0.75, 5.5), (-4.0, -0.5), (-1.75, 1.5), (0.0, 0.0), (-1.5, 253.5)}
    assert E.BITS == (2, 3, 4, 5, 6, 7, 8)
    assert {b for _, b, _, _ in E.LINEAR_CASES} == set(E.BITS)
    print("boundary data at %(elements)d elements: near-tie share >= %(near_tie_share).3f, grid coverage >= "
          "%(grid_coverage).3f, wrong codes without the exact path %(wrong_codes)s" % E.MEASURED)
    assert E.MEASURED["near_tie_share"] >= 0.40 and E.MEASURED["grid_coverage"] >= 0.90 and E.MEASURED["wrong_codes"][0] >= 1


def test_integers_of_every_case_fit_int32():
    assert E.integers_fit_int32() < 2 ** 31


def test_the_checks_fail_for_a_quantizer_without_its_exact_path():
    """The inputs discriminate: with ``need`` forced false, check (e) fails."""
    def never_exact(x, s, zero, bits, sym, r, exact=True):
        return E.emulate(x, s, zero, bits, sym, r, exact=False)
    with pytest.raises(AssertionError):
        E._check_inputs(never_exact)
    E._check_inputs()   # MEASURED as it was


def test_ulp_steps_cross_zero_and_specials_are_all_present():
    v = E.ulp_step(np.zeros(7, np.float32), np.arange(-3, 4))
    assert np.array_equal(v, np.arange(-3, 4).astype(np.float32) * np.float32(2.0 ** -149))
    assert E.ulp_step(np.float32([1.0]), [1])[0] == np.nextafter(np.float32(1.0), np.float32(2.0))
    assert E.ulp_step(np.float32([-1.0]), [1])[0] == np.nextafter(np.float32(-1.0), np.float32(0.0))
    x = E.with_specials(E.boundary_x((70, 168), (-1.3, 2.5), 8, False))
    bits = set(x.view(np.uint32).reshape(-1).tolist())
    for sp in (-0.0, 0.0, -1e-40, 1e-40, -E.FLT_MAX, E.FLT_MAX, -np.inf, np.inf):
        assert int(np.float32(sp).view(np.uint32)) in bits
    assert not np.isnan(x).any() and 0.015 <= float((~np.isfinite(x) | (np.abs(x) < 1e-30) | (np.abs(x) > 1e38)).mean()) <= 0.03


def test_huge_scale_rows_are_finite_and_tie_dense():
    """The rows of the subnormal-reciprocal cases: s above 2^126, every |x| <= FLT_MAX, and a
    reciprocal flushed to zero gets most codes wrong where the quantizer as written gets none."""
    for pair, bits, sym in (((-1e38, 1e38), 2, True), ((-2e38, 2.5e38), 2, False), ((-2.2e40, 2.2e40), 8, True)):
        s, zero = E.qparams(pair, bits, sym)
        assert float(s) > E.TWO_126
        x = E.boundary_x((8, 512), pair, bits, sym)
        assert np.isfinite(x).all()
        want = E.oracle_codes(x, pair, bits, sym)[0]
        r = np.float32(1.0 / np.float64(s))
        assert 0.0 < float(r) < float(np.finfo(np.float32).tiny)
        assert np.array_equal(E.emulate(x, s, zero, bits, sym, r)[0], want)
        # r == 0 makes every code that of 0 (qmin's where x + negmn overflows: inf * 0); k is uniform
        # over at most five values per row of the grid, and at least three of them have another code
        flushed = E.emulate(x, s, zero, bits, sym, np.float32(0.0))[0]
        assert float((flushed != want).mean()) > 0.4, (pair, float((flushed != want).mean()))
