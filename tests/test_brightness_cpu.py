"""The NumPy restatement of the brightness-distribution model (tests/brightness_oracle.py) against the unmodified reference's outputs
(tests/golden/brightness_<case>.npz) and against scipy.interpolate.griddata on the local scipy; the case builder's assertions; the
simplex-to-bitmap conversion.  Runs without a GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import brightness_cases as bc  # noqa: E402
import brightness_checks as ck  # noqa: E402
import brightness_oracle as bo  # noqa: E402


@pytest.mark.parametrize("case", list(bc.CASES))
def test_case_builder(case):
    """All three Jacobian branches, the stated lengths, no query on the grid's boundary: asserted inside build()."""
    o = bc.build(case)
    assert (case in bc.NAN_CASES) == bool(np.isnan(o["SS"]).any())


@pytest.mark.parametrize("case", list(bc.CASES))
def test_oracle_reproduces_golden(case):
    """With the stored bitmap: the loop body exactly, B exactly (the same np.fft calls), SS and acf to rounding; then the same with
    every transform through the Bluestein restatement -- the figures ORACLE_DEV that fix the device's tolerance."""
    g = ck.load_golden(case)
    o = bo.model(diagonals=g["diagonals"], **bc.kwargs(case))
    for k in ("jacobian", "thetax", "thetay", "B"):
        assert np.array_equal(o[k], g[k]), k
    for k in ("SS", "acf"):
        assert np.array_equal(np.isnan(o[k]), np.isnan(g[k]))
    ob = bo.model(diagonals=g["diagonals"], fft2=bo.fft2_bluestein, **bc.kwargs(case))
    for k in ("B", "SS", "acf"):
        d, db = ck.peak_dev(o[k], g[k]), ck.peak_dev(ob[k], g[k])
        print(case, k, "deviation / peak: np.fft", d, "Bluestein", db, "recorded", ck.ORACLE_DEV[k])
        assert np.isnan(d) or max(d, db) <= ck.ORACLE_DEV[k]


@pytest.mark.parametrize("case", list(bc.CASES))
def test_live_qhull_equals_griddata(case):
    """The oracle on the bitmap of this scipy's Delaunay against this scipy's griddata: the same interpolant to rounding."""
    a = bo.model(diagonals="qhull", **bc.kwargs(case))
    b = bo.model(use_griddata=True, **bc.kwargs(case))
    assert np.array_equal(np.isnan(a["SS"]), np.isnan(b["SS"]))
    d = ck.peak_dev(a["SS"], b["SS"])
    print(case, "SS deviation / peak", d)
    assert d <= ck.ORACLE_DEV["SS"]


def test_bluestein_restatement_equals_fft2():
    """For the power-of-two case (and the others): the oracle's chirp-z equals np.fft.fft2."""
    for case in ("b", "a", "c", "d"):
        rho = np.array(bc.build(case)["acf_efield"])
        ref = np.fft.fft2(rho)
        d = np.abs(bo.fft2_bluestein(rho) - ref).max() / np.abs(ref).max()
        print(case, rho.shape, d)
        assert d <= 1e-14
    k = np.arange(4000, 4093, dtype=np.int64)                   # the integer phase against the float one the issue warns of
    exact = np.exp(-1j * np.pi * ((k * k) % (2 * 4093)) / 4093)
    assert np.abs(exact - np.exp(-1j * np.pi * (k.astype(float) ** 2) / 4093)).max() > 1e-13


def test_main_diagonal_inside_envelope():
    for case in bc.CASES:
        g, o = ck.load_golden(case), bc.build(case)
        ok = ~np.isnan(g["SS"])
        assert np.all(np.abs(o["SS"] - g["SS"])[ok] <= o["envelope"][ok] + ck.TOL["SS"] * np.nanmax(np.abs(g["SS"])))
        assert np.abs(o["SS"] - g["SS"])[ok].max() > 1e-6 * np.nanmax(np.abs(g["SS"]))     # the two triangulations do differ


def test_diagonals_from_simplices():
    from scintools_amd.scint_sim import diagonals_from_simplices
    n = 5
    rng = np.random.default_rng(3)
    want = rng.random((n - 1, n - 1)) < 0.5
    tris = []
    for iy in range(n - 1):
        for ix in range(n - 1):
            p00, p10, p01, p11 = iy * n + ix, iy * n + ix + 1, (iy + 1) * n + ix, (iy + 1) * n + ix + 1
            tris += [[p00, p10, p11], [p11, p01, p00]] if want[iy, ix] else [[p00, p10, p01], [p10, p11, p01]]
    tris = np.array(tris)[rng.permutation(len(tris))]
    assert np.array_equal(diagonals_from_simplices(tris, n), want)
    with pytest.raises(ValueError, match="two simplices"):
        diagonals_from_simplices(tris[1:], n)
    bad = tris.copy()
    bad[0] = [0, 1, 2 * n]
    with pytest.raises(ValueError, match="one grid cell"):
        diagonals_from_simplices(bad, n)
    mixed = np.array([[0, 1, 3], [0, 2, 3]][:1] + [[0, 1, 2]])        # a 2 x 2 grid: one triangle of each diagonal
    with pytest.raises(ValueError, match="share a diagonal"):
        diagonals_from_simplices(mixed, 2)
