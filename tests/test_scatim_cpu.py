"""Dynspec.calc_scattered_image without a GPU: the NumPy / SciPy restatement (tests/scatim_oracle.py) against the unmodified
reference's outputs (tests/golden/scatim.npz), scipy's own behaviour that the port copies (clamping, non-finite pixels, short axes),
and the host logic of the port up to the device call."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import scatim_cases as sc  # noqa: E402
import scatim_checks as ck  # noqa: E402
import scatim_oracle as so  # noqa: E402


@pytest.fixture(scope="module")
def gold(golden):
    return golden("scatim.npz")


@pytest.mark.parametrize("case", list(sc.CASES))
def test_oracle_against_reference(gold, case):
    """The reference's image within K eps S |fdop_y| of the oracle's (this measures K_ref), its axis and crop equal."""
    o_im, o_ax, o_eta, lin, fdop_y = ck.oracle_case(case, gold)
    sspec, fdop, tdel, eta = ck.case_inputs(case, gold)
    r0, r1, c0, c1 = (int(v) for v in gold[f"{case}_crop"])
    assert lin.shape == (r1 - r0, c1 - c0)
    assert np.array_equal(o_ax, gold[f"{case}_scattered_image_ax"])
    ck.assert_close(f"{case} reference vs oracle:", gold[f"{case}_scattered_image"], o_im, lin, fdop_y)


def test_cases_cover_the_branches(gold):
    crop = {c: tuple(int(v) for v in gold[f"{c}_crop"]) for c in sc.CASES}
    assert crop["b"] == (0, 10, 316, 320)                  # the corner fallback: slice bound -4, the k = 3 minimum
    assert crop["d"][1] < 128 and crop["d"][2:] == (0, 256)  # flim == 0: rows cropped, every column kept
    sspec, fdop, tdel, eta = ck.case_inputs("e", gold)
    fx = gold["e_scattered_image_ax"]
    assert np.mean((fx[:, None]**2 + fx[None, :]**2) * eta > tdel[-1]) > 0.5          # most delays clamp
    assert len(set(np.round(np.diff(sc.field("uneven")[2]), 12))) > 30              # case f: uneven delay knots
    eta_c = so.beta_to_eta(float(gold["c_betaeta"]), sc.sim().freq)
    assert eta_c == float(gold["c_eta"])


def test_separable_evaluation_is_scipys():
    """RectBivariateSpline(x, y, z).ev equals the clamped nested not-a-knot CubicSpline, outside the knots too."""
    from scipy.interpolate import RectBivariateSpline
    rng = np.random.default_rng(1)
    for nx_, ny_ in ((4, 4), (5, 9), (37, 53)):
        x, y = np.cumsum(0.1 + rng.random(nx_)), np.cumsum(0.1 + rng.random(ny_))
        z = 10**(4 * rng.random((nx_, ny_)))
        ye = np.broadcast_to(np.linspace(y[0] - 1, y[-1] + 1, 13), (7, 13))
        xe = np.linspace(x[0] - 1, x[-1] + 1, 7)[:, None] + 0.01 * rng.random((7, 13))
        ref = RectBivariateSpline(x, y, z).ev(xe, ye)
        assert np.max(np.abs(so.spline_ev(x, y, z, xe, ye) - ref)) <= 16 * ck.EPS * z.max()


def test_scipy_nonfinite_and_short_axes():
    """What the port copies: a NaN or inf pixel raises nothing and makes every value NaN; an axis of 3 points raises FITPACK's error."""
    from scipy.interpolate import RectBivariateSpline
    from scintools_amd import arcfit
    x, y = np.arange(6.0), np.arange(7.0)
    for bad in (np.nan, np.inf):
        z = np.ones((6, 7))
        z[2, 3] = bad
        assert np.all(np.isnan(RectBivariateSpline(x, y, z).ev(np.array([0.0, 4.5]), np.array([0.0, 6.0]))))
    for shape in ((3, 7), (6, 3)):
        with pytest.raises(Exception) as ref:
            RectBivariateSpline(np.arange(float(shape[0])), np.arange(float(shape[1])), np.ones(shape))
        with pytest.raises(Exception) as got:
            arcfit._check_spline_axes(np.arange(float(shape[0])), np.arange(float(shape[1])), shape)
        assert type(got.value) is type(ref.value) and str(got.value) == str(ref.value)
    with pytest.raises(ValueError, match="x must be strictly increasing"):
        arcfit._check_spline_axes(np.array([0.0, 1, 1, 2]), y, (4, 7))
    with pytest.raises(ValueError, match="y dimension of z"):
        arcfit._check_spline_axes(x, y, (6, 8))


def test_spline_warm_is_the_blocking_rule():
    """_spline_warm (new) is what _spline_blocks sized its warm-up with: same blocks as before on a uniform and an uneven axis."""
    from scintools_amd import arcfit
    for x in (np.arange(700.0), np.cumsum(0.2 + np.random.default_rng(3).random(900))):
        h, sub, inv, sup, end = arcfit._spline_system(x)
        rows, warm = arcfit._spline_blocks(sub, inv, sup, len(x))
        assert rows == 128 and warm == arcfit._spline_warm(sub, inv, sup, len(x)) and 24 <= warm <= 96
        assert 0.5 ** warm < 1e-7 and np.max(np.abs(sup[1:-2])) <= 0.5 + 1e-12      # diagonally dominant: a factor of >= 2 per knot


def test_public_signature():
    import inspect
    from scintools_amd.dynspec import Dynspec
    sig = inspect.signature(Dynspec.calc_scattered_image)
    want = dict(input_sspec=None, input_eta=None, input_fdop=None, input_tdel=None, sampling=64, lamsteps=False, trap=False,
                ref_freq=1400, clean=True, s=None, veff=None, d=None, fit_arc=True, plot_fit=False, plot=False, plot_log=True,
                use_angle=False, use_spatial=False)
    assert [p for p in sig.parameters][1:] == list(want)
    assert {k: v.default for k, v in sig.parameters.items() if k != "self"} == want


def test_no_gpu_no_fallback():
    """Without a GPU the method raises, it never computes on the host; the keywords outside the hot path raise everywhere."""
    import torch
    from scintools_amd import _lib
    from scintools_amd.dynspec import Dynspec
    sspec, fdop, tdel = sc.field("uneven")
    d = Dynspec(dyn=sc.sim(), verbose=False)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.ScintHipError):
            d.calc_scattered_image(input_sspec=sspec, input_fdop=fdop, input_tdel=tdel, input_eta=0.3, plot_log=False)
    for kw in (dict(plot=True), dict(plot_fit=True), dict(trap=True)):
        with pytest.raises(NotImplementedError):
            d.calc_scattered_image(**kw)
