"""The thin-screen curvature search (fitting_proc='thin') on an MI355X against the reference's golden (tests/golden/thin.npz)
and the NumPy oracle (tests/thin_oracle.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import thin_oracle as to  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def thth():
    from scintools_amd import ththmod
    from scintools_amd.device import require_gpu
    require_gpu()
    return ththmod


@pytest.fixture(scope="module")
def g(golden):
    z = golden("thin.npz")
    d = {k: z[k] for k in z.files}
    d["CS"] = np.fft.fftshift(np.fft.fft2(d["dyn"]))
    return d


def _tutorial(golden):
    from scintools_amd.dynspec import Dynspec
    f = golden("fit_thetatheta.npz")

    class B:
        dyn, freqs, times, dt, df = f["dspec"], f["freq"], f["time"], float(f["dt"]), float(f["df"])
    d = Dynspec(dyn=B(), verbose=False)
    d.prep_thetatheta(cwf=64, edges_lim=.3, eta_min=30, eta_max=50, fitting_proc='thin', arclet_lim=.15, center_cut=.02)
    return d


@pytest.mark.parametrize("tag", ["eq_lo", "eq", "ne", "eq_hi"])
def test_two_curve_map_vs_reference_golden(thth, g, tag):
    f1, f2 = g[f"fac_{tag}"]
    e2 = g["edges"] if tag in ("eq_lo", "eq_hi") else g["arclet"]
    red, er1, er2 = thth.two_curve_map(g["CS"], g["tau"], g["fd"], f1 * g["eta_true"], g["edges"], f2 * g["eta_true"], e2)
    assert red.shape == g[f"map_{tag}"].shape
    assert np.count_nonzero(red != g[f"map_{tag}"]) == 0
    assert np.array_equal(np.asarray(er1), g[f"er1_{tag}"]) and np.array_equal(np.asarray(er2), g[f"er2_{tag}"])
    with pytest.raises(IndexError):
        thth.two_curve_map(g["CS"], g["tau"], g["fd"], 0.3 * g["eta_true"], g["wide"], 0.3 * g["eta_true"], g["wide"])


def test_singularvalue_calc_vs_reference_golden(thth, g):
    for tag in ("cut0", "cut1", "cutall"):
        sv = [thth.singularvalue_calc(g["CS"], g["tau"], g["fd"], e, g["edges"], e, g["arclet"], float(g[f"cutval_{tag}"]))
              for e in g["sv_etas"]]
        np.testing.assert_allclose(sv, g[f"sv_{tag}"], rtol=1e-10, atol=0)


def test_tutorial_thin_vs_reference_golden(golden, g):
    d = _tutorial(golden)
    etas, eigs, popt = d.thetatheta_single(cf=0, ct=0, plot=False, arrays=True)
    assert np.array_equal(etas, g["tut_single_etas"])
    np.testing.assert_allclose(eigs, g["tut_single_eigs"], rtol=1e-9)
    np.testing.assert_allclose(popt, g["tut_single_popt"], rtol=1e-6)
    d.fit_thetatheta()
    assert np.array_equal(d.f0s, g["tut_f0s"])
    np.testing.assert_allclose(d.eta_evo, g["tut_eta_evo"], rtol=1e-6)
    np.testing.assert_allclose(d.eta_evo_err, g["tut_eta_evo_err"], rtol=1e-4)
    assert d.ththeta == pytest.approx(float(g["tut_ththeta"]), rel=1e-6)
    assert d.ththetaerr == pytest.approx(float(g["tut_ththetaerr"]), rel=1e-4)
    assert d.thth_eigs.shape == (16, 1, d.neta) and np.all(np.isfinite(d.thth_eigs))


def test_pool_route_equals_the_batched_route(golden):
    from multiprocessing.pool import ThreadPool
    d = _tutorial(golden)
    d.fit_thetatheta()
    batched = d.eta_evo.copy()
    with ThreadPool(2) as pool:
        d.fit_thetatheta(pool=pool)
    np.testing.assert_allclose(d.eta_evo, batched, rtol=1e-9)


def test_2048_single_chunk_against_dense_svd(thth):
    """A 2048^2 arc_dynspec chunk (npad = 0, 2048 thin edges): sigma_1 at four curvatures within 1e-10 of LAPACK, and
    bit-identical from run to run."""
    from scintools_amd.synth import arc_dynspec
    dyn, freqs, times, eta_true = arc_dynspec(2048, 2048, seed=3, nimg=32)
    dyn = dyn - dyn.mean()
    fd = to.fft_axis(times, 1000.0, 0)
    tau = to.fft_axis(freqs, 1.0, 0)
    edges = np.linspace(-fd.max(), fd.max(), 2048)
    arclet = edges[np.abs(edges) < 0.5 * fd.max()]
    etas = np.array([0.6, 0.9, 1.2, 1.8]) * eta_true
    cs_t = thth.conjugate_spectrum(dyn, 0, pad_value=0.0)
    CS = cs_t.cpu().numpy()
    a, info = thth.sv_sweep_multi(cs_t.unsqueeze(0), [(tau, fd, edges, arclet)], [etas], 0.01, return_info=True)
    b = thth.sv_sweep_multi(cs_t.unsqueeze(0), [(tau, fd, edges, arclet)], [etas], 0.01)
    assert np.array_equal(a[0], b[0])
    assert info["ranges"][:, 3].max() > 1000
    for e, v in zip(etas, a[0]):
        red, er1, _ = to.two_curve_map(CS, tau, fd, e, edges, e, arclet)
        red[:, np.abs((er1[1:] + er1[:-1]) / 2) < 0.01] = 0
        assert v == pytest.approx(np.linalg.svd(red, compute_uv=False)[0], rel=1e-10)


def test_standard_result_unchanged_after_a_thin_run(golden):
    from scintools_amd.dynspec import Dynspec
    f = golden("fit_thetatheta.npz")
    _tutorial(golden).fit_thetatheta()

    class B:
        dyn, freqs, times, dt, df = f["dspec"], f["freq"], f["time"], float(f["dt"]), float(f["df"])
    d = Dynspec(dyn=B(), verbose=False)
    d.prep_thetatheta(cwf=64, edges_lim=.3, eta_min=30, eta_max=50)
    d.fit_thetatheta()
    np.testing.assert_allclose(d.eta_evo, f["eta_evo"], rtol=1e-6)
    assert d.ththeta == pytest.approx(float(f["ththeta"]), rel=1e-6)
