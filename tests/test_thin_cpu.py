"""Host side of the thin-screen search (fitting_proc='thin'): the NumPy oracle against the reference's golden, the
host logic of prep_thetatheta('thin'), the crop / cut ranges handed to the kernels, and the new C entry points' argument
checks.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import thin_oracle as to  # noqa: E402


@pytest.fixture(scope="module")
def g(golden):
    z = golden("thin.npz")
    return {k: z[k] for k in z.files}


def test_oracle_two_curve_map_is_the_reference_bit_for_bit(g):
    CS = np.fft.fftshift(np.fft.fft2(g["dyn"]))
    for tag in ("eq_lo", "eq", "ne", "eq_hi"):
        f1, f2 = g[f"fac_{tag}"]
        e2 = g["edges"] if tag in ("eq_lo", "eq_hi") else g["arclet"]
        red, er1, er2, wrap = to.two_curve_map(CS, g["tau"], g["fd"], f1 * g["eta_true"], g["edges"], f2 * g["eta_true"], e2,
                                               stats=True)
        assert np.array_equal(red, g[f"map_{tag}"]) and np.array_equal(er1, g[f"er1_{tag}"]) and np.array_equal(er2, g[f"er2_{tag}"])
        if tag == "eq_lo":
            assert wrap.sum() > 100         # the golden covers the negative-Doppler wrap
    assert bool(g["wide_raises"])
    with pytest.raises(IndexError):
        to.two_curve_map(CS, g["tau"], g["fd"], 0.3 * g["eta_true"], g["wide"], 0.3 * g["eta_true"], g["wide"])


def test_oracle_singularvalue_calc_is_the_reference_bit_for_bit(g):
    CS = np.fft.fftshift(np.fft.fft2(g["dyn"]))
    for tag in ("cut0", "cut1", "cutall"):
        sv = [to.singularvalue_calc(CS, g["tau"], g["fd"], e, g["edges"], e, g["arclet"], float(g[f"cutval_{tag}"]))
              for e in g["sv_etas"]]
        assert np.array_equal(sv, g[f"sv_{tag}"])
    assert np.all(g["sv_cutall"] == 0.0)


def _tutorial(golden):
    from scintools_amd.dynspec import Dynspec
    f = golden("fit_thetatheta.npz")

    class B:
        dyn, freqs, times, dt, df = f["dspec"], f["freq"], f["time"], float(f["dt"]), float(f["df"])
    return Dynspec(dyn=B(), verbose=False)


def test_prep_thetatheta_thin_host_logic(golden, g):
    d = _tutorial(golden)
    d.prep_thetatheta(cwf=64, edges_lim=.3, eta_min=30, eta_max=50, fitting_proc='thin', arclet_lim=.15, center_cut=.02)
    assert np.array_equal(d.edges, g["tut_edges"])
    assert d.arclet_lim == float(g["tut_arclet_lim"]) and d.center_cut == float(g["tut_center_cut"])
    assert d.neta == int(g["tut_neta"]) and d.thetatheta_proc == 'thin'
    # defaults: arclet_lim = edges_lim, center_cut = 0
    d2 = _tutorial(golden)
    d2.prep_thetatheta(cwf=64, edges_lim=.3, eta_min=30, eta_max=50, fitting_proc='thin')
    assert np.array_equal(d2.edges, g["def_edges"])
    assert d2.arclet_lim == float(g["def_arclet_lim"]) and d2.center_cut == 0 and d2.neta == int(g["def_neta"])
    # the thin edges reach fd.max(), not fd.max()/2: without edges_lim they differ from the standard ones
    d3, d4 = _tutorial(golden), _tutorial(golden)
    d3.prep_thetatheta(cwf=64, eta_min=30, eta_max=50, fitting_proc='thin')
    d4.prep_thetatheta(cwf=64, eta_min=30, eta_max=50)
    assert d3.edges.max() > 1.9 * d4.edges.max()


def test_fit_path_parameter_list_is_the_references(golden):
    d = _tutorial(golden)
    d.prep_thetatheta(cwf=64, edges_lim=.3, eta_min=30, eta_max=50, fitting_proc='thin', arclet_lim=.15, center_cut=.02,
                      tau_mask=0.5)
    p = d._search_params_thin(3, 0)
    assert len(p) == 13
    freq2 = d.freqs[3 * 64:4 * 64]
    # filtered by arclet_lim BEFORE the scaling to the chunk (dynspec.py:1706-1709)
    assert np.array_equal(p[11], d.edges[np.abs(d.edges) < .15] * (freq2.mean() / d.fref))
    assert p[12] == .02 and p[9] is True


@pytest.mark.parametrize("seed", range(6))
def test_host_ranges_against_the_reference_masks(seed):
    from scintools_amd import ththmod
    rng = np.random.default_rng(seed)
    n1, n2 = int(rng.integers(2, 300)), int(rng.integers(2, 200))
    lim1 = rng.uniform(0.5, 3.0)
    e1 = np.linspace(-lim1, lim1 * rng.uniform(0.7, 1.0), n1)
    e2 = e1[np.abs(e1) < lim1 * rng.uniform(0.2, 1.0)]
    if e2.size < 2:
        e2 = e1[:3]
    tau_max = rng.uniform(0.5, 5.0)
    etas = np.geomspace(0.05, 20.0, 17) * rng.uniform(0.5, 2.0)
    cut = rng.uniform(0.0, 0.5)
    got = ththmod._thin_ranges(tau_max, e1, e2, etas, cut)
    c1, c2 = (e1[1:] + e1[:-1]) / 2, (e2[1:] + e2[:-1]) / 2
    for k, eta in enumerate(etas):
        p1, p2 = np.abs(c1) < np.sqrt(tau_max / eta), np.abs(c2) < np.sqrt(tau_max / eta)
        if not p1.any() or not p2.any():
            assert got[k, 1] == 0 or got[k, 3] == 0
            continue
        r0, n2k, c0, n1k, cut0, cut1 = got[k]
        assert np.array_equal(np.nonzero(p1)[0], np.arange(c0, c0 + n1k))
        assert np.array_equal(np.nonzero(p2)[0], np.arange(r0, r0 + n2k))
        er1 = np.zeros(p1.sum() + 1)
        er1[:-1] = e1[:-1][p1]
        er1[-1] = e1[1:][p1].max()
        cm = np.abs((er1[1:] + er1[:-1]) / 2) < cut
        assert np.array_equal(np.nonzero(cm)[0], np.arange(cut0, cut1))


def test_entry_points_workspace_and_argument_errors():
    from scintools_amd import _lib
    lib = _lib.load()
    assert lib.scint_version() == 108 == _lib.ABI_VERSION
    need = ctypes.c_size_t()
    assert lib.scint_two_curve_map_workspace_bytes(ctypes.byref(need)) == 0 and need.value >= 512
    assert lib.scint_sv_sweep_multi_workspace_bytes(300, 150, 52, 52, 300, 1, ctypes.byref(need)) == 0
    small = need.value
    assert small >= 52 * 16 * 300 * 150
    assert lib.scint_sv_sweep_multi_workspace_bytes(300, 150, 52, 8, 300, 1, ctypes.byref(need)) == 0 and need.value < small
    assert lib.scint_sv_sweep_multi_workspace_bytes(0, 150, 52, 8, 300, 1, ctypes.byref(need)) == _lib.SCINT_E_ARG
    assert lib.scint_sv_sweep_multi_workspace_bytes(20000, 150, 52, 8, 300, 1, ctypes.byref(need)) == _lib.SCINT_E_ARG
    geom = _lib.ThinGeom(64, 64, 0.1, 0.1, 0.1, 0.1)
    rng = (ctypes.c_int32 * 6)(0, 1, 0, 1, 0, 0)
    assert lib.scint_two_curve_map(None, ctypes.byref(geom), None, 4, None, 4, 1.0, 1.0, rng, 0, None, None, None, 0,
                                   None) == _lib.SCINT_E_ARG
    assert "null pointer" in _lib.last_error()
    one = (ctypes.c_int32 * 1)(0)
    d1 = (ctypes.c_double * 1)(1.0)
    out = ctypes.c_void_p(1)
    assert lib.scint_sv_sweep_multi(out, 1, 64 * 64, one, ctypes.byref(geom), out, 4, out, 4, rng, one, d1, d1, 1, 1e-12,
                                    0, 1, out, out, out, out, 1 << 20, None) == _lib.SCINT_E_ARG
    bad = (ctypes.c_int32 * 6)(0, 9, 0, 1, 0, 0)           # a crop past the grid
    assert lib.scint_sv_sweep_multi(out, 1, 64 * 64, one, ctypes.byref(geom), out, 4, out, 4, bad, one, d1, d1, 1, 1e-12,
                                    300, 1, out, out, out, out, 1 << 20, None) == _lib.SCINT_E_ARG
    assert "crop" in _lib.last_error()


def test_thin_is_implemented():
    import inspect
    from scintools_amd import dynspec, ththmod
    for name in ("two_curve_map", "singularvalue_calc", "single_search_thin", "sv_sweep_multi"):
        assert callable(getattr(ththmod, name))
    assert "NotImplementedError" not in inspect.getsource(dynspec.Dynspec.prep_thetatheta)
