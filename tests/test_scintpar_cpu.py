"""CPU checks of the no-fit scintillation measurements: the NumPy oracle (tests/scintpar_oracle.py) reproduces the unmodified
reference's output (tests/golden/scintpar.npz, scintpar_cut.npz) bit for bit, and the product's argument and
NotImplementedError rules hold without a GPU."""
import json
import os

import numpy as np
import pytest

import scintpar_cases as cc
import scintpar_oracle as so
from oracle import sspec_oracle


@pytest.fixture(scope="module")
def g(golden):
    return golden("scintpar.npz")


@pytest.fixture(scope="module")
def gcut(golden):
    return golden("scintpar_cut.npz")


def test_stored_inputs_are_the_seeded_simulations(g):
    o = cc.simulate("even")
    s = cc.from_golden(g, "even")
    assert np.array_equal(o.dyn, s.dyn) and np.array_equal(o.freqs, s.freqs) and np.array_equal(o.times, s.times)
    assert (o.df, o.dt, o.bw, o.tobs) == (s.df, s.dt, s.bw, s.tobs)


@pytest.mark.parametrize("case", cc.OBS)
def test_oracle_reproduces_reference_bit_for_bit(g, case):
    o = cc.from_golden(g, case)
    acf = sspec_oracle.calc_acf(o.dyn)
    for variant, kw in cc.VARIANTS.items():
        p = so.nofit(acf, o.dyn, o, **kw)
        for name in cc.NOFIT_ATTRS:
            assert p[name] == float(g[f"{case}_{variant}_{name}"]), (variant, name)
        assert p["scint_param_method"] == "nofit"
    p = so.nofit(acf, o.dyn, o)
    tilt = so.acf_tilt(acf, o, p["tau"], p["dnu"])
    assert tilt == tuple(float(g[f"{case}_tilt_{name}"]) for name in cc.TILT_ATTRS)


def test_oracle_moments_skip_nan_inf_and_zero(g):
    o = cc.from_golden(g, "even")
    acf = sspec_oracle.calc_acf(o.dyn)
    holes = cc.poke_holes(o.dyn)
    assert np.isnan(holes).sum() == 84 and np.isinf(holes).sum() == 1 and (holes == 0).sum() == 80
    p = so.nofit(acf, holes, o)
    for name in cc.NOFIT_ATTRS:
        assert p[name] == float(g[f"holes_{name}"]), name
    keep = np.isfinite(holes) & (holes != 0)
    q = so.nofit_from_moments(acf, np.mean(holes[keep]), np.var(holes[keep]), o)
    assert all(q[name] == p[name] for name in cc.NOFIT_ATTRS)


def test_oracle_tie_fixture(g):
    acf = cc.tie_acf()
    assert np.array_equal(acf, g["tie_acf"])
    for row in cc.tie_rows():
        tied = np.flatnonzero(acf[row] == acf[row].max())
        assert len(tied) == 2 and np.argmax(acf[row]) == tied[0]
    o = cc.synthetic_observation()
    p = so.nofit(acf, o.dyn, o)
    for name in cc.NOFIT_ATTRS:
        assert p[name] == float(g[f"tie_{name}"]), name
    assert so.acf_tilt(acf, o, p["tau"], p["dnu"]) == tuple(float(g[f"tie_{name}"]) for name in cc.TILT_ATTRS)
    assert set(cc.tie_rows()) <= set(int(i[0]) for i in so.tilt_rows(acf.shape, o, p["dnu"]))


def test_edge_fixture_has_no_window():
    acf = cc.edge_acf()
    o = cc.synthetic_observation()
    p = so.nofit(acf, o.dyn, o)
    rows = [int(i[0]) for i in so.tilt_rows(acf.shape, o, p["dnu"])]
    assert acf.shape[0] // 2 + 1 in rows and np.argmax(acf[acf.shape[0] // 2 + 1]) == 1


@pytest.mark.parametrize("case", sorted(cc.CUTS))
def test_oracle_cut_dyn(g, gcut, case):
    o = cc.from_golden(g, case)
    tcuts, fcuts = cc.CUTS[case]
    cutdyn, cutsspec, cutacf = so.cut_dyn(o.dyn, len(o.freqs), len(o.times), tcuts, fcuts)
    assert np.array_equal(cutdyn, gcut[f"{case}_cutdyn"])
    assert np.array_equal(cutsspec, gcut[f"{case}_cutsspec"])
    fnum, tnum = o.dyn.shape[0] // (fcuts + 1), o.dyn.shape[1] // (tcuts + 1)
    assert cutdyn.shape == (fcuts + 1, tcuts + 1, fnum, tnum) and cutacf.shape == (fcuts + 1, tcuts + 1, 2 * fnum, 2 * tnum)


def test_oracle_acf_sspec(g, golden):
    with open(os.path.join(os.path.dirname(__file__), "golden", "scintpar_tolerances.json")) as fh:
        tol = json.load(fh)
    for case in cc.SSPEC_ACF:
        o = cc.from_golden(g, case)
        ref = g[f"{case}_acf_sspec"]
        got = so.acf_sspec(o.dyn)
        assert got.shape == ref.shape
        assert np.abs(got - ref).max() <= tol["acf_sspec_bound"][case]["bound"] * np.abs(ref).max()


# ---- the product without a GPU: what it refuses, and how -------------------------------------------------------------------
def _dynspec(g, case="small"):
    from scintools_amd.dynspec import Dynspec
    return Dynspec(dyn=cc.from_golden(g, case), verbose=False)


def test_acf_is_absent_before_calc_acf(g):
    d = _dynspec(g)
    assert not hasattr(d, "acf")
    d.acf = np.ones((4, 6))                      # a host assignment is an ordinary attribute
    assert hasattr(d, "acf") and d.acf.shape == (4, 6)
    del d.acf
    assert not hasattr(d, "acf")


@pytest.mark.parametrize("method", ["acf1d", "acf2d_approx", "acf2d", "sspec"])
def test_fitted_methods_name_lmfit(g, method):
    d = _dynspec(g)
    with pytest.raises(NotImplementedError, match=r"lmfit.*method='nofit'"):
        d.get_scint_params(method=method)
    with pytest.raises(NotImplementedError, match=r"lmfit.*method='nofit'"):    # the reference's default is a fitted method
        d.get_scint_params()
    d.acf = np.ones((48, 80))
    with pytest.raises(NotImplementedError, match=r"lmfit.*method='nofit'"):    # no dnu yet: goes through get_scint_params
        d.get_acf_tilt(method=method)
    assert not hasattr(d, "dnu")


def test_mcmc_and_plots_are_refused(g):
    d = _dynspec(g)
    with pytest.raises(NotImplementedError, match="mcmc"):
        d.get_scint_params(method="nofit", mcmc=True)
    for call in (lambda: d.get_scint_params(method="nofit", plot=True), lambda: d.get_acf_tilt(plot=True),
                 lambda: d.cut_dyn(1, 1, plot=True)):
        with pytest.raises(NotImplementedError, match="plot"):
            call()
    with pytest.raises(ValueError, match="Method not understood"):
        d.calc_acf(method="fft")


def test_no_cpu_fallback(g):
    """Without a GPU the measurements raise; they never compute on the host."""
    import torch
    from scintools_amd import _lib
    from scintools_amd import build
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    build.build(verbose=False)
    d = _dynspec(g)
    for call in (lambda: d.get_scint_params(method="nofit"), lambda: d.get_acf_tilt(method="nofit"), lambda: d.cut_dyn(1, 1),
                 lambda: d.calc_acf(method="sspec")):
        with pytest.raises(_lib.ScintHipError):
            call()


def test_cabi_argument_checks():
    """The new entry points through the one checked boundary (_lib.call): wrong kinds of argument are TypeErrors before the
    library is entered, bad sizes come back as SCINT_E_ARG with a message."""
    import ctypes
    import torch
    from scintools_amd import _lib, build
    build.build(verbose=False)
    _lib.load()
    for name in ("scint_acf_cuts", "scint_dyn_moments", "scint_dyn_moments_workspace_bytes", "scint_acf_row_peaks",
                 "scint_segment_cut", "scint_acf_sspec", "scint_acf_sspec_workspace_bytes"):
        assert name in _lib.header_symbols()
    a = torch.zeros(8, dtype=torch.float64)
    with pytest.raises(TypeError, match="cuts_out"):
        _lib.call("scint_acf_cuts", a, 2, 4, np.zeros(3), None)                   # a NumPy array where device memory goes
    with pytest.raises(TypeError, match="rows"):
        _lib.call("scint_acf_row_peaks", a, 2, 4, torch.zeros(1, dtype=torch.int64), 1, None, None, None, None)
    with pytest.raises(TypeError):
        _lib.call("scint_segment_cut", a, 2.0, 4, 1, 1, 1, 1, a, None)            # a float for a size
    need = ctypes.c_size_t()
    _lib.call("scint_dyn_moments_workspace_bytes", need)
    assert need.value >= 2 * 1024 * 8
    for name, args, msg in (
            ("scint_acf_cuts", (None, 2, 4, None, None), "null"),
            ("scint_dyn_moments", (None, 8, None, None, 0, None), "null"),
            ("scint_acf_row_peaks", (None, 2, 4, None, 1, None, None, None, None), "null"),
            ("scint_segment_cut", (None, 2, 4, 1, 1, 1, 1, None, None), "null"),
            ("scint_acf_sspec_workspace_bytes", (48, 64, need), "bad shape"),
            ("scint_acf_sspec_workspace_bytes", (64, 8, need), "bad shape")):
        with pytest.raises(_lib.ScintHipError, match=msg) as err:
            _lib.call(name, *args)
        assert err.value.status == _lib.SCINT_E_ARG
