"""scale_dyn('velocity' / 'trapezoid') without a GPU: the NumPy / SciPy restatement (tests/scale_oracle.py) and the host functions of
the port (read_par, get_true_anomaly, effective_velocity_annual, the veff**2 logic) against the unmodified reference's outputs
(tests/golden/scale.npz), the signatures, the error paths that need no device, and the new symbols of the C ABI."""
import inspect
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import scale_cases as sc  # noqa: E402
import scale_checks as ck  # noqa: E402
import scale_oracle as so  # noqa: E402


@pytest.fixture(scope="module")
def gold(golden):
    return golden("scale.npz")


def _mjd(gold):
    o = sc.observation()
    mjd = np.asarray(o.mjd, dtype=np.longdouble) + np.asarray(o.times, dtype=np.longdouble) / 86400
    mjd += np.divide(gold["eph_ssb"], 86400)
    return o, mjd


def _pars(name):
    pars, kw, _ = sc.VELOCITY[name]
    p = dict(pars)
    for key, arg in (("s", "s"), ("d", "d"), ("KIN", "inc"), ("KOM", "Omega")):       # dynspec.py:3993-4012
        if key not in p:
            p[key] = kw[arg]
    return p, kw


# ---------------------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("name", list(sc.TRAPEZOID))
def test_trapezoid_oracle_equals_the_reference(gold, name):
    okw, kw = sc.TRAPEZOID[name]
    o = sc.observation(**okw)
    assert ck.same_bits(so.trapezoid(o.dyn, o.freqs, o.times, **kw), gold[f"t_{name}_trapdyn"])


def test_trapezoid_keep_counts():
    from scintools_amd import arcfit
    for okw, _ in sc.TRAPEZOID.values():
        o = sc.observation(**okw)
        assert np.array_equal(arcfit.trapezoid_keep(o.freqs, o.times), so.trapezoid_keep(o.freqs, o.times))
    o = sc.observation(**sc.TRAPEZOID["wide"][0])
    assert so.trapezoid_keep(o.freqs, o.times)[0] == 1 and so.trapezoid_keep(o.freqs, o.times)[-1] == o.nsub
    o = sc.observation(**sc.TRAPEZOID["late"][0])
    assert so.trapezoid_keep(o.freqs, o.times)[0] == 0


@pytest.mark.parametrize("name", list(sc.VELOCITY))
def test_velocity_oracle_equals_the_reference(gold, name):
    """The same scipy routine on the same axes: array_equal, from the reference's own veff_ra / veff_dec."""
    from scintools_amd import arcfit
    p, kw = _pars(name)
    ra, dec = np.array(gold[f"v_{name}_eva_ra"]), np.array(gold[f"v_{name}_eva_dec"])
    veff2, ra, dec = arcfit.effective_velocity_squared(p, ra, dec, vism_ra=kw.get("vism_ra"), vism_dec=kw.get("vism_dec"),
                                                       vism_zeta=kw.get("vism_zeta"), zeta=kw.get("zeta"))
    assert np.array_equal(ra, gold[f"v_{name}_veff_ra"]) and np.array_equal(dec, gold[f"v_{name}_veff_dec"])   # same NumPy lines
    veff = np.sqrt(veff2)
    assert veff.dtype == np.longdouble
    o = sc.observation()
    assert np.array_equal(so.velocity(o.dyn, veff), gold[f"v_{name}_vdyn"])
    # the port's grid is the oracle's, cast to float64 as interp1d does before the spline sees it
    x, xnew = arcfit.velocity_grid(veff)
    x0, xnew0 = so.velocity_grid(veff)
    assert x.dtype == xnew.dtype == np.float64 and np.array_equal(x, x0.astype(float)) and np.array_equal(xnew, xnew0.astype(float))
    if f"v_{name}_vlamdyn" in gold.files:
        assert np.array_equal(so.velocity(gold[f"v_{name}_lamdyn"], veff), gold[f"v_{name}_vlamdyn"])


def test_moment_algorithm_within_the_recorded_tolerance(gold):
    """What tests/golden/scale_tolerances.json records is reproduced here (the GPU bound is 10 x that, at least 1e-12)."""
    with open(os.path.join(HERE, "golden", "scale_tolerances.json")) as fh:
        recorded = json.load(fh)["moment_algorithm_vs_reference"]
    o = sc.observation()
    worst = 0.0
    for name in sc.VELOCITY:
        p, kw = _pars(name)
        from scintools_amd import arcfit
        veff2 = arcfit.effective_velocity_squared(p, np.array(gold[f"v_{name}_eva_ra"]), np.array(gold[f"v_{name}_eva_dec"]),
                                                  vism_ra=kw.get("vism_ra"), vism_dec=kw.get("vism_dec"),
                                                  vism_zeta=kw.get("vism_zeta"), zeta=kw.get("zeta"))[0]
        x, xnew = arcfit.velocity_grid(np.sqrt(veff2))
        worst = max(worst, ck.rel(so.moments_rows(o.dyn, x, xnew), gold[f"v_{name}_vdyn"]))
    print(f"scale: moment algorithm vs reference {worst:.3e} (recorded {recorded:.3e})")
    assert worst <= 2 * recorded + 1e-16 and ck.TOL == 1e-12


def test_spline_system_matches_the_independent_one():
    from scintools_amd import arcfit
    x = np.cumsum(sc.contrast_veff(60, 50.0))
    h, a, b, c = so.spline_system(x)
    h2, sub, inv, sup, end = arcfit._spline_system(x)
    assert np.array_equal(h, h2) and np.array_equal(a, sub) and np.allclose(sup[1], c[1] / b[1], rtol=1e-15)
    # the warm-up rule never gives up: the Thomas factors of a spline system stay below about 1/2 for any spacing
    rng = np.random.default_rng(0)
    for veff in (np.ones(1100), sc.contrast_veff(1100, 50.0), 10 ** rng.uniform(0, 4, 1100), np.where(np.arange(1100) % 2, 1.0, 50.0)):
        assert arcfit.spline_rows_route(np.cumsum(veff))[0] == "blocked"
    assert arcfit.spline_rows_route(np.arange(130.0))[0] == "lds"
    assert arcfit.spline_rows_route(np.arange(4 * sc.BLOCK + 2.0))[0] == "blocked"
    assert arcfit.spline_rows_route(np.arange(4 * sc.BLOCK + 1.0))[0] == "lds"


# ------------------------------------------------------------------------------------------------------- the host functions
@pytest.mark.parametrize("name", list(sc.VELOCITY))
def test_host_functions_equal_the_reference(gold, name, capsys):
    from scintools_amd import scint_models, scint_utils
    p, kw = _pars(name)
    o, mjd = _mjd(gold)
    ta = scint_utils.get_true_anomaly(mjd, dict(p))
    assert ck.close_longdouble(ta, gold[f"v_{name}_true_anomaly"])
    out = scint_models.effective_velocity_annual(dict(p), np.array(gold[f"v_{name}_true_anomaly"]), np.array(gold["eph_vra"]),
                                                 np.array(gold["eph_vdec"]), mjd=mjd)
    for tag, v in zip(("eva_ra", "eva_dec", "vp_ra", "vp_dec"), out):
        assert ck.close_longdouble(v, gold[f"v_{name}_{tag}"]), tag


def test_read_par(gold, tmp_path):
    from scintools_amd import scint_utils
    path = tmp_path / "test.par"
    path.write_text(sc.PARFILE)
    got = scint_utils.read_par(str(path))
    assert got == json.loads(str(gold["par_json"]))
    assert got["ECC"] == 0.1 and got["PB_ERR"] == 1.2e-9 and got["PSRJ_TYPE"] == "s" and "NITS" not in got


def test_signatures_equal_the_reference():
    from scintools_amd import scint_models, scint_utils
    from scintools_amd.dynspec import Dynspec
    want = {
        (Dynspec, "scale_dyn"): dict(scale='lambda', window_frac=0.1, pars=None, parfile=None, window='hanning', spacing='auto',
                                     s=None, d=None, vism_ra=None, vism_dec=None, Omega=None, inc=None, vism_zeta=None, zeta=None,
                                     lamsteps=False, velocity=False, trap=False),
        (Dynspec, "calc_sspec"): dict(prewhite=False, halve=True, plot=False, lamsteps=False, input_dyn=None, input_x=None,
                                      input_y=None, trap=False, window='hanning', window_frac=0.1, return_sspec=False,
                                      velocity=False),
        (scint_utils, "get_ssb_delay"): dict(mjds=inspect.Parameter.empty, raj=inspect.Parameter.empty,
                                             decj=inspect.Parameter.empty, message=True),
        (scint_utils, "get_earth_velocity"): dict(mjds=inspect.Parameter.empty, raj=inspect.Parameter.empty,
                                                  decj=inspect.Parameter.empty, radial=False),
        (scint_utils, "read_par"): dict(parfile=inspect.Parameter.empty),
        (scint_utils, "get_true_anomaly"): dict(mjds=inspect.Parameter.empty, pars=inspect.Parameter.empty),
        (scint_models, "effective_velocity_annual"): dict(params=inspect.Parameter.empty, true_anomaly=inspect.Parameter.empty,
                                                          vearth_ra=inspect.Parameter.empty, vearth_dec=inspect.Parameter.empty,
                                                          mjd=None),
    }
    for (owner, name), kw in want.items():
        sig = inspect.signature(getattr(owner, name))
        assert [(k, v.default) for k, v in sig.parameters.items() if k != "self"] == list(kw.items()), name


# ------------------------------------------------------------------------------------------------------------- error paths
def test_missing_parameters(gold, monkeypatch):
    from scintools_amd.dynspec import Dynspec
    ck.seeded(monkeypatch, gold)
    d = Dynspec(dyn=sc.observation(), verbose=False)
    with pytest.raises(ValueError, match="Requires dictionary of parameters or .par file"):
        d.scale_dyn(scale='velocity')
    with pytest.raises(ValueError, match="Requires dictionary of parameters or .par file"):
        d.calc_sspec(velocity=True)                        # without a previous scale_dyn('velocity', pars=...)
    base = {k: v for k, v in sc.BINARY.items() if k not in ("s", "d", "KIN", "KOM")}
    for have, text in ((dict(), "screen distance s"), (dict(s=0.5), "pulsar distance d"), (dict(s=0.5, d=1.0), r"\(KIN\)"),
                       (dict(s=0.5, d=1.0, inc=60.0), r"\(KOM\)")):
        with pytest.raises(ValueError, match=text):
            d.scale_dyn(scale='velocity', pars=dict(base), **have)
    with pytest.raises(KeyError, match="PB"):              # the reference: get_true_anomaly needs PB (stored text below)
        d.scale_dyn(scale='velocity', pars=dict(sc.NO_PB))
    assert str(gold["no_pb_error"]) == "KeyError: 'PB'"
    with pytest.raises(ValueError, match="Window unknown"):
        d.scale_dyn(scale='trapezoid', window='boxcar')


def test_zeta_is_scaled_in_place_like_the_reference():
    """`zeta *= np.pi / 180` (dynspec.py:4022): a float is rebound, an array argument is changed for the caller."""
    from scintools_amd import arcfit
    ra, dec = np.ones(3, dtype=np.longdouble), np.ones(3, dtype=np.longdouble)
    z = np.array(90.0)
    v2 = arcfit.effective_velocity_squared({}, ra, dec, zeta=z, vism_zeta=0.0)[0]
    assert z == np.pi / 2 and np.allclose(np.asarray(v2, dtype=float), 1.0)
    p = dict(zeta=90.0)
    arcfit.effective_velocity_squared(p, ra, dec)
    assert p["zeta"] == 90.0


def test_ephemeris_functions_name_astropy(monkeypatch):
    from scintools_amd import scint_utils
    monkeypatch.setitem(sys.modules, "astropy", None)      # `import astropy` raises ImportError, installed or not
    with pytest.raises(ImportError, match="astropy"):
        scint_utils.get_ssb_delay(np.array([55000.0]), "04:37:15.9", "-47:15:09.1")
    with pytest.raises(ImportError, match="astropy"):
        scint_utils.get_earth_velocity(np.array([55000.0]), "04:37:15.9", "-47:15:09.1")


def test_still_refused():
    from scintools_amd.dynspec import Dynspec
    d = Dynspec(dyn=sc.observation(), verbose=False)
    for call in (lambda: d.norm_sspec(velocity=True), lambda: d.fit_arc(velocity=True), lambda: d.correct_dyn(velocity=True),
                 lambda: d.calc_scattered_image(trap=True)):
        with pytest.raises(NotImplementedError, match="not ported"):
            call()


def test_no_gpu_no_fallback(gold, monkeypatch):
    import torch
    from scintools_amd import _lib
    from scintools_amd.dynspec import Dynspec
    ck.seeded(monkeypatch, gold)
    d = Dynspec(dyn=sc.observation(), verbose=False)
    if not torch.cuda.is_available():
        for call in (lambda: d.scale_dyn(scale='velocity', pars=dict(sc.BINARY)), lambda: d.scale_dyn(scale='trapezoid'),
                     lambda: d.calc_sspec(trap=True)):
            with pytest.raises(_lib.ScintHipError):
                call()


def test_library_exports_the_new_symbols():
    from scintools_amd import _lib
    names = ("scint_spline_resample_rows", "scint_spline_resample_rows_workspace_bytes", "scint_trap_scale")
    assert set(names) <= set(_lib.header_symbols()) and set(names) <= set(_lib._SIGNATURES)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in names)
    assert [p.kind for p in _lib._PARAMS["scint_trap_scale"]] == ["device", "scalar", "scalar", "scalar", "device", "device",
                                                                  "device", "device", "device", "device"]
    assert _lib._PARAMS["scint_spline_resample_rows"][7].kind == "host"          # end[4]
