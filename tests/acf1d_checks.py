"""The checks of the 1-D ACF fit, shared by the GPU tests (tests/test_gpu_acf1d.py) and the host-interpreted ones
(tests/test_acf1d_emu_cpu.py) -- TEST INFRASTRUCTURE.  `sp` is scintools_amd.scintpar; `to_dev` turns a NumPy array into the
float64 tensor the entry point takes (device memory on a GPU, host memory under the interpreter).

Bounds (tests/golden/acf1d_fit_tolerances.json, written by tests/golden/make_acf1d_tolerances.py, per kind of case):
  stationarity   10 x the oracle's own max_i |J^T r|_i / chi^2 at ITS solutions (both starts);
  values, errors 10 x the larger of the oracle's spread between its two starts and 64 eps (see the maker).
Weights: n eps max(w), the rounding of a sum of n terms in another order."""
import json
import os

import numpy as np

import acf1d_cases as cc
import acf1d_oracle as ao

EPS = np.finfo(float).eps
CONVERGED, ITER_CAP, SINGULAR, NONFINITE_INPUT = 0, 1, 2, 3
OUT_KEYS = cc.FIT_KEYS + cc.ERR_KEYS + ("chisqr", "redchi", "niter", "status", "tau0", "dnu0", "amp0", "wn0", "n_t", "n_f")
_tol = None


def tolerances():
    global _tol
    if _tol is None:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "acf1d_fit_tolerances.json")) as fh:
            _tol = json.load(fh)
    return _tol


def to_dev(sp, a):
    import torch
    return sp.device.to_device(a, torch.float64)


def run(sp, name, **extra):
    c = cc.case(name)
    return sp.acf1d_fit_device(to_dev(sp, c.stack), c.dt, c.df, c.bw, c.tobs, **dict(c.kw, **extra))


def same_bits(a, b, keys=OUT_KEYS, rows=slice(None)):
    return all(np.array_equal(np.asarray(a[k])[rows], np.asarray(b[k]), equal_nan=True) for k in keys)


def check_setup(sp, name):
    """Start values and crop lengths equal the oracle's exactly; the cropped cuts are the ACF's own bits; the weights agree to
    n eps max(w)."""
    out = run(sp, name, return_setup=True)
    setups, _ = cc.oracle(name)
    for b, s in enumerate(setups):
        for key, okey in (("tau0", "tau"), ("dnu0", "dnu"), ("amp0", "amp"), ("wn0", "wn")):
            assert out[key][b] == s[okey], (name, b, key, out[key][b], s[okey])
        assert (out["n_t"][b], out["n_f"][b]) == (len(s["x_t"]), len(s["x_f"])), (name, b)
        for cut in ("t", "f"):
            assert np.array_equal(out["y_" + cut][b], s["y_" + cut]), (name, b, cut)
            w, ow = out["w_" + cut][b], s["w_" + cut]
            bound = len(ow) * EPS * np.abs(ow).max()
            worst = np.abs(w - ow).max()
            assert w[0] == 0.0 and worst <= bound, (name, b, cut, worst, bound)


def check_fit(sp, name):
    """Every problem converges; stationarity on the host, independent of the oracle; values and standard errors against the
    oracle; kind (a): the planted parameters."""
    c = cc.case(name)
    tol = tolerances()[c.kind]
    vary = c.kw.get("alpha", 5/3) is None
    out = run(sp, name)
    setups, fits = cc.oracle(name)
    assert all(f["success"] for f in fits), name                       # the case list's promise
    assert np.array_equal(out["status"], np.zeros(len(fits), dtype=out["status"].dtype)), (name, out["status"], out["niter"])
    worst = dict(ratio=0.0, values=0.0, errors=0.0, planted=0.0)
    for b, (s, f) in enumerate(zip(setups, fits)):
        p = [out[k][b] for k in cc.FIT_KEYS]
        g, chi = ao.stationarity(p, s, vary)
        worst["ratio"] = max(worst["ratio"], g / chi if chi > 0 else 0.0)
        assert g <= tol["stationarity"] * chi, (name, b, g, chi)
        assert out["chisqr"][b] >= 0, (name, b)
        if c.kind == "b":            # (a kind (a) chi^2 is the rounding of exp and pow: two libraries do not agree on it)
            assert abs(out["chisqr"][b] - chi) <= 1e-9 * chi, (name, b, out["chisqr"][b], chi)
        n = len(s["x_t"]) + len(s["x_f"]) - (4 if vary else 3)
        assert out["redchi"][b] == out["chisqr"][b] / n, (name, b)
        for k in cc.FIT_KEYS:
            d = abs(out[k][b] - f[k]) / abs(f[k])
            worst["values"] = max(worst["values"], d)
            assert d <= tol["values_rtol"], (name, b, k, out[k][b], f[k])
        for k in cc.ERR_KEYS:
            if k == "alphaerr" and not vary:
                assert out[k][b] == 0.0 and out["alpha"][b] == c.kw.get("alpha", 5/3)
                continue
            d = abs(out[k][b] - f[k]) / abs(f[k])
            worst["errors"] = max(worst["errors"], d)
            assert np.isfinite(out[k][b]) and d <= tol["errors_rtol"], (name, b, k, out[k][b], f[k])
        if c.planted is not None:
            for i, k in enumerate(cc.FIT_KEYS):
                d = abs(out[k][b] - c.planted[b, i]) / abs(c.planted[b, i])
                worst["planted"] = max(worst["planted"], d)
                assert d <= tol["values_rtol"], (name, b, k, out[k][b], c.planted[b, i])
    print(name, "kind", c.kind, "niter max", int(out["niter"].max()), "worst", worst, "allowed", tol)


def check_status_paths(sp):
    """An all-NaN and an all-zero ACF between good ones report their status with NaN outputs; the good ones keep their bits;
    max_iter=1 ends every problem at the cap."""
    c = cc.case("real12")
    clean = run(sp, "real12")
    stack = np.concatenate([c.stack[:2], np.full_like(c.stack[:1], np.nan), c.stack[2:5], np.zeros_like(c.stack[:1]), c.stack[5:]])
    out = sp.acf1d_fit_device(to_dev(sp, stack), c.dt, c.df, c.bw, c.tobs)
    good = np.array([0, 1, 3, 4, 5] + list(range(7, 14)))
    assert out["status"][2] == NONFINITE_INPUT and out["status"][6] == SINGULAR
    for b in (2, 6):
        for k in cc.FIT_KEYS + cc.ERR_KEYS + ("chisqr", "redchi"):
            assert np.isnan(out[k][b]), (b, k)
    assert same_bits(out, clean, rows=good)
    capped = run(sp, "real12", max_iter=1)
    assert np.all(capped["status"] == ITER_CAP) and np.all(capped["niter"] == 1)
    for k in cc.FIT_KEYS + cc.ERR_KEYS + ("chisqr", "redchi"):
        assert np.isnan(capped[k]).all(), k
    assert same_bits(capped, clean, keys=("tau0", "dnu0", "amp0", "wn0", "n_t", "n_f"))


def check_deterministic(sp, name):
    assert same_bits(run(sp, name), run(sp, name))


def _dynspec(obs):
    from scintools_amd.dynspec import Dynspec
    return Dynspec(dyn=obs, verbose=False)


FIT_ATTRS = ("tau", "dnu", "tscat", "nscint", "fse_tau", "fse_dnu", "tauerr", "dnuerr", "amp", "amperr", "wn", "talpha", "talphaerr")
BYPRODUCTS = ("dnu_est", "dnu_esterr", "tscat_est", "modulation_index")


def check_dynspec(sp, alpha):
    """Dynspec.fit_scint_params on a kind (b) observation: every attribute against the oracle applied to the SAME (device) ACF."""
    import scintpar_oracle as so
    o = cc.observation()
    d = _dynspec(o)
    d.fit_scint_params(alpha=alpha)
    acf = d.acf
    tol = tolerances()["b"]
    s = ao.setup(acf, o.dt, o.df, o.bw, o.tobs)
    f = ao.fit(s, alpha=alpha)
    assert f["success"] and d.scint_fit_status == CONVERGED and d.scint_param_method == "acf1d" and not hasattr(d, "report")
    want = ao.fit_attrs(f, o, alpha, name=d.name)
    for k in FIT_ATTRS:
        rtol = tol["errors_rtol"] if "err" in k else tol["values_rtol"]
        print("fit_scint_params", k, getattr(d, k), want[k])
        if want[k] == 0:
            assert getattr(d, k) == 0, k
        else:
            assert abs(getattr(d, k) - want[k]) <= rtol * abs(want[k]), (k, getattr(d, k), want[k])
    nofit = so.nofit(acf, o.dyn, o)
    for k in BYPRODUCTS:
        np.testing.assert_allclose(getattr(d, k), nofit[k], rtol=1e-12, err_msg=k)
    n = len(s["x_t"]) + len(s["x_f"]) - (4 if alpha is None else 3)
    assert abs(d.scint_fit_redchi - f["chisqr"] / n) <= 1e-6 * f["chisqr"] / n and 1 <= d.scint_fit_niter <= 200


def check_dynspec_not_converged(sp, pytest):
    """A fit that cannot converge (a constant ACF cut has a zero start amplitude) warns and leaves the no-fit values."""
    o = cc.observation()
    d = _dynspec(o)
    d.acf = np.zeros((2 * o.dyn.shape[0], 2 * o.dyn.shape[1]))
    with pytest.warns(UserWarning, match="did not converge"):
        d.fit_scint_params()
    assert d.scint_fit_status == SINGULAR and d.scint_param_method == "nofit" and np.isnan(d.scint_fit_redchi)
    assert (d.tau, d.dnu, d.amp) == (o.tobs, o.bw, 0.0)


def check_cut(sp):
    """fit_scint_params_cut(1, 2) = six single fits of the six segments, bit for bit."""
    import torch
    o = cc.observation(rng_seed=22, nf=48, nt=64)
    d = _dynspec(o)
    d.fit_scint_params_cut(tcuts=1, fcuts=2)
    fnum, tnum = 16, 32
    assert d.cut_tau.shape == d.cut_fit_status.shape == (3, 2)
    for ii in range(3):
        for jj in range(2):
            seg = np.ascontiguousarray(o.dyn[ii * fnum:(ii + 1) * fnum, jj * tnum:(jj + 1) * tnum])
            acf = sp.acf_device(to_dev(sp, seg), subtract_mean=False)
            one = sp.acf1d_fit_device(acf, o.dt, o.df, fnum * o.df, tnum * o.dt)
            for attr, k in (("cut_tau", "tau"), ("cut_dnu", "dnu"), ("cut_tauerr", "tauerr"), ("cut_dnuerr", "dnuerr"),
                            ("cut_amp", "amp"), ("cut_fit_status", "status")):
                assert np.array_equal(getattr(d, attr)[ii, jj], one[k][0], equal_nan=True), (ii, jj, attr)
    assert np.all(d.cut_fit_status == CONVERGED) and np.isfinite(d.cut_tau).all()


def check_arguments(sp, pytest):
    from scintools_amd import _lib
    c = cc.case("floor5")
    with pytest.raises(_lib.ScintHipError, match="max_iter"):
        run(sp, "floor5", max_iter=0)
    with pytest.raises(_lib.ScintHipError, match="bad shape"):
        sp.acf1d_fit_device(to_dev(sp, np.ones((1, 4, 16))), c.dt, c.df, c.bw, c.tobs)
    with pytest.raises(ValueError, match="stack of ACFs"):
        sp.acf1d_fit_device(to_dev(sp, np.ones((1, 1, 16, 16))), c.dt, c.df, c.bw, c.tobs)
