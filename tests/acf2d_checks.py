"""The checks of the approximate 2-D ACF fit, shared by the GPU tests (tests/test_gpu_acf2d.py) and the host-interpreted ones
(tests/test_acf2d_emu_cpu.py) -- TEST INFRASTRUCTURE.  `sp` is scintools_amd.scintpar.

Bounds (tests/golden/acf2d_fit_tolerances.json, written by tests/golden/make_acf2d_tolerances.py, per kind of case):
  stationarity   10 x the oracle's own max_i |J^T r|_i / chi^2 at ITS solutions (both starts);
  values, errors 10 x the larger of the oracle's spread between its two starts and 64 eps;
  phasegrad      the same on the scale max(|phasegrad|, the oracle's phasegraderr).
Weights: 16 eps relative -- two divisions, a square root, two reciprocals and three products, each within an ulp or two on either
side.  The model against the golden: see check_model."""
import json
import os

import numpy as np

import acf2d_cases as cc
import acf2d_oracle as ao

EPS = np.finfo(float).eps
CONVERGED, ITER_CAP, SINGULAR, NONFINITE_INPUT, NONFINITE_STEP, BAD_WINDOW = range(6)
RECT = ("f0", "nfw", "t0", "ntw")
START = tuple(k + "_start" for k in cc.FIT_KEYS)
OUT_KEYS = cc.FIT_KEYS + cc.ERR_KEYS + ("chisqr", "redchi", "niter", "status", "nnz", "argmax") + RECT + START
_tol = None


def tolerances():
    global _tol
    if _tol is None:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "acf2d_fit_tolerances.json")) as fh:
            _tol = json.load(fh)
    return _tol


def to_dev(sp, a):
    import torch
    return sp.device.to_device(a, torch.float64)


def run(sp, name, **extra):
    c = cc.case(name)
    return sp.acf2d_approx_fit_device(to_dev(sp, c.stack), c.dt, c.df, c.bw, c.tobs, **dict(c.kw, **extra))


def same_bits(a, b, keys=OUT_KEYS, rows=slice(None)):
    return all(np.array_equal(np.asarray(a[k])[rows], np.asarray(b[k]), equal_nan=True) for k in keys)


def check_setup(sp, name):
    """Rectangles, maxima and no-fit values equal the oracle's exactly; the start values are the device 1-D fit's where that
    converged (the no-fit values otherwise), alpha and phasegrad the oracle's; the window's y is the ACF's own bits; the weights
    agree to 16 eps with the zeros (so the roll and the centre) in the same places."""
    c = cc.case(name)
    out = run(sp, name, return_setup=True)
    one = sp.acf1d_fit_device(to_dev(sp, c.stack), c.dt, c.df, c.bw, c.tobs,
                              **{k: v for k, v in c.kw.items() if k in ("alpha", "nscale", "full_frame", "weighted", "bartlett")})
    setups, fits = cc.oracle(name)
    for b, s in enumerate(setups):
        if s is None:
            assert out["status"][b] == BAD_WINDOW and tuple(out[k][b] for k in RECT) == fits[b]["rect"], (name, b)
            continue
        assert tuple(out[k][b] for k in RECT) == s["rect"], (name, b, [out[k][b] for k in RECT], s["rect"])
        assert out["argmax"][b] == np.ravel_multi_index(s["argmax"], c.stack[b].shape), (name, b)
        for key in ("tau", "dnu", "amp"):
            assert out["fit1d"][key + "0"][b] == s["nofit"][key], (name, b, key)
            want = one[key][b] if one["status"][b] == CONVERGED else one[key + "0"][b]
            assert out[key + "_start"][b] == want, (name, b, key)
        assert out["alpha_start"][b] == s["p0"]["alpha"] and out["phasegrad_start"][b] == s["p0"]["phasegrad"], (name, b)
        assert np.array_equal(out["y"][b], s["y"]), (name, b)
        w, ow = out["w"][b], s["w"]
        assert np.array_equal(w == 0, ow == 0), (name, b)
        assert w[w.shape[0] // 2, w.shape[1] // 2] == 0.0 and out["nnz"][b] == np.count_nonzero(ow), (name, b)
        worst = np.abs(w - ow).max()
        assert worst <= 16 * EPS * np.abs(ow).max(), (name, b, worst)


def check_fit(sp, name):
    """Every problem converges; stationarity on the host, independent of the oracle's solution; values and standard errors against
    the oracle; kind (a): the planted parameters."""
    c = cc.case(name)
    tol = tolerances()[c.kind]
    vary = c.kw.get("alpha", 5/3) is None
    nv = 5 if vary else 4
    out = run(sp, name)
    setups, fits = cc.oracle(name)
    assert all(f["success"] for f in fits), name                       # the case list's promise
    assert np.array_equal(out["status"], np.zeros(len(fits), dtype=out["status"].dtype)), (name, out["status"], out["niter"])
    worst = dict(ratio=0.0, values=0.0, phasegrad=0.0, errors=0.0, planted=0.0)
    for b, (s, f) in enumerate(zip(setups, fits)):
        p = [out[k][b] for k in cc.FIT_KEYS]
        g, chi = ao.stationarity(p, s, vary)
        worst["ratio"] = max(worst["ratio"], g / chi if chi > 0 else 0.0)
        print(name, b, "ratio", g / chi if chi > 0 else 0.0, "niter", out["niter"][b])
        assert g <= tol["stationarity"] * chi, (name, b, g, chi)
        assert out["chisqr"][b] >= 0, (name, b)
        if c.kind == "b":            # (a kind (a) chi^2 is the rounding of exp and pow: two libraries do not agree on it)
            assert abs(out["chisqr"][b] - chi) <= 1e-9 * chi, (name, b, out["chisqr"][b], chi)
        assert out["redchi"][b] == out["chisqr"][b] / (s["y"].size - nv), (name, b)
        scale = max(abs(f["phasegrad"]), f["phasegraderr"])
        for k in cc.FIT_KEYS:
            if k == "alpha" and not vary:
                assert out[k][b] == c.kw.get("alpha", 5/3) and out["alphaerr"][b] == 0.0, (name, b)
                continue
            slot = "phasegrad" if k == "phasegrad" else "values"
            d = abs(out[k][b] - f[k]) / (scale if k == "phasegrad" else abs(f[k]))
            worst[slot] = max(worst[slot], d)
            print(name, b, k, out[k][b], f[k], d)
            assert d <= tol["phasegrad_tol" if k == "phasegrad" else "values_rtol"], (name, b, k, out[k][b], f[k])
        for k in cc.ERR_KEYS:
            if k == "alphaerr" and not vary:
                continue
            d = abs(out[k][b] - f[k]) / abs(f[k])
            worst["errors"] = max(worst["errors"], d)
            assert np.isfinite(out[k][b]) and d <= tol["errors_rtol"], (name, b, k, out[k][b], f[k])
        if c.planted is not None:
            for i, k in enumerate(cc.FIT_KEYS):
                if k == "alpha":
                    continue
                d = abs(out[k][b] - c.planted[b, i]) / abs(c.planted[b, i])
                worst["planted"] = max(worst["planted"], d)
                assert d <= tol["phasegrad_tol" if k == "phasegrad" else "values_rtol"], (name, b, k, out[k][b], c.planted[b, i])
    print(name, "kind", c.kind, "niter max", int(out["niter"].max()), "worst", worst, "allowed", tol)


def check_bad_window(sp):
    """FIT_BAD_WINDOW with NaN outputs between two good fits that keep their bits."""
    c = cc.case("badwin")
    out = run(sp, "badwin")
    assert list(out["status"]) == [CONVERGED, BAD_WINDOW, CONVERGED], out["status"]
    assert out["nfw"][1] % 2 == 0 or out["ntw"][1] % 2 == 0
    for k in cc.FIT_KEYS + cc.ERR_KEYS + ("chisqr", "redchi"):
        assert np.isnan(out[k][1]) and np.isfinite(out[k][[0, 2]]).all(), k
    alone = sp.acf2d_approx_fit_device(to_dev(sp, c.stack[[0, 2]]), c.dt, c.df, c.bw, c.tobs)
    assert same_bits(out, alone, rows=[0, 2])


def check_status_paths(sp):
    """An all-NaN and an all-zero ACF between good ones report their status with NaN outputs, the good ones keep their bits;
    max_iter=1 ends every problem at the cap; weighted=False zeroes nearly every weight: the fit is singular, as the
    reference's would be."""
    c = cc.case("real12")
    clean = run(sp, "real12")
    stack = np.concatenate([c.stack[:2], np.full_like(c.stack[:1], np.nan), c.stack[2:5], np.zeros_like(c.stack[:1]), c.stack[5:]])
    out = sp.acf2d_approx_fit_device(to_dev(sp, stack), c.dt, c.df, c.bw, c.tobs)
    good = np.array([0, 1, 3, 4, 5] + list(range(7, 14)))
    assert out["status"][2] == NONFINITE_INPUT and out["status"][6] == SINGULAR, out["status"]
    for b in (2, 6):
        for k in cc.FIT_KEYS + cc.ERR_KEYS + ("chisqr", "redchi"):
            assert np.isnan(out[k][b]), (b, k)
    assert same_bits(out, clean, rows=good)
    capped = run(sp, "real12", max_iter=1)
    assert np.all(capped["status"] == ITER_CAP) and np.all(capped["niter"] == 1)
    for k in cc.FIT_KEYS + cc.ERR_KEYS + ("chisqr", "redchi"):
        assert np.isnan(capped[k]).all(), k
    assert same_bits(capped, clean, keys=RECT + ("nnz", "argmax"))
    flat = run(sp, "real12", weighted=False, return_setup=True)
    for b, acf in enumerate(c.stack):
        s = ao.setup(acf, c.dt, c.df, c.bw, c.tobs, weighted=False)
        assert np.array_equal(flat["w"][b], s["w"]) and flat["nnz"][b] == np.count_nonzero(s["w"]) <= 2, (b, flat["nnz"][b])
    assert np.all(flat["status"] == SINGULAR), flat["status"]
    assert np.isnan(flat["tau"]).all()


def check_fixed_tau(sp):
    """tau_input with tau_vary_2d=False: tau stays, its error is 0, the other parameters agree with the oracle's fit of the rest."""
    c = cc.case("real12")
    tol = tolerances()["b"]
    out = run(sp, "real12", tau_input=120.0, tau_vary_2d=False)
    assert np.all(out["status"] == CONVERGED) and np.all(out["tau"] == 120.0) and np.all(out["tauerr"] == 0.0)
    for b in (0, 7):
        s = ao.setup(c.stack[b], c.dt, c.df, c.bw, c.tobs, tau_input=120.0)
        f = ao.fit(s, vary_tau=False)
        g, chi = ao.stationarity([out[k][b] for k in cc.FIT_KEYS], s, False, vary_tau=False)
        assert f["success"] and g <= tol["stationarity"] * chi, (b, g, chi)
        for k in ("dnu", "amp"):
            assert abs(out[k][b] - f[k]) <= tol["values_rtol"] * abs(f[k]), (b, k, out[k][b], f[k])
        assert abs(out["phasegrad"][b] - f["phasegrad"]) <= tol["phasegrad_tol"] * max(abs(f["phasegrad"]), f["phasegraderr"])
        assert out["redchi"][b] == out["chisqr"][b] / (s["y"].size - 3)


def check_deterministic(sp, name):
    assert same_bits(run(sp, name), run(sp, name))


def _dynspec(obs):
    from scintools_amd.dynspec import Dynspec
    return Dynspec(dyn=obs, verbose=False)


FIT_ATTRS = ("tau", "dnu", "tscat", "nscint", "fse_tau", "fse_dnu", "tauerr", "dnuerr", "amp", "amperr", "wn", "talpha", "talphaerr",
             "phasegrad", "phasegraderr", "fse_phasegrad")


def check_dynspec(sp, alpha):
    """Dynspec.fit_scint_params_2d on a kind (b) observation: every attribute against the oracle applied to the SAME (device) ACF;
    acf_model against the oracle's model at the fitted parameters."""
    o = cc.observation()
    d = _dynspec(o)
    d.fit_scint_params_2d(alpha=alpha)
    acf = d.acf
    tol = tolerances()["b"]
    s = ao.setup(acf, o.dt, o.df, o.bw, o.tobs, nsub=d.nsub, nchan=d.nchan, alpha=alpha)
    f = ao.fit(s, alpha=alpha)
    assert f["success"] and d.scint_fit_status == CONVERGED and d.scint_param_method == "acf2d_approx" and not hasattr(d, "report")
    want = ao.fit_attrs(f, o, alpha, name=d.name)
    scale = max(abs(f["phasegrad"]), f["phasegraderr"])
    for k in FIT_ATTRS:
        got = getattr(d, k)
        print("fit_scint_params_2d", k, got, want[k])
        if k in ("phasegrad", "fse_phasegrad"):
            assert abs(got - want[k]) <= tol["phasegrad_tol"] * scale, (k, got, want[k])
        elif want[k] == 0:
            assert got == 0, k
        else:
            rtol = tol["errors_rtol"] if "err" in k else tol["values_rtol"]
            assert abs(got - want[k]) <= rtol * abs(want[k]), (k, got, want[k])
    n = s["y"].size - (5 if alpha is None else 4)
    assert abs(d.scint_fit_redchi - f["chisqr"] / n) <= 1e-6 * f["chisqr"] / n and 1 <= d.scint_fit_niter <= 200
    assert type(d).acf_model.present(d) and d.__dict__["_devbacked_acf_model"][0] is None       # still on the device
    p = [getattr(d, "tau"), d.dnu, d.amp, d.talpha, d.phasegrad]
    model = -ao.model_residual(p, s["t"], s["f"], np.zeros(s["y"].shape), None, o.tobs, o.bw)
    assert d.acf_model.shape == model.shape and d.acf_model[model.shape[0] // 2, model.shape[1] // 2] == 0
    assert np.abs(d.acf_model - model).max() <= model_bound(p, s["t"], s["f"], 1.0, o.tobs, o.bw)


def check_dynspec_not_converged(sp, pytest):
    """A fit that cannot converge (a constant ACF has a zero start amplitude) warns and leaves the no-fit values."""
    o = cc.observation()
    d = _dynspec(o)
    d.acf = np.zeros((2 * o.dyn.shape[0], 2 * o.dyn.shape[1]))
    with pytest.warns(UserWarning, match="did not converge"):
        d.fit_scint_params_2d()
    assert d.scint_fit_status == SINGULAR and d.scint_param_method == "nofit" and np.isnan(d.scint_fit_redchi)
    assert (d.tau, d.dnu, d.amp) == (o.tobs, o.bw, 0.0) and not hasattr(d, "phasegrad")


def check_cut(sp):
    """fit_scint_params_2d_cut(1, 2) = six single fits of the six segments, bit for bit."""
    o = cc.observation(rng_seed=22, nf=96, nt=64)     # (segments of 32 channels: 16 MHz, more than nscale bandwidths)
    o.dyn = o.dyn - o.dyn.mean()      # cut_dyn's ACFs keep the mean; with one, no segment's ACF falls to half power (FIT_BAD_WINDOW)
    d = _dynspec(o)
    d.fit_scint_params_2d_cut(tcuts=1, fcuts=2)
    fnum, tnum = 32, 32
    assert d.cut_tau.shape == d.cut_fit_status.shape == d.cut_phasegrad.shape == (3, 2)
    for ii in range(3):
        for jj in range(2):
            seg = np.ascontiguousarray(o.dyn[ii * fnum:(ii + 1) * fnum, jj * tnum:(jj + 1) * tnum])
            acf = sp.acf_device(to_dev(sp, seg), subtract_mean=False)
            one = sp.acf2d_approx_fit_device(acf, o.dt, o.df, fnum * o.df, tnum * o.dt)
            for k in ("tau", "dnu", "amp", "phasegrad", "tauerr", "dnuerr", "amperr", "phasegraderr"):
                assert np.array_equal(getattr(d, "cut_" + k)[ii, jj], one[k][0], equal_nan=True), (ii, jj, k)
            assert d.cut_fit_status[ii, jj] == one["status"][0]
    print("fit_scint_params_2d_cut status", d.cut_fit_status.tolist())
    assert np.any(d.cut_fit_status == CONVERGED)


def model_bound(p, tdata, fdata, wmax, tobs, bw):
    """|device - host| allowed for a residual (y - model) w.  pow, exp and cbrt are each good to a few ulp on either side, so the
    exponent G = S^(2/3) carries a relative error of ~8 eps (3 alpha / 2 <= 3 times the 1-2 ulp of u, then pow and cbrt) and the
    model amp exp(-G) tri one of (8 G + 8) eps; G < 745 where the model is not zero.  The subtraction and the product add an ulp
    of |y| each, which 8 eps covers for |y| <= amp."""
    G = -np.log(np.maximum(np.abs(ao.model(p, tdata, fdata, tobs, bw)) / abs(p[2]), 1e-320))
    return float(((8 * G + 16) * EPS * abs(p[2])).max() * wmax)


def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "acf2d_approx.npz"))


GOLDEN_CASES = ("w3x3", "w21x31", "w19x5")


def golden_inputs(name):
    """Seeded inputs of a golden window `name` = w<nf>x<nt>: params, tdata, fdata, ydata, weights."""
    nf, nt = (int(v) for v in name[1:].split("x"))
    rng = np.random.default_rng(100 + nf * nt)
    tobs, bw = 1440.0, 16.0
    tdata = np.linspace(-tobs, tobs, 97)[:-1][48 - nt // 2:48 + nt // 2 + 1]
    fdata = np.linspace(-bw, bw, 65)[:-1][32 - nf // 2:32 + nf // 2 + 1]
    pars = dict(amp=0.85, dnu=1.3, tau=140.0, alpha=5/3 if nf != 19 else 1.8, phasegrad=0.4 if nf != 19 else -0.7, tobs=tobs,
                bw=bw, freq=1400.0)
    ydata = rng.normal(0.2, 0.3, size=(nf, nt))
    weights = rng.uniform(0.5, 12.0, size=(nf, nt))
    return pars, tdata, fdata, ydata, weights


def check_model(sp):
    """scint_models.scint_acf_model_2d_approx on the device against the reference's own output (tests/golden/acf2d_approx.npz)."""
    from scintools_amd import scint_models
    g = golden()
    for name in GOLDEN_CASES:
        pars, tdata, fdata, ydata, weights = golden_inputs(name)
        p = [pars[k] for k in cc.FIT_KEYS]
        for tag, w in (("w", weights), ("n", None)):
            got = scint_models.scint_acf_model_2d_approx(pars, tdata, fdata, ydata, None if w is None else w.copy())
            want = g[f"{name}_{tag}"]
            bound = model_bound(p, tdata, fdata, 12.0 if w is not None else 1.0, pars["tobs"], pars["bw"]) + \
                8 * EPS * np.abs(ydata).max() * (12.0 if w is not None else 1.0)
            assert got.shape == want.shape and got[(got.shape[0] - 1) // 2, (got.shape[1] - 1) // 2] == 0
            assert np.abs(got - want).max() <= bound, (name, tag, np.abs(got - want).max(), bound)


def check_arguments(sp, pytest):
    from scintools_amd import _lib
    c = cc.case("tiny")
    with pytest.raises(_lib.ScintHipError, match="max_iter"):
        run(sp, "tiny", max_iter=0)
    with pytest.raises(_lib.ScintHipError, match="bad shape"):
        sp.acf2d_approx_fit_device(to_dev(sp, np.ones((1, 4, 16))), c.dt, c.df, c.bw, c.tobs)
    with pytest.raises(_lib.ScintHipError, match="nsub"):
        run(sp, "tiny", nsub=0)
    with pytest.raises(ValueError, match="stack of ACFs"):
        sp.acf2d_approx_fit_device(to_dev(sp, np.ones((1, 1, 16, 16))), c.dt, c.df, c.bw, c.tobs)
