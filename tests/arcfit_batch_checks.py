"""Checks of the batched arc fit -- scint_arc_profile_batch, scint_arc_peak_fit, arcfit.fit_arc_stack_device, Dynspec.fit_arc_cut --
shared by the GPU tests (tests/test_gpu_arcfit_batch.py) and the host-interpreted ones (tests/test_arcfit_batch_emu_cpu.py).  `af` is
scintools_amd.arcfit.  The cases, and why these shapes: tests/arcfit_batch_cases.py.

The yardstick of the profile kernel is the chain of single calls (scint_norm_sspec, scint_masked_colavg, scint_block_std) on problem b
alone: the same BITS.  The yardstick of the peak fit's decisions is arcfit._arc_peak, the function fit_arc itself calls; of its
values the same least-squares parabola solved in np.longdouble, to the tolerances of tests/golden/arcfit_batch_tolerances.json
(made by tests/golden/make_arcfit_batch_tolerances.py on the host alone)."""
import ctypes
import json
import os

import numpy as np

import arcfit_batch_cases as cc

SCINT_E_ARG, SCINT_E_WORKSPACE = 1, 3
EPS = np.finfo(float).eps
HERE = os.path.dirname(os.path.abspath(__file__))
TOL_PATH = os.path.join(HERE, "golden", "arcfit_batch_tolerances.json")
MAX_EXCLUDED = 0.01                 # of all profiles, over the whole case list


def to_dev(af, a, dtype=None):
    import torch
    return af.to_device(a, dtype or torch.float64)


def raw(t):
    a = np.ascontiguousarray(t.cpu().numpy())
    return a.view(np.uint64) if a.dtype == np.float64 else a


def tolerances():
    with open(TOL_PATH) as fh:
        return json.load(fh)


# ---- the profile kernel ----------------------------------------------------------------------------------------------------------------
def batch_profiles(af, c, stack=None):
    import torch
    st = to_dev(af, c.stack if stack is None else stack)
    return af.arc_profile_stack_device(st, to_dev(af, c.fdop), to_dev(af, c.yaxis), c.row0, c.nr, c.eta, c.maxnormfac, c.cut_lo,
                                       c.cut_hi, c.noise_lo, c.noise_hi, to_dev(af, c.x))


def single_profile(af, c, spec):
    """The three existing entry points on one spectrum [R, nc], as norm_sspec and fit_arc call them."""
    import torch
    sp = to_dev(af, spec)
    fd, ya, x = to_dev(af, c.fdop), to_dev(af, c.yaxis), to_dev(af, c.x)
    norm = af.empty((c.nr, c.nx), torch.float64)
    mask = af.empty((c.nr, c.nx), torch.uint8)
    pw = af.empty((c.nr,), torch.float64)
    af._lib.call("scint_norm_sspec", sp, c.nc, c.nc, fd, ya, c.row0, c.nr, c.eta, c.maxnormfac, c.cut_lo, c.cut_hi, None, x, None,
                 c.nx, norm, mask, pw, af.stream_ptr())
    ws = af.workspace_for("scint_masked_colavg", c.nr, c.nx)
    avg = af.empty((c.nx,), torch.float64)
    none = af.empty((c.nx,), torch.uint8)
    af._lib.call("scint_masked_colavg", norm, mask, c.nr, c.nx, to_dev(af, np.ones(c.nr)), None, avg, none, ws, ws.numel(),
                 af.stream_ptr())
    avg, none = raw(avg), raw(none)                        # (before the workspace is handed to the next call)
    std = af.empty((1,), torch.float64)
    ws = af.workspace.get(8 * 1032)
    af._lib.call("scint_block_std", sp, c.nc, c.nc, c.R // 2, c.R, c.noise_lo, c.noise_hi, std, ws, ws.numel(), af.stream_ptr())
    return avg, none, raw(std)[0]


def check_bits_of_the_single_calls(af, name):
    c = cc.case(name)
    avg, none, noise = (raw(t) for t in batch_profiles(af, c))
    assert avg.shape == (c.B, c.nx) and none.shape == (c.B, c.nx) and noise.shape == (c.B,)
    for b in range(c.B):
        a1, n1, s1 = single_profile(af, c, c.stack[b])
        assert np.array_equal(avg[b], a1), (name, b, int((avg[b] != a1).sum()))
        assert np.array_equal(none[b], n1), (name, b)
        assert noise[b] == s1, (name, b)
    if name == "empty":
        assert none[:, 0].all() and none[:, -1].all() and not none[:, int(0.62 * c.nx)].any()       # x = -1, 1, 0.24
        assert not avg[:, 0].any()                          # 0.0 under the mask
    if name == "norows":
        import torch
        # the first rows select nothing: the single call masks them entirely
        norm = af.empty((c.nr, c.nx), torch.float64)
        mask = af.empty((c.nr, c.nx), torch.uint8)
        af._lib.call("scint_norm_sspec", to_dev(af, c.stack[0]), c.nc, c.nc, to_dev(af, c.fdop), to_dev(af, c.yaxis), c.row0, c.nr,
                     c.eta, c.maxnormfac, c.cut_lo, c.cut_hi, None, to_dev(af, c.x), None, c.nx, norm, mask,
                     af.empty((c.nr,), torch.float64), af.stream_ptr())
        m = mask.cpu().numpy()
        assert m[:2].all() and not m[2:].all(axis=1).any()


def check_leak(af):
    """A problem that is all NaN, or 10^6 times brighter (+60 dB), between two others: these keep the bits they have alone."""
    c = cc.case("r33")
    for middle in (np.full((c.R, c.nc), np.nan), c.stack[0] + 60.0):
        stack = np.ascontiguousarray(np.stack([c.stack[0], middle, c.stack[1]]))
        got = [raw(t) for t in batch_profiles(af, c, stack)]
        for k, b in ((0, 0), (2, 1)):
            alone = [raw(t) for t in batch_profiles(af, c, c.stack[b:b + 1])]
            for g, a in zip(got, alone):
                assert np.array_equal(g[k], a[0]), (k, b)


def check_deterministic(af, name):
    c = cc.case(name)
    one = [raw(t) for t in batch_profiles(af, c)]
    two = [raw(t) for t in batch_profiles(af, c)]
    rev = [raw(t) for t in batch_profiles(af, c, np.ascontiguousarray(c.stack[::-1]))]
    for a, b, r in zip(one, two, rev):
        assert np.array_equal(a, b) and np.array_equal(a, r[::-1]), name


# ---- the peak fit: the oracle ---------------------------------------------------------------------------------------------------------
PEAK_DEFAULTS = dict(constraint=(0, np.inf), nsmooth=5, low_power_diff=-1, high_power_diff=-0.5, noise_error=True,
                     log_parabola=False)


def fold(avg, side):
    half = len(avg) // 2
    pos, neg = avg[half:], np.flip(avg[:half])
    return (pos + neg) / 2 if side < 0 else (pos if side == 0 else neg)


def kept_points(af, spec, x, etamin, etamax):
    """(spec, eta) as fit_arc keeps them (dynspec.py:1197-1206)."""
    half = len(x) // 2
    ok = af.is_valid(spec)
    s = np.flip(spec[ok])
    e = etamin * np.flip((1 / x[half:])[ok])**2
    keep = e < etamax
    return s[keep], e[keep]


def oracle(af, avg, x, noise, etamin, etamax, side=-1, **kw):
    """dict(status, kept, pk, i1, i2, eta, etaerr, etaerr2, margin, xdata, ydata) of one profile from arcfit._arc_peak, its
    exceptions mapped to the statuses of scint_arc_peak_fit; `margin` is the oracle's own smallest distance to a decision."""
    par = dict(PEAK_DEFAULTS, **kw)
    half = len(x) // 2
    spec = fold(avg, side)
    s, e = kept_points(af, spec, x, etamin, etamax)
    out = dict(status=0, kept=len(s), spec=s, pk=-1, i1=-1, i2=-1, eta=np.nan, etaerr=np.nan, etaerr2=np.nan, margin=np.inf, scale=0.0)
    if len(s) < max(par["nsmooth"], 4):
        out["status"] = 1
        return out
    out["scale"] = float(np.max(np.abs(s)))
    try:
        with np.errstate(all="ignore"):
            pk = af._arc_peak(spec, 1 / x[half:], etamin, etamax, noise=noise, strict=True, **par)
    except af.ArcWindowError as err:
        out.update(status=3, pk=err.pk, i1=err.i1, i2=err.i2)
    except ValueError as err:
        if "zero-size" in str(err):
            out["status"] = 2
            return out
        if "forward parabola" not in str(err):
            raise
        out.update(status=4, pk=err.pk, i1=err.i1, i2=err.i2)
    else:
        out.update(pk=pk.pk, i1=pk.i1, i2=pk.i2, eta=float(pk.eta), etaerr=float(pk.etaerr) / np.sqrt(2),
                   etaerr2=float(pk.etaerr2) / np.sqrt(2))
        out["xdata"], out["ydata"] = e[pk.pk - pk.i1:pk.pk + pk.i2], s[pk.pk - pk.i1:pk.pk + pk.i2]
        if not (np.isfinite(out["eta"]) and np.isfinite(out["etaerr"]) and np.isfinite(out["etaerr2"])):
            out.update(status=5, eta=np.nan, etaerr=np.nan, etaerr2=np.nan)
    out["margin"] = _margin(af, s, e, noise, par, out)
    return out


def _margin(af, s, e, noise, par, out):
    """The oracle's smallest |smooth[j] - threshold| along its walks and the gap between the two largest distinct smoothed values
    inside the constraint (equal values tie in the kernel as in the oracle: each smooths the same points in the same way)."""
    from scipy.signal import savgol_filter
    smooth = savgol_filter(s, par["nsmooth"], 1)
    inside = smooth[(e > par["constraint"][0]) * (e < par["constraint"][1])]
    vals = np.unique(inside)
    margin = vals[-1] - vals[-2] if len(vals) > 1 else np.inf
    pk = int(np.argmin(np.abs(smooth - inside.max())))
    top, n = smooth[pk], len(smooth)
    walks = [(-1, top + par["low_power_diff"]), (1, top + par["high_power_diff"])]
    if par["noise_error"] and out["status"] == 0:
        walks += [(-1, top - noise), (1, top - noise)]
    for step, thr in walks:
        j = pk + step
        while 0 <= j < n:
            margin = min(margin, abs(smooth[j] - thr))
            if not smooth[j] > thr:
                break
            j += step
    return float(margin)


def truth(xdata, ydata, log_parabola):
    """(eta, etaerr2) of fit_parabola / fit_log_parabola on these points in np.longdouble: the same scaling, the abscissa centred,
    the parabola through an orthogonal basis; both errors divided by sqrt 2 as the attributes are."""
    ld = np.longdouble
    x, y = np.asarray(xdata, dtype=ld), np.asarray(ydata, dtype=ld)
    ptp1 = None
    if log_parabola:
        x = np.log(x)
        ptp1 = np.ptp(x)
        x = x * (ld(1000) / ptp1)
    ptp = np.ptp(x)
    xs = x * (ld(1000) / ptp)
    mean = xs.mean()
    u = xs - mean
    p1 = u - u.mean()
    q = u * u - (u * u).mean()
    r12 = (p1 * q).sum() / (p1 * p1).sum()
    p2 = q - r12 * p1
    n1, n2 = (p1 * p1).sum(), (p2 * p2).sum()
    d0, d1, d2 = y.mean(), (y * p1).sum() / n1, (y * p2).sum() / n2
    var = ((y - (d0 + d1 * p1 + d2 * p2))**2).sum() / ld(len(y) - 3)
    a = d2
    b = (d1 - d2 * r12) - 2 * a * mean                      # params[1] in xs; d1 and d2 are independent
    va, vb = var / n2, var / n1 + var / n2 * (r12 + 2 * mean)**2
    peak = -b / (2 * a)
    perr = np.sqrt(vb * (1 / (2 * a))**2 + va * (b / 2)**2)
    peak, perr = peak * (ptp / 1000), perr * (ptp / 1000)
    if log_parabola:
        frac = perr / peak
        peak = np.exp(peak * ptp1 / 1000)
        perr = frac * peak
    return float(peak), float(perr / np.sqrt(ld(2)))


def run_peak_fit(af, avg, x, noise, noise_div, etamin, etamax, asymm=False, **kw):
    par = dict(PEAK_DEFAULTS, **kw)
    prof, val, dec = af.arc_peak_fit_device(to_dev(af, np.atleast_2d(avg)), to_dev(af, np.atleast_1d(noise)), noise_div,
                                            to_dev(af, x), etamin, etamax, asymm=asymm, **par)
    return prof.cpu().numpy(), val.cpu().numpy(), dec.cpu().numpy()


def compare_profile(af, got_val, got_dec, got_prof, k, ref, kind, tol, log_parabola, stats):
    """Decisions equal to the oracle's (unless its own margin is below 64 eps max|spec|: counted), values within `tol` of the truth."""
    pk, i1, i2, kept, status = (int(v) for v in got_dec[:, k])
    stats["profiles"] += 1
    assert kept == ref["kept"], (kind, k, kept, ref["kept"])
    if ref["margin"] < 64 * EPS * ref["scale"]:
        stats["excluded"] += 1
        return
    assert status == ref["status"], (kind, k, status, ref["status"])
    if status != 0:
        assert np.isnan(got_val[:3, k]).all(), (kind, k)
    if status in (3, 4, 5):
        # the peak, and the high-side walk, which reads nothing below the peak; status 3 may end the low-side walk at the first
        # index below zero, where the reference wraps and walks on: its i1 is compared only where the window stays inside
        assert (pk, i2) == (ref["pk"], ref["i2"]), (kind, k, (pk, i2), (ref["pk"], ref["i2"]))
        if status != 3 or ref["pk"] - ref["i1"] >= 0:
            assert i1 == ref["i1"], (kind, k, i1, ref["i1"])
    if status != 0:
        return
    assert (pk, i1, i2) == (ref["pk"], ref["i1"], ref["i2"]), (kind, k, (pk, i1, i2), (ref["pk"], ref["i1"], ref["i2"]))
    assert np.array_equal(got_prof[k, :kept], ref["spec"]) and np.isnan(got_prof[k, kept:]).all(), (kind, k)
    eta_t, err2_t = truth(ref["xdata"], ref["ydata"], log_parabola)
    eta, etaerr, etaerr2 = got_val[:3, k]
    d_eta, d_err = abs(eta - eta_t) / abs(eta_t), abs(etaerr2 - err2_t) / abs(err2_t)
    h_eta, h_err = abs(ref["eta"] - eta_t) / abs(eta_t), abs(ref["etaerr2"] - err2_t) / abs(err2_t)
    print(f"{kind}[{k}]: eta {eta:.6g} |rel dev| {d_eta:.2e} (allowed {tol['peak']:.2e}), etaerr2 {etaerr2:.4g} |rel dev| {d_err:.2e} "
          f"(allowed {tol['error']:.2e}); host float64: {h_eta:.2e}, {h_err:.2e}")
    assert d_eta <= tol["peak"], (kind, k, d_eta, tol["peak"])
    assert d_err <= tol["error"], (kind, k, d_err, tol["error"])
    # with noise_error etaerr is a difference of two curvatures at the oracle's indices
    assert abs(etaerr - ref["etaerr"]) <= 4 * EPS * abs(ref["etaerr"]), (kind, k, etaerr, ref["etaerr"])


def check_peak_bumps(af, log_parabola, asymm, stats):
    """The seeded bumps: decisions and values, symmetric and per side, plain and in log."""
    kind = "log_parabola" if log_parabola else "plain"
    tol = tolerances()[kind]
    avg, x = cc.bump_profiles(), cc.peak_x()
    noise, div = 0.6, 3.0
    prof, val, dec = run_peak_fit(af, avg, x, np.full(len(avg), noise), div, cc.PEAK_ETAMIN, cc.PEAK_ETAMAX, asymm=asymm,
                                  log_parabola=log_parabola)
    assert np.array_equal(val[3], np.full(val.shape[1], noise / div))
    for k in range(val.shape[1]):
        p, side = (k // 2, k % 2) if asymm else (k, -1)
        ref = oracle(af, avg[p], x, noise / div, cc.PEAK_ETAMIN, cc.PEAK_ETAMAX, side=side, log_parabola=log_parabola)
        assert ref["status"] == 0, (kind, k, ref["status"])
        compare_profile(af, val, dec, prof, k, ref, kind, tol, log_parabola, stats)


def check_peak_synthetic(af, stats):
    """Every status, and the flat top where the first maximum wins."""
    tol = tolerances()["plain"]
    x = cc.peak_x()
    for name, (avg, kw, expect) in cc.synthetic_profiles().items():
        ref = oracle(af, avg, x, 0.1, cc.PEAK_ETAMIN, cc.PEAK_ETAMAX, **kw)
        assert ref["status"] == expect, (name, ref["status"], expect)
        prof, val, dec = run_peak_fit(af, avg, x, 0.1, 1.0, cc.PEAK_ETAMIN, cc.PEAK_ETAMAX, **kw)
        assert int(dec[4, 0]) == expect, (name, int(dec[4, 0]), expect)
        if name == "flat":
            s, e = kept_points(af, fold(avg, -1), x, cc.PEAK_ETAMIN, cc.PEAK_ETAMAX)
            from scipy.signal import savgol_filter
            sm = savgol_filter(s, 5, 1)
            assert (sm == sm.max()).sum() > 1 and int(dec[0, 0]) == int(np.argmax(sm == sm.max()))
        compare_profile(af, val, dec, prof, 0, ref, name, tol, False, stats)


def check_peak_on_case(af, name, stats):
    """Profiles the profile kernel made from a case's stack, through the peak fit: the decisions of the oracle on the same numbers."""
    c = cc.case(name)
    avg_t, none_t, noise_t = batch_profiles(af, c)
    avg, noise = avg_t.cpu().numpy(), noise_t.cpu().numpy()
    etamin, etamax, div = c.eta, c.eta * 400.0, float(np.sqrt(2 * c.R))
    tol = tolerances()["plain"]
    # the peak is sought where every case has data: `empty` has none below 4 etamin (|x| > 0.5), only the 0.0 of an empty column
    con = (4.2 * c.eta, np.inf)
    prof, val, dec = run_peak_fit(af, avg, c.x, noise, div, etamin, etamax, constraint=con)
    assert np.array_equal(val[3], noise / div, equal_nan=True)
    for b in range(c.B):
        ref = oracle(af, avg[b], c.x, noise[b] / div, etamin, etamax, constraint=con)
        compare_profile(af, val, dec, prof, b, ref, name, tol, False, stats)


def check_excluded(stats):
    print(f"peak-fit decisions: {stats['excluded']} of {stats['profiles']} profiles excluded by the oracle's own margin")
    assert stats["profiles"] > 0 and stats["excluded"] <= MAX_EXCLUDED * stats["profiles"], stats


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def arc_dynspec(nf=64, nt=96, seed=17):
    """A small observation with an arc (scintools_amd.synth) as a Dynspec.  The seed is the first from 11 on for which fit_arc
    succeeds plain, per side and in log AND its own float64 values lie within the tolerances of the long-double parabola through its
    own points (check_end_to_end asserts that): 11, 12, 14 and 16 raise in the reference, on 13 and 15 np.polyfit itself is further from the
    truth than the tolerance, so no comparison with it at that tolerance says anything about the other side."""
    from scintools_amd.dynspec import Dynspec
    from scintools_amd.synth import arc_dynspec as synth
    import scintpar_cases
    dyn, freqs, times, _ = synth(nf, nt, seed=seed, nimg=16)
    df, dt = float(freqs[1] - freqs[0]), float(times[1] - times[0])
    obs = scintpar_cases.observation(np.ascontiguousarray(dyn), freqs, times, df, dt, float(np.mean(freqs)), "arcfit_batch")
    return Dynspec(dyn=obs, verbose=False)


def check_end_to_end(af, asymm, log_parabola):
    """B = 1 against Dynspec.fit_arc(lamsteps=True) with explicit bounds: values to the tolerances of the peak fit, noise bit-equal."""
    from scintools_amd.dynspec import Dynspec
    kind = "log_parabola" if log_parabola else "plain"
    tol = tolerances()[kind]
    d = arc_dynspec()
    d.calc_sspec(lamsteps=True)
    fdop, beta = np.asarray(d.fdop, dtype=float), np.asarray(d.beta, dtype=float)
    etamin = (beta[1] - beta[0]) * 3 / np.max(fdop)**2
    etamax = beta[-1] / ((fdop[1] - fdop[0]) * 3)**2 / 4
    kw = dict(etamin=etamin, etamax=etamax, numsteps=600, asymm=asymm, log_parabola=log_parabola)
    d.fit_arc(lamsteps=True, **kw)
    st = Dynspec.lamsspec.tensor(d)
    fit = af.fit_arc_stack_device(st[None].contiguous(), fdop, beta, **kw)
    assert fit["noise"].shape == (1,) and fit["noise"][0] == d.noise
    assert not fit["status"].any()
    sides = ("_left", "_right") if asymm else ("",)
    x, avg = np.ravel(d.normsspec_fdop), np.array(d.normsspecavg)
    for i, side in enumerate(sides):
        # the reference's own values against the truth of its points: what makes it a yardstick at this tolerance (host values only)
        ref = oracle(af, avg, x, d.noise, etamin, etamax, side=(i if asymm else -1), log_parabola=log_parabola)
        eta_t, err2_t = truth(ref["xdata"], ref["ydata"], log_parabola)
        assert ref["eta"] == getattr(d, "betaeta" + side)
        assert abs(ref["eta"] - eta_t) <= tol["peak"] * abs(eta_t) and abs(ref["etaerr2"] - err2_t) <= tol["error"] * abs(err2_t)
        for key, attr, t in (("eta", "betaeta", tol["peak"]), ("etaerr2", "betaetaerr2", tol["error"])):
            got = fit[key][0, i] if asymm else fit[key][0]
            want = getattr(d, attr + side)
            print(f"{kind} asymm={asymm} {attr + side}: stack {got:.10g}, fit_arc {want:.10g}, |rel| {abs(got - want) / abs(want):.2e}")
            assert abs(got - want) <= t * abs(want), (attr + side, got, want)
        got = fit["etaerr"][0, i] if asymm else fit["etaerr"][0]
        want = getattr(d, "betaetaerr" + side)
        assert abs(got - want) <= 4 * EPS * abs(want), ("betaetaerr" + side, got, want)
    assert np.array_equal(fit["eta_array"], d.eta_array)


def check_fit_arc_cut(af, monkeypatch, pytest):
    import torch
    from scintools_amd import scintpar
    from scintools_amd.dynspec import Dynspec
    import warnings
    d = arc_dynspec()
    calls = []
    real = scintpar.cut_dyn
    monkeypatch.setattr(Dynspec, "cut_dyn", lambda self, **kw: (calls.append(kw), real(self, **kw))[1])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        d.fit_arc_cut(tcuts=2, fcuts=1, numsteps=400)
    assert calls == [dict(tcuts=2, fcuts=1)]
    assert isinstance(d.cut_arc_profile, torch.Tensor) and tuple(d.cut_arc_profile.shape[:2]) == (2, 3)
    assert Dynspec.cutsspec.on_device(d)                    # not copied to the host
    for attr in ("cut_eta", "cut_etaerr", "cut_etaerr2", "cut_arc_status", "cut_arc_noise"):
        assert getattr(d, attr).shape == (2, 3), attr
    st = Dynspec.cutsspec.tensor(d)
    nr, ncol = int(st.shape[2]), int(st.shape[3])
    fdop, tdel, sec = d.calc_sspec(input_dyn=d.cutdyn[0, 0])         # a segment's axes as calc_sspec returns them
    assert sec.shape == (nr, ncol) and np.array_equal(sec, d.cutsspec[0, 0])
    st = Dynspec.cutsspec.tensor(d)
    fit = af.fit_arc_stack_device(st.view(6, nr, ncol), fdop, tdel, numsteps=400)
    same = lambda a, b: np.array_equal(a, b, equal_nan=True)
    assert same(d.cut_eta, fit["eta"].reshape(2, 3)) and same(d.cut_etaerr, fit["etaerr"].reshape(2, 3))
    assert same(d.cut_etaerr2, fit["etaerr2"].reshape(2, 3)) and same(d.cut_arc_status, fit["status"].reshape(2, 3))
    assert same(d.cut_arc_noise, fit["noise"].reshape(2, 3)) and same(d.cut_eta_array, fit["eta_array"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        d.fit_arc_cut(tcuts=2, fcuts=1, numsteps=400, asymm=True)
    assert len(calls) == 1                                  # the same cut: cut_dyn is not run again
    assert d.cut_eta.shape == (2, 3, 2) and d.cut_arc_noise.shape == (2, 3)
    # no curvature inside the constraint: every fit ends in status 2, one warning with the count, NaN in the values
    with pytest.warns(UserWarning, match="4 of 4 arc fits") as rec:
        d.fit_arc_cut(tcuts=1, fcuts=1, numsteps=400, constraint=(1e30, 2e30), out_device=False)
    assert len([w for w in rec if "fit_arc_cut" in str(w.message)]) == 1
    assert len(calls) == 2 and d.cut_eta.shape == (2, 2) and np.isnan(d.cut_eta).all() and (d.cut_arc_status == 2).all()
    assert isinstance(d.cut_arc_profile, np.ndarray) and d.cut_arc_profile.shape[:2] == (2, 2)


# ---- arguments -------------------------------------------------------------------------------------------------------------------------
def check_arguments(af, pytest):
    import torch
    c = cc.case("r31")
    st = to_dev(af, c.stack)
    ok = dict(etamin=c.eta, etamax=400 * c.eta, numsteps=200)
    with pytest.raises(ValueError, match="65535"):
        af.fit_arc_stack_device(st[:0], c.fdop, c.yaxis, **ok)
    with pytest.raises(ValueError, match="65535"):
        af.fit_arc_stack_device(torch.empty((65536, 2, 2), dtype=torch.float64, device=st.device), c.fdop[:2], c.yaxis[:2], **ok)
    with pytest.raises(ValueError, match="ascending"):
        af.fit_arc_stack_device(st, c.fdop[::-1], c.yaxis, **ok)
    with pytest.raises(ValueError, match="nsmooth"):
        af.fit_arc_stack_device(st, c.fdop, c.yaxis, nsmooth=4, **ok)
    with pytest.raises(ValueError, match="cutmid"):
        af.fit_arc_stack_device(st, c.fdop, c.yaxis, cutmid=0, etamin=c.eta)
    for kw in (dict(weighted=True), dict(subtract_artefacts=True), dict(fit_spectrum=True), dict(etamin=[c.eta, 2 * c.eta]),
               dict(etamax=[300 * c.eta, 400 * c.eta])):
        with pytest.raises(NotImplementedError):
            af.fit_arc_stack_device(st, c.fdop, c.yaxis, **dict(ok, **kw))
    fit = af.fit_arc_stack_device(st, c.fdop, c.yaxis, out_device=True, **ok)
    assert isinstance(fit["profile"], torch.Tensor) and fit["eta"].shape == (c.B,)


def check_c_status(af):
    """The entry points themselves: SCINT_E_ARG for B = 0, B = 65536, an even nsmooth and null pointers, SCINT_E_WORKSPACE for a
    workspace one byte short; nothing is launched: the outputs keep what they held."""
    import torch
    lib = af._lib.load()
    c = cc.case("r31")
    ptr = lambda t: None if t is None else t.data_ptr()
    st, fd, ya, x = to_dev(af, c.stack), to_dev(af, c.fdop), to_dev(af, c.yaxis), to_dev(af, c.x)
    avg = af.empty((c.B, c.nx), torch.float64)
    none = af.empty((c.B, c.nx), torch.uint8)
    noise = af.empty((c.B,), torch.float64)
    avg.fill_(-7.0), none.fill_(9), noise.fill_(-7.0)
    need = ctypes.c_size_t()
    assert lib.scint_arc_profile_batch_workspace_bytes(c.B, c.R, c.nc, c.nr, ctypes.byref(need)) == 0
    assert lib.scint_arc_profile_batch_workspace_bytes(0, c.R, c.nc, c.nr, ctypes.byref(need)) == SCINT_E_ARG
    assert lib.scint_arc_profile_batch_workspace_bytes(65536, c.R, c.nc, c.nr, ctypes.byref(need)) == SCINT_E_ARG
    assert lib.scint_arc_profile_batch_workspace_bytes(c.B, c.R, c.nc, c.nr, None) == SCINT_E_ARG
    ws = af.empty((need.value,), torch.uint8)

    def profile(B=c.B, sspec=st, out=avg, wsb=need.value):
        return lib.scint_arc_profile_batch(ptr(sspec), B, c.R, c.nc, c.nc, ptr(fd), ptr(ya), c.row0, c.nr, c.eta, 1.0, c.cut_lo, c.cut_hi,
                                           c.noise_lo, c.noise_hi, ptr(x), c.nx, ptr(out), ptr(none), ptr(noise), ptr(ws), wsb, None)
    assert profile(B=0) == SCINT_E_ARG and profile(B=65536) == SCINT_E_ARG
    assert profile(sspec=None) == SCINT_E_ARG and profile(out=None) == SCINT_E_ARG
    assert profile(wsb=need.value - 1) == SCINT_E_WORKSPACE
    assert (avg.cpu().numpy() == -7.0).all() and (none.cpu().numpy() == 9).all() and (noise.cpu().numpy() == -7.0).all()
    assert profile() == 0
    assert np.array_equal(raw(avg), raw(batch_profiles(af, c)[0]))

    from scipy.signal import savgol_coeffs
    coef = to_dev(af, savgol_coeffs(5, 1))
    con = (ctypes.c_double * 2)(0.0, np.inf)
    half = c.nx // 2
    prof = af.empty((c.B, half), torch.float64)
    val = af.empty((4, c.B), torch.float64)
    dec = af.empty((5, c.B), torch.int32)
    val.fill_(-7.0), dec.fill_(-7)
    assert lib.scint_arc_peak_fit_workspace_bytes(c.B, c.nx, 0, ctypes.byref(need)) == 0
    assert lib.scint_arc_peak_fit_workspace_bytes(0, c.nx, 0, ctypes.byref(need)) == SCINT_E_ARG
    assert lib.scint_arc_peak_fit_workspace_bytes(c.B, c.nx + 1, 0, ctypes.byref(need)) == SCINT_E_ARG
    assert lib.scint_arc_peak_fit_workspace_bytes(c.B, c.nx, 0, ctypes.byref(need)) == 0
    ws2 = af.empty((need.value,), torch.uint8)

    def peak(P=c.B, a=avg, nsmooth=5, constraint=con, wsb=need.value):
        return lib.scint_arc_peak_fit(ptr(a), P, c.nx, ptr(noise), 1.0, ptr(x), c.eta, 400 * c.eta, constraint, nsmooth, ptr(coef), -1.0,
                                      -0.5, 1, 0, 0, ptr(prof), ptr(val), ptr(dec), ptr(ws2), wsb, None)
    assert peak(P=0) == SCINT_E_ARG and peak(a=None) == SCINT_E_ARG and peak(constraint=None) == SCINT_E_ARG
    assert peak(nsmooth=4) == SCINT_E_ARG and peak(nsmooth=1) == SCINT_E_ARG
    assert peak(wsb=need.value - 1) == SCINT_E_WORKSPACE
    assert (val.cpu().numpy() == -7.0).all() and (dec.cpu().numpy() == -7).all()
    assert peak() == 0
    assert set(np.unique(dec.cpu().numpy()[4])) <= {0, 1, 2, 3, 4, 5}
