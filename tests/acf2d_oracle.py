"""CPU oracle of the approximate 2-D ACF fit (scint_acf2d_approx_fit, Dynspec.fit_scint_params_2d) -- TEST INFRASTRUCTURE.

A NumPy restatement of what the reference's ``get_scint_params(method='acf2d_approx')`` does between its 1-D fit and its call of
lmfit: the window centred on the ACF's maximum (dynspec.py:2733-2783), the weights (dynspec.py:2716-2731, 2785-2789) and the
residual (scint_models.py:123-161).  lmfit is replaced by ``scipy.optimize.least_squares`` at tight tolerances on the SAME
least-squares problem, in (log tau, log dnu, log amp, phasegrad[, alpha]); the standard errors are
``sqrt(diag((J^T J)^-1 chi^2 / (N - nvary)))`` in the external parameters, N every point of the window.  The start values are
those of the 1-D oracle (tests/acf1d_oracle.py) unless given.  ``fit_attrs`` restates dynspec.py:2953-3021."""
import numpy as np
from scipy.optimize import least_squares

import acf1d_oracle as ao1

ALPHA0 = 5/3
NAMES = ("tau", "dnu", "amp", "alpha", "phasegrad")


class BadWindow(Exception):
    """The reference's window has an even or empty side: its double fftshift does not put the spike where the model zeroes it."""


def setup(acf, dt, df, bw, tobs, nsub=None, nchan=None, nscale=5, full_frame=False, weighted=True, bartlett=True, alpha=5/3,
          phasegrad0=0.0, tau_input=None, start=None):
    """Window, ticks, weights and start values of one ACF, statement for statement.  `start`: (tau, dnu, amp) in place of the 1-D
    oracle's fit (the no-fit values where that did not converge)."""
    acf = np.asarray(acf)
    nf, nt = np.shape(acf)
    nsub = nt // 2 if nsub is None else nsub
    nchan = nf // 2 if nchan is None else nchan
    s1 = ao1.setup(acf, dt, df, bw, tobs, nscale=nscale, full_frame=full_frame, weighted=weighted, bartlett=bartlett)
    tau, dnu = s1["tau"], s1["dnu"]            # the reference's locals: the no-fit values, whatever the 1-D fit found
    if start is None:
        f1 = ao1.fit(s1, alpha=alpha)
        start = (f1["tau"], f1["dnu"], f1["amp"]) if f1["success"] else (s1["tau"], s1["dnu"], s1["amp"])
    p0 = dict(tau=start[0] if tau_input is None else tau_input, dnu=start[1], amp=start[2],
              alpha=ALPHA0 if alpha is None else alpha, phasegrad=phasegrad0)

    tticks = np.linspace(-tobs, tobs, nt + 1)[:-1]
    fticks = np.linspace(-bw, bw, nf + 1)[:-1]

    T, F = np.meshgrid(tobs - abs(tticks), bw - abs(fticks))
    # Create weights array
    with np.errstate(divide="ignore", invalid="ignore"):
        N2d = nsub * nchan * (T/max(tticks)) * (F/max(fticks))
        errors_2d = 1/np.sqrt(N2d)
    errors_2d[~(np.isfinite(errors_2d)*(~np.isnan(errors_2d)))] = np.inf

    weights_2d = np.ones(np.shape(acf))
    if weighted:
        weights_2d = weights_2d / errors_2d

    wn_loc = np.unravel_index(np.argmax(acf, axis=None), acf.shape)

    fleft = wn_loc[0]
    fright = nf - wn_loc[0] - 1
    fmin = wn_loc[0] - min(fleft, fright)
    fmax = wn_loc[0] + min(fleft, fright) + 1

    tleft = wn_loc[1]
    tright = nt - wn_loc[1] - 1
    tmin = wn_loc[1] - min(tleft, tright)
    tmax = wn_loc[1] + min(tleft, tright) + 1

    ydata_centered = acf[fmin:fmax, tmin:tmax]
    weights_centered = weights_2d[fmin:fmax, tmin:tmax]
    tdata_centered = tticks[tmin:tmax]
    fdata_centered = fticks[fmin:fmax]
    rows_centered = np.arange(nf)[fmin:fmax]
    cols_centered = np.arange(nt)[tmin:tmax]

    if nscale is not None and not full_frame:
        ntau = nscale
        ndnu = nscale

        if ntau > (tobs / tau):
            tmin = 0
            tmax = nt
        else:
            tframe = int(round(ntau * (tau / dt)))
            tmin = int(np.floor(
                np.shape(ydata_centered)[1] / 2)) - tframe
            tmax = int(np.floor(
                np.shape(ydata_centered)[1] / 2)) + tframe + 1

        if ndnu > (bw / dnu):
            tmin = 0
            tmax = nf
        else:
            fframe = int(round(ndnu * (dnu / df)))
            fmin = int(np.floor(
                np.shape(ydata_centered)[0] / 2)) - fframe
            fmax = int(np.floor(
                np.shape(ydata_centered)[0] / 2)) + fframe + 1

        ydata_2d = ydata_centered[fmin:fmax, tmin:tmax]
        weights_2d = weights_centered[fmin:fmax, tmin:tmax]
        tdata = tdata_centered[tmin:tmax]
        fdata = fdata_centered[fmin:fmax]
        rows, cols = rows_centered[fmin:fmax], cols_centered[tmin:tmax]
    else:
        ydata_2d = ydata_centered
        tdata = tdata_centered
        fdata = fdata_centered
        weights_2d = weights_centered
        rows, cols = rows_centered, cols_centered
    rect = (int(rows[0]) if len(rows) else 0, len(rows), int(cols[0]) if len(cols) else 0, len(cols))
    if len(rows) % 2 == 0 or len(cols) % 2 == 0:
        raise BadWindow(rect)
    ydata_2d = np.array(ydata_2d)
    weights_2d = np.array(weights_2d)

    with np.errstate(divide="ignore"):
        weights_2d[ydata_2d - 1/weights_2d < 0] = 0

    weights_2d = np.fft.fftshift(weights_2d)
    weights_2d[0][0] = 1e10
    weights_2d = np.fft.fftshift(weights_2d)
    # what the model then does to them (scint_models.py:156-158)
    weights = np.fft.fftshift(weights_2d)
    weights[-1, -1] = 0  # Not fitting for the white noise spike
    weights = np.fft.ifftshift(weights)
    return dict(rect=rect, t=tdata, f=fdata, y=ydata_2d, w=weights, p0=p0, tobs=tobs, bw=bw, nofit=s1, argmax=wn_loc)


def model(p, tdata, fdata, tobs, bw):
    """The model of scint_acf_model_2d_approx [nf, nt] at p = (tau, dnu, amp, alpha, phasegrad), in the reference's statements."""
    tau, dnu, amp, alpha, phasegrad = p
    mu = phasegrad*60  # min/MHz to s/MHz
    nt = len(tdata)
    nf = len(fdata)
    tdata = np.reshape(tdata, (nt, 1))
    fdata = np.reshape(fdata, (1, nf))
    m = amp * np.exp(-(abs((tdata - mu*fdata)/tau)**(3 * alpha / 2) +
                     abs(fdata / (dnu / np.log(2)))**(3 / 2))**(2 / 3))
    # multiply by triangle function
    m = np.multiply(m, 1-np.divide(abs(tdata), tobs))
    m = np.multiply(m, 1-np.divide(abs(fdata), bw))
    return np.transpose(m)


def model_residual(p, tdata, fdata, ydata, weights, tobs, bw):
    """scint_acf_model_2d_approx (scint_models.py:123-161) with explicit parameters; weights None: ones."""
    if weights is None:
        weights = np.ones(np.shape(ydata))
    weights = np.fft.fftshift(weights)
    weights[-1, -1] = 0  # Not fitting for the white noise spike
    weights = np.fft.ifftshift(weights)
    return (ydata - model(p, tdata, fdata, tobs, bw)) * weights


def residuals(p, s):
    """The residual vector of the fit (row-major over the window) at p = (tau, dnu, amp, alpha, phasegrad)."""
    return ((s["y"] - model(p, s["t"], s["f"], s["tobs"], s["bw"])) * s["w"]).ravel()


def jacobian(p, s, log_scales=True):
    """d residuals / d (log tau, log dnu, log amp, alpha, phasegrad) -- or d / d (tau, dnu, amp, ...) -- at p, analytic.  [N, 5]."""
    tau, dnu, amp, alpha, pg = p
    t, f = np.meshgrid(s["t"], s["f"])
    w = s["w"]
    ex = 1.5 * alpha
    u = (t - 60 * pg * f) / tau
    au = np.abs(u)
    with np.errstate(divide="ignore", invalid="ignore"):
        A = au ** ex
        Bv = np.abs(f * np.log(2) / dnu) ** 1.5
        S = A + Bv
        G = S ** (2 / 3)
        m = amp * np.exp(-G) * (1 - np.abs(t) / s["tobs"]) * (1 - np.abs(f) / s["bw"])
        K = np.where(S > 0, m * (2 / 3) * G / S, 0.0)
        lnu = np.where(au > 0, A * np.log(au), 0.0)
        Aou = np.where(au > 0, A / u, 0.0)
    J = np.zeros(t.shape + (5,))
    J[..., 0] = -w * K * ex * A
    J[..., 1] = -w * K * 1.5 * Bv
    J[..., 2] = -w * m
    J[..., 3] = w * K * 1.5 * lnu
    J[..., 4] = -w * K * ex * Aou * 60 * f / tau
    J = J.reshape(-1, 5)
    if not log_scales:
        J[:, :3] /= np.array([tau, dnu, amp])
    return J


def _columns(vary_tau, vary_alpha):
    return ([0] if vary_tau else []) + [1, 2, 4] + ([3] if vary_alpha else [])


def stationarity(p, s, vary_alpha, vary_tau=True):
    """(max_i |J^T r|_i over the varying ones of (log tau, log dnu, log amp, phasegrad, alpha), chi^2) at p, on the host."""
    r = residuals(p, s)
    g = jacobian(p, s).T @ r
    return float(np.abs(g[_columns(vary_tau, vary_alpha)]).max()), float(r @ r)


def fit(s, alpha=5/3, vary_tau=True, start=None):
    """Solve the problem `setup` describes from s["p0"], or from `start` = (tau, dnu, amp, alpha, phasegrad)."""
    vary_alpha = alpha is None
    cols = _columns(vary_tau, vary_alpha)
    nv = len(cols)
    p0 = np.array([s["p0"][k] for k in NAMES] if start is None else start, dtype=float)
    if not (np.all(p0[:3] > 0) and np.all(np.isfinite(p0))):
        return dict(success=False)

    def ext(q):
        p = p0.copy()
        for qi, c in zip(q, cols):
            p[c] = np.exp(qi) if c < 3 else qi
        return p

    q0 = np.array([np.log(p0[c]) if c < 3 else p0[c] for c in cols])
    sol = least_squares(lambda q: residuals(ext(q), s), q0, jac=lambda q: jacobian(ext(q), s)[:, cols], method="lm",
                        ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=20000)
    p = ext(sol.x)
    r = residuals(p, s)
    chisqr = float(r @ r)
    redchi = chisqr / (len(r) - nv)
    Je = jacobian(p, s, log_scales=False)[:, cols]
    err = np.zeros(5)
    try:
        err[cols] = np.sqrt(np.diag(np.linalg.inv(Je.T @ Je) * redchi))
    except np.linalg.LinAlgError:
        err[cols] = np.nan
    out = {k: p[i] for i, k in enumerate(NAMES)}
    out.update({k + "err": err[i] for i, k in enumerate(NAMES)})
    out.update(chisqr=chisqr, redchi=redchi, nfev=sol.nfev,
               success=bool(sol.status > 0 and np.all(np.isfinite(err)) and np.all(np.isfinite(p))))
    return out


def second_start(s, vary_alpha):
    """Another start of the same problem: the oracle's two answers give its own spread."""
    p = s["p0"]
    pg = p["phasegrad"] + 0.1 * p["tau"] / (60 * p["dnu"])          # a tenth of the tilt tau / dnu, in min/MHz
    return [1.3 * p["tau"], 0.8 * p["dnu"], 1.1 * p["amp"], 1.5 if vary_alpha else p["alpha"], pg]


def fit_attrs(fit_, o, alpha, name=""):
    """What the reference sets after a successful acf2d_approx fit (dynspec.py:2953-3021), from a `fit` result."""
    out = ao1.fit_attrs(fit_, o, alpha, name=name)
    out["scint_param_method"] = "acf2d_approx"
    out["phasegrad"] = fit_["phasegrad"]
    out["phasegraderr"] = fit_["phasegraderr"]
    out["fse_phasegrad"] = fit_["phasegrad"] * np.sqrt((out["fse_dnu"]/out["dnu"])**2 +
                                                       (out["fse_tau"]/out["tau"])**2)
    return out
