"""CPU oracle of the 1-D ACF fit (scint_acf1d_fit, Dynspec.fit_scint_params) -- TEST INFRASTRUCTURE.

A NumPy restatement of what the reference's ``get_scint_params(method='acf1d')`` does between reading the ACF and calling lmfit:
the two half-cuts, start values and crop (dynspec.py:2575-2608), the weights (dynspec.py:2669-2687) and the residual vector
(scint_models.py:62-120).  lmfit itself is replaced by ``scipy.optimize.least_squares`` at tight tolerances on the SAME
least-squares problem, in (log tau, log dnu, log amp[, alpha]) so that the scales stay positive as the reference's ``min=0``
keeps them; the standard errors are ``sqrt(diag((J^T J)^-1 chi^2 / (N - nvary)))`` in the external parameters, which is what
lmfit reports for a fit away from its bounds.  The results attributes (dynspec.py:2953-3002) are restated in ``fit_attrs``."""
import numpy as np
from scipy.optimize import least_squares

ALPHA0 = 5/3           # the reference's start value when alpha varies (dynspec.py:2661)


def setup(acf, dt, df, bw, tobs, nscale=5, full_frame=False, weighted=True, bartlett=True):
    """Start values, cropped cuts and weights of one ACF, statement for statement (dynspec.py:2575-2608, 2669-2687)."""
    nf, nt = np.shape(acf)
    ydata_f = acf[int(nf/2):, int(nt/2)]
    xdata_f = df * np.linspace(0, len(ydata_f)-1, len(ydata_f))
    ydata_t = acf[int(nf/2), int(nt/2):]
    xdata_t = dt * np.linspace(0, len(ydata_t)-1, len(ydata_t))
    wn = min([ydata_f[0]-ydata_f[1], ydata_t[0]-ydata_t[1]])
    amp = max([ydata_f[0] - wn, ydata_t[0] - wn])
    if np.argwhere(ydata_t < amp/np.e).squeeze().size == 0:
        tau = dt if ydata_t[1] < 0 else tobs
    else:
        tau = xdata_t[np.argwhere(ydata_t < amp/np.e).squeeze()[0]]
    if np.argwhere(ydata_f < amp/2).squeeze().size == 0:
        dnu = df if ydata_f[1] < 0 else bw
    else:
        dnu = xdata_f[np.argwhere(ydata_f < amp/2).squeeze()[0]]
    if not full_frame:
        t_inds = np.argwhere(xdata_t <= nscale*tau).squeeze()
        f_inds = np.argwhere(xdata_f <= nscale*dnu).squeeze()
        if nscale*tau <= 5*dt:
            t_inds = np.argwhere(xdata_t <= 5*dt).squeeze()
        if nscale*dnu <= 5*df:
            f_inds = np.argwhere(xdata_f <= 5*df).squeeze()
        xdata_t = xdata_t[t_inds]
        ydata_t = ydata_t[t_inds]
        xdata_f = xdata_f[f_inds]
        ydata_f = ydata_f[f_inds]
    # Create weights array
    t_errors = np.ones(np.shape(xdata_t))/np.sqrt((nt/2))
    t_errors[0] = 1e-3
    f_errors = np.ones(np.shape(xdata_f))/np.sqrt((nf/2))
    f_errors[0] = 1e-3
    if bartlett:
        var_t = np.ones(np.shape(ydata_t)) / (nt / 2)
        var_t[0] = 1e-10
        var_t[2:] *= 1 + 2 * np.cumsum(ydata_t[1:-1] ** 2)
        t_errors = np.sqrt(var_t)
        var_f = np.ones(np.shape(ydata_f)) / (nf / 2)
        var_f[0] = 1e-10
        var_f[2:] *= 1 + 2 * np.cumsum(ydata_f[1:-1] ** 2)
        f_errors = np.sqrt(var_f)
    weights_t = 1/t_errors if weighted else np.ones(np.shape(ydata_t))
    weights_f = 1/f_errors if weighted else np.ones(np.shape(ydata_f))
    weights_t[0] = 0  # Not fitting for the white noise spike (scint_models.py:81, :105)
    weights_f[0] = 0
    return dict(wn=wn, amp=amp, tau=tau, dnu=dnu, x_t=xdata_t, y_t=np.array(ydata_t), x_f=xdata_f, y_f=np.array(ydata_f),
                w_t=weights_t, w_f=weights_f)


def residuals(p, s):
    """scint_acf_model (scint_models.py:62-120) at p = (tau, dnu, amp, alpha)."""
    tau, dnu, amp, alpha = p
    xt, xf = s["x_t"], s["x_f"]
    model_t = amp*np.exp(-np.divide(xt, tau)**(alpha))
    model_t = np.multiply(model_t, 1-np.divide(xt, max(xt)))
    model_f = amp*np.exp(-np.divide(xf, dnu/np.log(2)))
    model_f = np.multiply(model_f, 1-np.divide(xf, max(xf)))
    return np.concatenate(((s["y_t"] - model_t) * s["w_t"], (s["y_f"] - model_f) * s["w_f"]))


def jacobian(p, s, log_scales=True):
    """d residuals / d (log tau, log dnu, log amp, alpha) -- or d / d (tau, dnu, amp, alpha) -- at p, analytic.  [N, 4]."""
    tau, dnu, amp, alpha = p
    xt, xf, wt, wf = s["x_t"], s["x_f"], s["w_t"], s["w_f"]
    J = np.zeros((len(xt) + len(xf), 4))
    tri_t, tri_f = 1 - xt/max(xt), 1 - xf/max(xf)
    u = xt[1:]/tau
    sp = u**alpha
    m = amp*np.exp(-sp)*tri_t[1:]
    J[1:len(xt), 0] = -wt[1:]*m*alpha*sp
    J[1:len(xt), 2] = -wt[1:]*m
    J[1:len(xt), 3] = wt[1:]*m*sp*np.log(u)
    v = xf*np.log(2)/dnu
    mf = amp*np.exp(-v)*tri_f
    J[len(xt):, 1] = -wf*mf*v
    J[len(xt):, 2] = -wf*mf
    if not log_scales:
        J[:, :3] /= np.array([tau, dnu, amp])
    return J


def stationarity(p, s, vary_alpha):
    """(max_i |J^T r|_i in (log tau, log dnu, log amp[, alpha]), chi^2) at p, in float64 on the host."""
    r = residuals(p, s)
    g = jacobian(p, s).T @ r
    return float(np.abs(g[:4 if vary_alpha else 3]).max()), float(r @ r)


def fit(s, alpha=5/3, start=None):
    """Solve the problem `setup` describes.  `start`: (tau, dnu, amp[, alpha]) instead of the reference's start values.  Returns
    values, standard errors, chisqr, redchi and `success` (scipy's status > 0 and finite standard errors)."""
    vary = alpha is None
    nv = 4 if vary else 3
    p0 = [s["tau"], s["dnu"], s["amp"], ALPHA0 if vary else alpha] if start is None else list(start) + ([] if vary else [alpha])
    if not all(v > 0 and np.isfinite(v) for v in p0[:3]):
        return dict(success=False)

    def ext(q):
        return np.array([np.exp(q[0]), np.exp(q[1]), np.exp(q[2]), q[3] if vary else alpha])

    q0 = np.array([np.log(p0[0]), np.log(p0[1]), np.log(p0[2])] + ([p0[3]] if vary else []))
    sol = least_squares(lambda q: residuals(ext(q), s), q0, jac=lambda q: jacobian(ext(q), s)[:, :nv], method="lm",
                        ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=20000)
    p = ext(sol.x)
    r = residuals(p, s)
    chisqr = float(r @ r)
    redchi = chisqr / (len(r) - nv)
    Je = jacobian(p, s, log_scales=False)[:, :nv]
    try:
        cov = np.linalg.inv(Je.T @ Je) * redchi
        err = np.sqrt(np.diag(cov))
    except np.linalg.LinAlgError:
        err = np.full(nv, np.nan)
    out = dict(tau=p[0], dnu=p[1], amp=p[2], alpha=p[3], tauerr=err[0], dnuerr=err[1], amperr=err[2],
               alphaerr=err[3] if vary else 0.0, chisqr=chisqr, redchi=redchi, nfev=sol.nfev,
               success=bool(sol.status > 0 and np.all(np.isfinite(err)) and np.all(np.isfinite(p))))
    return out


def second_start(s, vary_alpha):
    """Another start of the same problem: the oracle's two answers give its own spread."""
    return [1.3 * s["tau"], 0.8 * s["dnu"], 1.1 * s["amp"]] + ([1.5] if vary_alpha else [])


def fit_stack(stack, dt, df, bw, tobs, alpha=5/3, **kw):
    """`setup` and `fit` of every ACF of a stack; bw and tobs scalars or one per problem."""
    B = len(stack)
    bw, tobs = np.broadcast_to(bw, (B,)), np.broadcast_to(tobs, (B,))
    setups = [setup(stack[b], dt, df, bw[b], tobs[b], **kw) for b in range(B)]
    return setups, [fit(s, alpha=alpha) for s in setups]


def fit_attrs(fit_, o, alpha, name=""):
    """What the reference sets after a successful acf1d fit (dynspec.py:2953-3002), from a `fit` result."""
    out = {"scint_param_method": "acf1d"}
    tau, dnu = fit_["tau"], fit_["dnu"]
    out["tau"], out["dnu"] = tau, dnu
    out["tscat"] = 1/(2*np.pi*dnu)
    nscint = (1 + 0.2*o.bw/(dnu)) * \
        (1 + 0.2*o.tobs/(tau*np.log(2)))
    out["nscint"] = nscint
    out["fse_tau"] = tau/(2*np.sqrt(nscint))
    out["fse_dnu"] = dnu/(2*np.sqrt(nscint))
    out["tauerr"] = np.sqrt(fit_["tauerr"]**2 + out["fse_tau"]**2)
    out["dnuerr"] = np.sqrt(fit_["dnuerr"]**2 + out["fse_dnu"]**2)
    out["amp"] = fit_["amp"]
    out["amperr"] = fit_["amperr"]
    out["wn"] = 0 if 'sim:mb2=' in name else 1 - fit_["amp"]
    out["talpha"] = fit_["alpha"] if alpha is None else alpha
    out["talphaerr"] = fit_["alphaerr"] if alpha is None else 0
    return out
