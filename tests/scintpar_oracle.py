"""CPU oracle of the no-fit scintillation measurements -- TEST INFRASTRUCTURE.

Plain NumPy restatement of four routines of the reference's ``Dynspec``: ``get_scint_params(method='nofit')``
(dynspec.py:2570-2648), ``get_acf_tilt`` (2358-2413, with ``scint_models.fit_parabola``, scint_models.py:300-326), ``cut_dyn``
(3158-3271) and ``calc_acf(method='sspec')`` (3798-3807).  Each takes the ACF or the dynamic spectrum as an ARRAY, so it can be
applied to the reference's ACF (tests/golden/make_golden_scintpar.py, tests/test_scintpar_cpu.py) or to the device's
(tests/test_gpu_scintpar.py).  `o` is anything with df, dt, bw, tobs (and freqs, times for cut_dyn).

PARITY PIN: tests/test_scintpar_cpu.py compares it bit for bit with tests/golden/scintpar.npz, the unmodified reference's output."""
import numpy as np

from oracle import sspec_oracle


def nofit(acf, dyn, o, full_frame=False, nscale=5, internals=None):
    """Every attribute get_scint_params(method='nofit') sets, as a dict (`internals`: a dict that receives the cropped time cut)."""
    out = {}
    nf, nt = np.shape(acf)
    ydata_f = acf[int(nf/2):, int(nt/2)]
    xdata_f = o.df * np.linspace(0, len(ydata_f)-1, len(ydata_f))
    ydata_t = acf[int(nf/2), int(nt/2):]
    xdata_t = o.dt * np.linspace(0, len(ydata_t)-1, len(ydata_t))
    wn = min([ydata_f[0]-ydata_f[1], ydata_t[0]-ydata_t[1]])
    amp = max([ydata_f[0] - wn, ydata_t[0] - wn])
    if np.argwhere(ydata_t < amp/np.e).squeeze().size == 0:
        tau = o.dt if ydata_t[1] < 0 else o.tobs
    else:
        tau = xdata_t[np.argwhere(ydata_t < amp/np.e).squeeze()[0]]
    if np.argwhere(ydata_f < amp/2).squeeze().size == 0:
        dnu = o.df if ydata_f[1] < 0 else o.bw
    else:
        dnu = xdata_f[np.argwhere(ydata_f < amp/2).squeeze()[0]]
    if not full_frame:
        t_inds = np.argwhere(xdata_t <= nscale*tau).squeeze()
        f_inds = np.argwhere(xdata_f <= nscale*dnu).squeeze()
        if nscale*tau <= 5*o.dt:
            t_inds = np.argwhere(xdata_t <= 5*o.dt).squeeze()
        if nscale*dnu <= 5*o.df:
            f_inds = np.argwhere(xdata_f <= 5*o.df).squeeze()
        xdata_t = xdata_t[t_inds]
        ydata_t = ydata_t[t_inds]
        xdata_f = xdata_f[f_inds]
        ydata_f = ydata_f[f_inds]
    out["tau"], out["dnu"], out["amp"], out["wn"] = tau, dnu, amp, wn
    if internals is not None:
        internals["ydata_t"] = np.atleast_1d(ydata_t)
    tau_half = xdata_t[np.argmin(abs(ydata_t - amp/2))]
    if tau_half < o.dt:
        tau_half = o.dt
    elif tau_half > o.tobs:
        tau_half = o.tobs
    nscint = (1 + 0.2*o.bw/(dnu)) * \
        (1 + 0.2*o.tobs/(tau_half))
    out["dnuerr"] = dnu / np.sqrt(nscint)
    out["tauerr"] = tau / np.sqrt(nscint)
    out["amperr"] = amp / np.sqrt(nscint)
    out["wnerr"] = wn / np.sqrt(nscint)
    out["tscat"] = 1/(2*np.pi*dnu)
    out["nscint"] = nscint
    out["scint_param_method"] = 'nofit'
    keep = np.isfinite(dyn) * (dyn != 0)
    mean = np.mean(dyn[keep])
    flux_var_est = mean**2
    flux_var = np.var(dyn[keep])
    dnu_est = o.df * (flux_var/flux_var_est - 1)
    if dnu_est < 0:
        dnu_est = 0
    out["dnu_est"] = dnu_est
    out["dnu_esterr"] = dnu_est / np.sqrt(nscint)
    out["tscat_est"] = 1/(2*np.pi*dnu_est) if dnu_est > 0 else 0
    out["modulation_index"] = np.sqrt(flux_var)/mean
    return out


def nofit_from_moments(acf, mean, flux_var, o, **kw):
    """`nofit` with the moments given (the device's): a 1-pixel dyn cannot carry them, so the moment lines are restated."""
    out = nofit(acf, np.ones((1, 1)), o, **kw)
    nscint = out["nscint"]
    flux_var_est = mean**2
    dnu_est = o.df * (flux_var/flux_var_est - 1)
    if dnu_est < 0:
        dnu_est = 0
    out["dnu_est"] = dnu_est
    out["dnu_esterr"] = dnu_est / np.sqrt(nscint)
    out["tscat_est"] = 1/(2*np.pi*dnu_est) if dnu_est > 0 else 0
    out["modulation_index"] = np.sqrt(flux_var)/mean
    return out


def nofit_margins(acf, o, variants=({}, dict(full_frame=True), dict(nscale=1))):
    """What the fixture conditions of the generator need: (smallest distance of a cut's sample from its threshold -- amp/e in
    time, amp/2 in frequency --, the smallest gap between the two samples closest to amp/2 in the cropped time cut over the
    `variants`, the number of samples below each threshold)."""
    nf, nt = np.shape(acf)
    yf, yt = acf[int(nf/2):, int(nt/2)], acf[int(nf/2), int(nt/2):]
    gaps = []
    for kw in variants:
        keep = {}
        amp = nofit(acf, np.ones((1, 1)), o, internals=keep, **kw)["amp"]
        d = np.sort(abs(keep["ydata_t"] - amp/2))
        gaps.append(d[1] - d[0])
    cross = min(np.abs(yt - amp/np.e).min(), np.abs(yf - amp/2).min())
    return cross, min(gaps), int((yt < amp/np.e).sum()), int((yf < amp/2).sum())


def fit_parabola(x, y):
    """scint_models.py:300-326"""
    ptp = np.ptp(x)
    x = x*(1000/ptp)
    params, pcov = np.polyfit(x, y, 2, cov=True)
    yfit = params[0]*np.power(x, 2) + params[1]*x + params[2]
    errors = []
    for i in range(len(params)):
        errors.append(np.absolute(pcov[i][i])**0.5)
    peak = -params[1]/(2*params[0])
    peak_error = np.sqrt((errors[1]**2)*((1/(2*params[0]))**2) +
                         (errors[0]**2)*((params[1]/2)**2))
    peak = peak*(ptp/1000)
    peak_error = peak_error*(ptp/1000)
    return yfit, peak, peak_error


def tilt_rows(acf_shape, o, dnu, nscale=0.8, nmin=5, fmax=None):
    """The ACF rows get_acf_tilt fits (dynspec.py:2361-2365)."""
    nr, nc = acf_shape
    if fmax is None:
        fmax = nscale*dnu
    f_shifts = np.linspace(-o.bw, o.bw, nr+1)[:-1]
    inds = np.argwhere(abs(f_shifts) <= fmax)
    if len(inds) < nmin:
        inds = np.argwhere(abs(f_shifts) <= nmin*o.df)
    return inds


def acf_tilt(acf, o, tau, dnu, nscale=0.8, nmin=5, fmax=None):
    """(acf_tilt, acf_tilt_err, fse_tilt) of get_acf_tilt (dynspec.py:2358-2413)."""
    nr, nc = np.shape(acf)
    t_delays = np.linspace(-o.tobs/60, o.tobs/60, nc+1)[:-1]
    f_shifts = np.linspace(-o.bw, o.bw, nr+1)[:-1]
    inds = tilt_rows((nr, nc), o, dnu, nscale=nscale, nmin=nmin, fmax=fmax)
    peak_array = []
    peakerr_array = []
    y_array = []
    for ii in inds:
        x_max = np.argmax(acf[ii, :]).squeeze()
        ydata = np.array(acf[ii, x_max - 3:x_max + 4]).squeeze()
        xdata = t_delays[x_max - 3:x_max + 4]
        yfit, peak, peakerr = fit_parabola(xdata, ydata)
        peak_array.append(peak)
        peakerr_array.append(peakerr)
        y_array.append(f_shifts[ii])
    peak_array = np.array(peak_array).squeeze()
    y_array = np.array(y_array).squeeze()
    peakerr_array = np.array(peakerr_array).squeeze()
    params, pcov = np.polyfit(peak_array, y_array, 1, cov=True,
                              w=1/peakerr_array)
    xfit = (y_array - params[1])/params[0]
    errors = []
    for i in range(len(params)):
        errors.append(np.absolute(pcov[i][i])**0.5)
    errors = np.array(errors).squeeze()
    res = np.array(peak_array - xfit).squeeze()
    reduced_chi_sq = np.sum(res**2/peakerr_array**2)/(len(xfit) - 2)
    errors *= np.sqrt(reduced_chi_sq)
    tilt = 1/(float(params[0].squeeze()))
    tilt_err = float(errors[0].squeeze()) * \
        1/float(params[0].squeeze())**2
    N = (1 + 0.2*o.bw/(dnu)) * \
        (1 + 0.2*o.tobs/(tau*np.log(2)))
    fse_tau = tau/(2*np.sqrt(N))
    fse_dnu = dnu/(2*np.sqrt(N))
    fse_tilt = tilt * np.sqrt((fse_dnu/dnu)**2 +
                              (fse_tau/tau)**2)
    return tilt, tilt_err, fse_tilt


def tilt_peak_margins(acf, inds):
    """(smallest distance of a fitted row's maximum from an edge, smallest gap between a row's two largest samples)."""
    edge, gap = np.inf, np.inf
    for ii in inds:
        row = acf[int(ii[0])]
        x = int(np.argmax(row))
        edge = min(edge, x, len(row) - 1 - x)
        top = np.sort(row)[-2:]
        gap = min(gap, top[1] - top[0])
    return edge, gap


def calc_acf_input(dyn, normalise=True):
    """calc_acf(input_dyn=...) (dynspec.py:3786-3797): no mean subtraction."""
    nf, nt = np.shape(dyn)
    arr = np.fft.fft2(dyn, s=[2*nf, 2*nt])
    arr = np.abs(arr)
    arr **= 2
    arr = np.fft.ifft2(arr)
    arr = np.fft.fftshift(arr)
    arr = np.real(arr)
    if normalise:
        arr /= np.max(arr)
    return arr


def cut_dyn(dyn, nchan, nsub, tcuts=0, fcuts=0):
    """(cutdyn, cutsspec, cutacf) of cut_dyn (dynspec.py:3188-3210); the reference discards the last."""
    fnum = np.floor(nchan/(fcuts + 1))
    tnum = np.floor(nsub/(tcuts + 1))
    cutdyn = np.empty(shape=(fcuts+1, tcuts+1, int(fnum), int(tnum)))
    nrfft = int(2**(np.ceil(np.log2(int(fnum)))+1)/2)
    ncfft = int(2**(np.ceil(np.log2(int(tnum)))+1))
    cutsspec = np.empty(shape=(fcuts+1, tcuts+1, nrfft, ncfft))
    cutacf = np.empty(shape=(fcuts+1, tcuts+1, 2*int(fnum), 2*int(tnum)))
    for ii in reversed(range(0, fcuts+1)):
        for jj in range(0, tcuts+1):
            cutdyn[ii][jj][:][:] = dyn[int(ii*fnum):int((ii+1)*fnum), int(jj*tnum):int((jj+1)*tnum)]
            cutsspec[ii][jj][:][:] = sspec_oracle.calc_sspec(cutdyn[ii][jj], 1.0, 1.0)[2]
            cutacf[ii][jj][:][:] = calc_acf_input(cutdyn[ii][jj])
    return cutdyn, cutsspec, cutacf


def acf_sspec(dyn, normalise=True, window_frac=0.1):
    """calc_acf(method='sspec') (dynspec.py:3798-3807)."""
    sspec = sspec_oracle.calc_sspec(dyn, 1.0, 1.0, prewhite=False, halve=False, window_frac=window_frac)[2]
    sspec = np.fft.fftshift(sspec)
    arr = np.fft.fft2(10**(sspec/10))
    arr = np.fft.fftshift(arr)
    arr = np.real(arr)
    if normalise:
        arr /= np.max(arr)
    return arr
