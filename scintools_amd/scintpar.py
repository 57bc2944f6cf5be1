"""Scintillation scales without a fit: ``get_scint_params(method='nofit')``, ``get_acf_tilt`` and ``cut_dyn`` of the reference
``Dynspec`` (dynspec.py:2470-2648, 2283-2413, 3158-3271), and the device half of ``calc_acf``.

The functions are bound onto ``scintools_amd.dynspec.Dynspec`` as ``arcfit``'s and ``clean``'s are.  What runs where:

* ``calc_acf`` leaves the ``[2 nf, 2 nt]`` ACF in HBM (``Dynspec.acf`` is a ``device.DeviceBacked`` attribute).
* ``get_scint_params(method='nofit')``: the two half-cuts through the ACF's centre (``scint_acf_cuts``) and count / mean /
  variance of the valid pixels of ``dyn`` (``scint_dyn_moments``) come from the device; the arithmetic on them is the
  reference's, statement for statement, on the host.
* ``get_acf_tilt``: per selected ACF row the first column of the maximum and the 7 samples around it come from the device
  (``scint_acf_row_peaks``); ``fit_parabola`` per row and the weighted ``np.polyfit`` run on the host.  A row whose 7-sample
  window would cross the first or last column raises ``ValueError`` (the reference's slice is empty, or short, there).
* ``cut_dyn``: one upload of ``dyn``; segments cut on the device (``scint_segment_cut``), every segment's secondary spectrum
  (``dynspec.sspec_stack_device``, ``scint_sspec_batch``) and ACF (``acf_stack_device``, ``scint_acf_batch``) from one batched call
  each, from device memory; the
  three stacks stay in HBM until they are read (``device.DeviceBacked``).  ``self.cutacf`` is the one addition: the reference
  computes every segment's ACF and discards it.

The fitted methods of ``get_scint_params`` (``acf1d``, ``acf2d_approx``, ``acf2d``, ``sspec``, ``mcmc``) need lmfit and raise
``NotImplementedError``.  The 1-D ACF fit itself -- the reference's default, dynspec.py:2650-2702 with scint_models.py:62-120 -- runs
on the device under names of its own:

* ``acf1d_fit_device``: a stack of ACFs in HBM, one Levenberg-Marquardt problem per wavefront, one launch (``scint_acf1d_fit``).
* ``fit_scint_params``: the batch of one on ``self.acf``; sets what the reference sets after an ``acf1d`` fit.
* ``fit_scint_params_cut``: every segment of ``cut_dyn`` -- cut, ACF and fit on the device, one fit launch for all of them.

So does the approximate 2-D fit (``method='acf2d_approx'``, dynspec.py:2689-2842 with scint_models.py:123-161), the one that yields
the phase gradient: ``acf2d_approx_fit_device`` (one workgroup per problem, ``scint_acf2d_approx_fit``, csrc/acf2d.hpp),
``fit_scint_params_2d`` and ``fit_scint_params_2d_cut``.
"""
import ctypes
import warnings

import numpy as np
import torch

from . import _lib, device
from .arcfit import fit_parabola

PEAK_WINDOW = 7            # acf[row, x - 3 : x + 4] (csrc/scintpar.hpp, kPeakWindow)

# status of a fit (csrc/scintpar.hpp, kFit*)
FIT_CONVERGED, FIT_ITER_CAP, FIT_SINGULAR, FIT_NONFINITE_INPUT, FIT_NONFINITE_STEP = range(5)
FIT_BAD_WINDOW = 5         # the 2-D fit only (csrc/acf2d.hpp, kFitBadWindow)
FIT_STATUS_TEXT = ("converged", "iteration cap reached", "singular normal matrix", "non-finite sample in a half-cut",
                   "non-finite cost or step", "the fit window has an even or empty side")

_NEEDS_LMFIT = ("get_scint_params(method={0!r}) needs lmfit and is outside the accelerated path; "
                "pass method='nofit' for the scales read off the ACF without a fit")


def _lib_ready():
    _lib.load()
    device.require_gpu()


# ----------------------------------------------------------------------------
# device calls
# ----------------------------------------------------------------------------
def acf_device(dyn_t, subtract_mean=True, normalise=True, out=None):
    """Direct-method ACF of a device dynamic spectrum [nf, nt] float64 -> device tensor [2 nf, 2 nt] (``scint_acf``)."""
    _lib_ready()
    nf, nt = (int(v) for v in dyn_t.shape)
    ws = device.workspace_for("scint_acf", nf, nt)
    if out is None:
        out = device.empty((2 * nf, 2 * nt), torch.float64)
    _lib.call("scint_acf", dyn_t, nf, nt, 1 if subtract_mean else 0, 1 if normalise else 0, out, ws, ws.numel(),
              device.stream_ptr())
    return out


STACK_GROUP_BYTES = 8 << 30     # workspace a group of a stack's problems may hold at once (ththmod.RETRIEVAL_GROUP_BYTES)
STACK_GROUP_MAX = 65535         # problems of one call: grid.z of the column passes (csrc/fft.hip)


def _stack_groups(B, bytes_per_problem, group_bytes):
    """``(start, count)`` of the groups a stack of B problems is taken in: as many problems as fit into ``group_bytes`` (None or 0:
    STACK_GROUP_BYTES), at least one, at most STACK_GROUP_MAX -- ``ththmod._group_size``'s rule."""
    per = min(STACK_GROUP_MAX, max(1, int((group_bytes or STACK_GROUP_BYTES) // bytes_per_problem)))
    return [(b0, min(per, B - b0)) for b0 in range(0, B, per)]


def _check_stack(what, stack_t):
    if not torch.is_tensor(stack_t) or stack_t.dim() != 3:
        raise ValueError(f"{what}: expected a stack of dynamic spectra [B, nf, nt]")
    if stack_t.dtype != torch.float64:
        raise ValueError(f"{what}: expected a float64 stack, got {stack_t.dtype}")
    if not stack_t.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous stack")
    if stack_t.shape[0] < 1:
        raise ValueError(f"{what}: the stack is empty")
    return (int(v) for v in stack_t.shape)


def acf_stack_device(stack_t, subtract_mean=False, normalise=True, out=None, group_bytes=None):
    """``acf_device`` of every dynamic spectrum of a contiguous device stack [B, nf, nt] float64 -> device tensor [B, 2 nf, 2 nt],
    problem for problem the bits of ``acf_device(stack_t[k], subtract_mean, normalise)`` (``scint_acf_batch``: the problems are
    slots and grid.z of the single call's kernels, so the launches do not grow with B).  The workspace does: the stack is taken in
    groups whose workspace stays below ``group_bytes`` (None: STACK_GROUP_BYTES), a handful of launches per group.  ``out``: a
    contiguous device tensor of the result's shape to write into.  (``subtract_mean`` defaults to ``cut_dyn``'s: none.)"""
    _lib_ready()
    B, nf, nt = _check_stack("acf_stack_device", stack_t)
    shape = (B, 2 * nf, 2 * nt)
    if out is None:
        out = device.empty(shape, torch.float64)
    elif tuple(out.shape) != shape or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError(f"acf_stack_device: out must be a contiguous float64 tensor of shape {shape}")
    one = ctypes.c_size_t()
    _lib.call("scint_acf_batch_workspace_bytes", 1, nf, nt, one)
    for b0, n in _stack_groups(B, one.value, group_bytes):
        ws = device.workspace_for("scint_acf_batch", n, nf, nt)      # (no more than n times one problem's)
        _lib.call("scint_acf_batch", stack_t[b0:b0 + n], n, nf, nt, 1 if subtract_mean else 0, 1 if normalise else 0,
                  out[b0:b0 + n], ws, ws.numel(), device.stream_ptr())
    return out


def acf_from_sspec_device(sec_t, normalise=True):
    """``real(fftshift(fft2(10**(fftshift(sec) / 10))))`` (/ max) of a full-frame secondary spectrum in dB on the device."""
    _lib_ready()
    R, C = (int(v) for v in sec_t.shape)
    ws = device.workspace_for("scint_acf_sspec", R, C)
    out = device.empty((R, C), torch.float64)
    _lib.call("scint_acf_sspec", sec_t, R, C, 1 if normalise else 0, out, ws, ws.numel(), device.stream_ptr())
    return out


def acf_cuts_device(acf_t):
    """``(acf[int(nf/2):, int(nt/2)], acf[int(nf/2), int(nt/2):])`` of a device ACF as host arrays: the ACF's own bits."""
    _lib_ready()
    R, C = (int(v) for v in acf_t.shape)
    nfc, ntc = R - R // 2, C - C // 2
    out = device.empty((nfc + ntc,), torch.float64)
    _lib.call("scint_acf_cuts", acf_t, R, C, out, device.stream_ptr())
    cuts = out.cpu().numpy()
    return cuts[:nfc], cuts[nfc:]


def dyn_moments_device(dyn_t):
    """(count, mean, population variance) of the finite, non-zero pixels of a device array (dynspec.py:2633-2635)."""
    _lib_ready()
    stats = device.empty((3,), torch.float64)
    ws = device.workspace_for("scint_dyn_moments")
    _lib.call("scint_dyn_moments", dyn_t, int(dyn_t.numel()), stats, ws, ws.numel(), device.stream_ptr())
    count, mean, var = (float(v) for v in stats.cpu().numpy())
    return int(count), mean, var


def acf_row_peaks_device(acf_t, rows):
    """Per row of ``rows``: (first column of the row maximum, the 7 samples ``acf[row, x - 3 : x + 4]``, flag) from the device.
    flag 1: the window would cross the first or last column (its samples are then zero, nothing outside the row is read)."""
    _lib_ready()
    R, C = (int(v) for v in acf_t.shape)
    rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
    if rows.size < 1 or rows.min() < 0 or rows.max() >= R:
        raise ValueError("acf_row_peaks_device: a row lies outside the ACF")
    n = int(rows.size)
    rows_t = device.to_device(rows, torch.int32)
    cols = device.empty((n,), torch.int32)
    wins = device.empty((n, PEAK_WINDOW), torch.float64)
    flags = device.empty((n,), torch.int32)
    _lib.call("scint_acf_row_peaks", acf_t, R, C, rows_t, n, cols, wins, flags, device.stream_ptr())
    return cols.cpu().numpy(), wins.cpu().numpy(), flags.cpu().numpy()


def segment_cut_device(dyn_t, fnum, tnum, nfseg, ntseg):
    """The segments ``dyn[ii*fnum:(ii+1)*fnum, jj*tnum:(jj+1)*tnum]`` as one device stack [nfseg * ntseg, fnum, tnum]."""
    _lib_ready()
    nf, nt = (int(v) for v in dyn_t.shape)
    out = device.empty((nfseg * ntseg, fnum, tnum), torch.float64)
    _lib.call("scint_segment_cut", dyn_t, nf, nt, fnum, tnum, nfseg, ntseg, out, device.stream_ptr())
    return out


def acf1d_fit_device(acf_stack_t, dt, df, bw, tobs, alpha=5/3, nscale=5, full_frame=False, weighted=True, bartlett=True,
                     max_iter=200, return_setup=False):
    """Fit the 1-D ACF model to the central cuts of every ACF of a device stack [B, R, C] float64 (or one ACF [R, C]) in one launch
    (``scint_acf1d_fit``; dynspec.py:2575-2608, 2650-2702, scint_models.py:62-120).  ``bw`` and ``tobs`` are scalars or one value per
    problem (the fallbacks for ``dnu`` and ``tau`` without a crossing); ``alpha=None`` fits alpha, started at 5/3.  Returns a dict
    of host arrays of length B: ``tau, dnu, amp, alpha`` and ``tauerr, dnuerr, amperr, alphaerr`` (the fit's standard errors: NaN
    unless ``status == FIT_CONVERGED``), ``chisqr, redchi, niter, status`` and the start values ``tau0, dnu0, amp0, wn0`` with the
    crop lengths ``n_t, n_f``.  ``return_setup`` adds ``y_t, y_f, w_t, w_f``: per problem the cropped cuts and their weights."""
    _lib_ready()
    if acf_stack_t.dim() == 2:
        acf_stack_t = acf_stack_t[None]
    if acf_stack_t.dim() != 3:
        raise ValueError("acf1d_fit_device: expected a stack of ACFs [B, R, C]")
    B, R, C = (int(v) for v in acf_stack_t.shape)
    bw_t = device.to_device(np.array(np.broadcast_to(np.asarray(bw, dtype=np.float64), (B,))), torch.float64)
    tobs_t = device.to_device(np.array(np.broadcast_to(np.asarray(tobs, dtype=np.float64), (B,))), torch.float64)
    values, errors = device.empty((B, 4), torch.float64), device.empty((B, 4), torch.float64)
    stats, setup = device.empty((B, 2), torch.float64), device.empty((B, 6), torch.float64)
    niter, status = device.empty((B,), torch.int32), device.empty((B,), torch.int32)
    ws = device.workspace_for("scint_acf1d_fit", B, R, C)
    _lib.call("scint_acf1d_fit", acf_stack_t, B, R, C, float(dt), float(df), bw_t, tobs_t, float(nscale), 1 if full_frame else 0,
              1 if weighted else 0, 1 if bartlett else 0, 5/3 if alpha is None else float(alpha), 1 if alpha is None else 0,
              int(max_iter), values, errors, stats, niter, status, setup, ws, ws.numel(), device.stream_ptr())
    values, errors, stats, setup = (t.cpu().numpy() for t in (values, errors, stats, setup))
    out = dict(tau=values[:, 0], dnu=values[:, 1], amp=values[:, 2], alpha=values[:, 3], tauerr=errors[:, 0], dnuerr=errors[:, 1],
               amperr=errors[:, 2], alphaerr=errors[:, 3], chisqr=stats[:, 0], redchi=stats[:, 1], niter=niter.cpu().numpy(),
               status=status.cpu().numpy(), wn0=setup[:, 0], amp0=setup[:, 1], tau0=setup[:, 2], dnu0=setup[:, 3],
               n_t=setup[:, 4].astype(np.int64), n_f=setup[:, 5].astype(np.int64))
    if return_setup:
        ntc, nfc = C - C // 2, R - R // 2
        rows = ws[:16 * B * (ntc + nfc)].view(torch.float64).cpu().numpy().reshape(B, 2, ntc + nfc)
        nt, nf = out["n_t"], out["n_f"]
        out["y_t"] = [rows[b, 0, :nt[b]] for b in range(B)]
        out["y_f"] = [rows[b, 0, ntc:ntc + nf[b]] for b in range(B)]
        out["w_t"] = [rows[b, 1, :nt[b]] for b in range(B)]
        out["w_f"] = [rows[b, 1, ntc:ntc + nf[b]] for b in range(B)]
    return out


# ----------------------------------------------------------------------------
# Dynspec methods
# ----------------------------------------------------------------------------
def get_scint_params(self, method="acf1d", plot=False, alpha=5/3, mcmc=False, full_frame=False, nscale=5, nwalkers=50,
                     steps=10000, burn=0.25, nitr=1, lnsigma=True, verbose=False, progress=True, display=True,
                     filename=None, dpi=200, nan_policy='raise', weighted=True, workers=1, tau_vary_2d=True,
                     tau_input=None, bartlett=True, get_fit_report=True):
    """Scintillation timescale and bandwidth read off the ACF without a fit (dynspec.py:2470-2648, ``method='nofit'``): the
    1/e and half-power crossings of the central cuts, the number of scintles and the errors it implies, and the modulation
    index and bandwidth estimate from the moments of ``dyn``.  Sets ``tau, dnu, amp, wn, dnuerr, tauerr, amperr, wnerr, tscat,
    nscint, scint_param_method, dnu_est, dnu_esterr, tscat_est, modulation_index``.  The cuts and the moments come from the
    device, the arithmetic is the reference's.  Every other ``method``, ``mcmc`` and ``plot`` raise ``NotImplementedError``."""
    if method != 'nofit':
        raise NotImplementedError(_NEEDS_LMFIT.format(method))
    if mcmc:
        raise NotImplementedError("get_scint_params(mcmc=True) needs lmfit and emcee and is outside the accelerated path")
    if plot:
        raise NotImplementedError("plotting is outside the accelerated path")
    cls = type(self)
    if not cls.acf.present(self):
        self.calc_acf()
    ydata_f, ydata_t = acf_cuts_device(cls.acf.tensor(self))
    count, mean, flux_var = dyn_moments_device(device.to_device(np.asarray(self.dyn, dtype=float), torch.float64))

    xdata_f = self.df * np.linspace(0, len(ydata_f)-1, len(ydata_f))
    xdata_t = self.dt * np.linspace(0, len(ydata_t)-1, len(ydata_t))

    # Estimate amp and white noise level
    wn = min([ydata_f[0]-ydata_f[1], ydata_t[0]-ydata_t[1]])
    amp = max([ydata_f[0] - wn, ydata_t[0] - wn])
    # Estimate tau. Closest index to 1/e power
    if np.argwhere(ydata_t < amp/np.e).squeeze().size == 0:
        tau = self.dt if ydata_t[1] < 0 else self.tobs
    else:
        tau = xdata_t[np.argwhere(ydata_t < amp/np.e).squeeze()[0]]
    # Estimate dnu. Closest index to 1/2 power
    if np.argwhere(ydata_f < amp/2).squeeze().size == 0:
        dnu = self.df if ydata_f[1] < 0 else self.bw
    else:
        dnu = xdata_f[np.argwhere(ydata_f < amp/2).squeeze()[0]]

    # crop arrays to nscale number of scales, or 5 samples
    if not full_frame:
        t_inds = np.argwhere(xdata_t <= nscale*tau).squeeze()
        f_inds = np.argwhere(xdata_f <= nscale*dnu).squeeze()
        if nscale*tau <= 5*self.dt:
            t_inds = np.argwhere(xdata_t <= 5*self.dt).squeeze()
        if nscale*dnu <= 5*self.df:
            f_inds = np.argwhere(xdata_f <= 5*self.df).squeeze()
        xdata_t = xdata_t[t_inds]
        ydata_t = ydata_t[t_inds]
        xdata_f = xdata_f[f_inds]
        ydata_f = ydata_f[f_inds]

    self.tau = tau
    self.dnu = dnu
    self.amp = amp
    self.wn = wn

    # Estimated number of scintles
    tau_half = xdata_t[np.argmin(abs(ydata_t - amp/2))]  # half power
    if tau_half < self.dt:
        tau_half = self.dt
    elif tau_half > self.tobs:
        tau_half = self.tobs
    nscint = (1 + 0.2*self.bw/(self.dnu)) * \
        (1 + 0.2*self.tobs/(tau_half))
    # Estimated errors
    self.dnuerr = dnu / np.sqrt(nscint)
    self.tauerr = tau / np.sqrt(nscint)
    self.amperr = amp / np.sqrt(nscint)
    self.wnerr = wn / np.sqrt(nscint)
    self.tscat = 1/(2*np.pi*self.dnu)  # scattering timescale
    self.nscint = nscint
    self.scint_param_method = 'nofit'

    flux_var_est = mean**2
    # Estimate of scint bandwidth
    self.dnu_est = self.df * (flux_var/flux_var_est - 1)
    if self.dnu_est < 0:
        self.dnu_est = 0
    self.dnu_esterr = self.dnu_est / np.sqrt(nscint)
    if self.dnu_est > 0:
        self.tscat_est = 1/(2*np.pi*self.dnu_est)  # scattering timescale
    else:
        self.tscat_est = 0
    self.modulation_index = np.sqrt(flux_var)/mean
    return


def get_acf_tilt(self, plot=False, tmax=None, fmax=None, display=True, filename=None, nscale=0.8, nscaleplot=2, nmin=5,
                 dpi=200, method='acf1d', tmaxplot=None, fmaxplot=None):
    """Tilt of the ACF, proportional to the phase gradient parallel to Veff (dynspec.py:2283-2413): the peak of every
    frequency-lag row within ``fmax`` (default ``nscale * dnu``; at least ``nmin`` rows) from a 7-point parabola, then a weighted
    straight line through the peaks.  Sets ``acf_tilt`` (min/MHz), ``acf_tilt_err`` and ``fse_tilt``.  Row maxima and windows
    come from the device, the fits run on the host.  Without ``dnu`` it calls ``get_scint_params(method=method)``: only
    ``method='nofit'`` is available here.  A peak closer than 3 columns to an edge raises ``ValueError``."""
    if plot:
        raise NotImplementedError("plotting is outside the accelerated path")
    cls = type(self)
    if not cls.acf.present(self):
        self.calc_acf()
    if not hasattr(self, 'dnu'):
        self.get_scint_params(method=method)

    if tmax is None:
        tmax = nscale*self.tau/60
    if fmax is None:
        fmax = nscale*self.dnu

    nr, nc = cls.acf.shape(self)
    t_delays = np.linspace(-self.tobs/60, self.tobs/60, nc+1)[:-1]
    f_shifts = np.linspace(-self.bw, self.bw, nr+1)[:-1]

    inds = np.argwhere(abs(f_shifts) <= fmax)
    if len(inds) < nmin:
        inds = np.argwhere(abs(f_shifts) <= nmin*self.df)
    if len(inds) < 1:
        raise ValueError("get_acf_tilt: no frequency lag within fmax")
    cols, wins, flags = acf_row_peaks_device(cls.acf.tensor(self), inds[:, 0])
    if np.any(flags != 0):
        bad = int(inds[np.flatnonzero(flags)[0], 0])
        raise ValueError(f"get_acf_tilt: the maximum of ACF row {bad} lies within 3 columns of the edge: "
                         "no 7-sample window for the parabola fit")
    peak_array = []
    peakerr_array = []
    y_array = []

    # Fit parabolas to find the peak in each frequency-slice
    for k, ii in enumerate(inds):
        x_max = int(cols[k])
        ydata = wins[k]
        xdata = t_delays[x_max - 3:x_max + 4]
        yfit, peak, peakerr = fit_parabola(xdata, ydata)
        peak_array.append(peak)
        peakerr_array.append(peakerr)
        y_array.append(f_shifts[ii])
    peak_array = np.array(peak_array).squeeze()
    y_array = np.array(y_array).squeeze()
    peakerr_array = np.array(peakerr_array).squeeze()

    # Now do a weighted fit of a straight line to the peaks
    params, pcov = np.polyfit(peak_array, y_array, 1, cov=True, w=1/peakerr_array)
    xfit = (y_array - params[1])/params[0]

    # Get parameter errors
    errors = []
    for i in range(len(params)):  # for each parameter
        errors.append(np.absolute(pcov[i][i])**0.5)
    errors = np.array(errors).squeeze()
    res = np.array(peak_array - xfit).squeeze()
    reduced_chi_sq = np.sum(res**2/peakerr_array**2)/(len(xfit) - 2)
    errors *= np.sqrt(reduced_chi_sq)

    self.acf_tilt = 1/(float(params[0].squeeze()))  # make min/MHz
    acf_tilt_err = float(errors[0].squeeze()) * \
        1/float(params[0].squeeze())**2

    # Compute finite scintle error
    N = (1 + 0.2*self.bw/(self.dnu)) * \
        (1 + 0.2*self.tobs/(self.tau*np.log(2)))  # 2*half power
    fse_tau = self.tau/(2*np.sqrt(N))
    fse_dnu = self.dnu/(2*np.sqrt(N))

    fse_tilt = self.acf_tilt * np.sqrt((fse_dnu/self.dnu)**2 +
                                       (fse_tau/self.tau)**2)

    self.fse_tilt = fse_tilt
    self.acf_tilt_err = acf_tilt_err
    return


def cut_dyn(self, tcuts=0, fcuts=0, plot=False, filename=None, dpi=200, lamsteps=False, maxfdop=np.inf, figsize=(8, 13),
            display=True):
    """Cut the dynamic spectrum into ``tcuts + 1`` segments in time and ``fcuts + 1`` in frequency (dynspec.py:3158-3271) and
    take every segment's secondary spectrum and ACF.  Sets ``cutdyn [fcuts+1, tcuts+1, fnum, tnum]`` and ``cutsspec [.., nrfft,
    ncfft]`` as the reference does (floor division, remainders dropped; ``lamsteps`` only changes the y-axis of a segment's
    spectrum in the reference, not its data, so it changes nothing here) and -- the one addition -- ``cutacf [.., 2 fnum,
    2 tnum]``, which the reference computes and discards.  ``dyn`` is uploaded once, the segments never visit the host, each
    stack stays in HBM until it is first read (``device.DeviceBacked``)."""
    if plot:
        raise NotImplementedError("plotting is outside the accelerated path")
    from .dynspec import sspec_stack_device
    _lib_ready()
    nchan = len(self.freqs)  # re-define in case of trimming
    nsub = len(self.times)
    fnum = int(np.floor(nchan/(fcuts + 1)))
    tnum = int(np.floor(nsub/(tcuts + 1)))
    if fcuts < 0 or tcuts < 0 or fnum < 2 or tnum < 5:
        raise ValueError(f"cut_dyn: segments of {fnum} channels x {tnum} sub-integrations are too small (at least 2 x 5)")
    dyn = np.asarray(self.dyn, dtype=float)
    if dyn.shape[0] < (fcuts + 1) * fnum or dyn.shape[1] < (tcuts + 1) * tnum:
        raise ValueError("cut_dyn: dyn is smaller than its frequency and time axes")
    if not np.all(np.isfinite(dyn[:(fcuts + 1) * fnum, :(tcuts + 1) * tnum])):
        raise ValueError("cut_dyn on the GPU needs a finite dynamic spectrum (run refill first)")
    # find the right fft lengths for rows and columns
    nrfft = int(2**(np.ceil(np.log2(int(fnum)))+1)/2)
    ncfft = int(2**(np.ceil(np.log2(int(tnum)))+1))
    nseg = (fcuts + 1) * (tcuts + 1)
    segs = segment_cut_device(device.to_device(dyn, torch.float64), fnum, tnum, fcuts + 1, tcuts + 1)
    sspecs = sspec_stack_device(segs)
    acfs = acf_stack_device(segs, subtract_mean=False)            # (with input_dyn the reference subtracts no mean)
    cls = type(self)
    cls.cutdyn.park(self, segs.view(fcuts + 1, tcuts + 1, fnum, tnum))
    cls.cutsspec.park(self, sspecs.view(fcuts + 1, tcuts + 1, nrfft, ncfft))
    cls.cutacf.park(self, acfs.view(fcuts + 1, tcuts + 1, 2 * fnum, 2 * tnum))


def fit_scint_params(self, alpha=5/3, full_frame=False, nscale=5, weighted=True, bartlett=True, verbose=False):
    """Scintillation timescale and bandwidth from the 1-D ACF fit, the reference's ``get_scint_params(method='acf1d')``
    (dynspec.py:2650-2702, 2953-3002), on the device: the batch of one of ``acf1d_fit_device`` on ``self.acf``.  First the no-fit
    values and by-products of ``get_scint_params(method='nofit')``; a converged fit then sets ``tau, dnu, tscat, nscint, fse_tau,
    fse_dnu, tauerr, dnuerr`` (fit error and finite-scintle error in quadrature), ``amp, amperr, wn, talpha, talphaerr`` and
    ``scint_param_method = 'acf1d'``.  ``alpha=None`` fits alpha.  Always sets ``scint_fit_status`` (``FIT_*``),
    ``scint_fit_redchi`` and ``scint_fit_niter``; no ``report``.  A fit that did not converge warns and leaves the no-fit values."""
    self.get_scint_params(method='nofit', full_frame=full_frame, nscale=nscale)
    fit = acf1d_fit_device(type(self).acf.tensor(self), self.dt, self.df, self.bw, self.tobs, alpha=alpha, nscale=nscale,
                           full_frame=full_frame, weighted=weighted, bartlett=bartlett)
    self.scint_fit_status = int(fit["status"][0])
    self.scint_fit_redchi = float(fit["redchi"][0])
    self.scint_fit_niter = int(fit["niter"][0])
    if self.scint_fit_status != FIT_CONVERGED:
        warnings.warn(f"fit_scint_params: the fit did not converge ({FIT_STATUS_TEXT[self.scint_fit_status]} after "
                      f"{self.scint_fit_niter} iterations); the no-fit values are kept")
        return
    self.scint_param_method = 'acf1d'
    self.tau = float(fit["tau"][0])
    self.dnu = float(fit["dnu"][0])
    self.tscat = 1/(2*np.pi*self.dnu)  # scattering timescale
    if self.dnu < self.df:
        print("Warning: Scint bandwidth < channel bandwidth.")
    # Compute finite scintle error
    nscint = (1 + 0.2*self.bw/(self.dnu)) * \
        (1 + 0.2*self.tobs/(self.tau*np.log(2)))
    self.nscint = nscint
    self.fse_tau = self.tau/(2*np.sqrt(nscint))
    fit_tau = float(fit["tauerr"][0])
    self.fse_dnu = self.dnu/(2*np.sqrt(nscint))
    fit_dnu = float(fit["dnuerr"][0])
    if verbose:
        print("\nFinite scintle errors (tau, dnu):\n", self.fse_tau, self.fse_dnu)
        print("\nFit errors (tau, dnu):\n", fit_tau, fit_dnu)
    self.tauerr = np.sqrt(fit_tau**2 + self.fse_tau**2)
    self.dnuerr = np.sqrt(fit_dnu**2 + self.fse_dnu**2)
    self.amp = float(fit["amp"][0])
    self.amperr = float(fit["amperr"][0])
    self.wn = 1 - self.amp
    if 'sim:mb2=' in self.name:
        self.wn = 0
    if alpha is None:
        self.talpha = float(fit["alpha"][0])
        self.talphaerr = float(fit["alphaerr"][0])
    else:
        self.talpha = alpha
        self.talphaerr = 0
    return


def fit_scint_params_cut(self, tcuts=0, fcuts=0, alpha=5/3, full_frame=False, nscale=5, weighted=True, bartlett=True,
                         verbose=False):
    """The 1-D ACF fit of every segment of ``cut_dyn(tcuts, fcuts)``: the segments are cut on the device, every segment's ACF
    (no mean subtracted, as ``cut_dyn``) goes into one stack ``[B, 2 fnum, 2 tnum]`` and ONE launch fits them all, each with its
    own ``bw = fnum df`` and ``tobs = tnum dt``.  Sets ``cut_tau, cut_dnu, cut_tauerr, cut_dnuerr`` (the fit's standard errors),
    ``cut_amp`` and ``cut_fit_status``, each ``[fcuts + 1, tcuts + 1]``; a segment whose fit did not converge holds NaN."""
    _lib_ready()
    nchan = len(self.freqs)  # re-define in case of trimming
    nsub = len(self.times)
    fnum = int(np.floor(nchan/(fcuts + 1)))
    tnum = int(np.floor(nsub/(tcuts + 1)))
    if fcuts < 0 or tcuts < 0 or fnum < 3 or tnum < 5:
        raise ValueError(f"fit_scint_params_cut: segments of {fnum} channels x {tnum} sub-integrations are too small "
                         "(at least 3 x 5)")
    dyn = np.asarray(self.dyn, dtype=float)
    if dyn.shape[0] < (fcuts + 1) * fnum or dyn.shape[1] < (tcuts + 1) * tnum:
        raise ValueError("fit_scint_params_cut: dyn is smaller than its frequency and time axes")
    if not np.all(np.isfinite(dyn[:(fcuts + 1) * fnum, :(tcuts + 1) * tnum])):
        raise ValueError("fit_scint_params_cut on the GPU needs a finite dynamic spectrum (run refill first)")
    nseg = (fcuts + 1) * (tcuts + 1)
    segs = segment_cut_device(device.to_device(dyn, torch.float64), fnum, tnum, fcuts + 1, tcuts + 1)
    acfs = acf_stack_device(segs, subtract_mean=False)
    fit = acf1d_fit_device(acfs, self.dt, self.df, fnum * self.df, tnum * self.dt, alpha=alpha, nscale=nscale,
                           full_frame=full_frame, weighted=weighted, bartlett=bartlett)
    shape = (fcuts + 1, tcuts + 1)
    self.cut_tau, self.cut_dnu, self.cut_amp = (fit[k].reshape(shape) for k in ("tau", "dnu", "amp"))
    self.cut_tauerr, self.cut_dnuerr = fit["tauerr"].reshape(shape), fit["dnuerr"].reshape(shape)
    self.cut_fit_status = fit["status"].reshape(shape)
    if verbose:
        print(f"fit_scint_params_cut: {int((self.cut_fit_status == FIT_CONVERGED).sum())} of {nseg} fits converged")
    return


# ----------------------------------------------------------------------------
# the approximate 2-D ACF fit: tau, dnu and the phase gradient (csrc/acf2d.hpp)
# ----------------------------------------------------------------------------
def acf_argmax_device(acf_stack_t):
    """``np.argmax`` of every ACF of a device stack [B, R, C] (first occurrence; NaN is never the maximum) as a host array."""
    _lib_ready()
    B, R, C = (int(v) for v in acf_stack_t.shape)
    idx = device.empty((B,), torch.int32)
    _lib.call("scint_acf_argmax", acf_stack_t, B, R, C, idx, device.stream_ptr())
    return idx.cpu().numpy().astype(np.int64)


def acf2d_window(nf, nt, loc, tau, dnu, dt, df, bw, tobs, nscale=5, full_frame=False):
    """The window of the 2-D fit as a rectangle ``(f0, nfw, t0, ntw)`` of ACF indices: dynspec.py:2733-2783 statement for
    statement, on index ranges instead of arrays (a ``range`` slices with NumPy's clipping).  ``loc`` is the flat index of the
    ACF's maximum, ``tau`` and ``dnu`` are the NO-FIT scales: the reference's locals are not updated by the 1-D fit.  Its
    frequency branch sets ``tmin = 0; tmax = nf`` and leaves ``fmin, fmax`` as they were; so does this."""
    tau, dnu = np.float64(tau), np.float64(dnu)
    wn_loc = divmod(int(loc), nt)

    fleft = wn_loc[0]
    fright = nf - wn_loc[0] - 1
    fmin = wn_loc[0] - min(fleft, fright)
    fmax = wn_loc[0] + min(fleft, fright) + 1

    tleft = wn_loc[1]
    tright = nt - wn_loc[1] - 1
    tmin = wn_loc[1] - min(tleft, tright)
    tmax = wn_loc[1] + min(tleft, tright) + 1

    rows = range(nf)[fmin:fmax]
    cols = range(nt)[tmin:tmax]

    if nscale is not None and not full_frame:
        ntau = nscale
        ndnu = nscale
        with np.errstate(divide="ignore", invalid="ignore"):
            if ntau > (tobs / tau):
                tmin = 0
                tmax = nt
            else:
                tframe = int(round(ntau * (tau / dt)))
                tmin = int(np.floor(len(cols) / 2)) - tframe
                tmax = int(np.floor(len(cols) / 2)) + tframe + 1

            if ndnu > (bw / dnu):
                tmin = 0
                tmax = nf
            else:
                fframe = int(round(ndnu * (dnu / df)))
                fmin = int(np.floor(len(rows) / 2)) - fframe
                fmax = int(np.floor(len(rows) / 2)) + fframe + 1
        rows = rows[fmin:fmax]
        cols = cols[tmin:tmax]
    return (rows[0] if len(rows) else 0, len(rows), cols[0] if len(cols) else 0, len(cols))


def acf2d_approx_fit_device(acf_stack_t, dt, df, bw, tobs, nsub=None, nchan=None, alpha=5/3, nscale=5, full_frame=False,
                            weighted=True, bartlett=True, phasegrad0=0.0, tau_vary_2d=True, tau_input=None, max_iter=200,
                            return_setup=False):
    """Fit the approximate 2-D ACF model (scint_models.py:123-161) to a window of every ACF of a device stack [B, R, C] float64 (or
    one ACF [R, C]): the reference's ``get_scint_params(method='acf2d_approx')`` (dynspec.py:2689-2842) for a batch.  Three
    launches: the 1-D fit (``acf1d_fit_device``, unchanged) for the start values -- its ``tau, dnu, amp`` where it converged, the
    no-fit values otherwise --, the ACFs' maxima (``scint_acf_argmax``), and the 2-D fit (``scint_acf2d_approx_fit``), one workgroup
    per problem.  The windows are computed here, on the host, from the NO-FIT scales (``acf2d_window``); the weights in the kernel.
    ``nsub``, ``nchan`` default to ``C // 2`` and ``R // 2``; ``alpha=None`` fits alpha from 5/3; ``phasegrad0`` and ``tau_input``
    are scalars or one value per problem; ``tau_vary_2d=False`` keeps tau at its start value.  Returns a dict of host arrays of
    length B: ``tau, dnu, amp, alpha, phasegrad``, their standard errors ``tauerr, ... phasegraderr`` (0 for a parameter that does
    not vary; everything NaN unless ``status == FIT_CONVERGED``), ``chisqr, redchi, niter, status``, the rectangle ``f0, nfw, t0,
    ntw``, ``nnz`` (non-zero weights), the start values ``tau_start, dnu_start, amp_start, alpha_start, phasegrad_start``, the
    maxima ``argmax`` and ``fit1d``, the 1-D fit's own dict.  ``return_setup`` adds ``y`` and ``w``: per problem the window's samples
    and weights [nfw, ntw].  ``FIT_BAD_WINDOW``: the reference's window has an even (or empty) side and is not centred."""
    _lib_ready()
    if acf_stack_t.dim() == 2:
        acf_stack_t = acf_stack_t[None]
    if acf_stack_t.dim() != 3:
        raise ValueError("acf2d_approx_fit_device: expected a stack of ACFs [B, R, C]")
    B, R, C = (int(v) for v in acf_stack_t.shape)
    ws = device.workspace_for("scint_acf2d_approx_fit", B, R, C, 1 if return_setup else 0)   # (checks the shape first)
    one = acf1d_fit_device(acf_stack_t, dt, df, bw, tobs, alpha=alpha, nscale=nscale, full_frame=full_frame, weighted=weighted,
                           bartlett=bartlett, max_iter=max_iter)
    bw_h = np.array(np.broadcast_to(np.asarray(bw, dtype=np.float64), (B,)))
    tobs_h = np.array(np.broadcast_to(np.asarray(tobs, dtype=np.float64), (B,)))
    locs = acf_argmax_device(acf_stack_t)

    ok1 = one["status"] == FIT_CONVERGED
    start = np.empty((B, 5))
    start[:, 0] = np.where(ok1, one["tau"], one["tau0"])
    start[:, 1] = np.where(ok1, one["dnu"], one["dnu0"])
    start[:, 2] = np.where(ok1, one["amp"], one["amp0"])
    start[:, 3] = 5/3 if alpha is None else float(alpha)
    start[:, 4] = np.broadcast_to(np.asarray(phasegrad0, dtype=np.float64), (B,))
    if tau_input is not None:
        start[:, 0] = np.broadcast_to(np.asarray(tau_input, dtype=np.float64), (B,))
    status_in = np.zeros(B, dtype=np.int32)
    rect = np.zeros((B, 4), dtype=np.int32)
    for b in range(B):
        if not (np.isfinite(one["tau0"][b]) and np.isfinite(one["dnu0"][b]) and np.all(np.isfinite(start[b]))):
            status_in[b] = FIT_NONFINITE_INPUT
            continue
        rect[b] = acf2d_window(R, C, locs[b], one["tau0"][b], one["dnu0"][b], dt, df, bw_h[b], tobs_h[b], nscale=nscale,
                               full_frame=full_frame)

    values, errors = device.empty((B, 5), torch.float64), device.empty((B, 5), torch.float64)
    stats = device.empty((B, 2), torch.float64)
    niter, status, nnz = (device.empty((B,), torch.int32) for _ in range(3))
    _lib.call("scint_acf2d_approx_fit", acf_stack_t, B, R, C, device.to_device(rect, torch.int32),
              device.to_device(start, torch.float64), device.to_device(status_in, torch.int32),
              device.to_device(bw_h, torch.float64), device.to_device(tobs_h, torch.float64),
              float(C // 2 if nsub is None else nsub), float(R // 2 if nchan is None else nchan), 1 if weighted else 0,
              1 if tau_vary_2d else 0, 1 if alpha is None else 0, int(max_iter), values, errors, stats, niter, status, nnz,
              1 if return_setup else 0, ws, ws.numel(), device.stream_ptr())
    values, errors, stats = (t.cpu().numpy() for t in (values, errors, stats))
    names = ("tau", "dnu", "amp", "alpha", "phasegrad")
    out = {k: values[:, i] for i, k in enumerate(names)}
    out.update({k + "err": errors[:, i] for i, k in enumerate(names)})
    out.update({k + "_start": start[:, i] for i, k in enumerate(names)})
    out.update(chisqr=stats[:, 0], redchi=stats[:, 1], niter=niter.cpu().numpy(), status=status.cpu().numpy(),
               nnz=nnz.cpu().numpy().astype(np.int64), argmax=locs, fit1d=one)
    out.update({k: rect[:, i].astype(np.int64) for i, k in enumerate(("f0", "nfw", "t0", "ntw"))})
    if return_setup:
        rows = np.array(ws[:16 * B * R * C].view(torch.float64).cpu().numpy()).reshape(B, 2, R * C)   # (the workspace is reused)
        good = [b for b in range(B) if out["status"][b] not in (FIT_BAD_WINDOW, FIT_NONFINITE_INPUT)]
        shape = {b: (int(rect[b, 1]), int(rect[b, 3])) for b in good}
        out["y"] = [rows[b, 0, :shape[b][0] * shape[b][1]].reshape(shape[b]) if b in shape else None for b in range(B)]
        out["w"] = [rows[b, 1, :shape[b][0] * shape[b][1]].reshape(shape[b]) if b in shape else None for b in range(B)]
    return out


def acf2d_approx_model_device(tdata, fdata, ydata, weights, tau, dnu, amp, alpha, phasegrad, tobs, bw):
    """``(ydata - model) * weights`` of ``scint_acf_model_2d_approx`` as a device tensor [nf, nt] (``scint_acf2d_approx_model``);
    ``ydata`` None: zeros, ``weights`` None: ones; host arrays are uploaded, device tensors are taken as they are."""
    _lib_ready()
    t = device.to_device(np.asarray(tdata, dtype=np.float64).reshape(-1), torch.float64) if not torch.is_tensor(tdata) else tdata
    f = device.to_device(np.asarray(fdata, dtype=np.float64).reshape(-1), torch.float64) if not torch.is_tensor(fdata) else fdata
    nt, nf = int(t.numel()), int(f.numel())

    def grid(a, what):
        if a is None or torch.is_tensor(a):
            a_t = a
        else:
            a_t = device.to_device(np.asarray(a, dtype=np.float64), torch.float64)
        if a_t is not None and tuple(a_t.shape) != (nf, nt):
            raise ValueError(f"scint_acf_model_2d_approx: {what} has shape {tuple(a_t.shape)}, expected ({nf}, {nt})")
        return a_t
    out = device.empty((nf, nt), torch.float64)
    _lib.call("scint_acf2d_approx_model", t, nt, f, nf, grid(ydata, "ydata"), grid(weights, "weights"), float(tau), float(dnu),
              float(amp), float(alpha), float(phasegrad), float(tobs), float(bw), out, device.stream_ptr())
    return out


def _set_fit_results(self, fit, alpha, method, verbose):
    """What the reference sets after a fit (dynspec.py:2953-3002) from problem 0 of a fit's dict."""
    self.scint_param_method = method
    self.tau = float(fit["tau"][0])
    self.dnu = float(fit["dnu"][0])
    self.tscat = 1/(2*np.pi*self.dnu)  # scattering timescale
    if self.dnu < self.df:
        print("Warning: Scint bandwidth < channel bandwidth.")
    # Compute finite scintle error
    nscint = (1 + 0.2*self.bw/(self.dnu)) * \
        (1 + 0.2*self.tobs/(self.tau*np.log(2)))
    self.nscint = nscint
    self.fse_tau = self.tau/(2*np.sqrt(nscint))
    fit_tau = float(fit["tauerr"][0])
    self.fse_dnu = self.dnu/(2*np.sqrt(nscint))
    fit_dnu = float(fit["dnuerr"][0])
    if verbose:
        print("\nFinite scintle errors (tau, dnu):\n", self.fse_tau, self.fse_dnu)
        print("\nFit errors (tau, dnu):\n", fit_tau, fit_dnu)
    self.tauerr = np.sqrt(fit_tau**2 + self.fse_tau**2)
    self.dnuerr = np.sqrt(fit_dnu**2 + self.fse_dnu**2)
    self.amp = float(fit["amp"][0])
    self.amperr = float(fit["amperr"][0])
    self.wn = 1 - self.amp
    if 'sim:mb2=' in self.name:
        self.wn = 0
    if alpha is None:
        self.talpha = float(fit["alpha"][0])
        self.talphaerr = float(fit["alphaerr"][0])
    else:
        self.talpha = alpha
        self.talphaerr = 0


def fit_scint_params_2d(self, alpha=5/3, full_frame=False, nscale=5, weighted=True, bartlett=True, tau_vary_2d=True,
                        tau_input=None, verbose=False):
    """Scintillation timescale, bandwidth and phase gradient from the approximate 2-D ACF fit, the reference's
    ``get_scint_params(method='acf2d_approx')`` (dynspec.py:2689-2842, 2953-3021), on the device: the batch of one of
    ``acf2d_approx_fit_device`` on ``self.acf``.  First the no-fit values and by-products of ``get_scint_params(method='nofit')``,
    then the 1-D fit for the start values; the phase gradient starts at ``acf_tilt`` when ``get_acf_tilt`` has set it with an
    error, at 0 otherwise.  A converged fit sets everything ``fit_scint_params`` sets, ``scint_param_method = 'acf2d_approx'``, and
    ``phasegrad`` (min/MHz), ``phasegraderr`` (the fit's standard error), ``fse_phasegrad`` and ``acf_model``: the model over the
    fit's window, left on the device until it is read.  Always sets ``scint_fit_status`` (``FIT_*``), ``scint_fit_redchi`` and
    ``scint_fit_niter``; no ``report``.  A fit that did not converge warns and keeps the 1-D fit's values where that converged
    (``scint_param_method = 'acf1d'``), the no-fit values otherwise."""
    self.get_scint_params(method='nofit', full_frame=full_frame, nscale=nscale)
    phasegrad0 = 0.0
    if hasattr(self, 'acf_tilt'):  # if have a confident measurement
        if self.acf_tilt_err is not None:
            phasegrad0 = self.acf_tilt
    cls = type(self)
    fit = acf2d_approx_fit_device(cls.acf.tensor(self), self.dt, self.df, self.bw, self.tobs, nsub=self.nsub, nchan=self.nchan,
                                  alpha=alpha, nscale=nscale, full_frame=full_frame, weighted=weighted, bartlett=bartlett,
                                  phasegrad0=phasegrad0, tau_vary_2d=tau_vary_2d, tau_input=tau_input)
    self.scint_fit_status = int(fit["status"][0])
    self.scint_fit_redchi = float(fit["redchi"][0])
    self.scint_fit_niter = int(fit["niter"][0])
    if self.scint_fit_status != FIT_CONVERGED:
        one = fit["fit1d"]
        kept = "1-D fit's" if one["status"][0] == FIT_CONVERGED else "no-fit"
        warnings.warn(f"fit_scint_params_2d: the fit did not converge ({FIT_STATUS_TEXT[self.scint_fit_status]} after "
                      f"{self.scint_fit_niter} iterations); the {kept} values are kept")
        if one["status"][0] == FIT_CONVERGED:
            _set_fit_results(self, one, alpha, 'acf1d', verbose)
        return
    _set_fit_results(self, fit, alpha, 'acf2d_approx', verbose)
    f0, nfw, t0, ntw = (int(fit[k][0]) for k in ("f0", "nfw", "t0", "ntw"))
    nr, nc = cls.acf.shape(self)
    tdata = np.linspace(-self.tobs, self.tobs, nc + 1)[:-1][t0:t0 + ntw]
    fdata = np.linspace(-self.bw, self.bw, nr + 1)[:-1][f0:f0 + nfw]
    model = acf2d_approx_model_device(tdata, fdata, None, None, self.tau, self.dnu, self.amp, float(fit["alpha"][0]),
                                      float(fit["phasegrad"][0]), self.tobs, self.bw)
    cls.acf_model.park(self, model.neg_())          # (the reference negates the residual of a zero ACF)
    self.phasegrad = float(fit["phasegrad"][0])
    fse_ph = self.phasegrad * np.sqrt((self.fse_dnu/self.dnu)**2 +
                                      (self.fse_tau/self.tau)**2)
    self.phasegraderr = float(fit["phasegraderr"][0])
    self.fse_phasegrad = fse_ph
    return


def fit_scint_params_2d_cut(self, tcuts=0, fcuts=0, alpha=5/3, full_frame=False, nscale=5, weighted=True, bartlett=True,
                            tau_vary_2d=True, verbose=False):
    """The approximate 2-D ACF fit of every segment of ``cut_dyn(tcuts, fcuts)``: cut, ACFs and fits on the device, ONE 1-D launch
    and ONE 2-D launch for all segments, each with its own ``bw = fnum df``, ``tobs = tnum dt``, ``nchan = fnum``, ``nsub = tnum``.
    Sets ``cut_tau, cut_dnu, cut_amp, cut_phasegrad``, their standard errors ``cut_tauerr, cut_dnuerr, cut_amperr,
    cut_phasegraderr`` and ``cut_fit_status``, each ``[fcuts + 1, tcuts + 1]``; a segment whose fit did not converge holds NaN."""
    _lib_ready()
    nchan = len(self.freqs)  # re-define in case of trimming
    nsub = len(self.times)
    fnum = int(np.floor(nchan/(fcuts + 1)))
    tnum = int(np.floor(nsub/(tcuts + 1)))
    if fcuts < 0 or tcuts < 0 or fnum < 3 or tnum < 5:
        raise ValueError(f"fit_scint_params_2d_cut: segments of {fnum} channels x {tnum} sub-integrations are too small "
                         "(at least 3 x 5)")
    dyn = np.asarray(self.dyn, dtype=float)
    if dyn.shape[0] < (fcuts + 1) * fnum or dyn.shape[1] < (tcuts + 1) * tnum:
        raise ValueError("fit_scint_params_2d_cut: dyn is smaller than its frequency and time axes")
    if not np.all(np.isfinite(dyn[:(fcuts + 1) * fnum, :(tcuts + 1) * tnum])):
        raise ValueError("fit_scint_params_2d_cut on the GPU needs a finite dynamic spectrum (run refill first)")
    nseg = (fcuts + 1) * (tcuts + 1)
    segs = segment_cut_device(device.to_device(dyn, torch.float64), fnum, tnum, fcuts + 1, tcuts + 1)
    acfs = acf_stack_device(segs, subtract_mean=False)
    fit = acf2d_approx_fit_device(acfs, self.dt, self.df, fnum * self.df, tnum * self.dt, nsub=tnum, nchan=fnum, alpha=alpha,
                                  nscale=nscale, full_frame=full_frame, weighted=weighted, bartlett=bartlett,
                                  tau_vary_2d=tau_vary_2d)
    shape = (fcuts + 1, tcuts + 1)
    for k in ("tau", "dnu", "amp", "phasegrad"):
        setattr(self, "cut_" + k, fit[k].reshape(shape))
        setattr(self, "cut_" + k + "err", fit[k + "err"].reshape(shape))
    self.cut_fit_status = fit["status"].reshape(shape)
    if verbose:
        print(f"fit_scint_params_2d_cut: {int((self.cut_fit_status == FIT_CONVERGED).sum())} of {nseg} fits converged")
    return
