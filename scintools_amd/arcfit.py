"""Arc normalisation of the secondary spectrum on the GPU: the numerics of

* ``Dynspec.scale_dyn(scale='lambda')``  dynspec.py:3928-3959  -> ``scint_spline_resample``
* ``Dynspec.scale_dyn(scale='velocity')``  dynspec.py:3961-4079  -> ``scint_spline_resample_rows``
* ``Dynspec.scale_dyn(scale='trapezoid')`` dynspec.py:4081-4128  -> ``scint_trap_scale``
* ``Dynspec.norm_sspec``                 dynspec.py:1920-2183  -> ``scint_norm_sspec`` +
                                                                   ``scint_masked_colavg`` (+ ``scint_row_nanmean``)
* ``Dynspec.fit_arc``                    dynspec.py:970-1313   -> ``scint_block_std`` + norm_sspec
* ``fit_arc_stack_device`` / ``Dynspec.fit_arc_cut``: fit_arc over a stack -> ``scint_arc_profile_batch`` + ``scint_arc_peak_fit``
  (there the 1-D profile logic runs on the device too, one wavefront per profile)

The O(rows x columns) work (cubic-spline resample of every time column, the per-delay-row
``np.interp`` resample, masked means) runs in HIP kernels; the 1-D profile logic of ``fit_arc``
(Savitzky-Golay smoothing, peak walk, parabola fit) stays on the host exactly as in the
reference.  Plotting, ``norm_sspec(velocity=True)`` / ``fit_arc(velocity=True)``, ``interp_nan`` (scipy griddata) and
``fit_spectrum`` (lmfit) are outside the accelerated path and raise ``NotImplementedError``.
"""
import collections
import ctypes
import warnings

import numpy as np
import scipy.constants as sc
import torch
from scipy.signal import savgol_filter

from . import _lib
from .device import empty, require_gpu, stream_ptr, to_device, workspace, workspace_for


def is_valid(array):
    """scint_utils.py:87-91."""
    return np.isfinite(array) * (~np.isnan(array))


# ----------------------------------------------------------------------------
# scale_dyn(scale='lambda')
# ----------------------------------------------------------------------------
def _spline_system(x):
    """Thomas factors of the not-a-knot cubic spline in second-derivative form on knots x
    (ascending, len >= 4): interior rows i = 1..n-2,
        a_i M[i-1] + b_i M[i] + c_i M[i+1] = 6 ((y[i+1]-y[i])/h[i] - (y[i]-y[i-1])/h[i-1]),
    with M[0] and M[n-1] eliminated through the not-a-knot conditions."""
    n = len(x)
    h = np.diff(x)
    a = np.zeros(n)
    b = np.zeros(n)
    c = np.zeros(n)
    a[1:n - 1] = h[:n - 2]
    b[1:n - 1] = 2 * (h[:n - 2] + h[1:n - 1])
    c[1:n - 1] = h[1:n - 1]
    b[1] = (h[0] + h[1]) * (h[0] + 2 * h[1]) / h[1]
    c[1] = (h[1]**2 - h[0]**2) / h[1]
    a[1] = 0.0
    b[n - 2] = (h[n - 2] + h[n - 3]) * (h[n - 2] + 2 * h[n - 3]) / h[n - 3]
    a[n - 2] = (h[n - 3]**2 - h[n - 2]**2) / h[n - 3]
    c[n - 2] = 0.0
    inv = np.zeros(n)
    sup = np.zeros(n)
    inv[1] = 1.0 / b[1]
    sup[1] = c[1] * inv[1]
    for i in range(2, n - 1):
        den = b[i] - a[i] * sup[i - 1]
        inv[i] = 1.0 / den
        sup[i] = c[i] * inv[i]
    end = np.array([(h[0] + h[1]) / h[1], -h[0] / h[1],
                    (h[n - 2] + h[n - 3]) / h[n - 3], -h[n - 2] / h[n - 3]])
    return h, a, inv, sup, end


_SPLINE_BLOCK_ROWS = 128


def _spline_blocks(sub, inv, sup, n):
    """Frequency blocking of the two Thomas sweeps.  An error e in the forward value d_{i-1}
    reaches d_i as -sub[i]*inv[i]*e, one in M[i+1] reaches M[i] as -sup[i]*e: both factors are
    ~0.27 on a uniform axis, so a block may start `warm` rows early from zero.  `warm` is the
    shortest run over which EVERY window of factors multiplies to < 1e-22 (far below the 1e-16
    rounding of the values themselves); if the axis is so irregular that this needs more than a
    few blocks' worth of rows, fall back to one block (the plain sequential sweep)."""
    rows = n - 2
    if rows < 4 * _SPLINE_BLOCK_ROWS:
        return 0, 0
    warm = _spline_warm(sub, inv, sup, n)
    if warm > 2 * _SPLINE_BLOCK_ROWS:
        return 0, 0
    return _SPLINE_BLOCK_ROWS, int(warm)


def _spline_warm(sub, inv, sup, n):
    """The shortest run of rows (a multiple of 8) over which every window of forward and of backward Thomas factors
    multiplies to < 1e-22: the warm-up after which a sweep started from zero has forgotten its start."""
    tiny = 1e-300                                              # an exact zero factor (uniform ends) decouples
    lf = np.log(np.maximum(np.abs(sub[2:n - 1] * inv[2:n - 1]), tiny))   # forward factors, rows 2..n-2
    lb = np.log(np.maximum(np.abs(sup[1:n - 2]), tiny))                   # backward factors, rows 1..n-3
    target = np.log(1e-22)
    warm = 0
    for lg in (lf, lb):
        c = np.concatenate([[0.0], np.cumsum(lg)])
        w = 8
        while w < len(lg) and np.max(c[w:] - c[:-w]) > target:
            w += 8
        warm = max(warm, w)
    return warm


def spline_resample_device(dyn_t, freqs, feq):
    """Cubic-spline (scipy ``interp1d(kind='cubic')``) resample of every time column of the
    device array dyn_t[nf, nt] from `freqs` to `feq`, rows flipped (dynspec.py:3948-3957)."""
    require_gpu()
    freqs = np.asarray(freqs, dtype=float)
    nf, nt = (int(v) for v in dyn_t.shape)
    if nf != len(freqs):
        raise ValueError("x and y arrays must be equal in length along interpolation axis.")
    if nf < 4:
        raise ValueError("The number of derivatives at boundaries does not match: expected 1, got 0+0")
    d = np.diff(freqs)
    reverse = 0
    if np.all(d > 0):
        x = freqs
    elif np.all(d < 0):
        x, reverse = freqs[::-1].copy(), 1
    else:                                   # interp1d sorts an unsorted axis
        order = np.argsort(freqs, kind="mergesort")
        x = freqs[order]
        dyn_t = dyn_t[to_device(order.astype(np.int64), torch.int64)].contiguous()
        if np.any(np.diff(x) <= 0):
            raise ValueError("Expect x to not have duplicates")
    feq = np.asarray(feq, dtype=float)
    if feq.min() < x[0] or feq.max() > x[-1]:
        raise ValueError("A value in x_new is outside the interpolation range.")
    h, sub, inv, sup, end = _spline_system(x)
    idx = np.clip(np.searchsorted(x, feq, side="right") - 1, 0, nf - 2)
    hk = h[idx]
    A = (x[idx + 1] - feq) / hk
    B = (feq - x[idx]) / hk
    coef = np.stack([A, B, (A**3 - A) * hk**2 / 6.0, (B**3 - B) * hk**2 / 6.0], axis=1)
    block_rows, warm = _spline_blocks(sub, inv, sup, nf)
    if block_rows:
        # A NaN/inf pixel must poison its whole time column, as scipy's sequential solve (and
        # the unblocked sweep) does; warm-started blocks would confine it to one block.  One
        # device reduction tells: the mean is non-finite iff some pixel is.
        m = ctypes.c_double()
        _lib.call("scint_mean", dyn_t, nf * nt, m, stream_ptr())
        if not np.isfinite(m.value):
            block_rows, warm = 0, 0
    ws = workspace.get(2 * 8 * nf * nt)
    out = empty((len(feq), nt), torch.float64)
    dev = lambda v: to_device(np.ascontiguousarray(v, dtype=float), torch.float64)
    h_t, sub_t, inv_t, sup_t, coef_t = dev(h), dev(sub), dev(inv), dev(sup), dev(coef)
    idx_t = to_device(idx.astype(np.int32), torch.int32)
    _lib.call("scint_spline_resample", dyn_t, nf, nt, reverse, h_t, sub_t, inv_t, sup_t, end, block_rows, warm, idx_t, coef_t,
              len(feq), out, ws, ws.numel(), stream_ptr())
    return out


def scale_dyn_lambda(self, spacing="auto"):
    """dyn(freq, t) -> dyn(lambda, t) in equal wavelength steps (dynspec.py:3928-3959).
    Sets ``lamdyn``, ``lam``, ``nlam``, ``dlam``."""
    freqs = np.array(self.freqs, dtype=float)
    lams = np.divide(sc.c, freqs * 10**6)
    step = np.abs(np.diff(lams))
    if spacing == "max":
        dlam = np.max(step)
    elif spacing == "median":
        dlam = np.median(step)
    elif spacing == "mean":
        dlam = np.mean(step)
    elif spacing == "min":
        dlam = np.min(step)
    elif spacing == "auto":
        dlam = (np.max(lams) - np.min(lams)) / len(freqs)
    else:
        raise UnboundLocalError("local variable 'dlam' referenced before assignment")
    lam_eq = np.arange(np.min(lams) + 1e-10, np.max(lams) - 1e-10, dlam)
    self.dlam = dlam
    feq = np.round(np.divide(sc.c, lam_eq) / 10**6, 6)
    if max(feq) > max(freqs):          # keep the rounded targets inside the band
        feq[np.argmax(feq)] = max(freqs)
    if min(feq) < min(freqs):
        feq[np.argmin(feq)] = min(freqs)
    dyn_t = to_device(np.asarray(self.dyn, dtype=float), torch.float64)
    lam_t = spline_resample_device(dyn_t, freqs, feq)
    type(self).lamdyn.park(self, lam_t)                 # stays in HBM until the host reads it
    self.lam = np.flipud(lam_eq)
    self.nlam = len(self.lam)


# ----------------------------------------------------------------------------
# scale_dyn(scale='velocity' | 'orbit')
# ----------------------------------------------------------------------------
_ROWS_LDS = 7680           # doubles of LDS one workgroup of the row kernel holds (csrc/scale.hpp, kRowsLds)
_ROWS_TRANSPOSE_MIN = 1 << 24     # pixels from which the blocked row resample goes through a transpose and the column kernel


def spline_rows_route(x):
    """How ``spline_resample_rows_device`` will sweep the ascending knots x: ('blocked', block, warm) when the time axis is cut
    into warm-started blocks, ('lds', 0, 0) for one sequential sweep per row inside LDS, ('workspace', 0, 0) for one sequential
    sweep per row through HBM (an axis that cannot be blocked and does not fit the tile).  A host-side decision from the
    Thomas factors alone (``_spline_blocks``); non-finite data turn 'blocked' into one of the other two at run time."""
    x = np.asarray(x, dtype=float)
    h, sub, inv, sup, end = _spline_system(x)
    block, warm = _spline_blocks(sub, inv, sup, len(x))
    if block:
        return "blocked", block, warm
    return ("lds" if len(x) + 1 <= _ROWS_LDS else "workspace"), 0, 0


def spline_resample_rows_device(dyn_t, x, xnew, force_one_block=False):
    """Cubic-spline (scipy ``interp1d(kind='cubic')``) resample of every ROW of the device array dyn_t[nf, nt] from the knots
    `x` (length nt) to `xnew` (dynspec.py:4062-4074): out[nf, len(xnew)] on the device.  `x` in any order without duplicates
    (interp1d sorts), `xnew` in any order inside the range of `x`.  ``force_one_block``: never block the time axis (the tests
    compare the two)."""
    require_gpu()
    x = np.asarray(x, dtype=float)
    nf, nt = (int(v) for v in dyn_t.shape)
    if nt != len(x):
        raise ValueError("x and y arrays must be equal in length along interpolation axis.")
    if nt < 4:
        raise ValueError("The number of derivatives at boundaries does not match: expected 1, got 0+0")
    d = np.diff(x)
    if not np.all(d > 0):                   # interp1d sorts an unsorted axis
        order = np.argsort(x, kind="mergesort")
        x = x[order]
        if np.any(np.diff(x) <= 0):
            raise ValueError("Expect x to not have duplicates")
        dyn_t = dyn_t[:, to_device(order.astype(np.int64), torch.int64)].contiguous()
    xnew = np.asarray(xnew, dtype=float)
    if xnew.ndim != 1 or len(xnew) < 1:
        raise ValueError("spline_resample_rows_device: xnew must be one-dimensional and not empty")
    if xnew.min() < x[0] or xnew.max() > x[-1]:
        raise ValueError("A value in x_new is outside the interpolation range.")
    unsort = None
    if np.any(np.diff(xnew) < 0):           # the kernel wants ascending targets: evaluate sorted, hand back in the caller's order
        order = np.argsort(xnew, kind="mergesort")
        unsort = np.empty_like(order)
        unsort[order] = np.arange(len(order))
        xnew = xnew[order]
    h, sub, inv, sup, end = _spline_system(x)
    idx = np.clip(np.searchsorted(x, xnew, side="right") - 1, 0, nt - 2)
    hk = h[idx]
    A = (x[idx + 1] - xnew) / hk
    B = (xnew - x[idx]) / hk
    coef = np.stack([A, B, (A**3 - A) * hk**2 / 6.0, (B**3 - B) * hk**2 / 6.0], axis=1)
    block, warm = (0, 0) if force_one_block else _spline_blocks(sub, inv, sup, nt)
    if block and nf * nt >= _ROWS_TRANSPOSE_MIN and len(xnew) <= 65535:
        # Measured at 4096 x 4096 (profiles/scale_timing.json): transpose, the column kernel and transpose back take 2.15 ms,
        # the row kernel 2.34 ms, with equal bits; at 1024 x 1024 the row kernel wins (0.73 against 0.80 ms).  The column kernel
        # writes its rows flipped, so it gets the targets reversed.
        out = spline_resample_device(dyn_t.t().contiguous(), x, xnew[::-1]).t().contiguous()
        return out if unsort is None else out[:, to_device(unsort.astype(np.int64), torch.int64)].contiguous()
    if block:
        # A NaN/inf pixel must poison its whole row, as scipy's sequential solve does; warm-started blocks would confine it.
        # One device reduction tells: the mean is non-finite iff some pixel is.
        m = ctypes.c_double()
        _lib.call("scint_mean", dyn_t, nf * nt, m, stream_ptr())
        if not np.isfinite(m.value):
            block, warm = 0, 0
    ws = workspace_for("scint_spline_resample_rows", nf, nt, block, warm)
    out = empty((nf, len(xnew)), torch.float64)
    dev = lambda v: to_device(np.ascontiguousarray(v, dtype=float), torch.float64)
    h_t, sub_t, inv_t, sup_t, coef_t = dev(h), dev(sub), dev(inv), dev(sup), dev(coef)
    idx_t = to_device(idx.astype(np.int32), torch.int32)
    _lib.call("scint_spline_resample_rows", dyn_t, nf, nt, h_t, sub_t, inv_t, sup_t, np.ascontiguousarray(end, dtype=float),
              block, warm, idx_t, coef_t, len(xnew), out, ws, ws.numel(), stream_ptr())
    if unsort is not None:
        out = out[:, to_device(unsort.astype(np.int64), torch.int64)].contiguous()
    return out


def velocity_grid(veff):
    """(vc_orig, vc_new) of dynspec.py:4056-4068: the cumulative effective velocity and its even grid with the reference's two
    clamps, in the precision of `veff` (the reference's is float128), then both as float64 -- which is what interp1d hands to
    its spline: make_interp_spline casts the knots, BSpline.__call__ the targets."""
    vc_orig = np.cumsum(veff)  # original cumulative sum of velocity
    vc_new = np.linspace(np.min(vc_orig), np.max(vc_orig), len(vc_orig))
    if max(vc_new) > max(vc_orig):
        vc_new[np.argmax(vc_new)] = max(vc_orig)
    if min(vc_new) < min(vc_orig):
        vc_new[np.argmin(vc_new)] = min(vc_orig)
    return np.asarray(vc_orig, dtype=np.float64), np.asarray(vc_new, dtype=np.float64)


def velocity_resample_device(dyn_t, veff):
    """Every channel of the device array dyn_t[nf, nt] resampled onto equal steps of the cumulative effective velocity
    (dynspec.py:4055-4074), for `veff` [nt] from any source (no ephemerides needed): out[nf, nt] on the device."""
    vc_orig, vc_new = velocity_grid(np.asarray(veff))
    return spline_resample_rows_device(dyn_t, vc_orig, vc_new)


def scale_dyn_velocity(self, pars=None, parfile=None, s=None, d=None, vism_ra=None, vism_dec=None, Omega=None, inc=None,
                       vism_zeta=None, zeta=None):
    """dyn(f, t) -> dyn(f, cumulative effective velocity) (dynspec.py:3961-4079).  Sets ``vdyn`` (and ``vlamdyn`` when ``lamdyn``
    is there), ``veff_ra``, ``veff_dec``.  The argument logic is the reference's, line by line; the ephemeris functions are
    looked up in ``scint_utils`` when called, as the reference imports them then."""
    from . import scint_models, scint_utils

    if pars is None and parfile is None:
        raise ValueError('Requires dictionary of parameters ' +
                         'or .par file for velocity calculation')
    if parfile is not None:
        pars = scint_utils.read_par(parfile)
    cls = type(self)
    mjd = np.asarray(self.mjd, dtype=np.longdouble) + \
        np.asarray(self.times, dtype=np.longdouble) / 86400

    ssb_delays = scint_utils.get_ssb_delay(mjd, pars['RAJ'], pars['DECJ'])
    mjd += np.divide(ssb_delays, 86400)  # add ssb delay
    vearth_ra, vearth_dec = scint_utils.get_earth_velocity(mjd, pars['RAJ'], pars['DECJ'])
    true_anomaly = scint_utils.get_true_anomaly(mjd, pars)
    if 's' not in pars.keys():
        if s is None:
            raise ValueError('Requires screen distance s in ' +
                             'parameter dictionary, or as input')
        pars['s'] = s
    if 'd' not in pars.keys():
        if d is None:
            raise ValueError('Requires pulsar distance d in ' +
                             'parameter dictionary, or as input')
        pars['d'] = d
    if 'KIN' not in pars.keys():
        if inc is None:
            raise ValueError('Requires inclination angle (KIN) in ' +
                             'parameter dictionary, or as input inc')
        pars['KIN'] = inc
    if 'KOM' not in pars.keys():
        if Omega is None:
            raise ValueError('Requires ascending node (KOM) in ' +
                             'parameter dictionary, or as input Omega')
        pars['KOM'] = Omega

    veff_ra, veff_dec, vp_ra, vp_dec = scint_models.effective_velocity_annual(pars, true_anomaly, vearth_ra, vearth_dec, mjd=mjd)
    veff2, veff_ra, veff_dec = effective_velocity_squared(pars, veff_ra, veff_dec, vism_ra=vism_ra, vism_dec=vism_dec,
                                                          vism_zeta=vism_zeta, zeta=zeta)
    veff = np.sqrt(veff2)
    vc_orig, vc_new = velocity_grid(veff)
    dyn_t = to_device(np.asarray(self.dyn, dtype=float), torch.float64)
    v_t = spline_resample_rows_device(dyn_t, vc_orig, vc_new)
    if cls.lamdyn.present(self):
        vlam_t = spline_resample_rows_device(cls.lamdyn.tensor(self), vc_orig, vc_new)
    self.veff_ra = veff_ra
    self.veff_dec = veff_dec
    cls.vdyn.park(self, v_t)                            # stay in HBM until the host reads them
    if cls.lamdyn.present(self):
        cls.vlamdyn.park(self, vlam_t)


def effective_velocity_squared(pars, veff_ra, veff_dec, vism_ra=None, vism_dec=None, vism_zeta=None, zeta=None):
    """veff**2 along the anisotropy, or isotropic, with the ISM velocity removed (dynspec.py:4018-4053).  Returns
    (veff2, veff_ra, veff_dec); the two components are changed IN PLACE where the reference does so (``-=`` on arrays)."""
    # anisotropic case
    if ('zeta' in pars.keys()) or (zeta is not None):
        if 'zeta' in pars.keys():
            zeta = pars['zeta']
        zeta *= np.pi / 180  # make radians
        # vism in direction of anisotropy
        if 'vism_zeta' in pars.keys():
            vism_zeta = pars['vism_zeta']
            veff2 = (veff_ra * np.sin(zeta) + veff_dec * np.cos(zeta) - vism_zeta)**2
        elif vism_zeta is not None:
            veff2 = (veff_ra * np.sin(zeta) + veff_dec * np.cos(zeta) - vism_zeta)**2
        else:  # no vism_zeta: RA and DEC velocities, if any
            if 'vism_ra' in pars.keys():
                veff_ra -= pars['vism_ra']
            elif vism_ra is not None:
                veff_ra -= vism_ra
            if 'vism_dec' in pars.keys():
                veff_dec -= pars['vism_dec']
            elif vism_dec is not None:
                veff_dec -= vism_dec
            veff2 = (veff_ra * np.sin(zeta) + veff_dec * np.cos(zeta))**2
    # isotropic case
    else:
        if 'vism_ra' in pars.keys():
            veff_ra -= pars['vism_ra']
        elif vism_ra is not None:
            veff_ra -= vism_ra
        if 'vism_dec' in pars.keys():
            veff_dec -= pars['vism_dec']
        elif vism_dec is not None:
            veff_dec -= vism_dec
        veff2 = veff_ra**2 + veff_dec**2
    return veff2, veff_ra, veff_dec


# ----------------------------------------------------------------------------
# scale_dyn(scale='trapezoid')
# ----------------------------------------------------------------------------
def trapezoid_keep(freqs, times):
    """Samples every channel keeps (dynspec.py:4111-4118): ``len(np.argwhere(times <= maxtime))`` for ascending times."""
    nf = len(freqs)
    scalefrac = 1 / (max(freqs) / min(freqs))
    timestep = max(times) * (1 - scalefrac) / (nf + 1)  # time step
    maxtime = max(times) - (nf - (np.arange(nf) + 1)) * timestep
    return np.searchsorted(times, maxtime, side="right").astype(np.int32)


def trap_scale_device(dyn, freqs, times, window='hanning', window_frac=0.1):
    """The trapezoid rescale of the HOST array dyn[nf, nt] (dynspec.py:4081-4128) in one device pass: every channel's time axis
    stretched in proportion to its frequency, zeros after.  Returns the device tensor [nf, nt]."""
    from .dynspec import get_window
    dyn = np.asarray(dyn, dtype=float)
    nf, nt = dyn.shape
    freqs = np.asarray(freqs, dtype=float)
    times = np.ascontiguousarray(times, dtype=float)
    if len(freqs) != nf or len(times) != nt:
        raise ValueError(f"trap_scale_device: dyn is {nf} x {nt}, freqs has {len(freqs)} and times {len(times)} entries")
    if np.any(np.diff(times) < 0):
        raise ValueError("trap_scale_device: times must be ascending")
    cw_t = sw_t = None
    if window is not None:
        cw, sw = get_window(nt, nf, window=window, frac=window_frac)       # ValueError for an unknown window
    require_gpu()
    if window is not None:
        cw_t, sw_t = to_device(cw, torch.float64), to_device(sw, torch.float64)
    mean = float(np.mean(dyn))
    out = empty((nf, nt), torch.float64)
    _lib.call("scint_trap_scale", to_device(dyn, torch.float64), nf, nt, mean, cw_t, sw_t, to_device(times, torch.float64),
              to_device(trapezoid_keep(freqs, times), torch.int32), out, stream_ptr())
    return out


def scale_dyn_trapezoid(self, window='hanning', window_frac=0.1):
    """Sets ``trapdyn`` (dynspec.py:4081-4128); it stays in HBM until the host reads it."""
    type(self).trapdyn.park(self, trap_scale_device(self.dyn, self.freqs, self.times, window=window, window_frac=window_frac))


# ----------------------------------------------------------------------------
# norm_sspec
# ----------------------------------------------------------------------------
def _sspec_for(self, lamsteps):
    """Device tensor of the dB spectrum norm_sspec / fit_arc work on and its delay axis,
    computing the spectrum if absent (dynspec.py:1993-2023, 1069-1090)."""
    cls = type(self)
    if lamsteps:
        if not cls.lamsspec.present(self):
            self.calc_sspec(lamsteps=True)
        return cls.lamsspec.tensor(self), self.beta
    if not cls.sspec.present(self):
        self.calc_sspec()
    return cls.sspec.tensor(self), self.tdel


def norm_sspec(self, eta=None, delmax=None, plot=False, startbin=1, maxnormfac=5, minnormfac=0, cutmid=0,
               lamsteps=True, scrunched=True, plot_fit=True, ref_freq=1400, velocity=False, numsteps=None,
               filename=None, display=True, weighted=True, unscrunched=True, logsteps=False, powerspec=True,
               interp_nan=False, fit_spectrum=False, powerspec_cut=False, figsize=(9, 9),
               subtract_artefacts=False, dpi=200):
    """Normalise the Doppler axis by the arc curvature and scrunch in delay
    (dynspec.py:1920-2183).  Sets ``normsspecavg``, ``normsspec`` (2-D masked array, copied
    from the device on first access), ``normsspec_tdel``, ``normsspec_fdop``, ``powerspectrum``,
    ``weights``, ``mask``."""
    if plot:
        raise NotImplementedError("plotting is outside the accelerated hot path")
    if velocity:
        raise NotImplementedError("the arc normalisation of the velocity-scaled spectrum (vsspec / vlamsspec) is not ported yet")
    if interp_nan:
        raise NotImplementedError("interp_nan (scipy.interpolate.griddata) is outside the accelerated path")
    if fit_spectrum:
        raise NotImplementedError("fit_spectrum needs lmfit and is outside the accelerated path")
    require_gpu()
    if not hasattr(self, "tdel"):
        self.calc_sspec(lamsteps=lamsteps)
    delmax = np.max(self.tdel) if delmax is None else delmax
    held = getattr(self, "_arc_dev_cache", None)          # a running fit_arc: (tensor, yaxis, lamsteps)
    if held is not None and held[2] == bool(lamsteps):
        sspec_t, yaxis = held[0], held[1]
    else:
        sspec_t, yaxis = _sspec_for(self, lamsteps)
    if eta is None:
        if not hasattr(self, "betaeta" if lamsteps else "eta"):
            self.fit_arc(lamsteps=lamsteps, delmax=delmax, plot=plot, startbin=startbin)
        eta = self.betaeta if lamsteps else self.eta
    elif not lamsteps:                                  # dynspec.py:2033-2038
        c = 299792458.0
        beta_to_eta = c * 1e6 / ((ref_freq * 10**6)**2)
        eta = eta / (self.freq / ref_freq)**2
        eta = eta * beta_to_eta
    eta = float(eta)
    fdop = np.asarray(self.fdop, dtype=float)
    if np.any(np.diff(fdop) <= 0):
        raise ValueError("norm_sspec: the fdop axis must be ascending")
    ind = int(np.argmin(abs(self.tdel - delmax)))
    nrow_all, nc = (int(v) for v in sspec_t.shape)
    row0 = int(startbin)
    nr = len(range(nrow_all)[startbin:ind])
    tdel = np.array(yaxis[startbin:ind], dtype=float)
    if nr < 1:
        raise IndexError("index -1 is out of bounds for axis 0 with size 0")
    cut_lo = int(nc / 2 - np.floor(cutmid / 2))
    cut_hi = int(nc / 2 + np.floor(cutmid / 2))
    fdop_t = to_device(fdop, torch.float64)
    yaxis_t = to_device(np.asarray(yaxis, dtype=float), torch.float64)
    offset_t = None
    if subtract_artefacts:                              # dynspec.py:2057-2063
        colsel = (np.abs(fdop) > 0.9 * np.max(fdop)).astype(np.uint8)
        colsel_t = to_device(colsel, torch.uint8)
        resp_t = empty((nr,), torch.float64)
        _lib.call("scint_row_nanmean", sspec_t, nc, nc, row0, nr, colsel_t, cut_lo, cut_hi, resp_t, stream_ptr())
        resp = resp_t.cpu().numpy()
        resp -= np.median(resp)
        offset_t = to_device(resp, torch.float64)
    maxfdop = maxnormfac * np.sqrt(tdel[-1] / eta)
    if maxfdop > max(fdop):
        maxfdop = max(fdop)
    nfdop = 2 * len(fdop[abs(fdop) <= maxfdop]) if numsteps is None else numsteps
    if nfdop % 2 != 0:
        nfdop += 1
    fdoplin = None
    if logsteps:                                        # dynspec.py:2076-2083
        fdoplin = np.abs(np.linspace(-maxnormfac, maxnormfac, int(nfdop)))
        fdop_pos = 10**np.linspace(np.log10(np.min(fdoplin)), np.log10(np.max(fdoplin)), int(nfdop / 2))
        fdopnew = np.concatenate((-np.flip(fdop_pos, axis=0), fdop_pos))
    else:
        fdopnew = np.linspace(-maxnormfac, maxnormfac, int(nfdop))
    if minnormfac > 0:
        fdopnew = fdopnew[np.argwhere(np.abs(fdopnew) > minnormfac)]
        if logsteps:
            raise ValueError("Mask and data not compatible: logsteps with minnormfac > 0 "
                             "(the reference fails the same way, dynspec.py:2117)")
    # the first (smallest-delay) row selects the fewest Doppler bins; np.interp raises on none
    if not np.any(abs(fdop) <= maxnormfac * np.sqrt(np.min(tdel) / eta)):
        raise ValueError("array of sample points is empty")
    x = np.ascontiguousarray(np.ravel(fdopnew), dtype=float)
    nx = len(x)
    x_t = to_device(x, torch.float64)
    xlin_t = to_device(np.ascontiguousarray(fdoplin, dtype=float), torch.float64) if logsteps else None
    norm_t = empty((nr, nx), torch.float64)
    mask_t = empty((nr, nx), torch.uint8)
    pow_t = empty((nr,), torch.float64)
    _lib.call("scint_norm_sspec", sspec_t, nc, nc, fdop_t, yaxis_t, row0, nr, eta, maxnormfac, cut_lo, cut_hi, offset_t, x_t, xlin_t,
              nx, norm_t, mask_t, pow_t, stream_ptr())
    self.powerspectrum = np.ma.masked_invalid(pow_t.cpu().numpy())
    xdata = np.sqrt(tdel)
    ydata = np.sqrt(tdel) * self.powerspectrum
    xdata = xdata[~np.isnan(xdata)]
    ydata = ydata[~np.isnan(ydata)]
    alpha = -11 / 3                                     # dynspec.py:2133-2137
    index = np.argmin(np.abs(xdata - 10))
    amp = ydata[index] * xdata[index]**-alpha
    wn = np.min(ydata)
    arc_spectrum = amp * xdata**alpha
    if weighted:
        self.weights = 10 * np.log10(arc_spectrum)
    else:
        self.weights = np.ones(np.shape(arc_spectrum))
    wts = np.ma.filled(np.ma.array(self.weights, dtype=float), np.nan).squeeze()
    if wts.shape != (nr,):
        raise ValueError("Length of weights not compatible with specified axis.")
    rowsel_t = None
    if powerspec_cut:                                   # dynspec.py:2171-2178
        rowsel = np.zeros(nr, dtype=np.uint8)
        rowsel[np.argwhere(np.ma.filled(arc_spectrum > wn, False)).ravel()] = 1
        rowsel_t = to_device(rowsel, torch.uint8)
    w_t = to_device(np.ascontiguousarray(wts), torch.float64)
    ws = workspace_for("scint_masked_colavg", nr, nx)
    avg_t = empty((nx,), torch.float64)
    none_t = empty((nx,), torch.uint8)
    _lib.call("scint_masked_colavg", norm_t, mask_t, nr, nx, w_t, rowsel_t, avg_t, none_t, ws, ws.numel(), stream_ptr())
    # a column with no unmasked entry is masked, with numpy.ma's 0.0 left under the mask
    self.normsspecavg = np.ma.array(avg_t.cpu().numpy(), mask=none_t.cpu().numpy().astype(bool))
    self._normsspec_dev = (norm_t, mask_t)
    self._normsspec_host = None
    self._mask_host = None
    self.normsspec_tdel = tdel
    self.normsspec_fdop = fdopnew
    return


def normsspec_host(self):
    """Materialise the 2-D normalised spectrum (masked array) from the device on first use."""
    if getattr(self, "_normsspec_host", None) is None:
        dev = getattr(self, "_normsspec_dev", None)
        if dev is None:
            raise AttributeError("'Dynspec' object has no attribute 'normsspec'")
        self._normsspec_host = np.ma.array(dev[0].cpu().numpy(), mask=dev[1].cpu().numpy().astype(bool))
    return self._normsspec_host


# ----------------------------------------------------------------------------
# parabola fits (scint_models.py:300-347)
# ----------------------------------------------------------------------------
def fit_parabola(x, y):
    """Peak of the least-squares parabola and its error (scint_models.py:300-326)."""
    ptp = np.ptp(x)
    x = x * (1000 / ptp)
    params, pcov = np.polyfit(x, y, 2, cov=True)
    yfit = params[0] * np.power(x, 2) + params[1] * x + params[2]
    errors = [np.absolute(pcov[i][i])**0.5 for i in range(len(params))]
    peak = -params[1] / (2 * params[0])
    peak_error = np.sqrt((errors[1]**2) * ((1 / (2 * params[0]))**2) + (errors[0]**2) * ((params[1] / 2)**2))
    return yfit, peak * (ptp / 1000), peak_error * (ptp / 1000)


def fit_log_parabola(x, y):
    """The same in log(x) (scint_models.py:329-347)."""
    logx = np.log(x)
    ptp = np.ptp(logx)
    x = logx * (1000 / ptp)
    yfit, peak, peak_error = fit_parabola(x, y)
    frac_error = peak_error / peak
    peak = np.e**(peak * ptp / 1000)
    return yfit, peak, frac_error * peak


# ----------------------------------------------------------------------------
# the peak of one power-against-curvature profile (dynspec.py:1190-1265)
# ----------------------------------------------------------------------------
ArcPeak = collections.namedtuple("ArcPeak", "eta etaerr etaerr2 pk i1 i2 spec eta_array smooth")


class ArcWindowError(IndexError):
    """``_arc_peak(strict=True)``: the fit window [pk - i1, pk + i2) leaves the profile or holds fewer than 4 points."""


def _arc_peak(spec, etafrac, etamin, etamax, constraint=(0, np.inf), nsmooth=5, low_power_diff=-1, high_power_diff=-0.5,
              noise=0.0, noise_error=True, log_parabola=False, strict=False):
    """What ``fit_arc`` does with one folded profile `spec` over the inverse normalised Doppler axis `etafrac` (both in the order
    of ``normsspec_fdop >= 0``): drop non-finite entries, flip, ``etaArray = etamin etafrac**2 < etamax``, smooth, find the peak
    inside `constraint`, walk down to `low_power_diff` / `high_power_diff`, fit the parabola to the unsmoothed points and take the
    errors.  Returns ``ArcPeak``: eta, etaerr (the noise walk's when `noise_error`, else the fit's), etaerr2 (the fit's) -- not
    yet divided by sqrt 2 --, pk, i1, i2 (the fit window is [pk - i1, pk + i2)), the kept `spec` and `eta_array`, `smooth`.
    The lines and the exceptions are the reference's.  ``strict``: where the reference's window would start at a negative index
    (it wraps) or hold fewer than 4 points, raise ``ArcWindowError`` -- what the batched fit reports as status 3.  That exception and
    the forward-parabola ``ValueError`` carry ``pk``, ``i1`` and ``i2``."""
    filt_ind = is_valid(spec)
    spec = np.flip(spec[filt_ind], axis=0)
    etafrac_array_avg = np.flip(etafrac[filt_ind], axis=0)
    etaArray = etamin * etafrac_array_avg**2
    keep = np.argwhere(etaArray < etamax)
    etaArray = etaArray[keep].squeeze()
    spec = spec[keep].squeeze()
    smooth = savgol_filter(spec, nsmooth, 1)
    indrange = np.argwhere((etaArray > constraint[0]) * (etaArray < constraint[1]))
    pk = np.argmin(np.abs(smooth - np.max(smooth[indrange])))
    max_power = smooth[pk]
    power, i1 = max_power, 1                 # dynspec.py:1222-1233
    while power > max_power + low_power_diff and pk + i1 < len(smooth) - 1:
        i1 += 1
        power = smooth[pk - i1]
    power, i2 = max_power, 1
    while power > max_power + high_power_diff and pk + i2 < len(smooth) - 1:
        i2 += 1
        power = smooth[pk + i2]
    fit_pk, fit_i1, fit_i2 = int(pk), int(i1), int(i2)
    if strict and (pk - i1 < 0 or i1 + i2 < 4):
        err = ArcWindowError(f"the fit window [{pk - i1}, {pk + i2}) leaves the profile or holds fewer than 4 points")
        err.pk, err.i1, err.i2 = fit_pk, fit_i1, fit_i2
        raise err
    xdata = etaArray[int(pk - i1):int(pk + i2)]
    ydata = spec[int(pk - i1):int(pk + i2)]
    if log_parabola:
        yfit, eta, etaerr = fit_log_parabola(xdata, ydata)
    else:
        yfit, eta, etaerr = fit_parabola(xdata, ydata)
    if np.mean(np.gradient(np.diff(yfit))) > 0:
        err = ValueError('Fit returned a forward parabola.')
        err.pk, err.i1, err.i2 = fit_pk, fit_i1, fit_i2       # (where it happened, for a caller that maps it to a status)
        raise err
    etaerr2 = etaerr                         # error from the parabola fit
    if noise_error:                          # dynspec.py:1250-1265
        power, i1 = max_power, 1
        while power > (max_power - noise) and (pk - i1 > 1):
            power = smooth[pk - i1]
            i1 += 1
        power, i2 = max_power, 1
        while power > (max_power - noise) and (pk + i2 < len(smooth) - 1):
            i2 += 1
            power = smooth[pk + i2]
        etaerr = np.abs(etaArray[int(pk - i1)] - etaArray[int(pk + i2)]) / 2
    return ArcPeak(eta, etaerr, etaerr2, fit_pk, fit_i1, fit_i2, spec, etaArray, smooth)


# ----------------------------------------------------------------------------
# fit_arc
# ----------------------------------------------------------------------------
def fit_arc(self, asymm=False, plot=False, delmax=None, numsteps=1e4, startbin=3, cutmid=3, lamsteps=False,
            etamax=None, etamin=None, low_power_diff=-1, high_power_diff=-0.5, ref_freq=1400,
            constraint=[0, np.inf], nsmooth=5, efac=1, filename=None, noise_error=True, display=True,
            figN=None, log_parabola=False, logsteps=False, plot_spec=False, fit_spectrum=False,
            subtract_artefacts=False, figsize=(9, 9), dpi=200, velocity=False, weighted=False):
    """Find the arc curvature with maximum power along it (dynspec.py:970-1313).  Sets
    ``eta / etaerr / etaerr2`` (or ``betaeta...`` with lamsteps, ``..._left / _right`` with
    asymm), ``noise``, ``eta_array``, ``norm_sspec_avg*``, ``prob_eta_peak*``, ``norm_delmax``."""
    if plot or plot_spec:
        raise NotImplementedError("plotting is outside the accelerated hot path")
    if velocity:
        raise NotImplementedError("the arc normalisation of the velocity-scaled spectrum (vsspec / vlamsspec) is not ported yet")
    require_gpu()
    if not hasattr(self, "tdel"):
        self.calc_sspec()
    delmax = np.max(self.tdel) if delmax is None else delmax
    sspec_t, yaxis_full = _sspec_for(self, lamsteps)
    yaxis = np.array(yaxis_full, dtype=float)
    ind = int(np.argmin(abs(self.tdel - delmax)))
    ymax = self.beta[ind]                                # dynspec.py:1092 (needs a lamsteps spectrum)
    nr, nc = (int(v) for v in sspec_t.shape)
    # noise of the spectrum: std of the outer half in delay, centre columns excluded (dynspec.py:1097-1101)
    c_hi = int(nc / 2 + np.ceil(cutmid / 2))
    c_lo = int(nc / 2 - np.floor(cutmid / 2))
    std_t = empty((1,), torch.float64)
    ws = workspace.get(8 * 1032)
    _lib.call("scint_block_std", sspec_t, nc, nc, int(nr / 2), nr, c_lo, c_hi, std_t, ws, ws.numel(), stream_ptr())
    noise = float(std_t.cpu().numpy()[0])
    yaxis = yaxis[0:ind]
    noise = np.sqrt(np.sum(np.power(noise, 2))) / np.sqrt(len(yaxis) * 2)
    self.noise = noise
    if etamax is None:
        etamax = ymax / ((self.fdop[1] - self.fdop[0]) * cutmid)**2
    if etamin is None:
        etamin = (yaxis[1] - yaxis[0]) * startbin / (max(self.fdop))**2
    try:
        len(etamin)
        etamin_array = np.array(etamin).squeeze()
        etamax_array = np.array(etamax).squeeze()
    except TypeError:
        etamin_array = np.array([etamin])
        etamax_array = np.array([etamax])
    sqrt_eta_all = np.linspace(np.sqrt(np.min(etamin_array)), np.sqrt(np.max(etamax_array)), int(numsteps))
    self._arc_dev_cache = (sspec_t, yaxis_full, bool(lamsteps))
    try:
        for iarc in range(len(etamin_array)):
            if len(etamin_array) != 1:
                etamin = etamin_array.squeeze()[iarc]
                etamax = etamax_array.squeeze()[iarc]
            if not lamsteps:                             # dynspec.py:1140-1148
                c = 299792458.0
                beta_to_eta = c * 1e6 / ((ref_freq * 10**6)**2)
                etamax = etamax / (self.freq / ref_freq)**2
                etamax = etamax * beta_to_eta
                etamin = etamin / (self.freq / ref_freq)**2
                etamin = etamin * beta_to_eta
                constraint = constraint / (self.freq / ref_freq)**2
                constraint = constraint * beta_to_eta
            sqrt_eta = sqrt_eta_all[(sqrt_eta_all <= np.sqrt(etamax)) * (sqrt_eta_all >= np.sqrt(etamin))]
            # normalised spectrum with etamin as the normalisation: 1/fdop_norm**2 scans eta
            self.norm_sspec(eta=etamin, delmax=delmax, plot=False, startbin=startbin, maxnormfac=1,
                            cutmid=cutmid, lamsteps=lamsteps, scrunched=True, logsteps=logsteps,
                            plot_fit=False, numsteps=len(sqrt_eta), fit_spectrum=fit_spectrum,
                            subtract_artefacts=subtract_artefacts, velocity=velocity, weighted=weighted)
            norm_sspec_avg_all = self.normsspecavg.squeeze()
            etafrac_array = self.normsspec_fdop
            ind1 = np.argwhere(etafrac_array >= 0)
            ind2 = np.argwhere(etafrac_array < 0)
            if asymm:
                profiles = [np.array(norm_sspec_avg_all[ind1]), np.flip(norm_sspec_avg_all[ind2], axis=0)]
            else:
                profiles = [np.add(norm_sspec_avg_all[ind1], np.flip(norm_sspec_avg_all[ind2], axis=0)) / 2]
            etafrac_array_avg_orig = 1 / etafrac_array[ind1].squeeze()
            for dummy, spec in enumerate(profiles):
                # np.array() drops the mask and keeps what numpy.ma left under it, as the reference does
                peak = _arc_peak(np.array(spec).squeeze(), etafrac_array_avg_orig, etamin, etamax, constraint=constraint,
                                 nsmooth=nsmooth, low_power_diff=low_power_diff, high_power_diff=high_power_diff, noise=noise,
                                 noise_error=noise_error, log_parabola=log_parabola)
                eta, etaerr, etaerr2, spec, etaArray = peak.eta, peak.etaerr, peak.etaerr2, peak.spec, peak.eta_array
                self.eta_array = etaArray
                sigma = self.noise * efac
                prob = 1 / (sigma * np.sqrt(2 * np.pi)) * np.exp(-0.5 * ((spec - np.max(spec)) / sigma)**2)
                if asymm:
                    if dummy == 0:
                        self.norm_sspec_avg1, self.prob_eta_peak1 = spec, prob
                    else:
                        self.norm_sspec_avg2, self.prob_eta_peak2 = spec, prob
                else:
                    self.norm_sspec_avg, self.prob_eta_peak = spec, prob
                if iarc == 0:                            # save primary (dynspec.py:1283-1313)
                    stem = "betaeta" if lamsteps else "eta"
                    side = ("_left" if dummy == 0 else "_right") if asymm else ""
                    setattr(self, stem + side, eta)
                    setattr(self, stem + "err" + side, etaerr / np.sqrt(2))
                    setattr(self, stem + "err2" + side, etaerr2 / np.sqrt(2))
            self.norm_delmax = delmax
    finally:
        self._arc_dev_cache = None


# ----------------------------------------------------------------------------
# fit_arc over a stack of spectra (csrc/arcbatch.hpp)
# ----------------------------------------------------------------------------
ARC_OK, ARC_SHORT, ARC_NO_RANGE, ARC_WINDOW, ARC_FORWARD, ARC_NONFINITE = range(6)
ARC_STATUS_TEXT = {ARC_OK: "ok", ARC_SHORT: "fewer than max(nsmooth, 4) points kept", ARC_NO_RANGE: "no point inside the constraint",
                   ARC_WINDOW: "the fit window leaves the profile or holds fewer than 4 points",
                   ARC_FORWARD: "the fit returned a forward parabola", ARC_NONFINITE: "non-finite result"}


def arc_profile_stack_device(sspec_stack_t, fdop_t, yaxis_t, row0, nr, eta, maxnormfac, cut_lo, cut_hi, noise_lo, noise_hi, x_t):
    """``scint_arc_profile_batch`` on device tensors: (avg [B, nx], empty [B, nx] uint8, noise [B]), problem b with the bits of
    ``scint_norm_sspec`` + ``scint_masked_colavg`` (unit weights) and of ``scint_block_std`` over the outer half in delay."""
    B, R, nc = (int(v) for v in sspec_stack_t.shape)
    nx = int(x_t.shape[0])
    avg_t = empty((B, nx), torch.float64)
    none_t = empty((B, nx), torch.uint8)
    noise_t = empty((B,), torch.float64)
    ws = workspace_for("scint_arc_profile_batch", B, R, nc, nr)
    _lib.call("scint_arc_profile_batch", sspec_stack_t, B, R, nc, nc, fdop_t, yaxis_t, row0, nr, eta, maxnormfac, cut_lo, cut_hi,
              noise_lo, noise_hi, x_t, nx, avg_t, none_t, noise_t, ws, ws.numel(), stream_ptr())
    return avg_t, none_t, noise_t


def arc_peak_fit_device(avg_t, noise_t, noise_div, x_t, etamin, etamax, constraint=(0, np.inf), nsmooth=5, low_power_diff=-1,
                        high_power_diff=-0.5, noise_error=True, log_parabola=False, asymm=False):
    """``scint_arc_peak_fit`` on device tensors: (profile [PP, nx/2], val [4, PP], dec [5, PP]) on the device, PP = P or 2 P."""
    from scipy.signal import savgol_coeffs
    P, nx = (int(v) for v in avg_t.shape)
    npp = P * (2 if asymm else 1)
    coef_t = to_device(np.ascontiguousarray(savgol_coeffs(nsmooth, 1), dtype=float), torch.float64)
    prof_t = empty((npp, nx // 2), torch.float64)
    val_t = empty((4, npp), torch.float64)
    dec_t = empty((5, npp), torch.int32)
    ws = workspace_for("scint_arc_peak_fit", P, nx, int(bool(asymm)))
    _lib.call("scint_arc_peak_fit", avg_t, P, nx, noise_t, noise_div, x_t, etamin, etamax,
              np.array([constraint[0], constraint[1]], dtype=float), nsmooth, coef_t, low_power_diff, high_power_diff,
              int(bool(noise_error)), int(bool(log_parabola)), int(bool(asymm)), prof_t, val_t, dec_t, ws, ws.numel(), stream_ptr())
    return prof_t, val_t, dec_t


def fit_arc_stack_device(sspec_stack_t, fdop, yaxis, etamin=None, etamax=None, delmax=None, numsteps=1e4, startbin=3, cutmid=3,
                         constraint=(0, np.inf), nsmooth=5, efac=1, noise_error=True, log_parabola=False, logsteps=False,
                         asymm=False, low_power_diff=-1, high_power_diff=-0.5, out_device=False, weighted=False,
                         subtract_artefacts=False, fit_spectrum=False):
    """``fit_arc`` for every spectrum of the device stack ``sspec_stack_t [B, R, nc]`` (dB) with the shared axes `fdop` [nc]
    (ascending) and `yaxis` [R]: two kernels (``scint_arc_profile_batch``, ``scint_arc_peak_fit``), seven launches and two small
    read-backs however large B is.  Curvatures are in units of ``yaxis / fdop**2``: there is no reference-frequency conversion.

    The defaults are ``fit_arc``'s formulas, with ``ymax = yaxis[ind]``, ``ind = argmin |yaxis - delmax|``:
    ``etamax = ymax / ((fdop[1] - fdop[0]) cutmid)**2`` (``cutmid = 0`` without ``etamax`` is a ValueError) and
    ``etamin = (yaxis[1] - yaxis[0]) startbin / max(fdop)**2``; the normalised Doppler grid is the one ``fit_arc`` ->
    ``norm_sspec(eta=etamin, maxnormfac=1, numsteps=len(sqrt_eta))`` builds, ``logsteps`` included.

    Returns a dict: ``eta, etaerr, etaerr2`` ([B], or [B, 2] with ``asymm``: left, right; both errors divided by sqrt 2 as the
    attributes of ``fit_arc`` are, NaN where ``status`` is not 0), ``status`` (``ARC_*``), ``noise`` [B], ``pk, i1, i2, kept``
    (the peak index, the fit window [pk - i1, pk + i2) and the number of points of each profile), ``eta_array`` (the curvature
    grid of a profile without non-finite entries; a profile that lost some has ``kept`` points on its own shorter grid) and
    ``profile`` ([B(, 2), nx/2], the folded power-against-curvature curves, NaN after the ``kept`` points; a device tensor with
    ``out_device``).  ``efac`` is accepted for ``fit_arc``'s signature; the probability curves it scales are not formed.

    Outside the batched path, each a ``NotImplementedError``: ``weighted=True``, ``subtract_artefacts``, ``fit_spectrum`` and
    array-valued ``etamin`` / ``etamax`` (several arcs)."""
    if weighted:
        raise NotImplementedError("fit_arc_stack_device: weighted=True (the power-spectrum weights of norm_sspec) is outside the batched path")
    if subtract_artefacts:
        raise NotImplementedError("fit_arc_stack_device: subtract_artefacts is outside the batched path")
    if fit_spectrum:
        raise NotImplementedError("fit_spectrum needs lmfit and is outside the accelerated path")
    if np.ndim(etamin) > 0 or np.ndim(etamax) > 0:
        raise NotImplementedError("fit_arc_stack_device: array-valued etamin / etamax (several arcs) are outside the batched path")
    if not isinstance(sspec_stack_t, torch.Tensor) or sspec_stack_t.dim() != 3:
        raise ValueError("fit_arc_stack_device: the stack must be a device tensor [B, R, nc]")
    if sspec_stack_t.dtype != torch.float64 or not sspec_stack_t.is_contiguous():
        raise ValueError("fit_arc_stack_device: the stack must be a contiguous float64 tensor")
    B, R, nc = (int(v) for v in sspec_stack_t.shape)
    if B < 1 or B > 65535:
        raise ValueError(f"fit_arc_stack_device: 1 to 65535 spectra in a stack ({B} given)")
    fdop = np.asarray(fdop, dtype=float)
    yaxis = np.asarray(yaxis, dtype=float)
    if fdop.shape != (nc,) or yaxis.shape != (R,) or R < 2 or nc < 2:
        raise ValueError(f"fit_arc_stack_device: spectra of {R} x {nc} with {len(yaxis)} delays and {len(fdop)} Doppler bins")
    if np.any(np.diff(fdop) <= 0):
        raise ValueError("fit_arc_stack_device: the fdop axis must be ascending")
    nsmooth = int(nsmooth)
    if nsmooth < 3 or nsmooth % 2 == 0:
        raise ValueError("fit_arc_stack_device: nsmooth must be odd and at least 3")
    if cutmid == 0 and etamax is None:
        raise ValueError("fit_arc_stack_device: cutmid = 0 needs an explicit etamax (the default divides by cutmid)")
    require_gpu()
    delmax = np.max(yaxis) if delmax is None else delmax
    ind = int(np.argmin(abs(yaxis - delmax)))
    ymax = yaxis[ind]
    if ind < 1:
        raise ValueError("fit_arc_stack_device: delmax leaves no delay row")
    noise_hi = int(nc / 2 + np.ceil(cutmid / 2))                 # fit_arc's noise columns (dynspec.py:1097-1101)
    noise_lo = int(nc / 2 - np.floor(cutmid / 2))
    noise_div = float(np.sqrt(len(yaxis[0:ind]) * 2))
    if etamax is None:
        etamax = ymax / ((fdop[1] - fdop[0]) * cutmid)**2
    if etamin is None:
        etamin = (yaxis[1] - yaxis[0]) * startbin / (max(fdop))**2
    etamin, etamax = float(etamin), float(etamax)
    sqrt_eta_all = np.linspace(np.sqrt(etamin), np.sqrt(etamax), int(numsteps))
    sqrt_eta = sqrt_eta_all[(sqrt_eta_all <= np.sqrt(etamax)) * (sqrt_eta_all >= np.sqrt(etamin))]
    # the grid of norm_sspec(eta=etamin, maxnormfac=1, numsteps=len(sqrt_eta)) (dynspec.py:2065-2091)
    row0 = int(startbin)
    nr = len(range(R)[startbin:ind])
    if nr < 1:
        raise IndexError("index -1 is out of bounds for axis 0 with size 0")
    tdel = yaxis[startbin:ind]
    cut_lo = int(nc / 2 - np.floor(cutmid / 2))
    cut_hi = int(nc / 2 + np.floor(cutmid / 2))
    nfdop = len(sqrt_eta)
    if nfdop % 2 != 0:
        nfdop += 1
    if logsteps:
        fdoplin = np.abs(np.linspace(-1, 1, int(nfdop)))
        fdop_pos = 10**np.linspace(np.log10(np.min(fdoplin)), np.log10(np.max(fdoplin)), int(nfdop / 2))
        fdopnew = np.concatenate((-np.flip(fdop_pos, axis=0), fdop_pos))
    else:
        fdopnew = np.linspace(-1, 1, int(nfdop))
    if not np.any(abs(fdop) <= np.sqrt(np.min(tdel) / etamin)):
        raise ValueError("array of sample points is empty")
    x = np.ascontiguousarray(fdopnew, dtype=float)
    half = len(x) // 2
    if len(x) < 2 or not (x[half - 1] < 0 <= x[half]):
        raise ValueError("fit_arc_stack_device: the normalised Doppler grid is not symmetric")
    fdop_t, yaxis_t, x_t = (to_device(v, torch.float64) for v in (fdop, yaxis, x))
    avg_t, none_t, noise_t = arc_profile_stack_device(sspec_stack_t, fdop_t, yaxis_t, row0, nr, etamin, 1.0, cut_lo, cut_hi,
                                                      noise_lo, noise_hi, x_t)
    prof_t, val_t, dec_t = arc_peak_fit_device(avg_t, noise_t, noise_div, x_t, etamin, etamax, constraint=constraint,
                                               nsmooth=nsmooth, low_power_diff=low_power_diff, high_power_diff=high_power_diff,
                                               noise_error=noise_error, log_parabola=log_parabola, asymm=asymm)
    val = val_t.cpu().numpy()                                    # the two read-backs
    dec = dec_t.cpu().numpy()
    shape = (B, 2) if asymm else (B,)
    eta_array = etamin * np.flip(1 / x[half:], axis=0)**2
    out = {"eta": val[0].reshape(shape), "etaerr": val[1].reshape(shape), "etaerr2": val[2].reshape(shape),
           "noise": val[3].reshape(shape)[:, 0].copy() if asymm else val[3].copy(),
           "pk": dec[0].reshape(shape), "i1": dec[1].reshape(shape), "i2": dec[2].reshape(shape), "kept": dec[3].reshape(shape),
           "status": dec[4].reshape(shape), "eta_array": eta_array[eta_array < etamax]}
    prof_t = prof_t.view(shape + (half,))
    out["profile"] = prof_t if out_device else prof_t.cpu().numpy()
    return out


def fit_arc_cut(self, tcuts=0, fcuts=0, **kwargs):
    """``fit_arc`` of every segment of ``cut_dyn(tcuts, fcuts)`` in one batched call (``fit_arc_stack_device`` and its keywords) on
    ``cutsspec`` as it sits in HBM; ``cut_dyn`` runs first if ``cutsspec`` is absent or belongs to another cut.  The axes are a
    segment's ``fdop`` and ``tdel`` as ``calc_sspec(input_dyn=segment)`` returns them, so curvatures are in us / mHz**2 without a
    reference-frequency conversion.  Sets ``cut_eta, cut_etaerr, cut_etaerr2, cut_arc_status`` ([fcuts + 1, tcuts + 1], with
    ``asymm`` [.., 2]: left, right), ``cut_arc_noise`` [fcuts + 1, tcuts + 1], ``cut_eta_array`` and ``cut_arc_profile`` (the folded profiles [fcuts + 1, tcuts + 1(, 2), nx/2]:
    a device tensor, 164 MB for 4096 segments, or a NumPy array with ``out_device=False``); warns once with the count when a
    segment's status is not 0 (its values are NaN)."""
    cls = type(self)
    fnum = int(np.floor(len(self.freqs) / (fcuts + 1)))
    tnum = int(np.floor(len(self.times) / (tcuts + 1)))
    if fcuts < 0 or tcuts < 0 or fnum < 2 or tnum < 5:
        raise ValueError(f"fit_arc_cut: segments of {fnum} channels x {tnum} sub-integrations are too small (at least 2 x 5)")
    nrfft = int(2**(np.ceil(np.log2(fnum)) + 1))
    ncfft = int(2**(np.ceil(np.log2(tnum)) + 1))
    shape = (fcuts + 1, tcuts + 1)
    if not cls.cutsspec.present(self) or tuple(cls.cutsspec.shape(self)) != shape + (nrfft // 2, ncfft):
        self.cut_dyn(tcuts=tcuts, fcuts=fcuts)
    fdop = np.arange(int(-ncfft / 2), int(ncfft / 2)) * (1e3 / (ncfft * self.dt))      # calc_sspec's axes for a segment
    tdel = np.arange(0, int(nrfft / 2)) / (nrfft * self.df)
    stack_t = cls.cutsspec.tensor(self).view(shape[0] * shape[1], nrfft // 2, ncfft)
    kwargs.setdefault("out_device", True)                        # unless asked for, the profiles stay in HBM
    fit = fit_arc_stack_device(stack_t, fdop, tdel, **kwargs)
    full = shape + ((2,) if kwargs.get("asymm") else ())
    self.cut_eta, self.cut_etaerr, self.cut_etaerr2 = (fit[k].reshape(full) for k in ("eta", "etaerr", "etaerr2"))
    self.cut_arc_status = fit["status"].reshape(full)
    self.cut_arc_noise = fit["noise"].reshape(shape)
    self.cut_eta_array = fit["eta_array"]
    self.cut_arc_profile = fit["profile"].reshape(full + (-1,))
    bad = int(np.count_nonzero(self.cut_arc_status))
    if bad:
        warnings.warn(f"fit_arc_cut: {bad} of {self.cut_arc_status.size} arc fits did not succeed (cut_arc_status; their values are NaN)")


# ----------------------------------------------------------------------------
# calc_scattered_image
# ----------------------------------------------------------------------------
_SCAT_REGION = 2048        # knots one workgroup of pass A solves (csrc/scatim.hpp, kScatRegion)
_SCAT_MAX_WARM = 256


def _check_spline_axes(x, y, shape):
    """What scipy's RectBivariateSpline(x, y, z) (kx = ky = 3) raises for these axes and this z.shape, in its order."""
    if not np.all(np.diff(x) > 0.0):
        raise ValueError('x must be strictly increasing')
    if not np.all(np.diff(y) > 0.0):
        raise ValueError('y must be strictly increasing')
    if not x.size == shape[0]:
        raise ValueError('x dimension of z must have same number of elements as x')
    if not y.size == shape[1]:
        raise ValueError('y dimension of z must have same number of elements as y')
    if x.size < 4 or y.size < 4:
        # FITPACK's own error (its type is private to scipy): let scipy raise it, on zeros of the offending size
        from scipy.interpolate import RectBivariateSpline
        mx, my = min(x.size, 4), min(y.size, 4)
        RectBivariateSpline(np.arange(float(mx)), np.arange(float(my)), np.zeros((mx, my)))
        raise ValueError("RectBivariateSpline needs at least 4 points per axis")      # not reached with the scipy in use


def scattered_image_device(sspec_t, rows, cols, tdel, fdop, eta, sampling):
    """image[nx, nx] of ``calc_scattered_image`` from the dB spectrum on the device, cropped to rows [rows[0], rows[1]) and columns
    [cols[0], cols[1]), with the cropped knots tdel / fdop (any strictly increasing spacing): the interpolating bicubic
    not-a-knot spline of 10**(sspec/10) evaluated through eta, times fdop_y, mirrored (``scint_scattered_image``).  Returns
    (image, fdop_x).  The Thomas factors, the intervals and the abscissae are host NumPy, handed over as data."""
    require_gpu()
    tdel = np.ascontiguousarray(tdel, dtype=float)
    fdop = np.ascontiguousarray(fdop, dtype=float)
    nrow, n = int(rows[1] - rows[0]), int(cols[1] - cols[0])
    _check_spline_axes(tdel, fdop, (max(nrow, 0), max(n, 0)))
    if sspec_t.stride(1) != 1:
        sspec_t = sspec_t.contiguous()
    nx, ny = 2 * sampling + 1, sampling + 1
    fdop_x = np.linspace(-max(fdop), max(fdop), nx)
    fdop_y = np.linspace(0, max(fdop), ny)
    # Doppler axis: factors in the form pass A consumes, intervals and weights of the clamped abscissae (bispev clamps)
    h, sub, inv, sup, end = _spline_system(fdop)
    row_sys = np.zeros((4, n))
    row_sys[0, :n - 1] = 1.0 / h
    row_sys[1] = 6.0 * inv
    row_sys[2] = -sub * inv
    row_sys[3] = sup
    row_warm = 0
    if n - 2 > _SCAT_REGION:
        row_warm = _spline_warm(sub, inv, sup, n) + 2
        if row_warm > _SCAT_MAX_WARM:
            raise ValueError("calc_scattered_image: the Doppler axis is too irregular for the chunked spline solve")
    xe = np.clip(fdop_x, fdop[0], fdop[-1])
    idx = np.clip(np.searchsorted(fdop, xe, side="right") - 1, 0, n - 2)
    hk = h[idx]
    a = (fdop[idx + 1] - xe) / hk
    b = (xe - fdop[idx]) / hk
    coef = np.stack([a, b, (a**3 - a) * hk**2 / 6.0, (b**3 - b) * hk**2 / 6.0], axis=1)
    # delay axis: the factors of scint_spline_resample's sweeps
    hc, subc, invc, supc, endc = _spline_system(tdel)
    col_sys = np.zeros((4, nrow))
    col_sys[0, :nrow - 1] = hc
    col_sys[1], col_sys[2], col_sys[3] = subc, invc, supc
    block_rows, col_warm = _spline_blocks(subc, invc, supc, nrow)
    dev = lambda v: to_device(np.ascontiguousarray(v, dtype=float), torch.float64)
    tdel_t, row_sys_t, coef_t, col_sys_t, fx_t, fy_t = dev(tdel), dev(row_sys), dev(coef), dev(col_sys), dev(fdop_x), dev(fdop_y)
    idx_t = to_device(idx.astype(np.int32), torch.int32)
    ws = workspace_for("scint_scattered_image", nrow, sampling)
    image_t = empty((nx, nx), torch.float64)
    flag_t = empty((1,), torch.int32)
    end, endc = np.ascontiguousarray(end, dtype=float), np.ascontiguousarray(endc, dtype=float)
    _lib.call("scint_scattered_image", sspec_t, sspec_t.stride(0), int(rows[0]), int(rows[1]), int(cols[0]), int(cols[1]), tdel_t,
              row_sys_t, end, int(row_warm), idx_t, coef_t, col_sys_t, endc, int(block_rows), int(col_warm), fx_t, fy_t, eta,
              int(sampling), image_t, flag_t,
              ws, ws.numel(), stream_ptr())
    image = image_t.cpu().numpy()
    if int(flag_t.cpu().numpy()[0]):
        # a NaN or inf in 10**(sspec/10): FITPACK's global solve spreads it over every coefficient and scipy returns NaN
        # everywhere without raising; the blocked device solve would confine it, so the flag decides
        image[:] = np.nan
    return image, fdop_x


def calc_scattered_image(self, input_sspec=None, input_eta=None, input_fdop=None, input_tdel=None, sampling=64,
                         lamsteps=False, trap=False, ref_freq=1400, clean=True, s=None, veff=None, d=None, fit_arc=True,
                         plot_fit=False, plot=False, plot_log=True, use_angle=False, use_spatial=False):
    """The scattered image B(theta_x, theta_y) from the secondary spectrum and the arc curvature (dynspec.py:3412-3582), assuming
    the primary arc; the x axis is aligned with the velocity.  Sets ``scattered_image`` ([2 sampling + 1] squared, float64) and
    ``scattered_image_ax``.  The host lines are the reference's, in its order; the spline interpolation of 10**(sspec/10)
    (scipy RectBivariateSpline) runs on the device, on a parked spectrum without a host copy.

    * ``input_sspec`` may be a NumPy array or a device tensor (dB), with ``input_fdop`` / ``input_tdel``.
    * ``clean`` is accepted and does nothing: the reference's block fills a copy of ``sspec`` that nothing reads afterwards
      (``linsspec`` is formed before it) and swallows its own exceptions.
    * When the curvature is so small that the arc stays inside the delay range at the first Doppler bin (``flim == 0``) the
      reference crops the delay rows and takes ``tdel = fdop[:tlim]`` -- the Doppler axis -- as their knots (dynspec.py:3521).
      That is reproduced as it stands, wrong axis included.
    * A NaN or +inf pixel in the cropped 10**(sspec/10) gives an all-NaN image and no exception, as scipy does; -inf dB is an exact 0.
    * ``trap``, ``plot`` and ``plot_fit`` raise ``NotImplementedError``; the default ``plot_log=True`` only warns that nothing is drawn.
    """
    if plot or plot_fit:
        raise NotImplementedError("plotting is outside the accelerated hot path")
    if trap:
        raise NotImplementedError("the scattered image of the trapezoid-scaled spectrum (trapsspec) is not ported yet")
    cls = type(self)
    if input_sspec is None:
        if lamsteps:
            if not cls.lamsspec.present(self):
                self.calc_sspec(lamsteps=lamsteps)
            sspec_t = cls.lamsspec.tensor(self)
        else:
            if not cls.sspec.present(self):
                self.calc_sspec(lamsteps=lamsteps)
            sspec_t = cls.sspec.tensor(self)
        fdop = np.array(self.fdop)
        tdel = np.array(self.tdel)
    else:
        sspec_t = to_device(input_sspec, torch.float64)
        fdop = input_fdop
        tdel = input_tdel
    nf, nt = len(fdop), len(tdel)
    if input_eta is None and fit_arc:
        if not hasattr(self, 'betaeta') and not hasattr(self, 'eta'):
            self.fit_arc(lamsteps=lamsteps, log_parabola=True)
        if lamsteps:
            c = 299792458.0  # m/s
            beta_to_eta = c * 1e6 / ((ref_freq * 1e6)**2)
            eta = self.betaeta / (self.freq / ref_freq)**2     # correct for freq
            eta = eta * beta_to_eta
        else:
            eta = self.eta
    else:
        if input_eta is None:
            eta = tdel[nt - 1] / fdop[nf - 1]**2
        else:
            eta = input_eta
    # crop sspec to desired region: Python's slice semantics on the spectrum's own shape and on the axes
    nrow_all, ncol_all = (int(v) for v in sspec_t.shape)
    flim = next(i for i, delay in enumerate(eta * fdop**2) if delay < np.max(tdel))
    if flim == 0:
        tlim = next(i for i, delay in enumerate(tdel) if delay > eta * fdop[0] ** 2)
        rows = range(nrow_all)[:tlim]
        cols = range(ncol_all)
        tdel = fdop[:tlim]
    else:
        rows = range(nrow_all)
        cols = range(ncol_all)[flim - int(0.02 * nf):nf - flim + int(0.02 * nf)]
        fdop = fdop[flim - int(0.02 * nf):nf - flim + int(0.02 * nf)]
    scat_im, xyaxes = scattered_image_device(sspec_t, (rows.start, max(rows.stop, rows.start)),
                                             (cols.start, max(cols.stop, cols.start)), tdel, fdop, eta, sampling)
    if plot_log:
        warnings.warn("scintools_amd: calc_scattered_image does not draw the image (plot_log=True); "
                      "it is in self.scattered_image")
    self.scattered_image = scat_im
    self.scattered_image_ax = xyaxes
