"""Drop-in for the hot-path entry points of ``scintools.dynspec.Dynspec``.

Only what the hot path needs is here: a ``Dynspec`` that is built from an object
carrying the reference's attributes (a ``scint_sim.Simulation``, a ``BasicDyn``, a
reference ``Dynspec``, or plain arrays) with

* ``calc_sspec`` (dynspec.py:3584-3748) -> HIP kernels (``scint_sspec``);
* ``prep_thetatheta`` / ``thetatheta_single`` / ``fit_thetatheta``
  (dynspec.py:1348-1763): the chunked curvature search -- chunking, eta grids, edges and
  the global eta ~ nu**-2 fit stay on the host exactly as in the reference, every
  chunk's conjugate spectrum + eta sweep runs on the GPU (``ththmod.single_search``).

* ``scale_dyn(scale='lambda')``, ``norm_sspec``, ``fit_arc`` (dynspec.py:3928-3959,
  1920-2183, 970-1313): the arc-curvature search on the secondary spectrum that supplies
  ``prep_thetatheta`` with its default curvature bounds (``scintools_amd/arcfit.py``).

* ``calc_scattered_image`` (dynspec.py:3412-3582): the secondary spectrum mapped through the curvature onto the sky; the
  bicubic spline interpolation runs on the GPU (``scint_scattered_image``).

* ``trim_edges``, ``crop_dyn``, ``zap``, ``refill``, ``correct_dyn``, ``auto_processing`` (dynspec.py:259-328, 3816-3870,
  3273-3410, 422-440): the cleaning chain; medians, the median filter, gap interpolation and the truncated SVD run on the GPU
  (``scintools_amd/clean.py``).  ``inpaint`` (not in the reference) is the biharmonic fill of ``refill``'s default method, for
  any mask, by conjugate gradients on the GPU.

* ``calc_acf``, ``get_scint_params(method='nofit')``, ``get_acf_tilt``, ``cut_dyn`` (dynspec.py:3750-3814, 2470-2648,
  2283-2413, 3158-3271): the ACF stays in HBM; the scintillation scales, the ACF tilt and the segment stacks read what they need
  from the device (``scintools_amd/scintpar.py``).

* ``scale_dyn(scale='velocity' | 'orbit' | 'trapezoid')`` and ``calc_sspec(velocity=True | trap=True)`` (dynspec.py:3961-4128):
  one cubic spline per channel along time (``scint_spline_resample_rows``) and the trapezoid stretch (``scint_trap_scale``).

The lmfit-driven fits and plotting are out of scope.
"""
import functools
import os
import warnings

import numpy as np
import scipy.constants as sc
import torch

from . import _lib, arcfit, clean, psrflux, scintpar, units
from . import ththmod as thth
from .device import DeviceBacked, empty, require_gpu, stream_ptr, to_device, workspace_for
from .device import workspace  # noqa: F401  (kept as a module attribute: the host-interpreter tests swap it per module)

_WINDOWS = {"hanning": np.hanning, "hamming": np.hamming,
            "blackman": np.blackman, "bartlett": np.bartlett}


def _walks_columns(a):
    """True when ``np.copy(a[window])`` (order='K') lays the window out column by column, so that NumPy's sums over the copy
    walk it that way: the first axis has the smaller stride.  Not only Fortran-contiguous arrays: a crop of a transposed array
    is neither C- nor F-contiguous and is copied column-major too."""
    return a.ndim == 2 and abs(a.strides[0]) < abs(a.strides[1])


def get_window(nt, nf, window="hanning", frac=0.1):
    """Edge tapers with a flat middle (scint_utils.py:810-832); host NumPy,
    the multiply is fused into the first FFT pass on the device."""
    try:
        fn = _WINDOWS[window.lower()]
    except KeyError:
        raise ValueError(f"Window unknown: {window!r}")
    cw = fn(np.floor(frac * nt))
    sw = fn(np.floor(frac * nf))
    chan_window = np.insert(cw, int(np.ceil(len(cw) / 2)), np.ones([nt - len(cw)]))
    subint_window = np.insert(sw, int(np.ceil(len(sw) / 2)), np.ones([nf - len(sw)]))
    return chan_window, subint_window


@functools.lru_cache(maxsize=32)
def _window_tables(nt, nf, window, frac, device):
    """The two taper vectors in HBM, kept per (shape, window, device): a repeated calc_sspec (the
    per-chunk loops of fit_thetatheta / the arc fits) re-uses them instead of rebuilding and
    uploading them on every call."""
    if window is None:
        return None, None
    cw, sw = get_window(nt, nf, window=window, frac=frac)
    return to_device(cw, torch.float64), to_device(sw, torch.float64)


@functools.lru_cache(maxsize=32)
def _postdark_tables(nrfft, ncfft, device):
    """Post-darkening factors of the prewhitened spectrum (dynspec.py:3700-3714), per device."""
    fd = np.array(list(range(int(-ncfft / 2), int(ncfft / 2))))
    td = np.array(list(range(0, int(nrfft / 2))))
    return (to_device(np.power(np.sin(np.multiply(sc.pi / ncfft, fd)), 2), torch.float64),
            to_device(np.power(np.sin(np.multiply(sc.pi / nrfft, td)), 2), torch.float64))


def sspec_device(dyn_t, prewhite=False, halve=True, window="hanning", window_frac=0.1, out=None):
    """Secondary spectrum of a device dynamic spectrum [nf, nt] float64 -> device
    tensor in dB, shape [(nrfft/2 if halve else nrfft), ncfft] (dynspec.py:3665-3721).
    ``out``: a contiguous device tensor of that shape to write into (a slice of a stack)."""
    require_gpu()
    nf, nt = (int(v) for v in dyn_t.shape)
    nrfft = int(2 ** (np.ceil(np.log2(nf)) + 1))      # dynspec.py:3677
    ncfft = int(2 ** (np.ceil(np.log2(nt)) + 1))      # dynspec.py:3678
    if prewhite and not halve:
        raise RuntimeError("Cannot apply prewhite to full frame")   # dynspec.py:3717
    wt, wf = _window_tables(nt, nf, window, window_frac, torch.cuda.current_device())
    pd_fd, pd_td = _postdark_tables(nrfft, ncfft, torch.cuda.current_device()) if prewhite else (None, None)
    ws = workspace_for("scint_sspec", nf, nt)
    shape = (nrfft // 2 if halve else nrfft, ncfft)
    if out is None:
        out = empty(shape, torch.float64)
    elif tuple(out.shape) != shape:
        raise ValueError(f"sspec_device: out has shape {tuple(out.shape)}, the spectrum {shape}")
    _lib.call("scint_sspec", dyn_t, nf, nt, wt, wf, 1 if prewhite else 0, 1 if halve else 0, pd_fd, pd_td, out, ws, ws.numel(),
              stream_ptr())
    return out


def sspec_stack_device(stack_t, prewhite=False, halve=True, window="hanning", window_frac=0.1, out=None, group_bytes=None):
    """``sspec_device`` of every dynamic spectrum of a contiguous device stack [B, nf, nt] float64 -> device tensor [B, rows, ncfft],
    problem for problem the bits of ``sspec_device(stack_t[k], prewhite, halve, window, window_frac)`` (``scint_sspec_batch``).  The
    window and post-darkening tables are built once per call.  Segments of up to 128 channels or 128 sub-integrations go through
    the single call's kernels as slots and grid.z, in launches that do not grow with B; the stack is then taken in groups whose
    workspace stays below ``group_bytes`` (None: ``scintpar.STACK_GROUP_BYTES``).  Larger segments run the single call's persistent
    kernels problem after problem inside the one library call.  ``out``: a contiguous device tensor of the result's shape."""
    import ctypes
    require_gpu()
    B, nf, nt = scintpar._check_stack("sspec_stack_device", stack_t)
    nrfft = int(2 ** (np.ceil(np.log2(nf)) + 1))      # dynspec.py:3677
    ncfft = int(2 ** (np.ceil(np.log2(nt)) + 1))      # dynspec.py:3678
    if prewhite and not halve:
        raise RuntimeError("Cannot apply prewhite to full frame")   # dynspec.py:3717
    wt, wf = _window_tables(nt, nf, window, window_frac, torch.cuda.current_device())
    pd_fd, pd_td = _postdark_tables(nrfft, ncfft, torch.cuda.current_device()) if prewhite else (None, None)
    shape = (B, nrfft // 2 if halve else nrfft, ncfft)
    if out is None:
        out = empty(shape, torch.float64)
    elif tuple(out.shape) != shape or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError(f"sspec_stack_device: out must be a contiguous float64 tensor of shape {shape}")
    hv = 1 if halve else 0
    one = ctypes.c_size_t()
    _lib.call("scint_sspec_batch_workspace_bytes", 1, nf, nt, hv, one)
    for b0, n in scintpar._stack_groups(B, one.value, group_bytes):
        ws = workspace_for("scint_sspec_batch", n, nf, nt, hv)
        _lib.call("scint_sspec_batch", stack_t[b0:b0 + n], n, nf, nt, wt, wf, 1 if prewhite else 0, hv, pd_fd, pd_td,
                  out[b0:b0 + n], ws, ws.numel(), stream_ptr())
    return out


class Dynspec:
    """Dynamic-spectrum holder with the reference's attribute names
    (dynspec.py:400-413) and a GPU ``calc_sspec``.

    ``sspec``, ``lamsspec``, ``lamdyn`` and ``acf`` are the reference's NumPy attributes, but a freshly
    computed one stays in HBM until it is first read (``device.DeviceBacked``): the chain
    ``scale_dyn -> calc_sspec(lamsteps=True) -> fit_arc`` then never crosses PCIe."""
    sspec = DeviceBacked("sspec")
    lamsspec = DeviceBacked("lamsspec")
    chunks = DeviceBacked("chunks")          # the retrieved wavefield chunks (1 GB for a 4096^2 observation): in HBM until read
    wavefield = DeviceBacked("wavefield")
    lamdyn = DeviceBacked("lamdyn")
    vdyn = DeviceBacked("vdyn")              # scale_dyn('velocity') / ('trapezoid') and their spectra, parked the same way
    vlamdyn = DeviceBacked("vlamdyn")
    trapdyn = DeviceBacked("trapdyn")
    vsspec = DeviceBacked("vsspec")
    vlamsspec = DeviceBacked("vlamsspec")
    trapsspec = DeviceBacked("trapsspec")
    acf_model = DeviceBacked("acf_model")    # the fitted approximate 2-D model over the fit's window (fit_scint_params_2d)
    acf =DeviceBacked("acf")                # [2 nf, 2 nt]: 512 MB for a 4096^2 observation; the scales read a few cuts of it
    cutdyn = DeviceBacked("cutdyn")          # cut_dyn's three stacks (0.94 GB for a 4096^2 observation): a caller who reads one
    cutsspec = DeviceBacked("cutsspec")      # of them downloads that one
    cutacf = DeviceBacked("cutacf")

    def __init__(self, filename=None, dyn=None, verbose=True, process=False, lamsteps=False,
                 remove_short_subs=True, subint_thresh=2.33, mjd=None):
        if process:
            raise NotImplementedError("process=True: cleaning is outside the accelerated hot path "
                                      "(and calls a missing method in the reference, dynspec.py:416)")
        if filename:
            self.load_file(filename, verbose=verbose, lamsteps=lamsteps, subint_thresh=subint_thresh,
                           remove_short_subs=remove_short_subs, mjd=mjd)
        elif dyn is not None:
            self.load_dyn_obj(dyn, verbose=verbose, lamsteps=lamsteps)
        else:
            raise ValueError("Error: No dynamic spectrum file or object")

    # ------------------------------------------------------------------ psrflux text I/O (host)
    def load_file(self, filename, verbose=True, process=False, lamsteps=False, remove_short_subs=True,
                  subint_thresh=2.33, mjd=None):
        """Load a psrflux-format dynamic spectrum (reference: dynspec.py:144-230).  The parsing
        lives in :mod:`scintools_amd.psrflux` (single-pass tokeniser, optional binary side-car);
        the attributes set here are the reference's."""
        if process:
            raise NotImplementedError("process=True: cleaning is outside the accelerated hot path")
        if verbose:
            print("LOADING {0}...".format(filename))
        parsed = psrflux.load_sidecar(filename) or psrflux.read_table(filename)
        obs = psrflux.observation(*parsed, mjd=mjd, mjd_known=getattr(self, "mjd", None))
        self.name = os.path.basename(filename)
        self.filename = filename
        self.__dict__.update(obs)
        if remove_short_subs and np.std(np.diff(self.times)) != 0:
            self.remove_short_subs(threshold=subint_thresh)
        self.lamsteps = lamsteps

    def remove_short_subs(self, threshold=2.33):
        """Drop short sub-integrations at the start of the observation (reference:
        dynspec.py:232-258) and re-derive the time attributes."""
        k = psrflux.leading_short_subs(self.times, threshold)
        self.dyn = self.dyn[:, k:]
        self.times = self.times[k:]
        self.mjd += self.times[0] / 86400
        self.times = self.times - self.times[0]
        self.nsub = len(self.times)
        self.dt = round(np.mean(np.diff(self.times)), 3)
        self.tobs = round(max(self.times) + self.dt, 3)

    def write_file(self, filename=None, verbose=True, note=None, sidecar=False):
        """Write the dynamic spectrum in psrflux format (reference: dynspec.py:330-376); with
        ``sidecar=True`` also the binary image that ``load_file`` prefers while it is current."""
        if filename is None:
            stem, ext = self.filename.rsplit('.', 1)
            filename = f"{stem}.processed.{ext}"
        psrflux.write(filename, self.header, self.mjd, self.times, self.freqs, self.dyn, note=note)
        if sidecar:
            psrflux.save_sidecar(filename, *psrflux.read_table(filename))
        if verbose:
            print("Wrote dynamic spectrum file as {}".format(filename))

    def load_dyn_obj(self, dyn, verbose=True, process=False, lamsteps=False):
        """Copy the reference's attribute set from any object that has it (dynspec.py:378-419)."""
        self.name = getattr(dyn, "name", "dynspec")
        self.header = getattr(dyn, "header", [self.name])
        self.times = np.asarray(dyn.times, dtype=float)
        self.freqs = np.asarray(dyn.freqs, dtype=float)
        self.dyn = np.asarray(dyn.dyn, dtype=float)
        self.nchan = int(getattr(dyn, "nchan", self.dyn.shape[0]))
        self.nsub = int(getattr(dyn, "nsub", self.dyn.shape[1]))
        # (the defaults are formed only when the attribute is missing: a single channel or sub-integration has no spacing)
        self.df = float(dyn.df if hasattr(dyn, "df") else np.abs(self.freqs[1] - self.freqs[0]))
        self.dt = float(dyn.dt if hasattr(dyn, "dt") else self.times[1] - self.times[0])
        self.bw = float(getattr(dyn, "bw", np.ptp(self.freqs) + self.df))
        self.freq = float(getattr(dyn, "freq", np.mean(self.freqs)))
        tobs = getattr(dyn, "tobs", None)
        self.tobs = float(tobs) if tobs is not None else float(np.ptp(self.times) + self.dt)
        m = getattr(dyn, "mjd", None)
        self.mjd = m if m is not None else 60000.0
        self.lamsteps = lamsteps
        if verbose:
            print(f"LOADING DYNSPEC OBJECT {self.name}...")

    def calc_sspec(self, prewhite=False, halve=True, plot=False, lamsteps=False, input_dyn=None,
                   input_x=None, input_y=None, trap=False, window="hanning", window_frac=0.1,
                   return_sspec=False, velocity=False):
        """Secondary spectrum (dynspec.py:3584-3748) on the GPU.

        Sets ``self.sspec / self.fdop / self.tdel`` (``self.lamsspec`` and ``self.beta`` with
        ``lamsteps``, on the wavelength-scaled spectrum of ``scale_dyn``) or, with ``input_dyn``
        or ``return_sspec``, returns ``(fdop, yaxis, sec)``.  ``velocity`` takes the velocity-scaled spectrum of
        ``scale_dyn('velocity', pars=...)`` and sets ``vsspec`` (``vlamsspec`` with ``lamsteps``); ``trap`` rescales
        to the trapezoid (every time, with scale_dyn's default window, as in the reference) and sets ``trapsspec``.
        """
        if plot:
            raise NotImplementedError("plotting is outside the accelerated hot path")
        cls = type(self)
        target = cls.sspec                                  # where the spectrum goes (dynspec.py:3723-3734)
        if input_dyn is not None:
            dyn_t = to_device(input_dyn, torch.float64)
        elif lamsteps:                                      # dynspec.py:3643-3661
            if not cls.lamdyn.present(self):
                self.scale_dyn()
            if velocity:
                if not cls.vlamdyn.present(self):
                    self.scale_dyn(scale='velocity')        # (without pars: the ValueError about the parameter dictionary)
                dyn_t, target = cls.vlamdyn.tensor(self), cls.vlamsspec
            else:
                dyn_t, target = cls.lamdyn.tensor(self), cls.lamsspec
        elif velocity:
            if not cls.vdyn.present(self):
                self.scale_dyn(scale='velocity')
            dyn_t, target = cls.vdyn.tensor(self), cls.vsspec
        elif trap:
            self.scale_dyn(scale='trapezoid')               # every time: the reference tests hasattr(self, 'trap'), never set
            dyn_t, target = cls.trapdyn.tensor(self), cls.trapsspec
        else:
            dyn_t = to_device(self.dyn, torch.float64)
        sec_t = sspec_device(dyn_t, prewhite=prewhite, halve=halve, window=window, window_frac=window_frac)
        nf, nt = dyn_t.shape
        nrfft = int(2 ** (np.ceil(np.log2(nf)) + 1))
        ncfft = int(2 ** (np.ceil(np.log2(nt)) + 1))
        td = np.array(list(range(0, int(nrfft / 2) if halve else int(nrfft))))
        fd = np.array(list(range(int(-ncfft / 2), int(ncfft / 2))))
        fdop = np.reshape(np.multiply(fd, 1e3 / (ncfft * self.dt)), [len(fd)])   # mHz
        tdel = np.reshape(np.divide(td, (nrfft * self.df)), [len(td)])           # us
        if lamsteps:
            beta = np.divide(td, (nrfft * self.dlam))                            # m^-1 (dynspec.py:3703-3704)
        if input_dyn is None and not return_sspec:
            target.park(self, sec_t)                # copied to the host when first read
            if lamsteps:
                self.beta = beta
            self.fdop = fdop
            self.tdel = tdel
            return None
        return fdop, (beta if lamsteps else tdel), sec_t.cpu().numpy()

    # ------------------------------------------------------------------ arc normalisation
    def scale_dyn(self, scale='lambda', window_frac=0.1, pars=None, parfile=None, window='hanning',
                  spacing='auto', s=None, d=None, vism_ra=None, vism_dec=None, Omega=None, inc=None,
                  vism_zeta=None, zeta=None, lamsteps=False, velocity=False, trap=False):
        """Rescale the dynamic spectrum (dynspec.py:3872-4128) on the GPU; a name that holds several scalings
        (``'lambda-velocity'``) runs them in this order.

        * ``'lambda'`` / ``'wavelength'`` / ``lamsteps``: the equal-wavelength resample, one not-a-knot cubic spline per
          time column; sets ``lamdyn / lam / nlam / dlam``.
        * ``'velocity'`` / ``'orbit'`` / ``velocity``: every channel onto equal steps of the cumulative effective velocity,
          one cubic spline per channel; needs ``pars`` (or ``parfile``) with RAJ, DECJ, the binary and proper-motion
          parameters, ``s`` and ``d``; sets ``vdyn`` (``vlamdyn`` when ``lamdyn`` is there), ``veff_ra``, ``veff_dec``.
          The two ephemeris look-ups (``scint_utils.get_ssb_delay`` / ``get_earth_velocity``) need astropy;
          ``arcfit.velocity_resample_device`` takes velocities from any other source.
        * ``'trapezoid'`` / ``trap``: every channel's time axis stretched in proportion to its frequency; sets ``trapdyn``.
        """
        if ('lambda' in scale) or ('wavelength' in scale) or lamsteps:
            arcfit.scale_dyn_lambda(self, spacing=spacing)
        if ('velocity' in scale) or ('orbit' in scale) or velocity:
            arcfit.scale_dyn_velocity(self, pars=pars, parfile=parfile, s=s, d=d, vism_ra=vism_ra, vism_dec=vism_dec,
                                      Omega=Omega, inc=inc, vism_zeta=vism_zeta, zeta=zeta)
        if 'trap' in scale or trap:
            arcfit.scale_dyn_trapezoid(self, window=window, window_frac=window_frac)

    norm_sspec = arcfit.norm_sspec
    fit_arc = arcfit.fit_arc
    calc_scattered_image = arcfit.calc_scattered_image

    trim_edges = clean.trim_edges
    crop_dyn = clean.crop_dyn
    zap = clean.zap
    refill = clean.refill
    inpaint = clean.inpaint
    correct_dyn = clean.correct_dyn
    auto_processing = clean.auto_processing

    get_scint_params = scintpar.get_scint_params
    get_acf_tilt = scintpar.get_acf_tilt
    cut_dyn = scintpar.cut_dyn
    fit_scint_params = scintpar.fit_scint_params
    fit_scint_params_cut = scintpar.fit_scint_params_cut
    fit_arc_cut = arcfit.fit_arc_cut
    fit_scint_params_2d = scintpar.fit_scint_params_2d
    fit_scint_params_2d_cut = scintpar.fit_scint_params_2d_cut

    @property
    def normsspec(self):
        """2-D normalised secondary spectrum of the last ``norm_sspec`` (masked array); copied
        from the device on first access."""
        return arcfit.normsspec_host(self)

    @normsspec.setter
    def normsspec(self, value):
        self._normsspec_host = value

    @property
    def mask(self):
        """Mask of ``normsspec`` (dynspec.py:2118-2126)."""
        override = getattr(self, "_mask_host", None)
        return override if override is not None else np.ma.getmaskarray(arcfit.normsspec_host(self))

    @mask.setter
    def mask(self, value):
        self._mask_host = value

    def calc_acf(self, method='direct', input_dyn=None, normalise=True, window_frac=0.1):
        """Autocovariance function (dynspec.py:3750-3814) on the GPU.  'direct': zero-padded fft2 -> |.|^2 -> ifft2 ->
        fftshift -> real (-> / max).  'sspec': the transform of the full-frame secondary spectrum of ``self.dyn`` (the
        reference takes ``self.dyn`` there even with ``input_dyn``): fftshift -> 10**(./10) -> fft2 -> fftshift -> real
        (-> / max).  Sets ``self.acf`` -- it stays in HBM until it is first read -- or, with ``input_dyn``, returns a NumPy
        array.  Non-finite pixels are not supported here (the reference only excludes them from the mean)."""
        if method not in ('direct', 'sspec'):
            raise ValueError('Method not understood. Choose "direct" or "sspec"')
        require_gpu()
        dyn = self.dyn if (input_dyn is None or method == 'sspec') else np.asarray(input_dyn)
        if not np.all(np.isfinite(dyn)):
            raise ValueError("calc_acf on the GPU needs a finite dynamic spectrum (run refill first)")
        dyn_t = to_device(dyn, torch.float64)
        if method == 'direct':
            # with input_dyn the reference does NOT subtract the mean (dynspec.py:3786-3789)
            out = scintpar.acf_device(dyn_t, subtract_mean=input_dyn is None, normalise=normalise)
        else:
            sec_t = sspec_device(dyn_t, prewhite=False, halve=False, window_frac=window_frac)
            out = scintpar.acf_from_sspec_device(sec_t, normalise=normalise)
        if input_dyn is None:
            type(self).acf.park(self, out)       # copied to the host when first read
            return None
        return out.cpu().numpy()

    # ------------------------------------------------------------------ theta-theta
    def prep_thetatheta(self, fw=.1, npad=3, verbose=False, fitting_proc='standard', **kwargs):
        """Set the theta-theta search parameters (dynspec.py:1348-1537).

        Same keywords as the reference: cwf, cwt, fref, eta_min, eta_max, nedge, edges_lim,
        tau_lim, tau_mask, and for ``fitting_proc='thin'`` arclet_lim (default: edges_lim) and
        center_cut (default 0) (bare numbers in s**3 / mHz / us / MHz, or astropy Quantities).
        Without ``eta_min`` / ``eta_max`` the bounds come from ``fit_arc(lamsteps=True)`` on
        the secondary spectrum, as in the reference (dynspec.py:1458-1473).  'thin' models only
        the arclet apexes: a rectangular theta-theta per curvature and its largest singular value
        (ththmod.two_curve_map / singularvalue_calc); its edges reach fd.max(), not fd.max()/2.
        """
        fitting_procs = ['standard', 'thin', 'incoherent']
        assert fitting_proc in fitting_procs, f'fitting_proc must be one of {fitting_procs}'
        val = lambda key, unit, name: float(units.strip(kwargs[key], name, unit, warn=False))
        self.thetatheta_proc = fitting_proc
        self.npad = npad
        self.fw = fw
        if 'cwf' in kwargs:
            self.cwf = 2 * (kwargs['cwf'] // 2)
            self.ncf_fit = self.dyn.shape[0] // self.cwf
            self.ncf_ret = (self.dyn.shape[0] // (self.cwf // 2)) - 1
        else:
            self.cwf, self.ncf_fit, self.ncf_ret = self.dyn.shape[0], 1, 1
        if 'cwt' in kwargs:
            self.cwt = 2 * (kwargs['cwt'] // 2)
            self.nct_fit = self.dyn.shape[1] // self.cwt
            self.nct_ret = (self.dyn.shape[1] // (self.cwt // 2)) - 1
        else:
            self.cwt, self.nct_fit, self.nct_ret = self.dyn.shape[1], 1, 1
        tau_lim = val('tau_lim', 'us', 'Tau Limit') if 'tau_lim' in kwargs else None
        self.fref = val('fref', 'MHz', 'reference frequency') if 'fref' in kwargs else self.freqs.mean()

        fd = thth.fft_axis(self.times[:self.cwt], 1000.0)       # mHz   (dynspec.py:1445)
        tau = thth.fft_axis(self.freqs[:self.cwf], 1.0)         # us    (dynspec.py:1446)
        eta_min = 4 * (tau[1] - tau[0]) / fd.max()**2            # dynspec.py:1448-1451
        eta_max = tau.max() / (fd[1] - fd[0])**2
        eta_min *= (self.freqs.max() / self.fref)**2
        eta_max *= (self.freqs.min() / self.fref)**2
        self.eta_min = max((val('eta_min', 's3', 'eta_min'), eta_min)) if 'eta_min' in kwargs else eta_min
        self.eta_max = min((val('eta_max', 's3', 'eta_max'), eta_max)) if 'eta_max' in kwargs else eta_max
        if not ('eta_min' in kwargs and 'eta_max' in kwargs):         # dynspec.py:1458-1473
            # curvature from the secondary spectrum; s**3 <-> 1/(m mHz**2) through c / fref**2
            if not hasattr(self, "betaeta"):
                self.fit_arc(lamsteps=True, numsteps=1e4, etamin=self.eta_min * self.fref**2 * 1e6 / sc.c,
                             etamax=self.eta_max * self.fref**2 * 1e6 / sc.c, delmax=tau_lim)
            eta_hough = sc.c * self.betaeta / (self.fref**2 * 1e6)
            err_hough = sc.c * 2 * max((self.betaetaerr, self.betaetaerr2)) / (self.fref**2 * 1e6)
            if 'eta_min' not in kwargs:
                self.eta_min = max((self.eta_min, eta_hough - err_hough))
            if 'eta_max' not in kwargs:
                self.eta_max = min((self.eta_max, eta_hough + err_hough))
        l0, l1 = np.log10(self.eta_min), np.log10(self.eta_max)
        self.neta = int(1 + (l1 - l0) / np.log10(1 + self.fw / 10))     # dynspec.py:1478
        if fitting_proc == 'thin':                                # dynspec.py:1480-1483
            fd_cut = fd.max() * (self.fref / self.freqs.max())
        else:
            fd_cut = (fd.max() / 2) * (self.fref / self.freqs.max())
        edges_lim = min((val('edges_lim', 'mHz', 'edges limit'), fd_cut)) if 'edges_lim' in kwargs else fd_cut
        if tau_lim is not None:
            edges_lim = min((edges_lim, np.sqrt(tau_lim / self.eta_max)))
        if 'nedge' in kwargs:
            assert np.mod(kwargs['nedge'], 2) == 0, 'nedge must be even!'
            self.edges = np.linspace(-edges_lim, edges_lim, kwargs['nedge'])
        else:                                                     # dynspec.py:1500-1503
            self.edges = np.asarray(thth.min_edges(edges_lim, fd, tau,
                                                   self.eta_max * (self.fref / self.freqs.min()), 2)) \
                * (self.freqs.min() / self.fref)
            if units.HAVE_ASTROPY:
                self.edges = np.asarray(getattr(self.edges, "value", self.edges))
        if fitting_proc == 'thin':                                # dynspec.py:1505-1516
            self.arclet_lim = val('arclet_lim', 'mHz', 'Arclet Limit') if 'arclet_lim' in kwargs else edges_lim
            self.center_cut = val('center_cut', 'mHz', 'Central Cut') if 'center_cut' in kwargs else 0
        self.thth_tau_mask = val('tau_mask', 'us', 'tau_mask') if 'tau_mask' in kwargs else 0.0
        if verbose:
            print("\n\t THETA-THETA PROPERTIES\n")
            print(f'Channels per chunk: {self.cwf}')
            print(f'Time bins per chunk: {self.cwt}')
            print(f'Number of fitting chunks: {self.ncf_fit}x{self.nct_fit}')
            print(f'Reference Frequency: {self.fref} MHz')
            print(f'Eta range: {self.eta_min} to {self.eta_max} s3 with {self.neta} points')
            print(f'Edges has {self.edges.shape[0]} point out to {self.edges[-1]} mHz')
            print(f'Fractional fitting width: {self.fw}')
            print(f'Zero paddings: {self.npad}')
            print(f'Fitting Procedure: {self.thetatheta_proc}')
            print(f'Masking |tau| < {self.thth_tau_mask} us')

    def _chunk(self, cf, ct):
        fs = slice(cf * self.cwf, (cf + 1) * self.cwf)
        ts = slice(ct * self.cwt, (ct + 1) * self.cwt)
        return fs, ts

    def _chunk_etas(self, freq2):
        return np.logspace(np.log10(self.eta_min), np.log10(self.eta_max), self.neta) \
            * (self.fref / freq2.mean())**2

    def thetatheta_single(self, cf=0, ct=0, fname=None, verbose=False, plot=True, arrays=False):
        """theta-theta curvature search on one chunk (dynspec.py:1539-1655).  Same defaults as
        the reference: with ``arrays=True`` returns (etas, eigs, popt); the diagnostic plot is
        outside the accelerated path, so ``plot=True`` only warns."""
        if not hasattr(self, 'cwf'):
            self.prep_thetatheta(verbose=verbose)            # dynspec.py:1555-1556
        if plot:
            warnings.warn("scintools_amd: thetatheta_single does not draw the diagnostic plot; "
                          "pass arrays=True for the curve and the fit")
        cf, ct = min(cf, self.ncf_fit - 1), min(ct, self.nct_fit - 1)
        fs, ts = self._chunk(cf, ct)
        freq2 = self.freqs[fs]
        edges = self.edges * (freq2.mean() / self.fref)
        tau, fd = thth._chunk_axes(self.times[ts], freq2, edges, self.npad)[3:]
        dspec2 = np.copy(self.dyn[fs, ts])
        dspec2 -= np.nanmean(dspec2)
        cs = thth.conjugate_spectrum(np.nan_to_num(dspec2), self.npad, tau, self.thth_tau_mask,
                                     self.thetatheta_proc != 'incoherent', pad_value=0.0)
        etas = self._chunk_etas(freq2)
        if self.thetatheta_proc == 'thin':
            # scaled to the chunk BEFORE the arclet filter here (dynspec.py:1590-1596), after it in fit_thetatheta
            eigs = thth.sv_sweep_multi(cs.unsqueeze(0), [(tau, fd, edges, edges[np.abs(edges) < self.arclet_lim])], [etas],
                                       self.center_cut)[0]
        else:
            eigs = thth.eval_sweep(cs, tau, fd, etas, edges)
        _, _, popt = thth.fit_eig_peak(etas, eigs, self.fw)
        if arrays:
            return etas, eigs, popt

    def _fit_chunks(self, group_all):
        """Curvature fits of the listed chunks on this GPU: rows [eta_fit, eta_sig, eigs...].
        Chunks are grouped so that a stack of conjugate spectra stays below ~8 GiB; each group is
        one ``eval_sweep_multi`` call (all (chunk, eta) pairs batched together)."""
        coher = (self.thetatheta_proc != 'incoherent')
        thin = self.thetatheta_proc == 'thin'
        R, C = (self.npad + 1) * self.cwf, (self.npad + 1) * self.cwt
        per_group = thth._group_size(16 * R * C)
        rows = np.full((len(group_all), 2 + self.neta), np.nan)
        for g0 in range(0, len(group_all), per_group):
            group = group_all[g0:g0 + per_group]
            stack = empty((len(group), R, C), torch.complex128)
            grids, etas_list, pads = [], [], []
            # the group's chunks travel to the device in ONE array (an upload from pageable memory per chunk, and a device mean
            # read back per chunk for the padding value, block the host once each: ththmod.chunk_retrieval_batch)
            d_all = np.empty((len(group), self.cwf, self.cwt))
            for k, (cf, ct) in enumerate(group):
                dspec2, freq2, time2, etas, edges = self._search_params(cf, ct)[:5]
                tau, fd = thth._chunk_axes(time2, freq2, edges, self.npad)[3:]      # ththmod.py:773-774
                d_all[k] = dspec2
                pads.append(float(d_all[k].mean()))                   # the padding value (ththmod.py:783)
                grids.append((tau, fd, edges))
                etas_list.append(etas)
            d_t = thth.to_device(d_all, torch.float64)
            for k in range(len(group)):
                # the thin search pads with the mean too but applies no delay mask, even when one was set (dynspec.py:1689-1719)
                thth.conjugate_spectrum(d_t[k], self.npad, None if thin else grids[k][0], self.thth_tau_mask, coher,
                                        pad_value=pads[k], out=stack[k])
            if thin:
                arclet = self._arclet_edges()
                eig_list = thth.sv_sweep_multi(stack, [g + (arclet * (self.freqs[self._chunk(cf, ct)[0]].mean() / self.fref),)
                                                       for g, (cf, ct) in zip(grids, group)], etas_list, self.center_cut)
            else:
                eig_list = thth.eval_sweep_multi(stack, grids, etas_list)
            for k, (etas, eigs) in enumerate(zip(etas_list, eig_list)):
                eta_fit, eta_sig, _ = thth.fit_eig_peak(etas, eigs, self.fw)   # ththmod.py:814-859
                rows[g0 + k, 0], rows[g0 + k, 1] = eta_fit, eta_sig
                rows[g0 + k, 2:] = eigs
        return rows

    def _arclet_edges(self):
        """fit_thetatheta's arclet grid: self.edges filtered by arclet_lim BEFORE the scaling to a chunk (dynspec.py:1706-1709)."""
        return self.edges[np.abs(self.edges) < self.arclet_lim]

    def _search_params_thin(self, cf, ct, verbose=False):
        """The 13-element parameter list the reference hands to ``single_search_thin`` (dynspec.py:1689-1709), plain floats."""
        p = self._search_params(cf, ct, verbose)
        freq2 = p[1]
        return p[:10] + [verbose, self._arclet_edges() * (freq2.mean() / self.fref), self.center_cut]

    def _search_params(self, cf, ct, verbose=False):
        """The 12-element parameter list the reference hands to ``single_search`` for fitting
        chunk (cf, ct) (dynspec.py:1689-1704), plain floats."""
        fs, ts = self._chunk(cf, ct)
        freq2, time2 = np.copy(self.freqs[fs]), np.copy(self.times[ts])
        dspec2 = np.copy(self.dyn[fs, ts])
        dspec2 -= np.nanmean(dspec2)
        dspec2 = np.nan_to_num(dspec2)
        coher = (self.thetatheta_proc != 'incoherent')
        return [dspec2, freq2, time2, self._chunk_etas(freq2), self.edges * (freq2.mean() / self.fref),
                None, False, self.fw, self.npad, coher, self.thth_tau_mask, verbose]

    def fit_thetatheta(self, verbose=False, plot=False, pool=None, time_avg=False):
        """Curvature search over all fitting chunks and the global eta ~ nu**-2 fit
        (dynspec.py:1657-1763).  Sets eta_evo, eta_evo_err, f0s, t0s, ththeta, ththetaerr
        (plain floats: s**3, MHz, s).

        Where the chunks run:
          * ``pool=None`` (default): every chunk's conjugate spectrum goes into one device stack
            and all (chunk, eta) pairs run as ONE continuously batched sweep on this GPU; under an
            initialised ``torch.distributed`` group the chunks are dealt round-robin to the ranks
            (one GPU each) and the fitted curvatures are all-gathered (``sweep.sharded_chunks``);
          * ``pool`` given: exactly the reference's ``pool.map(thth.single_search, pars)`` (``single_search_thin`` for 'thin')
            (dynspec.py:1715-1719) -- with ``sweep.gpu_pool(n)`` every worker process drives its
            own GPU.
        """
        if not hasattr(self, 'cwf'):
            self.prep_thetatheta(verbose=verbose)             # dynspec.py:1673-1674
        if plot:
            warnings.warn("scintools_amd: fit_thetatheta does not plot the curvature evolution")
        self.eta_evo = np.zeros((self.ncf_fit, self.nct_fit))
        self.eta_evo_err = np.zeros((self.ncf_fit, self.nct_fit))
        self.f0s = np.zeros(self.ncf_fit)
        self.t0s = np.zeros(self.nct_fit)
        self.thth_eigs = np.zeros((self.ncf_fit, self.nct_fit, self.neta))
        chunks = [(cf, ct) for cf in range(self.ncf_fit) for ct in range(self.nct_fit)]
        for cf, ct in chunks:
            fs, ts = self._chunk(cf, ct)
            self.f0s[cf] = self.freqs[fs].mean()
            self.t0s[ct] = self.times[ts].mean()
        if pool is not None:
            if getattr(self, 'thetatheta_proc', 'standard') == 'thin':
                res = pool.map(thth.single_search_thin, [self._search_params_thin(cf, ct, verbose) for cf, ct in chunks])
            else:
                res = pool.map(thth.single_search, [self._search_params(cf, ct, verbose) for cf, ct in chunks])
            for (cf, ct), r in zip(chunks, res):
                # with astropy present single_search returns Quantities (s**3): strip before the
                # plain-float arrays take them (a NumPy scalar assignment of a Quantity raises)
                self.eta_evo[cf, ct] = float(units.strip(r[0], 'eta', 's3', warn=False))
                self.eta_evo_err[cf, ct] = float(units.strip(r[1], 'eta_sig', 's3', warn=False))
                # single_search drops failed curvatures from the curve it returns (ththmod.py:817):
                # only a complete curve can be put back on the eta grid
                curve = np.asarray(r[4], dtype=float)
                self.thth_eigs[cf, ct] = curve if curve.shape == (self.neta,) else np.nan
        else:
            from . import sweep
            fits = sweep.sharded_chunks(len(chunks), lambda idx: self._fit_chunks([chunks[i] for i in idx]),
                                        self.neta)
            for (cf, ct), row in zip(chunks, fits):
                self.eta_evo[cf, ct], self.eta_evo_err[cf, ct] = row[0], row[1]
                self.thth_eigs[cf, ct] = row[2:]
        f0 = self.f0s[:, np.newaxis]
        with np.errstate(divide='ignore', invalid='ignore'):
            if time_avg:                                                   # dynspec.py:1724-1732
                eta_avg = np.nanmean(self.eta_evo, 1)
                eta_count = np.nansum(self.eta_evo, 1) / eta_avg
                avg_err = np.nanstd(self.eta_evo, 1) / np.sqrt(eta_count - 1)
                tofit = np.isfinite(eta_avg) * np.isfinite(avg_err)
                A = (np.sum(eta_avg[tofit] / (self.f0s * avg_err)[tofit] ** 2) /
                     np.sum(1 / (self.f0s**2 * avg_err)[tofit] ** 2))
                A_err = np.sqrt(1 / np.sum(2 / ((self.f0s**2) * avg_err)[tofit] ** 2))
            else:                                                          # dynspec.py:1734-1742
                tofit = np.isfinite(self.eta_evo) * np.isfinite(self.eta_evo_err)
                A = (np.sum(self.eta_evo[tofit] / (f0 * self.eta_evo_err)[tofit] ** 2) /
                     np.sum(1 / ((f0**2) * self.eta_evo_err)[tofit] ** 2))
                A_err = np.sqrt(1 / np.sum(2 / ((f0**2) * self.eta_evo_err)[tofit] ** 2))
        self.ththeta = A / self.fref**2
        self.ththetaerr = A_err / self.fref**2

    # ------------------------------------------------------------------ phase retrieval
    def _retrieval_chunks(self):
        """(cf, ct, fs, ts, freq2, eta, edges) of every half-overlapping retrieval chunk, frequency rows outermost
        (dynspec.py:1777-1800): its slices, its channels, the fitted curvature and the edges scaled to its mean frequency."""
        for cf in range(self.ncf_ret):
            fs = slice(cf * (self.cwf // 2), cf * (self.cwf // 2) + self.cwf)
            freq2 = np.copy(self.freqs[fs])
            freq = freq2.mean()
            eta = self.ththeta * (self.fref / freq)**2
            for ct in range(self.nct_ret):
                ts = slice(ct * (self.cwt // 2), ct * (self.cwt // 2) + self.cwt)
                yield cf, ct, fs, ts, freq2, eta, self.edges * (freq / self.fref)

    def thetatheta_chunks(self, verbose=False, pool=None, memmap=False):
        """theta-theta phase retrieval on all half-overlapping chunks (dynspec.py:1765-1826):
        fills ``self.chunks[ncf_ret, nct_ret, cwf, cwt]``.

        ``pool=None`` (default): every chunk's conjugate spectrum goes into one device stack, the dominant
        eigenpairs of all chunks come from ONE batched sweep and the back-maps / inverse FFTs are queued
        without a host round trip in between (``ththmod.chunk_retrieval_batch``).  With a ``pool`` it is the
        reference's ``pool.map(thth.single_chunk_retrieval, pars)`` (dynspec.py:1806-1812); `memmap` is
        accepted for signature compatibility."""
        if not hasattr(self, "ththeta"):
            self.fit_thetatheta(verbose=verbose, pool=pool)
        if pool is not None:
            self.chunks = np.zeros((self.ncf_ret, self.nct_ret, self.cwf, self.cwt), dtype=complex)
            pars = []
            for cf, ct, fs, ts, freq2, eta, edges in self._retrieval_chunks():
                dspec2 = np.copy(self.dyn[fs, ts])
                dspec2 -= np.nanmean(dspec2)
                dspec2 = np.nan_to_num(dspec2)
                pars.append((dspec2, edges, np.copy(self.times[ts]), freq2, eta, ct, cf, self.npad, self.thth_tau_mask, verbose))
            for res in pool.map(thth.single_chunk_retrieval, pars):
                self.chunks[res[1], res[2], :, :] = res[0]
            return
        # Round 6: the chunks are cut out of the dynamic spectrum ON the device (one upload of `dyn`; window, nanmean, nan_to_num and
        # the padding value in NumPy's own summation order: ththmod.chunk_cut_device) and the retrieved chunks stay there for the
        # mosaic -- the host loop above copied 0.5 GB up and 1 GB down and spent 0.2 s in nanmean / nan_to_num of 961 windows.
        pars, origins = [], []
        for cf, ct, fs, ts, freq2, eta, edges in self._retrieval_chunks():
            pars.append((None, edges, np.copy(self.times[ts]), freq2, eta))
            origins.append((fs.start, ts.start))
        dyn_h = np.asarray(self.dyn, dtype=float)
        dyn_t = thth.to_device(dyn_h, torch.float64)
        d_t, pad_t = thth.chunk_cut_device(dyn_t, origins, self.cwf, self.cwt, fortran_order=_walks_columns(dyn_h))
        out_t = thth.chunk_retrieval_batch(pars, self.npad, self.thth_tau_mask, verbose=verbose, dev_chunks=d_t,
                                           dev_pads=pad_t.cpu().numpy(), out_device=True)
        type(self).chunks.park(self, out_t.reshape(self.ncf_ret, self.nct_ret, self.cwf, self.cwt))

    def calc_wavefield(self, verbose=False, pool=None, gs=False, memmap=False, niter=1):
        """Mosaic the chunks into the final wavefield (dynspec.py:1828-1856)."""
        cls = type(self)
        if not cls.chunks.present(self):
            self.thetatheta_chunks(verbose=verbose, pool=pool, memmap=memmap)
        # the mosaic on the device (ththmod.mosaic_device: the reference's loop, NumPy's summation order, bit-identical to
        # thth.mosaic on the same chunks); the wavefield stays in HBM until it is read
        cls.wavefield.park(self, thth.mosaic_device(cls.chunks.tensor(self, torch.complex128)))
        if gs:
            self.gerchberg_saxton(verbose=verbose, pool=pool, niter=niter)

    def refine_wavefield(self, mode="rot", N=None, verbose=False, pool=None, **kw):
        """Mosaic the chunks with every chunk's phase fitted jointly (``mode="rot"``: ``rotInit`` + ``rotFit``, the reference
        tutorial's wavefield) or phase and amplitude against the dynamic spectrum (``"full"``: ``fullMosFit``), on the chunks
        parked in HBM (``ththmod.fit_mosaic``; ``kw`` goes there: x0, method, options).  ``N``: the noise map of ``"full"``
        (array like ``dyn``, or a number).  Its default is one number for the whole map, ``nanstd(diff(dyn, axis=1)) / sqrt(2)``:
        that ASSUMES white noise and a spectrum that is smooth in time over one sample (scintillation structure between
        neighbouring sub-integrations counts as noise otherwise) -- pass a measured map where that does not hold.  ``dyn`` and
        ``N`` are cropped to the mosaic's extent, as ``fullMosFit`` does.
        Fills ``self.wavefield`` and ``self.mosaic_params`` (and ``self.mosaic_result``, SciPy's report)."""
        cls = type(self)
        if not cls.chunks.present(self):
            self.thetatheta_chunks(verbose=verbose, pool=pool)
        chunks_t = cls.chunks.tensor(self, torch.complex128)
        if mode == "full":
            dyn = np.asarray(self.dyn, dtype=float)
            if N is None:
                N = np.nanstd(np.diff(dyn, axis=1)) / np.sqrt(2.0)
            ncf, nct, cwf, cwt = (int(v) for v in chunks_t.shape)
            F, T = (ncf - 1) * (cwf // 2) + cwf, (nct - 1) * (cwt // 2) + cwt      # the gradient wants the mosaic's own extent
            stack = thth.MosaicStack(chunks_t, dyn[:F, :T], np.broadcast_to(np.asarray(N, dtype=float), dyn.shape)[:F, :T])
        else:
            stack = thth.MosaicStack(chunks_t)
        wf_t, params, res = thth.fit_mosaic(stack, mode=mode, out_device=True, **kw)
        cls.wavefield.park(self, wf_t)
        self.mosaic_params, self.mosaic_result = params, res

    def gerchberg_saxton(self, niter=1, verbose=False, pool=None):
        """Gerchberg-Saxton: enforce the measured amplitudes and causality (tau >= 0)
        (dynspec.py:1858-1875); the FFT <-> projection iterations run on the GPU."""
        self.calc_wavefield(verbose=verbose, pool=pool)
        F = self.wavefield.shape[0]
        tau = thth.fft_axis(self.freqs[:F], 1.0)
        self.wavefield = thth.gerchberg_saxton_device(self.wavefield, self.dyn, tau, niter=niter)

    def calc_asymmetry(self, verbose=False, pool=None):
        """Arc asymmetry of every fitting chunk (dynspec.py:1877-1906), including the
        reference's time slice ``ct*cwt//2 : (ct+1)*cwt``."""
        if not hasattr(self, "ththeta"):
            self.fit_thetatheta(verbose=verbose, pool=pool)
        self.asymmetry = np.zeros((self.ncf_fit, self.nct_fit), dtype=complex)
        for cf in range(self.ncf_fit):
            fs = slice(cf * self.cwf, (cf + 1) * self.cwf)
            freq2 = np.copy(self.freqs[fs])
            freq = freq2.mean()
            eta = self.ththeta * (self.fref / freq)**2
            for ct in range(self.nct_fit):
                ts = slice(ct * self.cwt // 2, (ct + 1) * self.cwt)
                time2 = np.copy(self.times[ts])
                dspec2 = np.copy(self.dyn[fs, ts])
                dspec2 -= np.nanmean(dspec2)
                dspec2 = np.nan_to_num(dspec2)
                params = (dspec2, self.edges * (freq / self.fref), time2, freq2, eta, ct, cf, self.npad, verbose)
                self.asymmetry[cf, ct] = thth.calc_asymmetry(params)[0]
