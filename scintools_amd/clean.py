"""Dynamic-spectrum cleaning: ``trim_edges``, ``crop_dyn``, ``zap``, ``refill``, ``correct_dyn``, ``auto_processing`` of the
reference ``Dynspec`` (dynspec.py:259-328, 3816-3870, 3273-3410, 422-440) and ``ththmod.svd_model`` (ththmod.py:18-35).

The functions are bound onto ``scintools_amd.dynspec.Dynspec`` as ``arcfit``'s are.  ``self.dyn`` stays a NumPy attribute: every
method uploads the array once, runs the kernels of ``csrc/clean.hpp`` and downloads the result once.  What runs where:

* ``zap``: both medians (an exact radix select over float64, NaN excluded) and the NaN mask on the device; bit-exact.
* ``refill('median')``: the 2-D median filter (zero padding, only the NaN pixels) on the device; bit-exact.  The mean of the
  valid pixels -- the fill value, and the final mean fill of every method -- is one ``np.mean`` of the host array: its bits are
  those of NumPy's pairwise summation of the compacted pixels, which is the contract.
* ``refill('linear')`` (and ``'biharmonic'``, which falls back to it as the reference does without scikit-image): gaps that are
  whole channels or whole sub-integrations are interpolated across on the device; any other mask raises
  ``NotImplementedError`` (the reference's answer then depends on Qhull's tie-breaking on the regular grid).
* ``inpaint`` (not in the reference: the biharmonic fill that its ``refill()`` runs by default with scikit-image, for any mask):
  compaction of the mask, the 25-stencil matrix-free operator and conjugate gradients on the device (``csrc/inpaint.hpp``); the
  host builds the stencil table and counts the mask.  ``refill`` itself is unchanged and does not call it.
* ``correct_dyn(svd=True)``: the top ``nmodes`` singular triplets by block iteration on the device, the model and the divide
  too.  ``svd=False``: the two ``nanmean`` s and the divides on the device, ``savgol_filter`` of the two vectors on the host.
* ``trim_edges``, ``crop_dyn``: host only.

Stopping rule of the block iteration: ``|A^T A V - V H|_F <= SVD_TOL * lambda_p`` (``H = V^T A^T A V``, ``lambda_p`` its smallest
eigenvalue), the Ritz-residual rule of the eigenvalue sweeps with ``SVD_TOL = ththmod.DEFAULT_TOL = 1e-12``.
"""
import ctypes

import numpy as np
import torch

from . import _lib, device

SVD_TOL = 1e-12            # = ththmod.DEFAULT_TOL (tests/test_clean_cpu.py checks that they agree)
SVD_MAX_ITER = 4000
MAX_MODES = 4              # correct_dyn / svd_model; the kernels carry up to 8 columns (a complex array needs two per mode)
MEDIAN_MAX_WINDOW = 225    # kf * kt of refill('median') (csrc/clean.hpp, kMedMaxWindow)
INPAINT_TOL = 1e-12        # = ththmod.DEFAULT_TOL: the true relative residual of the biharmonic fill
INPAINT_MAX_ITER = 2000    # conjugate-gradient steps of the biharmonic fill (some 50 for isolated pixels and single lines)
LINES_MAX_LENGTH = 4096    # precond='lines': points of a transformed axis (or twice that: the longest row FFT itself)

_IRREGULAR = ("refill(method={0!r}): only gaps that are whole channels or whole sub-integrations are interpolated on the "
              "device.  For any other mask (isolated pixels, blocks, channels and sub-integrations together) the reference's "
              "griddata triangulates a regular grid, a degenerate Delaunay input whose answer depends on Qhull's tie-breaking; "
              "use method='median'")


def is_valid(array):
    """The pixels that count as data: finite ones (NaN and +-inf are not)."""
    return np.isfinite(array)


def _lib_ready():
    _lib.load()
    device.require_gpu()


# ----------------------------------------------------------------------------
# device calls on host arrays
# ----------------------------------------------------------------------------
def zap_device(dyn, sigma=7):
    """(zapped copy of ``dyn``, median, mdev) of ``Dynspec.zap`` from the device (``scint_zap``)."""
    _lib_ready()
    t = device.to_device(np.array(dyn, dtype=np.float64), torch.float64)
    stats = device.empty((2,), torch.float64)
    ws = device.workspace_for("scint_zap")
    _lib.call("scint_zap", t, t.numel(), sigma, stats, ws, ws.numel(), device.stream_ptr())
    med, mdev = (float(v) for v in stats.cpu().numpy())
    return t.cpu().numpy(), med, mdev


def _kernel_size(kernel_size):
    """(kf, kt) as scipy.signal.medfilt reads ``kernel_size`` for a 2-D array, with its error for an even size."""
    ks = np.asarray(kernel_size)
    if ks.shape == ():
        ks = np.repeat(ks.item(), 2)
    if ks.shape != (2,):
        raise ValueError("kernel_size must be an integer or one integer per axis")
    for k in ks:
        if (k % 2) != 1:
            raise ValueError("Each element of kernel_size should be odd.")
    kf, kt = int(ks[0]), int(ks[1])
    if kf * kt > MEDIAN_MAX_WINDOW:
        raise ValueError(f"refill(method='median'): a window of {kf} x {kt} holds more than {MEDIAN_MAX_WINDOW} elements, "
                         "the most the device filter selects from")
    return kf, kt


def median_fill_device(dyn, kf, kt, fill):
    """``dyn`` with every NaN replaced by the median of its kf x kt window of ``dyn with NaN -> fill`` (zero padded)."""
    _lib_ready()
    t = device.to_device(dyn, torch.float64)
    nf, nt = (int(v) for v in t.shape)
    out = device.empty((nf, nt), torch.float64)
    _lib.call("scint_refill_median", t, nf, nt, kf, kt, fill, out, device.stream_ptr())
    return out.cpu().numpy()


def linear_fill_device(dyn, axis, line_valid):
    """A copy of ``dyn`` with the lines (axis 0: channels, axis 1: sub-integrations) flagged invalid interpolated across."""
    _lib_ready()
    t = device.to_device(np.array(dyn, dtype=np.float64), torch.float64)
    nf, nt = (int(v) for v in t.shape)
    v = device.to_device(np.asarray(line_valid, dtype=np.uint8), torch.uint8)
    _lib.call("scint_refill_linear", t, nf, nt, int(axis), v, device.stream_ptr())
    return t.cpu().numpy()


def stencil_table():
    """The 25 stencils of the squared Laplacian, [25][5][5]: entry ``5 a + b`` holds, for a pixel of class ``(a, b)`` (per axis 0, 1:
    that far from the first line, 2: interior, 3, 4: one and zero from the last), the coefficients of ``L @ L`` at the offsets
    ``-2..2`` x ``-2..2`` around it, zero beyond the edge.  ``L`` is the 5-point Laplacian with reflecting edges.  A 5 x 5 image has
    one pixel of every class, and a column of ``L @ L`` reaches two pixels, so the table is read off that image."""
    global _STENCILS
    if _STENCILS is None:
        l1 = -2.0 * np.eye(5) + np.eye(5, k=1) + np.eye(5, k=-1)
        l1[0, 0] = l1[4, 4] = -1.0                      # the reflected neighbour of an edge pixel is the pixel itself
        lap = np.kron(l1, np.eye(5)) + np.kron(np.eye(5), l1)
        cols = (lap @ lap).reshape(5, 5, 5, 5)          # [row, column of the image][a, b of the pixel]
        table = np.zeros((5, 5, 5, 5))
        for a in range(5):
            for b in range(5):
                for dr in range(-2, 3):
                    for dc in range(-2, 3):
                        if 0 <= a + dr < 5 and 0 <= b + dc < 5:
                            table[a, b, dr + 2, dc + 2] = cols[a + dr, b + dc, a, b]
        _STENCILS = table.reshape(25, 5, 5)
    return _STENCILS


_STENCILS = None


def biharmonic_fill_device(dyn, mask=None, tol=INPAINT_TOL, max_iter=None, info=None, precond=None):
    """A copy of the 2-D ``dyn`` with the pixels of ``mask`` (default: the non-finite ones) replaced by the biharmonic fill, the
    method of ``refill(method='biharmonic')`` in the reference (scikit-image's ``inpaint_biharmonic``): with ``L`` the 5-point
    Laplacian with reflecting edges, ``m`` the masked and ``k`` the known pixels, the solution of ``(L L)_mm u_m = -(L L)_mk u_k``
    by conjugate gradients on the device (``scint_inpaint_biharmonic``, csrc/inpaint.hpp) down to a true relative residual of
    ``tol``.  Known pixels keep their bits.  ``info`` receives ``iters``, ``residual`` (the true relative residual) and ``nmask``.

    ``max_iter`` (default ``INPAINT_MAX_ITER``) bounds the steps; ``ScintHipError`` when they run out.  The condition number grows
    with the fourth power of the widest gap and the steps with its square root: isolated pixels and single lines take some 50
    steps, a gap 40 pixels wide will not finish within the default.

    ``precond='lines'`` (default ``None``: the route above, unchanged) runs PRECONDITIONED conjugate gradients
    (``scint_inpaint_biharmonic_lines``): the preconditioner inverts exactly the block of the matrix on the channels whose every
    pixel is masked (a DCT along time, one pentadiagonal solve per mode) and the block on the wholly masked sub-integrations, and
    divides by the diagonal elsewhere, so wide bands cost no more steps than narrow ones.  A mask of whole channels only, or of
    whole sub-integrations only, is solved directly (zero steps).  After a solve ``info`` also receives ``route`` (``'cg'`` without
    ``precond``; with it ``'direct'`` when no step was needed, else ``'pcg'``) and, with ``precond``, ``line_channels`` and
    ``line_subints``, the whole lines found (when nothing is masked nothing is solved and ``info`` has none of the three).  Limits: a line with even one known pixel is not whole -- a nearly whole band falls to the diagonal
    part and stays slow; a mask without any whole line is accepted and gains nothing; an axis that is transformed (time when
    there are whole channels, frequency when there are whole sub-integrations) must hold 5 .. 4096 points, or 8192
    (``ValueError`` otherwise).  Errors, and ``dyn`` untouched on failure, as on the plain route."""
    if precond not in (None, 'lines'):
        raise ValueError(f"biharmonic_fill_device: precond={precond!r}; None (plain conjugate gradients) or 'lines'")
    out = np.array(dyn, dtype=np.float64)
    if out.ndim != 2:
        raise ValueError("biharmonic_fill_device needs a 2-D array")
    bad = ~is_valid(out) if mask is None else np.asarray(mask, dtype=bool)
    if bad.shape != out.shape:
        raise ValueError(f"biharmonic_fill_device: the mask has shape {bad.shape}, the array {out.shape}")
    nf, nt = out.shape
    nmask = int(np.count_nonzero(bad))
    if info is not None:
        info.update(iters=0, residual=0.0, nmask=nmask)
    if nmask == 0:
        return out
    if nmask == bad.size:
        raise ValueError("biharmonic_fill_device: every pixel is masked, there is nothing to fill from")
    if nf < 5 or nt < 5:
        raise ValueError(f"biharmonic_fill_device: a {nf} x {nt} array; the 25 edge classes of the stencil need at least 5 x 5")
    if not is_valid(out[~bad]).all():
        raise ValueError("biharmonic_fill_device: a pixel outside the mask is not finite")
    if not 0.0 < tol < 1.0:
        raise ValueError("biharmonic_fill_device: tol must lie between 0 and 1")
    max_iter = INPAINT_MAX_ITER if max_iter is None else int(max_iter)
    if max_iter < 1:
        raise ValueError("biharmonic_fill_device: max_iter must be at least 1")
    counts = ()
    if precond == 'lines':
        counts = (int(np.count_nonzero(bad.all(axis=1))), int(np.count_nonzero(bad.all(axis=0))))
        for lines, n, axis in ((counts[0], nt, 'time'), (counts[1], nf, 'frequency')):
            if lines and not lines_length_ok(n):
                raise ValueError(f"biharmonic_fill_device(precond='lines'): the {axis} axis holds {n} points; the transform along "
                                 f"it takes 5 .. {LINES_MAX_LENGTH} points, or {2 * LINES_MAX_LENGTH}")
    entry = "scint_inpaint_biharmonic" if precond is None else "scint_inpaint_biharmonic_lines"
    _lib_ready()
    t = device.to_device(out, torch.float64)
    m = device.to_device(bad, torch.uint8)
    table = device.to_device(stencil_table(), torch.float64)
    ws = device.workspace_for(entry, nf, nt, nmask, *counts)
    residual, iters = ctypes.c_double(), ctypes.c_int32()
    try:
        _lib.call(entry, t, nf, nt, m, nmask, *counts, table, tol, max_iter, residual, iters, ws, ws.numel(), device.stream_ptr())
    except _lib.ScintHipError as err:
        if err.status == _lib.SCINT_E_NOCONV:
            noconv = _lib.ScintHipError(f"biharmonic_fill_device: conjugate gradients stopped after {iters.value} steps at a relative "
                                        f"residual of {residual.value:.3g} (wanted {tol:g}): a wide gap (the condition number grows "
                                        "with the fourth power of its width); raise max_iter")
            noconv.status = err.status
            raise noconv from None
        raise
    if info is not None:
        info.update(iters=iters.value, residual=residual.value)
        info.update(route='cg')
        if precond is not None:
            info.update(route='pcg' if iters.value else 'direct', line_channels=counts[0], line_subints=counts[1])
    return t.cpu().numpy()


def lines_length_ok(n):
    """Can an axis of ``n`` points be transformed by ``precond='lines'``?  A power of two from 16 runs the row FFT itself (to 8192
    points), any other length the chirp-z identity at the power of two >= 2 n - 1 (csrc/inpaint.hpp)."""
    return 5 <= n <= LINES_MAX_LENGTH or n == 2 * LINES_MAX_LENGTH


def _start_basis(nt, p):
    """Orthonormal start of the block iteration, [p][nt]: a seeded Gaussian block whose first column leans on the constant
    vector (a dynamic spectrum is positive); rows beyond min(nt, p) are zero (deflated from the start)."""
    g = np.random.default_rng(20240229).standard_normal((nt, p))
    g[:, 0] = 1.0 + 0.1 * g[:, 0]
    q = np.linalg.qr(g)[0]
    v0 = np.zeros((p, nt))
    v0[:q.shape[1]] = q.T
    return v0


def svd_device(arr, p, want_corrected=True, info=None):
    """(model, arr / |model|) of the real 2-D ``arr`` from its top ``p`` singular triplets (``scint_svd_model``)."""
    _lib_ready()
    t = device.to_device(arr, torch.float64)
    nf, nt = (int(v) for v in t.shape)
    v0 = device.to_device(_start_basis(nt, p), torch.float64)
    model = device.empty((nf, nt), torch.float64)
    corrected = device.empty((nf, nt), torch.float64) if want_corrected else None
    status = device.empty((12,), torch.float64)
    ws = device.workspace_for("scint_svd_model", nf, nt)
    iters = ctypes.c_int32()
    try:
        _lib.call("scint_svd_model", t, nf, nt, int(p), v0, SVD_TOL, SVD_MAX_ITER, model, corrected, status, iters, ws, ws.numel(),
                  device.stream_ptr())
    except _lib.ScintHipError as err:
        if err.status == _lib.SCINT_E_NONFINITE:
            raise ValueError("svd_model: the array holds a NaN or an infinite element (numpy.linalg.svd does not converge either)") from None
        if err.status == _lib.SCINT_E_NOCONV:
            st = status.cpu().numpy()
            raise _lib.ScintHipError(f"svd_model: the block iteration stopped after {iters.value} steps at a residual of {st[0]:.3g} "
                                     f"(wanted {SVD_TOL:g} * {st[1]:.3g}): singular values {p} and {p + 1} are too close, or mode {p} "
                                     "is below 3 % of the first") from None
        raise
    if info is not None:
        st = status.cpu().numpy()
        info.update(iters=iters.value, residual=st[0], lam_min=st[1], lam_max=st[2], active=int(st[3]), lam=st[4:4 + p].copy())
    return model.cpu().numpy(), (corrected.cpu().numpy() if want_corrected else None)


def _check_nmodes(nmodes):
    if int(nmodes) != nmodes or nmodes < 0:
        raise ValueError("nmodes must be a non-negative integer")
    if nmodes > MAX_MODES:
        raise ValueError(f"nmodes = {nmodes}: the device block iteration carries at most {MAX_MODES} modes")
    return int(nmodes)


def svd_model(arr, nmodes=1, info=None):
    """``ththmod.svd_model`` (ththmod.py:18-35): the model of ``arr`` from its first ``nmodes`` singular triplets, complex128.
    A complex array runs on the same real kernels through its real 2 x 2 block form (every mode then takes two columns)."""
    arr = np.asarray(arr)
    if arr.ndim != 2:
        raise ValueError("svd_model needs a 2-D array")
    nmodes = _check_nmodes(nmodes)
    nf, nt = arr.shape
    if nmodes == 0:
        return np.zeros((nf, nt), np.complex128)
    if np.iscomplexobj(arr):
        re, im = np.ascontiguousarray(arr.real, dtype=float), np.ascontiguousarray(arr.imag, dtype=float)
        m = svd_device(np.block([[re, -im], [im, re]]), 2 * nmodes, want_corrected=False, info=info)[0]
        return m[:nf, :nt] + 1j * m[nf:, :nt]
    return svd_device(np.ascontiguousarray(arr, dtype=float), nmodes, want_corrected=False, info=info)[0].astype(np.complex128)


def nanmean_device(t, axis):
    """np.nanmean of the device array ``t`` along ``axis`` as a host vector."""
    nf, nt = (int(v) for v in t.shape)
    out = device.empty((nf if axis == 1 else nt,), torch.float64)
    need = ctypes.c_size_t()
    _lib.call("scint_nanmean_axis_workspace_bytes", nf, nt, need)
    ws = device.workspace.get(max(need.value, 256))        # (axis 1 needs none: never a null pointer)
    _lib.call("scint_nanmean_axis", t, nf, nt, int(axis), out, ws, ws.numel(), device.stream_ptr())
    return out.cpu().numpy()


def divide_device(t, axis, vec):
    """t[i][j] /= vec[i] (axis 0) or vec[j] (axis 1), in place on the device."""
    nf, nt = (int(v) for v in t.shape)
    v = device.to_device(np.ascontiguousarray(vec, dtype=float), torch.float64)
    _lib.call("scint_divide_axis", t, nf, nt, int(axis), v, device.stream_ptr())


# ----------------------------------------------------------------------------
# the methods
# ----------------------------------------------------------------------------
def zap(self, sigma=7):
    """Basic zapping (RFI mitigation) of the dynamic spectrum (dynspec.py:3856-3870): NaN where the deviation from the median
    exceeds ``sigma`` median deviations.  Both medians and the mask come from the device; every other pixel keeps its bits."""
    out, _, _ = zap_device(self.dyn, sigma)
    np.copyto(self.dyn, out)


_NO_BIHARMONIC = 'Warning: biharmonic inpainting not available.Defaulting to linear interpolation.'   # the reference's text
_DEFAULT_KERNEL = "Warning: kernel size is set to default."


def _whole_line_gaps(bad):
    """(axis, validity flag per line) when the invalid pixels form whole channels (axis 0) or whole sub-integrations (axis 1)."""
    for axis in (0, 1):
        dead = bad.all(axis=1 - axis)
        if np.array_equal(bad, np.expand_dims(dead, 1 - axis) & np.ones_like(bad)):
            return axis, ~dead
    return None


def refill(self, method='biharmonic', zeros=True, kernel_size=5, linear=True):
    """Replace the NaN values (and by default the zeros) of the dynamic spectrum (dynspec.py:3273-3323); see the module text for
    which masks ``'linear'`` accepts.  ``'biharmonic'`` falls back to ``'linear'`` with the reference's warning."""
    if method == 'biharmonic':                          # scikit-image is never used here: the reference's fallback, always
        print(_NO_BIHARMONIC)
        method = 'linear'
    if zeros:
        np.copyto(self.dyn, np.nan, where=(self.dyn == 0))
    if method == 'median':
        if np.ndim(kernel_size) == 0 and kernel_size == 5:
            print(_DEFAULT_KERNEL)
        kf, kt = _kernel_size(kernel_size)
        np.copyto(self.dyn, median_fill_device(self.dyn, kf, kt, np.mean(self.dyn[is_valid(self.dyn)])))
    elif linear and method in ('linear', 'cubic', 'nearest'):
        if method != 'linear':
            raise NotImplementedError(_IRREGULAR.format(method) + " (and 'cubic' / 'nearest' are not built at all)")
        bad = ~is_valid(self.dyn)                       # griddata sees the finite pixels only (np.ma.masked_invalid)
        if bad.all():
            raise ValueError("refill: no valid pixel to interpolate from")
        if not bad.any():
            self.dyn = np.array(self.dyn, dtype=np.float64)
        else:
            found = _whole_line_gaps(bad)
            if found is None:
                raise NotImplementedError(_IRREGULAR.format(method))
            self.dyn = linear_fill_device(self.dyn, *found)
    # every method ends with the mean of the valid pixels in whatever is still NaN (gaps at an edge, linear=False)
    np.copyto(self.dyn, np.mean(self.dyn[is_valid(self.dyn)]), where=np.isnan(self.dyn))


def inpaint(self, zeros=True, tol=INPAINT_TOL, precond=None):
    """Replace the non-finite pixels (and with ``zeros`` the zeros, as ``refill`` does) of the dynamic spectrum by the biharmonic
    fill, in place: what the reference's ``refill()`` computes by default where scikit-image is installed.  Any mask is accepted:
    isolated pixels, blocks, whole channels and sub-integrations together.  ``precond='lines'`` fills bands of whole channels or
    sub-integrations of any width (the default route gives up on gaps some 40 pixels wide).  See ``biharmonic_fill_device``."""
    if precond not in (None, 'lines'):
        raise ValueError(f"inpaint: precond={precond!r}; None or 'lines'")
    if zeros:
        np.copyto(self.dyn, np.nan, where=(self.dyn == 0))
    np.copyto(self.dyn, biharmonic_fill_device(self.dyn, tol=tol, precond=precond))


def _without_zeros(vec):
    """The vector with its exact zeros replaced, in place, by the mean of the whole vector (the zeros included)."""
    vec[vec == 0] = np.mean(vec)
    return vec


def _smoothed(vec, nsmooth):
    if nsmooth is None:
        return vec
    from scipy.signal import savgol_filter
    return savgol_filter(vec, nsmooth, 1)


def correct_dyn(self, svd=True, nmodes=1, frequency=True, time=True, lamsteps=False, nsmooth=None, velocity=False):
    """Correct for apparent flux variations in time and frequency (dynspec.py:3325-3410).  The reference's aliasing is kept: in
    the plain case the working array IS ``self.dyn`` until the first divide makes a new one, so the in-place NaN -> 0, 0 -> NaN and
    NaN -> 0 steps on ``self.dyn`` hit it too; with ``lamsteps`` they hit ``self.dyn`` alone, which nothing then reads."""
    if velocity:
        raise NotImplementedError("correct_dyn of the velocity-scaled spectrum (vdyn) is not ported yet")
    if svd:
        nmodes = _check_nmodes(nmodes)
    if hasattr(self, 'svd_model'):
        print('Warning: An svd_model exists. Check before applying twice')
    if lamsteps and not type(self).lamdyn.present(self):
        self.scale_dyn(lamsteps=lamsteps)
    work = self.lamdyn if lamsteps else self.dyn
    work[np.isnan(work)] = 0

    if svd and nmodes == 0:
        self.svd_model = np.zeros(work.shape, np.complex128)
        work = work / np.abs(self.svd_model)
    elif svd:
        model, work = svd_device(np.ascontiguousarray(work, dtype=float), nmodes)
        self.svd_model = model.astype(np.complex128)
    else:
        on_device = None
        for axis, wanted in ((1, frequency), (0, time)):          # the mean over time per channel, then over frequency
            if not wanted:
                continue
            self.dyn[self.dyn == 0] = np.nan            # (aliases `work` in the plain case until the first divide)
            if on_device is None:
                _lib_ready()
                on_device = device.to_device(np.array(work, dtype=np.float64), torch.float64)
            profile = _without_zeros(nanmean_device(on_device, axis))
            if axis == 1:
                self.bandpass = profile                 # the unsmoothed one is what the reference keeps
            divide_device(on_device, 1 - axis, _smoothed(profile, nsmooth))
        self.dyn[np.isnan(self.dyn)] = 0
        if on_device is not None:
            work = on_device.cpu().numpy()

    if lamsteps:
        self.lamdyn = work
    else:
        self.dyn = work


def _edge_is_empty(line, most_zeros):
    """One look at an edge line (a view of the array): zero it when more than ``most_zeros`` of its pixels are zero; is it all
    zero now?"""
    if np.count_nonzero(line == 0) > most_zeros:
        line[...] = 0
    return not np.any(line)


def _rederive(self, digits, time_step):
    """Shift the time axis to start at zero (the start goes into ``mjd``) and re-derive the sizes, the band and the centre
    frequency, rounded to ``digits`` as the calling method of the reference rounds them."""
    start = np.min(self.times)
    self.mjd += start / 86400
    self.times -= start
    self.nchan, self.nsub = len(self.freqs), len(self.times)
    self.bw = round(max(self.freqs) - min(self.freqs) + self.df, digits)
    self.freq = round(np.mean(self.freqs), digits)
    if time_step:
        self.dt = round(np.mean(np.diff(self.times)), digits)
        self.tobs = round(max(self.times) + self.dt, digits)
        self.df = self.bw / self.nchan


def trim_edges(self, bandwagon_frac=0.5, remove_short_sub=True):
    """Find and remove the band edges (dynspec.py:259-328): NaN -> 0, then each edge line is dropped while it is all zero, an
    edge line with more than ``bandwagon_frac`` zeros being zeroed first.  The thresholds use the array's ORIGINAL sizes on both
    axes, as the reference's do; the attributes are re-derived with its roundings (3 digits; ``df`` becomes ``bw / nchan``).  An
    all-zero array raises ``ValueError`` (the reference's loop runs off the end).  ``remove_short_sub`` is accepted and unused,
    as in the reference."""
    self.dyn[np.isnan(self.dyn)] = 0
    nr, nc = self.dyn.shape
    if not np.any(self.dyn):
        raise ValueError("trim_edges: the dynamic spectrum is zero everywhere")
    # first and last channel, then first and last sub-integration
    for axis, at, most_zeros in ((0, 0, bandwagon_frac * nc), (0, -1, bandwagon_frac * nc),
                                 (1, 0, bandwagon_frac * nr), (1, -1, bandwagon_frac * nr)):
        while _edge_is_empty(self.dyn[at, :] if axis == 0 else self.dyn[:, at], most_zeros):
            self.dyn = np.delete(self.dyn, at, axis=axis)
            if axis == 0:
                self.freqs = np.delete(self.freqs, at)
            else:
                self.times = np.delete(self.times, at)
            if self.dyn.size == 0:
                raise ValueError("trim_edges: every line of the dynamic spectrum was trimmed")
    _rederive(self, 3, time_step=True)


def crop_dyn(self, fmin=0, fmax=np.inf, tmin=0, tmax=np.inf):
    """Crop the dynamic spectrum to fmin..fmax (MHz) and tmin..tmax (minutes) (dynspec.py:3816-3854).  ``bw`` and ``freq`` are
    rounded to 2 digits here; ``tobs`` becomes ``tmax - tmin`` when tmax cuts the observation and ``tobs - tmin`` otherwise (both
    in seconds, not re-derived from the kept samples); ``df`` and ``dt`` keep their values."""
    in_band = (self.freqs >= fmin) & (self.freqs <= fmax)
    first_s, last_s = 60 * tmin, 60 * tmax
    in_span = (self.times >= first_s) & (self.times <= last_s)
    self.tobs = (last_s if last_s < self.tobs else self.tobs) - first_s
    self.dyn = self.dyn[in_band][:, in_span]
    self.freqs, self.times = self.freqs[in_band], self.times[in_span]
    _rederive(self, 2, time_step=False)


def auto_processing(self, lamsteps=False, remove_short_sub=True):
    """The reference's automatic processing (dynspec.py:422-440): its five calls, in its order."""
    self.trim_edges(remove_short_sub=remove_short_sub)
    self.refill()
    self.calc_acf()
    if lamsteps:
        self.scale_dyn()
    self.calc_sspec(lamsteps=lamsteps)
