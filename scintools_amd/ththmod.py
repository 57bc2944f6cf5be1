"""Drop-in for the theta-theta functions of ``scintools.ththmod`` on one MI355X.

Same names, argument order and return values as the reference
(/root/reference/scintools/ththmod.py); the NumPy/SciPy bodies are replaced by
calls into libscint_hip.so:

=================  =====================  ========================================
function           reference lines        HIP entry point(s)
=================  =====================  ========================================
thth_map           ththmod.py:56-116      scint_thth_map
thth_redmap        ththmod.py:119-173     scint_thth_map (crop fused)
rev_map            ththmod.py:176-271     scint_rev_map
modeler            ththmod.py:274-327     scint_thth_map + scint_eigh_top +
                                          scint_rev_map + scint_model_from_recov
chisq_calc         ththmod.py:330-368     ... + scint_chisq
chisq_sweep        (a loop of chisq_calc) scint_chisq_sweep
Eval_calc          ththmod.py:371-401     scint_eval_sweep (one eta)
single_search      ththmod.py:715-895     scint_cs + scint_eval_sweep (+ SciPy fit)
eval_sweep         (the loop :788-799)    scint_eval_sweep
two_curve_map      ththmod.py:1557-1636   scint_two_curve_map
singularvalue_calc ththmod.py:496-513     scint_sv_sweep_multi (one map)
single_search_thin ththmod.py:516-712     scint_cs + scint_sv_sweep_multi (+ SciPy fit)
sv_sweep_multi     (fit_thetatheta thin)  scint_sv_sweep_multi
VLBI_chunk_retrieval ththmod.py:1223-1387 scint_cs_batch + scint_cs_complex_batch +
                                          scint_vlbi_composite + scint_eigh_top_batch +
                                          scint_retrieval_tail
rotMos / fullMos   ththmod.py:1708-1987   scint_mosaic_fit_eval
rotFit + rotDer,   ththmod.py:1773-2102   scint_mosaic_fit_eval (value and gradient
fullMosFit + Grad                         from one evaluation: MosaicStack)
fullMosHess        ththmod.py:2105-2310   scint_mosaic_fit_hess
rotInit            ththmod.py:1791-1856   scint_mosaic_phase + scint_mosaic_add
=================  =====================  ========================================

``tau, fd, eta, edges`` may be bare numbers (us, mHz, s**3, mHz) or, when astropy
is installed, Quantities -- converted exactly as ``unit_checks`` does.  ``CS`` may
be a NumPy array (uploaded on every call) or a ``torch`` complex128 CUDA tensor
(kept where it is; use :func:`to_device` once before a loop).  Results are NumPy
arrays like the reference's.  Grid construction, the crop mask and the parabola
fit stay on the host in NumPy/SciPy, in the reference's operation order.

There is no CPU fallback: without the HIP library or without a GPU every
function raises ``ScintHipError``.
"""
import ctypes
import types
import warnings

import numpy as np
import torch
from scipy.optimize import curve_fit, minimize

from . import _lib, units
from . import device as _dv
from .clean import svd_model  # noqa: F401  (ththmod.py:18-35, on the kernels of correct_dyn: csrc/clean.hpp)
from .device import empty, require_gpu, stream_ptr, workspace, workspace_for

DEFAULT_TOL = 1e-12       # Ritz-residual tolerance of the Lanczos eigen-solver
DEFAULT_MAX_ITER = 300    # Lanczos steps (ARPACK needs 30-50 restarts-equivalent mat-vecs)
DEFAULT_BATCH_BYTES = 32 << 30  # HBM budget for concurrently resident theta-theta matrices (of 288 GB)


# ----------------------------------------------------------------------------
# small host helpers (reference operation order)
# ----------------------------------------------------------------------------
def chi_par(x, A, x0, C):
    """Parabola for fitting the eigenvalue peak (ththmod.py:38-53)."""
    return A * (x - x0) ** 2 + C


def unit_checks(var, name, desired):
    """Reference-compatible unit coercion (ththmod.py:1639-1668); needs astropy
    for anything but bare numbers.  `desired` is an astropy unit."""
    if not units.HAVE_ASTROPY:
        raise _lib.ScintHipError("unit_checks with astropy units needs astropy")
    u = units.u
    var = var * u.dimensionless_unscaled
    if u.dimensionless_unscaled.is_equivalent(var.unit):
        var = var * desired
        warnings.warn(f"{name} missing units. Assuming {desired}.")
    elif desired.is_equivalent(var.unit):
        var = var.to(desired)
    else:
        raise u.UnitConversionError(f"{name} units ({var.unit}) not equivalent to {desired}")
    return var


def fft_axis(x, unit=None, pad=0):
    """Fourier-conjugate axis (ththmod.py:473-493).

    With astropy: same call as the reference (`unit` an astropy unit).  Without:
    `unit` is the scale factor of the conversion -- 1000.0 for s -> mHz, 1.0 for
    MHz -> us -- and a bare ndarray is returned.
    """
    if units.HAVE_ASTROPY and hasattr(x, "unit"):
        fx = np.fft.fftshift(np.fft.fftfreq((pad + 1) * x.shape[0], x[1] - x[0]).to_value(unit)) * unit
        return fx
    scale = 1.0 if unit is None else float(unit)
    fx = np.fft.fftfreq((pad + 1) * x.shape[0], x[1] - x[0])
    if scale != 1.0:
        fx = fx * scale
    return np.fft.fftshift(fx)


def min_edges(fd_lim, fd, tau, eta, factor=2):
    """Smallest edges array that oversamples the CS by `factor` (ththmod.py:1671-1705)."""
    fd_v = units.strip(fd, "fd", "mHz", warn=False)
    tau_v = units.strip(tau, "tau", "us", warn=False)
    eta_v = float(units.strip(eta, "eta", "s3", warn=False))
    lim = float(units.strip(fd_lim, "fD Limit", "mHz", warn=False))
    dtau_lim = (tau_v[1] - tau_v[0]) / factor
    dtau_lim /= 2 * eta_v * lim
    dfd_lim = (fd_v[1] - fd_v[0]) / factor
    npoints = (2 * lim) // (min(dfd_lim, dtau_lim))
    npoints += np.mod(npoints, 2)
    return units.attach(np.linspace(-lim, lim, int(npoints)), "mHz")


def _theta_centres(edges):
    th = (edges[1:] + edges[:-1]) / 2            # ththmod.py:83
    th -= th[np.abs(th) == np.abs(th).min()]     # ththmod.py:84
    return th


class _Grid:
    """Plain-float view of (tau, fd, edges) plus everything the kernels need."""

    def __init__(self, tau, fd, edges):
        self.tau = units.strip(tau, "tau", "us", warn=False)
        self.fd = units.strip(fd, "fd", "mHz", warn=False)
        self.edges = np.array(units.strip(edges, "edges", "mHz", warn=False), dtype=float)
        if self.tau.ndim != 1 or self.fd.ndim != 1 or self.tau.size < 2 or self.fd.size < 2:
            raise ValueError("tau and fd must be 1-D with at least two points")
        self.th_cents = _theta_centres(self.edges)
        g = _lib.CsGeom()
        g.ntau, g.nfd = self.tau.shape[0], self.fd.shape[0]
        g.tau0, g.dtau = float(self.tau[0]), float(np.diff(self.tau).mean())   # ththmod.py:90
        g.fd0, g.dfd = float(self.fd[0]), float(np.diff(self.fd).mean())       # ththmod.py:91
        g.tau_max = float(np.abs(self.tau.max()))
        g.fd_max = float(np.abs(self.fd.max()))
        g.tau1_step = float(self.tau[1] - self.tau[0])
        g.fd1_step = float(self.fd[1] - self.fd[0])
        self.geom = g
        self._th_dev = None

    @property
    def M(self):
        return self.th_cents.shape[0]

    def th_dev(self):
        if self._th_dev is None:
            self._th_dev = to_device(self.th_cents, torch.float64)
        return self._th_dev

    def keep(self, eta):
        """Crop of thth_redmap (ththmod.py:153-155) as ascending indices."""
        th = self.th_cents
        pnts = ((th**2) * eta < self.geom.tau_max) * (np.abs(th) < self.geom.fd_max / 2)
        return np.nonzero(pnts)[0].astype(np.int32)

    def edges_red(self, keep_idx):
        """edges of the reduced map (ththmod.py:157-172)."""
        c = self.th_cents[keep_idx]
        mid = (c[:-1] + c[1:]) / 2
        step = np.diff(mid).mean()
        return np.concatenate((np.array([mid[0] - step]), mid, np.array([mid[-1] + step])))


def to_device(CS, dtype=torch.complex128):
    """Upload a conjugate spectrum once; pass the result as ``CS`` to any function here."""
    return _dv.to_device(CS, dtype)


SWEEP_MAX_CS_ELEMENTS = (1 << 31) - 1    # the packed gather of the sweeps indexes the conjugate spectrum with 32 bits


def _check_sweep_cs(ntau, nfd):
    """The sweeps (eval / eigvec / chisq, single or multi, and the batched retrieval) refuse a conjugate spectrum of 2^31
    elements or more -- 32 GiB of complex128, e.g. a 16384^2 dynspec with npad = 3 -- inside the library (SCINT_E_ARG from
    run_sweep).  Say so here, before any workspace is allocated; the per-curvature entry points (thth_map,
    thth_redmap, modeler, Eval_calc through them) index with 64 bits and take such a spectrum."""
    if int(ntau) * int(nfd) > SWEEP_MAX_CS_ELEMENTS:
        raise ValueError(f"conjugate spectrum of {ntau} x {nfd} = {int(ntau) * int(nfd)} elements: the batched sweeps index it "
                         f"with 32 bits (limit {SWEEP_MAX_CS_ELEMENTS}); use a smaller npad, chunk the observation, or call "
                         "thth_redmap / modeler per curvature")


def _cs_dev(CS, grid):
    t = to_device(CS, torch.complex128)
    if tuple(t.shape) != (grid.geom.ntau, grid.geom.nfd):
        raise ValueError(f"CS shape {tuple(t.shape)} does not match (len(tau), len(fd)) = "
                         f"({grid.geom.ntau}, {grid.geom.nfd})")
    return t


def _eta_float(eta):
    return float(units.strip(eta, "eta", "s3", warn=False))


# ---- what every entry point does with a chunk (dspec2, edges, time, freq, eta) before anything reaches the device
def _chunk_strip(time, freq, edges, names=("time2", "freq2")):
    """(time [s], freq [MHz], edges [mHz]) of a chunk as plain floats; `names`: what a unit error calls time and freq."""
    return (units.strip(time, names[0], "s", warn=False), units.strip(freq, names[1], "MHz", warn=False),
            units.strip(edges, "edges", "mHz", warn=False))


def _chunk_axes(time, freq, edges, npad, names=("time2", "freq2")):
    """(time_v, freq_v, edges_v, tau [us], fd [mHz]): a chunk's axes and edges as plain floats and the conjugate axes of the
    chunk padded `npad` times (ththmod.py:773-774)."""
    time_v, freq_v, edges_v = _chunk_strip(time, freq, edges, names)
    return time_v, freq_v, edges_v, fft_axis(freq_v, 1.0, npad), fft_axis(time_v, 1000.0, npad)


def _chunk_grid(time, freq, edges, npad, cache=None):
    """The _Grid of a chunk.  `cache` (a dict; None: a fresh grid): chunks with equal axes and edges -- those of one frequency
    row -- get ONE object.  961 grid objects were 45 ms of a 0.23-s calc_wavefield before any GPU work was queued, and
    :func:`_multi_keep_dev` and :func:`_reduced_centres_cached` recognise a shared grid by its id.  The objects are read-only to
    their users (axes, centres, geometry).  The key does not hold `npad`: a cache serves one call."""
    time_v, freq_v, edges_v = _chunk_strip(time, freq, edges)
    # (fft_axis reads only the length and the first step of an axis)
    key = (time_v.shape[0], float(time_v[1] - time_v[0]), freq_v.shape[0], float(freq_v[1] - freq_v[0]), edges_v.tobytes())
    grid = None if cache is None else cache.get(key)
    if grid is None:
        grid = _Grid(fft_axis(freq_v, 1.0, npad), fft_axis(time_v, 1000.0, npad), edges_v)
        if cache is not None:
            cache[key] = grid
    return grid


def _tau_mask_rows(tau_v, tauMask):
    """Rows [lo, hi) of the conjugate spectrum that the delay mask |tau| < tauMask clears (ththmod.py:785); (0, 0) for none."""
    sel = np.nonzero(np.abs(tau_v) < float(units.strip(tauMask, "tauMask", "us", warn=False)))[0]
    if not sel.size:
        return 0, 0
    lo, hi = int(sel[0]), int(sel[-1]) + 1
    if hi - lo != sel.size:
        raise ValueError("tau mask is not a contiguous block of delays")
    return lo, hi


def _tau_mask_lohi(grids, tauMask):
    """:func:`_tau_mask_rows` of every chunk of a group as int64 [n, 2], worked out once per distinct grid object."""
    rows = {}
    for g in grids:
        if id(g) not in rows:
            rows[id(g)] = _tau_mask_rows(g.tau, tauMask)
    return np.array([rows[id(g)] for g in grids], dtype=np.int64).reshape(len(grids), 2)


def _reduced_centres_cached(grid, keep, cache):
    """Centres of the reduced edges of crop `keep` (ththmod.py:204-205 applied to :157-172).  A crop that is one run of centres
    is kept in `cache` (a dict) per (grid object, first centre, count): the chunks of a frequency row share it."""
    n = int(keep.shape[0])
    key = (id(grid), int(keep[0]), n) if n == int(keep[-1]) - int(keep[0]) + 1 else None
    th_red = cache.get(key) if key is not None else None
    if th_red is None:
        th_red = _theta_centres(grid.edges_red(keep))
        if key is not None:
            cache[key] = th_red
    return th_red


RETRIEVAL_GROUP_BYTES = 8 << 30   # device bytes a group of chunks may hold at once: the fit's and the retrievals' stacks of conjugate spectra


def _group_size(bytes_per_chunk, group_bytes=None, cap=None):
    """Chunks per group: as many as fit into `group_bytes` (None or 0: RETRIEVAL_GROUP_BYTES), at least one, at most `cap`."""
    n = max(1, int((group_bytes or RETRIEVAL_GROUP_BYTES) // bytes_per_chunk))
    return n if cap is None else min(cap, n)


# ----------------------------------------------------------------------------
# device-level building blocks (torch tensors in, torch tensors out)
# ----------------------------------------------------------------------------
def _thth_dev(cs_t, grid, eta, keep_idx, hermetian):
    require_gpu()
    n = int(keep_idx.shape[0])
    out = empty((n, n), torch.complex128)
    if n == 0:
        return out
    keep_t = to_device(keep_idx, torch.int32)
    _lib.call("scint_thth_map", cs_t, grid.geom, grid.th_dev(), grid.M, keep_t, n, eta, 1 if hermetian else 0, out, stream_ptr())
    return out


def _host_checked(arr, grid, hermetian):
    """NumPy raises IndexError when the non-Hermitian gather wraps an fd index below -len(fd)
    (ththmod.py:104); the kernel marks such pixels NaN.  Checked on the host copy, and only
    when the grid can produce such an index at all (a NaN in CS itself must pass through)."""
    if not hermetian and arr.size:
        g, th = grid.geom, grid.th_cents
        lowest = np.floor(((th.min() - th.max()) - g.fd0 + g.dfd / 2) / g.dfd)
        if lowest < -g.nfd and np.isnan(arr.real).any():
            raise IndexError("theta-theta gather index out of bounds for the conjugate spectrum")
    return arr


def _eigh_top_dev(a_t, v0_t=None, want_vec=True, tol=DEFAULT_TOL, max_iter=DEFAULT_MAX_ITER):
    """Top ('LA') eigenpair of a Hermitian device matrix.  Returns (w float, V tensor|None, iters)."""
    n = int(a_t.shape[0])
    if n < 2:
        raise ValueError("eigen-decomposition needs at least a 2x2 theta-theta matrix")
    ws = workspace_for("scint_eigh_top", n, max_iter)
    w_t = empty((1,), torch.float64)
    st_t = torch.zeros((2,), dtype=torch.int32, device=a_t.device)
    vec_t = empty((n,), torch.complex128) if want_vec else None
    _lib.call("scint_eigh_top", a_t, n, v0_t, tol, max_iter, w_t, vec_t, st_t[0:1], st_t[1:2], ws, ws.numel(), stream_ptr())
    status, iters = (int(v) for v in st_t.cpu())
    if status != _lib.SCINT_OK:
        raise ArithmeticError(f"top-eigenpair iteration failed (status {status}, {iters} steps)")
    return float(w_t.cpu()[0]), vec_t, iters


def _rev_map_dev(grid_geom, th_t, n, eta, hermetian, thth_t=None, vec_t=None, w_t=None, info=None):
    """`info` (a dict, tests): receives `uniform_grid` -- word 9 of the call's scratch, 1 when the rank-1 Hermitian image was
    formed by the uniform-grid kernel (csrc/thth.hip: rev_diag_kernel), 0 when by the general one."""
    recov = empty((grid_geom.ntau, grid_geom.nfd), torch.complex128)
    rank1 = thth_t is None
    scratch = empty((256,), torch.uint8)       # its own buffer: `workspace` may be live in a caller
    _lib.call("scint_rev_map", thth_t, vec_t, w_t, 1 if rank1 else 0, th_t, n, grid_geom, eta, 1 if hermetian else 0, recov,
              scratch, scratch.numel(), stream_ptr())
    if info is not None:
        info["uniform_grid"] = int(scratch.cpu().numpy().view(np.uint64)[9])
    return recov


def _model_dev(recov_t):
    ntau, nfd = (int(v) for v in recov_t.shape)
    ws = workspace_for("scint_model", ntau, nfd)
    model = empty((ntau, nfd), torch.float64)
    _lib.call("scint_model_from_recov", recov_t, ntau, nfd, model, ws, ws.numel(), stream_ptr())
    return model


# ----------------------------------------------------------------------------
# reference API
# ----------------------------------------------------------------------------
def thth_map(CS, tau, fd, eta, edges, hermetian=True):
    """CS -> theta-theta, nearest-bin gather (ththmod.py:56-116)."""
    grid = _Grid(tau, fd, edges)
    cs_t = _cs_dev(CS, grid)
    keep = np.arange(grid.M, dtype=np.int32)
    return _host_checked(_thth_dev(cs_t, grid, _eta_float(eta), keep, hermetian).cpu().numpy(), grid, hermetian)


def thth_redmap(CS, tau, fd, eta, edges, hermetian=True):
    """theta-theta for the largest filled-in square within edges (ththmod.py:119-173).
    Returns (thth_red, edges_red); edges_red carries mHz when astropy is present."""
    grid = _Grid(tau, fd, edges)
    cs_t = _cs_dev(CS, grid)
    e = _eta_float(eta)
    keep = grid.keep(e)
    red = _host_checked(_thth_dev(cs_t, grid, e, keep, hermetian).cpu().numpy(), grid, hermetian)
    return red, units.attach(grid.edges_red(keep), "mHz")


def rev_map(thth, tau, fd, eta, edges, hermetian=True):
    """theta-theta -> CS weighted-histogram inverse map (ththmod.py:176-271)."""
    grid = _Grid(tau, fd, edges)
    e = _eta_float(eta)
    thth_t = to_device(thth, torch.complex128)
    n = grid.M
    if tuple(thth_t.shape) != (n, n):
        raise ValueError(f"thth shape {tuple(thth_t.shape)} does not match len(edges)-1 = {n}")
    recov = _rev_map_dev(grid.geom, grid.th_dev(), n, e, hermetian, thth_t=thth_t)
    return recov.cpu().numpy()


def _modeler_dev(cs_t, grid, e):
    """Device pipeline of modeler; returns tensors (thth_red, V, w float, recov, model, keep)."""
    keep = grid.keep(e)
    red_t = _thth_dev(cs_t, grid, e, keep, True)
    n = int(keep.shape[0])
    w, V_t, _ = _eigh_top_dev(red_t, None, want_vec=True)
    # rev_map runs on the REDUCED edges: their centres are re-derived from edges_red
    # exactly as the reference does (ththmod.py:204-205 applied to :157-172)
    th_red = _theta_centres(grid.edges_red(keep))
    th_red_t = to_device(th_red, torch.float64)
    w_t = to_device(np.array([w]), torch.float64)
    recov_t = _rev_map_dev(grid.geom, th_red_t, n, e, True, vec_t=V_t, w_t=w_t)
    model_t = _model_dev(recov_t)
    return red_t, V_t, w, recov_t, model_t, keep


def modeler(CS, tau, fd, eta, edges, hermetian=True):
    """theta-theta, its rank-1 model, the model CS and model dynamic spectrum
    (ththmod.py:274-327).  Returns (thth_red, thth2_red, recov, model, edges_red, w, V).
    V has an arbitrary global phase (as ARPACK's has)."""
    if not hermetian:
        # the reference's SVD branch double-indexes U[:, 0][:, 0] and raises (ththmod.py:317-320)
        raise IndexError("modeler(hermetian=False) raises in the reference (ththmod.py:317-320)")
    grid = _Grid(tau, fd, edges)
    cs_t = _cs_dev(CS, grid)
    e = _eta_float(eta)
    red_t, V_t, w, recov_t, model_t, keep = _modeler_dev(cs_t, grid, e)
    V = V_t.cpu().numpy()
    thth2_red = np.outer(V, np.conjugate(V))      # ththmod.py:312-313
    thth2_red *= np.abs(w)
    return (red_t.cpu().numpy(), thth2_red, recov_t.cpu().numpy(), model_t.cpu().numpy(),
            units.attach(grid.edges_red(keep), "mHz"), w, V)


def chisq_calc(dspec, CS, tau, fd, eta, edges, N, mask=None):
    """chi**2 of the theta-theta model dynamic spectrum (ththmod.py:330-368)."""
    grid = _Grid(tau, fd, edges)
    cs_t = _cs_dev(CS, grid)
    _, _, _, _, model_t, _ = _modeler_dev(cs_t, grid, _eta_float(eta))
    d_t = to_device(dspec, torch.float64)
    nf, nt = (int(v) for v in d_t.shape)
    m_t = None if mask is None else to_device(np.asarray(mask, dtype=np.uint8), torch.uint8)
    out = empty((1,), torch.float64)
    _lib.call("scint_chisq", model_t, int(model_t.shape[1]), d_t, nf, nt, m_t, N, out, stream_ptr())
    return float(out.cpu()[0])


def default_batch(nmax, neta, eigenvalues_only=True):
    """Curvatures resident per launch: enough mat-vec workgroups to fill the 256 CUs several times over, within the HBM
    budget for the packed matrices (8 N^2 bytes each).

    The unit is the library's own: ``scint_sweep_workgroups(nb)`` mat-vec workgroups per matrix (block rows per workgroup and
    tiles per strip are build constants of the library -- ADVICE r4: the rule used to model the round-2 kernel's strips).  The
    targets are the slot counts measured on MI355X at N = 4095 (nb = 64: 27 workgroups per matrix, complex128 or complex64:
    eight block rows x <= 12 tiles each) times that unit:
      eigenvalue sweep, float64      107 slots (round 4: 69 / 92 / 100 / 108 / 116 -> +0 / +0.3 / +0.6 / +0.8 / +1.0 %; 20 -> 30 at
                                     N = 8191 +0.7 %; 69 -> 108 with npad = 3 +1.6 %)                        -> 2889 workgroups
      eigenPAIR sweeps, float64       90 slots (round 4, per-curvature tail: 836 / 832 / 827 eta/s at 69 / 100 / 128; round 5, batched  -> 2430
                                     tail: 854 / 857-861 / 873 / 870 at 56 / 69 / 90 / 107 on the chi^2 objective)
      mixed eigenvalue sweep         214 slots wanted, 157 within the HBM budget (a slot idles two of its ~19   -> 5778
                                     chunks around the certificate pass; 2400 eta/s, round 5 call 1)
      mixed-all eigenPAIR sweeps     138 slots                                                                 -> 3726"""
    nb = -(-nmax // 64)
    mode = _lib.call("scint_sweep_precision", -1)
    use32 = mode == 2 or (eigenvalues_only and mode == 1)
    wg = max(1, _lib.call("scint_sweep_workgroups", nb, 1 if use32 else 0))
    if use32:
        target = 5778 if eigenvalues_only else 3726
    else:
        target = 2889 if eigenvalues_only else 2430
    want = -(-target // wg)
    per_slot = 8 * (nb * 64) ** 2 + 1
    if use32:
        # a slot of the mixed sweeps also holds the complex64 copy and the Q history (ththmod.DEFAULT_BATCH_BYTES is a budget, not a limit)
        per_slot = per_slot * 3 // 2 + 130 * 32 * nb * 64
    cap = max(1, DEFAULT_BATCH_BYTES // per_slot)
    return int(max(1, min(neta, 256, want, cap)))


def sweep_precision(mode=None):
    """Operand precision of the iteration of the eigenvalue sweeps (``scint_sweep_precision``), per process.

    ``"f64"`` (default): every Lanczos pass streams the complex128 theta-theta.  ``"mixed"``: the passes stream a
    complex64 copy and the eigenvalue returned is the Ritz value of a certificate pass on the complex128 matrix that
    meets the same a-posteriori bound (same ``tol``, same status codes).  ``"mixed-all"``: the eigenPAIR sweeps
    (``eigvec_sweep``, ``chisq_sweep``, the batched retrieval) also iterate on the complex64 copy, and finish the vector on
    the complex128 matrix to the float64 sweep's own residual rule.  ``None`` only queries.  Returns the mode that was in
    force before the call.

    What it buys is HBM bytes: 1.6x the sweep rate at N = 4095 on one MI355X.  Sweeps of small matrices
    (the 64 x 150 chunks of the tutorial data: N ~ 100) are bound by launch latency, not bytes, and a curvature spends
    two to three extra chunks of passes around its certificate: leave those in ``"f64"``."""
    codes = {None: -1, "f64": 0, "mixed": 1, "mixed-all": 2}
    if mode not in codes:
        raise ValueError("sweep_precision: mode must be 'f64', 'mixed', 'mixed-all' or None")
    return {0: "f64", 1: "mixed", 2: "mixed-all"}[_lib.call("scint_sweep_precision", codes[mode])]


def _sweep_open(CS, tau, fd, etas, edges):
    """What every single-chunk sweep starts with: (grid, conjugate spectrum on the device, curvatures as a float64 array)."""
    grid = _Grid(tau, fd, edges)
    _check_sweep_cs(grid.geom.ntau, grid.geom.nfd)
    cs_t = _cs_dev(CS, grid)
    etas_v = np.ascontiguousarray(np.atleast_1d(units.strip(etas, "etas", "s3", warn=False)).astype(float))
    return grid, cs_t, etas_v


def _sweep_results(val_t, st_t):
    """What every sweep ends with: (values[neta] on the host, NaN where the curvature's status is not 0; st[2, neta] = status,
    Lanczos steps)."""
    val = val_t.cpu().numpy()
    st = st_t.cpu().numpy()
    val[st[0] != 0] = np.nan
    return val, st


def _split_chunks(val, bounds):
    return [val[bounds[i]:bounds[i + 1]] for i in range(len(bounds) - 1)]


def eval_sweep(CS, tau, fd, etas, edges, tol=DEFAULT_TOL, max_iter=DEFAULT_MAX_ITER, batch=None,
               return_info=False):
    """Dominant eigenvalue for every curvature in `etas`: the loop of
    single_search (ththmod.py:788-799) as one batched device call.

    Failed curvatures are NaN, as in the reference.  With `return_info` also
    returns a dict with per-eta matrix sizes N, Lanczos steps and status."""
    grid, cs_t, etas_v = _sweep_open(CS, tau, fd, etas, edges)
    neta, M = etas_v.shape[0], grid.M
    keep_t, keep_n = _sweep_inputs_dev(grid, etas_v)
    nmax = max(int(keep_n.max()), 1)
    if batch is None:
        batch = default_batch(nmax, neta)
    ws = workspace_for("scint_eval_sweep", M, neta, batch, max_iter)
    eigs_t = empty((neta,), torch.float64)
    st_t = empty((2, neta), torch.int32)              # status / step counts: initialised inside the library
    _lib.call("scint_eval_sweep", cs_t, grid.geom, grid.th_dev(), M, keep_t, keep_n, etas_v, neta, tol, max_iter, batch,
              eigs_t, st_t[0], st_t[1], ws, ws.numel(), stream_ptr())
    eigs, st = _sweep_results(eigs_t, st_t)           # failures -> NaN (ththmod.py:795-799)
    if return_info:
        return eigs, {"N": keep_n.copy(), "iters": st[1].copy(), "status": st[0].copy(), "batch": batch}
    return eigs


def _keep_ranges(grid, etas_v):
    """The crop of thth_redmap (ththmod.py:153-155) as index RANGES: (first[neta], n[neta]) with keep_i =
    arange(first_i, first_i + n_i), or None when the crop need not be one run of centres (theta not sorted, a negative
    curvature).  On sorted centres ``(th**2 * eta < tau_max) * (|th| < fd_max / 2)`` is a prefix of the centres
    >= 0 and a suffix of those < 0 (every operation is monotone in its rounded operand), so both ends come from a
    bisection with the reference's own expression at the probes: 2 x 13 vector steps over the curvatures instead of
    neta masks over all M centres (the Python loop of :func:`_sweep_inputs` was 1 % of a 4096^2 / 256-eta chi^2 step)."""
    th = grid.th_cents
    M = th.shape[0]
    if M < 1 or not np.all(np.diff(th) >= 0) or np.any(etas_v < 0) or not np.all(np.isfinite(th)):
        return None
    th2, inside, tau_max = th**2, np.abs(th) < grid.geom.fd_max / 2, grid.geom.tau_max
    z = int(np.searchsorted(th, 0.0, side="left"))        # th[z:] >= 0

    def kept(i):                                            # the reference's mask at centre i[k] for curvature k
        return (th2[i] * etas_v < tau_max) * inside[i]

    def first_false(lo, hi, flip):
        """per curvature: the number of kept centres walking from `lo` towards `hi` (exclusive), ascending or descending"""
        lo = np.full(etas_v.shape, lo, dtype=np.int64)
        hi = np.full(etas_v.shape, hi, dtype=np.int64)
        while np.any(lo < hi):
            mid = np.minimum((lo + hi) // 2, hi - 1)         # (a finished curvature probes a valid centre and ignores it)
            mid = np.maximum(mid, 0)
            ok = kept(z - 1 - mid if flip else z + mid) & (lo < hi)
            lo = np.where(ok, mid + 1, lo)
            hi = np.where(ok | (lo >= hi), hi, mid)
        return lo
    npos = first_false(0, M - z, False) if M > z else np.zeros(etas_v.shape, dtype=np.int64)
    nneg = first_false(0, z, True) if z > 0 else np.zeros(etas_v.shape, dtype=np.int64)
    return (z - nneg).astype(np.int64), (nneg + npos).astype(np.int32)


def _sweep_inputs(grid, etas_v):
    """Crop of thth_redmap (ththmod.py:153-155) for every curvature: keep_idx[neta, M]
    (left-packed ascending indices) and keep_n[neta]; same element-wise arithmetic as
    ``_Grid.keep`` with the eta-independent parts hoisted.  Curvatures that keep the same run of centres
    (:func:`_keep_ranges`) share one row."""
    th = grid.th_cents
    neta, M = etas_v.shape[0], grid.M
    keep_idx = np.zeros((neta, M), dtype=np.int32)
    keep_n = np.zeros(neta, dtype=np.int32)
    rng = _keep_ranges(grid, etas_v)
    if rng is not None:
        first, keep_n = rng
        ar = np.arange(M, dtype=np.int32)
        for a, n in {(int(a), int(n)) for a, n in zip(first, keep_n) if n > 0}:
            keep_idx[(first == a) & (keep_n == n), :n] = ar[a:a + n]
        return keep_idx, keep_n
    th2, inside, tau_max = th**2, np.abs(th) < grid.geom.fd_max / 2, grid.geom.tau_max
    for i, e in enumerate(etas_v):
        k = np.nonzero((th2 * e < tau_max) * inside)[0]
        keep_n[i] = k.shape[0]
        keep_idx[i, : k.shape[0]] = k
    return keep_idx, keep_n


def _reduced_centres_of_ranges(grid, first, keep_n):
    """:func:`_reduced_centres` for crops that are index RANGES of sorted centres (:func:`_keep_ranges`), without the
    [neta, M] index table: (th_red[neta, M], group[neta]).  The reference's arithmetic per crop (ththmod.py:157-172, then :83-84)
    is  mid = (c[:-1] + c[1:]) / 2,  step = diff(mid).mean(),  e = [mid[0] - step, mid, mid[-1] + step],  t = (e[1:] + e[:-1]) / 2,
    t -= t[|t| == |t|.min()].  Every interior value of t is (mid[k-1] + mid[k]) / 2 of the FULL grid's mids -- the same two
    operands, the same rounding, whatever the crop -- so a crop's row is a slice of one array with its two end values and its
    own `step` (a mean over the crop's slice of diff(mid): the same numbers in the same order) put in, and the subtracted
    centre is the full grid's innermost one unless an end value is closer to zero (then the crop takes the generic path).
    Bit-identical to the generic path (tests/test_arcfit_host_cpu.py); 7.5 -> 1 ms for the 96 distinct crops of the headline sweep."""
    th = grid.th_cents
    M, neta = th.shape[0], first.shape[0]
    th_red = np.zeros((neta, M))
    group = np.full(neta, -1, dtype=np.int32)
    if M < 3:
        return None
    mid = (th[:-1] + th[1:]) / 2                       # mid[k] between centres k and k + 1
    dmid = np.diff(mid)
    cen = np.zeros(M)
    cen[1:M - 1] = (mid[1:] + mid[:-1]) / 2            # cen[j], 1 <= j <= M - 2: the interior value of any crop that holds j inside
    inner = np.abs(cen[1:M - 1])
    if inner.size == 0:
        return None
    j0 = 1 + int(np.argmin(inner))
    v0 = float(inner[j0 - 1])
    unique = int(np.sum(inner == v0)) == 1
    done = {}
    for i in range(neta):
        a, n = int(first[i]), int(keep_n[i])
        if n < 3:
            continue
        j = done.get((a, n))
        if j is not None:
            th_red[i, :n] = th_red[j, :n]
            group[i] = j
            continue
        m0, m1 = mid[a], mid[a + n - 2]                # mid[0], mid[-1] of the crop
        step = dmid[a:a + n - 2].mean() if n > 2 else np.nan
        t0 = (m0 + (m0 - step)) / 2                    # (e[1] + e[0]) / 2
        t1 = ((m1 + step) + m1) / 2                    # (e[n] + e[n - 1]) / 2
        if unique and a < j0 < a + n - 1 and abs(t0) > v0 and abs(t1) > v0:
            row = cen[a:a + n].copy()
            row[0], row[n - 1] = t0, t1
            row -= cen[j0]
            th_red[i, :n] = row
        else:                                          # an end value is the innermost one, or a tie: the reference's expression as it stands
            th_red[i, :n] = _theta_centres(grid.edges_red(np.arange(a, a + n)))
        done[(a, n)] = i
        group[i] = i
    return th_red, group


def _reduced_centres(grid, keep_idx, keep_n, return_groups=False):
    """th_red[neta, M]: the centres of the reduced edges, re-derived as rev_map does (ththmod.py:204-205 on :157-172),
    one evaluation per DISTINCT crop (on the bench workload 161 of 256 curvatures keep all 4095 centres).
    With `return_groups` also group[neta] int32: curvatures with the same id have the SAME row (copied, element for
    element) -- what ``scint_chisq_sweep`` needs to share the back-map's partner table between them; -1 = no row."""
    neta, M = keep_idx.shape
    th_red = np.zeros((neta, M))
    group = np.full(neta, -1, dtype=np.int32)
    done = {}
    for i in range(neta):
        n = int(keep_n[i])
        if n < 3:                                   # (two centres have no mean edge step: the reference's rev_map raises)
            continue
        key = (int(keep_idx[i, 0]), int(keep_idx[i, n - 1]), n)
        j = done.get(key)
        if j is not None and (key[1] - key[0] + 1 == n or np.array_equal(keep_idx[i, :n], keep_idx[j, :n])):
            th_red[i, :n] = th_red[j, :n]
            group[i] = j
        else:
            th_red[i, :n] = _theta_centres(grid.edges_red(keep_idx[i, :n]))
            done[key] = i
            group[i] = i
    return (th_red, group) if return_groups else th_red


def _sweep_inputs_dev(grid, etas_v):
    """The same crop tables built on the device (``scint_sweep_keep``: NumPy's expression with its roundings):
    keep_idx as a device tensor [neta, M], keep_n on the host.  For the eigenvalue sweep, whose host side needs
    only the counts -- the Python loop of :func:`_sweep_inputs` and the 4 MB upload of its table were 3 % of a
    4096^2 / 256-eta step."""
    neta, M = etas_v.shape[0], grid.M
    keep_t = empty((neta, M), torch.int32)
    n_t = empty((neta,), torch.int32)
    _lib.call("scint_sweep_keep", grid.th_dev(), M, np.ascontiguousarray(etas_v, dtype=np.float64), neta, grid.geom.tau_max,
              grid.geom.fd_max / 2, keep_t, n_t, stream_ptr())
    return keep_t, n_t.cpu().numpy()


def eigvec_sweep(CS, tau, fd, etas, edges, tol=DEFAULT_TOL, max_iter=DEFAULT_MAX_ITER, batch=None):
    """Dominant eigenpair of the reduced theta-theta for every curvature: modeler's
    ``eigsh(thth_red, 1, which="LA")`` (ththmod.py:308) as one batched device call.

    Returns (w[neta] float64 signed, V device tensor [neta, M] complex128 -- row i holds
    N_i = len(keep_i) entries, unit norm, arbitrary phase --, info dict)."""
    grid, cs_t, etas_v = _sweep_open(CS, tau, fd, etas, edges)
    neta, M = etas_v.shape[0], grid.M
    keep_idx, keep_n = _sweep_inputs(grid, etas_v)
    nmax = max(int(keep_n.max()), 1)
    if batch is None:
        batch = default_batch(nmax, neta, eigenvalues_only=False)
    ws = workspace_for("scint_eigvec_sweep", M, neta, batch, max_iter)
    keep_t = _dv.to_device(keep_idx, torch.int32)
    w_t = empty((neta,), torch.float64)
    V_t = empty((neta, M), torch.complex128)          # zeroed (rows are N_i entries long) and filled inside the library
    st_t = empty((2, neta), torch.int32)              # status / step counts: initialised inside the library
    _lib.call("scint_eigvec_sweep", cs_t, grid.geom, grid.th_dev(), M, keep_t, keep_n, etas_v, neta, tol, max_iter, batch,
              w_t, V_t, M, st_t[0], st_t[1], ws, ws.numel(), stream_ptr())
    w, st = _sweep_results(w_t, st_t)
    info = {"N": keep_n.copy(), "iters": st[1].copy(), "status": st[0].copy(), "batch": batch,
            "keep_idx": keep_idx, "w_dev": w_t}
    return w, V_t, info


def chisq_sweep(dspec, CS, tau, fd, etas, edges, N, mask=None, return_info=False, tol=DEFAULT_TOL,
                max_iter=DEFAULT_MAX_ITER, batch=None, share_walk=True):
    """chi**2 of the theta-theta model for every curvature: the loop
    ``[chisq_calc(dspec, CS, tau, fd, eta, edges, N, mask) for eta in etas]``
    (ththmod.py:330-368) as ONE device call (``scint_chisq_sweep``): the eigenpairs of all
    curvatures come from the batched Lanczos sweep, and as each curvature retires its rank-1
    back-map, inverse FFT and chi**2 reduction are chained on a side stream while the sweep goes
    on -- no per-eta round trip through Python.  ``share_walk`` (default): curvatures that keep the same theta centres
    share the partner table of their back-maps (same pairs, same sums: not a bit changes; False exists for the test of that)."""
    grid, cs_t, etas_v = _sweep_open(CS, tau, fd, etas, edges)
    neta, M = etas_v.shape[0], grid.M
    # crop tables: when the crops are index ranges of sorted centres (always on the grids of the path) the [neta, M] index table is
    # built on the device and the reduced centres from the ranges alone (round 5: the host tables were 2.8 ms of a 290-ms step)
    rng = _keep_ranges(grid, etas_v)
    fast = _reduced_centres_of_ranges(grid, rng[0], rng[1]) if rng is not None else None
    if fast is not None:
        keep_t, keep_n = _sweep_inputs_dev(grid, etas_v)
        # the device table and the host bisection evaluate the same expression; th_red and crop_group below describe the host
        # ranges, the library walks the device table: the counts AND both ends of every run must agree (a run with the same
        # count but another start, or a mask that is not one run, would pair th_red with other centres -- ADVICE r5)
        same = np.array_equal(keep_n, rng[1])
        if same and neta:
            nz = keep_n > 0
            last = torch.from_numpy(np.maximum(keep_n.astype(np.int64) - 1, 0)).to(keep_t.device)
            ends = torch.stack([keep_t[:, 0], keep_t.gather(1, last[:, None])[:, 0]]).cpu().numpy()
            same = (np.array_equal(ends[0][nz], rng[0][nz]) and np.array_equal(ends[1][nz], (rng[0] + keep_n - 1)[nz]))
        if not same:
            fast = None
    if fast is not None:
        th_red, crop_group = fast
    else:
        keep_idx, keep_n = _sweep_inputs(grid, etas_v)
        th_red, crop_group = _reduced_centres(grid, keep_idx, keep_n, return_groups=True)
        keep_t = _dv.to_device(keep_idx, torch.int32)
    if batch is None:
        batch = default_batch(max(int(keep_n.max()), 1), neta, eigenvalues_only=False)
    d_t = _dv.to_device(dspec, torch.float64)
    nf, nt = (int(v) for v in d_t.shape)
    m_t = None if mask is None else _dv.to_device(np.asarray(mask, dtype=np.uint8), torch.uint8)
    if not share_walk:
        crop_group = np.full(neta, -1, dtype=np.int32)
    crop_group = np.ascontiguousarray(crop_group, dtype=np.int32)
    keep_n = np.ascontiguousarray(keep_n, dtype=np.int32)
    th_red_t = _dv.to_device(th_red, torch.float64)
    ws = workspace_for("scint_chisq_sweep", M, neta, batch, max_iter, grid.geom.ntau, grid.geom.nfd, nf, nt)
    out = empty((neta,), torch.float64)               # NaN-initialised inside the library
    w_t = empty((neta,), torch.float64)
    V_t = empty((neta, M), torch.complex128)          # zeroed (rows are N_i entries long) and filled inside the library
    st_t = empty((2, neta), torch.int32)
    _lib.call("scint_chisq_sweep", cs_t, grid.geom, grid.th_dev(), M, keep_t, keep_n, etas_v, neta, tol, max_iter, batch,
              th_red_t, crop_group, d_t, nf, nt, m_t, N, out, w_t, V_t, M, st_t[0], st_t[1], ws, ws.numel(), stream_ptr())
    st = st_t.cpu().numpy()
    chis = out.cpu().numpy()
    chis[(st[0] != 0) | (keep_n < 3)] = np.nan   # failed curvatures (the reference's loop would raise there)
    if return_info:
        w = w_t.cpu().numpy()
        w[(st[0] != 0) | (keep_n < 3)] = np.nan      # as chis: no model exists for these curvatures
        fused, redone = ctypes.c_int32(), ctypes.c_int64()
        _lib.call("scint_chisq_sweep_last_route", fused, redone)
        return chis, {"w": w, "N": keep_n.copy(), "iters": st[1].copy(), "status": st[0].copy(), "batch": batch,
                      "fused": bool(fused.value), "redone": int(redone.value)}
    return chis


def Eval_calc(CS, tau, fd, eta, edges):
    """Dominant eigenvalue of the reduced theta-theta at one curvature (ththmod.py:371-401)."""
    eigs, info = eval_sweep(CS, tau, fd, np.array([_eta_float(eta)]), edges, return_info=True)
    if info["status"][0] != 0:
        raise ArithmeticError(f"Eval_calc failed (status {int(info['status'][0])})")
    return float(eigs[0])


def _multi_keep_dev(G, etas_all, th_stack):
    """Crop tables of MANY chunks on the device: one [neta_total, M] index tensor, filled chunk by chunk by ``scint_sweep_keep``
    (each chunk has its own theta centres and axes), and the counts on the host after ONE read-back.  Round 5: the host loop
    of :func:`_sweep_inputs` over 256 chunks and the upload of its 171-MB table were a tenth of a ``fit_thetatheta`` of a 4096^2
    observation (bench.py --workload fit_thetatheta)."""
    M = G[0].M
    # (round 6) chunks that share their grid OBJECT and their curvatures (the chunks of one frequency row of the phase retrieval, where
    # chunk_retrieval_batch makes one grid per row) share their table: one call per distinct (grid, curvatures), rows expanded on the device
    first_of, cls_of = {}, []
    for c, (g, et) in enumerate(zip(G, etas_all)):
        cls_of.append(first_of.setdefault((id(g), et.tobytes()), c))
    uniq = sorted(set(cls_of))
    off_u, off = {}, 0
    for c in uniq:
        off_u[c] = off
        off += int(etas_all[c].shape[0])
    keep_u = empty((max(off, 1), M), torch.int32)
    n_u = empty((max(off, 1),), torch.int32)
    for c in uniq:
        g, et = G[c], etas_all[c]
        ne = int(et.shape[0])
        if ne == 0:
            continue
        o = off_u[c]
        _lib.call("scint_sweep_keep", th_stack[c], M, np.ascontiguousarray(et, dtype=np.float64), ne, g.geom.tau_max,
                  g.geom.fd_max / 2, keep_u[o:o + ne], n_u[o:o + ne], stream_ptr())
    n_host = np.ascontiguousarray(n_u.cpu().numpy(), dtype=np.int32)
    if len(uniq) == len(G):
        return keep_u[:off], n_host[:off]
    rows = np.concatenate([np.arange(off_u[cls_of[c]], off_u[cls_of[c]] + etas_all[c].shape[0], dtype=np.int64) for c in range(len(G))]) \
        if len(G) else np.zeros(0, dtype=np.int64)
    keep_t = keep_u.index_select(0, _dv.to_device(rows, torch.int64))
    return keep_t, np.ascontiguousarray(n_host[rows], dtype=np.int32)


def _multi_sweep_inputs(cs_stack, grids, etas_list):
    """What the sweeps over MANY chunks start with: the grids as ``_Grid``s, the stack checked against them, the curvatures of
    all chunks in one array (``etas_v``; chunk c owns ``bounds[c]:bounds[c + 1]``, ``cs_idx`` names each curvature's spectrum), the
    geometry array and the theta centres of every chunk, and the crop tables (``keep_t`` on the device, ``keep_cnt`` on the host)."""
    G = [g if isinstance(g, _Grid) else _Grid(*g) for g in grids]
    ncs = len(G)
    cs_t = _dv.to_device(cs_stack, torch.complex128)
    if cs_t.dim() != 3 or cs_t.shape[0] != ncs:
        raise ValueError("cs_stack must be [nchunk, ntau, nfd] with one spectrum per grid")
    M = G[0].M
    if any(g.M != M or (g.geom.ntau, g.geom.nfd) != tuple(cs_t.shape[1:]) for g in G):
        raise ValueError("all chunks must share the CS shape and the number of edges")
    _check_sweep_cs(G[0].geom.ntau, G[0].geom.nfd)
    etas_all = [np.atleast_1d(units.strip(et, "etas", "s3", warn=False)).astype(float) for _, et in zip(G, etas_list)]
    etas_v = np.ascontiguousarray(np.concatenate(etas_all))
    cs_idx = np.ascontiguousarray(np.concatenate([np.full(et.shape[0], c, dtype=np.int32) for c, et in enumerate(etas_all)]))
    th_stack = _dv.to_device(np.stack([g.th_cents for g in G]), torch.float64)
    keep_t, keep_cnt = _multi_keep_dev(G, etas_all, th_stack)
    return types.SimpleNamespace(G=G, ncs=ncs, cs_t=cs_t, cs_stride=int(cs_t.shape[1] * cs_t.shape[2]), M=M, etas_all=etas_all,
                                 etas_v=etas_v, cs_idx=cs_idx, neta=etas_v.shape[0], th_stack=th_stack,
                                 geoms=(_lib.CsGeom * ncs)(*[g.geom for g in G]), keep_t=keep_t, keep_cnt=keep_cnt,
                                 bounds=np.cumsum([0] + [e.shape[0] for e in etas_all]))


def eval_sweep_multi(cs_stack, grids, etas_list, tol=DEFAULT_TOL, max_iter=DEFAULT_MAX_ITER, batch=None,
                     return_info=False):
    """Eigenvalue curves of MANY chunks in one batched device call -- the chunk loop of
    Dynspec.fit_thetatheta (dynspec.py:1681-1719).

    cs_stack: CUDA complex128 tensor [nchunk, ntau, nfd]; grids: one (tau, fd, edges) triple per
    chunk (all conjugate spectra one shape, all edges one length); etas_list: per-chunk eta
    arrays.  Returns a list of eigenvalue arrays (NaN where a curvature failed)."""
    s = _multi_sweep_inputs(cs_stack, grids, etas_list)
    if batch is None:
        batch = default_batch(max(int(s.keep_cnt.max()), 1), s.neta)
    ws = workspace_for("scint_eval_sweep_multi", s.M, s.neta, batch, max_iter, s.ncs)
    eigs_t = empty((s.neta,), torch.float64)
    st_t = empty((2, s.neta), torch.int32)
    _lib.call("scint_eval_sweep_multi", s.cs_t, s.ncs, s.cs_stride, s.cs_idx, s.geoms, s.th_stack, s.M, s.keep_t, s.keep_cnt,
              s.etas_v, s.neta, tol, max_iter, batch, eigs_t, st_t[0], st_t[1], ws, ws.numel(), stream_ptr())
    eigs, st = _sweep_results(eigs_t, st_t)
    out = _split_chunks(eigs, s.bounds)
    if return_info:
        return out, {"N": s.keep_cnt, "iters": st[1], "status": st[0], "batch": batch}
    return out


def eigvec_sweep_multi(cs_stack, grids, etas_list, tol=DEFAULT_TOL, max_iter=DEFAULT_MAX_ITER, batch=None):
    """Dominant eigenPAIRS of MANY chunks in one batched device call: modeler's
    ``eigsh(thth_red, 1, which="LA")`` (ththmod.py:308) for every (chunk, eta) -- what
    Dynspec.thetatheta_chunks needs from its per-chunk modeler calls (dynspec.py:1765-1826).

    Arguments as :func:`eval_sweep_multi`.  Returns (w list of float64 arrays, V device tensor
    [n_total, M] complex128 in chunk order, keep list of index arrays per (chunk, eta), info)."""
    s = _multi_sweep_inputs(cs_stack, grids, etas_list)
    keep_t, keep_cnt = s.keep_t, s.keep_cnt
    # the callers want the kept indices on the host too: from the crop RANGES where the crops are ranges (sorted centres, eta >= 0:
    # the same expression at the bisection's probes), else from the device table
    keeps, rows_host, keep_cache = [], None, {}
    for g, et in zip(s.G, s.etas_all):
        if et.shape[0] == 1:                       # (one curvature per chunk, the phase retrieval's case: the mask itself is cheaper than a bisection)
            kk = keep_cache.get((id(g), float(et[0])))
            if kk is None:
                kk = keep_cache.setdefault((id(g), float(et[0])), g.keep(float(et[0])))
            if kk.shape[0] == int(keep_cnt[len(keeps)]):
                keeps.append(kk)
                continue
        rng = _keep_ranges(g, et)
        for k in range(et.shape[0]):
            i = len(keeps)
            if rng is not None and int(rng[1][k]) == int(keep_cnt[i]):
                keeps.append(np.arange(int(rng[0][k]), int(rng[0][k]) + int(rng[1][k]), dtype=np.int32))
            else:
                if rows_host is None:
                    rows_host = keep_t.cpu().numpy()
                keeps.append(rows_host[i, : keep_cnt[i]].copy())
    if batch is None:
        batch = default_batch(max(int(keep_cnt.max()), 1), s.neta, eigenvalues_only=False)
    ws = workspace_for("scint_eigvec_sweep_multi", s.M, s.neta, batch, max_iter, s.ncs)
    w_t = empty((s.neta,), torch.float64)
    V_t = empty((s.neta, s.M), torch.complex128)
    st_t = empty((2, s.neta), torch.int32)
    _lib.call("scint_eigvec_sweep_multi", s.cs_t, s.ncs, s.cs_stride, s.cs_idx, s.geoms, s.th_stack, s.M, keep_t, keep_cnt,
              s.etas_v, s.neta, tol, max_iter, batch, w_t, V_t, s.M, st_t[0], st_t[1], ws, ws.numel(), stream_ptr())
    w, st = _sweep_results(w_t, st_t)
    return (_split_chunks(w, s.bounds), V_t, keeps,
            {"N": keep_cnt, "iters": st[1], "status": st[0], "batch": batch, "bounds": s.bounds})


def conjugate_spectrum(dspec, npad, tau=None, tau_mask=0.0, coher=True, pad_value=None, out=None):
    """Device conjugate spectrum of a chunk (ththmod.py:777-787): returns a CUDA
    complex128 tensor [(npad+1)*nf, (npad+1)*nt] (written into `out` when given)."""
    if pad_value is None and not isinstance(dspec, torch.Tensor):
        # the reference's own expression for the padding value, `dspec.mean()` in NumPy (ththmod.py:783), while the chunk is still
        # on the host: the same bits whether the chunk comes alone (single_search) or in a group's array (Dynspec._fit_chunks,
        # chunk_retrieval_batch), and no device mean to read back
        pad_value = float(np.ascontiguousarray(dspec, dtype=float).mean())
    d_t = to_device(dspec, torch.float64)
    nf, nt = (int(v) for v in d_t.shape)
    if pad_value is None:
        m = ctypes.c_double()
        _lib.call("scint_mean", d_t, nf * nt, m, stream_ptr())
        pad_value = m.value
    R = (npad + 1) * nf
    lo, hi = (0, 0) if tau is None else _tau_mask_rows(units.strip(tau, "tau", "us", warn=False), tau_mask)
    ws = workspace_for("scint_cs", nf, nt, npad)
    cs_t = empty((R, (npad + 1) * nt), torch.complex128) if out is None else out
    if tuple(cs_t.shape) != (R, (npad + 1) * nt) or cs_t.dtype != torch.complex128 or not cs_t.is_contiguous():
        raise ValueError("conjugate_spectrum: `out` must be a contiguous complex128 tensor of the padded shape")
    _lib.call("scint_cs", d_t, nf, nt, npad, pad_value, lo, hi, 0 if coher else 1, cs_t, ws, ws.numel(), stream_ptr())
    return cs_t


def fit_eig_peak(etas, eigs, fw):
    """Parabola fit around the eigenvalue peak (ththmod.py:814-859), host SciPy.
    Returns (eta_fit, eta_sig, popt) -- NaN, NaN, None on failure."""
    try:
        good = np.isfinite(eigs)
        etas = etas[good]
        eigs = eigs[good]
        sel = np.abs(etas - etas[eigs == eigs.max()]) < fw * etas[eigs == eigs.max()]
        etas_fit = etas[sel]
        eigs_fit = eigs[sel]
        C = eigs_fit.max()
        x0 = etas_fit[eigs_fit == C][0]
        if x0 == etas_fit[0]:
            A = (eigs_fit[-1] - C) / ((etas_fit[-1] - x0) ** 2)
        else:
            A = (eigs_fit[0] - C) / ((etas_fit[0] - x0) ** 2)
        popt, _ = curve_fit(chi_par, etas_fit, eigs_fit, p0=np.array([A, x0, C]))
        eta_fit = popt[1]
        eta_sig = np.sqrt((eigs_fit - chi_par(etas_fit, *popt)).std() / np.abs(popt[0]))
        return eta_fit, eta_sig, popt
    except Exception:
        return np.nan, np.nan, None


def single_search(params):
    """Curvature search for one chunk (ththmod.py:715-895).

    params = [dspec2, freq, time, etas, edges, name, plot, fw, npad, coher,
    tauMask, verbose] as in the reference.  Plotting is not supported (the
    reference's plot_func is matplotlib-only); `plot=True` is ignored with a
    warning.  Returns (eta_fit, eta_sig, freq.mean(), time.mean(), eigs).
    """
    (dspec2, freq, time, etas, edges, name, plot, fw, npad, coher, tauMask, verbose) = params
    time_v, freq_v, edges_v, tau, fd = _chunk_axes(time, freq, edges, npad, ("time", "freq"))
    etas_v = units.strip(etas, "etas", "s3", warn=False)
    cs_t = conjugate_spectrum(dspec2, npad, tau, tauMask, coher)
    eigs = eval_sweep(cs_t, tau, fd, etas_v, edges_v)
    eta_fit, eta_sig, _ = fit_eig_peak(etas_v, eigs, fw)
    if plot:
        warnings.warn("scintools_amd.single_search does not plot")
    if verbose:
        print(f"Chunk completed (eta = {eta_fit} +- {eta_sig} at {freq_v.mean()})", flush=True)
    if np.isfinite(eta_fit):
        eta_fit, eta_sig = units.attach(eta_fit, "s3"), units.attach(eta_sig, "s3")
    # the reference returns the curve with failed curvatures removed (ththmod.py:817)
    return (eta_fit, eta_sig, units.attach(freq_v.mean(), "MHz"), units.attach(time_v.mean(), "s"),
            eigs[np.isfinite(eigs)])


# ----------------------------------------------------------------------------
# phase retrieval
# ----------------------------------------------------------------------------
def _ifft2_shifted_dev(x_t, scale=1.0, crop=None):
    """scale * ifft2(ifftshift(x))[:crop[0], :crop[1]] on the device (complex128)."""
    rows, cols = (int(v) for v in x_t.shape)
    cr, cc = crop if crop is not None else (rows, cols)
    ws = workspace_for("scint_fft2", rows, cols)
    out = empty((cr, cc), torch.complex128)
    _lib.call("scint_ifft2_shifted", x_t, rows, cols, scale, cr, cc, out, ws, ws.numel(), stream_ptr())
    return out


def _wavefield_from_eigpair(grid, e, keep, V, w, shape, row_t=None, th_t=None):
    """Chunk wavefield from the dominant eigenpair (ththmod.py:1457-1470): theta-theta of the E field with only
    its theta_2 = 0 row filled with conj(V) sqrt(w), non-Hermitian back-map, shifted inverse FFT cropped to the
    chunk.  Returns a device tensor [nf, nt] complex128.  `row_t` / `th_t`: that row and the centres of the reduced edges
    already on the device (:func:`chunk_retrieval_batch` uploads them for all its chunks at once: an upload from pageable
    memory per chunk blocks the host until the stream has drained)."""
    n = int(keep.shape[0])
    dev = require_gpu()
    E_t = torch.zeros((n, n), dtype=torch.complex128, device=dev)                # allocation + memset
    if row_t is None:
        row = np.conjugate(np.asarray(V)[:n]) * np.sqrt(w)                        # n numbers: host
        row_t = torch.from_numpy(row)
    E_t[n // 2].copy_(row_t)                                                      # memcpy
    if th_t is None:
        th_t = _dv.to_device(_theta_centres(grid.edges_red(keep)), torch.float64)
    recov_E = _rev_map_dev(grid.geom, th_t, n, e, False, thth_t=E_t)
    nf, nt = shape
    return _ifft2_shifted_dev(recov_E, scale=nf * nt / 4, crop=(nf, nt))


def chunk_retrieval_batch(chunks, npad, tauMask, verbose=False, group_bytes=None, dev_chunks=None, dev_pads=None, out_device=False):
    """Phase retrieval of MANY chunks of one shape (Dynspec.thetatheta_chunks, dynspec.py:1765-1826): the chunks'
    conjugate spectra in one device stack, all their dominant eigenpairs in ONE batched sweep
    (:func:`eigvec_sweep_multi`), then per chunk the back-map and the inverse FFT queued without a host
    synchronisation in between; one copy back per group.

    The chunks are processed in GROUPS whose stacked conjugate spectra stay below ``group_bytes`` (default
    ``RETRIEVAL_GROUP_BYTES`` = 8 GiB, the rule ``Dynspec._fit_chunks`` uses for the fit): an observation with many
    large chunks needs nchunk x (npad+1)^2 x nf x nt x 16 B for one stack of all of them, which the chunk-by-chunk
    reference path never did.  Tutorial-sized data is one group, as before.

    chunks: list of (dspec2[nf, nt], edges, time, freq, eta).  Returns complex [nchunk, nf, nt].  A chunk whose
    preparation, eigen-solve or back-map fails is zero and the error is printed -- what the reference's
    single_chunk_retrieval does (ththmod.py:1471-1475) -- and the other chunks are unaffected.

    ``dev_chunks`` / ``dev_pads`` (round 6): the chunks' pixels already in HBM ([nchunk, nf, nt] float64, cut there by
    :func:`chunk_cut_device`; the list's dspec2 entries are then ignored) and their padding values (host array);
    ``out_device``: return the device tensor instead of copying a gigabyte of chunks to the host (the mosaic reads them there)."""
    nf, nt = (int(v) for v in dev_chunks.shape[1:]) if dev_chunks is not None else np.asarray(chunks[0][0]).shape
    R, C = (npad + 1) * nf, (npad + 1) * nt
    per_group = _group_size(16 * R * C, group_bytes)
    dev = require_gpu()
    out = torch.zeros((len(chunks), nf, nt), dtype=torch.complex128, device=dev) if out_device else np.zeros((len(chunks), nf, nt), dtype=complex)
    for g0 in range(0, len(chunks), per_group):
        group = chunks[g0:g0 + per_group]
        stack = torch.empty((len(group), R, C), dtype=torch.complex128, device=dev)
        # Round 5: nothing is uploaded chunk by chunk any more.  An upload from pageable host memory blocks the host until the
        # stream has drained, so the three per chunk (the chunk's pixels, the theta-theta row, the reduced centres) made host and GPU
        # take turns (bench.py --workload wavefield: 1.4 ms per chunk with the mat-vec busy 4 % of the time).  The group's chunks
        # travel in ONE array each way; the padding value of a chunk (its mean, ththmod.py:783) is taken on the host.
        grids, etas, live, pads = [], [], [], []
        d_all = np.empty((len(group), nf, nt)) if dev_chunks is None else None
        grid_cache = {}                  # (round 6) the chunks of one frequency row share one _Grid
        for k, (dspec2, edges, time, freq, eta) in enumerate(group):
            try:
                grid = _chunk_grid(time, freq, edges, npad, grid_cache)
                e = np.array([_eta_float(eta)])
                if (grid.geom.ntau, grid.geom.nfd) != (R, C) or (grids and grid.M != grids[0].M):
                    raise ValueError("axes or edges of this chunk do not match the chunk shape (%d, %d)" % (nf, nt))
                if dev_chunks is None:
                    d_all[len(live)] = np.asarray(dspec2, dtype=float)
                    pads.append(float(np.asarray(dspec2, dtype=float).mean()))     # (the chunk's own memory order, as dspec.mean() of ththmod.py:783)
                else:
                    pads.append(float(dev_pads[g0 + k]))
            except Exception as exc:          # this chunk stays zero; the slot of the stack is reused by the next one
                print("Chunk %d: %s" % (g0 + k, exc), flush=True)
                continue
            grids.append(grid)
            etas.append(e)
            live.append(k)
        if not live:
            continue
        # (round 6) one call for the group's conjugate spectra, one for its back-maps and inverse transforms: a dozen Python-issued
        # launches per chunk were 0.17 s of a 0.31-s calc_wavefield of 961 chunks
        if dev_chunks is None:
            d_t = _dv.to_device(d_all[: len(live)], torch.float64)
        elif live == list(range(len(group))):
            d_t = dev_chunks[g0:g0 + len(group)]
        else:
            d_t = dev_chunks[g0 + torch.as_tensor(np.asarray(live), device=dev)].contiguous()
        lohi = _tau_mask_lohi(grids, tauMask)          # (outside the per-chunk try: a mask that is no block of delays ends the call)
        pads_a = np.ascontiguousarray(pads, dtype=np.float64)
        ws = workspace_for("scint_cs", nf, nt, npad)
        _lib.call("scint_cs_batch", d_t, len(live), nf, nt, npad, pads_a, lohi, 0, stack, ws, ws.numel(), stream_ptr())
        w_list, V_t, keeps, info = eigvec_sweep_multi(stack[: len(live)], grids, etas)
        V = V_t.cpu().numpy()
        M = grids[0].M
        rows_all, th_all = np.zeros((len(live), M), dtype=complex), np.zeros((len(live), M))
        keep_n = np.zeros(len(live), dtype=np.int32)
        th_cache = {}                    # reduced centres per (grid, crop): shared by the chunks of a frequency row
        for j, k in enumerate(live):
            n = int(keeps[j].shape[0])
            if info["status"][j] != 0 or n < 2:
                print("Chunk %d: eigen-decomposition failed" % (g0 + k), flush=True)
                continue
            try:
                rows_all[j, :n] = np.conjugate(V[j][:n]) * np.sqrt(float(w_list[j][0]))      # ththmod.py:1459-1461
                th_all[j, :n] = _reduced_centres_cached(grids[j], keeps[j], th_cache)
                keep_n[j] = n
            except Exception as exc:
                print("Chunk %d: %s" % (g0 + k, exc), flush=True)
        out_t = _retrieval_tail_dev(rows_all, th_all, keep_n, None, grids, [float(e_[0]) for e_ in etas], nf, nt)
        if verbose:
            for j, k in enumerate(live):
                if keep_n[j] >= 2:
                    print("Chunk %d success" % (g0 + k), flush=True)
        if out_device:
            out[g0 + torch.as_tensor(np.asarray(live), device=dev)] = out_t
        else:
            out[g0 + np.asarray(live)] = out_t.cpu().numpy()
        # release this group's device buffers BEFORE the next group allocates its own: while the names are bound the caching
        # allocator cannot reuse the blocks and the peak would be two groups -- the bound is `group_bytes`, not twice it
        del stack, V_t, out_t, d_t, ws
    return out


def _retrieval_tail_dev(rows, th_red, keep_n, class_id, grids, etas, nf, nt, out_t=None):
    """The tail of :func:`chunk_retrieval_batch` (scint_retrieval_tail): per chunk k with keep_n[k] >= 2, the theta-theta matrix
    of the E field that is zero but for row N/2 = rows[k, :N], its non-Hermitian back-map on the reduced centres th_red[k, :N]
    (ththmod.py:1457-1464) and nf nt / 4 * ifft2(ifftshift(.))[:nf, :nt].  rows: host complex [n, M]; th_red: host float [n, M];
    keep_n: int [n]; grids / etas: the chunk's _Grid and curvature.  class_id: int [n], consecutive chunks with equal ids share
    the pair counts of their back-maps (the caller's promise); None = the classes of equal (curvature, centres, axes).
    ``out_t``: device [n, nf, nt] complex128 the result is written into (chunks with keep_n < 2 keep what it holds); default
    zeros.  Returns the device tensor."""
    n, M = (int(v) for v in np.shape(rows))
    keep_n = np.ascontiguousarray(keep_n, dtype=np.int32)
    etas_a = np.ascontiguousarray(etas, dtype=np.float64)
    th_red = np.asarray(th_red, dtype=float)
    if class_id is None:
        # classes: consecutive chunks with the same reduced centres, curvature and axes (the chunks of one frequency row) share the
        # pair counts of their back-maps
        class_id, prev, cid = np.zeros(n, dtype=np.int32), None, -1
        for j in range(n):
            key = (float(etas_a[j]), int(keep_n[j]), th_red[j, :keep_n[j]].tobytes(), bytes(grids[j].geom))
            if key != prev:
                cid, prev = cid + 1, key
            class_id[j] = cid
    class_id = np.ascontiguousarray(class_id, dtype=np.int32)
    rows_t, th_t = _dv.to_device(np.asarray(rows, dtype=complex), torch.complex128), _dv.to_device(th_red, torch.float64)
    if out_t is None:
        out_t = torch.zeros((n, nf, nt), dtype=torch.complex128, device=require_gpu())
    geoms = (_lib.CsGeom * n)(*[g_.geom for g_ in grids])
    ws = workspace_for("scint_retrieval_tail", M, grids[0].geom.ntau, grids[0].geom.nfd)
    _lib.call("scint_retrieval_tail", rows_t, th_t, keep_n, class_id, geoms, etas_a, n, M, nf, nt, nf * nt / 4, out_t,
              ws, ws.numel(), stream_ptr())
    return out_t


def single_chunk_retrieval(params):
    """Phase retrieval on one time/frequency chunk (ththmod.py:1390-1476).

    params = (dspec2, edges, time, freq, eta, idx_t, idx_f, npad, tauMask, verbose) as in the
    reference.  Returns (model_E[nf, nt] complex, idx_f, idx_t); on failure a zero array, as
    the reference does.  The wavefield carries the arbitrary global phase of the eigenvector."""
    dspec2, edges, time, freq, eta, idx_t, idx_f, npad, tauMask, verbose = params
    _, _, edges_v, tau, fd = _chunk_axes(time, freq, edges, npad)      # (unit and axis errors propagate: outside the try)
    e = _eta_float(eta)
    dspec2 = np.asarray(dspec2, dtype=float)
    try:
        cs_t = conjugate_spectrum(dspec2, npad, tau, tauMask, True)
        grid = _Grid(tau, fd, edges_v)
        # of modeler's outputs (ththmod.py:1455) only the eigenpair is used here: no rank-1 back-map, no model
        keep = grid.keep(e)
        w, V_t, _ = _eigh_top_dev(_thth_dev(cs_t, grid, e, keep, True), None, want_vec=True)
        model_E = _wavefield_from_eigpair(grid, e, keep, V_t.cpu().numpy(), w, dspec2.shape).cpu().numpy()
        if verbose:
            print("Chunk %s-%s success" % (idx_f, idx_t), flush=True)
    except Exception as exc:   # the reference keeps going with a zero chunk
        print(exc, flush=True)
        model_E = np.zeros(dspec2.shape, dtype=complex)
    return (model_E, idx_f, idx_t)


# ----------------------------------------------------------------------------
# multi-station (VLBI) phase retrieval (ththmod.py:1223-1387)
# ----------------------------------------------------------------------------
def _vlbi_spectrum_index(n_dish, d1, d2):
    """Position of station pair (d1, d1 + d2) in [I1, V12, ..., V1N, I2, V23, ..., IN] (ththmod.py:1345-1349)."""
    return (n_dish * (n_dish + 1)) // 2 - ((n_dish - d1) * (n_dish - d1 + 1)) // 2 + d2


def _vlbi_gather_raises(grid, eta):
    """True where NumPy's fancy index of thth_map (ththmod.py:104) raises IndexError: a kept point (0 < tau_inv < ntau) whose
    Doppler index lies below -len(fd).  Only edges wider than 1.5 times the Doppler span can reach such an index; the M x M
    index maps are formed (on the host, the reference's expressions) only then."""
    g, th = grid.geom, grid.th_cents
    if not np.floor(((th.min() - th.max()) - g.fd0 + g.dfd / 2) / g.dfd) < -g.nfd:
        return False
    th1 = np.ones((th.shape[0], th.shape[0])) * th
    th2 = th1.T
    tau_inv = (((eta * (th1**2 - th2**2)) - g.tau0 + g.dtau / 2) // g.dtau).astype(int)
    fd_inv = (((th1 - th2) - g.fd0 + g.dfd / 2) // g.dfd).astype(int)
    return bool(((tau_inv > 0) * (tau_inv < g.ntau) * (fd_inv < -g.nfd)).any())


def _vlbi_composites_dev(stack_t, slots, grids, etas, keeps, n_dish, S=None):
    """The composite theta-theta of every chunk of a group (scint_vlbi_composite).  stack_t: device [nslot, ntau, nfd] conjugate
    spectra; slots: int [n, nspec], the slot of spectrum idx of chunk k (the reference's list order); grids / etas / keeps: per
    chunk its _Grid, curvature and the kept indices of thth_redmap's crop.  Returns the device tensor [n, S * S]: chunk k's dense
    [n_dish N_k, n_dish N_k] composite sits at the start of row k (S = n_dish max N_k unless given larger)."""
    n, M = len(grids), grids[0].M
    nspec = n_dish * (n_dish + 1) // 2
    slots = np.ascontiguousarray(slots, dtype=np.int64).reshape(n, nspec)
    if slots.min() < 0 or slots.max() >= stack_t.shape[0]:
        raise ValueError("spectrum slot outside the stack")
    etas = np.ascontiguousarray(etas, dtype=np.float64)
    keep_n = np.ascontiguousarray([k_.shape[0] for k_ in keeps], dtype=np.int32)
    if S is None:
        S = n_dish * int(keep_n.max())
    R, C = (int(v) for v in stack_t.shape[1:])
    th_all, keep_all = np.zeros((n, M)), np.zeros((n, M), dtype=np.int32)
    for j in range(n):
        if grids[j].M != M or (grids[j].geom.ntau, grids[j].geom.nfd) != (R, C) or (keep_n[j] and int(keeps[j].max()) >= M):
            raise ValueError("chunk %d: grid does not match the batch" % j)
        th_all[j] = grids[j].th_cents
        keep_all[j, :keep_n[j]] = keeps[j]
    th_t, keep_t = _dv.to_device(th_all, torch.float64), _dv.to_device(keep_all, torch.int32)
    comp = torch.empty((n, S * S), dtype=torch.complex128, device=stack_t.device)
    geoms = (_lib.CsGeom * n)(*[g_.geom for g_ in grids])
    ws = workspace_for("scint_vlbi_composite", n, n_dish)
    _lib.call("scint_vlbi_composite", stack_t, R * C, slots, geoms, th_t, M, keep_t, keep_n, etas, n, n_dish, comp, S * S,
              ws, ws.numel(), stream_ptr())
    return comp


def vlbi_retrieval_batch(chunks, npad, n_dish, tauMask, verbose=False, group_bytes=None, out_device=False,
                         tol=DEFAULT_TOL, max_iter=DEFAULT_MAX_ITER, info=None):
    """Multi-station phase retrieval of MANY chunks of one shape: VLBI_chunk_retrieval (ththmod.py:1223-1387) for all of them
    with everything between the input pixels and the wavefields on the device.

    chunks: list of (dspec2_list, edges, time, freq, eta); dspec2_list holds the n_dish (n_dish + 1) / 2 spectra of the chunk,
    each [nf, nt], in the reference's order [I1, V12, ..., V1N, I2, V23, ..., IN] (dynamic spectra real, visibilities complex).
    Returns complex [nchunk, n_dish, nf, nt] (a device tensor with ``out_device``): the wavefield of every station.

    Per group of chunks: the dynamic spectra's conjugate spectra (mean-padded, scint_cs_batch) and the visibilities'
    (zero-padded complex, scint_cs_complex_batch) in one device stack; every chunk's composite theta-theta -- block
    (d1 + d2, d1) the reduced theta-theta of pair (d1, d1 + d2), block (d1, d1 + d2) its conjugate transpose, Hermitian forcing
    on the dynamic spectra only -- written by ONE gather (scint_vlbi_composite) as dense matrices; their dominant eigenpairs by
    the batched Lanczos of scint_eigh_top_batch; then per chunk and station the row conj(V[d N:(d + 1) N]) sqrt(w) through
    scint_retrieval_tail (the stations of a chunk share the back-map's pair counts).  Groups are sized like
    :func:`chunk_retrieval_batch`'s: the device bytes of a chunk (its spectra, its composite and the Lanczos vectors) against
    ``group_bytes`` (default ``RETRIEVAL_GROUP_BYTES``).

    Like the reference function, and unlike single_chunk_retrieval, nothing is caught: a chunk whose crop keeps fewer than two
    centres raises IndexError (the reference's thth_redmap indexes an empty edges_red, ththmod.py:163), an eigen-solve that
    fails raises ArithmeticError, and either ends the whole call.

    Phases: the eigenvector has ONE arbitrary global phase per chunk, common to its stations; the phases BETWEEN stations are
    determined, and they come out consistent with the visibilities under the convention V_ab = E_a conj(E_b).

    ``info`` (a dict, tests and tools): receives ``composites`` (per chunk the host copy of its [n_dish N, n_dish N] composite),
    ``w`` and ``iters`` (eigenvalue and Lanczos steps per chunk), ``groups`` (the number of groups the chunks went in)."""
    n_dish = int(n_dish)
    if n_dish < 1:
        raise ValueError("n_dish must be at least 1")
    nspec = n_dish * (n_dish + 1) // 2
    nvis = nspec - n_dish
    dyn_idx = [_vlbi_spectrum_index(n_dish, d, 0) for d in range(n_dish)]
    vis_idx = [i for i in range(nspec) if i not in dyn_idx]
    if len(chunks) == 0:
        return np.zeros((0, n_dish, 0, 0), dtype=complex)
    for k, c in enumerate(chunks):
        if len(c[0]) != nspec:
            raise ValueError("chunk %d: %d spectra for n_dish = %d (%d expected)" % (k, len(c[0]), n_dish, nspec))
    nf, nt = np.asarray(chunks[0][0][0]).shape
    R, C = (npad + 1) * nf, (npad + 1) * nt
    _check_sweep_cs(R, C)
    dev = require_gpu()
    mask_us = float(units.strip(tauMask, "tauMask", "us", warn=False))
    out = torch.zeros((len(chunks), n_dish, nf, nt), dtype=torch.complex128, device=dev) if out_device else \
        np.zeros((len(chunks), n_dish, nf, nt), dtype=complex)

    # host preparation of every chunk (grids are shared between chunks with equal axes and edges, as in chunk_retrieval_batch)
    grid_cache, prep = {}, []
    for k, (dlist, edges, time, freq, eta) in enumerate(chunks):
        grid = _chunk_grid(time, freq, edges, npad, grid_cache)
        if (grid.geom.ntau, grid.geom.nfd) != (R, C) or (prep and grid.M != prep[0][0].M):
            raise ValueError("chunk %d: axes or edges do not match the chunk shape (%d, %d)" % (k, nf, nt))
        for x in dlist:
            if np.shape(x) != (nf, nt):
                raise ValueError("chunk %d: a spectrum of shape %s in a batch of (%d, %d)" % (k, np.shape(x), nf, nt))
        e = _eta_float(eta)
        keep = grid.keep(e)
        if keep.shape[0] < 2:
            raise IndexError("chunk %d: the crop of thth_redmap keeps %d theta centres (index 0 is out of bounds for edges_red, "
                             "ththmod.py:163)" % (k, keep.shape[0]))
        if _vlbi_gather_raises(grid, e):
            raise IndexError("chunk %d: theta-theta gather index out of bounds for the conjugate spectrum" % k)
        prep.append((grid, e, keep))
    M = prep[0][0].M
    nmax = max(p_[2].shape[0] for p_ in prep)
    S = n_dish * nmax
    per_chunk = 16 * (nspec * R * C + S * S + (min(max_iter, S) + 4) * S) + 16 * nspec * nf * nt
    per_group = _group_size(per_chunk, group_bytes, cap=65535)

    for g0 in range(0, len(chunks), per_group):
        group = chunks[g0:g0 + per_group]
        n = len(group)
        grids = [prep[g0 + j][0] for j in range(n)]
        etas = np.ascontiguousarray([prep[g0 + j][1] for j in range(n)], dtype=np.float64)
        keep_n = np.ascontiguousarray([prep[g0 + j][2].shape[0] for j in range(n)], dtype=np.int32)
        # one upload each way: dynamic spectra [n * n_dish], visibilities [n * nvis]; padding value = the spectrum's own mean
        d_all = np.empty((n * n_dish, nf, nt))
        v_all = np.empty((n * nvis, nf, nt), dtype=complex)
        pads = np.empty(n * n_dish)
        for j, c in enumerate(group):
            for q, i in enumerate(dyn_idx):
                a = np.asarray(c[0][i])
                a = np.asarray(a.real if np.iscomplexobj(a) else a, dtype=float)
                d_all[j * n_dish + q] = a
                pads[j * n_dish + q] = float(a.mean())                            # ththmod.py:1303
            for q, i in enumerate(vis_idx):
                v_all[j * nvis + q] = np.asarray(c[0][i])
        lohi = _tau_mask_lohi(grids, mask_us)                                     # ththmod.py:1308 / 1325
        stack = torch.empty((n * nspec, R, C), dtype=torch.complex128, device=dev)   # slots: the dynamic spectra, then the visibilities
        ws = workspace_for("scint_cs", nf, nt, npad)
        d_t = _dv.to_device(d_all, torch.float64)
        lohi_d = np.ascontiguousarray(np.repeat(lohi, n_dish, axis=0))
        _lib.call("scint_cs_batch", d_t, n * n_dish, nf, nt, npad, pads, lohi_d, 0, stack, ws, ws.numel(), stream_ptr())
        v_t = None
        if nvis:
            v_t = _dv.to_device(v_all, torch.complex128)
            lohi_v = np.ascontiguousarray(np.repeat(lohi, nvis, axis=0))
            _lib.call("scint_cs_complex_batch", v_t, n * nvis, nf, nt, npad, lohi_v, stack[n * n_dish:], ws, ws.numel(), stream_ptr())
        slots = np.empty((n, nspec), dtype=np.int64)
        for q, i in enumerate(dyn_idx):
            slots[:, i] = np.arange(n) * n_dish + q
        for q, i in enumerate(vis_idx):
            slots[:, i] = n * n_dish + np.arange(n) * nvis + q
        comp = _vlbi_composites_dev(stack, slots, grids, etas, [prep[g0 + j][2] for j in range(n)], n_dish, S)
        # dominant ('LA') eigenpair of every composite, started from the zero-theta row of the first station's block row
        sizes = np.ascontiguousarray(n_dish * keep_n, dtype=np.int32)
        start = np.ascontiguousarray(keep_n // 2, dtype=np.int32)
        ws = workspace_for("scint_eigh_top_batch", S, max_iter, n)
        w_t = empty((n,), torch.float64)
        V_t = torch.zeros((n, S), dtype=torch.complex128, device=dev)
        st_t = torch.zeros((2, n), dtype=torch.int32, device=dev)
        _lib.call("scint_eigh_top_batch", comp, S * S, sizes, start, n, tol, max_iter, w_t, V_t, S, st_t[0], st_t[1],
                  ws, ws.numel(), stream_ptr())
        st = st_t.cpu().numpy()
        if (st[0] != 0).any():
            j = int(np.nonzero(st[0])[0][0])
            raise ArithmeticError("chunk %d: top-eigenpair iteration of the composite failed (status %d, %d steps)"
                                  % (g0 + j, st[0][j], st[1][j]))
        w, V = w_t.cpu().numpy(), V_t.cpu().numpy()
        if info is not None:
            comp_h = comp.cpu().numpy()
            info.setdefault("composites", []).extend(comp_h[j, :int(sizes[j]) ** 2].reshape(int(sizes[j]), int(sizes[j])).copy() for j in range(n))
            info.setdefault("w", []).extend(float(x) for x in w)
            info.setdefault("iters", []).extend(int(x) for x in st[1])
            info["groups"] = info.get("groups", 0) + 1
        rows_all, th_rows = np.zeros((n * n_dish, M), dtype=complex), np.zeros((n * n_dish, M))
        th_cache = {}
        for j in range(n):
            N = int(keep_n[j])
            th_red = _reduced_centres_cached(grids[j], prep[g0 + j][2], th_cache)
            with np.errstate(invalid="ignore"):
                amp = np.sqrt(w[j])                                                # ththmod.py:1376
            for d in range(n_dish):
                rows_all[j * n_dish + d, :N] = np.conjugate(V[j, d * N:(d + 1) * N]) * amp
                th_rows[j * n_dish + d, :N] = th_red
        out_t = _retrieval_tail_dev(rows_all, th_rows, np.repeat(keep_n, n_dish), None, [g_ for g_ in grids for _ in range(n_dish)],
                                    np.repeat(etas, n_dish), nf, nt)
        if verbose:
            for j in range(n):
                print("Chunk %d success" % (g0 + j), flush=True)
        if out_device:
            out[g0:g0 + n] = out_t.view(n, n_dish, nf, nt)
        else:
            out[g0:g0 + n] = out_t.cpu().numpy().reshape(n, n_dish, nf, nt)
        del stack, comp, V_t, out_t, d_t, v_t, ws
    return out


def VLBI_chunk_retrieval(params):
    """Phase retrieval on one time/frequency chunk from the dynamic spectra and visibilities of several stations
    (ththmod.py:1223-1387): the one-chunk case of :func:`vlbi_retrieval_batch`.

    params = (dspec2_list, edges, time, freq, eta, idx_t, idx_f, npad, n_dish, tauMask, verbose) as in the reference;
    dspec2_list is ordered [I1, V12, ..., V1N, I2, V23, ..., IN].  time, freq, eta, edges and tauMask may be plain numbers
    (s, MHz, s**3, mHz, us) or Quantities.  Returns (model_E, idx_f, idx_t) with model_E a list of n_dish complex [nf, nt]
    arrays.  As in the reference there is no try/except: errors propagate.

    The wavefields share ONE arbitrary global phase (the eigenvector's); the phases between stations are determined.  They are
    consistent with the inputs when the visibilities follow V_ab = E_a conj(E_b) (and I_a = |E_a|**2): station b's wavefield then
    carries its phase offset against station a with the sign the data has."""
    dspec2_list, edges, time, freq, eta, idx_t, idx_f, npad, n_dish, tauMask, verbose = params
    if verbose:
        print("Starting Chunk %s-%s" % (idx_f, idx_t), flush=True)
    E = vlbi_retrieval_batch([(dspec2_list, edges, time, freq, eta)], int(npad), int(n_dish), tauMask)
    if verbose:
        print("Chunk %s-%s success" % (idx_f, idx_t), flush=True)
    return ([E[0, d] for d in range(int(n_dish))], idx_f, idx_t)


def mask_func(w):
    """Mask for combining chunks (ththmod.py:1479-1489)."""
    x = np.linspace(0, w - 1, w)
    return np.sin((np.pi / 2) * x / w) ** 2


def mosaic(chunks):
    """Stack half-overlapping wavefield chunks after removing their relative phase
    (ththmod.py:1492-1554).  Host NumPy: one pass over the output, sequentially dependent."""
    nct, ncf, cwf, cwt = chunks.shape[1], chunks.shape[0], chunks.shape[2], chunks.shape[3]
    E_recov = np.zeros(((ncf - 1) * (cwf // 2) + cwf, (nct - 1) * (cwt // 2) + cwt), dtype=complex)
    masks = {}          # the weight of a chunk depends only on which of its four sides have a neighbour: nine arrays, not one per chunk

    def mask_of(cf, ct):
        key = (cf > 0, cf < ncf - 1, ct > 0, ct < nct - 1)
        if key not in masks:
            mask = np.ones((cwf, cwt))
            if key[0]:
                mask[: cwf // 2, :] *= mask_func(cwf // 2)[:, np.newaxis]
            if key[1]:
                mask[cwf // 2:, :] *= 1 - mask_func(cwf // 2)[:, np.newaxis]
            if key[2]:
                mask[:, : cwt // 2] *= mask_func(cwt // 2)
            if key[3]:
                mask[:, cwt // 2:] *= 1 - mask_func(cwt // 2)
            masks[key] = mask
        return masks[key]
    for cf in range(ncf):
        for ct in range(nct):
            chunk_new = chunks[cf, ct, :, :]
            sl = (slice(cf * cwf // 2, cf * cwf // 2 + cwf), slice(ct * cwt // 2, ct * cwt // 2 + cwt))
            chunk_old = E_recov[sl]
            mask = mask_of(cf, ct)
            rot = np.angle((chunk_old * np.conjugate(chunk_new) * mask).mean())
            E_recov[sl] += chunk_new * mask * np.exp(1j * rot)
    return E_recov


_NUMPY_MODES = {}


def _numpy_mosaic_modes(cwf, cwt):
    """How THIS host's NumPy evaluates ``chunk_old * np.conjugate(chunk_new) * mask`` (ththmod.py:1550) for chunks of this
    shape -- two properties of the host, measured on random data with the very expression, so that the device mosaic can equal
    the host loop of :func:`mosaic` bit for bit (csrc/mosaic.hip: cmul_np):

    * fused: NumPy's x86 SIMD loops (AVX2 / AVX-512 with FMA3) multiply complex128 arrays as re = fma(ar, br, -(ai bi)),
      im = fma(ar, bi, ai br) -- one rounding fewer than the plain expressions of its scalar loop;
    * swapped: for temporaries of 256 KiB and more NumPy reuses ``conj(chunk_new)`` as the output of the product and, the
      operation being commutative, computes ``conj(chunk_new) * chunk_old`` -- the fused form is not symmetric in its operands.

    Returns (fused, swapped), or None if neither reading reproduces the expression (an unknown NumPy: the caller then warns
    and the device result agrees with the host loop to rounding only)."""
    key = (cwf, cwt)
    if key not in _NUMPY_MODES:
        rng = np.random.default_rng(12345)
        big = rng.standard_normal((cwf + 2, cwt + 2)) + 1j * rng.standard_normal((cwf + 2, cwt + 2))
        a = big[1:1 + cwf, 1:1 + cwt]                                 # a window of a larger array, as E_recov[sl] is
        b = rng.standard_normal((cwf, cwt)) + 1j * rng.standard_normal((cwf, cwt))
        m = rng.random((cwf, cwt))
        expr = a * np.conjugate(b) * m
        cb = np.conjugate(b)

        def plain(x, y):
            return (x.real * y.real - x.imag * y.imag) + 1j * (x.real * y.imag + x.imag * y.real)
        fused = not np.array_equal(np.multiply(a, cb), plain(a, cb))
        if np.array_equal(expr, np.multiply(np.multiply(a, cb), m)):
            _NUMPY_MODES[key] = (fused, False)
        elif np.array_equal(expr, np.multiply(np.multiply(cb, a), m)):
            _NUMPY_MODES[key] = (fused, True)
        else:
            _NUMPY_MODES[key] = None
    return _NUMPY_MODES[key]


def _mosaic_tapers(ncf, nct, cwf, cwt):
    """The taper of chunk (cf, ct) as mask[r, c] = fr[r] * fc[c] (ththmod.py:1526-1546 builds it by multiplying a matrix of ones
    by a row factor, then by a column factor: one product per element, the same bits).  Returns (rows[4, cwf], cols[4, cwt]) and
    the index function: variant 2 * (has a neighbour before) + (has a neighbour after).  An axis of ONE chunk uses variant 0 only
    (no taper): its size may be odd, and the other variants stay ones."""
    def variants(w, nchunk):
        v = np.ones((4, w))
        if nchunk == 1:
            return v
        if w % 2:
            raise ValueError("mosaic: chunk sizes must be even along an axis of several chunks (the reference's half-overlap tapers)")
        mf = mask_func(w // 2)
        for k in range(4):
            if k & 2:
                v[k, : w // 2] *= mf
            if k & 1:
                v[k, w // 2:] *= 1 - mf
        return v
    return variants(cwf, ncf), variants(cwt, nct)


def mosaic_device(chunks_t, angles=None):
    """:func:`mosaic` with the chunks and the wavefield in HBM (device tensor [ncf, nct, cwf, cwt] complex128 -> device tensor
    [F, T]).  The reference's loop (ththmod.py:1548-1553) is sequential, but chunk (cf, ct) only meets its four predecessors
    (cf, ct-1) and (cf-1, ct-1 .. ct+1): chunks with equal 2 cf + ct are independent, their windows disjoint, and every
    overlapping pair keeps its order -- so the mosaic walks 2 (ncf - 1) + nct STEPS (91 for the 961 chunks of a 4096^2
    observation).  Per step one kernel forms ``(chunk_old * conj(chunk_new) * mask)`` and its sum in NumPy's own summation order
    for every chunk of the step, the sums (16 bytes each) come to the host where ``mean``, ``numpy.angle`` and ``numpy.exp``
    are NumPy's, and a second kernel adds ``chunk_new * mask * exp(1j * rot)``.  Bit-identical to the host loop on the same
    chunks (tests); the host loop spent 0.26 s on those 961 chunks and needed them on the host (1 GB).
    ``angles``: a float array [ncf * nct] that receives every chunk's rotation (the reference's ``rotInit`` is this very loop)."""
    ncf, nct, cwf, cwt = (int(v) for v in chunks_t.shape)
    rows, cols = _mosaic_tapers(ncf, nct, cwf, cwt)             # (raises for an odd size along an axis of several chunks)
    F, T = (ncf - 1) * (cwf // 2) + cwf, (nct - 1) * (cwt // 2) + cwt
    rows_t, cols_t = _dv.to_device(rows, torch.float64), _dv.to_device(cols, torch.float64)
    E_t = torch.zeros((F, T), dtype=torch.complex128, device=chunks_t.device)
    modes = _numpy_mosaic_modes(cwf, cwt)
    if modes is None:
        warnings.warn("scintools_amd: this NumPy evaluates the mosaic's products in an unknown way; the device mosaic agrees with "
                      "the reference's host loop to rounding, not bit for bit")
        modes = (False, False)
    fused = (1 if modes[0] else 0) | (2 if modes[1] else 0)
    # the jobs in step order, at most 64 per launch
    steps = {}
    for cf in range(ncf):
        for ct in range(nct):
            steps.setdefault(2 * cf + ct, []).append((cf, ct))
    launches, table = [], []
    for t in sorted(steps):
        for k0 in range(0, len(steps[t]), 64):
            part = steps[t][k0:k0 + 64]
            launches.append((len(table), len(part)))
            for cf, ct in part:
                table.append(((cf * (cwf // 2)) * T + ct * (cwt // 2), cf * nct + ct, 2 * (cf > 0) + (cf < ncf - 1), 2 * (ct > 0) + (ct < nct - 1)))
    jobs_t = _dv.to_device(np.asarray(table, dtype=np.int64), torch.int64)
    most = max(n for _, n in launches)
    ws = workspace_for("scint_mosaic", cwf, cwt, most)
    sums_t = empty((most, 2), torch.float64)
    count = cwf * cwt
    st = stream_ptr()
    chunks_c = chunks_t.contiguous()
    ph = np.empty((most, 2))
    for first, n in launches:
        jobs = jobs_t[first:first + n]
        _lib.call("scint_mosaic_phase", E_t, T, chunks_c, cwf, cwt, jobs, n, rows_t, cols_t, fused, ws, ws.numel(), sums_t, st)
        sums = sums_t[:n].cpu().numpy()
        for k in range(n):
            tot = np.complex128(complex(sums[k, 0], sums[k, 1]))
            mean = tot.dtype.type(tot / count)                       # numpy's _mean: umr_sum(...) / rcount
            rot = np.angle(mean)
            e = np.exp(1j * rot)
            ph[k, 0], ph[k, 1] = e.real, e.imag
            if angles is not None:
                angles[table[first + k][1]] = rot
        _lib.call("scint_mosaic_add", E_t, T, chunks_c, cwf, cwt, jobs, n, rows_t, cols_t, fused, ph, st)
    return E_t


# ----------------------------------------------------------------------------
# the fitted mosaics (ththmod.py:1708-2310): every chunk's phase -- and amplitude -- a free parameter
# ----------------------------------------------------------------------------
class MosaicStack:
    """The chunk stack of a mosaic, its tapers and (optionally) the dynamic spectrum and its noise map, in HBM: what an
    optimiser of ``rotFit`` / ``fullMosFit`` evaluates tens to hundreds of times.  ``chunks``: NumPy array, stripped Quantity or
    device tensor [ncf, nct, cwf, cwt]; sizes are even along an axis of several chunks (``ValueError`` otherwise, as
    :func:`mosaic_device`).  One evaluation is three launches (csrc/mosaic.hip): the mosaic as a gather, the per-chunk window
    sums, their fixed-order totals -- the same inputs give the same bits.

    ``dspec`` / ``N`` keep the reference's shape rules: the objective crops them to the mosaic (``dspec[:F, :T]``), gradient and
    Hessian need exactly the mosaic's shape and raise ``ValueError`` otherwise, as the NumPy broadcast there does."""

    def __init__(self, chunks, dspec=None, N=None):
        if isinstance(chunks, torch.Tensor):
            chunks_t = chunks.to(torch.complex128)
        else:
            chunks_t = _dv.to_device(np.ascontiguousarray(np.asarray(getattr(chunks, "value", chunks), dtype=complex)), torch.complex128)
        if chunks_t.dim() != 4:
            raise ValueError("MosaicStack: chunks are [ncf, nct, cwf, cwt]")
        self.chunks_t = chunks_t.contiguous()
        self.ncf, self.nct, self.cwf, self.cwt = (int(v) for v in chunks_t.shape)
        rows, cols = _mosaic_tapers(self.ncf, self.nct, self.cwf, self.cwt)      # (raises for an odd size on a tapered axis)
        self.n = self.ncf * self.nct
        self.shape = ((self.ncf - 1) * (self.cwf // 2) + self.cwf, (self.nct - 1) * (self.cwt // 2) + self.cwt)
        self._rows_t, self._cols_t = _dv.to_device(rows, torch.float64), _dv.to_device(cols, torch.float64)
        modes = _numpy_mosaic_modes(self.cwf, self.cwt)
        if modes is None:
            warnings.warn("scintools_amd: this NumPy evaluates the mosaic's products in an unknown way; the device mosaic agrees with "
                          "the reference's host loop to rounding, not bit for bit")
            modes = (False, False)
        self._fused = 1 if modes[0] else 0
        need = ctypes.c_size_t()
        _lib.call("scint_mosaic_fit_workspace_bytes", self.ncf, self.nct, self.cwf, self.cwt, need)
        self._ws_bytes = need.value
        self._W_t = None
        self._maps = [self._map(dspec), self._map(N)]

    def with_maps(self, dspec, N):
        """A stack on the SAME chunks and tapers in HBM with another dynamic spectrum and noise map (and a mosaic buffer of its own)."""
        return MosaicStack(self.chunks_t, dspec, N)

    def _map(self, arr):
        """(device crop to the mosaic or None, is exactly the mosaic's shape, host shape)"""
        if arr is None:
            return None
        if isinstance(arr, torch.Tensor):
            shape = tuple(int(v) for v in arr.shape)
            crop = arr
        else:
            crop = np.asarray(getattr(arr, "value", arr), dtype=float)
            shape = crop.shape
        F, T = self.shape
        if len(shape) != 2 or shape[0] < F or shape[1] < T:
            return (None, False, shape)
        crop = crop[:F, :T]
        crop_t = crop.to(torch.float64).contiguous() if isinstance(crop, torch.Tensor) else _dv.to_device(np.ascontiguousarray(crop), torch.float64)
        return (crop_t, shape == (F, T), shape)

    def _fit_maps(self, exact):
        out = []
        for m, name in zip(self._maps, ("dspec", "N")):
            if m is None:
                raise ValueError(f"MosaicStack: the chi^2 fit needs {name}")
            if m[0] is None or (exact and not m[1]):
                raise ValueError(f"operands could not be broadcast together with shapes {self.shape} {m[2]} ({name})")
            out.append(m[0])
        return out

    # -- parameters -> per-chunk coefficients (amplitude, exp(1j * phase) in NumPy) -------------------------------------------
    def _coef(self, phases, amps):
        c = np.empty((self.n, 3))
        c[:, 0] = 1.0 if amps is None else amps
        e = np.exp(1j * np.concatenate(([0.0], np.asarray(phases, dtype=float))))       # chunk 0: exp(0j) = 1 + 0j, the same product
        c[:, 1], c[:, 2] = e.real, e.imag
        return _dv.to_device(c, torch.float64)

    def _split(self, p):
        p = np.asarray(p, dtype=float)
        if p.shape != (2 * self.n - 1,):
            raise IndexError(f"fullMos: p holds {self.n - 1} phases and {self.n} amplitudes, got shape {p.shape}")
        return p[:self.n - 1], p[self.n - 1:]

    def _rot_x(self, x):
        x = np.asarray(x, dtype=float)
        if x.shape != (self.n - 1,):
            raise IndexError(f"rotMos: x holds {self.n - 1} phases, got shape {x.shape}")
        return x

    def _eval(self, coef_t, full, want, maps=(None, None), W_t=None):
        if W_t is None:
            if self._W_t is None:
                self._W_t = empty(self.shape, torch.complex128)
            W_t = self._W_t
        out_t = empty((1 + 2 * self.n,), torch.float64) if want else None
        ws = workspace.get(self._ws_bytes) if want else None
        _lib.call("scint_mosaic_fit_eval", self.chunks_t, self.ncf, self.nct, self.cwf, self.cwt, self._rows_t, self._cols_t, coef_t,
                  1 if full else 0, self._fused, maps[0], maps[1], W_t, want, out_t, ws, ws.numel() if want else 0, stream_ptr())
        return W_t, (out_t.cpu().numpy() if want else None)

    def _mosaic(self, coef_t, full, out_device):
        W_t, _ = self._eval(coef_t, full, 0, W_t=empty(self.shape, torch.complex128))
        return W_t if out_device else W_t.cpu().numpy()

    # -- the phase fit ------------------------------------------------------------------------------------------------------------
    def rot_init(self):
        """``rotInit``: the greedy mosaic's own angles (the reference's ``rotInit`` and ``mosaic`` are the same loop)."""
        angles = np.zeros(self.n)
        mosaic_device(self.chunks_t, angles=angles)
        return angles[1:]

    def rot_mosaic(self, x, out_device=False):
        """``rotMos(chunks, x)``: bit-identical to the host loop on the same chunks."""
        return self._mosaic(self._coef(self._rot_x(x), None), False, out_device)

    def rot_value_and_grad(self, x):
        """(``rotFit(x, chunks)``, ``rotDer(x, chunks)``) from one evaluation."""
        _, out = self._eval(self._coef(self._rot_x(x), None), False, 2)
        return float(out[0]), out[2:1 + self.n].copy()

    def rot_value(self, x):
        return float(self._eval(self._coef(self._rot_x(x), None), False, 1)[1][0])

    # -- the chi^2 fit ------------------------------------------------------------------------------------------------------------
    def full_mosaic(self, p, out_device=False):
        """``fullMos(chunks, p)``: bit-identical to the host loop on the same chunks."""
        ph, amp = self._split(p)
        return self._mosaic(self._coef(ph, amp), True, out_device)

    def full_value(self, p):
        """``fullMosFit``: dspec and N cropped to the mosaic."""
        ph, amp = self._split(p)
        return float(self._eval(self._coef(ph, amp), True, 1, self._fit_maps(False))[1][0])

    def full_value_and_grad(self, p):
        """(``fullMosFit``, ``fullMosGrad``) from one evaluation; dspec and N of exactly the mosaic's shape."""
        ph, amp = self._split(p)
        _, out = self._eval(self._coef(ph, amp), True, 2, self._fit_maps(True))
        return float(out[0]), np.concatenate((out[2:1 + self.n], out[1 + self.n:]))

    def full_hess(self, p):
        """``fullMosHess``: dense [2 n - 1, 2 n - 1], zero outside the neighbour band, exactly symmetric."""
        ph, amp = self._split(p)
        maps = self._fit_maps(True)
        coef_t = self._coef(ph, amp)
        W_t, _ = self._eval(coef_t, True, 0)
        P = 2 * self.n - 1
        H_t = empty((P, P), torch.float64)
        ws = workspace.get(self._ws_bytes)
        _lib.call("scint_mosaic_fit_hess", self.chunks_t, self.ncf, self.nct, self.cwf, self.cwt, self._rows_t, self._cols_t, coef_t,
                  maps[0], maps[1], W_t, H_t, ws, ws.numel(), stream_ptr())
        return H_t.cpu().numpy()


def _as_stack(chunks, dspec=None, N=None):
    if isinstance(chunks, MosaicStack):
        return chunks if dspec is None and N is None else chunks.with_maps(dspec, N)
    return MosaicStack(chunks, dspec, N)


def rotMos(chunks, x):
    """Mosaic with given chunk phases (ththmod.py:1708-1770).  ``chunks`` may be a :class:`MosaicStack`."""
    return _as_stack(chunks).rot_mosaic(x)


def rotFit(x, chunks):
    """-sum |rotMos(chunks, x)|^2 (ththmod.py:1773-1788)."""
    return np.float64(_as_stack(chunks).rot_value(x))


def rotInit(chunks):
    """The greedy mosaic's phases as a start for :func:`rotFit` (ththmod.py:1791-1856)."""
    return _as_stack(chunks).rot_init()


def rotDer(x, chunks):
    """Analytic gradient of :func:`rotFit` (ththmod.py:1859-1919)."""
    return _as_stack(chunks).rot_value_and_grad(x)[1]


def fullMos(chunks, p):
    """Mosaic with given chunk phases and amplitudes (ththmod.py:1922-1987)."""
    return _as_stack(chunks).full_mosaic(p)


def fullMosFit(p, chunks, dspec, N):
    """chi^2 of |fullMos|^2 against the dynamic spectrum (ththmod.py:1990-2016)."""
    return np.float64(_as_stack(chunks, dspec, N).full_value(p))


def fullMosGrad(p, chunks, dspec, N):
    """Analytic gradient of :func:`fullMosFit` (ththmod.py:2019-2102)."""
    return _as_stack(chunks, dspec, N).full_value_and_grad(p)[1]


def fullMosHess(p, chunks, dspec, N):
    """Analytic Hessian of :func:`fullMosFit` (ththmod.py:2105-2310)."""
    return _as_stack(chunks, dspec, N).full_hess(p)


def fit_mosaic(stack, mode="rot", x0=None, method=None, options=None, out_device=False):
    """Fit every chunk's phase (``mode="rot"``: maximise the coherent power, L-BFGS-B) or phase and amplitude (``"full"``:
    minimise chi^2 against the stack's dynamic spectrum, Newton-CG with the analytic Hessian) with ``scipy.optimize.minimize``
    on the device objective and derivatives.  The start is ``rot_init()`` (amplitudes 1).  Returns (wavefield, parameters,
    OptimizeResult); the wavefield stays on the device with ``out_device``."""
    if mode not in ("rot", "full"):
        raise ValueError("fit_mosaic: mode is 'rot' or 'full'")
    if not isinstance(stack, MosaicStack):
        stack = MosaicStack(stack)
    if x0 is None:
        x0 = stack.rot_init()
        if mode == "full":
            x0 = np.concatenate((x0, np.ones(stack.n)))
    x0 = np.asarray(x0, dtype=float)
    if mode == "rot":
        res = minimize(stack.rot_value_and_grad, x0, jac=True, method=method or "L-BFGS-B", options=options)
        return stack.rot_mosaic(res.x, out_device=out_device), res.x, res
    res = minimize(stack.full_value_and_grad, x0, jac=True, hess=stack.full_hess, method=method or "Newton-CG", options=options)
    return stack.full_mosaic(res.x, out_device=out_device), res.x, res


def chunk_cut_device(dyn_t, origins, cwf, cwt, fortran_order=False):
    """The chunks of Dynspec.thetatheta_chunks cut on the device (dynspec.py:1782-1790: ``dspec2 = dyn[fs, ts]; dspec2 -=
    nanmean(dspec2); dspec2 = nan_to_num(dspec2)``) and the padding value of each (its mean, ththmod.py:783), NumPy's summation
    order restated (csrc/mosaic.hip).  dyn_t: device [nf, nt] float64; origins: [(r0, c0)].  Returns (chunks [n, cwf, cwt], pads [n]).
    ``fortran_order``: the host array the reference would slice is Fortran-ordered (a transposed view: how psrflux files load) --
    ``np.copy`` keeps that order and NumPy's sums walk the window column by column; the means are then formed in that order."""
    nf, nt = (int(v) for v in dyn_t.shape)
    n = len(origins)
    o = np.asarray(origins, dtype=np.int32).reshape(n, 2)
    if n < 1 or o.min() < 0 or (o[:, 0] + cwf).max() > nf or (o[:, 1] + cwt).max() > nt:
        raise ValueError("chunk_cut_device: a window lies outside the dynamic spectrum")
    r0_t, c0_t = _dv.to_device(np.ascontiguousarray(o[:, 0]), torch.int32), _dv.to_device(np.ascontiguousarray(o[:, 1]), torch.int32)
    out_t, pad_t = empty((n, cwf, cwt), torch.float64), empty((n,), torch.float64)
    ws = workspace_for("scint_mosaic", cwf, cwt, n)
    _lib.call("scint_chunk_cut", dyn_t, nf, nt, r0_t, c0_t, n, cwf, cwt, 1 if fortran_order else 0, out_t, pad_t, ws, ws.numel(),
              stream_ptr())
    return out_t, pad_t


def gerchberg_saxton_device(wavefield, dyn, tau, niter=1):
    """Gerchberg-Saxton clean-up of a wavefield (Dynspec.gerchberg_saxton, dynspec.py:1858-1875):
    host normalisation + first amplitude projection, then `niter` device iterations of
    fft2 -> zero tau < 0 -> ifft2 -> amplitude projection.  Returns the new wavefield (NumPy)."""
    _lib.load()
    wf = np.array(wavefield, dtype=complex)
    F, T = wf.shape
    d = np.asarray(dyn, dtype=float)[:F, :T]
    posdspec = np.isfinite(d) * (d > 0)
    wf *= np.sqrt(d[posdspec].mean() / np.abs(wf[posdspec] ** 2).mean())
    wf[posdspec] = np.sqrt(d[posdspec]) * np.exp(1j * np.angle(wf[posdspec]))
    if niter <= 0:
        return wf
    tau_v = units.strip(tau, "tau", "us", warn=False)
    neg = np.nonzero(tau_v < 0)[0]                      # rows of the fftshifted CWF to clear
    nat = np.sort((neg - F // 2) % F)                    # the same rows in natural FFT order
    if nat.size and (nat[-1] - nat[0] + 1 != nat.size):
        raise ValueError("tau < 0 is not a contiguous block of delays")
    lo, hi = (int(nat[0]), int(nat[-1]) + 1) if nat.size else (0, 0)
    amp = np.zeros((F, T))
    amp[posdspec] = np.sqrt(d[posdspec])
    wf_t = _dv.to_device(wf, torch.complex128)
    amp_t = _dv.to_device(amp, torch.float64)
    pos_t = _dv.to_device(posdspec.astype(np.uint8), torch.uint8)
    ws = workspace_for("scint_gs", F, T)
    _lib.call("scint_gerchberg_saxton", wf_t, F, T, amp_t, pos_t, lo, hi, int(niter), ws, ws.numel(), stream_ptr())
    return wf_t.cpu().numpy()


def calc_asymmetry(params):
    """Arc asymmetry of one chunk from the dominant theta-theta eigenvector
    (ththmod.py:2385-2463): (sum|V_left|^2 - sum|V_right|^2) / (sum|V_left|^2 + sum|V_right|^2).

    params = (dspec2, edges, time, freq, eta, idx_t, idx_f, npad, verbose).  Only the
    eigenvector of the reduced theta-theta is needed, so the model/back-map steps of the
    reference's modeler call are skipped.  Returns (asymm, idx_f, idx_t); NaN on failure."""
    dspec2, edges, time, freq, eta, idx_t, idx_f, npad, verbose = params
    _, _, edges_v, tau, fd = _chunk_axes(time, freq, edges, npad)
    e = _eta_float(eta)
    try:
        cs_t = conjugate_spectrum(np.asarray(dspec2, dtype=float), npad)
        w, V_t, info = eigvec_sweep(cs_t, tau, fd, np.array([e]), edges_v)
        if info["status"][0] != 0:
            raise ArithmeticError(f"eigenpair iteration failed (status {int(info['status'][0])})")
        n = int(info["N"][0])
        p = np.abs(V_t[0, :n].cpu().numpy()) ** 2
        half = (n - 1) // 2                     # cents.shape[0] == n  (ththmod.py:2447-2449)
        left, right = p[:half].sum(), p[1 + half:].sum()
        asymm = (left - right) / (left + right)
        if verbose:
            print("Chunk %s-%s success" % (idx_f, idx_t), flush=True)
    except Exception as exc:
        print(exc, flush=True)
        asymm = np.nan
    return (asymm, idx_f, idx_t)


# ----------------------------------------------------------------------------
# thin-screen curvature search (fitting_proc='thin', ththmod.py:496-712 and 1557-1636)
# ----------------------------------------------------------------------------
def _thin_geom(tau, fd):
    """scint_thin_geom of (tau, fd): the reference's own expressions (ththmod.py:1593-1604)."""
    g = _lib.ThinGeom()
    g.ntau, g.nfd = int(tau.shape[0]), int(fd.shape[0])
    g.tau1, g.dtau = float(tau[1]), float(np.diff(tau).mean())
    g.fd1, g.dfd = float(fd[1]), float(np.diff(fd).mean())
    return g


def _thin_centres(edges):
    return (edges[1:] + edges[:-1]) / 2                     # ththmod.py:1583-1584: no re-centring


def _run(mask):
    """(first, count) of a boolean mask that must be one run of True."""
    idx = np.nonzero(mask)[0]
    if idx.size == 0:
        return 0, 0
    if idx[-1] - idx[0] + 1 != idx.size:
        raise ValueError("thin theta-theta: a crop or centre cut is not one run of centres (edges must be monotonic)")
    return int(idx[0]), int(idx.size)


def _reduced_edges(edges, pnts):
    """edges_red of two_curve_map (ththmod.py:1625-1630); raises ValueError on an empty crop, as the reference's .max() does."""
    er = np.zeros(pnts[pnts].shape[0] + 1)
    er[:-1] = edges[:-1][pnts]
    er[-1] = edges[1:][pnts].max()
    return er


def _thin_crop(tau_max, edges1, edges2, eta1, eta2, center_cut):
    """ranges [r0, n2, c0, n1, cut0, cut1] of one map and its reduced edges, with the reference's masks:
    |centre| < sqrt(tau.max() / eta) on each axis (ththmod.py:1621-1624) and |reduced centre| < centerCut (:509)."""
    pnts_1 = np.abs(_thin_centres(edges1)) < np.sqrt(tau_max / eta1)
    pnts_2 = np.abs(_thin_centres(edges2)) < np.sqrt(tau_max / eta2)
    er1, er2 = _reduced_edges(edges1, pnts_1), _reduced_edges(edges2, pnts_2)
    c0, n1 = _run(pnts_1)
    r0, n2 = _run(pnts_2)
    cut0, ncut = _run(np.abs(_thin_centres(er1)) < center_cut)
    return np.array([r0, n2, c0, n1, cut0, cut0 + ncut], dtype=np.int32), er1, er2


def _thin_check(geom, th1, th2):
    """1 if some point of the grid can reach fd_inv < -nfd (NumPy's IndexError, ththmod.py:1612): fd_inv is monotone in
    th1 - th2, so its smallest value is at (min th1, max th2)."""
    if th1.size == 0 or th2.size == 0:
        return 0
    a = ((th1.min() - th2.max()) - geom.fd1) + geom.dfd / 2
    return int(np.floor_divide(a, geom.dfd) < -geom.nfd or not np.isfinite(a))


def _thin_cs_dev(CS, tau, fd):
    t = to_device(CS, torch.complex128)
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if tuple(t.shape[1:]) != (tau.shape[0], fd.shape[0]):
        raise ValueError(f"CS shape {tuple(t.shape[1:])} does not match (len(tau), len(fd)) = ({tau.shape[0]}, {fd.shape[0]})")
    return t.contiguous()


def two_curve_map(CS, tau, fd, eta1, edges1, eta2, edges2):
    """Rectangular theta-theta for arclets of another curvature (ththmod.py:1557-1636): returns
    (thth_red[n2, n1], edges_red1, edges_red2) -- rows theta2 (edges2), columns theta1 (edges1) -- with the reference's index
    quirks (tau[1] / fd[1] origins, the negative-Doppler wrap, IndexError below -nfd)."""
    require_gpu()
    tau_v = units.strip(tau, "tau", "us", warn=False)
    fd_v = units.strip(fd, "fd", "mHz", warn=False)
    e1 = np.array(units.strip(edges1, "edges1", "mHz", warn=False), dtype=float)
    e2 = np.array(units.strip(edges2, "edges2", "mHz", warn=False), dtype=float)
    eta1_v, eta2_v = _eta_float(eta1), _eta_float(eta2)
    geom = _thin_geom(tau_v, fd_v)
    th1, th2 = _thin_centres(e1), _thin_centres(e2)
    if th1.size < 1 or th2.size < 1:
        raise ValueError("two_curve_map: edges need at least two points")
    rng, er1, er2 = _thin_crop(tau_v.max(), e1, e2, eta1_v, eta2_v, 0.0)
    cs_t = _thin_cs_dev(CS, tau_v, fd_v)
    n2, n1 = int(rng[1]), int(rng[3])
    out = empty((max(n2, 1), max(n1, 1)), torch.complex128)
    flag = torch.zeros((1,), dtype=torch.int32, device=out.device)
    ws = workspace_for("scint_two_curve_map")
    th1_t, th2_t = to_device(th1, torch.float64), to_device(th2, torch.float64)
    _lib.call("scint_two_curve_map", cs_t, geom, th1_t, th1.size, th2_t, th2.size, eta1_v, eta2_v, rng, _thin_check(geom, th1, th2),
              out, flag, ws, ws.numel(), stream_ptr())
    if int(flag.cpu()[0]):
        raise IndexError("two_curve_map: a Doppler index below -len(fd) (NumPy's fancy index raises here, ththmod.py:1612)")
    red = out[:n2, :n1].cpu().numpy()
    return red, units.attach(er1, "mHz"), units.attach(er2, "mHz")


def _sv_run(cs_t, geoms, th1_stack, th2_stack, cs_index, ranges, checks, etas1, etas2, tol, max_iter, batch):
    """scint_sv_sweep_multi on prepared inputs: (sv[neta], NaN where the status is not 0; status[neta], iters[neta], batch)."""
    ncs, M1, M2 = len(geoms), int(th1_stack.shape[1]), int(th2_stack.shape[1])
    neta = int(etas1.shape[0])
    _check_sweep_cs(geoms[0].ntau, geoms[0].nfd)
    if batch is None:
        per = 16 * M1 * M2 + 96 * M1 + 16 * M1 * -(-M2 // max(4, -(-M2 // 256))) + 16 * max_iter + 4096
        batch = int(max(1, min(neta, 8192, DEFAULT_BATCH_BYTES // per)))
    ws = workspace_for("scint_sv_sweep_multi", M1, M2, neta, batch, max_iter, ncs)
    sv_t = empty((neta,), torch.float64)
    st_t = empty((2, neta), torch.int32)
    g_arr = (_lib.ThinGeom * ncs)(*geoms)
    ci = np.ascontiguousarray(cs_index, dtype=np.int32)
    rg = np.ascontiguousarray(ranges, dtype=np.int32)
    ck = np.ascontiguousarray(checks, dtype=np.int32)
    e1 = np.ascontiguousarray(etas1, dtype=np.float64)
    e2 = np.ascontiguousarray(etas2, dtype=np.float64)
    _lib.call("scint_sv_sweep_multi", cs_t, ncs, int(cs_t.shape[1] * cs_t.shape[2]), ci, g_arr, th1_stack, M1, th2_stack, M2,
              rg, ck, e1, e2, neta, tol, max_iter, batch, sv_t, st_t[0], st_t[1], ws, ws.numel(), stream_ptr())
    sv, st = _sweep_results(sv_t, st_t)       # NOCONV / EMPTY / NONFINITE / would-raise -> NaN (single_search_thin's except, :624-629)
    return sv, st[0].copy(), st[1].copy(), batch


def _thin_ranges(tau_max, edges1, edges2, etas, center_cut):
    """ranges[neta, 6] of one chunk's curvatures (eta1 = eta2 = eta); an empty crop gets n = 0 (status EMPTY -> NaN, where the
    reference's .max() of an empty selection raises inside single_search_thin's try)."""
    th1, th2 = _thin_centres(edges1), _thin_centres(edges2)
    out = np.zeros((etas.shape[0], 6), dtype=np.int32)
    a1, a2 = np.abs(th1), np.abs(th2)
    asc = th1.size > 0 and np.all(np.diff(edges1) > 0)
    cutc = a1 < center_cut
    for k, eta in enumerate(etas):
        if asc:   # ascending edges: the reduced centres are th1[c0:c0 + n1], bit for bit (same two operands per centre)
            p1 = a1 < np.sqrt(tau_max / eta)
            p2 = a2 < np.sqrt(tau_max / eta)
            c0, n1 = _run(p1)
            r0, n2 = _run(p2)
            if n1 == 0 or n2 == 0:
                continue
            cut0, ncut = _run(cutc[c0:c0 + n1])
            out[k] = (r0, n2, c0, n1, cut0, cut0 + ncut)
        else:
            try:
                out[k] = _thin_crop(tau_max, edges1, edges2, eta, eta, center_cut)[0]
            except ValueError as err:
                if "one run" in str(err):
                    raise
    return out


def sv_sweep_multi(cs_stack, grids, etas_list, center_cut=0.0, tol=DEFAULT_TOL, max_iter=DEFAULT_MAX_ITER, batch=None,
                   return_info=False):
    """Singular-value curves of MANY chunks in one batched device call -- the chunk loop of Dynspec.fit_thetatheta with
    fitting_proc='thin' (dynspec.py:1681-1719), each chunk's curvature loop being single_search_thin's (ththmod.py:588-643).

    cs_stack: [nchunk, ntau, nfd] complex128 (device tensor or array); grids: one (tau, fd, edges, edges_arclet) per chunk (all
    spectra one shape, all edges one length, all arclet edges one length); etas_list: per-chunk curvatures (main arc = arclets);
    center_cut in mHz.  Returns a list of sigma_1 arrays, NaN where single_search_thin would have caught an exception."""
    cs_t = _thin_cs_dev(cs_stack, *(units.strip(grids[0][i], n, k, warn=False) for i, n, k in ((0, "tau", "us"), (1, "fd", "mHz"))))
    ncs = len(grids)
    if cs_t.shape[0] != ncs:
        raise ValueError("cs_stack must be [nchunk, ntau, nfd] with one spectrum per grid")
    cut = float(units.strip(center_cut, "Center Cut", "mHz", warn=False))
    geoms, th1s, th2s, ranges, checks, etas_all, cs_index = [], [], [], [], [], [], []
    for c, ((tau, fd, edges, arclet), et) in enumerate(zip(grids, etas_list)):
        tau_v, fd_v = units.strip(tau, "tau", "us", warn=False), units.strip(fd, "fd", "mHz", warn=False)
        e1 = np.array(units.strip(edges, "edges", "mHz", warn=False), dtype=float)
        e2 = np.array(units.strip(arclet, "edgesArclet", "mHz", warn=False), dtype=float)
        et = np.atleast_1d(units.strip(et, "etas", "s3", warn=False)).astype(float)
        g = _thin_geom(tau_v, fd_v)
        th1, th2 = _thin_centres(e1), _thin_centres(e2)
        if (g.ntau, g.nfd) != tuple(cs_t.shape[1:]):
            raise ValueError("all chunks must share the CS shape")
        if th1s and (th1.size != th1s[0].size or th2.size != th2s[0].size):
            raise ValueError("all chunks must share the number of edges and of arclet edges")
        geoms.append(g)
        th1s.append(th1)
        th2s.append(th2)
        ranges.append(_thin_ranges(tau_v.max(), e1, e2, et, cut))
        checks.append(np.full(et.shape[0], _thin_check(g, th1, th2), dtype=np.int32))
        etas_all.append(et)
        cs_index.append(np.full(et.shape[0], c, dtype=np.int32))
    M1, M2 = th1s[0].size, th2s[0].size
    etas_v = np.concatenate(etas_all)
    if M1 < 1 or M2 < 1:          # fewer than two edges on an axis: every curvature fails, as the reference's do
        sv, st, it = np.full(etas_v.shape, np.nan), np.full(etas_v.shape, _lib.SCINT_E_EMPTY), np.zeros(etas_v.shape, int)
    else:
        th1_t = to_device(np.stack(th1s), torch.float64)
        th2_t = to_device(np.stack(th2s), torch.float64)
        sv, st, it, batch = _sv_run(cs_t, geoms, th1_t, th2_t, np.concatenate(cs_index), np.concatenate(ranges),
                                    np.concatenate(checks), etas_v, etas_v, tol, max_iter, batch)
    out = _split_chunks(sv, np.cumsum([0] + [e.shape[0] for e in etas_all]))
    if return_info:
        return out, {"status": st, "iters": it, "ranges": np.concatenate(ranges), "batch": batch}
    return out


def singularvalue_calc(CS, tau, fd, eta, edges, etaArclet, edgesArclet, centerCut):
    """Largest singular value of the centre-cut two-curvature map (ththmod.py:496-513).  Raises where the reference raises:
    ValueError for an empty crop, IndexError where the map's Doppler index is out of NumPy's range."""
    tau_v = units.strip(tau, "tau", "us", warn=False)
    fd_v = units.strip(fd, "fd", "mHz", warn=False)
    e1 = np.array(units.strip(edges, "edges", "mHz", warn=False), dtype=float)
    e2 = np.array(units.strip(edgesArclet, "edgesArclet", "mHz", warn=False), dtype=float)
    eta1_v, eta2_v = _eta_float(eta), _eta_float(etaArclet)
    cut = float(units.strip(centerCut, "Center Cut", "mHz", warn=False))
    rng, _, _ = _thin_crop(tau_v.max(), e1, e2, eta1_v, eta2_v, cut)       # ValueError on an empty crop, as the reference
    cs_t = _thin_cs_dev(CS, tau_v, fd_v)
    geom = _thin_geom(tau_v, fd_v)
    th1, th2 = _thin_centres(e1), _thin_centres(e2)
    sv, st, _, _ = _sv_run(cs_t, [geom], to_device(th1[None, :], torch.float64), to_device(th2[None, :], torch.float64),
                           np.zeros(1, np.int32), rng[None, :], np.array([_thin_check(geom, th1, th2)], np.int32),
                           np.array([eta1_v]), np.array([eta2_v]), DEFAULT_TOL, DEFAULT_MAX_ITER, 1)
    if st[0] == _lib.SCINT_E_ARG:
        raise IndexError("singularvalue_calc: a Doppler index below -len(fd) (NumPy's fancy index raises, ththmod.py:1612)")
    if st[0] == _lib.SCINT_E_NONFINITE:
        raise np.linalg.LinAlgError("singularvalue_calc: non-finite theta-theta (SVD did not converge)")
    if st[0] != 0:
        raise ArithmeticError(f"singularvalue_calc failed (status {int(st[0])})")
    return float(sv[0])


def single_search_thin(params):
    """Thin-screen curvature search for one chunk (ththmod.py:516-712).

    params = [dspec2, freq, time, etas, edges, name, plot, fw, npad, coher, verbose, edgesArclet, centerCut] as in the
    reference (padding with dspec2.mean(), no delay mask).  Plotting is not supported (`plot=True` only warns).  Returns
    (eta_fit, eta_sig, freq.mean(), time.mean(), eigs) with eigs the singular values of the curvatures that did not fail."""
    (dspec2, freq, time, etas, edges, name, plot, fw, npad, coher, verbose, edgesArclet, centerCut) = params
    time_v, freq_v, edges_v, tau, fd = _chunk_axes(time, freq, edges, npad, ("time", "freq"))      # ththmod.py:582-583
    etas_v = np.atleast_1d(units.strip(etas, "etas", "s3", warn=False)).astype(float)
    # coherent: CS; incoherent: |CS|^2 (ththmod.py:630-631) -- scint_cs's incoherent mode is |CS|, so square it here
    cs_t = conjugate_spectrum(dspec2, npad, coher=True)
    if not coher:
        cs_t = (cs_t.abs() ** 2).to(torch.complex128)
    eigs = sv_sweep_multi(cs_t.unsqueeze(0), [(tau, fd, edges_v, edgesArclet)], [etas_v], centerCut)[0]
    eta_fit, eta_sig, _ = fit_eig_peak(etas_v, eigs, fw)
    if plot:
        warnings.warn("scintools_amd.single_search_thin does not plot")
    if verbose:
        print(f"Chunk completed (eta = {eta_fit} +- {eta_sig} at {freq_v.mean()})", flush=True)
    if np.isfinite(eta_fit):
        eta_fit, eta_sig = units.attach(eta_fit, "s3"), units.attach(eta_sig, "s3")
    return (eta_fit, eta_sig, units.attach(freq_v.mean(), "MHz"), units.attach(time_v.mean(), "s"),
            eigs[np.isfinite(eigs)])
