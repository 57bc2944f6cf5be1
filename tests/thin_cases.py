"""Case builders for the thin-screen sigma_1 sweep (scint_sv_sweep_multi, scint_two_curve_map), shared by
tests/test_gpu_thin_classes.py (every mat-vec class, on an MI355X) and tests/test_thin_emu_cpu.py (the small ones, on the host
interpreter).  The reference for every value is tests/thin_oracle.py followed by a dense LAPACK SVD.

The number of theta edges is independent of the spectrum size, so one 256 x 256 conjugate spectrum serves maps of 1 x 150 up to
300 x 16384 pixels: theta1 edges `linspace(-fd_max, fd_max, n1 + 1)`, arclet edges `linspace(-fd_max / 2, fd_max / 2, n2 + 1)`
and the curvature eta0 = 0.9 tau_max / fd_max^2, whose crop |theta| < sqrt(tau_max / eta0) = 1.054 fd_max keeps every centre.
The kept sizes are therefore exactly (n1, n2); the tests still read them back from the call (info["ranges"]).

sv_class restates the documented class boundaries of sv_matvec_kernel (eigen.hip): 256 threads x K = 1, 2, 4, 8, 16 columns
per thread for n1 <= 256 .. 4096, then 512 x 16 and 1024 x 16; K <= 8 takes two rows at a time.  A workgroup owns
R = max(4, ceil(n2 / 256)) rows."""
import numpy as np

import thin_oracle as to

NS = 256                        # the spectrum is NS x NS
SV_BOUNDS = (256, 512, 1024, 2048, 4096, 8192, 16384)
SV_MAX_COLS = 16384
FIRST_CHECK = 16                # the first convergence check of the sweep
MAX_ITER = 300                  # ththmod.DEFAULT_MAX_ITER (asserted by the tests that rely on it)

# n1 of every class: both sides of every boundary and one interior point
CLASS_N1 = ((150, 256), (257, 400, 512), (513, 777, 1024), (1025, 1500, 2048), (2049, 3001, 4096), (4097, 4750, 8192),
            (8193, 11999, 16384))
# n2: one row, two, three (odd: the two-rows-at-a-time tail), one full strip, one full and one partial strip, fewer rows than
# steps before the first check, and R = 4 with G = 75 strips
N2_EDGE = (1, 2, 3, 4, 5, 11, 300)
N2_TALL = 1301                  # R = 6, G = 217, last strip 5 rows (the two smallest classes)


def sv_class(n1):
    for k, b in enumerate(SV_BOUNDS):
        if n1 <= b:
            return k
    raise ValueError(n1)


def rows_per_group(n2):
    return max(4, -(-n2 // 256))


def class_cases():
    """[(n1, n2, kind, cut_fraction)]: every n1 of CLASS_N1 with every n2 of N2_EDGE (n2 = 1301 for n1 <= 512 too); the spectrum
    kind and the centre cut rotate so that each class sees both spectra with and without the cut."""
    out = []
    for cls, n1s in enumerate(CLASS_N1):
        for n1 in n1s:
            for n2 in N2_EDGE + ((N2_TALL,) if cls < 2 else ()):
                i = len(out)
                out.append((n1, n2, ("arc", "gauss")[i % 2], (0.0, 0.02)[(i // 2) % 2]))
    return out


def small_class_cases():
    """The members the host interpreter runs: n1 <= 513 with the n2 edge values below the first check."""
    return [c for c in class_cases() if c[0] <= 513 and c[1] < FIRST_CHECK]


def axes():
    """(tau, fd, eta_true) of the NS x NS arc_dynspec chunk."""
    from scintools_amd.synth import arc_axes
    freqs, times, _, _ = arc_axes(NS, NS, 0.02, None, 30.0, 1400.0, None)
    return to.fft_axis(freqs, 1.0, 0), to.fft_axis(times, 1000.0, 0)


def spectrum(kind, seed=0):
    """Conjugate spectrum [NS, NS]: 'arc' a simulated scintillation arc, 'gauss' dense complex Gaussian numbers (every map a
    dense random rectangle whose top singular value is poorly separated), 'code' the 1-based flat pixel index (to find which
    pixels a map reads), 'zero'."""
    if kind == "arc":
        from scintools_amd.synth import arc_dynspec
        dyn = arc_dynspec(NS, NS, seed=seed + 5, nimg=24)[0]
        return np.fft.fftshift(np.fft.fft2(dyn - dyn.mean()))
    if kind == "gauss":
        rng = np.random.default_rng(100 + seed)
        return rng.standard_normal((NS, NS)) + 1j * rng.standard_normal((NS, NS))
    if kind == "code":
        return np.arange(1, NS * NS + 1, dtype=float).reshape(NS, NS).astype(complex)
    if kind == "zero":
        return np.zeros((NS, NS), dtype=complex)
    raise ValueError(kind)


def eta0(tau, fd):
    return 0.9 * tau.max() / fd.max() ** 2


def grid(n1, n2, tau, fd, span2=0.5):
    """(tau, fd, edges, arclet) whose maps at eta0 are n2 x n1."""
    fdm = fd.max()
    return tau, fd, np.linspace(-fdm, fdm, n1 + 1), np.linspace(-span2 * fdm, span2 * fdm, n2 + 1)


def oracle_map(CS, tau, fd, eta1, edges, eta2, arclet, cut):
    """The centre-cut map singularvalue_calc decomposes (thin_oracle.two_curve_map, then the cut)."""
    red, er1, _ = to.two_curve_map(CS, tau, fd, eta1, edges, eta2, arclet)
    red = red.copy()
    red[:, np.abs((er1[1:] + er1[:-1]) / 2) < cut] = 0
    return red


def oracle_sv(CS, tau, fd, eta1, edges, eta2, arclet, cut, with_gap=False):
    s = np.linalg.svd(oracle_map(CS, tau, fd, eta1, edges, eta2, arclet, cut), compute_uv=False)
    if with_gap:
        return s[0], (s[1] / s[0] if s.shape[0] > 1 and s[0] > 0 else 0.0)
    return s[0]


def pixels_read(tau, fd, eta1, edges, eta2, arclet, row=None):
    """Flat indices of the spectrum pixels the kept map reads with a non-zero weight (all kept rows, or kept row `row`): the
    oracle on the index-coded spectrum, the sqrt(|2 eta1 th1 - 2 eta2 th2|) weight divided out again."""
    red, er1, er2 = to.two_curve_map(spectrum("code"), tau, fd, eta1, edges, eta2, arclet)
    th1 = (er1[1:] + er1[:-1]) / 2
    th2 = (er2[1:] + er2[:-1]) / 2
    w = np.sqrt(np.abs(2 * eta1 * th1[None, :] - 2 * eta2 * th2[:, None]))
    if row is not None:
        red, w = red[row:row + 1], w[row:row + 1]
    ok = w > 0
    idx = np.rint(red.real[ok] / w[ok]).astype(np.int64)
    return np.unique(idx[idx > 0]) - 1


def zero_middle_row(CS, tau, fd, eta, edges, arclet):
    """CS with the pixels of the kept middle row (n2 // 2, the Lanczos start vector) zeroed; checked with the oracle: that row
    is zero and the map is not."""
    out = CS.copy()
    n2 = to.two_curve_map(CS, tau, fd, eta, edges, eta, arclet)[0].shape[0]
    out.flat[pixels_read(tau, fd, eta, edges, eta, arclet, row=n2 // 2)] = 0
    red = to.two_curve_map(out, tau, fd, eta, edges, eta, arclet)[0]
    assert not red[n2 // 2].any() and np.count_nonzero(red) > red.shape[1]
    return out


def poisoned(CS, tau, fd, eta, edges, arclet, value, which=0):
    """CS with one pixel the kept map reads (not in the middle row when the map has other rows) set to `value`."""
    out = CS.copy()
    n2 = to.two_curve_map(CS, tau, fd, eta, edges, eta, arclet)[0].shape[0]
    px = pixels_read(tau, fd, eta, edges, eta, arclet)
    if n2 > 1:
        px = np.setdiff1d(px, pixels_read(tau, fd, eta, edges, eta, arclet, row=n2 // 2))
    out.flat[px[(which * 7919) % px.size]] = value
    with np.errstate(invalid="ignore"):
        red = to.two_curve_map(out, tau, fd, eta, edges, eta, arclet)[0]
    assert not np.all(np.isfinite(red))
    return out


# ---- the gather fuzz ---------------------------------------------------------------------------------------------------
GATHER_SHAPES = ((75, 101), (128, 96), (600, 256), (96, 128), (256, 256), (64, 333))
GATHER_CASES = 60


def gather_case(k):
    """Case k of the two_curve_map fuzz: dict(CS, tau, fd, eta1, edges1, eta2, edges2).  Spectrum shapes that are neither square
    nor powers of two; curvatures 0.3 .. 3 x the one that fills the arc, independent per axis; uniform or quadratically spaced
    ascending edges spanning 0.2 .. 1.0 fd_max (every sixth case 1.5 .. 1.7 fd_max, where the Doppler index goes below
    -len(fd) and NumPy raises); every fifth case more than 4096 kept columns."""
    rng = np.random.default_rng(7000 + k)
    ntau, nfd = GATHER_SHAPES[k % len(GATHER_SHAPES)]
    tau = to.fft_axis(1400.0 + 0.1 * np.arange(ntau), 1.0, 0)
    fd = to.fft_axis(10.0 * np.arange(nfd), 1000.0, 0)
    CS = rng.standard_normal((ntau, nfd)) + 1j * rng.standard_normal((ntau, nfd))
    fdm = fd.max()
    raising = k % 6 == 3
    big = k % 5 == 2

    def edges(n, span, offset):
        if rng.integers(2):
            e = np.linspace(-1.0, 1.0, n)
        else:
            u = np.linspace(-1.0, 1.0, n)
            e = np.sign(u) * u ** 2 * 0.7 + 0.3 * u          # quadratic spacing, ascending
        return (e * span + offset) * fdm

    span1 = rng.uniform(1.5, 1.7) if raising else rng.uniform(0.2, 1.0)
    span2 = rng.uniform(1.5, 1.7) if raising else rng.uniform(0.2, 1.0)
    n1 = int(rng.integers(5000, 9000)) if big else int(rng.integers(3, 700))
    n2 = int(rng.integers(2, 40)) if big else int(rng.integers(2, 300))
    e1 = edges(n1, span1, rng.uniform(-0.05, 0.05))
    e2 = edges(n2, span2, rng.uniform(-0.05, 0.05))
    eta_fill = tau.max() / (span1 * fdm) ** 2
    # big cases keep the whole span (factor < 1), the others crop at factor > 1
    f1 = rng.uniform(0.3, 0.95) if big else rng.uniform(0.3, 3.0)
    f2 = rng.uniform(0.3, 3.0)
    return dict(CS=CS, tau=tau, fd=fd, eta1=f1 * eta_fill, edges1=e1, eta2=f2 * eta_fill, edges2=e2)
