"""NumPy restatement of the reference's thin-screen search (ththmod.py:496-712, 1557-1636) on plain floats (us, mHz, s**3).

Test tooling: it does not import the reference; tests/test_thin_cpu.py pins it bit for bit to tests/golden/thin.npz, which the
reference itself wrote (tests/golden/make_golden_thin.py).  Besides the values it can report where the negative Doppler index
wraps (``two_curve_map(..., stats=True)``).
"""
import numpy as np
from scipy.optimize import curve_fit


def fft_axis(x, scale, pad=0):
    """ththmod.fft_axis with the unit conversion as a factor (1000 for s -> mHz, 1 for MHz -> us)."""
    fx = np.fft.fftfreq((pad + 1) * x.shape[0], x[1] - x[0])
    if scale != 1.0:
        fx = fx * scale
    return np.fft.fftshift(fx)


def two_curve_map(CS, tau, fd, eta1, edges1, eta2, edges2, stats=False):
    th_cents1 = (edges1[1:] + edges1[:-1]) / 2
    th_cents2 = (edges2[1:] + edges2[:-1]) / 2
    th1 = np.ones((th_cents2.shape[0], th_cents1.shape[0])) * th_cents1
    th2 = np.ones((th_cents2.shape[0], th_cents1.shape[0])) * th_cents2[:, np.newaxis]
    dtau = np.diff(tau).mean()
    dfd = np.diff(fd).mean()
    tau_inv = (((eta1 * th1**2 - eta2 * th2**2) - tau[1] + dtau / 2) // dtau).astype(int)
    fd_inv = (((th1 - th2) - fd[1] + dfd / 2) // dfd).astype(int)
    thth = np.zeros(tau_inv.shape, dtype=complex)
    pnts = (tau_inv > 0) * (tau_inv < tau.shape[0] - 1) * (fd_inv < fd.shape[0] - 1)
    thth[pnts] = CS[tau_inv[pnts], fd_inv[pnts]]          # IndexError below -len(fd), a wrap above it
    thth *= np.sqrt(np.abs(2 * eta1 * th1 - 2 * eta2 * th2))
    th2_max = np.sqrt(tau.max() / eta2)
    th1_max = np.sqrt(tau.max() / eta1)
    pnts_1 = np.abs(th_cents1) < th1_max
    pnts_2 = np.abs(th_cents2) < th2_max
    edges_red1 = np.zeros(pnts_1[pnts_1].shape[0] + 1)
    edges_red1[:-1] = edges1[:-1][pnts_1]
    edges_red1[-1] = edges1[1:][pnts_1].max()
    edges_red2 = np.zeros(pnts_2[pnts_2].shape[0] + 1)
    edges_red2[:-1] = edges2[:-1][pnts_2]
    edges_red2[-1] = edges2[1:][pnts_2].max()
    thth_red = thth[pnts_2, :][:, pnts_1]
    if stats:
        wrap = (pnts & (fd_inv < 0))[pnts_2, :][:, pnts_1]
        return thth_red, edges_red1, edges_red2, wrap
    return thth_red, edges_red1, edges_red2


def singularvalue_calc(CS, tau, fd, eta, edges, etaArclet, edgesArclet, centerCut):
    thth_red, edges_red1, edges_red2 = two_curve_map(CS, tau, fd, eta, edges, etaArclet, edgesArclet)
    cents1 = (edges_red1[1:] + edges_red1[:-1]) / 2
    thth_red[:, np.abs(cents1) < centerCut] = 0
    U, S, W = np.linalg.svd(thth_red)        # (with the vectors, as the reference: another LAPACK path than compute_uv=False)
    return S[0]


def chi_par(x, A, x0, C):
    return A * (x - x0) ** 2 + C


def single_search_thin(params):
    """(eta_fit, eta_sig, freq.mean(), time.mean(), eigs) with plain floats; plotting is not restated."""
    (dspec2, freq, time, etas, edges, name, plot, fw, npad, coher, verbose, edgesArclet, centerCut) = params
    fd = fft_axis(time, 1000.0, npad)
    tau = fft_axis(freq, 1.0, npad)
    dspec_pad = np.pad(dspec2, ((0, npad * dspec2.shape[0]), (0, npad * dspec2.shape[1])), mode="constant",
                       constant_values=dspec2.mean())
    CS = np.fft.fftshift(np.fft.fft2(dspec_pad))
    src = CS if coher else np.abs(CS) ** 2
    eigs = np.zeros(etas.shape)
    for i in range(eigs.shape[0]):
        try:
            eigs[i] = singularvalue_calc(src, tau, fd, etas[i], edges, etas[i], edgesArclet, centerCut)
        except Exception:
            eigs[i] = np.nan
    try:
        etas = etas[np.isfinite(eigs)]
        eigs = eigs[np.isfinite(eigs)]
        sel = np.abs(etas - etas[eigs == eigs.max()]) < fw * etas[eigs == eigs.max()]
        etas_fit, eigs_fit = etas[sel], eigs[sel]
        C = eigs_fit.max()
        x0 = etas_fit[eigs_fit == C][0]
        if x0 == etas_fit[0]:
            A = (eigs_fit[-1] - C) / ((etas_fit[-1] - x0) ** 2)
        else:
            A = (eigs_fit[0] - C) / ((etas_fit[0] - x0) ** 2)
        popt, _ = curve_fit(chi_par, etas_fit, eigs_fit, p0=np.array([A, x0, C]))
        eta_fit = popt[1]
        eta_sig = np.sqrt((eigs_fit - chi_par(etas_fit, *popt)).std() / np.abs(popt[0]))
    except Exception:
        eta_fit, eta_sig = np.nan, np.nan
    return eta_fit, eta_sig, freq.mean(), time.mean(), eigs
