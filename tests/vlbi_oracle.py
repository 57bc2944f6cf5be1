"""Plain-float NumPy restatement of the reference's VLBI_chunk_retrieval (scintools/ththmod.py:1223-1387), built on the
functions of oracle/thth_oracle.py (imported, not edited).  Same operation order as the reference; no units."""
import numpy as np
from scipy.sparse.linalg import eigsh

from oracle import thth_oracle as to


def spectrum_index(n_dish, d1, d2):
    """ththmod.py:1345-1349."""
    return int(((n_dish * (n_dish + 1)) // 2) - (((n_dish - d1) * (n_dish - d1 + 1)) // 2) + d2)


def reduced_maps(dlist, edges, time, freq, eta, npad, n_dish, tau_mask=0.0):
    """ththmod.py:1284-1331: (list of reduced theta-theta, hermetian flags, edges_red, tau, fd)."""
    fd = to.fft_axis(time, 1000.0, npad)
    tau = to.fft_axis(freq, 1.0, npad)
    dspec_args = (n_dish * (n_dish + 1)) / 2 - np.cumsum(np.linspace(1, n_dish, n_dish))
    reds, flags, edges_red = [], [], None
    for i in range(len(dlist)):
        x = np.asarray(dlist[i])
        herm = bool(np.isin(i, dspec_args))
        pad = np.pad(x, ((0, npad * x.shape[0]), (0, npad * x.shape[1])), mode="constant",
                     constant_values=x.mean() if herm else 0)
        CS = np.fft.fftshift(np.fft.fft2(pad))
        CS[np.abs(tau) < tau_mask] = 0
        red, edges_red = to.thth_redmap(CS, tau, fd, eta, edges, hermetian=herm)
        reds.append(red)
        flags.append(herm)
    return reds, flags, edges_red, tau, fd


def composite(reds, n_dish):
    """ththmod.py:1333-1362."""
    n = reds[0].shape[0]
    comp = np.zeros((n * n_dish, n * n_dish), dtype=complex)
    for d1 in range(n_dish):
        for d2 in range(n_dish - d1):
            idx = spectrum_index(n_dish, d1, d2)
            comp[d1 * n:(d1 + 1) * n, (d1 + d2) * n:(d1 + d2 + 1) * n] = np.conjugate(reds[idx].T)
            comp[(d1 + d2) * n:(d1 + d2 + 1) * n, d1 * n:(d1 + 1) * n] = reds[idx]
    return comp


def vlbi_chunk_retrieval(dlist, edges, time, freq, eta, npad, n_dish, tau_mask=0.0):
    """ththmod.py:1223-1387 -> model_E [n_dish, nf, nt]."""
    reds, _, edges_red, tau, fd = reduced_maps(dlist, edges, time, freq, eta, npad, n_dish, tau_mask)
    n = reds[0].shape[0]
    comp = composite(reds, n_dish)
    w, V = eigsh(comp, 1, which="LA")
    w, V = w[0], V[:, 0]
    nf, nt = np.asarray(dlist[0]).shape
    out = np.empty((n_dish, nf, nt), dtype=complex)
    tmp = np.zeros((n, n), dtype=complex)
    for d in range(n_dish):
        tmp *= 0
        tmp[n // 2, :] = np.conjugate(V[d * n:(d + 1) * n]) * np.sqrt(w)
        with np.errstate(all="ignore"):
            recov = to.rev_map(tmp, tau, fd, eta, edges_red, hermetian=False)
        out[d] = np.fft.ifft2(np.fft.ifftshift(recov))[:nf, :nt] * (nf * nt / 4)
    return out
