"""NumPy / SciPy restatement of the array work of Dynspec.scale_dyn(scale='velocity') and (scale='trapezoid'), with the reference's
line numbers (scintools/dynspec.py), and the float64 tridiagonal-moment algorithm the row kernel runs.  Pinned to the unmodified
reference's outputs by tests/test_scale_cpu.py; the GPU tests compare the device with these."""
import numpy as np
from scipy.interpolate import interp1d


# ---------------------------------------------------------------------------------------------------------------- velocity
def velocity_grid(veff):
    """dynspec.py:4056-4068, in the precision of veff (float128 in the reference)."""
    vc_orig = np.cumsum(veff)                                                   # 4056
    vc_new = np.linspace(np.min(vc_orig), np.max(vc_orig), len(vc_orig))         # 4059-4060
    if max(vc_new) > max(vc_orig):                                              # 4065-4066
        vc_new[np.argmax(vc_new)] = max(vc_orig)
    if min(vc_new) < min(vc_orig):                                              # 4067-4068
        vc_new[np.argmin(vc_new)] = min(vc_orig)
    return vc_orig, vc_new


def spline_rows(arin, x, xnew):
    """dynspec.py:4062-4069: one interp1d(kind='cubic') per row, the same scipy routine on the same axes."""
    arout = np.zeros([arin.shape[0], len(xnew)])
    for ii in range(arin.shape[0]):
        arout[ii, :] = interp1d(x, arin[ii, :], kind='cubic')(xnew)
    return arout


def velocity(arin, veff):
    """vdyn of dynspec.py:4055-4077 for a given effective velocity."""
    vc_orig, vc_new = velocity_grid(veff)
    return spline_rows(arin, vc_orig, vc_new)


def spline_system(x):
    """Thomas factors of the not-a-knot spline in second-derivative form on ascending knots x: interior rows i = 1..n-2,
    a_i M[i-1] + b_i M[i] + c_i M[i+1] = 6 ((y[i+1]-y[i])/h[i] - (y[i]-y[i-1])/h[i-1]), M[0] and M[n-1] eliminated through the
    not-a-knot conditions (written out here independently of scintools_amd.arcfit._spline_system)."""
    n = len(x)
    h = np.diff(x)
    a, b, c = np.zeros(n), np.zeros(n), np.zeros(n)
    for i in range(1, n - 1):
        a[i], b[i], c[i] = h[i - 1], 2 * (h[i - 1] + h[i]), h[i]
    b[1] = (h[0] + h[1]) * (h[0] + 2 * h[1]) / h[1]
    c[1] = (h[1]**2 - h[0]**2) / h[1]
    a[1] = 0.0
    b[n - 2] = (h[n - 2] + h[n - 3]) * (h[n - 2] + 2 * h[n - 3]) / h[n - 3]
    a[n - 2] = (h[n - 3]**2 - h[n - 2]**2) / h[n - 3]
    c[n - 2] = 0.0
    return h, a, b, c


def moments_rows(arin, x, xnew):
    """The algorithm of scint_spline_resample_rows in float64 NumPy, every row in ONE sequential Thomas sweep: moments M from the
    tridiagonal system, then S = A y[k] + B y[k+1] + ((A^3 - A) M[k] + (B^3 - B) M[k+1]) h[k]^2 / 6 on the interval k of a target."""
    x = np.asarray(x, dtype=float)
    xnew = np.asarray(xnew, dtype=float)
    y = np.asarray(arin, dtype=float)
    n = len(x)
    h, a, b, c = spline_system(x)
    r = np.zeros_like(y)
    r[:, 1:n - 1] = 6.0 * ((y[:, 2:] - y[:, 1:n - 1]) / h[1:] - (y[:, 1:n - 1] - y[:, :n - 2]) / h[:n - 2])
    d = np.zeros_like(y)
    sup = np.zeros(n)
    den = b[1]
    sup[1] = c[1] / den
    d[:, 1] = r[:, 1] / den
    for i in range(2, n - 1):
        den = b[i] - a[i] * sup[i - 1]
        sup[i] = c[i] / den
        d[:, i] = (r[:, i] - a[i] * d[:, i - 1]) / den
    M = np.zeros_like(y)
    M[:, n - 2] = d[:, n - 2]
    for i in range(n - 3, 0, -1):
        M[:, i] = d[:, i] - sup[i] * M[:, i + 1]
    M[:, 0] = (h[0] + h[1]) / h[1] * M[:, 1] - h[0] / h[1] * M[:, 2]
    M[:, n - 1] = (h[n - 2] + h[n - 3]) / h[n - 3] * M[:, n - 2] - h[n - 2] / h[n - 3] * M[:, n - 3]
    k = np.clip(np.searchsorted(x, xnew, side="right") - 1, 0, n - 2)
    A = (x[k + 1] - xnew) / h[k]
    B = (xnew - x[k]) / h[k]
    return A * y[:, k] + B * y[:, k + 1] + ((A**3 - A) * M[:, k] + (B**3 - B) * M[:, k + 1]) * h[k]**2 / 6.0


# --------------------------------------------------------------------------------------------------------------- trapezoid
_WINDOWS = {"hanning": np.hanning, "hamming": np.hamming, "blackman": np.blackman, "bartlett": np.bartlett}


def trapezoid(dyn_in, freqs, times, window='hanning', window_frac=0.1):
    """trapdyn of dynspec.py:4081-4128.  Line 4126 as the reference means it: `k` trailing zeros (as shipped,
    list(np.zeros(np.shape(indzeros))) is a list of 1-element arrays and line 4127 raises ValueError in current NumPy)."""
    dyn = np.array(dyn_in, dtype=float)                                         # 4082
    dyn -= np.mean(dyn)                                                         # 4083
    nf = np.shape(dyn)[0]                                                       # 4084
    nt = np.shape(dyn)[1]                                                       # 4085
    if window is not None:                                                      # 4086
        fn = _WINDOWS[window]                                                   # 4088-4101
        cw = fn(np.floor(window_frac * nt))
        sw = fn(np.floor(window_frac * nf))
        chan_window = np.insert(cw, int(np.ceil(len(cw) / 2)), np.ones([nt - len(cw)]))        # 4102-4103
        subint_window = np.insert(sw, int(np.ceil(len(sw) / 2)), np.ones([nf - len(sw)]))      # 4104-4105
        dyn = np.multiply(chan_window, dyn)                                     # 4106
        dyn = np.transpose(np.multiply(subint_window, np.transpose(dyn)))       # 4107-4108
    arin = dyn                                                                  # 4109
    scalefrac = 1 / (max(freqs) / min(freqs))                                   # 4111
    timestep = max(times) * (1 - scalefrac) / (nf + 1)                          # 4112
    trapdyn = np.empty(shape=np.shape(arin))                                    # 4113
    for ii in range(0, nf):                                                     # 4114
        idyn = arin[ii, :]                                                      # 4115
        maxtime = max(times) - (nf - (ii + 1)) * timestep                       # 4116
        inddata = np.argwhere(times <= maxtime)                                 # 4118
        indzeros = np.argwhere(times > maxtime)                                 # 4120
        newline = np.interp(np.linspace(min(times), max(times), len(inddata)), times, idyn)    # 4122-4124
        newline = list(newline) + [0.0] * len(indzeros)                         # 4126 (see above)
        trapdyn[ii, :] = newline                                                # 4127
    return trapdyn


def trapezoid_keep(freqs, times):
    """len(inddata) of every row (dynspec.py:4111-4118)."""
    nf = len(freqs)
    scalefrac = 1 / (max(freqs) / min(freqs))
    timestep = max(times) * (1 - scalefrac) / (nf + 1)
    return np.array([len(np.argwhere(times <= max(times) - (nf - (ii + 1)) * timestep)) for ii in range(nf)])
