"""Dynspec.calc_scattered_image restated in NumPy / SciPy (reference dynspec.py:3492-3582): the host lines verbatim in meaning, the
interpolation -- scipy's RectBivariateSpline(tdel, fdop, linsspec).ev(...) with kx = ky = 3, s = 0 -- as the separable evaluation it
is: CubicSpline(bc_type='not-a-knot') along fdop for every row, then along tdel, both arguments clamped to the knots first
(FITPACK's bispev clamps, it does not extrapolate).  Pinned to the unmodified reference's outputs by tests/test_scatim_cpu.py."""
import numpy as np
from scipy.interpolate import CubicSpline


def beta_to_eta(betaeta, freq, ref_freq=1400):
    """dynspec.py:3499-3505."""
    c = 299792458.0
    factor = c * 1e6 / ((ref_freq * 1e6)**2)
    eta = betaeta / (freq / ref_freq)**2
    return eta * factor


def spline_ev(x, y, z, xe, ye):
    """RectBivariateSpline(x, y, z).ev(xe, ye) for xe[ny, nx], ye[ny, nx] = the same row of abscissae in every row."""
    xe = np.clip(xe, x[0], x[-1])
    yrow = np.clip(ye[0], y[0], y[-1])
    assert np.array_equal(np.clip(ye, y[0], y[-1]), np.broadcast_to(yrow, ye.shape))
    a = CubicSpline(y, z, axis=1, bc_type='not-a-knot')(yrow)                 # [len(x), nx]
    out = np.empty(xe.shape)
    for j in range(xe.shape[1]):
        out[:, j] = CubicSpline(x, a[:, j], bc_type='not-a-knot')(xe[:, j])
    return out


def crop(fdop, tdel, eta):
    """dynspec.py:3514-3525: (row slice, column slice, tdel, fdop, flim) -- the flim == 0 branch takes fdop[:tlim] as tdel."""
    nf = len(fdop)
    flim = next(i for i, delay in enumerate(eta * fdop**2) if delay < np.max(tdel))
    if flim == 0:
        tlim = next(i for i, delay in enumerate(tdel) if delay > eta * fdop[0] ** 2)
        return slice(None, tlim), slice(None), fdop[:tlim], fdop, flim
    cols = slice(flim - int(0.02 * nf), nf - flim + int(0.02 * nf))
    return slice(None), cols, tdel, fdop[cols], flim


def scattered_image(sspec, fdop, tdel, eta=None, sampling=64):
    """(scat_im, axis, eta, linsspec_cropped, fdop_y) of the reference; eta=None is its corner fallback."""
    fdop, tdel = np.asarray(fdop, dtype=float), np.asarray(tdel, dtype=float)
    nf, nt = len(fdop), len(tdel)
    linsspec = 10**(np.asarray(sspec) / 10)
    if eta is None:
        eta = tdel[nt - 1] / fdop[nf - 1]**2
    rows, cols, tdel, fdop, _ = crop(fdop, tdel, eta)
    linsspec = linsspec[rows, cols]
    scat_im, fdop_x, fdop_y = image_from_crop(linsspec, tdel, fdop, eta, sampling)
    return scat_im, fdop_x, eta, linsspec, fdop_y


def image_from_crop(linsspec, tdel, fdop, eta, sampling):
    """dynspec.py:3553-3572 on the cropped plane: (scat_im, fdop_x, fdop_y)."""
    nx, ny = 2 * sampling + 1, sampling + 1
    fdop_x = np.linspace(-max(fdop), max(fdop), nx)
    fdop_y = np.linspace(0, max(fdop), ny)
    fdop_x_est, fdop_y_est = np.meshgrid(fdop_x, fdop_y)
    tdel_est = (fdop_x_est**2 + fdop_y_est**2) * eta
    image = spline_ev(tdel, fdop, linsspec, tdel_est, fdop_x_est)
    image = image * fdop_y_est
    scat_im = np.zeros((nx, nx))
    scat_im[ny - 1:nx, :] = image
    scat_im[0:ny - 1, :] = image[ny - 1:0:-1, :]
    return scat_im, fdop_x, fdop_y
