"""NumPy restatement of the reference's brightness-distribution model (scintools/scint_sim.py:768-958, Brightness; Yao et al. 2020)
and of the device's route through it (scintools_amd/csrc/bright.hpp): the reference's double loop over the pixels vectorised, and its
two scipy.interpolate.griddata(method='linear') calls replaced by the piecewise-linear interpolant on a triangulation that is one bit
per grid cell (True = the cell is split along the diagonal from corner (ix, iy) to (ix + 1, iy + 1)).  tests/test_brightness_cpu.py
pins it to the unmodified reference's outputs (tests/golden/brightness_*.npz) with the bitmap scipy's Delaunay gave in the same run,
and its live route to scipy.interpolate.griddata on the local scipy."""
import numpy as np

DEFAULTS = dict(ar=1.0, psi=0, alpha=1.67, thetagx=0, thetagy=0, thetarx=0, thetary=0, df=0.02, dt=0.08, dx=0.1, nf=10, nt=80, nx=30)


def efield(x, ar, psi, alpha):
    """acf_efield (scint_sim.py:843-857)."""
    X, Y = np.meshgrid(x, x)
    R = (ar**2 - 1) / (ar**2 + 1)
    cosa = np.cos(2 * (90 - psi) * np.pi / 180)
    sina = np.sin(2 * (90 - psi) * np.pi / 180)
    a = (1 - R * cosa) / np.sqrt(1 - R**2)
    b = (1 + R * cosa) / np.sqrt(1 - R**2)
    c = -2 * R * sina / np.sqrt(1 - R**2)
    return np.exp(-0.5 * (a * X**2 + b * Y**2 + c * X * Y) ** (alpha / 2))


def bluestein(x, axis):
    """The DFT along `axis` by Bluestein's chirp-z as the device does it: chirp phase pi k^2 / n from k^2 mod 2 n in integers,
    zero-padded to the power of two M >= 2 n - 1 (at least 16), the inverse transform as conj(fft(conj(.))) / M."""
    x = np.moveaxis(np.asarray(x, dtype=np.complex128), axis, -1)
    n = x.shape[-1]
    M = max(16, 1 << int(np.ceil(np.log2(2 * n - 1))))
    k = np.arange(n, dtype=np.int64)
    w = np.exp(-1j * np.pi * ((k * k) % (2 * n)) / n)
    b = np.zeros(M, dtype=np.complex128)
    b[:n] = np.conj(w)
    b[M - n + 1:] = np.conj(w[:0:-1])
    a = np.zeros(x.shape[:-1] + (M,), dtype=np.complex128)
    a[..., :n] = x * w
    y = np.conj(np.fft.fft(np.conj(np.fft.fft(a, axis=-1) * np.fft.fft(b)), axis=-1)) / M
    return np.moveaxis(y[..., :n] * w, -1, axis)


def fft2_bluestein(x):
    return bluestein(bluestein(x, 1), 0)


def brightness(rho, fft2=np.fft.fft2):
    """B (scint_sim.py:867-868): one fftshift and one ifftshift -- they differ on odd lengths."""
    return np.abs(np.fft.ifftshift(fft2(np.fft.fftshift(rho))))


def theta_map(fd, td, thetagx, thetagy, thetarx, thetary, df):
    """thetax, thetay, amp [ntd, nfd] and the branch of every pixel (0: Jacobian, 1: bounded Jacobian, 2: on or outside the arc):
    the loop body of calc_SS (scint_sim.py:911-925), vectorised operation by operation."""
    thetax = np.broadcast_to((fd - thetagx + thetarx)[None, :], (len(td), len(fd))).copy()
    t = thetax + thetagx
    sq = td[:, None] - t * t + thetarx**2 + thetary**2
    pos = sq > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        thym = np.sqrt(np.where(pos, sq, 1.0))
        thetay = np.where(pos, 0.0 + (thym - thetagy), 0.0)
        bounded = pos & (thym < 0.5 * df)
        amp = np.where(pos, np.where(bounded, 2 / df, 1 / thym), 10**(-6))
    branch = np.where(pos, np.where(bounded, 1, 0), 2)
    return thetax, thetay, amp, branch


def cells(x, q):
    """For queries q inside [x[0], x[-1]]: the cell index i with x[i] <= q <= x[i+1] (i <= n - 2)."""
    return np.clip(np.searchsorted(x, q, side="right") - 1, 0, len(x) - 2)


def interp(B, x, qx, qy, diag, twist=False):
    """The piecewise-linear interpolant of B [n, n] (B[iy, ix] at (x[ix], x[iy])) at the queries, NaN outside the grid: barycentric
    weights on the triangle of the cell, in the device's order of operations.  diag: bool [n-1, n-1].  twist=True returns instead
    |B00 + B11 - B01 - B10| / 2 of every query's cell: the most the two diagonals' interpolants can differ by there."""
    qx, qy = np.asarray(qx, dtype=np.float64), np.asarray(qy, dtype=np.float64)
    inside = (qx >= x[0]) & (qx <= x[-1]) & (qy >= x[0]) & (qy <= x[-1])
    sx, sy = np.where(inside, qx, x[0]), np.where(inside, qy, x[0])
    ix, iy = cells(x, sx), cells(x, sy)
    u = (sx - x[ix]) / (x[ix + 1] - x[ix])
    v = (sy - x[iy]) / (x[iy + 1] - x[iy])
    b00, b10, b01, b11 = B[iy, ix], B[iy, ix + 1], B[iy + 1, ix], B[iy + 1, ix + 1]
    if twist:
        return np.where(inside, np.abs(b00 + b11 - b01 - b10) / 2, np.nan)
    m = diag[iy, ix]
    main = np.where(u >= v, ((1.0 - u) * b00 + (u - v) * b10) + v * b11, ((1.0 - v) * b00 + (v - u) * b01) + u * b11)
    anti = np.where(u + v <= 1.0, (((1.0 - u) - v) * b00 + u * b10) + v * b01,
                    ((1.0 - v) * b10 + (1.0 - u) * b01) + ((u + v) - 1.0) * b11)
    return np.where(inside, np.where(m, main, anti), np.nan)


def fold(SS0):
    """SS[1:, 1:] += flip(flip(SS[1:, 1:])) (scint_sim.py:947-948) out of place, and LSS."""
    SS = SS0.copy()
    SS[1:, 1:] += SS0[:0:-1, :0:-1]
    with np.errstate(invalid="ignore", divide="ignore"):
        return SS, 10 * np.log10(SS)


def acf_of(SS, fft2=np.fft.fft2):
    """calc_acf (scint_sim.py:953-958): fftshift twice; np.max is NaN if any element is."""
    acf = np.real(np.fft.fftshift(fft2(np.fft.fftshift(SS))))
    with np.errstate(invalid="ignore"):
        return acf / np.max(acf)


def qhull_diagonals(x):
    """The bitmap of the triangulation griddata(method='linear') builds on this scipy (the package's own conversion, which checks that
    every simplex lies in one cell and every cell holds two)."""
    from scintools_amd.scint_sim import qhull_diagonals as q
    return q(x)


def model(diagonals="main", use_griddata=False, fft2=np.fft.fft2, **kw):
    """Every array of the model as a dict.  diagonals: 'main', 'qhull' or a bool [n-1, n-1] array.  use_griddata: the two interpolations
    are scipy.interpolate.griddata calls, exactly the reference's lines (scint_sim.py:933-938)."""
    p = dict(DEFAULTS, **kw)
    x = np.arange(-p["nx"], p["nx"], p["dx"])
    n = len(x)
    rho = efield(x, p["ar"], p["psi"], p["alpha"])
    B = brightness(rho, fft2)
    fd = np.arange(-p["nf"], p["nf"], p["df"])
    td = np.arange(-p["nt"], p["nt"], p["dt"])
    thetax, thetay, amp, branch = theta_map(fd, td, p["thetagx"], p["thetagy"], p["thetarx"], p["thetary"], p["df"])
    if use_griddata:
        from scipy.interpolate import griddata
        X, Y = np.meshgrid(x, x)
        pts = (np.ravel(X), np.ravel(Y))
        up = griddata(pts, np.ravel(B), (np.ravel(thetax), np.ravel(thetay)), method="linear").reshape(thetax.shape)
        dn = griddata(pts, np.ravel(B), (np.ravel(thetax), np.ravel(-thetay)), method="linear").reshape(thetax.shape)
        diag = None
    else:
        if isinstance(diagonals, str):
            diag = np.ones((n - 1, n - 1), dtype=bool) if diagonals == "main" else qhull_diagonals(x)
        else:
            diag = np.asarray(diagonals, dtype=bool)
        up, dn = interp(B, x, thetax, thetay, diag), interp(B, x, thetax, -thetay, diag)
    SS0 = up * amp + dn * amp
    SS, LSS = fold(SS0)
    env0 = (interp(B, x, thetax, thetay, None, twist=True) + interp(B, x, thetax, -thetay, None, twist=True)) * amp
    env = env0.copy()
    env[1:, 1:] += env0[:0:-1, :0:-1]
    return dict(x=x, acf_efield=rho, B=B, fd=fd, td=td, thetax=thetax, thetay=thetay, jacobian=amp, branch=branch, SS0=SS0, SS=SS,
                LSS=LSS, acf=acf_of(SS, fft2), diagonals=diag, envelope=env)


def boundary_margin(x, thetax, thetay):
    """The smallest distance, in grid steps, of a query (thetax, +-thetay) from the outer boundary of the grid (either side of it)."""
    dx = (x[-1] - x[0]) / (len(x) - 1)
    d = [np.abs(q - e).min() for q in (thetax, thetay, -thetay) for e in (x[0], x[-1])]
    return min(d) / dx
