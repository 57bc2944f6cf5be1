"""Seeded geometry for the fitted-mosaic tests (rotMos / rotFit / rotDer / rotInit, fullMos / fullMosFit / fullMosGrad /
fullMosHess): a random complex field cut into half-overlapping windows, each window with a random phase and an amplitude in
[0.5, 2] plus complex noise; the dynamic spectrum is |field|^2 with 10 % noise, its noise map a constant."""
import numpy as np

# (ncf, nct, cwf, cwt)
SHAPES = [
    (1, 1, 8, 8),       # one chunk: empty x
    (2, 2, 2, 2),       # tapers of length 1
    (2, 1, 6, 5),       # odd size on an axis of one chunk
    (1, 3, 7, 8),
    (3, 3, 8, 12),      # one chunk with all eight neighbours
    (2, 3, 34, 50),     # windows that are no multiple of a wavefront or a workgroup
    (9, 9, 4, 6),       # 81 chunks: past the 64 chunks a launch of mosaic_device takes
    (5, 5, 32, 32),
]
GOLDEN_SHAPES = SHAPES[:-1]                      # stored in tests/golden/rotmos.npz (all but the largest)
DRIVER_SHAPE = (4, 5, 16, 16)


def name_of(shape):
    return "s" + "x".join(str(v) for v in shape)


def extent(shape):
    ncf, nct, cwf, cwt = shape
    return (ncf - 1) * (cwf // 2) + cwf, (nct - 1) * (cwt // 2) + cwt


def case(shape, seed=0, noise=0.1, nans=False):
    """dict(chunks [ncf, nct, cwf, cwt], dspec [F, T], N [F, T], x [n - 1], p [2 n - 1])"""
    ncf, nct, cwf, cwt = shape
    F, T = extent(shape)
    rng = np.random.default_rng(1000 * seed + 17 * ncf + 5 * nct + 3 * cwf + cwt)
    field = rng.standard_normal((F, T)) + 1j * rng.standard_normal((F, T))
    chunks = np.empty(shape, dtype=complex)
    for cf in range(ncf):
        for ct in range(nct):
            win = field[cf * (cwf // 2): cf * (cwf // 2) + cwf, ct * (cwt // 2): ct * (cwt // 2) + cwt]
            amp, phase = rng.uniform(0.5, 2.0), rng.uniform(-np.pi, np.pi)
            chunks[cf, ct] = amp * np.exp(1j * phase) * win + noise * (rng.standard_normal((cwf, cwt)) + 1j * rng.standard_normal((cwf, cwt)))
    dspec = np.abs(field) ** 2 * (1 + 0.1 * rng.standard_normal((F, T)))
    N = np.full((F, T), 0.5)
    n = ncf * nct
    x = rng.uniform(-np.pi, np.pi, n - 1)
    p = np.concatenate((x, rng.uniform(0.5, 2.0, n)))
    if nans:
        # a few NaNs in dspec, one NaN and one zero in N -- in pixels that several chunks share: where a chunk is alone,
        # y conj(W) is real up to rounding, and the SIGN of the infinity that a zero of N makes of its imaginary part is noise
        inner = np.zeros((F, T), dtype=bool)
        inner[cwf // 2: F - cwf // 2, cwt // 2: T - cwt // 2] = True
        flat = rng.permutation(np.flatnonzero(inner))
        for q in flat[:3]:
            dspec[q // T, q % T] = np.nan
        N[flat[3] // T, flat[3] % T] = np.nan
        N[flat[4] // T, flat[4] % T] = 0.0
    return dict(shape=shape, chunks=chunks, dspec=dspec, N=N, x=x, p=p)


def neighbour_band(shape):
    """Boolean [2 n - 1, 2 n - 1]: the entries of fullMosHess that a pair of neighbouring chunks (or one chunk) can fill."""
    ncf, nct = shape[:2]
    n = ncf * nct
    band = np.zeros((2 * n - 1, 2 * n - 1), dtype=bool)
    for a in range(n):
        for b in range(n):
            if abs(a // nct - b // nct) <= 1 and abs(a % nct - b % nct) <= 1:
                ia, ib = [a + n - 1] + ([a - 1] if a else []), [b + n - 1] + ([b - 1] if b else [])
                for i in ia:
                    for j in ib:
                        band[i, j] = True
    return band


def close_in_scale(got, want, scale, tol, product_scale=None):
    """|got - want| <= tol * scale where both are finite; elsewhere the same infinity or both NaN.  Returns the worst error in
    units of the bound.  `product_scale` (tests/rotmos_oracle.py: P): where the scale itself has fallen to rounding level
    (scale < 1e-6 P: whole summands have cancelled) the bound gains the rounding floor 8 eps P; everywhere else it is tol * scale."""
    got, want, scale = np.atleast_1d(got), np.atleast_1d(want), np.atleast_1d(scale)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), "finite pattern differs"
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN pattern differs"
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), "infinities differ"
    if not fin.any():
        return 0.0
    # (a finite sum whose scale is not finite cannot occur: a term of infinite magnitude makes the sum non-finite)
    assert np.all(np.isfinite(scale[fin]))
    bound = tol * np.where(fin, scale, 0.0)
    if product_scale is not None:
        P = np.where(fin, np.atleast_1d(product_scale), 0.0)
        bound = bound + np.where(np.where(fin, scale, 0.0) < 1e-6 * P, 8 * np.finfo(float).eps * P, 0.0)
    err = np.abs(np.where(fin, got - want, 0.0))
    assert np.all(err <= bound), f"error {float((err - bound).max()):.3e} above the bound; worst error / scale {float((err[fin] / np.where(scale[fin] > 0, scale[fin], 1.0)).max()):.3e}"
    return float((err[fin] / np.where(scale[fin] > 0, scale[fin], np.inf)).max())
