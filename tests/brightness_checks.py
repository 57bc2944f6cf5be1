"""The checks of the brightness-distribution model, shared by the GPU tests (tests/test_gpu_brightness.py) and the host-interpreter
tests (tests/test_brightness_emu_cpu.py): `S` is scintools_amd.scint_sim bound to a GPU or to the interpreter, the goldens are the
unmodified reference's outputs (tests/golden/brightness_<case>.npz, with the Delaunay bitmap of the same run), the oracle is
tests/brightness_oracle.py.  A model is computed once per backend and shared, read-only; so is the oracle's.

Tolerances
  fft2_any   1e-13 of the output's peak magnitude against np.fft.fft2: the level the existing FFT tests hold (tests/test_gpu_edges.py
             sets no other figure for the power-of-two transform).
  jacobian, thetax, thetay   1e-15 relative: the loop body is restated operation by operation.
  B, SS, acf   relative to each golden array's peak.  MEASURED on the CPU (tests/test_brightness_cpu.py asserts it): the oracle, with the
             stored bitmap and every transform through its Bluestein restatement (the route the device takes; with np.fft.fft2 its B
             IS the golden's, which says nothing about a transform), deviates from the goldens by at most ORACLE_DEV = 4.5e-16 (B),
             6.6e-16 (SS), 3.4e-16 (acf) over all cases.  The device gets ten times that (TOL): the margin covers the other summation
             order of its transforms and its barycentric arithmetic.  The yardstick is the reference's golden, never a device output.
             What the kernels reach against the goldens: 4.7e-16 / 5.9e-16 / 2.2e-16 on an MI355X (profiles/brightness_gpu.txt, written
             by tests/tools/time_brightness.py), 4.7e-16 / 4.7e-16 / 3.3e-16 on the host interpreter."""
import numpy as np

import brightness_cases as bc
import brightness_oracle as bo

FFT_TOL = 1e-13
THETA_RTOL = 1e-15
ORACLE_DEV = {"B": 4.5e-16, "SS": 6.6e-16, "acf": 3.4e-16}
TOL = {k: 10 * v for k, v in ORACLE_DEV.items()}
FFT_SHAPES = ((30, 50), (61, 75), (32, 64), (4093, 16))

_runs = {}


def run(S, backend, case, mode):
    """Brightness of a case on this backend: mode 'golden' (diagonals from the golden file), 'qhull' or 'main'.  Computed once."""
    key = (backend, case, mode)
    if key not in _runs:
        kw = bc.kwargs(case)
        if mode == "golden":
            kw["diagonals"] = load_golden(case)["diagonals"]
        else:
            kw["triangulation"] = mode
        b = S.Brightness(**kw)
        out = {k: np.array(getattr(b, k)) for k in bc.ARRAYS + ("LSS", "acf_efield", "x", "fd", "td")}
        for v in out.values():
            v.setflags(write=False)
        _runs[key] = out
    return _runs[key]


_gold = {}


def load_golden(case):
    import os
    if case not in _gold:
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"brightness_{case}.npz")) as f:
            _gold[case] = {k: f[k] for k in f.files}
    return _gold[case]


def peak_dev(a, ref):
    """max |a - ref| over the non-NaN elements of ref, relative to ref's peak magnitude (NaN if ref is all NaN)."""
    if np.isnan(ref).all():
        return np.nan
    return float(np.nanmax(np.abs(a - ref)) / np.nanmax(np.abs(ref)))


def check_fft2_any(S, shape, seed=0):
    """1. scint_fft2_any against np.fft.fft2: complex input, real input (flag), and the shifted forms the model uses."""
    rng = np.random.default_rng(seed)
    R, C = shape
    z = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    x = rng.standard_normal(shape)
    ref_z, ref_x = np.fft.fft2(z), np.fft.fft2(x)
    got_z, got_x = S.fft2_any(z).cpu().numpy(), S.fft2_any(x).cpu().numpy()
    dz, dx = np.abs(got_z - ref_z).max() / np.abs(ref_z).max(), np.abs(got_x - ref_x).max() / np.abs(ref_x).max()
    print(shape, "fft2_any: complex", dz, "real", dx, "of the peak; asserted", FFT_TOL)
    assert got_z.shape == shape and got_z.dtype == np.complex128 and dz <= FFT_TOL and dx <= FFT_TOL
    ref_b = np.abs(np.fft.ifftshift(np.fft.fft2(np.fft.fftshift(x))))
    got_b = S.fft2_any(x, in_shift="fftshift", out_shift="ifftshift", out="abs").cpu().numpy()
    ref_a = np.real(np.fft.fftshift(np.fft.fft2(np.fft.fftshift(x))))
    got_a = S.fft2_any(x, in_shift="fftshift", out_shift="fftshift", out="real").cpu().numpy()
    db, da = np.abs(got_b - ref_b).max() / ref_b.max(), np.abs(got_a - ref_a).max() / np.abs(ref_x).max()
    print(shape, "shifted: abs", db, "real", da)
    assert got_b.dtype == np.float64 and db <= FFT_TOL and da <= FFT_TOL


def check_golden(S, backend, case):
    """2. Every array against the reference's, with the reference's triangulation."""
    g = load_golden(case)
    r = run(S, backend, case, "golden")
    for k in ("SS", "acf"):
        assert np.array_equal(np.isnan(r[k]), np.isnan(g[k])), f"{case}: the NaN mask of {k} differs"
    for k in ("jacobian", "thetax", "thetay"):
        assert r[k].shape == g[k].shape
        np.testing.assert_allclose(r[k], g[k], rtol=THETA_RTOL, atol=0, err_msg=f"{case} {k}")
    for k in ("B", "SS", "acf"):
        d = peak_dev(r[k], g[k])
        print(case, k, "deviation / peak", d, "asserted", TOL[k])
        assert r[k].shape == g[k].shape and (np.isnan(d) or d <= TOL[k]), (case, k, d)
    with np.errstate(invalid="ignore", divide="ignore"):                 # LSS is 10 log10 of the SS beside it (one rounding of log10)
        np.testing.assert_allclose(r["LSS"], 10 * np.log10(r["SS"]), rtol=0, atol=1e-12, equal_nan=True)


def check_qhull(S, backend, case):
    """3. triangulation='qhull' against the oracle's live scipy.interpolate.griddata route on this machine."""
    o = bo.model(use_griddata=True, **bc.kwargs(case))
    r = run(S, backend, case, "qhull")
    assert np.array_equal(np.isnan(r["SS"]), np.isnan(o["SS"]))
    for k in ("B", "SS", "acf"):
        d = peak_dev(r[k], o[k])
        print(case, "qhull", k, "deviation / peak", d)
        assert np.isnan(d) or d <= TOL[k], (case, k, d)


def check_main(S, backend, case):
    """4. triangulation='main' against the oracle with the main diagonal, and inside the two-triangulation envelope of the golden:
    per interpolated value the two diagonals differ by at most |B00 + B11 - B01 - B10| / 2 of the cell; the oracle carries that through
    the Jacobian, the two-term sum and the fold."""
    g = load_golden(case)
    o = bc.build(case)
    r = run(S, backend, case, "main")
    assert np.array_equal(np.isnan(r["SS"]), np.isnan(o["SS"]))
    for k in ("B", "SS", "acf"):
        d = peak_dev(r[k], o[k])
        print(case, "main", k, "deviation / peak", d)
        assert np.isnan(d) or d <= TOL[k], (case, k, d)
    ok = ~np.isnan(g["SS"])
    excess = np.abs(r["SS"] - g["SS"])[ok] - (o["envelope"][ok] + TOL["SS"] * np.nanmax(np.abs(g["SS"])))
    print(case, "main vs golden: max |diff|", np.abs(r["SS"] - g["SS"])[ok].max(), "worst excess over the envelope", excess.max())
    assert np.all(excess <= 0)


def check_errors(S, pytest):
    """5. A grid axis of 4097 points, a transform axis of 4097 and a bitmap of the wrong shape raise ValueError; plots only warn."""
    import warnings
    with pytest.raises(ValueError, match="4096"):
        S.Brightness(nx=4097 / 16, dx=0.125)
    with pytest.raises(ValueError, match="4096"):
        S.fft2_any(np.zeros((4097, 16)))
    with pytest.raises(ValueError, match="diagonals"):
        S.Brightness(**dict(bc.kwargs("a"), diagonals=np.ones((30, 30), dtype=bool)))
    with pytest.raises(ValueError):
        S.Brightness(triangulation="delaunay")
    with pytest.raises(ValueError, match="one grid cell"):
        S.diagonals_from_simplices(np.array([[0, 1, 8]]), 4)
    with pytest.raises(ValueError, match="two simplices"):
        S.diagonals_from_simplices(np.array([[0, 1, 4]]), 4)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        b = S.Brightness(**dict(bc.kwargs("e"), triangulation="main", plot=True))
        b.plot_cuts()
    assert len(seen) == 6
    assert b.X.shape == b.Y.shape == (24, 24) and np.array_equal(b.X[0], b.x)


def check_deterministic(S, case="d"):
    """6. The same case twice: identical bits."""
    kw = dict(bc.kwargs(case), triangulation="main")
    a, b = S.Brightness(**kw), S.Brightness(**kw)
    for k in bc.ARRAYS + ("LSS", "acf_efield"):
        assert np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True), k
