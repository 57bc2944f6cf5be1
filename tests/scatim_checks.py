"""The checks of Dynspec.calc_scattered_image, shared by the GPU tests (tests/test_gpu_scatim.py) and the host-interpreter tests
(tests/test_scatim_emu_cpu.py).  `D` is scintools_amd.dynspec bound to a GPU or to the interpreter; the expected values come from
the NumPy / SciPy restatement (tests/scatim_oracle.py), which tests/test_scatim_cpu.py pins to the unmodified reference's outputs
(tests/golden/scatim.npz).  Inputs are regenerated from seeds (tests/scatim_cases.py), computed once and shared read-only.

Tolerance.  The interpolant is linear in the data, so per pixel |image - image_oracle| <= K eps S |fdop_y|, S = max |linsspec| over
the cropped plane (the fdop_y = 0 row is therefore exact).  Test fields span at most 1e4 in linear power; the real spectrum uses the
same bound.  K is MEASURED as the worst ratio over all cases and pixels:
  (a) the unmodified reference (goldens) against the oracle:          K_ref = 2.87  (case f; tests/test_scatim_cpu.py prints it)
  (b) the kernels on the host interpreter against the oracle:        K_emu = 4.01  (case f; every check prints its own)
  (c) on an MI355X: printed per case by tests/test_gpu_scatim.py (DESIGN 4j records the value of the last GPU run).
Asserted: K = 32 = four times the larger of (a) and (b) (16.06), rounded up to a power of two (the margin is for libm `pow` differences
between machines).  The axes and the mirror symmetry are exact."""
import functools
import warnings

import numpy as np

import scatim_cases as sc
import scatim_oracle as so

EPS = 2.0 ** -52
K = 32.0

# cropped rows x columns at which the kernels are checked: the k = 3 minimum; small and odd; odd sizes without alignment; a row one
# knot longer than one workgroup's chunk of pass A (2048 interior knots); a row of four chunks (interior warm-ups); more rows than
# one launch's row groups (512 groups of 4 rows)
KERNEL_SHAPES = [(4, 4), (5, 9), (37, 53), (6, 2051), (5, 6200), (2052, 5)]


def ratio(image, ref, lin, fdop_y):
    """Worst |image - ref| / (eps S |fdop_y|) over the pixels with fdop_y > 0; the fdop_y = 0 row must be equal."""
    ny = len(fdop_y)
    fy = np.abs(np.concatenate((fdop_y[:0:-1], fdop_y)))[:, None]
    S = np.max(np.abs(lin))
    assert image.shape == ref.shape == (2 * ny - 1, 2 * ny - 1) and image.dtype == np.float64
    assert np.array_equal(image[ny - 1], ref[ny - 1])
    d = np.abs(image - ref)
    keep = np.arange(2 * ny - 1) != ny - 1
    return float((d[keep] / (EPS * S * fy[keep])).max())


def assert_close(tag, image, ref, lin, fdop_y):
    r = ratio(image, ref, lin, fdop_y)
    print(tag, "measured K", r, "asserted", K)
    assert r <= K
    assert np.array_equal(image, image[::-1, :])                     # the mirrored halves are copies


@functools.lru_cache(maxsize=None)
def screen_spectrum(lamsteps=False):
    """(sspec dB, fdop, tdel) of the seeded screen from the NumPy oracles, read-only."""
    from oracle import arcfit_oracle, sspec_oracle
    s = sc.sim()
    if lamsteps:
        o = arcfit_oracle.calc_sspec_lam(s.dyn, s.freqs, s.dt, s.df)
        out = (o["lamsspec"], o["fdop"], o["tdel"])
    else:
        fdop, tdel, sec = sspec_oracle.calc_sspec(s.dyn, s.dt, s.df)
        out = (sec, fdop, tdel)
    for v in out:
        v.setflags(write=False)
    return out


def case_inputs(case, gold):
    """(sspec, fdop, tdel, eta) the oracle needs for a stored case; eta is the reference's."""
    kw = sc.call_kwargs(case)
    if "input_sspec" in kw:
        sspec, fdop, tdel = kw["input_sspec"], kw["input_fdop"], kw["input_tdel"]
    else:
        sspec, fdop, tdel = screen_spectrum(bool(kw.get("lamsteps")))
    return sspec, fdop, tdel, float(gold[f"{case}_eta"])


@functools.lru_cache(maxsize=None)
def _oracle_case(case, eta, sampling):
    kw = sc.call_kwargs(case)
    if "input_sspec" in kw:
        sspec, fdop, tdel = kw["input_sspec"], kw["input_fdop"], kw["input_tdel"]
    else:
        sspec, fdop, tdel = screen_spectrum(bool(kw.get("lamsteps")))
    out = so.scattered_image(sspec, fdop, tdel, eta=eta, sampling=sampling)
    for v in out:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def oracle_case(case, gold):
    return _oracle_case(case, float(gold[f"{case}_eta"]), sc.CASES[case]["sampling"])


def new_dynspec(D):
    return D.Dynspec(dyn=sc.sim(), verbose=False)


def check_golden(D, gold, case):
    """A stored case through the public method, on the oracle's spectrum and the reference's curvature: the image within the bound
    of the oracle AND of the reference's stored image, the axis bit-equal to the reference's."""
    kw = sc.call_kwargs(case)
    d = new_dynspec(D)
    if "input_sspec" not in kw:
        sspec, fdop, tdel = screen_spectrum(bool(kw.get("lamsteps")))
        d.fdop, d.tdel = np.array(fdop), np.array(tdel)
        if kw.get("lamsteps"):
            d.lamsspec = np.array(sspec)
            d.betaeta = float(gold[f"{case}_betaeta"])               # an existing betaeta is used first
        else:
            d.sspec = np.array(sspec)
            if "input_eta" not in kw and kw.get("fit_arc", True):
                d.eta = float(gold[f"{case}_eta"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        d.calc_scattered_image(**kw)
    o_im, o_ax, o_eta, lin, fdop_y = oracle_case(case, gold)
    assert np.array_equal(d.scattered_image_ax, gold[f"{case}_scattered_image_ax"])
    assert_close(f"{case} vs oracle:", d.scattered_image, o_im, lin, fdop_y)
    assert_close(f"{case} vs reference:", d.scattered_image, gold[f"{case}_scattered_image"], lin, fdop_y)


def _axes(nrow, ncol, uneven):
    if uneven:
        rng = np.random.default_rng(nrow * 1000 + ncol)
        fdop = np.cumsum(0.5 + rng.random(ncol))
        fdop -= 0.5 * (fdop[0] + fdop[-1]) + 0.3                      # not symmetric: the lowest abscissae clamp at fdop[0]
        tdel = np.cumsum(0.2 + rng.random(nrow)) - 0.2
    else:
        fdop = (np.arange(ncol) - ncol // 2) * 0.37
        tdel = np.arange(nrow) * 0.11
    return fdop, tdel


def check_kernel_shape(A, nrow, ncol, uneven=False, offset=(0, 0, 0), sampling=8):
    """scattered_image_device (A = scintools_amd.arcfit) on an nrow x ncol crop of a seeded bounded field against the oracle's
    spline; offset = (row0, col0, extra leading dimension) places the crop inside a larger array (odd origins: unaligned pairs)."""
    import torch
    row0, col0, extra = offset
    lin_db = sc.bounded_field((nrow, ncol), nrow * 7919 + ncol)
    full = sc.bounded_field((nrow + row0 + 1, ncol + col0 + extra), 5)
    full[row0:row0 + nrow, col0:col0 + ncol] = lin_db
    fdop, tdel = _axes(nrow, ncol, uneven)
    eta = 0.6 * tdel[-1] / max(fdop)**2                                # the outer pixels clamp at tdel[-1]
    image, ax = A.scattered_image_device(A.to_device(full, torch.float64), (row0, row0 + nrow), (col0, col0 + ncol), tdel, fdop, eta,
                                         sampling)
    lin = 10**(lin_db / 10)
    ref, ref_ax, fdop_y = so.image_from_crop(lin, tdel, fdop, eta, sampling)
    assert np.array_equal(ax, ref_ax)
    assert_close(f"{nrow} x {ncol}{' uneven' if uneven else ''} {offset}:", image, ref, lin, fdop_y)


def check_on_knots(A):
    """Abscissae exactly on knots and on both ends of both axes: integer knots, eta = 1, fdop_x on every second Doppler knot."""
    import torch
    sampling, nrow = 8, 40
    fdop = np.arange(-16.0, 17.0)                                      # 33 knots: fdop_x = -16, -14, ..., 16
    tdel = np.arange(float(nrow))                                      # delays fx^2 + fy^2 are integers: on knots, or clamped at 39
    db = sc.bounded_field((nrow, 33), 99)
    image, ax = A.scattered_image_device(A.to_device(db, torch.float64), (0, nrow), (0, 33), tdel, fdop, 1.0, sampling)
    lin = 10**(db / 10)
    assert np.array_equal(ax, fdop[::2])
    fy = np.linspace(0, 16, 9)
    for i in range(9):
        for j in range(17):
            t = min(ax[j]**2 + fy[i]**2, tdel[-1])
            if t == int(t):
                exact = lin[int(t), 2 * j] * fy[i]                    # an interpolating spline returns the data on a knot
                assert abs(image[8 + i, j] - exact) <= K * EPS * lin.max() * fy[i], (i, j)
    ref, _, fdop_y = so.image_from_crop(lin, tdel, fdop, 1.0, sampling)
    assert_close("on knots:", image, ref, lin, fdop_y)


def check_neg_inf(A):
    """-inf dB is an exact 0 in linear power and ordinary data."""
    import torch
    db = sc.bounded_field((12, 21), 3)
    db[3, 4] = db[0, 0] = db[11, 20] = db[6, 10:14] = -np.inf
    fdop, tdel = _axes(12, 21, False)
    eta = 0.6 * tdel[-1] / max(fdop)**2
    image, _ = A.scattered_image_device(A.to_device(db, torch.float64), (0, 12), (0, 21), tdel, fdop, eta, 8)
    lin = 10**(db / 10)
    assert np.count_nonzero(lin == 0) == 7 and np.all(np.isfinite(image))
    ref, _, fdop_y = so.image_from_crop(lin, tdel, fdop, eta, 8)
    assert_close("-inf dB:", image, ref, lin, fdop_y)


def check_nonfinite(A):
    """A NaN or +inf pixel anywhere in the crop: scipy's RectBivariateSpline raises nothing and returns NaN everywhere (its solve is
    global); so does the port, from the device-side flag.  A NaN outside the crop changes nothing."""
    import torch
    fdop, tdel = _axes(12, 6200, False)
    eta = 0.6 * tdel[-1] / max(fdop)**2
    clean = sc.bounded_field((12, 6200), 4)
    good, _ = A.scattered_image_device(A.to_device(clean, torch.float64), (0, 12), (0, 6200), tdel, fdop, eta, 8)
    for bad in (np.nan, np.inf):
        db = clean.copy()
        db[7, 5000] = bad                                             # in the last chunk of a row: a blocked solve alone would confine it
        image, _ = A.scattered_image_device(A.to_device(db, torch.float64), (0, 12), (0, 6200), tdel, fdop, eta, 8)
        assert image.shape == (17, 17) and np.all(np.isnan(image))
    db = np.full((14, 6203), np.nan)
    db[1:13, 2:6202] = clean
    image, _ = A.scattered_image_device(A.to_device(db, torch.float64), (1, 13), (2, 6202), tdel, fdop, eta, 8)
    assert np.array_equal(image, good)


def check_deterministic(D):
    """Two calls give equal bits."""
    sspec, fdop, tdel = screen_spectrum()
    d = new_dynspec(D)
    ims = []
    for _ in range(2):
        d.calc_scattered_image(input_sspec=sspec, input_fdop=fdop, input_tdel=tdel, input_eta=0.02, sampling=16, plot_log=False)
        ims.append(d.scattered_image)
    assert ims[0] is not ims[1] and np.array_equal(ims[0], ims[1])


def check_plot_keywords(D, pytest):
    """plot / plot_fit / trap raise; the default plot_log=True warns once and still sets the image; plot_log=False is silent."""
    sspec, fdop, tdel = screen_spectrum()
    d = new_dynspec(D)
    base = dict(input_sspec=sspec, input_fdop=fdop, input_tdel=tdel, input_eta=0.02, sampling=8)
    for bad in ("plot", "plot_fit", "trap"):
        with pytest.raises(NotImplementedError):
            d.calc_scattered_image(**base, **{bad: True})
    assert not hasattr(d, "scattered_image")
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        d.calc_scattered_image(**base)
    assert len(seen) == 1 and "plot" in str(seen[0].message) and d.scattered_image.shape == (17, 17)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        d.calc_scattered_image(**base, plot_log=False, clean=False)
    assert not seen


def check_parked(D):
    """calc_sspec parks the spectrum in device memory; calc_scattered_image uses it in place (it is still parked afterwards) and
    gives the bits of the input_sspec route on the same spectrum as a NumPy array."""
    d = new_dynspec(D)
    d.calc_sspec()
    slot = d.__dict__["_devbacked_sspec"]
    assert slot[0] is None and slot[1] is not None
    d.calc_scattered_image(input_eta=0.02, sampling=8, plot_log=False)
    assert slot[0] is None and slot[1] is not None, "the parked spectrum was copied to the host"
    parked = d.scattered_image
    host = np.array(d.sspec)                                           # reading it hands it to the host
    assert host.shape == (128, 256)
    d.calc_scattered_image(input_sspec=host, input_fdop=d.fdop, input_tdel=d.tdel, input_eta=0.02, sampling=8, plot_log=False)
    assert np.array_equal(parked, d.scattered_image)
    o_im, _, _, lin, fdop_y = so.scattered_image(host, d.fdop, d.tdel, eta=0.02, sampling=8)
    assert_close("parked 128 x 256:", parked, o_im, lin, fdop_y)


def check_chain(D, gold):
    """The default chain in wavelength steps: scale_dyn -> calc_sspec -> fit_arc -> calc_scattered_image, all on the device.  The
    image is checked against the oracle on the device's own spectrum and curvature; the curvature against the reference's."""
    d = new_dynspec(D)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        d.calc_scattered_image(lamsteps=True, sampling=16)
    eta = so.beta_to_eta(d.betaeta, d.freq)
    print("chain: betaeta", d.betaeta, "reference", float(gold["c_betaeta"]))
    assert abs(d.betaeta / float(gold["c_betaeta"]) - 1) <= 1e-6
    o_im, o_ax, _, lin, fdop_y = so.scattered_image(np.array(d.lamsspec), d.fdop, d.tdel, eta=eta, sampling=16)
    assert np.array_equal(d.scattered_image_ax, o_ax)
    assert_close("chain:", d.scattered_image, o_im, lin, fdop_y)


def check_small_axes(D, pytest):
    """Fewer than 4 points on an axis: FITPACK's own error, as scipy raises it for k = 3 (on the seeded screen the reference's
    corner fallback crops to 3 columns and fails this way)."""
    sspec, fdop, tdel = screen_spectrum()
    d = new_dynspec(D)
    with pytest.raises(Exception) as err:
        d.calc_scattered_image(input_sspec=sspec, input_fdop=fdop, input_tdel=tdel, fit_arc=False, sampling=8, plot_log=False)
    assert type(err.value).__name__ == "error" and "my>ky" in str(err.value)
    with pytest.raises(ValueError, match="x dimension of z"):
        d.calc_scattered_image(input_sspec=sspec, input_fdop=fdop, input_tdel=tdel[:-1], input_eta=0.02, plot_log=False)
    with pytest.raises(StopIteration), np.errstate(invalid="ignore"):  # the reference's next(...) finds no Doppler bin
        d.calc_scattered_image(input_sspec=sspec, input_fdop=fdop, input_tdel=tdel, input_eta=np.inf, plot_log=False)
