"""The checks of the theoretical 2-D ACF model, shared by the GPU tests (tests/test_gpu_acf.py) and the host-interpreter tests
(tests/test_acf_emu_cpu.py): `S` is scintools_amd.scint_sim bound to a GPU or to the interpreter, `gold` the unmodified reference's
outputs (tests/golden/acf.npz, tests/golden/make_golden_acf.py), the complex field comes from the direct-sum restatement
(tests/acf_oracle.py, pinned bit for bit to the goldens by tests/test_acf_cpu.py).  A case is computed once per backend and shared,
read-only; so is the oracle's result.

Tolerances
  field     |gamma_dev - gamma_ref| <= delta = K eps S per lag, S = step^2 sum(G) / (2 pi dnun[idn]): the value the sum would have if
            every phase were zero (the rounding scale).  K is MEASURED as the worst ratio over every case, lag and sample against the
            oracle: 2.44 on the host interpreter (ACF(ar=3) at the default size, the case of tests/test_gpu_acf.py with the
            full-size core grid, run there through --emu; 1.77 over the cases a-g, case a the worst); on an MI355X: NOT MEASURED
            (no GPU run was available), so the assertion rests on the interpreter's value; the NumPy restatement of the
            factorisation reached 2.1.  Asserted: K = 16, four times the larger measured value (9.8) rounded up to a power of two
            (the margin is for libm differences between machines).
  acf       follows from it: |d acf| <= amp (2 sqrt(acf_ref / amp) delta + delta^2); the dnun = 0 row is host NumPy and must be equal.
  acf_efield  |dG| <= 8 eps (1 + u / 2) G with u = ((x / sqrt(ar))^2 + (y sqrt(ar))^2)^(alpha / 2): about five roundings in u,
            amplified by the exponent, and the exp itself.
  fn, tn, sn, snp and every scalar attribute: equal.
  scint_acf_model_2d   the acf bound times |weights * triangle|.  (This bound carries no term for the roundings of
            (ydata - model) * weights itself: where it falls below the spacing of the residual -- 1.0e-16 against 1.1e-16 at one pixel
            of case a with K = 8 -- a model inside its bound can move the residual by one spacing.  With K = 16 no pixel of the two
            stored cases is that close: worst |diff| 1.1e-16 against 2.0e-16 there.)"""
import functools

import numpy as np

import acf_cases as ac
import acf_oracle as ao

EPS = 2.0 ** -52
K = 16.0

_runs = {}


def run(S, backend, case):
    """The model of a case on this backend ('gpu' / 'emu'): computed once, arrays read-only."""
    key = (backend, case)
    if key not in _runs:
        a = S.ACF(**ac.kwargs(case))
        for v in vars(a).values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _runs[key] = a
    return _runs[key]


@functools.lru_cache(maxsize=None)
def _oracle_frozen(items):
    o = ao.acf_model(**dict(items))
    for v in o.values():
        v.setflags(write=False)
    return o


def oracle(**kw):
    return _oracle_frozen(tuple(sorted(kw.items())))


def acf_tolerance(o, amp):
    """Bound on |acf - acf_ref| [nf, nt] from delta = K eps S of each lag (zero on the dnun = 0 row)."""
    ndnun = len(o["dnun"])
    delta = K * EPS * np.abs(o["scale"])
    rows = np.concatenate((delta[:0:-1], delta))               # the lags of acf's rows: -dnumax .. 0 .. dnumax
    assert rows.shape[0] == 2 * ndnun - 1 == o["acf"].shape[0]
    d = rows[:, None]
    return amp * (2 * np.sqrt(o["acf"] / amp) * d + d ** 2)


def check_golden(S, backend, gold, case):
    """1. acf against the reference's, the dnun = 0 row, the axes and the scalars equal;  2. acf_efield within its bound."""
    a = run(S, backend, case)
    kw = ac.kwargs(case)
    o = oracle(**kw)
    g = {k: gold[f"{case}_{k}"] for k in ac.ARRAYS + ac.SCALARS}
    amp = kw.get("amp", 1)
    assert a.acf.shape == g["acf"].shape and a.acf.dtype == np.float64
    tol = acf_tolerance(o, amp)
    diff = np.abs(a.acf - g["acf"])
    mid = (g["acf"].shape[0] - 1) // 2
    with np.errstate(divide="ignore", invalid="ignore"):
        print(case, "acf: max |diff|", diff.max(), "worst diff / bound", np.nanmax(np.where(tol > 0, diff / tol, np.nan)))
    assert np.all(diff <= tol)
    assert np.array_equal(a.acf[mid], g["acf"][mid])
    for k in ("fn", "tn", "sn", "snp"):
        assert np.array_equal(getattr(a, k), g[k]), k
    for k in ac.SCALARS:
        assert getattr(a, k) == g[k][()], (k, getattr(a, k), g[k][()])
    # acf_efield
    G = g["acf_efield"]
    X, Y = np.meshgrid(g["snp"], g["snp"])
    sqrtar = np.sqrt(kw.get("ar", 1))
    u = ((X / sqrtar) ** 2 + (Y * sqrtar) ** 2) ** (kw.get("alpha", 5 / 3) / 2)
    bound = 8 * EPS * (1 + u / 2) * G
    dG = np.abs(a.acf_efield - G)
    print(case, "acf_efield: worst diff / bound", (dG / bound).max(), "max ulp", (dG / np.spacing(G)).max())
    assert a.acf_efield.shape == G.shape and np.all(dG <= bound)


def field_ratio(a, o):
    """Worst |gamma - gamma_ref| / (eps S) over the lags >= 1: the measured K of this case."""
    d = np.abs(a.gammitv - o["field"])[:, 1:]
    return float((d / (EPS * np.abs(o["scale"][1:]))).max())


def check_field(S, backend, case):
    """3. The complex field against the oracle's direct sums, within delta; its dnun = 0 column is host NumPy: equal."""
    a = run(S, backend, case)
    o = oracle(**ac.kwargs(case))
    r = field_ratio(a, o)
    print(case, "field: measured K", r, "asserted", K)
    assert a.gammitv.shape == o["field"].shape and r <= K
    assert np.array_equal(a.gammitv[:, 0], o["field"][:, 0])


def check_symmetry(S, backend, case):
    """4. Without a phase gradient the ACF equals both its flips, with one its point mirror -- exactly."""
    a = run(S, backend, case)
    if ac.kwargs(case).get("phasegrad", 0) == 0:
        assert np.array_equal(a.acf, a.acf[::-1, :]) and np.array_equal(a.acf, a.acf[:, ::-1])
    else:
        assert np.array_equal(a.acf, a.acf[::-1, ::-1])


def check_deterministic(S):
    """5. Two calls with the same arguments: identical bits."""
    for case in ("b", "c"):
        a, b = S.ACF(**ac.kwargs(case)), S.ACF(**ac.kwargs(case))
        assert np.array_equal(a.gammitv, b.gammitv) and np.array_equal(a.acf, b.acf) and np.array_equal(a.acf_efield, b.acf_efield)
        a.calc_acf()
        assert np.array_equal(a.acf, b.acf)


def model_kwargs(pars, shape):
    """The ACF arguments scint_acf_model_2d derives from its parameters (scint_models.py:171-192)."""
    nf_crop, nt_crop = shape
    dt, df = 2 * pars["tobs"] / pars["nt"], 2 * pars["bw"] / pars["nf"]
    return dict(taumax=nt_crop * dt / np.abs(pars["tau"]), dnumax=nf_crop * df / np.abs(pars["dnu"]), nt=nt_crop, nf=nf_crop,
                ar=np.abs(pars["ar"]), alpha=pars["alpha"], phasegrad=pars["phasegrad"], theta=pars["theta"], amp=pars["amp"],
                psi=pars["psi"])


def check_model_2d(M, gold, case):
    """6. scint_acf_model_2d (M = scintools_amd.scint_models) against the reference's stored residual."""
    pars, ydata, weights = ac.model_inputs(case)
    ref = gold[f"{case}_resid"]
    keep = weights.copy()
    got = M.scint_acf_model_2d(ac.Params(pars), ydata, weights)
    assert np.array_equal(M.scint_acf_model_2d(pars, ydata, keep.copy()), got)      # a plain mapping is accepted too
    o = oracle(**model_kwargs(pars, ydata.shape))
    _, triangle, w, _ = ao.scint_acf_model_2d(pars, ydata, keep.copy(), o["acf"])
    tol = acf_tolerance(o, pars["amp"]) * np.abs(w * triangle)
    diff = np.abs(got - ref)
    print(case, "residual: max |diff|", diff.max(), "of", tol.max())
    assert got.shape == ref.shape and np.all(diff <= tol)
    nf_crop, nt_crop = ydata.shape
    assert got[nf_crop // 2, nt_crop // 2] == 0                                    # the white-noise pixel carries no weight


def check_errors(S, pytest):
    import warnings
    with pytest.raises(IndexError):                 # dnun has one element: dnun[1]
        S.ACF(nf=1)
    with pytest.raises(ZeroDivisionError):          # dsp = 4 taumax / (nt - 1)
        S.ACF(nt=1)
    # 2 is made odd before either line (confirmed on the unmodified reference: ACF(nf=2).acf is 3 x 51, ACF(nt=2).acf 51 x 3)
    small, same = S.ACF(nf=2, nt=2), S.ACF(nf=3, nt=3)
    assert small.acf.shape == (3, 3) and (small.nf, small.nt) == (3, 3) and np.array_equal(small.acf, same.acf)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        a = S.ACF(nf=3, nt=5, plot=True)
        a.plot_acf_efield()
        a.plot_sspec()
    assert len(seen) == 3


def check_sspec(S, backend, case="a"):
    """calc_sspec is the reference's NumPy lines on the model array: finite, the shape of acf, its peak at the centre."""
    a = run(S, backend, case)
    b = S.ACF.__new__(S.ACF)
    b.acf = a.acf
    b.calc_sspec(window="hanning", window_frac=1)
    nf, nt = a.acf.shape
    assert b.sspec.shape == (nf, nt) and np.all(np.isfinite(b.sspec))
    assert np.unravel_index(np.argmax(b.sspec), b.sspec.shape) == (nf // 2, nt // 2)
