"""The checks of the cleaning methods, shared by the host-interpreter run (tests/test_clean_emu_cpu.py) and the GPU run
(tests/test_gpu_clean.py).  `D` is the scintools_amd.dynspec module in force (patched onto the interpreter, or on a GPU).  Every
tolerance check prints the K it measured before it asserts.

Tolerances
----------
* zap, refill('median'), the mean fill, trim_edges, crop_dyn: the same bits as the reference (NaN where it has NaN).
* refill('linear'): |got - ref| <= K eps max(|v0|, |v1|) of the bracketing valid values.  The NumPy restatement itself is within
  K_LINEAR_ORACLE = 0.97 of the reference's griddata on the stored cases (tests/test_clean_cpu.py measures and asserts this:
  0.924, 0.965, 0.924 measured, the largest rounded up to two digits); the limit is four times that.
* correct_dyn(svd=True), svd_model: the error of |model| relative to max|model| is held to
  bound = SVD_ROUNDINGS * SVD_TOL / relgap, from the singular values s of the decomposed array (the stored ones for the stored
  cases), relgap = 1 - (s[nmodes] / s[nmodes-1])**2.  The iteration stops when |A^T A V - V H|_F <= SVD_TOL lambda_p
  (csrc/clean.hpp); by the Davis-Kahan sin-theta theorem the subspace is then within sin(theta) <= SVD_TOL lambda_p /
  (lambda_p - lambda_(p+1)) = SVD_TOL / relgap of the true one, which is the relative size of model - model_true = A (P - P_true).
  SVD_ROUNDINGS = 2: one for that bound, one for what it leaves out -- the host sees the residual of the basis before the last
  step's Gram-Schmidt pass, and both models carry the float64 rounding of an nt-term dot product (sqrt(nt) eps < 1e-14, a
  hundredth of SVD_TOL).  The corrected array a / |model| is mapped back to model units (|d corrected| model^2 / |a|) and held to
  the same bound.
* correct_dyn(svd=False): |got - ref| <= 4 (nf + nt) eps |ref| for the array, 4 nt eps |ref| for the bandpass (a mean of nt terms).  A mean of n positive terms summed in any order is within
  (n - 1) eps/2 of the exact one relatively, so two different orders differ by at most (n - 1) eps, a divide adds eps/2: the
  bandpass within nt eps, the divided array within (nt + 1) eps, the time mean of those within (nt + 1 + nf) eps, the second divide
  within (nt + nf + 2) eps; savgol_filter(window, 1) is a moving average with positive weights except at the ends, where its
  linear extrapolation weights sum in absolute value to < 2: a factor 2, and 2 (nf + nt + 2) <= 4 (nf + nt).  Data are positive.
"""
import io
from contextlib import redirect_stdout

import numpy as np

import clean_cases as cc
import clean_oracle as co

EPS = np.finfo(float).eps
K_LINEAR_ORACLE = 0.97
K_LINEAR_LIMIT = 4 * K_LINEAR_ORACLE
SVD_ROUNDINGS = 2.0


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def quiet(fn, *args, **kw):
    with redirect_stdout(io.StringIO()) as out:
        res = fn(*args, **kw)
    return res, out.getvalue()


# ---------------------------------------------------------------------------- tolerance checks
def assert_linear(label, got, ref, before):
    """`before`: the array refill interpolated (zeros already NaN)."""
    scale = co.brackets(before)
    gap = scale > 0
    assert same_bits(got[~gap & co.valid(before)], ref[~gap & co.valid(before)]), f"{label}: a valid pixel changed"
    k = np.max(np.abs(got - ref)[gap] / (EPS * scale[gap])) if gap.any() else 0.0
    edge = ~gap & ~co.valid(before)                      # no bracket: the mean of the valid and the interpolated pixels
    ke = np.max(np.abs(got - ref)[edge] / (EPS * np.abs(ref[edge]))) if edge.any() else 0.0
    print(f"{label}: K = {k:.3f} (limit {K_LINEAR_LIMIT}), mean-filled edge pixels K = {ke:.3f}")
    assert np.isfinite(got).all() and k <= K_LINEAR_LIMIT and ke <= K_LINEAR_LIMIT


def svd_bound(s, nmodes):
    from scintools_amd import clean
    s = np.asarray(s, dtype=float)
    relgap = 1.0 if nmodes >= len(s) or s[nmodes - 1] == 0 else 1.0 - (s[nmodes] / s[nmodes - 1]) ** 2
    return SVD_ROUNDINGS * clean.SVD_TOL / relgap, relgap


def assert_svd(label, s, nmodes, a, model, model_ref, corrected=None, corrected_ref=None):
    mm = np.max(np.abs(model_ref))
    bound, relgap = svd_bound(s, nmodes)
    err = np.max(np.abs(np.abs(model) - np.abs(model_ref))) / mm
    msg = f"{label}: relgap {relgap:.3f}, bound {bound:.3g}, |model| error {err:.3g} (K = {err / bound:.3g})"
    ok = err <= bound
    if corrected is not None:
        fin = np.isfinite(corrected_ref) & (a != 0)
        assert same_bits(np.isfinite(corrected), np.isfinite(corrected_ref))
        errc = np.max(np.abs(corrected - corrected_ref)[fin] * np.abs(model_ref[fin]) ** 2 / np.abs(a[fin])) / mm
        msg += f", corrected error {errc:.3g} (K = {errc / bound:.3g})"
        ok = ok and errc <= bound
    print(msg)
    assert ok, msg


def assert_nosvd(label, got, ref, terms):
    """`terms`: the number of summed terms behind every element (nt for the bandpass, nf + nt for the corrected array)."""
    assert same_bits(np.isnan(got), np.isnan(ref)), f"{label}: NaN masks differ"
    assert same_bits(got[ref == 0], ref[ref == 0])
    fin = np.isfinite(ref) & (ref != 0)
    k = np.max(np.abs(got - ref)[fin] / (EPS * np.abs(ref[fin]))) if fin.any() else 0.0
    print(f"{label}: K = {k:.2f} (limit {4 * terms})")
    assert k <= 4 * terms


# ---------------------------------------------------------------------------- the stored cases
def check_golden(D, gold, case):
    kind, steps = cc.CASES[case]
    d = D.Dynspec(dyn=cc.observation(kind), verbose=False)
    for k, (method, kw) in enumerate(steps):
        before = np.array(d.dyn)
        if method == "refill" and kw.get("zeros", True):
            before[before == 0] = np.nan
        if method == "correct_dyn":
            before[np.isnan(before)] = 0
        quiet(getattr(d, method), **kw)
        for name in cc.ATTRS[1:]:
            ref = gold[f"{case}_{k}_{name}"]
            assert same_bits(getattr(d, name), ref), f"{case} step {k} ({method}): {name} = {getattr(d, name)!r}, reference {ref!r}"
        if f"{case}_{k}_dyn" not in gold.files:
            continue
        ref = gold[f"{case}_{k}_dyn"]
        label = f"{case} step {k} {method}{kw}"
        assert d.dyn.shape == ref.shape and d.dyn.dtype == np.float64
        if method == "refill" and kw.get("method", "biharmonic") in ("linear", "biharmonic") and kw.get("linear", True):
            assert_linear(label, d.dyn, ref, before)
        elif method == "correct_dyn" and kw.get("svd", True):
            mref = gold[f"{case}_{k}_svd_model"]
            assert d.svd_model.dtype == np.complex128 and d.svd_model.shape == mref.shape
            assert_svd(label, gold[f"{case}_sv"], kw.get("nmodes", 1), before, d.svd_model, mref, d.dyn, ref)
        elif method == "correct_dyn":
            if f"{case}_{k}_bandpass" in gold.files:
                assert_nosvd(label + " bandpass", d.bandpass, gold[f"{case}_{k}_bandpass"], ref.shape[1])
            assert_nosvd(label, d.dyn, ref, sum(ref.shape))
        else:
            assert same_bits(d.dyn, ref), f"{label}: not the reference's bits"


# ---------------------------------------------------------------------------- kernel shapes against the oracle
def check_zap(name, x):
    from scintools_amd import clean
    for sigma in (7, 3):
        out, med, mdev = clean.zap_device(x, sigma)
        rmed, rmdev = co.zap_stats(x)
        o = type("O", (), {})()
        o.dyn = x.copy()
        co.zap(o, sigma)
        assert same_bits(med, rmed) and same_bits(mdev, rmdev), f"zap {name}: medians {med!r}, {mdev!r}; NumPy {rmed!r}, {rmdev!r}"
        assert same_bits(out, o.dyn), f"zap {name} sigma {sigma}: mask or pixels differ"
        keep = ~np.isnan(o.dyn)
        assert np.array_equal(out[keep].view(np.uint64), x[keep].view(np.uint64)), f"zap {name}: a kept pixel changed its bits"


def check_zap_method(D):
    x = cc.zap_inputs()["nan30"]
    d = D.Dynspec(dyn=_obs(x), verbose=False)
    alias = d.dyn
    d.zap(sigma=3)
    o = _obs(x)
    co.zap(o, 3)
    assert d.dyn is alias and same_bits(d.dyn, o.dyn) and np.isnan(d.dyn).sum() > np.isnan(x).sum()


MEDIAN_SHAPES = ((7, 9), (64, 64), (37, 130))
MEDIAN_KERNELS = (3, 5, (1, 7), (15, 15))


def _obs(x):
    o = cc.observation()
    o.dyn = np.array(x, dtype=float)
    o.freqs, o.times = 1300.0 + o.df * np.arange(x.shape[0]), o.dt * np.arange(x.shape[1], dtype=float)
    o.nchan, o.nsub = x.shape
    return o


def check_median(D, shape, kernel):
    x = cc.holes(*shape, seed=shape[0])
    d = D.Dynspec(dyn=_obs(x), verbose=False)
    _, said = quiet(d.refill, method="median", kernel_size=kernel)
    assert ("kernel size is set to default" in said) == (kernel == 5)
    o = _obs(x)
    co.refill(o, method="median", kernel_size=kernel)
    assert same_bits(d.dyn, o.dyn) and np.isfinite(d.dyn).all(), f"median {shape} {kernel}"
    assert np.array_equal(d.dyn[~np.isnan(x)], x[~np.isnan(x)])
    if shape == (7, 9) and kernel == (15, 15):           # the window exceeds the array: mostly padding, the median is 0
        assert (d.dyn[np.isnan(x)] == 0.0).all()


LINEAR_SHAPES = ((5, 300, 1), (300, 5, 0), (48, 40, 0), (48, 40, 1), (5, 300, 0), (300, 5, 1))


def check_linear(D, nf, nt, axis):
    for seed in (0, 1, 3):
        x = cc.gaps(nf, nt, axis, seed)
        d = D.Dynspec(dyn=_obs(x), verbose=False)
        alias = d.dyn
        d.refill(method="linear", zeros=False)
        o = _obs(x)
        co.refill(o, method="linear", zeros=False)
        assert d.dyn is not alias
        assert_linear(f"linear {nf}x{nt} axis {axis} seed {seed}", d.dyn, o.dyn, x)


def check_refill_other(D, pytest):
    x = cc.holes(12, 14, seed=2)
    for kw in (dict(method="linear"), dict(), dict(method="cubic"), dict(method="nearest")):
        d = D.Dynspec(dyn=_obs(x), verbose=False)
        with pytest.raises(NotImplementedError, match="median"):
            quiet(d.refill, **kw)
    both = 0.5 + np.random.default_rng(0).random((9, 8))
    both[4, :] = np.nan
    both[:, 3] = np.nan
    block = 0.5 + np.random.default_rng(0).random((9, 8))
    block[2:4, 5:7] = 0.0                                # zeros=True makes the block a hole
    for y in (both, block):
        with pytest.raises(NotImplementedError, match="Qhull"):
            D.Dynspec(dyn=_obs(y), verbose=False).refill(method="linear")
    for method in ("linear", "cubic", "nearest", "biharmonic"):      # linear=False: only the mean fill, bit-equal
        d = D.Dynspec(dyn=_obs(x), verbose=False)
        quiet(d.refill, method=method, linear=False)
        ref = np.where(np.isnan(x), np.mean(x[np.isfinite(x)]), x)
        assert same_bits(d.dyn, ref)
    _, said = quiet(D.Dynspec(dyn=_obs(cc.gaps(8, 8, 0, 0)), verbose=False).refill)
    assert "biharmonic inpainting not available" in said
    for bad in (4, (3, 4)):
        with pytest.raises(ValueError, match="should be odd"):
            D.Dynspec(dyn=_obs(x), verbose=False).refill(method="median", kernel_size=bad)
    with pytest.raises(ValueError, match="225"):
        D.Dynspec(dyn=_obs(x), verbose=False).refill(method="median", kernel_size=17)


SVD_SHAPES = ((1, 64, 1), (64, 1, 1), (33, 70, 1), (33, 70, 2), (33, 70, 4), (257, 129, 2), (512, 96, 1), (512, 96, 4),
              (1, 64, 2), (64, 1, 3), (3, 50, 4))


def check_svd(D, nf, nt, nmodes, nans=False):
    a = cc.svd_matrix(nf, nt, nmodes, seed=nf + nt + nmodes, nans=nans)
    d = D.Dynspec(dyn=_obs(a), verbose=False)
    d.correct_dyn(nmodes=nmodes)
    o = _obs(a)
    co.correct_dyn(o, nmodes=nmodes)
    a0 = np.nan_to_num(a, nan=0.0)
    s = np.linalg.svd(a0, compute_uv=False)
    assert nmodes >= len(s) or 1 - (s[nmodes] / s[nmodes - 1]) ** 2 >= 0.5
    assert_svd(f"svd {nf}x{nt} nmodes {nmodes}" + (" with zeros and NaNs" if nans else ""), s, nmodes, a0, d.svd_model,
               o.svd_model, d.dyn, o.dyn)
    assert d.svd_model.dtype == np.complex128


def check_svd_model(T):
    z = cc.complex_matrix()
    s = np.linalg.svd(z, compute_uv=False)
    for nmodes in (1, 2):
        ref = co.svd_model(z, nmodes)[0]
        got = T.svd_model(z, nmodes=nmodes)
        mm = np.max(np.abs(ref))
        bound, relgap = svd_bound(s, nmodes)
        err = np.max(np.abs(got - ref)) / mm
        print(f"svd_model 40x24 complex nmodes {nmodes}: relgap {relgap:.3f}, bound {bound:.3g}, error {err:.3g} (K = {err / bound:.3g})")
        assert got.dtype == np.complex128 and err <= bound
    r = cc.svd_matrix(33, 70, 1, seed=3)
    got = T.svd_model(r)
    ref = co.svd_model(r, 1)[0]
    assert got.dtype == np.complex128
    assert np.max(np.abs(got - ref)) <= svd_bound(np.linalg.svd(r, compute_uv=False), 1)[0] * np.abs(ref).max()


def check_svd_errors(D, pytest):
    a = cc.svd_matrix(20, 30, 1, seed=1)
    d = D.Dynspec(dyn=_obs(a), verbose=False)
    with pytest.raises(ValueError, match="at most 4"):
        d.correct_dyn(nmodes=5)
    with pytest.raises(NotImplementedError):
        d.correct_dyn(velocity=True)
    from scintools_amd import ththmod
    with pytest.raises(ValueError, match="at most 4"):
        ththmod.svd_model(a, nmodes=5)
    d.correct_dyn()
    _, said = quiet(d.correct_dyn)
    assert "An svd_model exists" in said


def check_nosvd(D, kw):
    a = cc.intensity(37, 53, seed=4)                     # positive, as the bound assumes
    rng = np.random.default_rng(4)
    a[rng.random(a.shape) < 0.03] = np.nan
    a[rng.random(a.shape) < 0.03] = 0.0
    d = D.Dynspec(dyn=_obs(a), verbose=False)
    d.correct_dyn(svd=False, **kw)
    o = _obs(a)
    co.correct_dyn(o, svd=False, **kw)
    if kw.get("frequency", True):
        assert_nosvd(f"svd=False {kw} bandpass", d.bandpass, o.bandpass, a.shape[1])
    assert_nosvd(f"svd=False {kw}", d.dyn, o.dyn, sum(a.shape))


def check_lamsteps(D):
    """correct_dyn(lamsteps=True) works on lamdyn (scale_dyn is called when it is absent) and leaves dyn's pixels alone."""
    a = cc.intensity(40, 36, seed=2)
    d = D.Dynspec(dyn=_obs(a), verbose=False)
    d.correct_dyn(lamsteps=True)
    lam_before = D.Dynspec(dyn=_obs(a), verbose=False)
    lam_before.scale_dyn()
    ref = np.array(lam_before.lamdyn)
    o = _obs(ref)
    co.correct_dyn(o)
    s = np.linalg.svd(ref, compute_uv=False)
    assert same_bits(d.dyn, a)
    assert_svd("correct_dyn(lamsteps=True)", s, 1, ref, d.svd_model, o.svd_model, np.asarray(d.lamdyn), o.dyn)


def check_auto_processing(D):
    o = cc.observation("channels")
    d = D.Dynspec(dyn=o, verbose=False)
    quiet(d.auto_processing)
    r = cc.observation("channels")
    co.trim_edges(r)
    assert same_bits(d.freqs, r.freqs) and same_bits(d.times, r.times) and d.dyn.shape == r.dyn.shape
    assert np.isfinite(d.dyn).all() and d.acf.shape == (2 * d.dyn.shape[0], 2 * d.dyn.shape[1])
    assert d.sspec.shape[1] == len(d.fdop) and d.sspec.shape[0] == len(d.tdel)


def check_deterministic(D):
    a = cc.svd_matrix(33, 70, 2, seed=8)
    runs = []
    for _ in range(2):
        d = D.Dynspec(dyn=_obs(a), verbose=False)
        d.correct_dyn(nmodes=2)
        runs.append((d.dyn, d.svd_model))
    assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1])
