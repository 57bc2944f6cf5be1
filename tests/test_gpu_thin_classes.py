"""The thin-screen sigma_1 sweep on an MI355X across every instantiation of sv_matvec_kernel (eigen.hip): kept row lengths on
both sides of every class boundary and inside every class, with 1 .. 1301 rows, against tests/thin_oracle.py followed by a
dense LAPACK SVD; mixed classes and chunks in one call; degenerate and non-finite maps; the 16384-column limit; and the
gather (thin_gather_kernel) fuzzed bit for bit against the oracle.  Cases come from tests/thin_cases.py, which the host
interpreter test (tests/test_thin_emu_cpu.py) shares.

Every test prints what it measured (class, sizes, relative error, steps) before it asserts: run with -s to collect the figures."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import thin_cases as tc  # noqa: E402
import thin_oracle as to  # noqa: E402

pytestmark = pytest.mark.gpu

REL = 1e-10          # the sigma_1 tolerance of tests/test_gpu_thin.py and of the golden tests


@pytest.fixture(scope="module")
def thth():
    from scintools_amd import ththmod
    from scintools_amd.device import require_gpu
    require_gpu()
    assert ththmod.DEFAULT_MAX_ITER == tc.MAX_ITER
    return ththmod


@pytest.fixture(scope="module")
def ax():
    return tc.axes()


@pytest.fixture(scope="module")
def spectra():
    return {k: tc.spectrum(k) for k in ("arc", "gauss", "zero")}


# ---- 1. every mat-vec class against LAPACK -------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2,kind,cutf", tc.class_cases(), ids=lambda v: str(v))
def test_class_against_lapack(thth, ax, spectra, n1, n2, kind, cutf):
    tau, fd = ax
    CS = spectra[kind]
    g = tc.grid(n1, n2, tau, fd)
    eta = tc.eta0(tau, fd)
    cut = cutf * fd.max()
    ref, gap = tc.oracle_sv(CS, tau, fd, eta, g[2], eta, g[3], cut, with_gap=True)
    a, info = thth.sv_sweep_multi(CS[None], [g], [np.array([eta])], cut, return_info=True)
    b = thth.sv_sweep_multi(CS[None], [g], [np.array([eta])], cut)
    sv, st, it = float(a[0][0]), int(info["status"][0]), int(info["iters"][0])
    print(f"\nTHINCLASS cls={tc.sv_class(n1)} n1={n1} n2={n2} kind={kind} cut={cutf} rel={abs(sv - ref) / ref:.3e} "
          f"iters={it} status={st} s2/s1={gap:.4f}")
    assert int(info["ranges"][0, 3]) == n1 and int(info["ranges"][0, 1]) == n2      # the intended class is the one that ran
    assert st == 0
    assert sv == pytest.approx(ref, rel=REL, abs=0)
    assert it < tc.MAX_ITER
    if n2 < tc.FIRST_CHECK:
        assert it <= tc.FIRST_CHECK       # an exhausted Krylov space stops at the first check
    assert np.array_equal(a[0], b[0])


# ---- 2. mixed classes and chunks in one call -----------------------------------------------------------------------------
def test_mixed_classes_and_chunks_in_one_call(thth, ax):
    tau, fd = ax
    n1, n2 = tc.SV_MAX_COLS, 23
    base = tc.grid(n1, n2, tau, fd)
    grids = [base, (tau, fd * 1.01, base[2] * 0.99, base[3] * 0.99), (tau * 1.02, fd, base[2] * 0.97, base[3] * 1.03)]
    stack = np.stack([tc.spectrum("arc", 1), tc.spectrum("gauss", 1), tc.spectrum("arc", 2)])
    etas = [np.geomspace(1.0, 4000.0, 40) * tc.eta0(g[0], g[1]) for g in grids]
    cut = 0.01
    both, info = thth.sv_sweep_multi(stack, grids, etas, cut, return_info=True)
    kept = info["ranges"][:, 3]
    classes = sorted({tc.sv_class(int(n)) for n in kept})
    print(f"\nTHINMIXED n1 {kept.min()}..{kept.max()} classes {classes} max iters {info['iters'].max()}")
    assert len(classes) >= 4 and kept.max() == n1
    assert np.all(info["status"] == 0)
    worst = 0.0
    for k in range(3):
        for e, v in zip(etas[k], both[k]):
            ref = tc.oracle_sv(stack[k], *grids[k][:2], e, grids[k][2], e, grids[k][3], cut)
            worst = max(worst, abs(v - ref) / ref)
            assert v == pytest.approx(ref, rel=REL, abs=0)
    print(f"THINMIXED worst rel {worst:.3e}")
    for k in range(3):
        one = thth.sv_sweep_multi(stack[k:k + 1], grids[k:k + 1], etas[k:k + 1], cut)[0]
        assert np.array_equal(one, both[k])
    one_by_one = thth.sv_sweep_multi(stack, grids, etas, cut, batch=1)
    for k in range(3):
        assert np.array_equal(one_by_one[k], both[k])


# ---- 3. degenerate and hostile maps --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2", [(200, 9), (4750, 9), (8193, 6)])
def test_zero_middle_row(thth, ax, spectra, n1, n2):
    """The Lanczos start vector (the kept middle row) is zero and the map is not: the constant-vector start of sv_q."""
    tau, fd = ax
    g = tc.grid(n1, n2, tau, fd)
    eta = tc.eta0(tau, fd)
    CS = tc.zero_middle_row(spectra["gauss"], tau, fd, eta, g[2], g[3])
    ref = tc.oracle_sv(CS, tau, fd, eta, g[2], eta, g[3], 0.0)
    sv, info = thth.sv_sweep_multi(CS[None], [g], [np.array([eta])], 0.0, return_info=True)
    print(f"\nTHINZERO n1={n1} n2={n2} rel={abs(sv[0][0] - ref) / ref:.3e} iters={info['iters'][0]}")
    assert info["status"][0] == 0 and ref > 0
    assert sv[0][0] == pytest.approx(ref, rel=REL, abs=0)
    assert thth.singularvalue_calc(CS, tau, fd, eta, g[2], eta, g[3], 0.0) == sv[0][0]


@pytest.mark.parametrize("n1,n2", [(150, 7), (16384, 7), (256, 1), (8193, 1)])
def test_all_zero_spectrum_is_exactly_zero(thth, ax, spectra, n1, n2):
    tau, fd = ax
    g = tc.grid(n1, n2, tau, fd)
    eta = tc.eta0(tau, fd)
    sv, info = thth.sv_sweep_multi(spectra["zero"][None], [g], [np.array([eta])], 0.0, return_info=True)
    assert info["status"][0] == 0 and sv[0][0] == 0.0
    assert thth.singularvalue_calc(spectra["zero"], tau, fd, eta, g[2], eta, g[3], 0.0) == 0.0


@pytest.mark.parametrize("n1,n2", [(200, 9), (4750, 9), (11999, 5)])
@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_non_finite_pixel(thth, ax, spectra, n1, n2, value):
    from scintools_amd import _lib
    tau, fd = ax
    g = tc.grid(n1, n2, tau, fd)
    eta = tc.eta0(tau, fd)
    clean = spectra["arc"]
    bad = tc.poisoned(clean, tau, fd, eta, g[2], g[3], value, which=n1)
    for order in (0, 1):                     # the poisoned chunk first, then second
        stack = np.stack([bad, clean] if order == 0 else [clean, bad])
        sv, info = thth.sv_sweep_multi(stack, [g, g], [np.array([eta]), np.array([eta])], 0.0, return_info=True)
        assert np.isnan(sv[order][0]) and info["status"][order] == _lib.SCINT_E_NONFINITE
        assert info["status"][1 - order] == 0
        assert sv[1 - order][0] == pytest.approx(tc.oracle_sv(clean, tau, fd, eta, g[2], eta, g[3], 0.0), rel=REL, abs=0)
    with pytest.raises(np.linalg.LinAlgError):
        thth.singularvalue_calc(bad, tau, fd, eta, g[2], eta, g[3], 0.0)


def test_doppler_index_below_range_is_nan_for_its_chunk_only(thth, ax, spectra):
    """One chunk of three whose grid reaches fd_inv < -len(fd) (NumPy raises IndexError): NaN for every curvature of that chunk,
    the others right, at more than 4096 kept columns."""
    from scintools_amd import _lib
    tau, fd = ax
    n1, n2 = 11999, 9
    g = tc.grid(n1, n2, tau, fd)
    wide = (tau, fd, g[2] * 2.2, g[3] * 3.4)       # theta1 - theta2 < -3.02 fd_max at in-range delays
    eta = tc.eta0(tau, fd)
    etas = np.array([1.0, 1.5]) * eta
    with pytest.raises(IndexError):
        to.two_curve_map(spectra["arc"], tau, fd, eta, wide[2], eta, wide[3])
    stack = np.stack([spectra["arc"], spectra["arc"], spectra["gauss"]])
    sv, info = thth.sv_sweep_multi(stack, [g, wide, g], [etas] * 3, 0.0, return_info=True)
    assert info["ranges"][2, 3] > 4096                    # the flagged chunk's kept columns
    assert np.all(np.isnan(sv[1])) and np.all(info["status"][2:4] == _lib.SCINT_E_ARG)
    for k in (0, 2):
        for e, v in zip(etas, sv[k]):
            assert v == pytest.approx(tc.oracle_sv(stack[k], tau, fd, e, g[2], e, g[3], 0.0), rel=REL, abs=0)
    with pytest.raises(IndexError):
        thth.singularvalue_calc(spectra["arc"], tau, fd, eta, wide[2], eta, wide[3], 0.0)


@pytest.mark.parametrize("n1,n2", [(1500, 40), (4750, 40)])
@pytest.mark.parametrize("f1,f2", [(0.6, 1.0), (1.0, 1.7)])
def test_singularvalue_calc_with_two_curvatures(thth, ax, spectra, n1, n2, f1, f2):
    tau, fd = ax
    g = tc.grid(n1, n2, tau, fd)
    eta = tc.eta0(tau, fd)
    cut = 0.02 * fd.max()
    red = tc.oracle_map(spectra["arc"], tau, fd, f1 * eta, g[2], f2 * eta, g[3], cut)
    assert red.shape == (n2, n1)
    got = thth.singularvalue_calc(spectra["arc"], tau, fd, f1 * eta, g[2], f2 * eta, g[3], cut)
    ref = np.linalg.svd(red, compute_uv=False)[0]
    print(f"\nTHINTWO n1={n1} f=({f1},{f2}) rel={abs(got - ref) / ref:.3e}")
    assert got == pytest.approx(ref, rel=REL, abs=0)


def test_column_limit(thth, ax, spectra):
    """scint_sv_sweep_multi takes at most 16384 theta1 centres (M1, before the crop: SCINT_REQUIRE(M1 <= kSvMaxCols)).  16385
    edges run; 16386 edges are refused with an error that names the limit, also where the crop would keep fewer than 16385."""
    from scintools_amd._lib import ScintHipError
    tau, fd = ax
    eta = tc.eta0(tau, fd)
    g = tc.grid(tc.SV_MAX_COLS + 1, 3, tau, fd)
    assert g[2].shape[0] == 16386
    for e in (eta, 4.0 * eta):               # keeps all 16385 centres / about half of them
        assert (to.two_curve_map(spectra["arc"], tau, fd, e, g[2], e, g[3])[0].shape[1] > tc.SV_MAX_COLS) == (e == eta)
        with pytest.raises(ScintHipError, match="16384"):
            thth.sv_sweep_multi(spectra["arc"][None], [g], [np.array([e])])
        with pytest.raises(ScintHipError, match="16384"):
            thth.singularvalue_calc(spectra["arc"], tau, fd, e, g[2], e, g[3], 0.0)


# ---- 4. the gather against the oracle, bit for bit -----------------------------------------------------------------------
def test_gather_bit_exact_vs_oracle(thth):
    raised = wrapped = big = 0
    for k in range(tc.GATHER_CASES):
        c = tc.gather_case(k)
        args = (c["CS"], c["tau"], c["fd"], c["eta1"], c["edges1"], c["eta2"], c["edges2"])
        try:
            red, er1, er2, wrap = to.two_curve_map(*args, stats=True)
        except IndexError:
            raised += 1
            with pytest.raises(IndexError):
                thth.two_curve_map(*args)
            continue
        got, g1, g2 = thth.two_curve_map(*args)
        assert got.shape == red.shape, k
        assert np.count_nonzero(got != red) == 0, k
        assert np.array_equal(np.asarray(g1), er1) and np.array_equal(np.asarray(g2), er2), k
        wrapped += bool(wrap.any())
        big += red.shape[1] > 4096
    print(f"\nTHINGATHER cases={tc.GATHER_CASES} raised={raised} wrapped={wrapped} over4096={big}")
    assert 0.05 * tc.GATHER_CASES <= raised <= 0.25 * tc.GATHER_CASES
    assert wrapped >= tc.GATHER_CASES / 4
    assert big >= 5
