"""The thin-screen kernels (thth.hip thin_gather_kernel, eigen.hip sv_* Lanczos) run through the host interpreter (tests/emu)
at small sizes, through the same C ABI and Python wrappers as on the GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)
import thin_cases as tc  # noqa: E402
import thin_oracle as to  # noqa: E402


@pytest.fixture()
def emu(monkeypatch):
    import emulated
    emulated.install(monkeypatch)
    from scintools_amd import ththmod
    return ththmod


@pytest.fixture(scope="module")
def small(golden):
    g = golden("thin.npz")
    d = {k: g[k] for k in g.files if not k.startswith(("tut_", "def_"))}
    d["CS"] = np.fft.fftshift(np.fft.fft2(d["dyn"]))
    return d


@pytest.mark.parametrize("tag", ["eq_lo", "eq", "ne", "eq_hi"])
def test_two_curve_map_zero_mismatch(emu, small, tag):
    s = small
    f1, f2 = s[f"fac_{tag}"]
    e2 = s["edges"] if tag in ("eq_lo", "eq_hi") else s["arclet"]
    red, er1, er2 = emu.two_curve_map(s["CS"], s["tau"], s["fd"], f1 * s["eta_true"], s["edges"], f2 * s["eta_true"], e2)
    assert red.shape == s[f"map_{tag}"].shape
    assert np.count_nonzero(red != s[f"map_{tag}"]) == 0
    assert np.array_equal(np.asarray(er1), s[f"er1_{tag}"]) and np.array_equal(np.asarray(er2), s[f"er2_{tag}"])
    if tag == "eq_lo":                       # the negative-Doppler wrap is exercised
        assert to.two_curve_map(s["CS"], s["tau"], s["fd"], 0.5 * s["eta_true"], s["edges"], 0.5 * s["eta_true"],
                                s["edges"], stats=True)[3].sum() > 100


def test_index_error_cases(emu, small):
    s = small
    e = 0.3 * s["eta_true"]
    with pytest.raises(IndexError):
        to.two_curve_map(s["CS"], s["tau"], s["fd"], e, s["wide"], e, s["wide"])
    with pytest.raises(IndexError):
        emu.two_curve_map(s["CS"], s["tau"], s["fd"], e, s["wide"], e, s["wide"])
    with pytest.raises(IndexError):
        emu.singularvalue_calc(s["CS"], s["tau"], s["fd"], e, s["wide"], e, s["wide"], 0.0)
    # in a sweep such a curvature is NaN (single_search_thin's except); the other chunk of the same call is computed
    etas = np.array([0.3, 2.0]) * s["eta_true"]
    sv = emu.sv_sweep_multi(np.stack([s["CS"], s["CS"]]), [(s["tau"], s["fd"], s["wide"], s["wide"]),
                                                           (s["tau"], s["fd"], s["wide"] * 0.3, s["wide"] * 0.3)],
                            [etas, etas])
    assert np.all(np.isnan(sv[0]))
    for e, v in zip(etas, sv[1]):
        ref = to.singularvalue_calc(s["CS"], s["tau"], s["fd"], e, s["wide"] * 0.3, e, s["wide"] * 0.3, 0.0)
        assert v == pytest.approx(ref, rel=1e-10)


@pytest.mark.parametrize("cut", ["cut0", "cut1", "cutall"])
def test_singular_values_against_the_golden(emu, small, cut):
    s = small
    sv = emu.sv_sweep_multi(s["CS"][None], [(s["tau"], s["fd"], s["edges"], s["arclet"])], [s["sv_etas"]],
                            float(s[f"cutval_{cut}"]))[0]
    if cut == "cutall":
        assert np.all(sv == 0.0)
    else:
        np.testing.assert_allclose(sv, s[f"sv_{cut}"], rtol=1e-10)


@pytest.mark.parametrize("nedge1,nedge2", [(2, 2), (3, 2), (4, 3), (2, 5), (3, 4)])
def test_tiny_matrices_exact(emu, small, nedge1, nedge2):
    """n = 1, 2, 3 columns / rows: the Krylov space is complete before the residual rule is met."""
    s = small
    fdm = s["fd"].max()
    e1 = np.linspace(-0.1 * fdm, 0.1 * fdm, nedge1)
    e2 = np.linspace(-0.05 * fdm, 0.07 * fdm, nedge2)
    eta = s["eta_true"]
    red = to.two_curve_map(s["CS"], s["tau"], s["fd"], eta, e1, eta, e2)[0]
    assert red.shape == (nedge2 - 1, nedge1 - 1)
    got = emu.singularvalue_calc(s["CS"], s["tau"], s["fd"], eta, e1, eta, e2, 0.0)
    assert got == pytest.approx(np.linalg.svd(red, compute_uv=False)[0], rel=1e-10, abs=0)


def test_all_zero_map_is_zero(emu, small):
    s = small
    z = np.zeros_like(s["CS"])
    got = emu.singularvalue_calc(z, s["tau"], s["fd"], s["eta_true"], s["edges"], s["eta_true"], s["arclet"], 0.0)
    assert got == 0.0


def test_random_rectangular_matrices_against_lapack(emu, small):
    """CS of random numbers: every map is a dense random rectangle, where the top singular value is not well separated."""
    s = small
    rng = np.random.default_rng(4)
    cs = rng.standard_normal(s["CS"].shape) + 1j * rng.standard_normal(s["CS"].shape)
    etas = np.array([0.7, 1.1]) * s["eta_true"]
    sv = emu.sv_sweep_multi(cs[None], [(s["tau"], s["fd"], s["edges"], s["arclet"])], [etas], 0.05 * s["fd"].max())[0]
    for e, v in zip(etas, sv):
        red = to.two_curve_map(cs, s["tau"], s["fd"], e, s["edges"], e, s["arclet"])
        c = (red[1][1:] + red[1][:-1]) / 2
        m = red[0].copy()
        m[:, np.abs(c) < 0.05 * s["fd"].max()] = 0
        assert v == pytest.approx(np.linalg.svd(m, compute_uv=False)[0], rel=1e-10)


def test_multi_chunk_call_equals_chunk_by_chunk(emu, small):
    s = small
    rng = np.random.default_rng(1)
    cs2 = s["CS"] * (1 + 0.1 * rng.standard_normal(s["CS"].shape))
    grids = [(s["tau"], s["fd"], s["edges"], s["arclet"]), (s["tau"], s["fd"] * 1.01, s["edges"] * 0.99, s["arclet"] * 0.99)]
    etas = [s["sv_etas"][:5], s["sv_etas"][2:]]
    stack = np.stack([s["CS"], cs2])
    both = emu.sv_sweep_multi(stack, grids, etas, 0.02)
    for k in range(2):
        one = emu.sv_sweep_multi(stack[k:k + 1], grids[k:k + 1], etas[k:k + 1], 0.02)[0]
        assert np.array_equal(one, both[k])
    # and resident one at a time
    one_by_one = emu.sv_sweep_multi(stack, grids, etas, 0.02, batch=1)
    for k in range(2):
        assert np.array_equal(one_by_one[k], both[k])


# ---- the small members of the MI355X case list (tests/thin_cases.py, tests/test_gpu_thin_classes.py) --------------------------
@pytest.fixture(scope="module")
def ax():
    return tc.axes()


@pytest.fixture(scope="module")
def spectra():
    return {k: tc.spectrum(k) for k in ("arc", "gauss", "zero")}


@pytest.mark.parametrize("n1,n2,kind,cutf", tc.small_class_cases() + [(150, 300, "arc", 0.02), (257, tc.N2_TALL, "gauss", 0.02), (4097, 3, "arc", 0.0),
                                                                  (8193, 2, "gauss", 0.0)],
                         ids=lambda v: str(v))
def test_class_cases_against_lapack(emu, ax, spectra, n1, n2, kind, cutf):
    """Classes 0, 1 and 2 (n1 <= 513) with 1, 2, 3, 4, 5 and 11 rows, one R = 4 map of 75 strips, one tall map (R = 6, last strip
    of 5 rows) and one few-row map in each of the 512- and 1024-thread classes: the assertions of
    test_gpu_thin_classes.py::test_class_against_lapack."""
    tau, fd = ax
    g = tc.grid(n1, n2, tau, fd)
    eta = tc.eta0(tau, fd)
    cut = cutf * fd.max()
    ref = tc.oracle_sv(spectra[kind], tau, fd, eta, g[2], eta, g[3], cut)
    sv, info = emu.sv_sweep_multi(spectra[kind][None], [g], [np.array([eta])], cut, return_info=True)
    assert int(info["ranges"][0, 3]) == n1 and int(info["ranges"][0, 1]) == n2
    assert info["status"][0] == 0
    assert sv[0][0] == pytest.approx(ref, rel=1e-10, abs=0)
    assert info["iters"][0] < tc.MAX_ITER
    if n2 < tc.FIRST_CHECK:
        assert info["iters"][0] <= tc.FIRST_CHECK


@pytest.mark.parametrize("n1,n2", [(200, 9), (513, 6)])
def test_zero_middle_row(emu, ax, spectra, n1, n2):
    tau, fd = ax
    g = tc.grid(n1, n2, tau, fd)
    eta = tc.eta0(tau, fd)
    CS = tc.zero_middle_row(spectra["gauss"], tau, fd, eta, g[2], g[3])
    ref = tc.oracle_sv(CS, tau, fd, eta, g[2], eta, g[3], 0.0)
    sv, info = emu.sv_sweep_multi(CS[None], [g], [np.array([eta])], 0.0, return_info=True)
    assert info["status"][0] == 0 and ref > 0
    assert sv[0][0] == pytest.approx(ref, rel=1e-10, abs=0)
    assert info["iters"][0] <= tc.FIRST_CHECK


@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_non_finite_pixel(emu, ax, spectra, value):
    from scintools_amd import _lib
    tau, fd = ax
    g = tc.grid(300, 9, tau, fd)
    eta = tc.eta0(tau, fd)
    clean = spectra["arc"]
    bad = tc.poisoned(clean, tau, fd, eta, g[2], g[3], value, which=3)
    sv, info = emu.sv_sweep_multi(np.stack([bad, clean]), [g, g], [np.array([eta])] * 2, 0.0, return_info=True)
    assert np.isnan(sv[0][0]) and info["status"][0] == _lib.SCINT_E_NONFINITE
    assert sv[1][0] == pytest.approx(tc.oracle_sv(clean, tau, fd, eta, g[2], eta, g[3], 0.0), rel=1e-10, abs=0)
    with pytest.raises(np.linalg.LinAlgError):
        emu.singularvalue_calc(bad, tau, fd, eta, g[2], eta, g[3], 0.0)


def test_column_limit_names_the_limit(emu, ax, spectra):
    from scintools_amd._lib import ScintHipError
    tau, fd = ax
    g = tc.grid(tc.SV_MAX_COLS + 1, 2, tau, fd)
    with pytest.raises(ScintHipError, match="16384"):
        emu.sv_sweep_multi(spectra["arc"][None], [g], [np.array([4.0 * tc.eta0(tau, fd)])])


PROBE = os.path.join(HERE, "thin_order_probe.py")


def test_results_do_not_depend_on_the_interpreter_order(tmp_path, emu):
    outs = []
    for order in ("", "rev"):
        env = dict(os.environ)
        env.pop("SCINT_EMU_ORDER", None)
        if order:
            env["SCINT_EMU_ORDER"] = order
        path = str(tmp_path / f"o{order or 'fwd'}.npz")
        r = subprocess.run([sys.executable, PROBE, path], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(np.load(path))
    for k in outs[0].files:
        assert np.array_equal(outs[0][k], outs[1][k], equal_nan=True), k
