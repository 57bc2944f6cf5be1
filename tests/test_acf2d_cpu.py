"""CPU checks of the approximate 2-D ACF fit without a GPU and without the interpreter: the oracle's residual is the reference's
(tests/golden/acf2d_approx.npz) bit for bit, its analytic Jacobian agrees with central differences, the new names exist and raise
the package's "no GPU" error, the case list keeps its promises and the committed tolerances are the maker's."""
import ctypes

import numpy as np
import pytest

import acf2d_cases as cc
import acf2d_checks as ck
import acf2d_oracle as ao


@pytest.mark.parametrize("name", ck.GOLDEN_CASES)
def test_oracle_residual_is_the_references(name):
    g = ck.golden()
    pars, tdata, fdata, ydata, weights = ck.golden_inputs(name)
    p = [pars[k] for k in cc.FIT_KEYS]
    assert np.array_equal(ao.model_residual(p, tdata, fdata, ydata, weights.copy(), pars["tobs"], pars["bw"]), g[name + "_w"])
    assert np.array_equal(ao.model_residual(p, tdata, fdata, ydata, None, pars["tobs"], pars["bw"]), g[name + "_n"])
    nf, nt = ydata.shape
    assert g[name + "_w"][nf // 2, nt // 2] == 0 and np.count_nonzero(g[name + "_w"]) == nf * nt - 1


@pytest.mark.parametrize("name,b", [("real12", 0), ("real12", 7), ("tilted", 1), ("odd", 0)])
def test_jacobian_by_central_differences(name, b):
    """h = 1e-6 in each of (log tau, log dnu, log amp, alpha, phasegrad): the truncation error is h^2 |r'''| / 6 ~ 1e-12 |r|, the
    rounding error eps |r| / h ~ 2e-10 |r|; the bound is 1e-7 of the largest entry of the column."""
    setups, fits = cc.oracle(name)
    s, f = setups[b], fits[b]
    p = np.array([f[k] for k in cc.FIT_KEYS])
    J = ao.jacobian(p, s)
    h = 1e-6
    for col in range(5):
        def at(step):
            q = p.copy()
            q[col] = q[col] * np.exp(step) if col < 3 else q[col] + step
            return ao.residuals(q, s)
        num = (at(h) - at(-h)) / (2 * h)
        assert np.abs(num - J[:, col]).max() <= 1e-7 * np.abs(J[:, col]).max(), (name, b, col)
        assert np.abs(J[:, col]).max() > 0


def test_new_names_exist_and_need_a_gpu():
    import torch
    from scintools_amd import _lib, build, scint_models, scintpar
    from scintools_amd.dynspec import Dynspec
    assert Dynspec.fit_scint_params_2d is scintpar.fit_scint_params_2d
    assert Dynspec.fit_scint_params_2d_cut is scintpar.fit_scint_params_2d_cut
    assert callable(scintpar.acf2d_approx_fit_device) and callable(scint_models.scint_acf_model_2d_approx)
    for sym in ("scint_acf2d_approx_fit", "scint_acf2d_approx_fit_workspace_bytes", "scint_acf2d_approx_model", "scint_acf_argmax"):
        assert sym in _lib.header_symbols()
    if torch.cuda.is_available():
        return
    build.build(verbose=False)
    d = Dynspec(dyn=cc.observation(), verbose=False)
    for call in (d.fit_scint_params_2d, lambda: d.fit_scint_params_2d_cut(1, 2),
                 lambda: scintpar.acf2d_approx_fit_device(torch.zeros((1, 16, 16), dtype=torch.float64), 30.0, 0.5, 4.0, 240.0)):
        with pytest.raises(_lib.ScintHipError):
            call()
    assert not hasattr(d, "phasegrad") and not hasattr(d, "cut_phasegrad")
    with pytest.raises(NotImplementedError):
        d.get_scint_params(method="acf2d_approx")


def test_entry_points_check_their_arguments():
    import torch
    from scintools_amd import _lib, build
    build.build(verbose=False)
    _lib.load()
    need = ctypes.c_size_t()
    _lib.call("scint_acf2d_approx_fit_workspace_bytes", 4096, 128, 128, 0, need)
    assert need.value == 256
    _lib.call("scint_acf2d_approx_fit_workspace_bytes", 3, 16, 20, 1, need)
    assert need.value >= 3 * 2 * 16 * 20 * 8
    a = torch.zeros(8, dtype=torch.float64)
    i = torch.zeros(8, dtype=torch.int32)
    good = [a, 1, 16, 16, i, a, i, a, a, 8.0, 8.0, 1, 1, 0, 200, a, a, a, i, i, i, 0, a, 1 << 20, None]
    for pos, value, msg in ((0, None, "null"), (2, 4, "bad shape"), (1, 0, "bad shape"), (9, 0.0, "nsub"), (14, 0, "max_iter"),
                            (21, 1, "workspace")):
        args = list(good)
        args[pos] = value
        if pos == 21:
            args[23] = 8
        with pytest.raises(_lib.ScintHipError, match=msg):
            _lib.call("scint_acf2d_approx_fit", *args)
    with pytest.raises(TypeError, match="rect"):
        _lib.call("scint_acf2d_approx_fit", *(good[:4] + [a] + good[5:]))         # float64 where int32 device memory goes
    with pytest.raises(_lib.ScintHipError, match="bad shape"):
        _lib.call("scint_acf2d_approx_model", a, 0, a, 3, None, None, 1.0, 1.0, 1.0, 5/3, 0.0, 1.0, 1.0, a, None)
    with pytest.raises(_lib.ScintHipError, match="bad shape"):
        _lib.call("scint_acf_argmax", a, 1, 1 << 20, 1 << 20, i, None)


def test_shapes_of_the_case_list():
    """What the shapes are there for (tests/acf2d_cases.py)."""
    tiny, _ = cc.oracle("tiny")
    assert len(tiny) == 5 and all(s["y"].size < 64 for s in tiny)
    tilted, _ = cc.oracle("tilted")
    assert all(s["y"].size > 256 for s in tilted) and set(np.sign(cc.case("tilted").planted[:, 4])) == {-1.0, 1.0}
    assert cc.case("odd").stack.shape[1:] == (37, 51)
    full, _ = cc.oracle("full")
    assert all(s["y"].shape == (39, 63) for s in full)
    long_, _ = cc.oracle("long")
    assert long_[0]["y"].shape == (19, 1999)
    assert len(cc.case("real300").stack) == 300 and cc.case("real12_alpha").kw["alpha"] is None
    bad, fits = cc.oracle("badwin")
    assert bad[0] is not None and bad[1] is None and bad[2] is not None
    assert fits[1]["rect"][1] % 2 == 0 or fits[1]["rect"][3] % 2 == 0


@pytest.mark.parametrize("name", cc.FIT_CASES)
def test_oracle_converges_on_every_case(name):
    c = cc.case(name)
    setups, fits = cc.oracle(name)
    vary = c.kw.get("alpha", 5/3) is None
    tol = ck.tolerances()
    assert tol["_made_by"] == "tests/golden/make_acf2d_tolerances.py" and tol["_factor"] == 10
    made = tol["_oracle_per_case"][name]
    assert made["kind"] == c.kind and made["problems"] == len(fits)
    for s, f in zip(setups, fits):
        assert f["success"], name
        g, chi = ao.stationarity([f[k] for k in cc.FIT_KEYS], s, vary)
        assert g <= tol[c.kind]["stationarity"] * chi
    if c.planted is not None:
        got = np.array([[f[k] for k in cc.FIT_KEYS] for f in fits])
        assert np.abs(got / c.planted - 1).max() <= tol["a"]["values_rtol"]


def test_committed_tolerances_are_the_makers():
    tol = ck.tolerances()
    for kind in ("a", "b"):
        cases = [m for m in tol["_oracle_per_case"].values() if m["kind"] == kind]
        assert tol[kind]["stationarity"] == 10 * max(m["stationarity"] for m in cases)
        for slot in ("values_rtol", "phasegrad_tol", "errors_rtol"):
            assert tol[kind][slot] == 10 * max(max(m[slot] for m in cases), tol["_floor"])
