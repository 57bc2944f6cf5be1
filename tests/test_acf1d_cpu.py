"""CPU checks of the 1-D ACF fit without a GPU and without the interpreter: the new names exist and raise the package's "no GPU"
error, get_scint_params still refuses the fitted methods, the case list keeps its promises (the oracle converges everywhere,
the committed tolerances are the maker's), and the entry point checks its arguments."""
import json
import os

import numpy as np
import pytest

import acf1d_cases as cc
import acf1d_checks as ck
import acf1d_oracle as ao


def _dynspec():
    from scintools_amd.dynspec import Dynspec
    return Dynspec(dyn=cc.observation(), verbose=False)


def test_new_names_exist_and_need_a_gpu():
    import torch
    from scintools_amd import _lib, build, scintpar
    from scintools_amd.dynspec import Dynspec
    assert Dynspec.fit_scint_params is scintpar.fit_scint_params and Dynspec.fit_scint_params_cut is scintpar.fit_scint_params_cut
    assert callable(scintpar.acf1d_fit_device) and "scint_acf1d_fit" in _lib.header_symbols()
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    build.build(verbose=False)
    d = _dynspec()
    for call in (d.fit_scint_params, lambda: d.fit_scint_params_cut(1, 2),
                 lambda: scintpar.acf1d_fit_device(torch.zeros((1, 16, 16), dtype=torch.float64), 30.0, 0.5, 4.0, 240.0)):
        with pytest.raises(_lib.ScintHipError):
            call()
    assert not hasattr(d, "scint_fit_status") and not hasattr(d, "cut_tau")


def test_get_scint_params_still_refuses_the_fitted_methods():
    d = _dynspec()
    for kw in (dict(method="acf1d"), {}):
        with pytest.raises(NotImplementedError, match=r"lmfit.*method='nofit'"):
            d.get_scint_params(**kw)


def test_entry_point_checks_its_arguments():
    import ctypes
    import torch
    from scintools_amd import _lib, build
    build.build(verbose=False)
    _lib.load()
    need = ctypes.c_size_t()
    _lib.call("scint_acf1d_fit_workspace_bytes", 4096, 128, 128, need)
    assert need.value >= 4096 * 2 * 128 * 8
    a = torch.zeros(8, dtype=torch.float64)
    i = torch.zeros(8, dtype=torch.int32)
    good = [a, 1, 16, 16, 30.0, 0.5, a, a, 5.0, 0, 1, 1, 5/3, 0, 200, a, a, a, i, i, None, a, 1 << 20, None]
    for pos, value, msg in ((0, None, "null"), (2, 4, "bad shape"), (1, 0, "bad shape"), (4, 0.0, "positive"),
                            (8, float("nan"), "nscale"), (14, 0, "max_iter"), (22, 8, "workspace")):
        args = list(good)
        args[pos] = value
        with pytest.raises(_lib.ScintHipError, match=msg):
            _lib.call("scint_acf1d_fit", *args)
    with pytest.raises(TypeError, match="status_out"):
        _lib.call("scint_acf1d_fit", *(good[:19] + [a] + good[20:]))       # float64 where int32 device memory goes


def test_shapes_of_the_case_list():
    """What the shapes are there for (tests/acf1d_cases.py)."""
    floor, _ = cc.oracle("floor5")
    assert len(floor) == 5 and all(len(s["x_t"]) == 6 and len(s["x_f"]) == 6 for s in floor)
    wave, _ = cc.oracle("wave65")
    assert all(len(s["x_t"]) == 65 and len(s["x_f"]) == 65 for s in wave) and cc.case("wave65").kw["alpha"] is None
    assert cc.case("odd").stack.shape[1:] == (37, 51)
    long_, _ = cc.oracle("long")
    assert all(len(s["x_t"]) == 3000 for s in long_)
    assert len(cc.case("real300").stack) == 300
    nc = cc.case("nocross")
    s, _ = cc.oracle("nocross")
    assert s[1]["tau"] == nc.tobs and s[1]["dnu"] == nc.bw and s[0]["tau"] < nc.tobs and s[2]["tau"] < nc.tobs


@pytest.mark.parametrize("name", cc.CASES)
def test_oracle_converges_on_every_case(name):
    c = cc.case(name)
    setups, fits = cc.oracle(name)
    vary = c.kw.get("alpha", 5/3) is None
    tol = ck.tolerances()
    assert tol["_made_by"] == "tests/golden/make_acf1d_tolerances.py" and tol["_factor"] == 10
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
    """Each kind's bound is 10 x the largest per-case figure the maker recorded (or the 64 eps floor)."""
    tol = ck.tolerances()
    for kind in ("a", "b"):
        cases = [m for m in tol["_oracle_per_case"].values() if m["kind"] == kind]
        assert tol[kind]["stationarity"] == 10 * max(m["stationarity"] for m in cases)
        for slot in ("values_rtol", "errors_rtol"):
            assert tol[kind][slot] == 10 * max(max(m[slot] for m in cases), tol["_floor"])
    assert json.dumps(tol)          # plain JSON
    assert os.path.exists(os.path.join(os.path.dirname(__file__), "golden", "make_acf1d_tolerances.py"))
