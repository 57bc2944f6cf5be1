"""The cleaning methods without a GPU: the NumPy / SciPy restatement (tests/clean_oracle.py) against the unmodified reference's
outputs (tests/golden/clean.npz), the host-only methods of the port (trim_edges, crop_dyn) against the same, and the error paths
that need no device."""
import inspect
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import clean_cases as cc  # noqa: E402
import clean_checks as ck  # noqa: E402
import clean_oracle as co  # noqa: E402


@pytest.fixture(scope="module")
def gold(golden):
    return golden("clean.npz")


def _oracle_steps(case):
    kind, steps = cc.CASES[case]
    o = cc.observation(kind)
    for k, (method, kw) in enumerate(steps):
        before = np.array(o.dyn)
        if method == "refill":
            before[before == 0] = np.nan
        if method == "correct_dyn":
            before[np.isnan(before)] = 0
        co.METHODS[method](o, **{a: v for a, v in kw.items()})
        yield k, method, kw, before, o


@pytest.mark.parametrize("case", list(cc.CASES))
def test_oracle_against_reference(gold, case):
    """Every stored attribute after every step; the linear fill within K_LINEAR_ORACLE eps of griddata (this measures it)."""
    for k, method, kw, before, o in _oracle_steps(case):
        for name in cc.ATTRS[1:]:
            assert ck.same_bits(getattr(o, name), gold[f"{case}_{k}_{name}"]), (case, k, name)
        if f"{case}_{k}_dyn" not in gold.files:
            continue
        ref = gold[f"{case}_{k}_dyn"]
        if method == "refill" and kw.get("method", "biharmonic") in ("linear", "biharmonic"):
            scale = co.brackets(before)
            gap = scale > 0
            K = np.max(np.abs(o.dyn - ref)[gap] / (ck.EPS * scale[gap]))
            print(f"{case}: the restatement against griddata, K = {K:.3f}")
            assert gap.sum() >= 3 * min(ref.shape) and K <= ck.K_LINEAR_ORACLE and ck.same_bits(o.dyn[~gap], ref[~gap])
        elif method == "correct_dyn" and kw.get("svd", True):
            s = gold[f"{case}_sv"]
            ck.assert_svd(f"{case} oracle", s, kw.get("nmodes", 1), before, o.svd_model, gold[f"{case}_{k}_svd_model"], o.dyn, ref)
        elif method == "correct_dyn":
            ck.assert_nosvd(f"{case} oracle", o.dyn, ref, sum(ref.shape))
        else:
            assert ck.same_bits(o.dyn, ref), (case, k, method)


def test_golden_svd_gaps(gold):
    """The stored SVD cases have a relative gap of at least 0.5 at their nmodes, and so has every generated matrix."""
    for case, nmodes in cc.SVD_CASES.items():
        s = gold[f"{case}_sv"]
        assert len(s) == nmodes + 1 and 1 - (s[nmodes] / s[nmodes - 1]) ** 2 >= 0.5
    for nf, nt, nmodes in ck.SVD_SHAPES:
        for nans in (False, True):
            s = np.linalg.svd(np.nan_to_num(cc.svd_matrix(nf, nt, nmodes, seed=nf + nt + nmodes, nans=nans)), compute_uv=False)
            for k in range(1, min(nmodes, len(s) - 1) + 1):
                assert 1 - (s[k] / s[k - 1]) ** 2 >= 0.5, (nf, nt, nmodes, k)
    s = np.linalg.svd(cc.complex_matrix(), compute_uv=False)
    assert 1 - (s[1] / s[0]) ** 2 >= 0.5 and 1 - (s[2] / s[1]) ** 2 >= 0.5


def test_golden_cases_cover_the_issue(gold):
    o = cc.observation("channels")
    assert o.dyn.shape == (48, 40) and (o.dyn >= 0).all()
    assert not o.dyn[0].any() and not o.dyn[-1].any() and not o.dyn[:, 0].any() and not o.dyn[[10, 25, 26]].any()
    assert not cc.observation("subints").dyn[:, [8, 20, 21]].any()
    assert gold["chan_zap_1_dyn"].shape == (46, 39) and np.isnan(gold["chan_zap_1_dyn"]).sum() == 4      # the four spikes
    assert [m for m, _ in cc.CASES["chain"][1]] == ["trim_edges", "zap", "refill", "correct_dyn"]


@pytest.mark.parametrize("case", ["chan_zap", "crop"])
def test_host_methods_against_reference(gold, case):
    """trim_edges and crop_dyn of the port need no device: the reference's bits, attributes and roundings included."""
    from scintools_amd.dynspec import Dynspec
    kind, steps = cc.CASES[case]
    d = Dynspec(dyn=cc.observation(kind), verbose=False)
    for k, (method, kw) in enumerate(steps):
        if method not in ("trim_edges", "crop_dyn"):
            break
        getattr(d, method)(**kw)
        for name in cc.ATTRS[1:]:
            assert ck.same_bits(getattr(d, name), gold[f"{case}_{k}_{name}"]), (case, k, name)
        if f"{case}_{k}_dyn" in gold.files:
            assert ck.same_bits(d.dyn, gold[f"{case}_{k}_dyn"])
    if case == "chan_zap":                                # the trimmed array itself is stored with the chain case
        assert ck.same_bits(d.dyn, gold["chain_0_dyn"])


def test_trim_edges_original_size_threshold_and_all_zero():
    from scintools_amd.dynspec import Dynspec
    o = cc.observation()
    o.dyn[1, ::2] = 0.0                                   # half of the second channel: 20 zeros of 40 is not MORE than half
    o.dyn[2, :21] = 0.0
    d = Dynspec(dyn=o, verbose=False)
    d.trim_edges()
    r = cc.observation()
    r.dyn[1, ::2] = 0.0
    r.dyn[2, :21] = 0.0
    co.trim_edges(r)
    assert ck.same_bits(d.dyn, r.dyn) and d.dyn.shape[0] == 46
    z = cc.observation()
    z.dyn[:] = 0.0
    with pytest.raises(ValueError, match="zero everywhere"):
        Dynspec(dyn=z, verbose=False).trim_edges()
    z = cc.observation()
    z.dyn[:, 1::2] = np.nan                               # every line is half empty: bandwagon_frac=0.4 trims all of them
    with pytest.raises(ValueError, match="trimmed"):
        Dynspec(dyn=z, verbose=False).trim_edges(bandwagon_frac=0.4)


def test_signatures_and_exports():
    from scintools_amd import clean, ththmod
    from scintools_amd.dynspec import Dynspec
    want = {
        "zap": dict(sigma=7),
        "refill": dict(method='biharmonic', zeros=True, kernel_size=5, linear=True),
        "correct_dyn": dict(svd=True, nmodes=1, frequency=True, time=True, lamsteps=False, nsmooth=None, velocity=False),
        "trim_edges": dict(bandwagon_frac=0.5, remove_short_sub=True),
        "crop_dyn": dict(fmin=0, fmax=np.inf, tmin=0, tmax=np.inf),
        "auto_processing": dict(lamsteps=False, remove_short_sub=True),
    }
    for name, kw in want.items():
        sig = inspect.signature(getattr(Dynspec, name))
        assert {k: v.default for k, v in sig.parameters.items() if k != "self"} == kw, name
    assert [p for p in inspect.signature(ththmod.svd_model).parameters][:2] == ["arr", "nmodes"]
    assert clean.SVD_TOL == ththmod.DEFAULT_TOL
    with pytest.raises(NotImplementedError):
        Dynspec(dyn=cc.observation(), process=True, verbose=False)


def test_no_gpu_no_fallback():
    """Without a GPU the device methods raise (after the argument checks); they never compute on the host."""
    import torch
    from scintools_amd import _lib, ththmod
    from scintools_amd.dynspec import Dynspec
    d = Dynspec(dyn=cc.observation(), verbose=False)
    with pytest.raises(ValueError, match="should be odd"):
        d.refill(method="median", kernel_size=4)
    with pytest.raises(ValueError, match="at most 4"):
        d.correct_dyn(nmodes=5)
    with pytest.raises(NotImplementedError):
        d.correct_dyn(velocity=True)
    if not torch.cuda.is_available():
        for call in (lambda: d.zap(), lambda: d.refill(method="median", kernel_size=3), lambda: d.correct_dyn(),
                     lambda: d.correct_dyn(svd=False), lambda: ththmod.svd_model(np.ones((4, 5)))):
            with pytest.raises(_lib.ScintHipError):
                call()


def test_library_exports_the_new_symbols():
    from scintools_amd import _lib
    names = ("scint_zap", "scint_zap_workspace_bytes", "scint_refill_median", "scint_refill_linear", "scint_svd_model",
             "scint_svd_model_workspace_bytes", "scint_nanmean_axis", "scint_nanmean_axis_workspace_bytes", "scint_divide_axis")
    assert set(names) <= set(_lib.header_symbols()) and set(names) <= set(_lib._SIGNATURES)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in names) and lib.scint_version() == 108
