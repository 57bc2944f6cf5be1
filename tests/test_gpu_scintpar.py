"""GPU checks of the no-fit scintillation measurements (scintools_amd/scintpar.py, csrc/scintpar.hpp): what the device hands
over is the ACF's own bits, the host arithmetic on it is the oracle's (exact), and the results agree with the unmodified
reference's (tests/golden/scintpar.npz) within what a 1e-12 difference of the ACF allows."""
import json
import os

import numpy as np
import pytest

import scintpar_cases as cc
import scintpar_oracle as so

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g(golden):
    return golden("scintpar.npz")


@pytest.fixture(scope="module")
def gcut(golden):
    return golden("scintpar_cut.npz")


@pytest.fixture(scope="module")
def tol():
    with open(os.path.join(os.path.dirname(__file__), "golden", "scintpar_tolerances.json")) as fh:
        return json.load(fh)


def _dynspec(obs):
    from scintools_amd.dynspec import Dynspec
    return Dynspec(dyn=obs, verbose=False)


def _device_acf(d):
    """The parked ACF as a device tensor, without handing it to the host."""
    return type(d).acf.tensor(d)


@pytest.mark.parametrize("case", cc.OBS)
def test_scales_and_tilt(g, tol, case):
    """64 x 96 (even), 75 x 101 (odd centre indices and halves), 192 x 256 (several workgroups), 24 x 40."""
    import torch
    from scintools_amd import scintpar
    o = cc.from_golden(g, case)
    d = _dynspec(o)
    assert not hasattr(d, "acf")
    d.get_acf_tilt(method='nofit')             # -> calc_acf -> get_scint_params(method='nofit')
    assert type(d).acf.present(d) and d.__dict__["_devbacked_acf"][0] is None        # still parked: nothing was downloaded
    acf_t = _device_acf(d)
    cut_f, cut_t = scintpar.acf_cuts_device(acf_t)
    rows = so.tilt_rows(tuple(acf_t.shape), o, d.dnu)[:, 0]
    cols, wins, flags = scintpar.acf_row_peaks_device(acf_t, rows)
    count, mean, var = scintpar.dyn_moments_device(scintpar.device.to_device(o.dyn, torch.float64))
    acf = d.acf                                # the one download
    assert d.__dict__["_devbacked_acf"][1] is None and acf.shape == (2 * o.dyn.shape[0], 2 * o.dyn.shape[1])
    nf, nt = acf.shape
    # cuts and windows: the same elements of the downloaded ACF, exactly
    assert np.array_equal(cut_f, acf[int(nf/2):, int(nt/2)]) and np.array_equal(cut_t, acf[int(nf/2), int(nt/2):])
    assert np.array_equal(cols, np.argmax(acf[rows], axis=1)) and not flags.any()
    assert np.array_equal(wins, np.stack([acf[r, c - 3:c + 4] for r, c in zip(rows, cols)]))
    # moments against NumPy
    keep = np.isfinite(o.dyn) & (o.dyn != 0)
    print(case, "moments", count, mean, var, "numpy", keep.sum(), np.mean(o.dyn[keep]), np.var(o.dyn[keep]))
    assert count == keep.sum()
    np.testing.assert_allclose([mean, var], [np.mean(o.dyn[keep]), np.var(o.dyn[keep])], rtol=1e-12)
    # every attribute equals the oracle applied to the DEVICE's ACF (and moments), exactly
    for variant, kw in cc.VARIANTS.items():
        d.get_scint_params(method='nofit', **kw)
        p = so.nofit_from_moments(acf, mean, var, o, **kw)
        for name in cc.NOFIT_ATTRS:
            assert getattr(d, name) == p[name], (variant, name)
        assert d.scint_param_method == 'nofit'
        # ... and the reference's: grid-valued tau and dnu equal, the others smooth functions of an ACF that agrees to 1e-12
        for name in cc.NOFIT_ATTRS:
            ref = float(g[f"{case}_{variant}_{name}"])
            print(case, variant, name, getattr(d, name), ref)
            if name in cc.GRID_ATTRS:
                assert getattr(d, name) == ref, (variant, name)
            else:
                np.testing.assert_allclose(getattr(d, name), ref, rtol=1e-9, err_msg=f"{variant} {name}")
    d.get_scint_params(method='nofit')
    tilt = so.acf_tilt(acf, o, d.tau, d.dnu)
    assert (d.acf_tilt, d.acf_tilt_err, d.fse_tilt) == tilt
    for name in cc.TILT_ATTRS:
        ref, allowed = float(g[f"{case}_tilt_{name}"]), 10 * tol["tilt_spread"][case][name]
        print(case, name, getattr(d, name), ref, "allowed", allowed)
        assert abs(getattr(d, name) - ref) <= allowed, name
    # after the host read the ACF is re-uploaded when it is needed again: the same answer
    d.get_acf_tilt(method='nofit')
    assert (d.acf_tilt, d.acf_tilt_err, d.fse_tilt) == tilt


def test_moments_skip_nan_inf_and_zero(g):
    import torch
    from scintools_amd import scintpar
    o = cc.from_golden(g, "even")
    d = _dynspec(o)
    d.calc_acf()
    d.dyn = cc.poke_holes(d.dyn)
    d.get_scint_params(method='nofit')
    keep = np.isfinite(d.dyn) & (d.dyn != 0)
    count, mean, var = scintpar.dyn_moments_device(scintpar.device.to_device(d.dyn, torch.float64))
    assert count == keep.sum() == d.dyn.size - 84 - 1 - 80
    np.testing.assert_allclose([mean, var], [np.mean(d.dyn[keep]), np.var(d.dyn[keep])], rtol=1e-12)
    p = so.nofit_from_moments(d.acf, mean, var, o)
    for name in cc.NOFIT_ATTRS:
        assert getattr(d, name) == p[name], name
        if name in cc.GRID_ATTRS:
            assert getattr(d, name) == float(g[f"holes_{name}"])
        else:
            np.testing.assert_allclose(getattr(d, name), float(g[f"holes_{name}"]), rtol=1e-9, err_msg=name)
    # nothing valid at all: count 0 and NaN, as np.mean of an empty selection
    count, mean, var = scintpar.dyn_moments_device(scintpar.device.to_device(np.full((3, 5), np.nan), torch.float64))
    assert count == 0 and np.isnan(mean) and np.isnan(var)


def test_row_maximum_ties_take_the_first_column(g):
    """Exact ties inside a wavefront, across wavefronts and across a thread's strides resolve to the lowest column."""
    import torch
    from scintools_amd import scintpar
    acf = cc.tie_acf()
    rows = np.arange(acf.shape[0])
    cols, wins, flags = scintpar.acf_row_peaks_device(scintpar.device.to_device(acf, torch.float64), rows)
    assert np.array_equal(cols, np.argmax(acf, axis=1)) and not flags.any()
    for row in cc.tie_rows():
        assert cols[row] == np.flatnonzero(acf[row] == acf[row].max())[0]
    assert np.array_equal(wins, np.stack([acf[r, c - 3:c + 4] for r, c in zip(rows, cols)]))
    o = cc.synthetic_observation()
    d = _dynspec(o)
    d.acf = acf
    d.get_acf_tilt(method='nofit')
    p = so.nofit(acf, o.dyn, o)
    assert (d.tau, d.dnu) == (p["tau"], p["dnu"]) == (float(g["tie_tau"]), float(g["tie_dnu"]))
    assert (d.acf_tilt, d.acf_tilt_err, d.fse_tilt) == so.acf_tilt(acf, o, d.tau, d.dnu)
    # the same ACF on both sides: only the platform's polyfit (LAPACK) can differ from the stored run
    np.testing.assert_allclose([d.acf_tilt, d.acf_tilt_err, d.fse_tilt], [float(g[f"tie_{n}"]) for n in cc.TILT_ATTRS], rtol=1e-9)


def test_window_across_an_edge_is_flagged_not_read():
    import torch
    from scintools_amd import scintpar
    acf = cc.edge_acf()
    R, C = acf.shape
    bad = R // 2 + 1
    acf[2, C - 2] = 3.0                          # and one at the far edge
    cols, wins, flags = scintpar.acf_row_peaks_device(scintpar.device.to_device(acf, torch.float64), np.arange(R))
    assert np.array_equal(cols, np.argmax(acf, axis=1)) and cols[bad] == 1 and cols[2] == C - 2
    assert flags[bad] == 1 and flags[2] == 1 and flags.sum() == 2
    assert not wins[bad].any() and not wins[2].any()
    with pytest.raises(ValueError, match="outside the ACF"):
        scintpar.acf_row_peaks_device(scintpar.device.to_device(acf, torch.float64), [0, R])
    d = _dynspec(cc.synthetic_observation())
    d.acf = cc.edge_acf()
    with pytest.raises(ValueError, match=f"row {bad} lies within 3 columns of the edge"):
        d.get_acf_tilt(method='nofit')


@pytest.mark.parametrize("case", sorted(cc.CUTS))
def test_cut_dyn(g, gcut, case):
    """cut_dyn(3, 2) on 130 x 203: 43 x 50 segments, remainders dropped, ACF lengths 86 x 100 (no powers of two), spectrum
    lengths padded to 64 x 128; and cut_dyn(0, 0).  Tolerances: those of the calc_sspec and calc_acf parity tests."""
    o = cc.from_golden(g, case)
    tcuts, fcuts = cc.CUTS[case]
    d = _dynspec(o)
    d.cut_dyn(tcuts=tcuts, fcuts=fcuts, lamsteps=(case == "small"))
    ref_dyn, ref_sspec = gcut[f"{case}_cutdyn"], gcut[f"{case}_cutsspec"]
    assert np.array_equal(d.cutdyn, ref_dyn)
    assert d.cutsspec.shape == ref_sspec.shape
    _, _, ref_acf = so.cut_dyn(o.dyn, len(o.freqs), len(o.times), tcuts, fcuts)
    assert d.cutacf.shape == ref_acf.shape
    for ii in range(fcuts + 1):
        for jj in range(tcuts + 1):
            lin, lref = 10 ** (d.cutsspec[ii, jj] / 10), 10 ** (ref_sspec[ii, jj] / 10)
            assert np.abs(lin - lref).max() <= 1e-10 * lref.max(), (ii, jj)
            strong = lref > 1e-6 * lref.max()
            assert np.abs(d.cutsspec[ii, jj] - ref_sspec[ii, jj])[strong].max() <= 1e-8, (ii, jj)
            assert np.abs(d.cutacf[ii, jj] - ref_acf[ii, jj]).max() <= 1e-12, (ii, jj)


def test_calc_acf_sspec(g, tol):
    from scintools_amd.dynspec import Dynspec  # noqa: F401
    for case in cc.SSPEC_ACF:
        o = cc.from_golden(g, case)
        d = _dynspec(o)
        d.calc_acf(method='sspec')
        ref = g[f"{case}_acf_sspec"]
        assert d.acf.shape == ref.shape
        err = np.abs(d.acf - ref).max() / np.abs(ref).max()
        print(case, "acf(sspec) error / max", err)
        assert err <= tol["acf_sspec_bound"][case]["bound"]
        raw = d.calc_acf(method='sspec', input_dyn=o.dyn, normalise=False, window_frac=0.2)
        oref = so.acf_sspec(o.dyn, normalise=False, window_frac=0.2)
        assert isinstance(raw, np.ndarray) and np.abs(raw - oref).max() <= 1e-10 * np.abs(oref).max()
    # a larger frame (the maximum spans several workgroups) against the oracle
    o = cc.from_golden(g, "odd")
    d = _dynspec(o)
    d.calc_acf(method='sspec')
    oref = so.acf_sspec(o.dyn)
    assert d.acf.shape == oref.shape == (256, 256) and np.abs(d.acf - oref).max() <= 1e-10 * np.abs(oref).max()


def test_acf_sspec_of_an_exact_zero_of_power():
    """-inf dB maps to 0, not NaN."""
    import torch
    from scintools_amd import scintpar
    rng = np.random.default_rng(3)
    sec = 10 * np.log10(rng.random((32, 64)) + 0.1)
    sec[5, 7] = -np.inf
    out = scintpar.acf_from_sspec_device(scintpar.device.to_device(sec, torch.float64), normalise=False).cpu().numpy()
    ref = np.real(np.fft.fftshift(np.fft.fft2(10 ** (np.fft.fftshift(sec) / 10))))
    assert np.isfinite(out).all() and np.abs(out - ref).max() <= 1e-10 * np.abs(ref).max()
