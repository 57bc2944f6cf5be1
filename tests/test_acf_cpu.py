"""Host-only tests of the theoretical 2-D ACF model: the direct-sum oracle (tests/acf_oracle.py) pinned bit for bit to the unmodified
reference's outputs (tests/golden/acf.npz), and the host parts of scintools_amd.scint_sim.ACF and scint_models.scint_acf_model_2d --
axes, grid lengths, mirroring, exceptions, the residual's arithmetic -- with the device call replaced by the oracle's field.  No GPU
and no interpreter: the kernels are tested by tests/test_acf_emu_cpu.py and tests/test_gpu_acf.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import acf_cases as ac  # noqa: E402
import acf_checks as ck  # noqa: E402
import acf_oracle as ao  # noqa: E402


@pytest.fixture(scope="module")
def gold(golden):
    return golden("acf.npz")


@pytest.fixture()
def host_acf(monkeypatch):
    """scint_sim with ACF's device call answered by the oracle's direct sums for the same grids."""
    from scintools_amd import scint_sim
    seen = []

    def field(snp, snp2, snx, sny, dnun, sigxn, sigyn, sqrtar, alph2, step, step2):
        seen.append(dict(m=len(snp), m2=len(snp2), nsn=len(snx), ndnun=len(dnun)))
        out = np.zeros((len(snx), len(dnun)), dtype=np.complex128)
        for idn in range(1, len(dnun)):
            grid, st = (snp2, step2) if idn == 1 else (snp, step)
            X, Y, G = ao.efield_plane(grid, sqrtar, alph2)
            cx, cy = snx - 2 * sigxn * dnun[idn], sny - 2 * sigyn * dnun[idn]
            for isn in range(len(snx)):
                arg = ((X - cx[isn])**2 + (Y - cy[isn])**2) / (2 * dnun[idn])
                out[isn, idn] = -1j * (st**2 * np.sum(G * np.exp(1j * arg)) / ((2 * np.pi) * dnun[idn]))
        return out, ao.efield_plane(snp, sqrtar, alph2)[2]

    monkeypatch.setattr(scint_sim.ACF, "_device_field", staticmethod(field))
    scint_sim._seen = seen
    return scint_sim


@pytest.mark.parametrize("case", list(ac.CASES))
def test_oracle_is_the_reference_bit_for_bit(gold, case):
    o = ck.oracle(**ac.kwargs(case))
    for k in ("acf", "acf_efield", "fn", "tn", "snp"):
        assert np.array_equal(o[k], gold[f"{case}_{k}"]), k
    assert np.all(o["scale"][1:] > 0) and o["field"].shape == (len(o["tn"]) if ac.kwargs(case).get("phasegrad") else (len(o["tn"]) + 1) // 2,
                                                                len(o["dnun"]))


@pytest.mark.parametrize("case", list(ac.CASES))
def test_host_parts_against_reference(host_acf, gold, case):
    """Axes, grid lengths, scalars, the dnun = 0 column, the spike and the mirroring: with the oracle's field the ACF is the reference's."""
    a = host_acf.ACF(**ac.kwargs(case))
    for k in ac.ARRAYS:
        assert np.array_equal(getattr(a, k), gold[f"{case}_{k}"]), k
    for k in ac.SCALARS:
        assert getattr(a, k) == gold[f"{case}_{k}"][()], k
    o = ck.oracle(**ac.kwargs(case))
    assert host_acf._seen[-1] == dict(m=len(o["snp"]), m2=len(o["snp2"]), nsn=o["field"].shape[0], ndnun=len(o["dnun"]))
    assert np.array_equal(a.gammitv, o["field"])


def test_grid_lengths_cover_the_tile_classes():
    """What the cases exercise: column counts below, just past and at two 16-column groups; grids that are no multiple of the tile."""
    nsn = sorted({ck.oracle(**ac.kwargs(c))["field"].shape[0] for c in ac.CASES})
    assert nsn == [3, 7, 11, 16, 17, 25, 26]
    lens = [(len(ck.oracle(**ac.kwargs(c))["snp"]), len(ck.oracle(**ac.kwargs(c))["snp2"])) for c in ac.CASES]
    assert max(m for m, _ in lens) == 76 and max(m2 for _, m2 in lens) == 301 and sum(m2 > 128 for _, m2 in lens) >= 4
    assert all(m2 % 16 for _, m2 in lens)


def test_exceptions_of_the_reference(host_acf):
    ck.check_errors(host_acf, pytest)


def test_calc_sspec(host_acf):
    ck.check_sspec(host_acf, "host")


@pytest.mark.parametrize("case", list(ac.MODEL_CASES))
def test_oracle_residual_is_the_reference(gold, case):
    pars, ydata, weights = ac.model_inputs(case)
    o = ck.oracle(**ck.model_kwargs(pars, ydata.shape))
    resid = ao.scint_acf_model_2d(pars, ydata, weights.copy(), o["acf"])[0]
    assert np.array_equal(resid, gold[f"{case}_resid"])


def test_scint_acf_model_2d_arithmetic_with_a_stubbed_model(monkeypatch):
    """The residual around a known model array: triangles, the zeroed white-noise weight, both kinds of params, weights=None."""
    from scintools_amd import scint_models
    calls = []

    class Stub:
        def __init__(self, **kw):
            calls.append(kw)
            self.acf = np.full((kw["nf"], kw["nt"]), 2.0)

    monkeypatch.setattr(scint_models, "ACF", Stub)
    pars = dict(tau=-200.0, dnu=-2.0, alpha=1.6, ar=-1.5, psi=10.0, phasegrad=0.1, theta=5.0, amp=2.0, tobs=1000.0, bw=32.0, nt=50, nf=40)
    ydata = np.arange(35.0).reshape(5, 7)
    got = scint_models.scint_acf_model_2d(ac.Params(pars), ydata, None)
    kw = calls[-1]
    taumax, dnumax = 7 * (2 * 1000.0 / 50) / 200.0, 5 * (2 * 32.0 / 40) / 2.0
    assert kw == dict(taumax=taumax, dnumax=dnumax, nt=7, nf=5, ar=1.5, alpha=1.6, phasegrad=0.1, theta=5.0, amp=2.0, psi=10.0)
    tri = np.outer(1 - np.abs(np.linspace(-dnumax * 2.0, dnumax * 2.0, 5)) / 32.0, 1 - np.abs(np.linspace(-taumax * 200.0, taumax * 200.0, 7)) / 1000.0)
    want = ydata - 2.0 * tri
    want[2, 3] = 0.0
    assert got.shape == (5, 7) and np.allclose(got, want, rtol=1e-15, atol=0) and got[2, 3] == 0
    w = np.full((5, 7), 3.0)
    assert np.array_equal(scint_models.scint_acf_model_2d(pars, ydata, w), 3.0 * got)
    assert np.array_equal(scint_models.scint_acf_model_2d(pars, ydata, w), ao.scint_acf_model_2d(pars, ydata, np.full((5, 7), 3.0), np.full((5, 7), 2.0))[0])
