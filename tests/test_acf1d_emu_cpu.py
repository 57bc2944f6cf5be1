"""The batched 1-D ACF fit -- scint_acf1d_fit, scintpar.acf1d_fit_device, Dynspec.fit_scint_params and fit_scint_params_cut --
interpreted on the host (tests/emu) through the same C ABI and Python wrappers as on a GPU, against the host oracle
(tests/acf1d_oracle.py).  The checks are those of the GPU tests (tests/acf1d_checks.py).  Runs without a GPU."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)
import acf1d_cases as cc  # noqa: E402
import acf1d_checks as ck  # noqa: E402


@pytest.fixture()
def sp(monkeypatch):
    import emulated
    emulated.install(monkeypatch)
    from scintools_amd import scintpar
    return scintpar


@pytest.mark.parametrize("name", cc.CASES)
def test_start_values_crop_and_weights(sp, name):
    ck.check_setup(sp, name)


@pytest.mark.parametrize("name", cc.CASES)
def test_fit_is_stationary_and_agrees_with_the_oracle(sp, name):
    ck.check_fit(sp, name)


def test_status_paths(sp):
    ck.check_status_paths(sp)


@pytest.mark.parametrize("name", ["real12_alpha", "long", "wave65"])
def test_deterministic(sp, name):
    ck.check_deterministic(sp, name)


@pytest.mark.parametrize("alpha", [5/3, None])
def test_fit_scint_params(sp, alpha):
    ck.check_dynspec(sp, alpha)


def test_fit_scint_params_that_does_not_converge(sp):
    ck.check_dynspec_not_converged(sp, pytest)


def test_fit_scint_params_cut(sp):
    ck.check_cut(sp)


def test_arguments(sp):
    ck.check_arguments(sp, pytest)
