"""The batched approximate 2-D ACF fit -- scint_acf2d_approx_fit, scintpar.acf2d_approx_fit_device, Dynspec.fit_scint_params_2d and
fit_scint_params_2d_cut, scint_models.scint_acf_model_2d_approx -- interpreted on the host (tests/emu) through the same C ABI and
Python wrappers as on a GPU, against the host oracle (tests/acf2d_oracle.py).  The checks are those of the GPU tests
(tests/acf2d_checks.py).  Runs without a GPU."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)
import acf2d_cases as cc  # noqa: E402
import acf2d_checks as ck  # noqa: E402


@pytest.fixture()
def sp(monkeypatch):
    import emulated
    emulated.install(monkeypatch)
    from scintools_amd import scintpar
    return scintpar


@pytest.mark.parametrize("name", cc.CASES)
def test_windows_start_values_and_weights(sp, name):
    ck.check_setup(sp, name)


@pytest.mark.parametrize("name", cc.FIT_CASES)
def test_fit_is_stationary_and_agrees_with_the_oracle(sp, name):
    ck.check_fit(sp, name)


def test_bad_window(sp):
    ck.check_bad_window(sp)


def test_status_paths(sp):
    ck.check_status_paths(sp)


def test_fixed_tau(sp):
    ck.check_fixed_tau(sp)


@pytest.mark.parametrize("name", ["tilted", "real12_alpha"])
def test_deterministic(sp, name):
    ck.check_deterministic(sp, name)


@pytest.mark.parametrize("alpha", [5/3, None])
def test_fit_scint_params_2d(sp, alpha):
    ck.check_dynspec(sp, alpha)


def test_fit_scint_params_2d_that_does_not_converge(sp):
    ck.check_dynspec_not_converged(sp, pytest)


def test_fit_scint_params_2d_cut(sp):
    ck.check_cut(sp)


def test_model_against_the_reference(sp):
    ck.check_model(sp)


def test_arguments(sp):
    ck.check_arguments(sp, pytest)
