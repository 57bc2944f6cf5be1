"""GPU checks of the batched 1-D ACF fit (scint_acf1d_fit, scintpar.acf1d_fit_device, Dynspec.fit_scint_params and
fit_scint_params_cut) against the same least-squares problem solved on the host (tests/acf1d_oracle.py).  The checks are
tests/acf1d_checks.py; the cases, and why these shapes, tests/acf1d_cases.py."""
import pytest

import acf1d_cases as cc
import acf1d_checks as ck

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sp():
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


@pytest.mark.parametrize("name", ["real300", "long", "wave65"])
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
