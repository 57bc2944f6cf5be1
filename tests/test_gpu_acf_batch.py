"""GPU checks of the batched ACF (scint_acf_batch, scintpar.acf_stack_device) and of what runs on it (cut_dyn, fit_scint_params_cut,
fit_scint_params_2d_cut): problem for problem the bits of the single call.  The checks are tests/acf_batch_checks.py; the cases,
and why these shapes, tests/acf_batch_cases.py."""
import pytest

import acf_batch_cases as cc
import acf_batch_checks as ck

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sp():
    from scintools_amd import scintpar
    return scintpar


@pytest.mark.parametrize("name", cc.CASES)
def test_every_problem_has_the_bits_of_the_single_call(sp, name):
    ck.check_bits_of_the_single_call(sp, name)


@pytest.mark.parametrize("name", cc.CASES)
def test_against_numpy(sp, name):
    ck.check_against_numpy(sp, name)


def test_mean_and_maximum_stay_with_their_problem(sp):
    ck.check_leak(sp)


@pytest.mark.parametrize("name", ["b37", "odd", "groups"])
def test_deterministic(sp, name):
    ck.check_deterministic(sp, name)


def test_out_is_filled_in_place(sp):
    ck.check_out(sp)


def test_arguments(sp):
    ck.check_arguments(sp, pytest)


def test_c_entry_point_status(sp):
    ck.check_c_status(sp)


@pytest.mark.parametrize("name", cc.SSPEC_CASES)
def test_every_secondary_spectrum_has_the_bits_of_the_single_call(sp, name):
    ck.check_sspec_bits_of_the_single_call(sp, name)


def test_sspec_stack_arguments(sp):
    ck.check_sspec_arguments(sp, pytest)


def test_cut_dyn_keeps_its_bits_and_stays_on_the_device(sp):
    ck.check_cut_dyn(sp)


def test_cut_fits_keep_their_bits(sp):
    ck.check_cut_fits(sp)
