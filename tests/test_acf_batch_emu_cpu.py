"""The batched ACF -- scint_acf_batch, scintpar.acf_stack_device, and cut_dyn / fit_scint_params_cut / fit_scint_params_2d_cut on
it -- interpreted on the host (tests/emu) through the same C ABI and Python wrappers as on a GPU.  The checks are those of the GPU
tests (tests/acf_batch_checks.py).  Runs without a GPU."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)
import acf_batch_cases as cc  # noqa: E402
import acf_batch_checks as ck  # noqa: E402


@pytest.fixture()
def sp(monkeypatch):
    import emulated
    emulated.install(monkeypatch)
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
