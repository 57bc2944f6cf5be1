"""The batched arc fit -- scint_arc_profile_batch, scint_arc_peak_fit, arcfit.fit_arc_stack_device, Dynspec.fit_arc_cut --
interpreted on the host (tests/emu) through the same C ABI and Python wrappers as on a GPU.  The checks are those of the GPU tests
(tests/arcfit_batch_checks.py).  Runs without a GPU."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)
import arcfit_batch_cases as cc  # noqa: E402
import arcfit_batch_checks as ck  # noqa: E402


@pytest.fixture()
def af(monkeypatch):
    import emulated
    emulated.install(monkeypatch)
    from scintools_amd import arcfit
    return arcfit


@pytest.mark.parametrize("name", cc.CASES)
def test_every_problem_has_the_bits_of_the_single_calls(af, name):
    ck.check_bits_of_the_single_calls(af, name)


def test_a_problem_does_not_leak_into_its_neighbours(af):
    ck.check_leak(af)


@pytest.mark.parametrize("name", ["r33", "b37", "long"])
def test_deterministic_and_reversible(af, name):
    ck.check_deterministic(af, name)


def test_peak_fit_decisions_and_values(af):
    stats = dict(profiles=0, excluded=0)
    for log_parabola in (False, True):
        for asymm in (False, True):
            ck.check_peak_bumps(af, log_parabola, asymm, stats)
    ck.check_peak_synthetic(af, stats)
    for name in cc.CASES:
        ck.check_peak_on_case(af, name, stats)
    ck.check_excluded(stats)


@pytest.mark.parametrize("asymm,log_parabola", [(False, False), (True, False), (False, True)])
def test_end_to_end_against_fit_arc(af, asymm, log_parabola):
    ck.check_end_to_end(af, asymm, log_parabola)


def test_fit_arc_cut(af, monkeypatch):
    ck.check_fit_arc_cut(af, monkeypatch, pytest)


def test_arguments(af):
    ck.check_arguments(af, pytest)


def test_c_entry_point_status(af):
    ck.check_c_status(af)
