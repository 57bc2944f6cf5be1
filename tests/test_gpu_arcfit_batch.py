"""GPU checks of the batched arc fit (scint_arc_profile_batch, scint_arc_peak_fit, arcfit.fit_arc_stack_device, Dynspec.fit_arc_cut):
problem for problem the bits of the single calls, the decisions of arcfit._arc_peak, the values of the long-double parabola.  The
checks are tests/arcfit_batch_checks.py; the cases, and why these shapes, tests/arcfit_batch_cases.py."""
import pytest

import arcfit_batch_cases as cc
import arcfit_batch_checks as ck

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def af():
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
