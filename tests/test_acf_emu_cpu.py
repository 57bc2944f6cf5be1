"""The theoretical 2-D ACF model -- scint_acf_model, scintools_amd.scint_sim.ACF and scint_models.scint_acf_model_2d -- interpreted on
the host (tests/emu) through the same C ABI and Python wrappers as on a GPU, against the reference's outputs (tests/golden/acf.npz)
and the direct-sum oracle (tests/acf_oracle.py).  The checks are those of the GPU tests (tests/acf_checks.py).  Runs without a GPU."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)
import acf_cases as ac  # noqa: E402
import acf_checks as ck  # noqa: E402


@pytest.fixture()
def emu(monkeypatch):
    import emulated
    emulated.install(monkeypatch)
    from scintools_amd import scint_sim
    return scint_sim


@pytest.fixture(scope="module")
def gold(golden):
    return golden("acf.npz")


@pytest.mark.parametrize("case", list(ac.CASES))
def test_against_reference(emu, gold, case):
    ck.check_golden(emu, "emu", gold, case)


@pytest.mark.parametrize("case", ["c", "e", "g"])
def test_field_against_oracle(emu, case):
    ck.check_field(emu, "emu", case)


@pytest.mark.parametrize("case", list(ac.CASES))
def test_symmetry(emu, case):
    ck.check_symmetry(emu, "emu", case)


def test_deterministic(emu):
    ck.check_deterministic(emu)


@pytest.mark.parametrize("case", list(ac.MODEL_CASES))
def test_scint_acf_model_2d(emu, gold, case):
    from scintools_amd import scint_models
    ck.check_model_2d(scint_models, gold, case)


def test_errors_and_plot_warnings(emu):
    ck.check_errors(emu, pytest)


def test_calc_sspec(emu):
    ck.check_sspec(emu, "emu")
