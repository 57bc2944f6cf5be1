"""The screen simulator -- scint_sim_screen, scint_sim_field, scint_sim_pulse and scintools_amd.scint_sim.Simulation -- interpreted
on the host (tests/emu) through the same C ABI and Python wrapper as on a GPU, against the reference's outputs
(tests/golden/sim.npz).  The checks are those of the GPU tests (tests/sim_checks.py).  Runs without a GPU."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)
import sim_checks as ck  # noqa: E402


@pytest.fixture()
def emu(monkeypatch):
    import emulated
    emulated.install(monkeypatch)
    from scintools_amd import scint_sim
    return scint_sim


@pytest.fixture(scope="module")
def gold(golden):
    return golden("sim.npz")


@pytest.mark.parametrize("case", ["a", "b", "c", "d", "f"])      # f: the one case whose 2 nf is a row-transform length (pulsewin)
def test_against_reference(emu, gold, case):
    ck.check_golden(emu, "emu", gold, case, pytest)


@pytest.mark.parametrize("case", ["b", "d"])
def test_shortcut_vs_full_transform(emu, gold, case):
    ck.check_shortcut(emu, gold, case)


def test_frequency_grouping(emu):
    ck.check_grouping(emu, "emu")


def test_errors(emu):
    ck.check_errors(emu, pytest)
