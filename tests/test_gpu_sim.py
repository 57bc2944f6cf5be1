"""scintools_amd.scint_sim.Simulation on the GPU against the reference's outputs (tests/golden/sim.npz), the host oracle
(oracle/sim_oracle.py) and itself (shortcut vs full transform, grouping, determinism).  The checks and their tolerances are in
tests/sim_checks.py, shared with the host-interpreter run (tests/test_sim_emu_cpu.py).

Share of spe elements not bit-identical to the reference's (printed by the first test, recorded in DESIGN.md, not asserted)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sim_cases as sc  # noqa: E402
import sim_checks as ck  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    from scintools_amd import scint_sim
    return scint_sim


@pytest.fixture(scope="module")
def gold(golden):
    return golden("sim.npz")


@pytest.mark.parametrize("case", list(sc.CASES))
def test_against_reference(S, gold, case):
    ck.check_golden(S, "gpu", gold, case, pytest)


@pytest.mark.parametrize("case", ["b", "d"])
def test_shortcut_vs_full_transform(S, gold, case):
    ck.check_shortcut(S, gold, case)


def test_frequency_grouping(S):
    ck.check_grouping(S, "gpu")


def test_deterministic(S):
    ck.check_deterministic(S)


def test_against_oracle_512(S):
    ck.check_oracle(S)


def test_drop_in_for_dynspec(S):
    from scintools_amd.dynspec import Dynspec
    sim = S.Simulation(**sc.kwargs("b"))
    d = Dynspec(dyn=sim, verbose=False)
    d.calc_sspec()
    assert np.array_equal(d.dyn, sim.dyn) and d.dyn.shape == (5, 64)
    assert np.array_equal(d.freqs, sim.freqs) and d.name == sim.name and np.all(np.isfinite(d.sspec))


def test_errors(S):
    ck.check_errors(S, pytest)
