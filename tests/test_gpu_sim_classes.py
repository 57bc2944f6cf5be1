"""scintools_amd.scint_sim.Simulation on the GPU, product build, in every row and column transform class of the two FFT kernels it is
built from, against the host oracle (oracle/sim_oracle.py).  Cases and what each is there for: tests/sim_class_cases.py; checks and
tolerances (those of tests/sim_checks.py, unchanged): tests/sim_class_checks.py, shared with the host-interpreter run
(tests/test_sim_classes_emu_cpu.py).  Every case asserts its class from the restated launcher or planner, and its route from
scint_sim_last_route.

The tiled column passes run here in class (16, 16) with batches = 2560 in one launch (test_tiled_group_of_2560_frequencies).  The
other six tiled classes and the tiled transform of g cannot be reached at a test size: nx >= 512 beyond 300 MiB needs more than 4096
frequencies in a group at ny = 16 (the group limit) or a wider screen, a workspace above 10 GB and a host oracle of about half a
minute; tests/test_sim_classes_emu_cpu.py runs them at threshold 0 on the interpreter.

Observed on an MI355X (every case prints its own figures; 32 tests in 5.9 s):
                                              observed                    bound
    xyp  rms(diff), 40 runs                   0.9 .. 3.7 % of the bound   8 eps log2(nx ny) rms(xyp)
    xyp  max|diff|                            <= 0.44 % of the bound      sqrt(nx ny) times that
    spe  worst element, both routes           <= 0.8 % of the bound       2^-22 |ref| + 1e-12 max|ref|
    xyi  max|diff| / max                      2.0e-15 .. 2.9e-14          1e-12
    pulsewin, 2 nf = 16 .. 8192               1.5e-16 .. 1.0e-15          2e-12
    spe elements not bit-identical to the oracle's: 0 in all ten row classes, 32 x 256 x 5, the column plans of 2^10 .. 2^14 and
    2^17 and the ten pulse shapes; 1 of 98304 at 2^15 (1.0e-5), 1 of 196608 at 2^16 (5.1e-6), 1 of 655360 (1.5e-6) in the
    2560-frequency case -- the same element on both routes and in both groupings.  Column route against full route, and one tiled
    group against the default six groups on the radix passes: 0 elements differ in every case.
    The screens: rms(xyp) 6.3 .. 33 rad, unscattered share at most 2.3e-3 (conditions: >= pi, <= 0.05).
    Wall time per test, the host oracle included: at most 0.9 s (the 2560-frequency case; 0.7 s at 2^17 x 16, under 0.35 s the
    others).  A constructor call (host draw, upload, kernels, download) takes 0.4 .. 75 ms after the process's first (192 ms): 2.9 ms
    for the one tiled group of 2560 frequencies, 2.3 ms for its six default groups; pulsewin 0.1 .. 0.4 ms."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim_class_cases as cc  # noqa: E402
import sim_class_checks as ck  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    from scintools_amd import scint_sim
    from scintools_amd.device import require_gpu
    require_gpu()
    return scint_sim


@pytest.mark.parametrize("case", cc.ROW_CASES, ids=lambda c: cc.ident(c["shape"]))
def test_row_class_both_routes(S, case):
    ck.check_row_class(S, "gpu", case)


@pytest.mark.parametrize("shape", cc.REDUCE_CASES, ids=cc.ident)
def test_slot_reduction_order(S, shape):
    ck.check_reduce_order(S, "gpu", shape)


@pytest.mark.parametrize("case", cc.COL_CASES, ids=lambda c: cc.ident(c["shape"]))
def test_column_plan_both_routes(S, case):
    ck.check_col_plan(S, "gpu", case)


@pytest.mark.parametrize("nf", cc.PULSE_NF)
def test_pulse_length(S, nf):
    ck.check_pulse(S, "gpu", nf)


def test_tiled_group_of_2560_frequencies(S):
    from scintools_amd import device
    try:
        ck.check_tiled_gpu(S, "gpu")
    finally:
        device.workspace.release()          # 0.67 GB: not kept for the modules that run after this one
