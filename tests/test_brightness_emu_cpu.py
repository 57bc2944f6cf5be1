"""The brightness-distribution model -- scint_fft2_any, scint_bright_* and scintools_amd.scint_sim.Brightness -- interpreted on the
host (tests/emu, its plain mode) through the same C ABI and Python wrappers as on a GPU, against the reference's outputs
(tests/golden/brightness_<case>.npz) and the NumPy restatement (tests/brightness_oracle.py).  The checks are those of the GPU tests
(tests/brightness_checks.py); the 4093 x 16 transform is left to the GPU (the interpreter needs minutes for its 8192-point rows).
Runs without a GPU."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)
import brightness_cases as bc  # noqa: E402
import brightness_checks as ck  # noqa: E402


@pytest.fixture()
def emu(monkeypatch):
    import emulated
    emulated.install(monkeypatch)
    from scintools_amd import scint_sim
    return scint_sim


@pytest.mark.parametrize("shape", ck.FFT_SHAPES[:3], ids=lambda s: f"{s[0]}x{s[1]}")
def test_fft2_any(emu, shape):
    ck.check_fft2_any(emu, shape)


@pytest.mark.parametrize("case", list(bc.CASES))
def test_against_reference(emu, case):
    ck.check_golden(emu, "emu", case)


@pytest.mark.parametrize("case", ["b", "e"])
def test_qhull_against_live_griddata(emu, case):
    ck.check_qhull(emu, "emu", case)


@pytest.mark.parametrize("case", ["a", "d", "e"])
def test_main_diagonal(emu, case):
    ck.check_main(emu, "emu", case)


def test_errors_and_plot_warnings(emu):
    ck.check_errors(emu, pytest)


def test_deterministic(emu):
    ck.check_deterministic(emu, case="a")
