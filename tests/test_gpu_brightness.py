"""scintools_amd.scint_sim.Brightness and the any-length transform scint_fft2_any on the GPU, against the unmodified reference's
outputs (tests/golden/brightness_<case>.npz) and the NumPy restatement (tests/brightness_oracle.py).  The checks and their tolerances
are in tests/brightness_checks.py, shared with the host-interpreter run (tests/test_brightness_emu_cpu.py)."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import brightness_cases as bc  # noqa: E402
import brightness_checks as ck  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    from scintools_amd import scint_sim
    return scint_sim


@pytest.mark.parametrize("shape", ck.FFT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fft2_any(S, shape):
    ck.check_fft2_any(S, shape)


@pytest.mark.parametrize("case", list(bc.CASES))
def test_against_reference(S, case):
    ck.check_golden(S, "gpu", case)


@pytest.mark.parametrize("case", list(bc.CASES))
def test_qhull_against_live_griddata(S, case):
    ck.check_qhull(S, "gpu", case)


@pytest.mark.parametrize("case", list(bc.CASES))
def test_main_diagonal(S, case):
    ck.check_main(S, "gpu", case)


def test_errors_and_plot_warnings(S):
    ck.check_errors(S, pytest)


def test_deterministic(S):
    ck.check_deterministic(S)


def test_tutorial_lines(S):
    """The tutorial's call at a reduced size: runs, with the reference's attribute names and shapes."""
    b = S.Brightness(ar=2, psi=30, thetagx=0.5, thetarx=0.5, nx=8, nt=20, dt=0.25, nf=5, df=0.0625)
    assert b.SS.shape == b.LSS.shape == b.acf.shape == b.jacobian.shape == b.thetax.shape == (160, 160)
    assert b.B.shape == b.acf_efield.shape == b.X.shape == (160, 160) and b.acf.max() == 1.0
