"""Dynspec.calc_scattered_image on the GPU against the NumPy / SciPy oracle (tests/scatim_oracle.py) and the unmodified reference's
outputs (tests/golden/scatim.npz).  The checks, their shapes and the tolerance are in tests/scatim_checks.py, shared with the
host-interpreter run (tests/test_scatim_emu_cpu.py); every check prints the K it measured."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import scatim_cases as sc  # noqa: E402
import scatim_checks as ck  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def D():
    from scintools_amd import dynspec
    return dynspec


@pytest.fixture(scope="module")
def A(D):
    from scintools_amd import arcfit
    return arcfit


@pytest.fixture(scope="module")
def gold(golden):
    return golden("scatim.npz")


@pytest.mark.parametrize("case", list(sc.CASES))
def test_against_reference(D, gold, case):
    ck.check_golden(D, gold, case)


@pytest.mark.parametrize("shape", ck.KERNEL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_shapes(A, shape):
    ck.check_kernel_shape(A, *shape)


def test_uneven_knots_unaligned_crop(A):
    ck.check_kernel_shape(A, 37, 53, uneven=True, offset=(2, 3, 4))
    ck.check_kernel_shape(A, 5, 6200, uneven=True, offset=(1, 1, 2))


def test_abscissae_on_knots_and_ends(A):
    ck.check_on_knots(A)


def test_neg_inf_db_is_zero(A):
    ck.check_neg_inf(A)


def test_nonfinite_pixel_gives_nan_image(A):
    ck.check_nonfinite(A)


def test_deterministic(D):
    ck.check_deterministic(D)


def test_plot_keywords(D):
    ck.check_plot_keywords(D, pytest)


def test_parked_spectrum_stays_on_device(D):
    ck.check_parked(D)


def test_default_chain_after_fit_arc(D, gold):
    ck.check_chain(D, gold)


def test_short_axes_and_host_errors(D):
    ck.check_small_axes(D, pytest)
