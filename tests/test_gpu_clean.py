"""Dynspec.zap / refill / correct_dyn / auto_processing and ththmod.svd_model -- the kernels of csrc/clean.hpp and their Python
wrappers -- on the GPU against the unmodified reference's outputs
(tests/golden/clean.npz) and the NumPy / SciPy restatement (tests/clean_oracle.py).  The checks, their shapes and the tolerances
are in tests/clean_checks.py, shared with the host-interpreter run (tests/test_clean_emu_cpu.py); every check prints the K it
measured."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import clean_cases as cc  # noqa: E402
import clean_checks as ck  # noqa: E402


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def D():
    from scintools_amd import dynspec
    return dynspec


@pytest.fixture(scope="module")
def gold(golden):
    return golden("clean.npz")


@pytest.fixture(scope="module")
def zap_inputs():
    return cc.zap_inputs()


@pytest.mark.parametrize("case", list(cc.CASES))
def test_against_reference(D, gold, case):
    ck.check_golden(D, gold, case)


@pytest.mark.parametrize("name", list(cc.zap_inputs()))
def test_zap_shapes(D, zap_inputs, name):
    ck.check_zap(name, zap_inputs[name])


def test_zap_method_in_place(D):
    ck.check_zap_method(D)


@pytest.mark.parametrize("shape", ck.MEDIAN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kernel", ck.MEDIAN_KERNELS, ids=str)
def test_refill_median(D, shape, kernel):
    ck.check_median(D, shape, kernel)


@pytest.mark.parametrize("shape", ck.LINEAR_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-axis{s[2]}")
def test_refill_linear(D, shape):
    ck.check_linear(D, *shape)


def test_refill_masks_methods_and_errors(D):
    ck.check_refill_other(D, pytest)


@pytest.mark.parametrize("shape", ck.SVD_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-n{s[2]}")
def test_correct_dyn_svd(D, shape):
    ck.check_svd(D, *shape)


def test_correct_dyn_svd_zeros_and_nans(D):
    ck.check_svd(D, 33, 70, 2, nans=True)


def test_svd_model_complex(D):
    from scintools_amd import ththmod
    ck.check_svd_model(ththmod)


def test_correct_dyn_errors(D):
    ck.check_svd_errors(D, pytest)


@pytest.mark.parametrize("kw", [dict(), dict(nsmooth=5), dict(frequency=False), dict(time=False), dict(frequency=False, time=False)],
                         ids=str)
def test_correct_dyn_nosvd(D, kw):
    ck.check_nosvd(D, kw)


def test_correct_dyn_lamsteps(D):
    ck.check_lamsteps(D)


def test_auto_processing(D):
    ck.check_auto_processing(D)


def test_deterministic(D):
    ck.check_deterministic(D)
