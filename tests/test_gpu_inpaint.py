"""Dynspec.inpaint / clean.biharmonic_fill_device -- the kernels of csrc/inpaint.hpp and their Python wrappers -- on the GPU against
the direct sparse solve of the same system (tests/inpaint_oracle.py).  The checks, their cases and the bounds are in
tests/inpaint_checks.py and tests/inpaint_cases.py, shared with the host-interpreter run (tests/test_inpaint_emu_cpu.py); every
check prints what it measured."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import inpaint_cases as ic  # noqa: E402
import inpaint_checks as ck  # noqa: E402


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def C():
    from scintools_amd import clean
    return clean


@pytest.fixture(scope="module")
def D():
    from scintools_amd import dynspec
    return dynspec


@pytest.mark.parametrize("name", ic.NAMES)
def test_against_the_direct_solve(C, name):
    ck.check_case(C, name)


def test_nothing_masked_is_a_copy(C):
    ck.check_nothing_masked(C)


def test_inpaint_after_zap(D, C):
    ck.check_method(D, C)


def test_errors(C):
    ck.check_errors(C, pytest)
