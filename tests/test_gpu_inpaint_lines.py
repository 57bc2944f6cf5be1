"""biharmonic_fill_device(precond='lines') / Dynspec.inpaint(precond='lines') -- the line-block preconditioner of csrc/inpaint.hpp
and its Python wrappers -- on the GPU against the direct sparse solve of the same system (tests/inpaint_oracle.py).  The checks,
their cases and the bounds are in tests/inpaint_lines_checks.py and tests/inpaint_lines_cases.py, shared with the host-interpreter
run (tests/test_inpaint_lines_emu_cpu.py); every check prints what it measured."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import inpaint_cases as ic  # noqa: E402
import inpaint_lines_cases as lc  # noqa: E402
import inpaint_lines_checks as ck  # noqa: E402


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def C():
    from scintools_amd import clean
    return clean


@pytest.fixture(scope="module")
def D():
    from scintools_amd import dynspec
    return dynspec


@pytest.mark.parametrize("name", lc.NAMES)
def test_against_the_direct_solve(C, name):
    ck.check_case(C, name)


@pytest.mark.parametrize("name", ic.NAMES)
def test_default_route_is_unchanged(C, name):
    ck.check_default_route_unchanged(C, name)


def test_inpaint_after_zap(D, C):
    ck.check_method(D, C)


def test_errors(C, D):
    ck.check_errors(C, D, pytest)
