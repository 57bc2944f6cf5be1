"""biharmonic_fill_device(precond='lines') / Dynspec.inpaint(precond='lines') -- the second half of csrc/inpaint.hpp and the Python
wrappers -- interpreted on the host (tests/emu) through the same C ABI as on a GPU, against the direct sparse solve
(tests/inpaint_oracle.py).  The checks are those of the GPU tests (tests/inpaint_lines_checks.py).  Runs without a GPU."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)
import inpaint_lines_cases as lc  # noqa: E402
import inpaint_lines_checks as ck  # noqa: E402


@pytest.fixture()
def C(monkeypatch):
    import emulated
    emulated.install(monkeypatch)
    from scintools_amd import clean
    return clean


@pytest.mark.parametrize("name", lc.NAMES)
def test_against_the_direct_solve(C, name):
    ck.check_case(C, name)


@pytest.mark.parametrize("name", ("a", "d"))
def test_default_route_is_unchanged(C, name):
    ck.check_default_route_unchanged(C, name)


def test_inpaint_after_zap(C):
    from scintools_amd import dynspec
    ck.check_method(dynspec, C)


def test_errors(C):
    from scintools_amd import dynspec
    ck.check_errors(C, dynspec, pytest)
