"""Dynspec.inpaint / clean.biharmonic_fill_device -- the kernels of csrc/inpaint.hpp and their Python wrappers -- interpreted on the
host (tests/emu) through the same C ABI as on a GPU, against the direct sparse solve (tests/inpaint_oracle.py).  The checks are
those of the GPU tests (tests/inpaint_checks.py); cases (a) and (c).  Runs without a GPU."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)
import inpaint_checks as ck  # noqa: E402


@pytest.fixture()
def C(monkeypatch):
    import emulated
    emulated.install(monkeypatch)
    from scintools_amd import clean
    return clean


@pytest.mark.parametrize("name", ("a", "c"))
def test_against_the_direct_solve(C, name):
    ck.check_case(C, name)


def test_inpaint_after_zap(C):
    from scintools_amd import dynspec
    ck.check_method(dynspec, C)
