"""The single calls scint_acf and scint_sspec as the B = 1 of the stacked routes, interpreted on the host (tests/emu) through the same
C ABI and Python wrappers as on a GPU.  The checks are those of the GPU tests (tests/single_route_checks.py).  Runs without a GPU."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)
import single_route_checks as ck  # noqa: E402


@pytest.fixture()
def sp(monkeypatch):
    import emulated
    emulated.install(monkeypatch)
    from scintools_amd import scintpar
    return scintpar


@pytest.mark.parametrize("nf,nt", ck.SSPEC_SHAPES)
def test_sspec_of_a_stack_of_one_is_the_single_call(sp, nf, nt):
    ck.check_sspec_stack_of_one(sp, nf, nt)


@pytest.mark.parametrize("nf,nt", ck.SSPEC_SHAPES)
def test_sspec_workspace_size_is_exact(sp, nf, nt):
    ck.check_sspec_workspace(sp, nf, nt)


@pytest.mark.parametrize("nf,nt", ck.SSPEC_SHAPES)
def test_sspec_against_oracle(sp, nf, nt):
    ck.check_sspec_oracle(sp, nf, nt)


@pytest.mark.parametrize("nf,nt", ck.ACF_SHAPES)
def test_acf_of_a_stack_of_one_is_the_single_call(sp, nf, nt):
    ck.check_acf_stack_of_one(sp, nf, nt)


@pytest.mark.parametrize("nf,nt", ck.ACF_SHAPES)
def test_acf_workspace_size_is_exact(sp, nf, nt):
    ck.check_acf_workspace(sp, nf, nt)


@pytest.mark.parametrize("nf,nt", ck.ACF_SHAPES)
def test_acf_against_oracle(sp, nf, nt):
    ck.check_acf_oracle(sp, nf, nt)
