"""GPU checks of the single calls scint_acf and scint_sspec as the B = 1 of the stacked routes: the stack of one bit for bit, the
ABI's workspace size to the byte, and the independent oracles.  The checks, and why these shapes: tests/single_route_checks.py."""
import pytest

import single_route_checks as ck

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sp():
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
