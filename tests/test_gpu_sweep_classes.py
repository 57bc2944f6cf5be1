"""The theta-theta eigen sweep on an MI355X across every class of the packed Hermitian mat-vec (csrc/eigen_packed.hip,
csrc/packed.hpp, the packed gather of thth.hip): every strip length, full and short row groups, groups of one, two and three
strips, last tiles with 1, 63 and 64 live rows -- float64 and mixed precision, eigenvalue and eigenpair, against LAPACK on the
oracle's matrix; sizes from two to seventeen block rows through the same three slots in one call; a stack of spectra through
eval_sweep_multi.  The matrices are noise-like, so that every tile carries at least 1e-6 of the eigenvalue (the conditions are
checked on the CPU in tests/test_sweep_classes_emu_cpu.py).  Cases: tests/sweep_class_cases.py; checks and bars:
tests/sweep_class_checks.py, shared with the host-interpreter run.

Every test prints what it measured on a SWEEPCLASS line before it asserts: run with -s to collect the figures
(profiles/sweep_classes_gpu.txt holds those of one run)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep_class_cases as sc  # noqa: E402
import sweep_class_checks as ck  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def thth():
    from scintools_amd import ththmod
    from scintools_amd.device import require_gpu
    require_gpu()
    ck.check_defaults(ththmod)
    yield ththmod
    assert ththmod.sweep_precision("f64") == "f64"


@pytest.mark.parametrize("n", sc.SIZES)
def test_float64_eigenvalue(thth, n):
    ck.check_value_f64(thth, "gpu", n)


@pytest.mark.parametrize("n", sc.SIZES)
def test_float64_eigenpair(thth, n):
    ck.check_pair_f64(thth, "gpu", n)


@pytest.mark.parametrize("n", sc.SIZES)
def test_mixed_eigenvalue(thth, n):
    ck.check_value_mixed(thth, "gpu", n)


@pytest.mark.parametrize("n", sc.SIZES)
def test_mixed_all_eigenpair(thth, n):
    ck.check_pair_mixed(thth, "gpu", n)


def test_two_to_seventeen_block_rows_through_three_slots(thth):
    ck.check_mixed_sizes_in_one_call(thth, "gpu", 1087, 2, 17)


def test_stack_of_spectra_in_three_strip_classes(thth):
    ck.check_stack(thth, "gpu")
