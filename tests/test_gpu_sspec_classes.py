"""calc_sspec's two-trip kernels (csrc/sspec.hip) on the GPU in all six length classes of both axes, with and without prewhite:
the 18 instantiations of sspec_cols_kernel, sspec_cols2_kernel and sspec_rows2_kernel, each at two shapes or more, against a
long-double evaluation of the secondary spectrum; and the persistent kernels' walk over several tiles / row groups per workgroup
(SCINT_SSPEC_MAXGRID = 1, 3, 8, 13) against the default launch, bit for bit.  Cases: tests/sspec_class_cases.py; reference, metric
(amplitude before post-darkening, of the largest amplitude) and bound (8 x the float64 oracle's own error per group, at least
64 eps = 1.42e-14; tests/golden/sspec_class_tolerances.json): tests/sspec_class_checks.py.  The same cases run on the host
interpreter in tests/test_sspec_classes_emu_cpu.py.

Observed on an MI355X, amplitude error of the largest amplitude, the worse of the class's two shapes (every case prints its
own SSPECCLASS line), device / float64 oracle alone; the bound is 1.42e-14 (64 eps)
in every group but cols-4096 without prewhite, 1.46e-14 (8 x the oracle's 1.83e-15):

    class    columns, plain      columns, prewhite   rows, plain         rows, prewhite
    256      1.34e-15 / 8.6e-16  1.76e-15 / 1.4e-15  1.75e-15 / 9.5e-16  1.55e-15 / 1.0e-15
    512      1.97e-15 / 1.2e-15  1.75e-15 / 1.2e-15  2.03e-15 / 1.2e-15  1.66e-15 / 1.1e-15
    1024     1.75e-15 / 1.3e-15  1.82e-15 / 1.2e-15  2.31e-15 / 1.3e-15  1.98e-15 / 1.3e-15
    2048     4.75e-15 / 1.1e-15  1.70e-15 / 1.2e-15  2.31e-15 / 1.5e-15  1.96e-15 / 1.2e-15
    4096     2.67e-15 / 1.8e-15  2.11e-15 / 1.3e-15  3.38e-15 / 1.5e-15  2.06e-15 / 1.2e-15
    8192     4.26e-15 / 1.7e-15  1.73e-15 / 1.4e-15  1.80e-15 / 1.6e-15  2.06e-15 / 1.6e-15
    mixed 600 x 1030 (1024 x 2048): plain 1.57e-15 / 1.2e-15, prewhite 1.89e-15 / 1.1e-15

The largest, 4.75e-15 at 1025 x 200 (sspec_cols2_kernel<16,16,8,1>), is a third of the bound and 5 times the oracle's; a misplaced
or dropped element is at least 1e-3.  In linear power of the peak the same runs give 1.4e-15 .. 3.5e-15 without prewhite and
5.5e-15 .. 6.9e-14 with it (the oracle alone: up to 7.7e-14): the post-darkening's amplification, which is why the bound is not
set there.  All 96 capped launches of the walk (12 shapes, prewhite off and on, four caps) had the
bits of the default launch.

Wall time per class case 0.2 .. 3.7 s, nearly all of it the long-double reference and the 10^x of the comparison (the device call
is milliseconds); the slowest are the 8192-class shapes and 600 x 1030 at 3.3 .. 3.7 s (4097 x 200 prewhite: 3.68 s).  A walk
case (five calls) takes under 0.1 s.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sspec_class_cases as cc  # noqa: E402
import sspec_class_checks as ck  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from scintools_amd import dynspec
    from scintools_amd.device import require_gpu
    require_gpu()
    return dynspec


def test_every_instantiation_is_reached_twice():
    cols, rows = cc.coverage(cc.GPU_CASES)
    assert cols == cc.COLS_SHAPES and rows == cc.ROWS_SHAPES
    assert set(cols) == set(rows) == set(cc.CLASSES) and min(cols.values()) >= 2 and min(rows.values()) >= 2
    ck.check_tolerance_file()


@pytest.mark.parametrize("prewhite", cc.PREWHITE, ids=["plain", "prewhite"])
@pytest.mark.parametrize("shape", cc.GPU_CASES, ids=cc.case_id)
def test_class_against_long_double(gpu, shape, prewhite):
    ck.check_class(shape, prewhite, "gpu")


@pytest.mark.parametrize("shape", cc.AXES_CASES, ids=cc.case_id)
def test_calc_sspec_axes(gpu, shape):
    ck.check_axes(shape)


@pytest.mark.parametrize("prewhite", cc.PREWHITE, ids=["plain", "prewhite"])
@pytest.mark.parametrize("axis,n,shape", cc.WALK_CASES, ids=[f"{a}-{n}" for a, n, _ in cc.WALK_CASES])
def test_persistent_walk_has_the_bits_of_the_default_launch(gpu, monkeypatch, axis, n, shape, prewhite):
    ck.check_walk(monkeypatch, axis, n, shape, prewhite)
