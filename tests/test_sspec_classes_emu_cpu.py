"""calc_sspec's two-trip kernels (csrc/sspec.hip) in all six length classes of both axes, with and without prewhite, interpreted
on the host (tests/emu): 18 instantiations of sspec_cols_kernel, sspec_cols2_kernel and sspec_rows2_kernel against a long-double
evaluation of the secondary spectrum, and the persistent kernels' walk over several tiles / row groups per workgroup against the
default launch, bit for bit.  Cases: tests/sspec_class_cases.py; reference, metric and bound: tests/sspec_class_checks.py.
Runs without a GPU; tests/test_gpu_sspec_classes.py runs the same cases on the device."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)
import sspec_class_cases as cc  # noqa: E402
import sspec_class_checks as ck  # noqa: E402


@pytest.fixture()
def emu(monkeypatch):
    import emulated
    emulated.install(monkeypatch)
    from scintools_amd import dynspec
    return dynspec


def test_every_instantiation_is_reached_twice():
    """The table of the cases module against next_pow2 and sspec_fast_supported's rule: every class of both axes has at least
    two shapes, each run with prewhite off (cols2, rows2) and on (cols, rows2 with the post-darkening)."""
    cols, rows = cc.coverage(cc.GPU_CASES)
    assert cols == cc.COLS_SHAPES and rows == cc.ROWS_SHAPES
    assert set(cols) == set(rows) == set(cc.CLASSES) == set(cc.FACTORS) and min(cols.values()) >= 2 and min(rows.values()) >= 2
    assert all(a * b * c * d == n for n, (a, b, c, d) in cc.FACTORS.items())
    assert [cc.spb(n) for n in cc.CLASSES] == [16, 8, 4, 2, 1, 1] and [cc.block(n) for n in cc.CLASSES] == [256] * 5 + [512]
    ecols, erows = cc.coverage(cc.EMU_CASES)
    assert ecols[2048] == cols[2048] + 1 and erows[4096] == rows[4096] + 1
    # the edges of the rule: one sample less leaves the class, or the path
    for n in cc.CLASSES:
        assert cc.next_pow2(n // 2 + 1) == n == cc.next_pow2(n) and cc.next_pow2(n // 2) == n // 2
    assert not cc.fast_supported(128, 200) and not cc.fast_supported(200, 8193) and not cc.fast_supported(300, 300, halve=False)
    assert sorted({n for _, n, _ in cc.WALK_CASES}) == list(cc.CLASSES) and len(cc.WALK_CASES) == 12
    assert len(cc.AXES_CASES) == 6 and all(s in cc.GPU_CASES for s in cc.AXES_CASES)


def test_tolerance_file_is_the_generators():
    ck.check_tolerance_file()


@pytest.mark.parametrize("prewhite", cc.PREWHITE, ids=["plain", "prewhite"])
@pytest.mark.parametrize("shape", cc.EMU_CASES, ids=cc.case_id)
def test_class_against_long_double(emu, shape, prewhite):
    ck.check_class(shape, prewhite, "emu")


@pytest.mark.parametrize("shape", cc.AXES_CASES, ids=cc.case_id)
def test_calc_sspec_axes(emu, shape):
    ck.check_axes(shape)


@pytest.mark.parametrize("prewhite", cc.PREWHITE, ids=["plain", "prewhite"])
@pytest.mark.parametrize("axis,n,shape", cc.WALK_CASES, ids=[f"{a}-{n}" for a, n, _ in cc.WALK_CASES])
def test_persistent_walk_has_the_bits_of_the_default_launch(emu, monkeypatch, axis, n, shape, prewhite):
    ck.check_walk(monkeypatch, axis, n, shape, prewhite)
