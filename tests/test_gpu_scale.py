"""Dynspec.scale_dyn(scale='velocity' | 'orbit' | 'trapezoid') and calc_sspec(velocity=True | trap=True) on the GPU: the kernels of
csrc/scale.hpp and their Python against scipy / NumPy (tests/scale_oracle.py) and the unmodified reference's outputs
(tests/golden/scale.npz).  The checks, their shapes and the derived tolerance are in tests/scale_checks.py; every check prints the
E it measured.  (`pytest --emu tests/test_gpu_scale.py -m gpu` runs the same file on the host interpreter.)"""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import scale_cases as sc  # noqa: E402
import scale_checks as ck  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold(golden):
    return golden("scale.npz")


@pytest.fixture()
def seeded(monkeypatch, gold):
    ck.seeded(monkeypatch, gold)
    return gold


# ---- the row spline
@pytest.mark.parametrize("shape", ck.ROW_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rows(shape):
    ck.check_rows(*shape, route="blocked" if shape[1] - 2 >= 4 * sc.BLOCK else "lds")


def test_rows_velocity_contrast_50_to_1():
    ck.check_contrast()


def test_rows_through_the_workspace():
    ck.check_workspace_route()


def test_rows_blocked_vs_one_block():
    ck.check_blocked_vs_one_block()


def test_rows_large_arrays_go_through_the_transpose(monkeypatch):
    ck.check_transpose_route(monkeypatch)


def test_rows_other_targets():
    ck.check_nout()


def test_rows_nan_pixel_poisons_its_row_only():
    ck.check_nan()


def test_rows_errors():
    ck.check_errors(pytest)


def test_velocity_resample_device():
    ck.check_velocity_helper()


# ---- the trapezoid
@pytest.mark.parametrize("name", list(sc.TRAPEZOID))
def test_trapezoid(name):
    ck.check_trapezoid(name)


def test_trapezoid_more_than_one_workgroup():
    ck.check_trapezoid_long()


# ---- through Dynspec
def test_scale_dyn_velocity_sets_vdyn(seeded):
    ck.check_velocity_case(seeded, "ecc")


@pytest.mark.parametrize("name", [n for n in sc.VELOCITY if n != "ecc"])
def test_scale_dyn_velocity_cases(seeded, name):
    ck.check_velocity_case(seeded, name)


def test_calc_sspec_velocity(seeded):
    ck.check_velocity_spectra(seeded)


def test_calc_sspec_trap(gold):
    ck.check_trap_spectrum(gold)


def test_orbit_velocity_flag_and_combined_names(seeded):
    ck.check_names(seeded)


def test_parfile(seeded, tmp_path):
    ck.check_parfile(seeded, tmp_path)
