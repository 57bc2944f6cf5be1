"""The theta-theta eigen sweep across the packed mat-vec classes -- the checks of tests/test_gpu_sweep_classes.py
(tests/sweep_class_checks.py) on the kernel sources interpreted on the host (tests/emu), for the cases with nb <= 17, and the
one-call check on crops of two to nine block rows -- and the conditions the inputs of both files have to meet, from the oracle
and LAPACK alone.  Runs without a GPU.

The conditions (tests/sweep_class_cases.py builds the inputs): for every size the relative gap (lambda_1 - lambda_2) / lambda_1
is at least 0.01, and zeroing any one stored tile moves lambda_1 by at least 1e-6 of itself to first order -- 1000 times the bar
of the eigenvalue check, so a tile that is dropped, doubled or read from the wrong place fails that check.  The exceptions are
listed in sweep_class_cases.ONE_ROW_TILES (the one-row last block column of the N = 1 (mod 64) sizes); for those sizes zeroing
the live last row and column must move lambda_1 by 1e-6 as well."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)
import sweep_class_cases as sc  # noqa: E402
import sweep_class_checks as ck  # noqa: E402

EMU_NB_MAX = 17
EMU_SIZES = [n for n in sc.SIZES if sc.nb_of(n) <= EMU_NB_MAX]


@pytest.fixture()
def emu(monkeypatch):
    import subprocess
    import emulated
    try:
        emulated.install(monkeypatch)
    except (RuntimeError, OSError, subprocess.CalledProcessError) as exc:    # no usable clang++ on this machine
        pytest.skip(f"host interpreter could not be built: {exc}")
    from scintools_amd import ththmod
    ck.check_defaults(ththmod)
    return ththmod


def test_case_list_covers_what_it_claims():
    """14 nb x 2 sizes + 4 full last tiles; every strip length; full, short and one-row last groups; groups of 1, 2 and 3 strips."""
    assert len(EMU_SIZES) == 11 * 2 + 3 and max(EMU_SIZES) == 1088
    assert {sc.strip_len(nb) for nb in sc.CLASS_NB} == {1, 2, 4, sc.MAX_STRIP}
    last_rows = {sc.group_strips(nb)[-1][1] for nb in sc.CLASS_NB}
    assert {1, 3, 4, 5, 7, 8} <= last_rows
    assert {g[2] for nb in sc.CLASS_NB if nb >= 16 for g in sc.group_strips(nb)} == {1, 2, 3}
    assert {n % sc.TILE for n in sc.SIZES} == {0, 1, 63}


def test_input_conditions_hold_for_every_size():
    worst = dict(gap=np.inf, tile=np.inf, last_row=np.inf, lam_ratio=0.0)
    checked = 0
    for n in sc.SIZES:
        if n in sc.DEGENERATE:
            continue
        r = ck.input_conditions(n)
        print(f"\nSWEEPINPUT N={n} nb={sc.nb_of(n)} gap={r['gap']:.4f} min_tile={r['tile']:.3e} at={r['tile_at']} "
              f"last_row={'-' if r['last_row'] is None else format(r['last_row'], '.3e')} lam_min/lam_max={r['lam_ratio']:.3f}")
        assert r["gap"] >= ck.GAP, n
        assert r["tile"] >= ck.TILE_SENSITIVITY, (n, r["tile_at"])
        assert (r["last_row"] is not None) == (n in sc.ONE_ROW_TILES)
        if r["last_row"] is not None:
            assert r["last_row"] >= ck.TILE_SENSITIVITY, n
            worst["last_row"] = min(worst["last_row"], r["last_row"])
        worst["gap"], worst["tile"] = min(worst["gap"], r["gap"]), min(worst["tile"], r["tile"])
        worst["lam_ratio"] = min(worst["lam_ratio"], r["lam_ratio"])
        checked += 1
    print(f"\nSWEEPINPUT worst of {checked} sizes: gap={worst['gap']:.4f} min_tile={worst['tile']:.3e} "
          f"last_row={worst['last_row']:.3e} lam_min/lam_max={worst['lam_ratio']:.3f}")
    assert checked == len(sc.SIZES) - len(sc.DEGENERATE) == 31


@pytest.mark.parametrize("n", EMU_SIZES)
def test_float64_eigenvalue(emu, n):
    ck.check_value_f64(emu, "emu", n)


@pytest.mark.parametrize("n", EMU_SIZES)
def test_float64_eigenpair(emu, n):
    ck.check_pair_f64(emu, "emu", n)


@pytest.mark.parametrize("n", EMU_SIZES)
def test_mixed_eigenvalue(emu, n):
    ck.check_value_mixed(emu, "emu", n)


@pytest.mark.parametrize("n", EMU_SIZES)
def test_mixed_all_eigenpair(emu, n):
    ck.check_pair_mixed(emu, "emu", n)


def test_two_to_nine_block_rows_through_three_slots(emu):
    ck.check_mixed_sizes_in_one_call(emu, "emu", 575, 2, 9)
