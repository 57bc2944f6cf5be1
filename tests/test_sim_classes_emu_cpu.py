"""The screen simulator in every row and column transform class, interpreted on the host (tests/emu) through the same C ABI and Python
wrapper as on a GPU, against the host oracle (oracle/sim_oracle.py).  Cases and what each is there for: tests/sim_class_cases.py;
checks and tolerances (those of tests/sim_checks.py): tests/sim_class_checks.py, shared with tests/test_gpu_sim_classes.py.

Two builds: the default one (ten row classes, eight column plans, ten pulse lengths, the slot reduction's order) and the
-DSCINT_COLS_CACHE_BYTES=0.0 variant of tests/fft_tiled_cases.py, in which every transform along x of 256 .. 16384 points takes the
two tiled passes: the simulator's loaders and storers behind the tile functors in all seven tiled classes, g's transform with one
tile of 3 live columns.  On a GPU the product reaches the tiled passes beyond 300 MiB only: class (16, 16) at a test size
(tests/test_gpu_sim_classes.py, 2560 frequencies of 256 x 32), the other six and the tiled g transform only with workspaces above
10 GB and a host oracle of about half a minute -- no test sizes; they run here.  Runs without a GPU."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)
import fft_tiled_cases as tc  # noqa: E402
import sim_class_cases as cc  # noqa: E402
import sim_class_checks as ck  # noqa: E402


@pytest.fixture()
def emu(monkeypatch):
    import emulated
    emulated.install(monkeypatch)
    from scintools_amd import scint_sim
    return scint_sim


@pytest.fixture()
def emu_tiled(monkeypatch):
    import emulated
    emulated.install(monkeypatch, defines=tc.EMU_DEFINES)
    from scintools_amd import scint_sim
    return scint_sim


def test_the_tables_hold_every_class():
    assert sorted(c["shape"][1] for c in cc.ROW_CASES[:10]) == [1 << l for l in range(4, 14)]
    assert all(c["shape"][0] == 16 and c["shape"][2] == 3 for c in cc.ROW_CASES[:10])
    assert [c["stages"] for c in cc.ROW_CASES[:10]] == [cc.ROW_STAGES[l] for l in range(4, 14)]
    assert [c["shape"][0] for c in cc.COL_CASES] == [1 << l for l in range(10, 18)]
    assert sorted({c["plan"][-1] for c in cc.COL_CASES}) == [4, 8, 16, 32] and {len(c["plan"]) for c in cc.COL_CASES} == {3, 4}
    assert [2 * nf for nf in cc.PULSE_NF] == [1 << l for l in range(4, 14)]
    # the widths of SimFilterReduce's tree: inside one wavefront, exactly one, and 2, 4, 8 wavefronts per slot
    assert [c["tr"] for c in cc.ROW_CASES[:10]] == [1, 2, 4, 8, 16, 32, 64, 128, 256, 512]
    assert [cc.row_class(c["shape"][1], 48)["waves_per_slot"] for c in cc.ROW_CASES[7:10]] == [2, 4, 8]


@pytest.mark.parametrize("case", cc.ROW_CASES, ids=lambda c: cc.ident(c["shape"]))
def test_row_class_both_routes(emu, case):
    ck.check_row_class(emu, "emu", case)


@pytest.mark.parametrize("shape", cc.REDUCE_CASES, ids=cc.ident)
def test_slot_reduction_order(emu, shape):
    ck.check_reduce_order(emu, "emu", shape)


@pytest.mark.parametrize("case", cc.COL_CASES, ids=lambda c: cc.ident(c["shape"]))
def test_column_plan_both_routes(emu, case):
    ck.check_col_plan(emu, "emu", case)


@pytest.mark.parametrize("nf", cc.PULSE_NF)
def test_pulse_length(emu, nf):
    ck.check_pulse(emu, "emu", nf)


def test_the_tiled_variant_is_a_build_of_its_own(emu_tiled):
    from scintools_amd import _lib
    import build_emu
    name = _lib.load()._name
    assert os.path.basename(name) == "libscint_emu_test.so" and os.path.dirname(name) == build_emu.out_dir(tc.EMU_DEFINES)
    assert os.path.dirname(name) != build_emu.out_dir([])


@pytest.mark.parametrize("nx", tc.CLASSES)
def test_tiled_class_both_routes(emu_tiled, nx):
    ck.check_tiled_emu(emu_tiled, "emu_tiled", nx)
