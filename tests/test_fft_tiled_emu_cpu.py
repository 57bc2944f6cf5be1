"""The tiled column route of run_cols_fft (csrc/fft.hpp) in every length class, interpreted on the host: a build of the kernel
sources with -DSCINT_COLS_CACHE_BYTES=0.0 (tests/emu/build_emu.py, a build directory of its own), in which EVERY strided transform
of 256 .. 16384 points takes the two tiled passes that the product takes only beyond 300 MiB.  Against a long-double DFT
(tests/fft_tiled_checks.py); the cases and what each is there for: tests/fft_tiled_cases.py.  Runs without a GPU."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)
import fft_tiled_cases as tc  # noqa: E402
import fft_tiled_checks as ck  # noqa: E402


@pytest.fixture()
def emu(monkeypatch):
    import emulated
    emulated.install(monkeypatch, defines=tc.EMU_DEFINES)
    from scintools_amd import ththmod
    return ththmod


@pytest.fixture()
def sp(emu):
    from scintools_amd import scintpar
    return scintpar


def test_the_variant_is_a_build_of_its_own(emu):
    from scintools_amd import _lib
    import build_emu
    import emulated
    name = _lib.load()._name
    assert os.path.basename(name) == "libscint_emu_test.so" and os.path.dirname(name) == build_emu.out_dir(tc.EMU_DEFINES)
    assert os.path.dirname(name) != build_emu.out_dir([]) and emulated.load(tc.EMU_DEFINES) is _lib.load()
    # what the variant changes, restated: at threshold 0 every case below is beyond it, at the product's none is
    for rows, cols in tc.EMU_FFT2 + [(tc.next_pow2(2 * r - 1), c) for r, c in tc.EMU_CHIRP]:
        assert tc.tiled(rows, cols, cache_bytes=0.0) and not tc.tiled(rows, cols)
    assert [tc.class_of(n) for n in tc.CLASSES] == [(16, 16), (32, 16), (32, 32), (64, 32), (64, 64), (128, 64), (128, 128)]


def test_reference_split_equals_the_matrix_product():
    ck.check_reference_split()


@pytest.mark.parametrize("shape", tc.EMU_FFT2, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fft2_every_class_one_two_three_tiles(emu, shape):
    ck.check_fft2(shape)


@pytest.mark.parametrize("nf,nt", tc.EMU_CS_PARTIAL)
def test_conjugate_spectrum_last_tile_not_full(emu, nf, nt):
    ck.check_cs_partial_tile(nf, nt)


@pytest.mark.parametrize("nf,nt,npad", tc.EMU_CS_PADDED)
def test_conjugate_spectrum_padded_rows(emu, nf, nt, npad):
    ck.check_cs_padded(emu, nf, nt, npad)


@pytest.mark.parametrize("shape", tc.EMU_CHIRP, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fft2_chirp_on_the_strided_axis(emu, shape):
    ck.check_fft2(shape)


@pytest.mark.parametrize("B,nf,nt", tc.EMU_CS_BATCH)
def test_cs_batch_has_the_bits_of_the_single_call(emu, B, nf, nt):
    ck.check_cs_batch(emu, B, nf, nt)


@pytest.mark.parametrize("B,nf,nt", tc.EMU_ACF_BATCH)
def test_acf_batch_one_launch_has_the_bits_of_the_single_call(sp, B, nf, nt):
    ck.check_acf_batch(sp, B, nf, nt)
