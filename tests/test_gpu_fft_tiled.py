"""The tiled column route of run_cols_fft (csrc/fft.hpp) on the GPU, in the product build at its real threshold: the smallest
power-of-two arrays that take the route in each of its seven length classes (tests/fft_tiled_cases.py) -- 2^25 complex points,
512 MiB, per case: test sizes, not workload sizes.  Every case asserts, from run_cols_fft's own formula, that it IS beyond the
threshold (and that half of it is not): a later change of the constant makes this module say so.

Reference: np.fft in float64 for the whole array, |got - ref| <= 1e-12 max|ref| (the project's FFT tolerance), and in addition eight
output columns -- 0, 15, 16, ncols-17, ncols-16, ncols-1 (both ends of the first and the last tile) and two seeded ones -- against
the long-double column DFT (tests/fft_tiled_checks.py) of the float64 row transform, to the same tolerance.  The reference alone
(np.fft against the long-double columns) is printed too and must stay a factor 10 inside the bound for the bound to mean the device.

Real input (the half-width route: Ch = nt / 2 + 1 columns, a last tile with ONE live column, the half sink): the non-redundant
half against np.fft.rfft2 under the project's shift, the other half against the device's own first half by conjugate symmetry.
Classes 256 .. 2048 cannot reach a partly filled tile from a public entry point on the GPU -- beyond 300 MiB their rows would
be longer than the 131072 points the row transform takes; tests/test_fft_tiled_emu_cpu.py covers them at threshold 0.

Observed on an MI355X (|.| / max|ref|; every case prints its own), 1.3 - 1.9 s per case:
                            device - np.fft   device - long double   np.fft - long double (the reference alone)
    scint_fft2, 7 classes   9.0e-16 .. 1.1e-15   4.7e-16 .. 6.8e-16   1.3e-16 .. 3.4e-16
    real (16384, 4096)      9.6e-20              1.0e-16              1.0e-16      mirrored half: 0 (the sink's conj is exact)
    real (4096, 16384)      8.2e-20              3.7e-17              3.7e-17      mirrored half: 0
The reference alone stays 3.5 orders inside the bound.  The real cases' peak is the sum of 2^26 samples of unit mean, 5e4 times a
typical value: against typical values their errors are ~5e-15, and a misplaced or dropped element is ~2e-5 of the peak.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fft_tiled_cases as tc  # noqa: E402
import fft_tiled_checks as ck  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def thth():
    from scintools_amd import ththmod
    from scintools_amd.device import require_gpu
    require_gpu()
    return ththmod


@pytest.fixture()
def device_memory():
    """Cases run one at a time on a device that holds nothing of the one before; yields a function that returns the case's peak:
    the bytes allocated above what other modules of the run still hold when the case starts."""
    import torch
    from scintools_amd import device

    def free():
        device.workspace.release()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    free()
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()
    yield lambda: torch.cuda.max_memory_allocated() - held
    free()


def eight_columns(ncols, seed):
    rng = np.random.default_rng(seed)
    return np.array([0, 15, 16, ncols - 17, ncols - 16, ncols - 1] + list(rng.integers(17, ncols - 17, 2)))


def reference(rowft, cols):
    """(np.fft along the strided axis of the float64 row transform, the long-double DFT of its columns `cols`)."""
    ld = ck.dft_ld(rowft[:, cols], 0)
    return np.fft.fft(rowft, axis=0), ld


def compare(what, got_half, ref, ld, cols):
    """got_half / ref: the arrays in natural order; ld: long-double columns `cols` of ref.  Prints, then asserts."""
    peak = float(np.abs(ref).max())
    err_full = float(np.abs(got_half - ref).max()) / peak
    err_cols = float(np.abs(got_half[:, cols].astype(ck.CLD) - ld).max()) / peak
    ref_cols = float(np.abs(ref[:, cols].astype(ck.CLD) - ld).max()) / peak
    print(f"{what}: device - np.fft {err_full:.3e}, device - long double (8 columns) {err_cols:.3e}, "
          f"np.fft - long double (8 columns) {ref_cols:.3e}" + ("  [REFERENCE WITHIN 10x OF THE BOUND]" if ref_cols > ck.TOL / 10 else ""))
    assert err_full <= ck.TOL, (what, err_full)
    assert err_cols <= ck.TOL, (what, err_cols)


@pytest.mark.parametrize("shape", tc.GPU_FFT2, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fft2_every_class_beyond_the_threshold(thth, device_memory, shape):
    from scintools_amd import _lib
    rows, cols = shape
    assert tc.tiled(rows, cols) and not tc.tiled(rows, cols // 2), "not the smallest power-of-two array on the tiled route"
    need = ctypes.c_size_t()
    _lib.check(_lib.load().scint_fft2_workspace_bytes(rows, cols, ctypes.byref(need)))
    assert need.value <= 2 * 16 * rows * cols + 4096          # the row result and one column working array
    x = tc.complex_input(shape)
    got = ck.fft2_device(x)
    assert device_memory() <= 4 * 16 * rows * cols + 4096     # input, output and the workspace: 2 GiB
    cs = eight_columns(cols, rows)
    ref, ld = reference(np.fft.fft(x, axis=1), cs)
    del x
    compare(f"scint_fft2 {shape} class {tc.class_of(rows)}", got, ref, ld, cs)


@pytest.mark.parametrize("nf,nt", tc.GPU_CS)
def test_conjugate_spectrum_real_input_last_tile_not_full(thth, device_memory, nf, nt):
    Ch = nt // 2 + 1
    assert tc.tiled(nf, Ch) and Ch % 16 == 1
    dyn = tc.real_input(nf, nt)
    G = thth.conjugate_spectrum(dyn, 0).cpu().numpy()
    assert G.shape == (nf, nt)
    assert device_memory() <= 7 * 8 * nf * nt + (1 << 20)     # input 8, output 16, workspace 32 bytes per point: 3.5 GiB
    # the non-redundant half in natural order: X[r, c] = CS[(r + R/2) % R, (c + C/2) % C], c = 0 .. C/2
    half = np.roll(np.concatenate([G[:, nt // 2:], G[:, :1]], axis=1), nf // 2, axis=0)
    cs = eight_columns(Ch, nf)
    ref, ld = reference(np.fft.rfft(dyn, axis=1), cs)
    del dyn
    compare(f"conjugate spectrum ({nf}, {nt}) class {tc.class_of(nf)} Ch = {Ch}", half, ref, ld, cs)
    # the other half: CS[i, j] = conj(CS[(R - i) % R, C - j]) for j = 1 .. C/2 - 1, against the device's own first half
    mirror = np.conj(G[(nf - np.arange(nf)) % nf][:, nt - 1:nt // 2:-1])
    err = float(np.abs(G[:, 1:nt // 2] - mirror).max()) / float(np.abs(ref).max())
    print(f"conjugate spectrum ({nf}, {nt}): mirrored half against the conjugate of the first {err:.3e}")
    assert err <= ck.TOL
