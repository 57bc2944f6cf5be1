"""Shapes that send a strided-axis transform through the TILED column route of run_cols_fft (csrc/fft.hpp: the four-step
algorithm on 16-column tiles, two trips through memory) instead of the in-place radix passes; the checks are
tests/fft_tiled_checks.py.

The route is chosen by bytes: len * ncols * batches * 16 B > SCINT_COLS_CACHE_BYTES (300 MiB in the product) and
256 <= len <= 16384.  It has seven length classes (l = log2 len, l2 = l / 2, l1 = l - l2; pass A runs L1-point, pass B L2-point
transforms through launch_fft_rows<4, 7>):

    len        256    512    1024   2048   4096   8192    16384
    (L1, L2)   16,16  32,16  32,32  64,32  64,64  128,64  128,128

Two builds run them:
  * the host-interpreted one with -DSCINT_COLS_CACHE_BYTES=0.0 (tests/test_fft_tiled_emu_cpu.py): EVERY strided transform of
    256..16384 points is tiled, so small shapes reach every class, every source and sink and the partly filled last tile;
  * the product at its real threshold (tests/test_gpu_fft_tiled.py): the smallest power-of-two arrays beyond 300 MiB.

Every case below says which class and which edge it is there for."""
import numpy as np

CLASSES = (256, 512, 1024, 2048, 4096, 8192, 16384)
CACHE_BYTES = 300.0 * 1048576.0         # SCINT_COLS_CACHE_BYTES of the product build (csrc/fft.hpp)
EMU_DEFINES = ["-DSCINT_COLS_CACHE_BYTES=0.0"]


def class_of(length):
    """(L1, L2) of the tiled route for a strided length."""
    l = int(length).bit_length() - 1
    assert 1 << l == length and 256 <= length <= 16384, length
    return 1 << (l - l // 2), 1 << (l // 2)


def tiled(length, ncols, batches=1, cache_bytes=CACHE_BYTES):
    """run_cols_fft's own route test (fft.hpp), restated: True where the tiled passes run."""
    return float(length) * float(ncols) * float(batches) * 16.0 > cache_bytes and 256 <= length <= 16384


def next_pow2(n):
    return 1 << (int(n) - 1).bit_length()


# ---- the interpreted build (threshold 0) ------------------------------------------------------------------------------------------
# scint_fft2 [rows, cols], complex: every class x one, two and three tiles.  cols = 16 and 32 are power-of-two rows (the plain first
# loader ColSourcePlain); cols = 48 takes the chirp-z ROW path (the first loader is ColSource with the row post-factor) and gives
# ntiles = 3, no power of two, to tile_slot's divide.
EMU_FFT2 = [(rows, cols) for rows in CLASSES for cols in (16, 32, 48)]

# conjugate spectrum of a REAL [nf, nt] chunk, npad = 0: the half-width route with Ch = nt / 2 + 1 = 9, 17, 33 columns in rows of
# ChL = 16, 24, 40 -- the last tile holds 9, 1 and 1 live columns (the s.ok guard of all four tile functors) -- and the half sink
# that emits every value with its conjugate partner, shifted.  Every class: 256 is reachable here, not on a GPU.
EMU_CS_PARTIAL = [(nf, nt) for nf in CLASSES for nt in (16, 32, 64)]

# conjugate spectrum with mean padding, (nf, nt, npad): nvalid = nf < R = (npad + 1) nf rows exist, the rest is `fill0` (the padded
# rows' transform: C * mean at column 0, zero elsewhere) from the tiled first loader.  R = 512 (32,16), 1024 (32,32) and 8192 (128,64).
EMU_CS_PADDED = [(256, 16, 1), (256, 8, 3), (2048, 8, 3)]

# scint_fft2 with a strided length that is no power of two: both Bluestein passes of length mR = 1024 and 8192 are tiled -- the
# chirp first loader, the `to_b` store into the second working array, the `mulconj_b` source and the post-factor sink.  17 columns:
# a second tile with one live column.
EMU_CHIRP = [(300, 17), (3000, 17)]

# stacks, (B, nf, nt): R = 512 (l1 != l2: a wrong shift in `q >> lbits` cannot cancel), Ch = 17.
#   scint_cs_batch      queues its problems one after the other (batch 0 of one-problem passes): each against scint_cs alone
#   scint_acf_batch     R = 2 nf = 512, Ch = nt + 1 = 17: ONE tiled launch for all B problems -- the batch bits of the slot decode,
#                       StackFirst and StackSink -- for both of its transforms; each problem against scint_acf alone
EMU_CS_BATCH = [(1, 512, 32), (3, 512, 32)]
EMU_ACF_BATCH = [(1, 256, 16), (3, 256, 16)]

# ---- the product build on a GPU ---------------------------------------------------------------------------------------------------
# scint_fft2, complex: the smallest power-of-two arrays beyond the threshold in each class, 2^25 points (512 MiB) each.  The first
# four also run the decimated row transform (rows_fft_src, n > 8192) at n1 = 32, 16, 8 and 4.
GPU_FFT2 = [(256, 131072), (512, 65536), (1024, 32768), (2048, 16384), (4096, 8192), (8192, 4096), (16384, 2048)]

# conjugate spectrum of a real [nf, nt] chunk, npad = 0: Ch = 2049 (in-LDS pair rows) and 8193 (PairSplitSource) columns, so the
# last of 129 / 513 tiles holds ONE live column; classes 16384 and 4096.
GPU_CS = [(16384, 4096), (4096, 16384)]


def complex_input(shape):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def real_input(nf, nt, seed=0):
    """A positive flux: unit mean, 30 % scatter (float64 drawn once, no complex intermediate)."""
    rng = np.random.default_rng(nf * 31 + nt + seed)
    x = rng.random((nf, nt))
    x *= 0.6
    x += 0.7
    return x
