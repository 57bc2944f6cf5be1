"""Shapes that send calc_sspec through every instantiation of the two-trip kernels of csrc/sspec.hip; the checks are
tests/sspec_class_checks.py, the bounds tests/golden/sspec_class_tolerances.json (make_sspec_class_tolerances.py).

The path (`halve`, next_pow2 of both axes in 256 .. 8192: sspec_fast_supported) has three kernels templated on the transform
length, six classes each (SCINT_SSPEC_DISPATCH).  The class of an axis of length L is next_pow2(L) -- of nf and nt themselves,
also under `prewhite`, which transforms nf - 1 by nt - 1 samples:

    class   factorisation   threads   sequences per workgroup (SPB)
    256     <16,16,1,1>     256       16
    512     <16,16,2,1>     256       8
    1024    <16,16,4,1>     256       4
    2048    <16,16,8,1>     256       2
    4096    <16,16,16,1>    256       1
    8192    <16,16,16,2>    512       1      (the only fourth radix)

    sspec_cols2_kernel   class of nf, prewhite off (persistent: a workgroup walks over tiles of SPB column pairs)
    sspec_cols_kernel    class of nf, prewhite on  (one-shot, with sspec_prep_means_kernel)
    sspec_rows2_kernel   class of nt, both         (persistent: groups of SPB rows; the post-darkening under prewhite only)

What the suite reached before this module.  On a GPU: 4096 x 4096 (test_gpu_fullsize.py: class 4096 on both axes; 2048 tiles and
4096 rows on 512 workgroups, so 4 and 8 iterations each) and 300 x 260 (test_gpu_edges.py: 512 on both; its 17 column tiles run
on 16 workgroups -- the grid is rounded down to whole rounds of eight -- so ONE workgroup takes a second tile, and its 64 row groups
run on 64).  tests/golden/sim_sspec.npz is 96 x 128, class 128 on both axes: the generic FFT path, no class of this one.  So on
the device the prefetch into the next iteration had run in classes 4096 and, for a single workgroup, 512.  On the host
interpreter: 256, 512 and 1024 (test_emu_cpu.py).  Classes 1024 and 2048 ran in no GPU test, 256 and 8192 in no test at all.

Every case below runs with prewhite off and on, in both test files (the last one on the interpreter only)."""
import numpy as np

CLASSES = (256, 512, 1024, 2048, 4096, 8192)
FACTORS = {256: (16, 16, 1, 1), 512: (16, 16, 2, 1), 1024: (16, 16, 4, 1), 2048: (16, 16, 8, 1), 4096: (16, 16, 16, 1),
           8192: (16, 16, 16, 2)}
CUS = 256                   # kSspecCUs of sspec.hip
CAPS = (1, 3, 8, 13)        # SCINT_SSPEC_MAXGRID: 3 runs without the XCD remap, 8 with it, 13 rounds down to 8


def next_pow2(n):
    return 1 << (int(n) - 1).bit_length()


def fast_supported(nf, nt, halve=True):
    """sspec_fast_supported of sspec.hip, restated."""
    if not halve or nf < 3 or nt < 3:
        return False
    return 256 <= next_pow2(nf) <= 8192 and 256 <= next_pow2(nt) <= 8192


def ceil_div(a, b):
    return -(-a // b)


def block(n):
    """Threads of a workgroup of class n (ColsBlock; launch_rows2 has the same rule)."""
    return max(n // 16, 256)


def spb(n):
    return block(n) // (n // 16)


# ---- the cases --------------------------------------------------------------------------------------------------------------------
# Per class n of an axis, the other axis in class 256:
#   n/2 + 1   the lower edge of the class; an even other axis (16-byte input loads, whole column pairs).  Under prewhite exactly
#             n/2 samples go into class n.
#   n         the axis fills its half (the kernels' `full` branch; n - 1 samples under prewhite); an odd other axis of 131
#             (8-byte input loads, a last column pair with one column, 66 pairs: an odd number of tiles in no class).
COL_CASES = [s for n in CLASSES for s in ((n // 2 + 1, 200), (n, 131))]
ROW_CASES = [s for n in CLASSES for s in ((200, n // 2 + 1), (131, n))]
MIXED = (600, 1030)         # 1024 x 2048: neither axis in class 256
EMU_ONLY = (1030, 2050)     # 2048 x 4096; its long-double transform has 33 M points: too slow for a GPU test
GPU_CASES = COL_CASES + ROW_CASES + [MIXED]
EMU_CASES = GPU_CASES + [EMU_ONLY]
PREWHITE = (False, True)

# The shapes of GPU_CASES that reach each instantiation: class -> number of shapes, the same for all three kernels because every
# shape runs with prewhite off (cols2 + rows2) and on (cols + rows2).  3 kernels x 6 classes = 18 instantiations, each reached by
# at least two shapes; test_every_instantiation_is_reached_twice recomputes the table from the cases with next_pow2 and the rule
# of sspec_fast_supported.  (EMU_ONLY adds one to column class 2048 and row class 4096 on the interpreter.)
#            class:   256  512  1024  2048  4096  8192
COLS_SHAPES = {256: 14, 512: 2, 1024: 3, 2048: 2, 4096: 2, 8192: 2}     # by next_pow2(nf): sspec_cols_kernel, sspec_cols2_kernel
ROWS_SHAPES = {256: 14, 512: 2, 1024: 2, 2048: 3, 4096: 2, 8192: 2}     # by next_pow2(nt): sspec_rows2_kernel


def classes_of(shape):
    return next_pow2(shape[0]), next_pow2(shape[1])


def coverage(cases):
    cols, rows = {n: 0 for n in CLASSES}, {n: 0 for n in CLASSES}
    for nf, nt in cases:
        assert fast_supported(nf, nt), (nf, nt)
        cols[next_pow2(nf)] += 1
        rows[next_pow2(nt)] += 1
    return cols, rows


def group(shape, prewhite):
    """The tolerance group of a case: (axis, class, prewhite)."""
    if shape in COL_CASES:
        key = f"cols-{next_pow2(shape[0])}"
    elif shape in ROW_CASES:
        key = f"rows-{next_pow2(shape[1])}"
    else:
        key = "mixed"
    return key + ("-prewhite" if prewhite else "")


def case_id(shape):
    return f"{shape[0]}x{shape[1]}"


def dynspec_input(nf, nt):
    """Seeded white noise of unit variance on a mean of 3 plus a weak separable sinusoid (test_secondary_spectrum_two_trip_path):
    every bin's amplitude stays within a few orders of the largest, so no region of the frame is invisible."""
    rng = np.random.default_rng(nf * 1000 + nt)
    return rng.standard_normal((nf, nt)) + 3.0 + 0.5 * np.sin(0.07 * np.arange(nt))[None, :] * np.cos(0.11 * np.arange(nf))[:, None]


# ---- the persistent walk ----------------------------------------------------------------------------------------------------------
def persistent_grid(units, per_cu, cap=0):
    """persistent_grid of sspec.hip, restated: workgroups launched for `units` tiles / row groups under SCINT_SSPEC_MAXGRID = cap."""
    g = per_cu * CUS
    if cap > 0 and g > cap:
        g = cap
    if g > units:
        g = units
    if g >= 8:
        g &= ~7
    return max(g, 1)


def walk(shape, prewhite, cap=0):
    """{kernel: (class, units, grid, most iterations of one workgroup, xcd_remap)} of the persistent kernels of a call
    (launch_cols2, launch_rows2)."""
    nf, nt = shape
    nr, nc = classes_of(shape)
    nt_eff = nt - 1 if prewhite else nt
    out = {}
    if not prewhite:
        tiles = ceil_div(ceil_div(nt_eff, 2), spb(nr))
        g = persistent_grid(tiles, 1 if block(nr) >= 512 else 2, cap)
        out["cols2"] = (nr, tiles, g, ceil_div(tiles, g), g % 8 == 0)
    groups = ceil_div(nr, spb(nc))
    g = persistent_grid(groups, 1 if block(nc) >= 512 else 2, cap)
    out["rows2"] = (nc, groups, g, ceil_div(groups, g), g % 8 == 0)
    return out


def walk_shape(axis, n):
    """The first shape of the list, for class n of `axis` ("cols" / "rows"), at which the persistent kernel of that axis gives
    some workgroup two iterations under every cap (more than 8 units): column class 256 needs more than 128 column pairs, which
    no shape with nt in class 256 has -- it takes (200, 257) from the row cases; every other class walks at its first shape."""
    for shape in GPU_CASES:
        if classes_of(shape)[0 if axis == "cols" else 1] != n:
            continue
        w = walk(shape, False, max(CAPS))["cols2" if axis == "cols" else "rows2"]
        if w[0] == n and w[3] >= 2:
            return shape
    raise AssertionError((axis, n))


WALK_CASES = [(axis, n, walk_shape(axis, n)) for axis in ("cols", "rows") for n in CLASSES]
# one case per class for the axes of Dynspec.calc_sspec: the lower edge on the column axis, the full half on the row axis
AXES_CASES = [(n // 2 + 1, 200) if i % 2 == 0 else (131, n) for i, n in enumerate(CLASSES)]
