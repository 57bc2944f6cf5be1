"""The screen simulator (csrc/sim.hpp; scint_sim_screen / scint_sim_field / scint_sim_pulse) in EVERY class of the two FFT kernels it
is built from: the cases of tests/test_gpu_sim_classes.py (product build on a GPU) and tests/test_sim_classes_emu_cpu.py (the host
interpreter); the checks are tests/sim_class_checks.py.  tests/sim_cases.py stays the golden comparison at nx <= 512, ny <= 64; here
the reference is the host oracle (oracle/sim_oracle.py), which regenerates every expected value from the seed.

The simulator supplies its own loaders and storers, each (loader, storer) pair a template instantiation of fft_rows_kernel or
fft_cols_kernel of its own, so a class the FFT's own tests cover with the plain array functors is NOT thereby covered for these:

    fft_rows_kernel  SimScreenLoad -> SimRowStore     screen, rows            SimRowLoad -> SimFilterReduce   field, default route
                     SimRowLoad -> SimFilterStore     field, full route       SimRowLoad -> SimRowStore       field, full route
                     SimPulseLoad -> SimPulseStore    pulsewin
    fft_cols_kernel  ... -> SimRealStore  screen      SimPhaseLoad -> ...     both routes, the plane transform (batch = frequency)
                     ... -> SimSpeStore   g[kx][frequency], ncols = frequencies of the group     ... -> SimFullStore   full route

What decides a class is restated below from csrc/fft.hpp (`row_class`: launch_fft_rows; `col_plan`: make_col_plan) and every table
entry carries its expected class as a literal: a later change of the launcher or the planner makes the test of that entry say which
class lost its case.  The other axis is 16 and nf is 2 or 3 throughout: the smallest shapes that still reach the class."""
import math

SEED = 7
KEPT = 16                       # elements per thread of fft_rows_kernel (kEPT)


def screen(nx, ny):
    """Screen parameters under which the checks bite (the conditions are asserted from the oracle's arrays: sim_class_checks.strong):
    the golden case b's strength (mb2 = 200) on a sample spacing of 0.2 Fresnel scales, narrowed so that no axis is longer than
    12.8 Fresnel scales.  A Kolmogorov screen's rms phase grows as length^(5/6): at one spacing for all shapes the 2^17-point axis
    carries 1e5 rad, where the rounding of the PHASE (eps * 1e5 rad) and not the transform under test would decide the comparison."""
    return dict(mb2=200, dx=min(0.2, 12.8 / nx), dy=min(0.2, 12.8 / ny))


def kwargs(shape):
    nx, ny, nf = shape
    return dict(nx=nx, ny=ny, nf=nf, seed=SEED, **screen(nx, ny))


def ident(shape):
    return "x".join(str(n) for n in shape)


# ---- rows: launch_fft_rows, restated ----------------------------------------------------------------------------------------------
ROW_STAGES = {4: (16,), 5: (16, 2), 6: (16, 4), 7: (16, 8), 8: (16, 16), 9: (16, 16, 2), 10: (16, 16, 4), 11: (16, 16, 8),
              12: (16, 16, 16), 13: (16, 16, 16, 2)}


def row_class(n, nslots):
    """What launch_fft_rows(n, nslots, ...) launches for a storer that is no pair storer: the stage sequence, the split LDS exchange,
    threads per slot (the width Tr of SimFilterReduce's tree), slots per workgroup, workgroups, whether the last one has inactive
    slots, dynamic LDS bytes and whether that needs the hipFuncSetAttribute call."""
    l = n.bit_length() - 1
    assert 1 << l == n and 16 <= n <= 8192, n
    tr = n // KEPT
    block = max(tr, 128 if n <= 128 else 256)
    spb = block // tr
    split = 32 <= n <= 128
    lds = spb * (n + n // 16) * (8 if split else 16)
    return dict(stages=ROW_STAGES[l], split=split, tr=tr, waves_per_slot=max(1, tr // 64), slots_per_block=spb,
                blocks=-(-nslots // spb), idle_slots=(-nslots) % spb, lds=lds, set_attribute=lds > 64 * 1024)


def _row(nx, ny, nf, stages, split, tr, slots_per_block, idle_slots, lds_kib):
    return dict(shape=(nx, ny, nf), stages=stages, split=split, tr=tr, slots_per_block=slots_per_block, idle_slots=idle_slots,
                lds=int(lds_kib * 1024), set_attribute=lds_kib > 64)


# One table for all ten stage sequences (log2 ny = 4 .. 13), expected class as literals.  The field's row launches have nf * nx = 48
# slots: the last workgroup of 128 / 64 / 32 slots is not full (the inactive-slot edge: zero inputs, the `active` guards, scale[] not
# read past its end); from ny = 128 on a workgroup holds at most 16 slots and all are full.  tr = 128, 256, 512: ONE slot spans 2, 4, 8
# wavefronts, so the __syncthreads() inside SimFilterReduce's tree loop is what keeps its sum right.  From ny = 256 on the dynamic LDS
# (68 KiB; 136 KiB at 8192) is above 64 KiB and needs the hipFuncSetAttribute call.
ROW_CASES = [
    _row(16, 16, 3, (16,), False, 1, 128, 80, 34),
    _row(16, 32, 3, (16, 2), True, 2, 64, 16, 17),
    _row(16, 64, 3, (16, 4), True, 4, 32, 16, 17),
    _row(16, 128, 3, (16, 8), True, 8, 16, 0, 17),              # the last length with the split exchange
    _row(16, 256, 3, (16, 16), False, 16, 16, 0, 68),
    _row(16, 512, 3, (16, 16, 2), False, 32, 8, 0, 68),
    _row(16, 1024, 3, (16, 16, 4), False, 64, 4, 0, 68),        # a slot is exactly one wavefront
    _row(16, 2048, 3, (16, 16, 8), False, 128, 2, 0, 68),
    _row(16, 4096, 3, (16, 16, 16), False, 256, 1, 0, 68),
    _row(16, 8192, 3, (16, 16, 16, 2), False, 512, 1, 0, 136),
    # a multi-slot class with FULL workgroups and more than one of them on the screen's launch too (32 slots of 16 per workgroup)
    _row(32, 256, 5, (16, 16), False, 16, 16, 0, 68),
]

# SimFilterReduce's order: several slots per workgroup, and one slot across four wavefronts
REDUCE_CASES = [(16, 64, 3), (16, 4096, 3)]


# ---- columns: make_col_plan, restated ---------------------------------------------------------------------------------------------
def col_plan(length):
    """make_col_plan (csrc/fft.hpp): radix-16 passes first, the remainder last; a remainder of 2 widens the pass before it to 32."""
    l = length.bit_length() - 1
    assert 1 << l == length and length >= 2, length
    radix = []
    while l >= 4:
        radix.append(16)
        l -= 4
    if l > 0:
        if l == 1 and radix:
            radix[-1] = 32
        else:
            radix.append(1 << l)
    return tuple(radix)


# nx = 2^10 .. 2^17: three- and four-pass plans -- the un-scrambling last pass decodes 2 or 3 earlier digits (pre_radix) and ends in
# radix 4, 8, 16 or 32.  tests/sim_cases.py reaches one and two passes only.  Every launch of the simulator along x takes the plan:
# the screen (-> SimRealStore), the plane transform (SimPhaseLoad, batch = frequency), g[kx][frequency] with ncols = 3 (or 2) live
# lanes of a 64-thread workgroup (-> SimSpeStore) and, with SCINT_SIM_COLUMN=0, the inverse plane transform (-> SimFullStore).
# 2^17 is the simulator's limit (grid.y = nx / radix <= 65535): nf = 2 there keeps it light.  A frequency of 2^17 x 16 needs 66 MiB, so
# the default 128 MiB workspace holds ONE: two groups, g's transform with a single live column; every other case here is one group.
COL_CASES = [
    dict(shape=(1 << 10, 16, 3), plan=(16, 16, 4)),
    dict(shape=(1 << 11, 16, 3), plan=(16, 16, 8)),
    dict(shape=(1 << 12, 16, 3), plan=(16, 16, 16)),             # the column class of the documented 4096 x 128 workload
    dict(shape=(1 << 13, 16, 3), plan=(16, 16, 32)),
    dict(shape=(1 << 14, 16, 3), plan=(16, 16, 16, 4)),
    dict(shape=(1 << 15, 16, 3), plan=(16, 16, 16, 8)),
    dict(shape=(1 << 16, 16, 3), plan=(16, 16, 16, 16)),
    dict(shape=(1 << 17, 16, 2), plan=(16, 16, 16, 32)),
]

# ---- pulsewin: scint_sim_pulse, a row transform of 2 nf = 16 .. 8192 points (all ten stage sequences again, SimPulseLoad -> SimPulseStore)
# over nx = 16 slots; tests/sim_cases.py has 2 nf = 16 only.  nf = 4096 also makes the g transform a launch of 4096 columns.
PULSE_NF = [8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096]


def pulse_shape(nf):
    return (16, 16, nf)


# ---- the tiled column route inside the simulator ----------------------------------------------------------------------------------
# Product build, GPU only: one group of 2560 frequencies is 256 * 32 * 2560 * 16 B = 320 MiB of planes, beyond run_cols_fft's
# 300 MiB; a caller gets there by passing group_bytes above the default.  ONE tiled launch with batches = 2560 and a batch-indexed
# first loader (SimPhaseLoad); class (16, 16).  The workspace is 0.67 GB, the host oracle about 2 s.
TILED_GPU = (256, 32, 2560)
# Interpreter only, the -DSCINT_COLS_CACHE_BYTES=0.0 build of tests/fft_tiled_cases.py: every transform along x of 256 .. 16384
# points is tiled -- the screen, the planes (batches = 3), the full route's inverse, and g, ONE tile with 3 live columns of 16 into
# SimSpeStore (the s.ok guard).  nx runs over fft_tiled_cases.CLASSES.
TILED_EMU_NY, TILED_EMU_NF = 16, 3


def freq_bytes(nx, ny):
    """sim_freq_bytes (csrc/fft.hip): two [nx][ny] complex planes and one column of g per frequency of a group."""
    return 16 * (2 * nx * ny + nx)


def group_of(nx, ny, nf, group_bytes):
    """Frequencies per group for a workspace of scint_sim_field_workspace_bytes(nx, ny, G) bytes sized from `group_bytes` as
    Simulation.get_intensity sizes it."""
    per = freq_bytes(nx, ny)
    one = per + 768
    return int(min(nf, max(1, 1 + (int(group_bytes) - one) // per), 4096, (1 << 28) // nx))


def groups_of(nx, ny, nf, group_bytes):
    return math.ceil(nf / group_of(nx, ny, nf, group_bytes))
