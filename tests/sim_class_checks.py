"""The checks of the screen simulator's class coverage (cases and what each is there for: tests/sim_class_cases.py), shared by the GPU
tests (tests/test_gpu_sim_classes.py) and the host-interpreter tests (tests/test_sim_classes_emu_cpu.py): `S` is
scintools_amd.scint_sim bound to a GPU or to the interpreter, `backend` names the build ('gpu', 'emu', 'emu_tiled').

Reference: oracle/sim_oracle.py (NumPy float64 transforms, bit-pinned to the unmodified reference by tests/test_oracle_golden.py),
one run per shape, shared and read-only.  The oracle keeps neither xyi nor pulsewin; they are formed here:
    xyi       |ifft2(frfilt3(fft2(exp(1j xyp scale_last))))|^2 with the oracle's own _frfilt3 and xyp
    pulsewin  transpose(roll(|fft(spe blackman(nf), 2 nf)|^2, nf)) from the DEVICE's own complex64 spe: both sides transform
              identical inputs, so what is compared is the 2 nf-point transform, the window, |.|^2 and the roll.

Tolerances: those of tests/sim_checks.py, unchanged -- xyp_bounds, spe_close, intensity_close, 1e-12 of the maximum for xyi.  One
new bound, pulsewin against the expression above: 2e-12 max(ref) -- the project's FFT tolerance, 1e-12 of the maximum, on the
amplitude, squared as intensity_close squares spe's (d|z|^2 = 2 |z| d|z|).

The inputs must make the checks bite: spe is compared after rounding to complex64, so in a nearly unscattered field a dropped
partial sum hides under 2^-22 |spe|.  `strong` asserts from the ORACLE's arrays (conditions on the inputs, not measurements of the
code under test): rms(xyp) >= pi, and at the middle frequency the unscattered mode holds |F[0,0]|^2 <= 0.05 sum|F|^2."""
import ctypes
import functools
import time

import numpy as np

import sim_class_cases as cc
from sim_checks import column_switch, intensity_close, spe_close, xyp_bounds

PULSE_TOL = 2e-12


def _freeze(obj):
    for v in vars(obj).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return obj


def scale_of(o, ifreq):
    return 1 / (1.0 + o.dlam * (-0.5 + ifreq / o.nf))                    # scint_sim.py:218-224, lamsteps=False


@functools.lru_cache(maxsize=None)
def oracle(shape):
    """The oracle's run of a shape with xyi added (the plane of the last frequency), read-only."""
    from oracle.sim_oracle import Simulation
    o = Simulation(**cc.kwargs(shape))
    sc = scale_of(o, o.nf - 1)
    o.xyi = np.abs(np.fft.ifft2(o._frfilt3(np.fft.fft2(np.exp(1j * o.xyp * sc)), sc))) ** 2
    return _freeze(o)


def strong(shape):
    """The strong-screen conditions on the inputs, from the oracle's arrays."""
    o = oracle(shape)
    rms = float(np.sqrt(np.mean(o.xyp ** 2)))
    P = np.abs(np.fft.fft2(np.exp(1j * o.xyp * scale_of(o, o.nf // 2)))) ** 2
    share = float(P[0, 0] / P.sum())
    print(f"{cc.ident(shape)} screen: rms(xyp) {rms:.2f} rad, unscattered share {share:.2e}")
    assert rms >= np.pi, (shape, rms)
    assert share <= 0.05, (shape, share)


_runs = {}


def run(S, backend, shape, column=True, **kw):
    """The simulation of a shape on this backend and route, computed once, arrays read-only; the route is asserted."""
    key = (backend, shape, column) + tuple(sorted(kw.items()))
    if key not in _runs:
        _runs[key] = fresh(S, shape, column, **kw)
    return _runs[key]


def fresh(S, shape, column=True, groups=None, **kw):
    t0 = time.perf_counter()
    with column_switch(None if column else "0"):
        s = S.Simulation(**cc.kwargs(shape), **kw)
        route = S.last_route()
    s.seconds = time.perf_counter() - t0
    assert route[0] is column, (shape, route)
    if groups is not None:
        assert route == (column, groups), (shape, route)
    return _freeze(s)


def workspace_bytes(nx, ny, group):
    from scintools_amd import _lib
    need = ctypes.c_size_t()
    _lib.check(_lib.load().scint_sim_field_workspace_bytes(nx, ny, group, ctypes.byref(need)), "workspace_bytes")
    assert need.value == cc.freq_bytes(nx, ny) * group + 768
    return need.value


def compare(what, s, o):
    """One simulation against the oracle: xyp, spe, spi / dyn, xyi.  Prints every figure, then asserts; returns the share of spe
    elements not bit-identical to the oracle's."""
    nx, ny, nf = o.nx, o.ny, o.nf
    assert s.xyp.shape == (nx, ny) and s.xyp.dtype == np.float64
    rms_tol, max_tol = xyp_bounds(o.xyp)
    d = s.xyp - o.xyp
    rms, worst = float(np.sqrt(np.mean(d ** 2))), float(np.abs(d).max())
    assert s.spe.shape == (nx, nf) and s.spe.dtype == np.complex64 and s.spi.shape == (nx, nf) and s.spi.dtype == np.float32
    differ = float(np.mean(s.spe != o.spe))
    spe_err = float((np.abs(s.spe - o.spe) / (2.0 ** -22 * np.abs(o.spe) + 1e-12 * np.abs(o.spe).max())).max())
    xyi_err = float(np.abs(s.xyi - o.xyi).max() / o.xyi.max())
    print(f"{what}: xyp rms {rms / rms_tol:.3f} max {worst / max_tol:.4f} of their bounds; spe worst element {spe_err:.3f} of its bound, "
          f"not bit-identical {int(np.sum(s.spe != o.spe))} of {s.spe.size} ({differ:.1e}); xyi {xyi_err:.2e} of its maximum (bound 1e-12); constructor {1e3 * s.seconds:.1f} ms")
    assert rms <= rms_tol and worst <= max_tol
    assert spe_close(s.spe, o.spe)
    assert intensity_close(s.spi, o.dyn.T)
    assert s.dyn.shape == (nf, nx) and s.dyn.dtype == o.dyn.dtype and intensity_close(s.dyn, o.dyn)
    assert s.xyi.shape == (nx, ny) and np.abs(s.xyi - o.xyi).max() <= 1e-12 * o.xyi.max()
    return differ


def check_both_routes(S, backend, shape):
    """A shape on the default (column) route and with SCINT_SIM_COLUMN=0, each against the oracle, and against each other."""
    nx, ny, nf = shape
    strong(shape)
    o = oracle(shape)
    # the groups of the default workspace, restated: ONE for every shape but 2^17 x 16, whose frequencies need 66 MiB each
    groups = cc.groups_of(nx, ny, nf, S.SIM_GROUP_BYTES)
    assert groups == (nf if nx * ny == 1 << 21 else 1)
    col = run(S, backend, shape, True, groups=groups)
    full = run(S, backend, shape, False, groups=groups)
    differ = compare(f"{cc.ident(shape)} column route", col, o), compare(f"{cc.ident(shape)} full route", full, o)
    print(f"{cc.ident(shape)} column vs full: spe elements not bit-identical {int(np.sum(col.spe != full.spe))} of {col.spe.size}")
    assert spe_close(col.spe, full.spe)
    assert np.array_equal(col.xyp, full.xyp)                             # the screen does not depend on the route
    assert np.abs(col.xyi - full.xyi).max() <= 1e-12 * col.xyi.max()
    return differ


def check_row_class(S, backend, case):
    """The class table entry against the restated launcher, then both routes."""
    nx, ny, nf = case["shape"]
    field = cc.row_class(ny, nf * nx)                                    # SimRowLoad -> SimFilterReduce / SimFilterStore / SimRowStore
    for k in ("stages", "split", "tr", "slots_per_block", "idle_slots", "lds", "set_attribute"):
        assert field[k] == case[k], (case["shape"], k, field[k], case[k])
    assert int(np.prod(case["stages"])) == ny and case["tr"] * case["slots_per_block"] == max(case["tr"], 128 if ny <= 128 else 256)
    return check_both_routes(S, backend, case["shape"])


def check_col_plan(S, backend, case):
    nx, ny, nf = case["shape"]
    plan = cc.col_plan(nx)
    assert plan == case["plan"] and int(np.prod(plan)) == nx, (nx, plan)
    assert len(plan) in (3, 4) and all(nx // r <= 65535 for r in plan)   # grid.y of every pass
    import fft_tiled_cases as tc
    assert not tc.tiled(nx, ny, batches=nf) and not tc.tiled(nx, nf)     # the radix passes, not the tiled ones, in the product build
    return check_both_routes(S, backend, case["shape"])


def check_reduce_order(S, backend, shape):
    """SimFilterReduce's slot reduction has a fixed order: two runs give equal bits, and groups of 2 + 1 frequencies the bits of
    one group of 3 (g is then [kx][2] and [kx][1] instead of [kx][3]: other slots share a workgroup, the sums must not change)."""
    nx, ny, nf = shape
    assert nf == 3
    whole = run(S, backend, shape, True, groups=1)
    again = fresh(S, shape, True, groups=1)
    for k in ("spe", "spi", "xyp", "xyi", "w"):
        assert np.array_equal(getattr(again, k), getattr(whole, k)), (shape, k)
    need = workspace_bytes(nx, ny, 2)
    assert cc.groups_of(nx, ny, nf, need) == 2
    part = fresh(S, shape, True, groups=2, group_bytes=need)
    for k in ("spe", "spi", "xyi"):
        assert np.array_equal(getattr(part, k), getattr(whole, k)), (shape, k)
    assert spe_close(whole.spe, oracle(shape).spe)


def pulse_reference(spe, nf):
    """get_pulse (scint_sim.py:267-270) in NumPy from a given complex64 spe."""
    p = np.fft.fft(spe * np.blackman(nf), 2 * nf)
    return np.transpose(np.roll(np.real(p * np.conj(p)), nf)), np.real(p * np.conj(p))


def check_pulse(S, backend, nf):
    shape = cc.pulse_shape(nf)
    nx = shape[0]
    row = cc.row_class(2 * nf, nx)
    assert row["stages"] == cc.ROW_STAGES[(2 * nf).bit_length() - 1] and int(np.prod(row["stages"])) == 2 * nf
    strong(shape)
    o = oracle(shape)
    s = run(S, backend, shape, True, groups=1)
    differ = float(np.mean(s.spe != o.spe))
    print(f"{cc.ident(shape)}: spe not bit-identical {int(np.sum(s.spe != o.spe))} of {s.spe.size} ({differ:.1e}); constructor {1e3 * s.seconds:.1f} ms")
    assert spe_close(s.spe, o.spe) and intensity_close(s.dyn, o.dyn)
    t0 = time.perf_counter()
    pw = s.pulsewin
    seconds = time.perf_counter() - t0
    ref, power = pulse_reference(s.spe, nf)
    assert ref.shape == (2 * nf, nx)
    err = float(np.abs(pw - ref).max() / ref.max())
    print(f"pulsewin 2 nf = {2 * nf}: max |diff| / max {err:.2e} (bound {PULSE_TOL:.0e}); {1e3 * seconds:.1f} ms")
    assert pw.shape == (2 * nf, nx) and pw.dtype == np.float64
    assert np.abs(pw - ref).max() <= PULSE_TOL * ref.max()
    # np.roll without an axis rolls the FLATTENED [nx, 2 nf] array: the upper half of a row's transform lands in the next row, and the
    # last row's upper half wraps (SimPulseStore: o >= total) into row 0's lower half.  The comparison above covers it; by name:
    assert np.abs(pw[:nf, 0] - power[nx - 1, nf:]).max() <= PULSE_TOL * ref.max()
    assert np.abs(pw[:nf, 1] - power[0, nf:]).max() <= PULSE_TOL * ref.max()
    return differ


def check_tiled_gpu(S, backend):
    """The tiled column passes with batches > 1 in ONE launch, product build: a group of 2560 frequencies beyond 300 MiB."""
    import fft_tiled_cases as tc
    shape = cc.TILED_GPU
    nx, ny, nf = shape
    assert tc.tiled(nx, ny, batches=nf) and tc.class_of(nx) == (16, 16)
    assert not tc.tiled(nx, nf)                                          # g[kx][frequency] stays on the radix passes
    default_group = cc.group_of(nx, ny, nf, S.SIM_GROUP_BYTES)
    assert not tc.tiled(nx, ny, batches=default_group)                   # the default grouping is not beyond the threshold
    strong(shape)
    o = oracle(shape)
    need = workspace_bytes(nx, ny, nf)
    assert cc.group_of(nx, ny, nf, need) == nf
    big = fresh(S, shape, True, groups=1, group_bytes=need)
    small = run(S, backend, shape, True, groups=cc.groups_of(nx, ny, nf, S.SIM_GROUP_BYTES))
    d_big, d_small = compare(f"{cc.ident(shape)} one tiled group", big, o), compare(f"{cc.ident(shape)} default groups", small, o)
    print(f"{cc.ident(shape)} tiled vs radix passes: spe elements not bit-identical {int(np.sum(big.spe != small.spe))} of {big.spe.size}")
    assert spe_close(big.spe, small.spe)                                 # the two routes round differently: not bit for bit
    return d_big, d_small


def check_tiled_emu(S, backend, nx):
    """-DSCINT_COLS_CACHE_BYTES=0.0: every transform along x is tiled, g's too (one tile, 3 live columns of 16)."""
    import fft_tiled_cases as tc
    shape = (nx, cc.TILED_EMU_NY, cc.TILED_EMU_NF)
    assert tc.tiled(nx, shape[1], batches=shape[2], cache_bytes=0.0) and tc.tiled(nx, shape[2], cache_bytes=0.0)
    assert not tc.tiled(nx, shape[1], batches=shape[2])
    assert tc.class_of(nx) == {256: (16, 16), 512: (32, 16), 1024: (32, 32), 2048: (64, 32), 4096: (64, 64), 8192: (128, 64),
                               16384: (128, 128)}[nx]
    return check_both_routes(S, backend, shape)
