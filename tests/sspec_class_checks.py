"""Checks of calc_sspec's two-trip kernels (csrc/sspec.hip) in every length class, shared by the host-interpreted tests
(tests/test_sspec_classes_emu_cpu.py) and the GPU tests (tests/test_gpu_sspec_classes.py).  The cases, and what each is there for:
tests/sspec_class_cases.py.

Reference: oracle/sspec_oracle.calc_sspec (halve) restated in np.longdouble -- both means, the window and the 2 x 2 prewhitening
difference in long double, scipy.fft.fft2 on the long-double array (it keeps clongdouble; asserted), the post-darkening in long
double with its [0, :] and [:, C/2] entries set to 1 -- as LINEAR power.  The float64 oracle runs beside it as "the reference
alone".

Metric: the transform's forward error.  Linear power relative to the peak hides most of a prewhitened frame behind its
low-frequency corner (the post-darkening divides by sin^2 sin^2 down to 1e-13), and the suite's usual "dB of strong bins to 1e-8
of the float64 oracle" is no property of the kernel there: the division amplifies the FFT's rounding in exactly the bins it
makes strong, and the device is closer to the long-double evaluation than NumPy is.  So the post-darkening is taken out again:
with D the float64 post-darkening array (all ones without prewhite), A = sqrt(P D) for device and reference alike, and

    err = max |A_dev - A_ld| / max A_ld,

the project's "of max|ref|" measure for transforms.  The same number is formed for the float64 oracle, and linear power relative
to the peak is printed for both so that the figures can be set beside the existing tests'.

Bound: tests/golden/sspec_class_tolerances.json, written by tests/golden/make_sspec_class_tolerances.py from the float64 oracle
alone -- per group (axis, class, prewhite) 8 x the oracle's worst amplitude error over the group's cases, at least 64 eps.  The
device's radix-16 stages and pocketfft's mixed radix factor the transform differently, so equal errors are not expected; the
factor covers that spread.  It does not cover an error of another kind: a misplaced or dropped element is at least 1e-3 in this
metric.  No bound may reach 1e-10 (checked): beyond that the case, not the factor, would have to change.

The persistent walk: SCINT_SSPEC_MAXGRID (read per call, in the product too) caps the workgroups of the persistent kernels at
1, 3, 8 and 13 -- 3 runs without the XCD remap, 8 with it, 13 rounds down to 8.  Each capped result must have the bits of the
uncapped launch's, and the restated persistent_grid must say that some workgroup of the kernel under test ran twice or more.

That the cases can fail was shown once on copies of sspec.hip with one line changed each (interpreted build, all 84 tests of
tests/test_sspec_classes_emu_cpu.py; the walk tests compare two launches of the same build and fail in none of these):
    columns, prewhite path only: class 8192 dispatched as <16,16,8,4>
            nothing fails, and nothing should: sspec_cols_kernel runs the generic slot_fft, for which 16 * 16 * 8 * 4 is as good
            a factorisation of 8192 as 16 * 16 * 16 * 2 (the persistent kernels refuse it at compile time: StageW's static_assert)
    ... dispatched as class 4096's <16,16,16,1>
            both prewhite cases of column class 8192 fail (4097x200, 8192x131)
    cols2: `(ok && has1) ? d01 : 0.0` -> `ok ? d01 : 0.0` (the zeroing of a last pair's missing column)
            nothing fails, and nothing can: the column is element nt_eff of every row, which sspec_rows2_kernel zeroes itself
    rows2: the zeroing of a short row's tail (`t + m * Tr < a.nt_eff` dropped from `ok`)
            46 of 52 class tests fail: every case but the six whose row fills its half (131 x n without prewhite)
    StageW::load: `w[2] = stage_w<R3>(t, ...)` -> `(t + 1, ...)` (the twiddle of the stage only R3 > 1 runs)
            class 8192 alone: 4097x200 and 8192x131 without prewhite (cols2), 200x4097 and 131x8192 with and without (rows2)
    sspec_fast: `ra.nt_eff = nt_eff` -> `nt`
            even nt passes, rightly (the extra element is the zeroed second column of the last pair); at the first odd nt under
            prewhite, 256x131, the row kernel reads past the intermediate and the interpreter aborts the run
"""
import functools
import json
import os
import time

import numpy as np

import sspec_class_cases as cc

HERE = os.path.dirname(os.path.abspath(__file__))
TOLERANCES = os.path.join(HERE, "golden", "sspec_class_tolerances.json")
LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
FACTOR, FLOOR, CEILING = 8.0, 64 * EPS, 1e-10
DT, DF = 30.0, 1.0


# ---- the references ---------------------------------------------------------------------------------------------------------------
def _window_ld(n, frac=0.1):
    """scint_utils.get_window's hanning taper with a flat middle (oracle/sspec_oracle.get_window), in long double."""
    m = int(np.floor(frac * n))
    pi = 4 * np.arctan(LD(1))
    w = (LD(0.5) - LD(0.5) * np.cos(2 * pi * np.arange(m, dtype=LD) / LD(m - 1))) if m > 1 else np.ones(m, dtype=LD)
    return np.insert(w, int(np.ceil(m / 2)), np.ones(n - m, dtype=LD))


def postdark(nrfft, ncfft, dtype=np.float64):
    """The post-darkening array [nrfft / 2, ncfft] of dynspec.py:3704-3717, row 0 and column C/2 set to 1."""
    pi = 4 * np.arctan(LD(1)) if dtype is LD else np.pi
    fd = np.arange(-ncfft // 2, ncfft // 2).astype(dtype)
    td = np.arange(0, nrfft // 2).astype(dtype)
    v1 = np.sin(pi / dtype(ncfft) * fd) ** 2
    v2 = np.sin(pi / dtype(nrfft) * td) ** 2
    pd = v2[:, None] * v1[None, :]
    pd[:, ncfft // 2] = 1
    pd[0, :] = 1
    return pd


def sspec_ld(dyn, prewhite):
    """calc_sspec (halve, hanning window of 0.1) in long double: LINEAR power [nrfft / 2, ncfft]."""
    import scipy.fft
    nf, nt = dyn.shape
    x = dyn.astype(LD)
    x = x - x.sum() / LD(x.size)
    x = _window_ld(nt)[None, :] * x
    x = _window_ld(nf)[:, None] * x
    x = x - x.sum() / LD(x.size)
    if prewhite:
        x = x[1:, 1:] - x[1:, :-1] - x[:-1, 1:] + x[:-1, :-1]          # convolve2d([[1, -1], [-1, 1]], x, 'valid')
    nrfft, ncfft = 2 * cc.next_pow2(nf), 2 * cc.next_pow2(nt)
    f = scipy.fft.fft2(x, s=[nrfft, ncfft])
    assert f.dtype == np.clongdouble, f.dtype
    p = f.real ** 2 + f.imag ** 2
    del f
    p = np.roll(p, (nrfft // 2, ncfft // 2), axis=(0, 1))[nrfft // 2:]
    if prewhite:
        p = p / postdark(nrfft, ncfft, LD)
    return p


class Case:
    """Input and both references of one (shape, prewhite), built once (`case`) and never written again."""

    def __init__(self, shape, prewhite):
        from oracle import sspec_oracle
        nf, nt = shape
        self.shape, self.prewhite = shape, prewhite
        self.dyn = cc.dynspec_input(nf, nt)
        self.nrfft, self.ncfft = 2 * cc.next_pow2(nf), 2 * cc.next_pow2(nt)
        self.D = postdark(self.nrfft, self.ncfft) if prewhite else None
        t0 = time.perf_counter()
        self.P_ld = sspec_ld(self.dyn, prewhite)
        self.ld_seconds = time.perf_counter() - t0
        self.A_ld = self.amplitude(self.P_ld)
        self.fdop, self.tdel, self.sec_oracle = sspec_oracle.calc_sspec(self.dyn, DT, DF, prewhite=prewhite)
        for a in (self.dyn, self.P_ld, self.A_ld, self.sec_oracle):
            a.setflags(write=False)

    def amplitude(self, power):
        """A = sqrt(P D): the transform's modulus, the post-darkening taken out again."""
        power = power.astype(LD)
        return np.sqrt(power * self.D if self.prewhite else power)

    def errors(self, sec_db):
        """(amplitude error of max A_ld, linear-power error of the peak) of a spectrum in dB against the long-double reference."""
        power = 10 ** (sec_db.astype(LD) / 10)
        amp = float(np.abs(self.amplitude(power) - self.A_ld).max() / self.A_ld.max())
        lin = float(np.abs(power - self.P_ld).max() / self.P_ld.max())
        return amp, lin


@functools.lru_cache(maxsize=2)
def case(shape, prewhite):
    return Case(shape, prewhite)


def tolerances():
    with open(TOLERANCES) as fh:
        return json.load(fh)


def check_tolerance_file():
    """Every group of the cases has a bound, every bound is FACTOR x the recorded oracle error or the floor, none reaches 1e-10."""
    tol = tolerances()
    groups = {cc.group(s, pw) for s in cc.EMU_CASES for pw in cc.PREWHITE}
    assert set(tol) == groups, sorted(groups ^ set(tol))
    for key, t in tol.items():
        assert t["bound"] == max(FACTOR * t["oracle_amplitude_error"], FLOOR), key
        assert t["bound"] < CEILING, (key, t["bound"])


# ---- the device side --------------------------------------------------------------------------------------------------------------
def device_sspec(dyn, prewhite):
    import torch
    from scintools_amd.device import to_device
    from scintools_amd.dynspec import sspec_device
    return sspec_device(to_device(dyn, torch.float64), prewhite=prewhite).cpu().numpy()


def check_finite(c, sec, bound):
    """No NaN and no +inf anywhere; -inf (a power of exactly zero) only where the spectrum IS zero in exact arithmetic:
      * the bin (delay 0, Doppler 0): the second mean is subtracted, so the samples sum to zero;
      * under prewhite the whole Doppler-0 column C/2 and the whole delay-0 row: the window's end values are 0, so the first and the
        last column (row) hold -mean2 throughout, and the 2 x 2 difference telescopes to zero along each row (column).
    What a float64 evaluation leaves there is rounding, and which of these bins round to exactly 0 is luck: the interpreter gives
    -inf in three of them at 129 x 200, the float64 oracle in others.  That the bins are of that kind is asserted on the long-double
    reference (they stay below the bound of the case); everywhere else the output must be finite."""
    assert not np.isnan(sec).any() and not np.isposinf(sec).any(), (int(np.isnan(sec).sum()), int(np.isposinf(sec).sum()))
    zero = np.zeros(sec.shape, dtype=bool)
    zero[0, c.ncfft // 2] = True
    if c.prewhite:
        zero[:, c.ncfft // 2] = True
        zero[0, :] = True
    assert float(c.A_ld[zero].max() / c.A_ld.max()) <= bound
    assert np.isfinite(sec[~zero]).all(), f"{int((~np.isfinite(sec[~zero])).sum())} values are infinite outside the zero bins"


def check_class(shape, prewhite, where):
    """One case: shape, finiteness, and the amplitude error against the long-double reference within the group's bound."""
    c = case(shape, prewhite)
    bound = tolerances()[cc.group(shape, prewhite)]["bound"]
    t0 = time.perf_counter()
    sec = device_sspec(np.array(c.dyn), prewhite)       # (a copy: the case's arrays are read-only)
    seconds = time.perf_counter() - t0
    assert sec.shape == (c.nrfft // 2, c.ncfft) == c.sec_oracle.shape
    check_finite(c, sec, bound)
    amp, lin = c.errors(sec)
    o_amp, o_lin = c.errors(c.sec_oracle)
    nr, nc = cc.classes_of(shape)
    print(f"SSPECCLASS {where} {cc.case_id(shape)} prewhite={int(prewhite)} classes {nr}x{nc} group {cc.group(shape, prewhite)}: "
          f"amplitude device {amp:.2e} oracle {o_amp:.2e} bound {bound:.2e}; linear power device {lin:.2e} oracle {o_lin:.2e}; "
          f"call {seconds:.2f} s, long-double reference {c.ld_seconds:.2f} s")
    assert amp <= bound, (shape, prewhite, amp, bound)
    return amp, o_amp, bound


def check_axes(shape):
    """fdop and tdel of Dynspec.calc_sspec equal the oracle's, and its spectrum is sspec_device's."""
    from oracle import sspec_oracle
    from scintools_amd.dynspec import Dynspec
    nf, nt = shape
    dyn = cc.dynspec_input(nf, nt)
    fdop, tdel, _ = sspec_oracle.calc_sspec(dyn, DT, DF)

    class Holder:
        pass
    h = Holder()
    h.dyn, h.freqs, h.times = dyn, 1400.0 + DF * np.arange(nf), DT * np.arange(nt)
    d = Dynspec(dyn=h, verbose=False)
    d.calc_sspec()
    assert d.fdop.shape == (2 * cc.next_pow2(nt),) and d.tdel.shape == (cc.next_pow2(nf),)
    assert np.array_equal(d.fdop, fdop) and np.array_equal(d.tdel, tdel)
    assert np.array_equal(np.array(d.sspec), device_sspec(dyn, False))


def check_walk(monkeypatch, axis, n, shape, prewhite):
    """The capped launches have the bits of the uncapped one; from persistent_grid's formula, every capped launch gives some
    workgroup of the kernel under test -- the class-n kernel of `axis`; under prewhite the column kernel is the one-shot form, and
    the row kernel is the one that walks -- at least two iterations.  (The default launch is no walk-free yardstick: it rounds its
    grid down to whole rounds of eight, so 9 tiles run on 8 workgroups.  It is the launch every other test checks.)"""
    dyn = cc.dynspec_input(*shape)
    kernel = "cols2" if axis == "cols" and not prewhite else "rows2"
    monkeypatch.delenv("SCINT_SSPEC_MAXGRID", raising=False)
    ref = device_sspec(dyn, prewhite)
    free = cc.walk(shape, prewhite)[kernel]
    if kernel == "cols2" or axis == "rows":
        assert free[0] == n
    for cap in cc.CAPS:
        cls, units, grid, iters, remap = cc.walk(shape, prewhite, cap)[kernel]
        assert iters >= 2 and grid == {1: 1, 3: 3, 8: 8, 13: 8}[cap] and remap == (cap >= 8), (shape, cap, units, grid, iters)
        monkeypatch.setenv("SCINT_SSPEC_MAXGRID", str(cap))
        got = device_sspec(dyn, prewhite)
        same = np.array_equal(got.view(np.uint64), ref.view(np.uint64))
        print(f"SSPECWALK {axis}-{n} {cc.case_id(shape)} prewhite={int(prewhite)} cap {cap}: {kernel} class {cls}, {units} units on "
              f"{grid} workgroups, {iters} iterations, remap {int(remap)}: {'same bits' if same else 'DIFFERENT'}")
        assert same, (shape, prewhite, cap, int((got.view(np.uint64) != ref.view(np.uint64)).sum()))
    monkeypatch.delenv("SCINT_SSPEC_MAXGRID", raising=False)
