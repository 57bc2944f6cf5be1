"""Checks of the single calls scint_acf and scint_sspec (generic route) now that they are the B = 1 of the stacked routes
(csrc/fft.hip: acf_stack, sspec_generic), shared by the GPU tests (tests/test_gpu_single_route.py) and the host-interpreted ones
(tests/test_single_route_emu_cpu.py).  `sp` is scintools_amd.scintpar.

The shapes are the smallest at which each branch exists: (2, 5) the smallest spectrum there is (one row left under prewhitening),
(3, 7) odd lengths, (16, 16) powers of two, (33, 20) more rows than one padded power of two below; (1, 1) the smallest ACF, (3, 5)
odd (chirp-z on both axes), (16, 16) the power-of-two route.  Per shape and option:

  a. the stack of one (scint_*_batch with B = 1) and the single call agree bit for bit;
  b. the single call succeeds in a workspace of exactly scint_*_workspace_bytes bytes -- that size is ABI and older than the shared
     carve -- and returns SCINT_E_WORKSPACE with one byte less;
  c. the single call keeps a reference that shares no code with it: oracle/sspec_oracle.py's calc_sspec to the bounds of
     tests/test_gpu_parity.py (1e-10 of the peak in linear power, 1e-8 dB where the power is above 1e-6 of the peak), and for the
     ACF oracle/sspec_oracle.py's calc_acf and its statement with the two flags, tests/acf_batch_cases.numpy_acf, to the 1e-12 of the
     maximum of tests/acf_batch_checks.py.  (tests/acf_oracle.py is the oracle of the theoretical ACF MODEL, not of calc_acf.)

The windows are Hanning tapers over half of each axis (window_frac = 0.5), so that they are not all ones at these sizes."""
import ctypes

import numpy as np

import acf_batch_cases as cc

SSPEC_SHAPES = [(2, 5), (3, 7), (16, 16), (33, 20)]
SSPEC_FLAGS = [(False, True), (True, True), (False, False)]      # (prewhite, halve); prewhite needs halve
WINDOWS = [None, "hanning"]                                       # none, both
WINDOW_FRAC = 0.5
ACF_SHAPES = [(1, 1), (3, 5), (16, 16)]
ACF_FLAGS = [(False, False), (False, True), (True, False), (True, True)]      # (subtract_mean, normalise)
ACF_TOL = 1e-12
SCINT_E_WORKSPACE = 3
_cache = {}


def dyn(nf, nt):
    """The shape's dynamic spectrum (built once, shared: do not write into it): a positive flux with unit mean and 30 % scatter."""
    if (nf, nt) not in _cache:
        x = 1.0 + 0.3 * np.random.default_rng(100 * nf + nt).standard_normal((nf, nt))
        x.setflags(write=False)
        _cache[nf, nt] = x
    return _cache[nf, nt]


def to_dev(sp, a):
    import torch
    return sp.device.to_device(np.array(a), torch.float64)


def bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint64)


def _need(sp, name, *args):
    need = ctypes.c_size_t()
    assert getattr(sp._lib.load(), name)(*args, ctypes.byref(need)) == 0
    return need.value


# ---- the secondary spectrum ---------------------------------------------------------------------------------------------------
def check_sspec_stack_of_one(sp, nf, nt):
    from scintools_amd import dynspec
    x = to_dev(sp, dyn(nf, nt))
    for prewhite, halve in SSPEC_FLAGS:
        for window in WINDOWS:
            kw = dict(prewhite=prewhite, halve=halve, window=window, window_frac=WINDOW_FRAC)
            one = bits(dynspec.sspec_device(x, **kw))
            got = bits(dynspec.sspec_stack_device(x[None], **kw))
            assert got.shape == (1,) + one.shape and np.array_equal(got[0], one), (nf, nt, kw, int((got[0] != one).sum()))


def check_sspec_workspace(sp, nf, nt):
    import torch
    from scintools_amd import dynspec
    lib, ptr = sp._lib.load(), sp.device.ptr
    x = to_dev(sp, dyn(nf, nt))
    need = _need(sp, "scint_sspec_workspace_bytes", nf, nt)
    ws = sp.device.empty((need,), torch.uint8)
    nrfft, ncfft = 2 * 2 ** int(np.ceil(np.log2(nf))), 2 * 2 ** int(np.ceil(np.log2(nt)))
    for prewhite, halve in SSPEC_FLAGS:
        for window in WINDOWS:
            wt, wf = dynspec._window_tables(nt, nf, window, WINDOW_FRAC, torch.cuda.current_device())
            pd_fd, pd_td = dynspec._postdark_tables(nrfft, ncfft, torch.cuda.current_device()) if prewhite else (None, None)
            out = sp.device.empty((nrfft // 2 if halve else nrfft, ncfft), torch.float64)
            args = (ptr(x), nf, nt, ptr(wt), ptr(wf), int(prewhite), int(halve), ptr(pd_fd), ptr(pd_td), ptr(out), ptr(ws))
            assert lib.scint_sspec(*args, need - 1, None) == SCINT_E_WORKSPACE, (nf, nt, prewhite, halve, window)
            assert lib.scint_sspec(*args, need, None) == 0, (nf, nt, prewhite, halve, window, sp._lib.last_error())
            ref = dynspec.sspec_device(x, prewhite=prewhite, halve=halve, window=window, window_frac=WINDOW_FRAC)
            assert np.array_equal(bits(out), bits(ref)), (nf, nt, prewhite, halve, window)


def check_sspec_oracle(sp, nf, nt):
    from oracle import sspec_oracle as so
    from scintools_amd import dynspec
    x = dyn(nf, nt)
    for prewhite, halve in SSPEC_FLAGS:
        for window in WINDOWS:
            kw = dict(prewhite=prewhite, halve=halve, window=window, window_frac=WINDOW_FRAC)
            sec = dynspec.sspec_device(to_dev(sp, x), **kw).cpu().numpy()
            ref = so.calc_sspec(x, 30.0, 0.1, **kw)[2]
            assert sec.shape == ref.shape, (nf, nt, kw)
            lin, lref = 10 ** (sec / 10), 10 ** (ref / 10)
            strong = lref > 1e-6 * lref.max()
            with np.errstate(invalid="ignore"):         # an exact zero of power is -inf dB in both, and never a strong bin
                err, err_db = np.abs(lin - lref).max() / lref.max(), np.abs(sec - ref)[strong].max()
            print(f"sspec {nf} x {nt} {kw}: |lin - oracle| / peak = {err:.3e} (1e-10), strong bins {err_db:.3e} dB (1e-8)")
            assert err <= 1e-10 and err_db <= 1e-8, (nf, nt, kw, err, err_db)


# ---- the ACF --------------------------------------------------------------------------------------------------------------------
def check_acf_stack_of_one(sp, nf, nt):
    x = to_dev(sp, dyn(nf, nt))
    for subtract_mean, normalise in ACF_FLAGS:
        one = bits(sp.acf_device(x, subtract_mean=subtract_mean, normalise=normalise))
        got = bits(sp.acf_stack_device(x[None], subtract_mean=subtract_mean, normalise=normalise))
        assert got.shape == (1,) + one.shape and np.array_equal(got[0], one), (nf, nt, subtract_mean, normalise)


def check_acf_workspace(sp, nf, nt):
    import torch
    lib, ptr = sp._lib.load(), sp.device.ptr
    x = to_dev(sp, dyn(nf, nt))
    need = _need(sp, "scint_acf_workspace_bytes", nf, nt)
    ws = sp.device.empty((need,), torch.uint8)
    for subtract_mean, normalise in ACF_FLAGS:
        out = sp.device.empty((2 * nf, 2 * nt), torch.float64)
        args = (ptr(x), nf, nt, int(subtract_mean), int(normalise), ptr(out), ptr(ws))
        assert lib.scint_acf(*args, need - 1, None) == SCINT_E_WORKSPACE, (nf, nt, subtract_mean, normalise)
        assert lib.scint_acf(*args, need, None) == 0, (nf, nt, subtract_mean, normalise, sp._lib.last_error())
        assert np.array_equal(bits(out), bits(sp.acf_device(x, subtract_mean=subtract_mean, normalise=normalise)))


def check_acf_oracle(sp, nf, nt):
    """A 1 x 1 problem less its mean is all zero (and 0 / 0 when normalised): zero for zero, NaN for NaN."""
    from oracle import sspec_oracle as so
    x = dyn(nf, nt)
    for subtract_mean, normalise in ACF_FLAGS:
        got = sp.acf_device(to_dev(sp, x), subtract_mean=subtract_mean, normalise=normalise).cpu().numpy()
        refs = [cc.numpy_acf(x, subtract_mean, normalise)]
        if subtract_mean:
            with np.errstate(invalid="ignore", divide="ignore"):
                refs.append(so.calc_acf(np.array(x), normalise=normalise))
        for ref in refs:
            assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref)), (nf, nt, subtract_mean, normalise)
            ok = ~np.isnan(ref)
            if not ok.any():
                continue
            err, tol = np.abs(got - ref)[ok].max(), ACF_TOL * np.abs(ref[ok]).max()
            print(f"acf {nf} x {nt} subtract_mean={subtract_mean} normalise={normalise}: |acf - oracle| = {err:.3e}, allowed {tol:.3e}")
            assert err <= tol, (nf, nt, subtract_mean, normalise, err, tol)
