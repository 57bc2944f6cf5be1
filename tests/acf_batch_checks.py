"""Checks of the batched ACF -- scint_acf_batch, scintpar.acf_stack_device and what is built on it: cut_dyn, fit_scint_params_cut,
fit_scint_params_2d_cut -- shared by the GPU tests (tests/test_gpu_acf_batch.py) and the host-interpreted ones
(tests/test_acf_batch_emu_cpu.py).  `sp` is scintools_amd.scintpar.  The cases, and why these shapes: tests/acf_batch_cases.py.

The yardstick of the stack is the single call: problem k of the stack must hold the BITS of acf_device(stack[k]).  The single call's
own yardstick is NumPy's statement of the reference, to the 1e-12 (of the ACF's maximum, 1 when normalised) that
tests/test_gpu_scintpar.py allows it.

The single calls are the B = 1 of the stacked routes (csrc/fft.hip: acf_stack, sspec_generic), which decode no problem there.  So
the bit checks below no longer hold two implementations together: they guard the problem decode of the one route -- the row a
problem's values and means are read from, the pairs of real rows formed inside a problem, its partials, its slice of the output."""
import ctypes

import numpy as np

import acf_batch_cases as cc

ACF_TOL = 1e-12                 # tests/test_gpu_scintpar.py: |acf - reference| of the single call
FLAGS = [(False, False), (False, True), (True, False), (True, True)]      # (subtract_mean, normalise)
SCINT_E_ARG, SCINT_E_WORKSPACE = 1, 3


def to_dev(sp, a):
    import torch
    return sp.device.to_device(a, torch.float64)


def bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint64)


def problem_bytes(sp, name):
    _, nf, nt = cc.SHAPES[name]
    one = ctypes.c_size_t()
    sp._lib.call("scint_acf_batch_workspace_bytes", 1, nf, nt, one)
    return one.value


def group_bytes(sp, name):
    """The byte cap under which the case is taken in groups of cc.GROUPS[name] problems (None: in one group)."""
    if name not in cc.GROUPS:
        return None
    return cc.GROUPS[name] * problem_bytes(sp, name) + problem_bytes(sp, name) // 2


def check_bits_of_the_single_call(sp, name):
    """Problem k of the stack has the bits of acf_device(stack[k]) for every k and all four subtract_mean / normalise: the problem
    decode of the one route (acf_device is its B = 1, which decodes nothing)."""
    x = to_dev(sp, cc.stack(name))
    gb = group_bytes(sp, name)
    if gb is not None:
        assert [n for _, n in sp._stack_groups(x.shape[0], problem_bytes(sp, name), gb)] == [5, 5, 2]
    for subtract_mean, normalise in FLAGS:
        got = bits(sp.acf_stack_device(x, subtract_mean=subtract_mean, normalise=normalise, group_bytes=gb))
        for k in range(x.shape[0]):
            one = bits(sp.acf_device(x[k], subtract_mean=subtract_mean, normalise=normalise))
            assert np.array_equal(got[k], one), (name, k, subtract_mean, normalise, int((got[k] != one).sum()))


def check_against_numpy(sp, name):
    """Every problem against NumPy's statement of the reference, to the single call's tolerance: ACF_TOL of the ACF's maximum.
    Two problems of `leak` are ill-conditioned when the mean is subtracted, alone as in the stack (the bit check ties them to
    the single call).  The constant one is rounding noise over rounding noise: check_leak.  The one with mean m = 10^6 and
    unit scatter: two correct means of its N values differ by up to N eps |m|, and a shift d of the mean moves an ACF sample by up
    to 2 d sum|x - m| -- that much, which the input's conditioning sets and no ACF code can undo, is added to its bound."""
    x = cc.stack(name)
    for subtract_mean, normalise in FLAGS:
        got = sp.acf_stack_device(to_dev(sp, x), subtract_mean=subtract_mean, normalise=normalise,
                                  group_bytes=group_bytes(sp, name)).cpu().numpy()
        assert got.shape == (x.shape[0], 2 * x.shape[1], 2 * x.shape[2])
        for k in range(x.shape[0]):
            if name == "leak" and k == 2 and subtract_mean:
                continue            # a constant problem less its mean: rounding noise over rounding noise (checked below)
            ref = cc.numpy_acf(x[k], subtract_mean, normalise)
            tol = ACF_TOL * np.abs(ref).max()
            if name == "leak" and k == 4 and subtract_mean:
                m = np.mean(x[k])
                shift = 2 * (x[k].size * np.finfo(float).eps * abs(m)) * np.abs(x[k] - m).sum()
                tol += shift / (cc.numpy_acf(x[k], True, False).max() if normalise else 1.0)
            err = np.abs(got[k] - ref).max()
            print(f"{name}[{k}] subtract_mean={subtract_mean} normalise={normalise}: |acf - numpy| = {err:.3e}, allowed {tol:.3e}")
            assert err <= tol, (name, k, subtract_mean, normalise, err, tol)


def check_leak(sp):
    """The constant problem with subtract_mean is the degenerate problem of the single call (all zero, then 0 / 0: the bit check
    covers it, NaN for NaN); its neighbours, and the problem with the large mean, are untouched by it."""
    x = to_dev(sp, cc.stack("leak"))
    raw = sp.acf_stack_device(x, subtract_mean=True, normalise=False).cpu().numpy()
    assert np.all(raw[2] == 0.0)
    out = sp.acf_stack_device(x, subtract_mean=True, normalise=True).cpu().numpy()
    assert np.all(np.isnan(out[2]))
    for k in (0, 1, 3, 4, 5):
        assert np.isfinite(out[k]).all() and out[k].max() == 1.0, k


def check_deterministic(sp, name):
    x = to_dev(sp, cc.stack(name))
    a = bits(sp.acf_stack_device(x, subtract_mean=True, group_bytes=group_bytes(sp, name)))
    b = bits(sp.acf_stack_device(x, subtract_mean=True, group_bytes=group_bytes(sp, name)))
    assert np.array_equal(a, b)


def check_out(sp):
    import torch
    x = to_dev(sp, cc.stack("pow2"))
    out = sp.device.empty((5, 32, 32), torch.float64)
    out.fill_(-7.0)
    ret = sp.acf_stack_device(x, out=out)
    assert ret is out and np.array_equal(bits(out), bits(sp.acf_stack_device(x)))
    for bad in (sp.device.empty((5, 32, 31), torch.float64), sp.device.empty((5, 32, 64), torch.float64)[:, :, ::2]):
        try:
            sp.acf_stack_device(x, out=bad)
        except ValueError as err:
            assert "out must be" in str(err)
        else:
            raise AssertionError("a wrong out= was accepted")


def check_arguments(sp, pytest):
    import torch
    x = to_dev(sp, cc.stack("pow2"))
    with pytest.raises(ValueError, match="contiguous"):
        sp.acf_stack_device(x[:, :, ::2])
    with pytest.raises(ValueError, match="float64"):
        sp.acf_stack_device(x.to(torch.float32))
    with pytest.raises(ValueError, match="empty"):
        sp.acf_stack_device(x[:0])
    with pytest.raises(ValueError, match=r"\[B, nf, nt\]"):
        sp.acf_stack_device(x[0])


def check_c_status(sp):
    """The entry point itself: SCINT_E_WORKSPACE for a workspace one byte short, SCINT_E_ARG for nf = 0 (and for B beyond a grid)."""
    import torch
    lib = sp._lib.load()
    B, nf, nt = cc.SHAPES["pow2"]
    x = to_dev(sp, cc.stack("pow2"))
    out = sp.device.empty((B, 2 * nf, 2 * nt), torch.float64)
    need = ctypes.c_size_t()
    assert lib.scint_acf_batch_workspace_bytes(B, nf, nt, ctypes.byref(need)) == 0
    # the complex intermediate: 16 * 2 nf * 2 nt bytes per problem, at least the spectrum and one working array
    assert need.value >= 2 * 16 * 4 * nf * nt * B
    ws = sp.device.empty((need.value,), torch.uint8)
    ptr = sp.device.ptr
    assert lib.scint_acf_batch(ptr(x), B, nf, nt, 0, 1, ptr(out), ptr(ws), need.value - 1, None) == SCINT_E_WORKSPACE
    assert lib.scint_acf_batch(ptr(x), B, 0, nt, 0, 1, ptr(out), ptr(ws), need.value, None) == SCINT_E_ARG
    assert lib.scint_acf_batch(ptr(x), 65536, nf, nt, 0, 1, ptr(out), ptr(ws), need.value, None) == SCINT_E_ARG
    assert lib.scint_acf_batch_workspace_bytes(B, 0, nt, ctypes.byref(need)) == SCINT_E_ARG
    assert lib.scint_acf_batch(ptr(x), B, nf, nt, 0, 1, ptr(out), ptr(ws), ws.numel(), None) == 0
    assert np.array_equal(bits(out), bits(sp.acf_stack_device(x)))


# ---- the secondary spectra of a stack ---------------------------------------------------------------------------------------------
SSPEC_FLAGS = [(False, True), (True, True), (False, False)]      # (prewhite, halve); prewhite without halve raises, as sspec_device


def check_sspec_bits_of_the_single_call(sp, name):
    """Problem k of sspec_stack_device has the bits of sspec_device(stack[k]) for every k, prewhite and halve: on the generic route
    the problem decode of the one source (SRC_SSPEC; sspec_device is its B = 1), on `big` the persistent kernels run per problem."""
    from scintools_amd import dynspec
    x = to_dev(sp, cc.stack(name))
    B, nf, nt = cc.SHAPES[name]
    for prewhite, halve in SSPEC_FLAGS:
        gb = None
        if name in cc.GROUPS:
            one = ctypes.c_size_t()
            sp._lib.call("scint_sspec_batch_workspace_bytes", 1, nf, nt, 1 if halve else 0, one)
            gb = cc.GROUPS[name] * one.value + one.value // 2
            assert [n for _, n in sp._stack_groups(B, one.value, gb)] == [5, 5, 2]
        got = bits(dynspec.sspec_stack_device(x, prewhite=prewhite, halve=halve, group_bytes=gb))
        again = bits(dynspec.sspec_stack_device(x, prewhite=prewhite, halve=halve, group_bytes=gb))
        assert np.array_equal(got, again), (name, prewhite, halve)
        for k in range(B):
            one = bits(dynspec.sspec_device(x[k], prewhite=prewhite, halve=halve))
            assert np.array_equal(got[k], one), (name, k, prewhite, halve, int((got[k] != one).sum()))
    try:
        dynspec.sspec_stack_device(x, prewhite=True, halve=False)
    except RuntimeError as err:
        assert "prewhite" in str(err)
    else:
        raise AssertionError("prewhite without halve was accepted")


def check_sspec_arguments(sp, pytest):
    import torch
    from scintools_amd import dynspec
    x = to_dev(sp, cc.stack("pow2"))
    out = sp.device.empty((5, 16, 32), torch.float64)
    assert dynspec.sspec_stack_device(x, out=out) is out
    assert np.array_equal(bits(out), bits(dynspec.sspec_stack_device(x)))
    with pytest.raises(ValueError, match="contiguous"):
        dynspec.sspec_stack_device(x[:, :, ::2])
    with pytest.raises(ValueError, match="float64"):
        dynspec.sspec_stack_device(x.to(torch.float32))
    with pytest.raises(ValueError, match="empty"):
        dynspec.sspec_stack_device(x[:0])
    with pytest.raises(ValueError, match="out must be"):
        dynspec.sspec_stack_device(x, out=sp.device.empty((5, 32, 32), torch.float64))
    lib = sp._lib.load()
    need = ctypes.c_size_t()
    assert lib.scint_sspec_batch_workspace_bytes(5, 16, 16, 1, ctypes.byref(need)) == 0
    ws = sp.device.empty((need.value,), torch.uint8)
    ptr = sp.device.ptr
    args = (None, None, 0, 1, None, None, ptr(out), ptr(ws))
    assert lib.scint_sspec_batch(ptr(x), 5, 16, 16, *args, need.value - 1, None) == SCINT_E_WORKSPACE
    assert lib.scint_sspec_batch(ptr(x), 5, 0, 16, *args, need.value, None) == SCINT_E_ARG
    assert lib.scint_sspec_batch(ptr(x), 65536, 16, 16, *args, need.value, None) == SCINT_E_ARG


# ---- cut_dyn and the cut fits: the per-segment loop they ran before, written out -----------------------------------------------
TCUTS = FCUTS = 3


def _dynspec(obs):
    from scintools_amd.dynspec import Dynspec
    return Dynspec(dyn=obs, verbose=False)


def _segment_loop(sp, o):
    """(segs, sspecs, acfs) as device stacks: one acf_device / sspec_device call per segment."""
    import torch
    from scintools_amd.dynspec import sspec_device
    fnum, tnum = o.dyn.shape[0] // (FCUTS + 1), o.dyn.shape[1] // (TCUTS + 1)
    nseg = (FCUTS + 1) * (TCUTS + 1)
    segs = sp.segment_cut_device(to_dev(sp, o.dyn), fnum, tnum, FCUTS + 1, TCUTS + 1)
    nrfft = int(2 ** (np.ceil(np.log2(fnum)) + 1) / 2)
    ncfft = int(2 ** (np.ceil(np.log2(tnum)) + 1))
    sspecs = sp.device.empty((nseg, nrfft, ncfft), torch.float64)
    acfs = sp.device.empty((nseg, 2 * fnum, 2 * tnum), torch.float64)
    for k in range(nseg):
        sspec_device(segs[k], out=sspecs[k])
        sp.acf_device(segs[k], subtract_mean=False, out=acfs[k])
    return segs, sspecs, acfs, fnum, tnum


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def check_cut_dyn(sp):
    """cutdyn / cutsspec / cutacf hold the bits of the per-segment loop, stay on the device until they are read, and read twice
    give the same array."""
    from scintools_amd.dynspec import Dynspec
    o = cc.observation()
    segs, sspecs, acfs, fnum, tnum = _segment_loop(sp, o)
    d = _dynspec(o)
    d.cut_dyn(tcuts=TCUTS, fcuts=FCUTS)
    for attr in ("cutdyn", "cutsspec", "cutacf"):
        assert getattr(Dynspec, attr).present(d) and getattr(Dynspec, attr).on_device(d), attr     # nothing downloaded yet
    acf = d.cutacf
    assert not Dynspec.cutacf.on_device(d) and Dynspec.cutdyn.on_device(d) and Dynspec.cutsspec.on_device(d)
    assert d.cutacf is acf and isinstance(acf, np.ndarray)
    shape = (FCUTS + 1, TCUTS + 1)
    assert acf.shape == shape + (2 * fnum, 2 * tnum) and d.cutdyn.shape == shape + (fnum, tnum)
    assert np.array_equal(acf.view(np.uint64), bits(acfs).reshape(acf.shape))
    assert np.array_equal(d.cutdyn.view(np.uint64), bits(segs).reshape(d.cutdyn.shape))
    assert np.array_equal(d.cutsspec.view(np.uint64), bits(sspecs).reshape(d.cutsspec.shape))
    assert np.array_equal(d.cutdyn[1, 2], o.dyn[fnum:2 * fnum, 2 * tnum:3 * tnum])


def check_cut_fits(sp):
    """fit_scint_params_cut and fit_scint_params_2d_cut: every cut_* array has the bits of the fits of the looped ACF stack."""
    o = cc.observation()
    _, _, acfs, fnum, tnum = _segment_loop(sp, o)
    shape = (FCUTS + 1, TCUTS + 1)
    d = _dynspec(o)
    d.fit_scint_params_cut(tcuts=TCUTS, fcuts=FCUTS)
    one = sp.acf1d_fit_device(acfs, o.dt, o.df, fnum * o.df, tnum * o.dt)
    for attr, k in (("cut_tau", "tau"), ("cut_dnu", "dnu"), ("cut_tauerr", "tauerr"), ("cut_dnuerr", "dnuerr"), ("cut_amp", "amp"),
                    ("cut_fit_status", "status")):
        assert _same(getattr(d, attr), one[k].reshape(shape)), attr
    assert (d.cut_fit_status == sp.FIT_CONVERGED).any()
    d2 = _dynspec(o)
    d2.fit_scint_params_2d_cut(tcuts=TCUTS, fcuts=FCUTS)
    two = sp.acf2d_approx_fit_device(acfs, o.dt, o.df, fnum * o.df, tnum * o.dt, nsub=tnum, nchan=fnum)
    for k in ("tau", "dnu", "amp", "phasegrad"):
        assert _same(getattr(d2, "cut_" + k), two[k].reshape(shape)), k
        assert _same(getattr(d2, "cut_" + k + "err"), two[k + "err"].reshape(shape)), k
    assert _same(d2.cut_fit_status, two["status"].reshape(shape))
