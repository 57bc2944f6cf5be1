"""The checks of the biharmonic fill, shared by the GPU tests (tests/test_gpu_inpaint.py) and the host-interpreter run
(tests/test_inpaint_emu_cpu.py).  Every check prints what it measured before it asserts.

Bounds (none of them tuned on the device's output):
* the true relative residual rho_dev = |b - A u_dev| / |b|, recomputed here with the oracle's sparse matrix, is <= 10 tol: the
  device stops at a true residual <= tol by its own arithmetic, and the two evaluations of the residual differ by rounding, of
  relative size eps * kappa ~ 4e-14 for these cases -- a factor 10 covers it with room;
* |u_dev - u_ref| <= kappa (rho_dev + rho_ref) |u_ref|: from A (u_dev - u_ref) = r_ref - r_dev, |u_dev - u_ref| <=
  |A^-1| (|r_dev| + |r_ref|) and |b| <= |A| |u_ref|; kappa is the recorded condition number (tests/inpaint_cases.py);
* known pixels keep their bits, and two runs give the same bits."""
import functools

import numpy as np

import inpaint_cases as ic
import inpaint_oracle as io

TOL = 1e-12
RESIDUAL_FACTOR = 10.0


@functools.lru_cache(maxsize=None)
def reference(name):
    """(filled image, A, b, rho_ref) of the oracle for case ``name``: computed once, shared, read-only."""
    dyn, bad = ic.case(name)
    out, a, b = io.fill(dyn, bad, return_system=True)
    out.setflags(write=False)
    return out, a, b, io.residual(a, b, out[bad])


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_case(C, name):
    dyn, bad = ic.case(name)
    ref, a, b, rho_ref = reference(name)
    info = {}
    got = C.biharmonic_fill_device(dyn, info=info)
    rho_dev = io.residual(a, b, got[bad])
    err = np.linalg.norm(got[bad] - ref[bad]) / np.linalg.norm(ref[bad])
    bound = ic.KAPPA[name] * (rho_dev + rho_ref)
    print(f"inpaint {name}: nmask {info['nmask']} iters {info['iters']} residual(device) {info['residual']:.3g} "
          f"residual(host) {rho_dev:.3g} rho_ref {rho_ref:.3g} error {err:.3g} bound {bound:.3g}")
    assert np.isfinite(got).all() and info["nmask"] == int(bad.sum())
    assert same_bits(got[~bad], dyn[~bad]), "a known pixel changed its bits"
    assert info["residual"] <= TOL, "the device's own true residual exceeds tol"
    assert rho_dev <= RESIDUAL_FACTOR * TOL
    assert err <= bound
    assert info["iters"] >= 1 and (name != "d" or info["iters"] == 1)
    again = C.biharmonic_fill_device(dyn)
    assert same_bits(got, again), "two runs differ"
    # an explicit mask, with garbage instead of NaN under it: the same bits (the masked values are never read)
    junk = np.where(bad, 1e300, dyn)
    assert same_bits(C.biharmonic_fill_device(junk, mask=bad), got)


def check_nothing_masked(C):
    dyn = ic.image(6, 7, seed=1)
    info = {}
    out = C.biharmonic_fill_device(dyn, info=info)
    assert out is not dyn and same_bits(out, dyn) and info == dict(iters=0, residual=0.0, nmask=0)
    small = np.ones((3, 4))                              # below 5 x 5, but nothing to fill: a copy
    assert same_bits(C.biharmonic_fill_device(small), small)


def check_method(D, C):
    """Dynspec.inpaint() after zap() on case (a)'s image: no NaN is left, in place, and it is biharmonic_fill_device's result."""
    import clean_checks as ck
    x, spikes = ic.spiky_observation()
    x[5, :] = 0.0                                       # a dead channel: inpaint(zeros=True) flags it
    d = D.Dynspec(dyn=ck._obs(x), verbose=False)
    alias = d.dyn
    d.zap()
    flagged = np.isnan(d.dyn)
    print(f"inpaint after zap: {int(flagged.sum())} pixels flagged by zap, {int((d.dyn == 0).sum())} zeros")
    assert all(flagged[i, j] for i, j in spikes)
    want = np.where(flagged | (x == 0), np.nan, x)
    d.inpaint()
    assert d.dyn is alias and np.isfinite(d.dyn).all() and not (d.dyn == 0).any()
    assert same_bits(d.dyn, C.biharmonic_fill_device(want))
    keep = np.isfinite(want)
    assert same_bits(d.dyn[keep], x[keep])
    # zeros=False keeps the zeros as data
    d2 = D.Dynspec(dyn=ck._obs(x), verbose=False)
    d2.zap()
    d2.inpaint(zeros=False)
    assert np.isfinite(d2.dyn).all() and (d2.dyn[5] == 0).all()


def check_errors(C, pytest):
    from scintools_amd import _lib
    with pytest.raises(ValueError, match="every pixel is masked"):
        C.biharmonic_fill_device(np.full((6, 6), np.nan))
    for shape in ((4, 9), (9, 4)):
        x = ic.image(*shape, seed=2)
        x[1, 1] = np.nan
        with pytest.raises(ValueError, match="5 x 5"):
            C.biharmonic_fill_device(x)
    with pytest.raises(ValueError, match="mask has shape"):
        C.biharmonic_fill_device(np.ones((6, 6)), mask=np.zeros((6, 5), bool))
    x = ic.image(6, 6, seed=2)
    x[2, 2] = np.inf
    mask = np.zeros((6, 6), bool)
    mask[4, 4] = True
    with pytest.raises(ValueError, match="not finite"):
        C.biharmonic_fill_device(x, mask=mask)
    dyn, bad = ic.case("b")
    with pytest.raises(_lib.ScintHipError, match=r"stopped after 2 steps at a relative residual of [0-9.e+-]+ \(wanted 1e-12\)") as exc:
        C.biharmonic_fill_device(dyn, max_iter=2)
    assert exc.value.status == _lib.SCINT_E_NOCONV
    # the C ABI's own refusals: a count that is not the mask's, a size below 5
    import torch
    from scintools_amd import device
    t = device.to_device(np.where(bad, 0.0, dyn), torch.float64)
    m = device.to_device(bad, torch.uint8)
    table = device.to_device(C.stencil_table(), torch.float64)
    nmask = int(bad.sum())
    ws = device.workspace_for("scint_inpaint_biharmonic", 96, 80, nmask + 3)
    for args in ((96, 80, m, nmask + 3), (96, 80, m, nmask - 3), (4, 1920, m, nmask)):
        with pytest.raises(_lib.ScintHipError) as exc:
            _lib.call("scint_inpaint_biharmonic", t, *args, table, 1e-12, 100, None, None, ws, ws.numel(), device.stream_ptr())
        assert exc.value.status == _lib.SCINT_E_ARG
