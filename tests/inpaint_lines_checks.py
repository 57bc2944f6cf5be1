"""The checks of the biharmonic fill with the line-block preconditioner (``precond='lines'``), shared by the GPU tests
(tests/test_gpu_inpaint_lines.py) and the host-interpreter run (tests/test_inpaint_lines_emu_cpu.py).  Every check prints what it
measured before it asserts.

Bounds (none of them tuned on the device's output):
* the true relative residual rho_dev = |b - A u_dev| / |b|, recomputed here with the oracle's sparse matrix, is <= 1e-11 at
  tol = 1e-12: the plain route's criterion (tests/inpaint_checks.py: 10 tol);
* |u_dev - u_ref| <= kappa (rho_dev + rho_ref) |u_ref|, kappa the recorded condition number (tests/inpaint_lines_cases.py), as
  in tests/inpaint_checks.py;
* known pixels keep their bits, and two runs give the same bits;
* steps: at most 1.25 x the steps of the NumPy restatement of the same algorithm (tests/inpaint_lines_oracle.py, recorded in
  tests/golden/inpaint_lines_tolerances.json by make_inpaint_lines_tolerances.py) + 2 -- the margin covers other summation orders."""
import functools
import json
import os

import numpy as np

import inpaint_cases as ic
import inpaint_lines_cases as lc
import inpaint_oracle as io
from inpaint_checks import RESIDUAL_FACTOR, TOL, same_bits

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def recorded():
    with open(os.path.join(HERE, "golden", "inpaint_lines_tolerances.json")) as fh:
        return json.load(fh)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(filled image, A, b, rho_ref) of the oracle for case ``name``: computed once, shared, read-only."""
    dyn, bad = lc.case(name)
    out, a, b = io.fill(dyn, bad, return_system=True)
    out.setflags(write=False)
    return out, a, b, io.residual(a, b, out[bad])


def check_case(C, name):
    dyn, bad = lc.case(name)
    ref, a, b, rho_ref = reference(name)
    info = {}
    got = C.biharmonic_fill_device(dyn, info=info, precond='lines')
    rho_dev = io.residual(a, b, got[bad])
    err = np.linalg.norm(got[bad] - ref[bad]) / np.linalg.norm(ref[bad])
    bound = lc.KAPPA[name] * (rho_dev + rho_ref)
    print(f"inpaint lines {name}: nmask {info['nmask']} route {info['route']} iters {info['iters']} lines "
          f"{info['line_channels']} + {info['line_subints']} residual(device) {info['residual']:.3g} residual(host) {rho_dev:.3g} "
          f"rho_ref {rho_ref:.3g} error {err:.3g} bound {bound:.3g}")
    assert np.isfinite(got).all() and info["nmask"] == int(bad.sum())
    assert info["line_channels"] == int(bad.all(axis=1).sum()) and info["line_subints"] == int(bad.all(axis=0).sum())
    assert same_bits(got[~bad], dyn[~bad]), "a known pixel changed its bits"
    assert info["residual"] <= TOL, "the device's own true residual exceeds tol"
    assert rho_dev <= RESIDUAL_FACTOR * TOL
    assert err <= bound
    if name in lc.DIRECT:
        assert info["route"] == "direct" and info["iters"] == 0
    else:
        assert info["route"] == "pcg" and info["iters"] >= 1
    if name in lc.COUNTED:
        limit = 1.25 * recorded()[name]["pcg_steps"] + 2
        print(f"inpaint lines {name}: {info['iters']} steps, the restatement took {recorded()[name]['pcg_steps']} (limit {limit:g}); "
              f"plain conjugate gradients {recorded()[name]['cg_steps']}")
        assert info["iters"] <= limit
    again = C.biharmonic_fill_device(dyn, precond='lines')
    assert same_bits(got, again), "two runs differ"
    # an explicit mask, with garbage instead of NaN under it: the same bits (the masked values are never read)
    junk = np.where(bad, 1e300, dyn)
    assert same_bits(C.biharmonic_fill_device(junk, mask=bad, precond='lines'), got)


def check_default_route_unchanged(C, name):
    """precond=None on a case of tests/inpaint_cases.py: the bits of the existing entry point, called directly."""
    import ctypes
    import torch
    from scintools_amd import _lib, device
    dyn, bad = ic.case(name)
    info = {}
    got = C.biharmonic_fill_device(dyn, info=info, precond=None)
    assert info["route"] == "cg" and same_bits(got, C.biharmonic_fill_device(dyn))
    nf, nt = dyn.shape
    nmask = int(bad.sum())
    t = device.to_device(np.array(dyn), torch.float64)
    m = device.to_device(bad, torch.uint8)
    table = device.to_device(C.stencil_table(), torch.float64)
    ws = device.workspace_for("scint_inpaint_biharmonic", nf, nt, nmask)
    residual, iters = ctypes.c_double(), ctypes.c_int32()
    _lib.call("scint_inpaint_biharmonic", t, nf, nt, m, nmask, table, TOL, C.INPAINT_MAX_ITER, residual, iters, ws, ws.numel(),
              device.stream_ptr())
    print(f"inpaint {name}, precond=None: {info['iters']} steps, the entry point itself {iters.value}")
    assert same_bits(got, t.cpu().numpy()) and info["iters"] == iters.value


def check_method(D, C):
    """Dynspec.inpaint(precond='lines') after zap() on a field with a band of dead channels."""
    import clean_checks as ck
    x, spikes = lc.band_observation()
    d = D.Dynspec(dyn=ck._obs(x), verbose=False)
    alias = d.dyn
    d.zap()
    flagged = np.isnan(d.dyn)
    print(f"inpaint lines after zap: {int(flagged.sum())} pixels flagged by zap, {int((d.dyn == 0).sum())} zeros")
    assert all(flagged[i, j] for i, j in spikes)
    want = np.where(flagged | (x == 0), np.nan, x)
    d.inpaint(precond='lines')
    assert d.dyn is alias and np.isfinite(d.dyn).all() and not (d.dyn == 0).any()
    info = {}
    assert same_bits(d.dyn, C.biharmonic_fill_device(want, info=info, precond='lines'))
    assert info["line_channels"] == 12 and info["route"] == "pcg"
    keep = np.isfinite(want)
    assert same_bits(d.dyn[keep], x[keep])
    ref = io.fill(want, ~keep)
    err = np.linalg.norm(d.dyn[~keep] - ref[~keep]) / np.linalg.norm(ref[~keep])
    print(f"inpaint lines after zap: {info['iters']} steps, error against the direct solve {err:.3g}")
    assert err <= 1e-6                                  # (kappa of a 12-channel band ~ 1e4, residuals ~ 1e-12: loose on purpose)


def check_errors(C, D, pytest):
    from scintools_amd import _lib
    dyn, bad = lc.case("f")
    for fn in (lambda: C.biharmonic_fill_device(dyn, precond='jacobi'), lambda: C.biharmonic_fill_device(dyn, precond=True)):
        with pytest.raises(ValueError, match="precond"):
            fn()
    import clean_checks as ck
    with pytest.raises(ValueError, match="precond"):
        D.Dynspec(dyn=ck._obs(lc.band_observation()[0]), verbose=False).inpaint(precond='bands')
    with pytest.raises(ValueError, match="every pixel is masked"):
        C.biharmonic_fill_device(np.full((6, 6), np.nan), precond='lines')
    # a transformed axis beyond the limit: time (whole channels), frequency (whole sub-integrations); no limit without lines
    wide = np.ones((5, 4100))
    wide[2, :] = np.nan
    with pytest.raises(ValueError, match=r"time axis holds 4100 points.*5 \.\. 4096 points, or 8192"):
        C.biharmonic_fill_device(wide, precond='lines')
    with pytest.raises(ValueError, match=r"frequency axis holds 4100 points"):
        C.biharmonic_fill_device(wide.T, precond='lines')
    # out of steps: ScintHipError with the status, the array untouched
    dyn, bad = lc.case("c")
    before = np.array(dyn)
    with pytest.raises(_lib.ScintHipError, match=r"stopped after 2 steps at a relative residual of [0-9.e+-]+ \(wanted 1e-12\)") as exc:
        C.biharmonic_fill_device(dyn, max_iter=2, precond='lines')
    assert exc.value.status == _lib.SCINT_E_NOCONV and same_bits(before, np.array(dyn))
    # the C ABI's own refusals: line counts that are not the mask's
    import torch
    from scintools_amd import device
    nf, nt = bad.shape
    t = device.to_device(np.where(bad, 0.0, dyn), torch.float64)
    m = device.to_device(bad, torch.uint8)
    table = device.to_device(C.stencil_table(), torch.float64)
    nmask, nchan, nsub = int(bad.sum()), int(bad.all(axis=1).sum()), int(bad.all(axis=0).sum())
    ws = device.workspace_for("scint_inpaint_biharmonic_lines", nf, nt, nmask + 3, nchan + 1, nsub + 1)
    for args in ((nmask, nchan + 1, nsub), (nmask, nchan, nsub - 1), (nmask + 3, nchan, nsub)):
        with pytest.raises(_lib.ScintHipError) as exc:
            _lib.call("scint_inpaint_biharmonic_lines", t, nf, nt, m, *args, table, 1e-12, 100, None, None, ws, ws.numel(),
                      device.stream_ptr())
        assert exc.value.status == _lib.SCINT_E_ARG
    with pytest.raises(_lib.ScintHipError) as exc:
        _lib.call("scint_inpaint_biharmonic_lines_workspace_bytes", 5, 4100, 4100, 1, 0, __import__("ctypes").c_size_t())
    assert exc.value.status == _lib.SCINT_E_ARG
