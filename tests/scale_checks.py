"""The checks of Dynspec.scale_dyn(scale='velocity' / 'trapezoid'), shared by the GPU tests (tests/test_gpu_scale.py) and a
host-interpreter run of the same file (pytest --emu).  The truth of the row spline is scipy's interp1d(kind='cubic') per row
(tests/scale_oracle.spline_rows, the reference's own call); of the trapezoid, tests/scale_oracle.trapezoid, bit for bit.
tests/test_scale_cpu.py pins both to the unmodified reference's outputs (tests/golden/scale.npz).

Tolerance of the row spline (TOL): tests/golden/make_golden_scale.py measures the worst difference, relative to the array maximum,
between the float64 moment algorithm the kernel runs and the reference's vdyn over all velocity cases (6.1e-16, in
tests/golden/scale_tolerances.json); the bound is 10 x that -- the factor covers another summation order in the blocked sweeps --
and not below 1e-12, the bound of the lambda resample.  So TOL = 1e-12.

Shapes and the constants they straddle (csrc/scale.hpp; a workgroup takes min(64, 7680 // (span | 1)) rows, span = nt with one block):
  1 x 4      the fewest knots a cubic takes            3 x 5      one interior interval more
  65 x 100   64 rows per workgroup + 1                 59 x 130   58 rows per workgroup (7680 // 131) + 1
  5 x 700    698 interior knots >= 4 * 128: blocked, 5 full blocks + 58 knots
  2 x 1100   an effective velocity changing 50 : 1
  2 x 7700   one block of 7700 knots > 7679: the sweep through the workspace
"""
import json
import os

import numpy as np

import scale_cases as sc
import scale_oracle as so

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "scale_tolerances.json")) as _fh:
    TOL = max(10 * json.load(_fh)["moment_algorithm_vs_reference"], 1e-12)

ROW_SHAPES = [(1, 4), (3, 5), (65, 100), (59, 130), (5, 700)]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True) and \
        np.array_equal(np.signbit(a), np.signbit(b))


def close_longdouble(a, b):
    """Host quantities the reference carries as np.float128 (MJDs, true anomaly, velocities): the same dtype and within 16 units
    of the last place of THAT format, relative to the largest value.  Not bit-equality: the long-double arctan2 / sin / cos are
    x87 instructions good to one unit of the last place whose last bit differs between CPU makes, so the goldens, made on one
    host, differ from a run on another by a few of these units (seen: `circular` on the GPU host); 16 covers the chain
    arctan2 -> +2 pi -> sin / cos -> two products -> two sums.  In float64 terms this is 2e-18 relative: no test is loosened."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.longdouble:
        return np.array_equal(a, b)
    return bool(np.abs(a - b).max() <= 16 * np.finfo(np.longdouble).eps * np.abs(b).max())


def rel(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def _arcfit():
    from scintools_amd import arcfit
    return arcfit


def _dev(a):
    import torch
    from scintools_amd.device import to_device
    return to_device(np.ascontiguousarray(a, dtype=float), torch.float64)


def rows_input(nf, nt, seed=0, ratio=None):
    rng = np.random.default_rng(1000 * nf + nt + seed)
    dyn = rng.random((nf, nt)) + 1
    veff = sc.contrast_veff(nt, ratio) if ratio else 30.0 + 10.0 * np.sin(np.arange(nt) / 9.0) + rng.random(nt)
    x, xnew = so.velocity_grid(veff)
    return dyn, x, xnew


_truth = {}


def rows_truth(key, dyn, x, xnew):
    """scipy's answer, computed once per input and shared read-only."""
    if key not in _truth:
        t = so.spline_rows(dyn, x, xnew)
        t.setflags(write=False)
        _truth[key] = t
    return _truth[key]


def check_rows(nf, nt, route):
    A = _arcfit()
    dyn, x, xnew = rows_input(nf, nt)
    assert A.spline_rows_route(x)[0] == route, A.spline_rows_route(x)
    got = A.spline_resample_rows_device(_dev(dyn), x, xnew).cpu().numpy()
    e = rel(got, rows_truth((nf, nt), dyn, x, xnew))
    print(f"scale: rows {nf}x{nt} {route} E = {e:.3e} bound = {TOL:.1e}")
    assert got.shape == (nf, nt) and e <= TOL


def check_contrast():
    """2 x 1100 with veff changing 50 : 1.  The issue expected the warm-up rule to give up here and the sequential sweep to run; it
    does not, and cannot: the Thomas factors of a spline system are bounded (|sub*inv|, |sup| <= about 1/2 for ANY spacing, the
    matrix being diagonally dominant by a factor 2), so `warm` stays at 24..40 knots for every axis tried (uniform, random 1e4 : 1,
    alternating 50 : 1).  The host-side decision is therefore 'blocked', asserted here; the sequential sweep of the same input
    is forced beside it and both meet the bound."""
    A = _arcfit()
    dyn, x, xnew = rows_input(2, 1100, ratio=50.0)
    h = np.diff(x)
    assert h.max() / h.min() > 45
    route = A.spline_rows_route(x)
    assert route[0] == 'blocked' and route[1] == sc.BLOCK and 8 <= route[2] <= 2 * sc.BLOCK, route
    truth = rows_truth("contrast", dyn, x, xnew)
    for force in (False, True):
        got = A.spline_resample_rows_device(_dev(dyn), x, xnew, force_one_block=force).cpu().numpy()
        e = rel(got, truth)
        print(f"scale: rows 2x1100 50:1 {'one block' if force else route} E = {e:.3e} bound = {TOL:.1e}")
        assert e <= TOL


def check_workspace_route():
    import ctypes
    from scintools_amd import _lib
    A = _arcfit()
    nf, nt = 2, sc.ROWS_LDS + 20
    dyn, x, xnew = rows_input(nf, nt)
    need = ctypes.c_size_t()
    _lib.call("scint_spline_resample_rows_workspace_bytes", nf, nt, 0, 0, need)
    assert need.value == 8 * nf * nt
    _lib.call("scint_spline_resample_rows_workspace_bytes", nf, sc.ROWS_LDS - 1, 0, 0, need)
    assert need.value == 256
    got = A.spline_resample_rows_device(_dev(dyn), x, xnew, force_one_block=True).cpu().numpy()
    e = rel(got, rows_truth((nf, nt), dyn, x, xnew))
    print(f"scale: rows {nf}x{nt} through the workspace E = {e:.3e} bound = {TOL:.1e}")
    assert e <= TOL
    blocked = A.spline_resample_rows_device(_dev(dyn), x, xnew).cpu().numpy()
    assert rel(blocked, got) <= TOL


def check_blocked_vs_one_block():
    A = _arcfit()
    dyn, x, xnew = rows_input(5, 700)
    a = A.spline_resample_rows_device(_dev(dyn), x, xnew).cpu().numpy()
    b = A.spline_resample_rows_device(_dev(dyn), x, xnew, force_one_block=True).cpu().numpy()
    e = rel(a, b)
    print(f"scale: blocked vs one block 5x700 E = {e:.3e}")
    assert e <= TOL
    assert np.array_equal(a, A.spline_resample_rows_device(_dev(dyn), x, xnew).cpu().numpy())       # deterministic


def check_transpose_route(monkeypatch):
    """From 2^24 pixels on the blocked resample goes through a transpose and the column kernel (measured faster at 4096^2); with
    the threshold lowered the small input takes that route and gives the row kernel's result to the same bound."""
    A = _arcfit()
    dyn, x, xnew = rows_input(5, 700)
    assert A._ROWS_TRANSPOSE_MIN == 1 << 24
    rows = A.spline_resample_rows_device(_dev(dyn), x, xnew).cpu().numpy()
    monkeypatch.setattr(A, "_ROWS_TRANSPOSE_MIN", 0)
    got = A.spline_resample_rows_device(_dev(dyn), x, xnew).cpu().numpy()
    e = rel(got, rows_truth((5, 700), dyn, x, xnew))
    print(f"scale: rows 5x700 through the transpose E = {e:.3e}, vs the row kernel {rel(got, rows):.3e}")
    assert e <= TOL and rel(got, rows) <= TOL
    order = np.random.default_rng(3).permutation(len(xnew))
    shuffled = A.spline_resample_rows_device(_dev(dyn), x, xnew[order]).cpu().numpy()
    assert np.array_equal(shuffled, got[:, order])


def check_nout():
    """nout != nt, targets in any order, through the helper."""
    A = _arcfit()
    dyn, x, _ = rows_input(5, 700)
    rng = np.random.default_rng(5)
    xnew = rng.uniform(x[0], x[-1], 333)
    xnew[:2] = x[0], x[-1]
    got = A.spline_resample_rows_device(_dev(dyn), x, xnew).cpu().numpy()
    e = rel(got, so.spline_rows(dyn, x, xnew))
    print(f"scale: 333 unsorted targets E = {e:.3e}")
    assert got.shape == (5, 333) and e <= TOL
    # a descending axis: interp1d sorts it
    got = A.spline_resample_rows_device(_dev(dyn[:, ::-1]), x[::-1], np.sort(xnew)).cpu().numpy()
    assert rel(got, so.spline_rows(dyn, x, np.sort(xnew))) <= TOL


def check_nan():
    """One NaN pixel: its row is all NaN (scipy's sequential solve), every other row is unchanged to the tolerance."""
    A = _arcfit()
    for shape in ((5, 700), (59, 130)):
        dyn, x, xnew = rows_input(*shape)
        clean = rows_truth(shape, dyn, x, xnew)
        bad = dyn.copy()
        bad[2, shape[1] // 3] = np.nan
        got = A.spline_resample_rows_device(_dev(bad), x, xnew).cpu().numpy()
        assert np.isnan(got[2]).all() and np.isnan(so.spline_rows(bad[2:3], x, xnew)).all()
        keep = np.arange(shape[0]) != 2
        assert np.isfinite(got[keep]).all() and rel(got[keep], clean[keep]) <= TOL


def check_errors(pytest):
    A = _arcfit()
    dyn, x, xnew = rows_input(3, 40)
    veff = np.diff(x, prepend=0.0)
    veff[7] = 0.0
    with pytest.raises(ValueError, match="Expect x to not have duplicates"):
        A.velocity_resample_device(_dev(dyn), veff)
    with pytest.raises(ValueError, match="equal in length"):
        A.spline_resample_rows_device(_dev(dyn), x[:-1], xnew)
    with pytest.raises(ValueError, match="derivatives at boundaries"):
        A.spline_resample_rows_device(_dev(dyn[:, :3]), x[:3], x[:3])
    with pytest.raises(ValueError, match="outside the interpolation range"):
        A.spline_resample_rows_device(_dev(dyn), x, xnew + 1.0)


def check_velocity_helper():
    A = _arcfit()
    dyn, x, xnew = rows_input(3, 40)
    veff = np.diff(x, prepend=0.0).astype(np.longdouble)
    got = A.velocity_resample_device(_dev(dyn), veff).cpu().numpy()
    assert rel(got, so.velocity(dyn, veff)) <= TOL


# -------------------------------------------------------------------------------------------------------------- trapezoid
def check_trapezoid(name):
    A = _arcfit()
    okw, kw = sc.TRAPEZOID[name]
    o = sc.observation(**okw)
    got = A.trap_scale_device(o.dyn, o.freqs, o.times, **kw).cpu().numpy()
    ref = so.trapezoid(o.dyn, o.freqs, o.times, **kw)
    keep = so.trapezoid_keep(o.freqs, o.times)
    assert keep[-1] == o.nsub                              # the last row always keeps every sample
    if name == "wide":
        assert keep[0] == 1
    if name == "late":
        assert keep[0] == 0 and not ref[0].any()
    assert same_bits(got, ref), (name, np.abs(got - ref).max())


def check_trapezoid_long():
    """More than one workgroup along time (256 samples each), sub-integrations of unequal length."""
    A = _arcfit()
    o = sc.observation(nf=7, nt=300, uneven=True, seed=9, f0=700.0, f1=1400.0)
    for kw in (dict(), dict(window=None)):
        assert same_bits(A.trap_scale_device(o.dyn, o.freqs, o.times, **kw).cpu().numpy(),
                         so.trapezoid(o.dyn, o.freqs, o.times, **kw))


# ---------------------------------------------------------------------------------------------------------- through Dynspec
def seeded(monkeypatch, gold):
    """scint_utils' two ephemeris look-ups replaced by the arrays the reference was given."""
    from scintools_amd import scint_utils
    monkeypatch.setattr(scint_utils, "get_ssb_delay", lambda mjds, raj, decj, message=True: np.array(gold["eph_ssb"]))
    monkeypatch.setattr(scint_utils, "get_earth_velocity",
                        lambda mjds, raj, decj, radial=False: (np.array(gold["eph_vra"]), np.array(gold["eph_vdec"])))


def dynspec(**okw):
    from scintools_amd.dynspec import Dynspec
    return Dynspec(dyn=sc.observation(**okw), verbose=False)


def lin_close(sec, ref):
    lin, lref = 10 ** (sec / 10), 10 ** (ref / 10)
    return np.abs(lin - lref).max() <= 1e-10 * lref.max()


def check_velocity_case(gold, name):
    pars, kw, lam = sc.VELOCITY[name]
    d = dynspec()
    if lam:
        d.scale_dyn(scale='lambda')
    d.scale_dyn(scale='velocity', pars=dict(pars), **dict(kw))
    ulp = np.finfo(np.longdouble).eps * np.abs(gold[f"v_{name}_veff_ra"]).max()
    print(f"scale: velocity case {name} veff_ra differs by {float(np.abs(d.veff_ra - gold[f'v_{name}_veff_ra']).max() / ulp):.2f}, "
          f"veff_dec by {float(np.abs(d.veff_dec - gold[f'v_{name}_veff_dec']).max() / ulp):.2f} long-double units (bound 16)")
    assert close_longdouble(d.veff_ra, gold[f"v_{name}_veff_ra"]) and close_longdouble(d.veff_dec, gold[f"v_{name}_veff_dec"])
    e = rel(d.vdyn, gold[f"v_{name}_vdyn"])
    print(f"scale: velocity case {name} E = {e:.3e} bound = {TOL:.1e}")
    assert d.vdyn.dtype == np.float64 and e <= TOL
    if lam:
        # lamdyn itself is within 1e-12 of the reference's (the lambda resample's bound), and the row spline is linear in it
        assert rel(d.vlamdyn, gold[f"v_{name}_vlamdyn"]) <= 1e-12 + TOL
    else:
        assert not type(d).vlamdyn.present(d)


def check_velocity_spectra(gold):
    d = dynspec()
    d.scale_dyn(scale='lambda')
    d.scale_dyn(scale='velocity', pars=dict(sc.BINARY))
    cls = type(d)
    assert cls.vdyn.present(d) and d.__dict__[cls.vdyn.slot][1] is not None          # parked: still on the device
    d.calc_sspec(velocity=True)
    assert d.__dict__[cls.vdyn.slot][1] is not None and d.__dict__[cls.vsspec.slot][0] is None   # no download yet
    assert lin_close(d.vsspec, gold["v_ecc_vsspec"])
    assert np.array_equal(d.fdop, gold["v_ecc_fdop"]) and np.array_equal(d.tdel, gold["v_ecc_tdel"])
    d.calc_sspec(velocity=True, lamsteps=True)
    assert lin_close(d.vlamsspec, gold["v_ecc_vlamsspec"]) and np.allclose(d.beta, gold["v_ecc_beta"], rtol=1e-14, atol=0)
    first = d.vdyn
    assert d.vdyn is first and d.__dict__[cls.vdyn.slot][1] is None                  # downloaded once, then the host owns it
    assert not cls.sspec.present(d) and not cls.lamsspec.present(d)


def check_trap_spectrum(gold):
    d = dynspec()
    d.calc_sspec(trap=True)
    assert same_bits(d.trapdyn, gold["t_default_trapdyn"]) and lin_close(d.trapsspec, gold["t_default_trapsspec"])
    d.dyn = d.dyn * 2.0                                     # trap=True rescales every time (hasattr(self, 'trap') is never true)
    d.calc_sspec(trap=True)
    assert not same_bits(d.trapdyn, gold["t_default_trapdyn"])


def check_names(gold):
    """'orbit' equals 'velocity'; velocity=True too; 'lambda-velocity' runs both branches in the reference's order."""
    a, b, c, e = dynspec(), dynspec(), dynspec(), dynspec()
    a.scale_dyn(scale='velocity', pars=dict(sc.BINARY))
    b.scale_dyn(scale='orbit', pars=dict(sc.BINARY))
    c.scale_dyn(scale='none', velocity=True, pars=dict(sc.BINARY))
    assert same_bits(a.vdyn, b.vdyn) and same_bits(a.vdyn, c.vdyn)
    e.scale_dyn(scale='lambda-velocity', pars=dict(sc.BINARY))
    assert rel(e.vlamdyn, gold["v_ecc_vlamdyn"]) <= 1e-12 + TOL and same_bits(e.vdyn, a.vdyn)
    t = dynspec()
    t.scale_dyn(scale='none', trap=True)
    assert same_bits(t.trapdyn, gold["t_default_trapdyn"])


def check_parfile(gold, tmp_path):
    path = tmp_path / "test.par"
    path.write_text(sc.PARFILE)
    d = dynspec()
    d.scale_dyn(scale='velocity', parfile=str(path), **sc.PARFILE_KW)
    assert rel(d.vdyn, gold["v_parfile_vdyn"]) <= TOL
