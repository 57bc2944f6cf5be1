"""The checks of the theta-theta eigen sweep across the packed mat-vec classes, shared by the GPU tests
(tests/test_gpu_sweep_classes.py) and the host-interpreter tests (tests/test_sweep_classes_emu_cpu.py): `thth` is
scintools_amd.ththmod bound to a GPU or to the interpreter, `backend` ('gpu' / 'emu') only labels the printed lines and keys the
float64 results the mixed-precision checks compare with.  Inputs and references come from tests/sweep_class_cases.py.

Every check prints what it measured on a SWEEPCLASS line before it asserts (run with -s to collect them).

Bars (none of them new)
  REL      1e-9   eigenvalue against LAPACK's eigvalsh of the oracle's reduced matrix (tests/test_gpu_edges.py)
  RESID    1e-8   || A v - w v || <= RESID |w| on the oracle's matrix (tests/test_gpu_edges.py)
  MIXED    1e-12  mixed-precision value against the float64 sweep's (tests/test_gpu_zz_mixed.py)"""
import contextlib
import ctypes
import warnings

import numpy as np

import sweep_class_cases as sc
from oracle import thth_oracle as to

REL = 1e-9
RESID = 1e-8
MIXED = 1e-12
EMPTY = 5                       # status of a curvature whose crop keeps fewer than two centres

_f64 = {}                       # (backend, what, n) -> the float64 sweep's result, for the mixed-precision checks


def stats():
    from scintools_amd import _lib
    st = (ctypes.c_double * 4)()
    _lib.check(_lib.load().scint_sweep_stats(st), "scint_sweep_stats")
    return dict(bytes32=st[0], bytes64=st[1], certified=st[2], cert_passes=st[3])


@contextlib.contextmanager
def precision(thth, mode):
    assert thth.sweep_precision(mode) == "f64"
    try:
        yield
    finally:
        assert thth.sweep_precision("f64") == mode


def check_defaults(thth):
    from scintools_amd import _lib
    assert thth.DEFAULT_MAX_ITER == sc.MAX_ITER and thth.DEFAULT_TOL == sc.TOL
    assert thth.sweep_precision(None) == "f64"
    sc.assert_build_constants(_lib.load())


def _line(backend, mode, what, n, **kw):
    nb = sc.nb_of(n)
    print(f"\nSWEEPCLASS {backend} mode={mode} check={what} N={n} nb={nb} strip={sc.strip_len(nb)} wg={sc.workgroups(nb)} "
          + " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in kw.items()))


def _degenerate(thth, backend, mode, n, pair):
    """N = 1: the reduced map is the 1 x 1 zero matrix.  The reference raises, the sweep reports an empty crop and NaN."""
    c = sc.case(n)
    args = (c["CS"], c["tau"], c["fd"], np.array([c["eta"]]), c["edges"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # (the mean of an empty slice, on its way to the IndexError)
        try:
            to.thth_redmap(c["CS"], c["tau"], c["fd"], c["eta"], c["edges"])
            raised = False
        except IndexError:
            raised = True
    if pair:
        w, V, info = thth.eigvec_sweep(*args)
        vals = w
        assert not V.cpu().numpy().any()
    else:
        vals, info = thth.eval_sweep(*args, return_info=True)
    _line(backend, mode, "pair" if pair else "value", n, status=int(info["status"][0]), value=float(vals[0]))
    assert raised and int(info["N"][0]) == n
    assert int(info["status"][0]) == EMPTY and np.isnan(vals[0])


def _value(thth, backend, mode, n):
    c = sc.case(n)
    args = (c["CS"], c["tau"], c["fd"], np.array([c["eta"]]), c["edges"])
    ref = sc.lapack_top(n)
    a, info = thth.eval_sweep(*args, return_info=True)
    st = stats()
    b = thth.eval_sweep(*args)
    rel = abs(a[0] - ref) / ref
    out = dict(value=a[0], rel=float(rel), iters=int(info["iters"][0]), status=int(info["status"][0]), N=int(info["N"][0]),
               same_bits=bool(np.array_equal(a, b)), stats=st)
    return out


def check_value_f64(thth, backend, n):
    """1. eval_sweep, one curvature, against LAPACK; a second call gives the same bits."""
    if n in sc.DEGENERATE:
        return _degenerate(thth, backend, "f64", n, False)
    r = _value(thth, backend, "f64", n)
    _f64[(backend, "value", n)] = r["value"]
    _line(backend, "f64", "value", n, rel=r["rel"], iters=r["iters"], status=r["status"])
    assert r["N"] == n and sc.matrix(n).shape == (n, n)
    assert r["status"] == 0 and r["iters"] < sc.MAX_ITER
    assert r["rel"] <= REL
    assert r["same_bits"]
    assert r["stats"]["bytes32"] == 0


def _pair(thth, backend, n):
    c = sc.case(n)
    args = (c["CS"], c["tau"], c["fd"], np.array([c["eta"]]), c["edges"])
    A, ref = sc.matrix(n), sc.lapack_top(n)
    w, V, info = thth.eigvec_sweep(*args)
    st = stats()
    row = V.cpu().numpy()[0]
    v = row[:n]
    resid = float(np.linalg.norm(A @ v - w[0] * v) / abs(w[0]))
    return dict(w=w[0], v=v, rel=float(abs(w[0] - ref) / ref), resid=resid, iters=int(info["iters"][0]),
                status=int(info["status"][0]), N=int(info["N"][0]), tail_zero=not row[n:].any(),
                norm=float(np.linalg.norm(v)), stats=st)


def _assert_pair(r, n):
    assert r["N"] == n and sc.matrix(n).shape == (n, n)
    assert r["status"] == 0 and r["iters"] < sc.MAX_ITER
    assert r["rel"] <= REL
    assert r["resid"] <= RESID
    assert r["tail_zero"]                                    # v is exactly zero beyond N
    assert abs(r["norm"] - 1.0) <= 1e-12


def check_pair_f64(thth, backend, n):
    """2. eigvec_sweep: w against LAPACK, the residual on the oracle's matrix, v zero beyond N."""
    if n in sc.DEGENERATE:
        return _degenerate(thth, backend, "f64", n, True)
    r = _pair(thth, backend, n)
    _f64[(backend, "pair", n)] = r["w"]
    _line(backend, "f64", "pair", n, rel=r["rel"], resid=r["resid"], iters=r["iters"], status=r["status"])
    _assert_pair(r, n)
    assert r["stats"]["bytes32"] == 0


def check_value_mixed(thth, backend, n):
    """3a. the eigenvalue under sweep_precision('mixed'): LAPACK, the float64 sweep, one certificate."""
    if n in sc.DEGENERATE:
        with precision(thth, "mixed"):
            return _degenerate(thth, backend, "mixed", n, False)
    if (backend, "value", n) not in _f64:
        _f64[(backend, "value", n)] = _value(thth, backend, "f64", n)["value"]
    e64 = _f64[(backend, "value", n)]
    with precision(thth, "mixed"):
        r = _value(thth, backend, "mixed", n)
    d64 = float(abs(r["value"] - e64) / abs(e64))
    _line(backend, "mixed", "value", n, rel=r["rel"], vs_f64=d64, iters=r["iters"], status=r["status"],
          certified=int(r["stats"]["certified"]), cert_passes=int(r["stats"]["cert_passes"]))
    assert r["N"] == n and r["status"] == 0 and r["iters"] < sc.MAX_ITER
    assert r["rel"] <= REL
    assert d64 <= MIXED
    assert r["same_bits"]
    assert r["stats"]["certified"] == 1 and r["stats"]["bytes32"] > 0


def check_pair_mixed(thth, backend, n):
    """3b. the eigenpair under sweep_precision('mixed-all'): the bars of check 2, the float64 sweep's w, one certificate."""
    if n in sc.DEGENERATE:
        with precision(thth, "mixed-all"):
            return _degenerate(thth, backend, "mixed-all", n, True)
    if (backend, "pair", n) not in _f64:
        _f64[(backend, "pair", n)] = _pair(thth, backend, n)["w"]
    w64 = _f64[(backend, "pair", n)]
    with precision(thth, "mixed-all"):
        r = _pair(thth, backend, n)
    d64 = float(abs(r["w"] - w64) / abs(w64))
    _line(backend, "mixed-all", "pair", n, rel=r["rel"], resid=r["resid"], vs_f64=d64, iters=r["iters"], status=r["status"],
          certified=int(r["stats"]["certified"]))
    _assert_pair(r, n)
    assert d64 <= MIXED
    assert r["stats"]["certified"] == 1 and r["stats"]["bytes32"] > 0


def check_mixed_sizes_in_one_call(thth, backend, full, nb_lo, nb_hi):
    """4. One eval_sweep and one eigvec_sweep of twelve curvatures whose crops span nb_lo .. nb_hi block rows, batch = 3 (every
    slot is used four times), in descending and in ascending order of N: every value against LAPACK, and bit-equal to the same
    curvature swept alone."""
    c = sc.mixed_case(full)
    n_ref, lam = sc.mixed_reference(full)
    args = (c["CS"], c["tau"], c["fd"])
    etas = c["etas"]
    assert len(etas) >= 12 and len(etas) >= 3 * sc.MIXED_BATCH and np.all(np.diff(n_ref) < 0)
    alone_e = np.array([thth.eval_sweep(*args, etas[k:k + 1], c["edges"])[0] for k in range(len(etas))])
    alone = [thth.eigvec_sweep(*args, etas[k:k + 1], c["edges"]) for k in range(len(etas))]
    alone_w = np.array([a[0][0] for a in alone])
    alone_v = np.stack([a[1].cpu().numpy()[0] for a in alone])
    for name, order in (("descending", np.arange(len(etas))), ("ascending", np.arange(len(etas))[::-1])):
        e, info = thth.eval_sweep(*args, etas[order], c["edges"], batch=sc.MIXED_BATCH, return_info=True)
        w, V, vinfo = thth.eigvec_sweep(*args, etas[order], c["edges"], batch=sc.MIXED_BATCH)
        V = V.cpu().numpy()
        nbs = [sc.nb_of(int(n)) for n in info["N"]]
        classes = sorted({sc.strip_len(nb) for nb in nbs})
        rel_e, rel_w = np.abs(e - lam[order]) / lam[order], np.abs(w - lam[order]) / lam[order]
        resid = 0.0
        for k, j in enumerate(order):
            n = int(n_ref[j])
            red = to.thth_redmap(c["CS"], c["tau"], c["fd"], etas[j], c["edges"])[0]
            resid = max(resid, float(np.linalg.norm(red @ V[k, :n] - w[k] * V[k, :n]) / abs(w[k])))
            assert not V[k, n:].any()
        print(f"\nSWEEPCLASS {backend} mode=f64 check=onecall order={name} N={list(map(int, info['N']))} nb={nbs} strips={classes} "
              f"batch={info['batch']} rel={rel_e.max():.3e} rel_pair={rel_w.max():.3e} resid={resid:.3e} "
              f"iters={int(max(info['iters'].max(), vinfo['iters'].max()))} "
              f"bits_value={bool(np.array_equal(e, alone_e[order]))} bits_pair={bool(np.array_equal(w, alone_w[order]) and np.array_equal(V, alone_v[order]))}")
        assert np.array_equal(info["N"], n_ref[order]) and np.array_equal(vinfo["N"], n_ref[order])
        assert min(nbs) <= nb_lo and max(nbs) >= nb_hi and len(classes) >= 3
        assert info["batch"] == sc.MIXED_BATCH and vinfo["batch"] == sc.MIXED_BATCH
        assert np.all(info["status"] == 0) and np.all(vinfo["status"] == 0)
        assert max(info["iters"].max(), vinfo["iters"].max()) < sc.MAX_ITER
        assert rel_e.max() <= REL and rel_w.max() <= REL and resid <= RESID
        assert np.array_equal(e, alone_e[order])
        assert np.array_equal(w, alone_w[order]) and np.array_equal(V, alone_v[order])


def check_stack(thth, backend):
    """5. eval_sweep_multi on three spectra with their own grids, N in three strip-length classes: bit-equal to the per-spectrum
    sweeps, and against LAPACK."""
    stack, grids, etas = sc.stack_case()
    out, info = thth.eval_sweep_multi(stack, grids, etas, return_info=True)
    classes = sorted({sc.strip_len(sc.nb_of(int(n))) for n in info["N"]})
    worst, same, k = 0.0, True, 0
    for s, (g, et) in enumerate(zip(grids, etas)):
        one = thth.eval_sweep(stack[s], g[0], g[1], et, g[2])
        same = same and bool(np.array_equal(one, out[s]))
        for e, v in zip(et, out[s]):
            red = to.thth_redmap(stack[s], g[0], g[1], e, g[2])[0]
            assert red.shape[0] == int(info["N"][k])
            ref = np.linalg.eigvalsh(red)[-1]
            worst = max(worst, float(abs(v - ref) / ref))
            k += 1
    print(f"\nSWEEPCLASS {backend} mode=f64 check=stack N={list(map(int, info['N']))} strips={classes} rel={worst:.3e} "
          f"iters={int(info['iters'].max())} bits={same}")
    assert len(classes) >= 3
    assert np.all(info["status"] == 0) and info["iters"].max() < sc.MAX_ITER
    assert worst <= REL
    assert same


# ---- conditions on the inputs (oracle and LAPACK alone) ------------------------------------------------------------------------
TILE_SENSITIVITY = 1e-6         # 1000 x REL
GAP = 0.01


def input_conditions(n):
    """dict(gap, tile, tile_at, last_row, lam_ratio) of case n: the relative gap (lambda_1 - lambda_2) / lambda_1; the smallest
    first-order shift of lambda_1 from zeroing one stored tile, |v_I^H A_IJ v_J| (doubled for I < J) / lambda_1, over the tiles
    not in ONE_ROW_TILES, and where; for N = 1 (mod 64) the exact relative shift of lambda_1 from zeroing the live last row and
    column; lambda_min / lambda_max."""
    import scipy.linalg as sl
    A = sc.matrix(n)
    w, V = sl.eigh(A, subset_by_index=[n - 2, n - 1])
    lam, lam2, v = float(w[1]), float(w[0]), V[:, 1]
    assert abs(lam - sc.lapack_top(n)) <= 1e-12 * lam
    nb = sc.nb_of(n)
    skip = set(sc.ONE_ROW_TILES.get(n, ()))
    tile, at = np.inf, None
    T = sc.TILE
    for i in range(nb):
        vi = v[T * i:T * i + T]
        for j in range(i, nb):
            if (i, j) in skip:
                continue
            s = (2 if j > i else 1) * abs(np.vdot(vi, A[T * i:T * i + T, T * j:T * j + T] @ v[T * j:T * j + T])) / lam
            if s < tile:
                tile, at = float(s), (i, j)
    last = None
    if n in sc.ONE_ROW_TILES:
        B = A.copy()
        B[-1, :] = 0
        B[:, -1] = 0
        last = float((lam - sl.eigh(B, eigvals_only=True, subset_by_index=[n - 1, n - 1])[0]) / lam)
    lam_min = float(sl.eigh(A, eigvals_only=True, subset_by_index=[0, 0])[0])
    return dict(gap=(lam - lam2) / lam, tile=tile, tile_at=at, last_row=last, lam_ratio=lam_min / lam)
