"""The checks of the screen simulator, shared by the GPU tests (tests/test_gpu_sim.py) and the host-interpreter tests
(tests/test_sim_emu_cpu.py): `S` is scintools_amd.scint_sim bound to a GPU or to the interpreter, `gold` the reference's outputs
(tests/golden/sim.npz, tests/golden/make_golden_sim.py).  A case is simulated once per backend and shared, read-only.

Tolerances (derived, none measured on the code under test):
  w         4 ulp of each entry (a pow, an exp and three products on top of correctly rounded inputs); the entries the reference
            leaves at zero are exactly zero.
  xyp       rms(diff) <= 8 eps log2(nx ny) rms(xyp): the standard FFT rounding bound, the constant 8 covering both
            implementations; no element off by more than sqrt(nx ny) times that.
  spe       |diff| <= 2^-22 |spe_ref| + 1e-12 max|spe_ref| per element: both sides round a double that agrees to 1e-13 to complex64,
            so they differ by at most one float ulp of a component (<= 2^-23 |spe|); twice that plus the double-precision floor.
  spi, dyn  the same rule squared: |diff| <= 2^-21 ref + 2e-12 max(ref) (d|z|^2 = 2 |z| d|z|).  With efield=True dyn is real(spe),
            a component of spe, and takes spe's bound on the modulus.
  xyi       1e-12 of its maximum.
  pulsewin  1e-5 of its maximum: the two complex64 inputs differ by at most 2^-22 |spe| per element (a float ulp in each component),
            the transforms therefore by d <= 2^-22 max|spe| ||window||_1, the intensities by 2 |p| d + d^2.  With
            R = max|spe| ||window||_1 / max|p| (the triangle bound over the actual peak, from the REFERENCE's data; asserted <= 20)
            that is <= 2^-21 R (1 + 2^-23 R) max|p|^2 <= 1e-5 max|p|^2.
  dm        xyp's per-element bound times dlam / pi.
  scalars and axes: equal."""
import contextlib
import functools
import os

import numpy as np

import sim_cases as sc

EPS = 2.0 ** -52


def spe_close(got, ref):
    return bool(np.all(np.abs(got - ref) <= 2.0 ** -22 * np.abs(ref) + 1e-12 * np.abs(ref).max()))


def intensity_close(got, ref):
    return bool(np.all(np.abs(got.astype(float) - ref.astype(float)) <= 2.0 ** -21 * np.abs(ref) + 2e-12 * np.abs(ref).max()))


def xyp_bounds(ref):
    n = ref.size
    rms = 8 * EPS * np.log2(n) * np.sqrt(np.mean(ref ** 2))
    return rms, np.sqrt(n) * rms


_runs = {}


def run(S, backend, case):
    """The simulation of a case on this backend ('gpu' / 'emu'): computed once, arrays read-only."""
    key = (backend, case)
    if key not in _runs:
        s = S.Simulation(**sc.kwargs(case))
        for v in vars(s).values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _runs[key] = s
    return _runs[key]


@contextlib.contextmanager
def column_switch(value):
    old = os.environ.get("SCINT_SIM_COLUMN")
    if value is None:
        os.environ.pop("SCINT_SIM_COLUMN", None)
    else:
        os.environ["SCINT_SIM_COLUMN"] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("SCINT_SIM_COLUMN", None)
        else:
            os.environ["SCINT_SIM_COLUMN"] = old


def check_golden(S, backend, gold, case, pytest):
    with column_switch(None):
        s = run(S, backend, case)
    g = {k: gold[f"{case}_{k}"] for k in sc.ARRAYS + sc.SCALARS}
    nx, ny, nf = (sc.CASES[case][k] for k in ("nx", "ny", "nf"))
    # w
    assert s.w.shape == (nx, ny) and s.w.dtype == np.float64
    ulps = np.abs(s.w - g["w"]) / np.spacing(np.abs(g["w"]))
    print(case, "w: max ulp", ulps.max(), "zeros", int((g["w"] == 0).sum()))
    assert np.all(s.w[g["w"] == 0] == 0) and (g["w"] == 0).sum() == 2
    assert ulps.max() <= 4
    # xyp
    rms_tol, max_tol = xyp_bounds(g["xyp"])
    d = s.xyp - g["xyp"]
    print(case, "xyp: rms", np.sqrt(np.mean(d ** 2)), "of", rms_tol, "max", np.abs(d).max(), "of", max_tol)
    assert np.sqrt(np.mean(d ** 2)) <= rms_tol and np.abs(d).max() <= max_tol
    # spe, spi, dyn, xyi
    assert s.spe.dtype == np.complex64 and s.spe.shape == (nx, nf) and s.spi.dtype == np.float32
    differ = float(np.mean(s.spe != g["spe"]))
    print(case, "spe: share of elements not bit-identical", differ, "max |diff| / |ref|", (np.abs(s.spe - g["spe"]) / np.abs(g["spe"])).max())
    assert spe_close(s.spe, g["spe"])
    assert intensity_close(s.spi, g["spi"])
    assert s.dyn.shape == g["dyn"].shape and s.dyn.dtype == g["dyn"].dtype
    if sc.CASES[case].get("efield"):
        nsub = s.dyn.shape[1]
        assert np.all(np.abs(s.dyn - g["dyn"]) <= 2.0 ** -22 * np.abs(g["spe"][:nsub].T) + 1e-12 * np.abs(g["spe"]).max())
    else:
        assert intensity_close(s.dyn, g["dyn"])
    print(case, "xyi: max |diff| / max", np.abs(s.xyi - g["xyi"]).max() / g["xyi"].max())
    assert np.abs(s.xyi - g["xyi"]).max() <= 1e-12 * g["xyi"].max()
    # dm, pulsewin
    assert np.abs(s.dm - g["dm"]).max() <= max_tol * sc.CASES[case].get("dlam", 0.25) / np.pi * (1 + 1e-12)
    n2 = 2 * nf
    if n2 >= 16 and n2 & (n2 - 1) == 0:
        R = np.abs(g["spe"]).max() * np.abs(np.blackman(nf)).sum() / np.sqrt(g["pulsewin"].max())
        assert R <= 20
        pw = s.pulsewin
        print(case, "pulsewin: max |diff| / max", np.abs(pw - g["pulsewin"]).max() / g["pulsewin"].max(), "R", R)
        assert pw.shape == g["pulsewin"].shape and np.abs(pw - g["pulsewin"]).max() <= 1e-5 * g["pulsewin"].max()
    else:
        with pytest.raises(NotImplementedError):
            s.pulsewin
    # scalars and axes: host arithmetic restated operation by operation
    for k in ("freqs", "times", "x", "lams"):
        assert np.array_equal(getattr(s, k), g[k]), k
    for k in sc.SCALARS:
        assert getattr(s, k) == g[k][()], (k, getattr(s, k), g[k][()])
    assert s.name == str(gold[f"{case}_name"][()]) and s.header[0] == s.name
    return differ


def check_shortcut(S, gold, case):
    """The column shortcut against the full inverse transform (SCINT_SIM_COLUMN=0): the switch changes the route, spe agrees."""
    ref = gold[f"{case}_spe"]
    with column_switch("0"):
        full = S.Simulation(**sc.kwargs(case))
        assert S.last_route()[0] is False
    with column_switch(None):
        col = S.Simulation(**sc.kwargs(case))
        assert S.last_route()[0] is True
    print(case, "shortcut vs full: share of elements not bit-identical", float(np.mean(full.spe != col.spe)))
    assert spe_close(full.spe, ref) and spe_close(col.spe, ref) and spe_close(col.spe, full.spe)
    assert np.abs(full.xyi - col.xyi).max() <= 1e-12 * col.xyi.max()


def check_grouping(S, backend):
    """Case b's 5 frequencies in groups of 2 + 2 + 1: bit-identical to the ungrouped run."""
    import ctypes
    from scintools_amd import _lib
    with column_switch(None):
        whole = run(S, backend, "b")
        kw = sc.kwargs("b")
        need = ctypes.c_size_t()
        _lib.check(_lib.load().scint_sim_field_workspace_bytes(kw["nx"], kw["ny"], 2, ctypes.byref(need)), "workspace_bytes")
        part = S.Simulation(group_bytes=need.value, **kw)
        assert S.last_route() == (True, 3)
        assert np.array_equal(part.spe, whole.spe) and np.array_equal(part.spi, whole.spi) and np.array_equal(part.xyi, whole.xyi)
        S.Simulation(**kw)
        assert S.last_route() == (True, 1)


def check_deterministic(S):
    with column_switch(None):
        a, b = S.Simulation(**sc.kwargs("b")), S.Simulation(**sc.kwargs("b"))
    assert np.array_equal(a.spe, b.spe) and np.array_equal(a.xyp, b.xyp) and np.array_equal(a.w, b.w)


def check_errors(S, pytest):
    for bad in (dict(nx=48, ny=16, nf=2), dict(nx=16, ny=8, nf=2), dict(nx=16, ny=16, nf=1), dict(nx=2 ** 18, ny=16, nf=2)):
        with pytest.raises(ValueError):
            S.Simulation(seed=1, **bad)
    with pytest.raises(NotImplementedError):
        S.Simulation(nx=16, ny=16, nf=2, seed=1, plot=True)


@functools.lru_cache(maxsize=None)
def oracle_512():
    from oracle.sim_oracle import BASELINE_SCREEN, Simulation
    return Simulation(nx=512, ny=16, nf=7, seed=3, **BASELINE_SCREEN)


def check_oracle(S):
    """A size the goldens do not hold (three column passes on x), against the host restatement."""
    from oracle.sim_oracle import BASELINE_SCREEN
    o = oracle_512()
    with column_switch(None):
        s = S.Simulation(nx=512, ny=16, nf=7, seed=3, **BASELINE_SCREEN)
    print("oracle 512 x 16 x 7: share of elements not bit-identical", float(np.mean(s.spe != o.spe)))
    assert spe_close(s.spe, o.spe)
    assert intensity_close(s.dyn, o.dyn) and np.array_equal(s.freqs, o.freqs) and s.eta == o.eta
