"""The cases of the brightness-distribution model (scint_sim.Brightness), shared by the golden maker
(tests/golden/make_golden_brightness.py), the CPU tests, the host-interpreter tests and the GPU tests.  Every step is a dyadic number,
so np.arange gives the stated lengths on any machine.  A case is at most a few tens of thousands of pixels.

  a  grid 30 (even, no power of two), isotropic, equal gradient and reference angles (the tutorial's form); spectrum 240 x 32
  b  grid 32 (a power of two), ar = 2, psi = 30, thetag != thetar on both axes; spectrum 256 x 37 (non-square, one odd length)
  c  grid 75 (odd), ar = 1.5, psi = 60, alpha = 1.5; spectrum 240 x 32
  d  grid 61 (prime), ar = 3, psi = -20; spectrum 193 x 40 (odd delay axis)
  e  grid 24, too small for the spectrum: queries fall outside it and SS, LSS and acf hold NaN (NAN_CASES)

build() asserts, from the oracle alone, that every case but e takes all three branches of the Jacobian, has no NaN, and that no query
of any case lies within 1e-6 dx of the grid's outer boundary (Qhull's inside / outside tolerance never decides a pixel)."""
import functools

import numpy as np

import brightness_oracle as bo

CASES = {
    "a": dict(nx=3.75, dx=0.25, thetagx=0.3, thetarx=0.3, nf=2, df=0.125, nt=3.75, dt=0.03125),
    "b": dict(nx=4, dx=0.25, ar=2, psi=30, thetagx=0.5, thetagy=0.25, thetarx=0.23, thetary=0.1, nf=2.3125, df=0.125, nt=4, dt=0.03125),
    "c": dict(nx=9.375, dx=0.25, ar=1.5, psi=60, alpha=1.5, thetagx=-0.4, thetarx=0.1, thetary=0.3, nf=3, df=0.1875, nt=7.5, dt=0.0625),
    "d": dict(nx=7.625, dx=0.25, ar=3, psi=-20, thetagx=0.7, thetagy=-0.3, thetarx=0.1, thetary=0.1, nf=2.5, df=0.125, nt=6.03125, dt=0.0625),
    "e": dict(nx=1.5, dx=0.125, ar=2, psi=30, thetagx=0.5, thetagy=0.07, thetarx=0.45, nf=2, df=0.125, nt=3, dt=0.0625),
}
SHAPES = {"a": (30, 240, 32), "b": (32, 256, 37), "c": (75, 240, 32), "d": (61, 193, 40), "e": (24, 96, 32)}     # grid, td, fd
NAN_CASES = ("e",)
ARRAYS = ("B", "SS", "jacobian", "thetax", "thetay", "acf")


def kwargs(case):
    return dict(CASES[case])


@functools.lru_cache(maxsize=None)
def build(case):
    """The oracle's model of a case with the main diagonal everywhere (read-only arrays), after the assertions above."""
    o = bo.model(diagonals="main", **CASES[case])
    assert (len(o["x"]), len(o["td"]), len(o["fd"])) == SHAPES[case], (case, len(o["x"]), len(o["td"]), len(o["fd"]))
    assert len(o["td"]) * len(o["fd"]) <= 40000
    margin = bo.boundary_margin(o["x"], o["thetax"], o["thetay"])
    assert margin > 1e-6, (case, margin)
    if case in NAN_CASES:
        assert np.isnan(o["SS"]).any() and np.isnan(o["acf"]).all()
    else:
        assert sorted(np.unique(o["branch"])) == [0, 1, 2], (case, np.unique(o["branch"], return_counts=True))
        assert np.isfinite(o["SS"]).all() and np.isfinite(o["acf"]).all()
    for v in o.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return o
