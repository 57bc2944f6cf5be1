"""Inputs of the approximate 2-D ACF fit tests (tests/test_gpu_acf2d.py, tests/test_acf2d_emu_cpu.py, tests/test_acf2d_cpu.py) and
of tests/golden/make_acf2d_tolerances.py -- TEST INFRASTRUCTURE.  Everything is seeded and made with NumPy alone.

Two kinds of ACF stack:

  (a) known answers: the whole ACF is the model (scint_models.py:123-161) at chosen (tau, dnu, amp, 5/3, phasegrad) on the ACF's own
      ticks, plus a white-noise spike at its maximum (the window's centre, whose weight is zero).  The phase gradient is never
      planted at 0: it is compared on its own scale;
  (b) realistic: the ACFs of tests/acf1d_cases.py (small dynamic spectra of a correlated complex Gaussian field plus noise), and one
      hand-made stack whose middle ACF never falls to half power along frequency.

The shapes are the smallest at which the kernel (one 256-thread workgroup per problem, thread tid walks points tid, tid + 256, ...,
a wave butterfly and a four-wave LDS stage per reduction) can still go wrong:

  tiny          (a) B = 5, 16 x 16, nscale=1: windows of 7 x 7 = 49 points, fewer than a wavefront
  tilted        (a) B = 3, 40 x 64, phase gradients of both signs: windows of more than 256 points
  odd           (a) B = 2, 37 x 51: odd ACF sides (no tick at zero lag)
  full          (b) B = 2, 40 x 64, full_frame: 39 x 63 = 2457 points, ten trips per thread
  real12        (b) B = 12, 64 x 96 (32 x 48 spectra, seed 5); real12_alpha: alpha varies
  real300       (b) B = 300, 48 x 64
  long          (a) B = 1, 20 x 2000, full_frame: 19 x 1999 points
  badwin        (b) B = 3, 40 x 64: the middle ACF never crosses half power, so its window has an even side (FIT_BAD_WINDOW)
"""
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import acf1d_cases as c1  # noqa: E402
import acf2d_oracle as ao  # noqa: E402

DT, DF = c1.DT, c1.DF
FIT_KEYS = ao.NAMES
ERR_KEYS = tuple(k + "err" for k in FIT_KEYS)
SETUP_KW = ("nsub", "nchan", "nscale", "full_frame", "weighted", "bartlett", "alpha", "phasegrad0", "tau_input")


def _case(stack, kind, planted=None, **kw):
    B, R, C = stack.shape
    return types.SimpleNamespace(stack=np.ascontiguousarray(stack), kind=kind, planted=planted, dt=DT, df=DF, bw=(R // 2) * DF,
                                 tobs=(C // 2) * DT, kw=kw)


def planted_acf(R, C, tau, dnu, amp, pg, wn):
    tobs, bw = (C // 2) * DT, (R // 2) * DF
    tticks = np.linspace(-tobs, tobs, C + 1)[:-1]
    fticks = np.linspace(-bw, bw, R + 1)[:-1]
    acf = ao.model((tau, dnu, amp, 5/3, pg), tticks, fticks, tobs, bw)
    acf[np.unravel_index(np.argmax(acf), acf.shape)] += wn
    return acf


def _planted(R, C, params, **kw):
    stack = np.stack([planted_acf(R, C, *p) for p in params])
    return _case(stack, "a", planted=np.array([[p[0], p[1], p[2], 5/3, p[3]] for p in params]), **kw)


def _realistic(seed, B, nf, nt, lf, lt, noise, **kw):
    from oracle import sspec_oracle
    rng = np.random.default_rng(seed)
    stack = np.stack([sspec_oracle.calc_acf(c1.realistic_dyn(rng, nf, nt, lf, lt, noise)) for _ in range(B)])
    return _case(stack, "b", **kw)


def _badwin():
    """Two realistic ACFs around one that decays along frequency to 70 % only: dnu starts at bw, nscale exceeds bw / dnu, and the
    reference's frequency branch leaves a window with an even side."""
    R, C = 40, 64
    good = _realistic(9, 2, R // 2, C // 2, 2.0, 3.0, 0.05).stack
    t = DT * (np.arange(C) - C // 2)[None, :]
    f = DF * (np.arange(R) - R // 2)[:, None]
    mid = 0.8 * np.exp(-np.abs(t / 150.0) ** (5/3)) * (0.7 + 0.3 * np.exp(-np.abs(f)))
    mid[R // 2, C // 2] += 0.2
    return _case(np.stack([good[0], mid, good[1]]), "b")


_BUILDERS = {
    "tiny": lambda: _planted(16, 16, [(70.0, 1.2, 0.8, 0.3, 0.2), (65.0, 1.1, 0.9, -0.25, 0.1), (75.0, 1.3, 0.7, 0.2, 0.3),
                                      (60.0, 1.15, 1.0, -0.15, 0.05), (72.0, 1.25, 0.85, 0.35, 0.15)], nscale=1),
    "tilted": lambda: _planted(40, 64, [(150.0, 1.2, 0.8, 0.5, 0.2), (130.0, 1.0, 0.9, -0.8, 0.1), (170.0, 1.3, 0.7, 0.2, 0.3)]),
    "odd": lambda: _planted(37, 51, [(100.0, 1.0, 0.8, 0.4, 0.2), (90.0, 1.1, 0.9, -0.3, 0.1)]),
    # (a whole realistic ACF is a large-residual problem: Gauss-Newton steps converge linearly, the oracle itself takes 123
    # evaluations on the first one -- so the caller raises the iteration cap from its default of 200)
    "full": lambda: _realistic(13, 2, 20, 32, 2.0, 3.0, 0.05, full_frame=True, max_iter=1000),
    "real12": lambda: _realistic(5, 12, 32, 48, 2.5, 3.5, 0.1),
    "real12_alpha": lambda: _realistic(5, 12, 32, 48, 2.5, 3.5, 0.1, alpha=None),
    "real300": lambda: _realistic(8, 300, 24, 32, 2.0, 3.0, 0.05),     # (seed 7: the oracle finds two minima in problem 84)
    "long": lambda: _planted(20, 2000, [(3000.0, 1.0, 0.8, 4.0, 0.2)], full_frame=True),
    "badwin": _badwin,
}
FIT_CASES = tuple(k for k in _BUILDERS if k != "badwin")        # every problem of these converges
CASES = tuple(_BUILDERS)
_cache = {}


def case(name):
    """The case `name` (built once, then shared: do not write into its arrays)."""
    if name not in _cache:
        _cache[name] = _BUILDERS[name]()
    return _cache[name]


def setup_kw(c):
    return {k: v for k, v in c.kw.items() if k in SETUP_KW}


def oracle(name):
    """(setups, fits) of the host oracle for every problem of the case (computed once); a setup is None where the window is bad."""
    key = ("oracle", name)
    if key not in _cache:
        c = case(name)
        setups, fits = [], []
        for acf in c.stack:
            try:
                s = ao.setup(acf, c.dt, c.df, c.bw, c.tobs, **setup_kw(c))
                setups.append(s)
                fits.append(ao.fit(s, alpha=c.kw.get("alpha", 5/3)))
            except ao.BadWindow as bad:
                setups.append(None)
                fits.append(dict(success=False, rect=bad.args[0]))
        _cache[key] = (setups, fits)
    return _cache[key]


def observation(rng_seed=21, nf=32, nt=48):
    """A kind (b) observation for Dynspec.fit_scint_params_2d and fit_scint_params_2d_cut (that of the 1-D tests)."""
    return c1.observation(rng_seed=rng_seed, nf=nf, nt=nt)
