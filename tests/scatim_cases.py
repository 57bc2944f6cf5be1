"""Inputs of the scattered-image tests, regenerated from seeds by tests/golden/make_golden_scatim.py and by the tests: a 128 x 128
seeded screen (oracle/sim_oracle.py) whose secondary spectrum is 128 x 256, and two seeded fields of bounded dynamic range (field()).
tests/golden/scatim.npz stores only the unmodified reference's outputs for CASES."""
import functools
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SIM = dict(mb2=20, ar=2, psi=0, alpha=5 / 3, inner=0.001, ds=0.01, dlam=0.25, freq=1400, dt=30, nx=128, ny=32, nf=128, seed=2024)

# keyword arguments of calc_scattered_image per stored case; 'field': the input_sspec route
CASES = {
    "a": dict(input_eta=0.02, sampling=8),                      # frequency steps, a given curvature
    "b": dict(fit_arc=False, sampling=8, field="wide"),         # no curvature: the corner fallback (slice bound -4: 4 columns)
    "c": dict(lamsteps=True, sampling=16),                      # wavelength steps after fit_arc
    "d": dict(input_eta=2e-4, sampling=8),                      # flim == 0: the rows are cropped, tdel = fdop[:tlim]
    "e": dict(input_eta=0.5, sampling=16),                      # most delays clamp at tdel[-1]
    "f": dict(input_eta=0.3, sampling=16, field="uneven"),     # input_sspec, non-uniform input_tdel
}
STORED = ("scattered_image", "scattered_image_ax")


@functools.lru_cache(maxsize=None)
def sim():
    from oracle import sim_oracle
    s = sim_oracle.Simulation(**SIM)
    s.dyn = np.array(s.dyn, dtype=np.float64)
    s.dyn.setflags(write=False)
    return s


def bounded_field(shape, seed, decades=4.0):
    """Linear power spread log-uniformly over `decades` decades (bounded dynamic range), in dB."""
    rng = np.random.default_rng(seed)
    return 10.0 * decades * (rng.random(shape) - 1.0)


@functools.lru_cache(maxsize=None)
def field(which):
    """(sspec dB, fdop, tdel).  'uneven': 40 x 60, tdel strictly increasing with uneven steps.  'wide': 10 x 320, where the
    reference's corner fallback gives flim = 2 and the column slice [2 - 6 : 320 - 2 + 6] = the last 4 columns."""
    if which == "wide":
        sspec = bounded_field((10, 320), 12)
        fdop = np.arange(-160, 160) * 0.1
        tdel = np.arange(10) * 0.5
    else:
        rng = np.random.default_rng(7)
        sspec = bounded_field((40, 60), 11)
        fdop = np.arange(-30, 30) * 0.25
        tdel = np.cumsum(0.05 + 0.1 * rng.random(40)) - 0.05
    for v in (sspec, fdop, tdel):
        v.setflags(write=False)
    return sspec, fdop, tdel


def call_kwargs(case):
    """The keyword arguments for calc_scattered_image (reference or port) of a stored case."""
    kw = dict(CASES[case])
    which = kw.pop("field", None)
    if which:
        sspec, fdop, tdel = field(which)
        kw.update(input_sspec=sspec, input_fdop=fdop, input_tdel=tdel)
    return kw
