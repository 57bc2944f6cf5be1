"""Inputs of the slow_FT tests, regenerated from seeds by tests/golden/make_golden_slowft.py and by the tests.
tests/golden/slowft.npz stores only the unmodified reference's outputs for GOLDEN."""
import functools

import numpy as np

B = 32            # table block of the stage-1 kernel (csrc/slowft.hpp, kSlowB)
G = 8             # blocks per outer phase (kSlowG): B * G samples share one

FREQ_KINDS = ("asc", "desc", "uneven")

# stored cases: ntime x nfreq and the ordering of freqs.  The three shapes of the issue with all three orderings, except that
# 256 x 64 is stored once (its output is 256 KiB; three of them would push slowft.npz past the size limit of a committed file).
GOLDEN = {
    "a_asc": (64, 48, "asc"), "a_desc": (64, 48, "desc"), "a_uneven": (64, 48, "uneven"),
    "b_desc": (256, 64, "desc"),
    "c_asc": (250, 37, "asc"), "c_desc": (250, 37, "desc"), "c_uneven": (250, 37, "uneven"),
}


def freqs(nf, kind, lo=1200.0, hi=1600.0):
    """nf channel frequencies in MHz between lo and hi: ascending, descending, or ascending with uneven steps."""
    if kind == "const":
        return np.full(nf, 1400.0)
    if nf == 1:
        return np.array([lo])
    if kind == "uneven":
        rng = np.random.default_rng(1000 + nf)
        f = np.concatenate(([0.0], np.cumsum(0.25 + rng.random(nf - 1))))
        return lo + (hi - lo) * f / f[-1]
    f = np.linspace(lo, hi, nf)
    return f[::-1].copy() if kind == "desc" else f


@functools.lru_cache(maxsize=None)
def dyn(nt, nf, seed=0):
    """A seeded [time, frequency] dynamic spectrum: unit-variance noise on a positive level, read-only."""
    rng = np.random.default_rng(7919 * nt + 31 * nf + seed)
    d = 1.0 + rng.standard_normal((nt, nf))
    d.setflags(write=False)
    return d


def golden_inputs(case):
    nt, nf, kind = GOLDEN[case]
    return dyn(nt, nf), freqs(nf, kind)
