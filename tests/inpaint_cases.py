"""Seeded inputs of the biharmonic-fill tests (tests/test_inpaint_cpu.py, test_inpaint_emu_cpu.py, test_gpu_inpaint.py): the
smallest that reach every path of csrc/inpaint.hpp.

  a  24 x 20   8 % random pixels, a whole channel, a whole sub-integration, 2 x 2 blocks in three corners, a 6 x 6 block and a
               3 x 3 block on the bottom edge (in the fourth corner): all 25 stencil classes occur among the masked pixels
  b  96 x 80   the same recipe: 847 unknowns, so several workgroups and several partial sums per dot product
  c  5 x 5     the smallest image the 25 classes allow: a masked corner and the masked centre
  d  12 x 9    a single masked pixel (one conjugate-gradient step)

KAPPA records the condition number of every case's matrix, computed densely (tests/test_inpaint_cpu.py checks the record).  It
must stay below 1000: conjugate gradients reach a relative residual of about eps * kappa, so 1e-12 is then well within reach."""
import functools

import numpy as np

KAPPA_LIMIT = 1000.0
KAPPA = {"a": 179.59, "b": 180.38, "c": 3.3334, "d": 1.0}            # lambda_max / lambda_min, rounded up


def image(nf, nt, seed):
    """A positive, smooth scintillation-like pattern with 2 % noise."""
    rng = np.random.default_rng(seed)
    f, t = np.linspace(-1, 1, nf)[:, None], np.linspace(0, 1, nt)[None, :]
    smooth = 1.0 + 0.45 * np.sin(5.0 * f + 1.0) * np.cos(7.0 * t) + 0.2 * np.cos(11.0 * f) * np.sin(13.0 * t + 0.5)
    return smooth * (1.0 + 0.3 * np.sin(2.1 * np.pi * t)) * (1.0 + 0.02 * rng.standard_normal((nf, nt)))


def stencil_class(i, n):
    return i if i < 2 else (4 - (n - 1 - i) if i >= n - 2 else 2)


def classes(bad):
    """The set of stencil classes 5 a + b among the pixels of the mask."""
    nf, nt = bad.shape
    return {5 * stencil_class(r, nf) + stencil_class(c, nt) for r, c in zip(*np.nonzero(bad))}


def recipe_mask(nf, nt, seed):
    rng = np.random.default_rng(seed)
    bad = rng.random((nf, nt)) < 0.08
    bad[nf // 3, :] = True                              # a whole channel
    bad[:, (2 * nt) // 3] = True                        # a whole sub-integration
    bad[:2, :2] = bad[:2, -2:] = bad[-2:, :2] = True    # three corners
    bad[nf // 2:nf // 2 + 6, nt // 5:nt // 5 + 6] = True
    bad[-3:, -3:] = True                                # on the bottom edge
    assert classes(bad) == set(range(25)), "the recipe must reach all 25 stencil classes"
    return bad


@functools.lru_cache(maxsize=None)
def case(name):
    """(image with NaN under the mask, mask) of case ``name``; the arrays are shared and read-only."""
    if name in ("a", "b"):
        nf, nt = (24, 20) if name == "a" else (96, 80)
        dyn, bad = image(nf, nt, seed=3), recipe_mask(nf, nt, seed=4)
    elif name == "c":
        dyn = image(5, 5, seed=5)
        bad = np.zeros((5, 5), bool)
        bad[0, 0] = bad[2, 2] = True
    elif name == "d":
        dyn = image(12, 9, seed=6)
        bad = np.zeros((12, 9), bool)
        bad[7, 4] = True
    else:
        raise KeyError(name)
    dyn = np.where(bad, np.nan, dyn)
    dyn.setflags(write=False)
    bad.setflags(write=False)
    return dyn, bad


NAMES = ("a", "b", "c", "d")


def spiky_observation():
    """Case (a)'s image, unmasked, with strong spikes and one dead channel for zap() to flag: (array, spikes)."""
    dyn = image(24, 20, seed=3)
    spikes = ((3, 4), (0, 0), (23, 7), (11, 19), (12, 10), (1, 18))
    for k, (i, j) in enumerate(spikes):
        dyn[i, j] = 40.0 + 7.0 * k
    return dyn, spikes
