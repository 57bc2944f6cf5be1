"""Seeded inputs of the tests of the line-block preconditioner of the biharmonic fill (``precond='lines'``; tests/
test_inpaint_lines_cpu.py, test_inpaint_lines_emu_cpu.py, test_gpu_inpaint_lines.py): a few thousand unknowns at the most.

  a  96 x 40   a band of 60 whole channels: M = A, the direct route (time transform of 40 points: chirp-z)
  b  40 x 96   a band of 50 whole sub-integrations: the direct route, axes exchanged (frequency transform of 40 points)
  c  80 x 72   a band of 30 channels crossing one of 24 sub-integrations, 1 % isolated pixels and pixels inside the two-pixel rim
               at all four edges: the overlap of the two blocks, the diagonal part, all 25 stencil classes
  d  48 x 64   bands on the first and on the last channel and two bands two rows apart (one row with known pixels between them),
               isolated pixels: coupled bands in the compressed numbering; a time transform of 64 points (a power of two)
  e  32 x 64   a channel band and a sub-integration band: powers of two on both axes (the plain row transform)
  f  24 x 20   8 % random pixels and no whole line: the diagonal part alone
  g  7 x 5     one channel and one sub-integration: the shortest transforms (5 and 7 points in 16)

KAPPA records the condition number of every case's matrix, computed densely (tests/test_inpaint_lines_cpu.py checks the record);
RHO_REF_LIMIT bounds kappa * rho_ref of the oracle's direct solve, so that the oracle is good to 1e-4 at the very least."""
import functools

import numpy as np

import inpaint_cases as ic

RHO_REF_LIMIT = 1e-4
# lambda_max / lambda_min, rounded up in the fourth digit
KAPPA = {"a": 1884800.0, "b": 932250.0, "c": 205240.0, "d": 2557.2, "e": 8472.0, "f": 26.469, "g": 8.4358}
NAMES = ("a", "b", "c", "d", "e", "f", "g")
DIRECT = ("a", "b")                     # whole lines along one axis only: zero steps
ITERATED = ("c", "d")                   # route 'pcg'
COUNTED = ("c", "d", "f")               # step counts recorded in tests/golden/inpaint_lines_tolerances.json
SHAPES = {"a": (96, 40), "b": (40, 96), "c": (80, 72), "d": (48, 64), "e": (32, 64), "f": (24, 20), "g": (7, 5)}


def _sprinkle(bad, fraction, seed):
    rng = np.random.default_rng(seed)
    bad |= rng.random(bad.shape) < fraction


def mask(name):
    nf, nt = SHAPES[name]
    bad = np.zeros((nf, nt), bool)
    if name == "a":
        bad[18:78, :] = True
    elif name == "b":
        bad[:, 23:73] = True
    elif name == "c":
        _sprinkle(bad, 0.01, seed=11)
        bad[25:55, :] = True
        bad[:, 30:54] = True
        for r in (0, 1, 78, 79):                        # the 16 corner classes
            for c in (0, 1, 70, 71):
                bad[r, c] = True
        for r, c in ((0, 9), (1, 62), (79, 12), (78, 22), (5, 0), (12, 1), (9, 70), (62, 71)):
            bad[r, c] = True
        assert ic.classes(bad) == set(range(25))
    elif name == "d":
        _sprinkle(bad, 0.01, seed=12)
        bad[0:5, :] = True
        bad[14:22, :] = True
        bad[23:31, :] = True                            # row 22 lies between two bands
        bad[43:48, :] = True
        bad[22, 7] = bad[22, 40] = True
        assert not bad[22].all()
    elif name == "e":
        bad[9:20, :] = True
        bad[:, 40:52] = True
        bad[3, 5] = bad[28, 60] = True
    elif name == "f":
        _sprinkle(bad, 0.08, seed=13)
        bad[:2, :2] = bad[-2:, -2:] = True
        assert not bad.all(axis=0).any() and not bad.all(axis=1).any()
    elif name == "g":
        bad[3, :] = True
        bad[:, 1] = True
    else:
        raise KeyError(name)
    return bad


@functools.lru_cache(maxsize=None)
def case(name):
    """(image with NaN under the mask, mask) of case ``name``; the arrays are shared and read-only."""
    bad = mask(name)
    dyn = np.where(bad, np.nan, ic.image(*bad.shape, seed=20 + NAMES.index(name)))
    dyn.setflags(write=False)
    bad.setflags(write=False)
    return dyn, bad


def band_observation():
    """An unmasked 40 x 36 image with spikes for zap() to flag and a band of 12 dead (zero) channels: (array, spikes).  Two spikes
    lie within two pixels of the band (coupled to it: the preconditioner is then not the inverse and steps are needed)."""
    dyn = ic.image(40, 36, seed=31)
    spikes = ((3, 4), (0, 0), (39, 7), (27, 35), (12, 10), (1, 30))
    for k, (i, j) in enumerate(spikes):
        dyn[i, j] = 40.0 + 7.0 * k
    dyn[14:26, :] = 0.0
    return dyn, spikes
