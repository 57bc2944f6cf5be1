"""Seeded stacks of small dynamic spectra for the batched ACF (scint_acf_batch, scintpar.acf_stack_device); the checks are
tests/acf_batch_checks.py.  Every case is [B, nf, nt] with what it could break:

  one        [1, 4, 8]     the batch of one against the single call
  odd        [3, 5, 7]     odd lengths: 2 nf = 10 and 2 nt = 14 take the any-length (chirp-z) route on both axes
  pow2       [5, 16, 16]   the power-of-two route (two real rows per transform, half the columns)
  b37        [37, 8, 16]   a B that is no multiple of any grouping or wavefront count
  mixed      [9, 6, 32]    any-length along the strided axis, a power of two along the contiguous one
  groups     [12, 8, 8]    taken in groups of 5, 5 and 2 (GROUPS): a later group must not read the workspace of an earlier one
  leak       [6, 8, 16]    problem 2 is constant, problem 4 has a mean 10^6 times its scatter: a problem's mean and maximum stay its own
  onerow     [3, 1, 8]     one row per problem: the row pass pairs real rows, and a problem's only row has no partner -- the next
                           problem's first row must not become it
  longrow    [2, 2, 8192]  2 nt = 16384: the decimated row transform (rows beyond the in-LDS limit), pairs formed per problem

The last two are not in the list the batched ACF was specified with; they are the two places where the stacked row pass decodes
the problem differently from the single call."""
import numpy as np

SHAPES = {
    "one": (1, 4, 8),
    "odd": (3, 5, 7),
    "pow2": (5, 16, 16),
    "b37": (37, 8, 16),
    "mixed": (9, 6, 32),
    "groups": (12, 8, 8),
    "leak": (6, 8, 16),
    "onerow": (3, 1, 8),
    "longrow": (2, 2, 8192),
}
CASES = tuple(SHAPES)
# The secondary spectra of a stack (dynspec.sspec_stack_device) run on the same stacks where a spectrum exists (nf >= 2, nt >= 5), and on
#   big      [2, 130, 132]  padded half-lengths of 256: the single call's persistent kernels, here problem after problem
SHAPES["big"] = (2, 130, 132)
SSPEC_CASES = ("one", "odd", "pow2", "b37", "mixed", "groups", "leak", "longrow", "big")
GROUPS = {"groups": 5}          # problems per group of the cases that are taken in groups
_cache = {}


def stack(name):
    """The case's stack (built once, then shared: do not write into it): a positive flux with unit mean and 30 % scatter."""
    if name not in _cache:
        rng = np.random.default_rng(1000 + list(SHAPES).index(name))
        x = 1.0 + 0.3 * rng.standard_normal(SHAPES[name])
        if name == "leak":
            x[2] = 0.75
            x[4] = 1e6 + rng.standard_normal(SHAPES[name][1:])
        _cache[name] = np.ascontiguousarray(x)
    return _cache[name]


def numpy_acf(x, subtract_mean, normalise):
    """NumPy's statement of the reference (dynspec.py:3780-3797) for one dynamic spectrum."""
    nf, nt = x.shape
    if subtract_mean:
        x = x - np.mean(x)
    arr = np.fft.fft2(x, s=[2 * nf, 2 * nt])
    arr = np.real(np.fft.fftshift(np.fft.ifft2(np.abs(arr) ** 2)))
    with np.errstate(invalid="ignore", divide="ignore"):
        return arr / np.max(arr) if normalise else arr


def observation():
    """A 64 x 80 zero-mean correlated field as an observation for cut_dyn and the cut fits (the generator of acf1d_cases)."""
    import acf1d_cases
    import scintpar_cases
    nf, nt = 64, 80
    dyn = acf1d_cases.realistic_dyn(np.random.default_rng(77), nf, nt, 2.5, 3.5, 0.1)
    dyn = dyn - dyn.mean()
    DF, DT = acf1d_cases.DF, acf1d_cases.DT
    return scintpar_cases.observation(dyn, 1400.0 + DF * np.arange(nf), DT * np.arange(nt), DF, DT, 1400.0 + DF * nf / 2,
                                      "acf_batch")
