"""Inputs and case list for the theta-theta eigen sweep across every class of the packed Hermitian mat-vec (csrc/eigen_packed.hip,
csrc/packed.hpp, the packed gather of thth.hip), shared by tests/test_gpu_sweep_classes.py (every case, on an MI355X) and
tests/test_sweep_classes_emu_cpu.py (the cases the host interpreter can afford, and the conditions on the inputs).  The reference
for every value is oracle/thth_oracle.thth_redmap followed by dense LAPACK.  Nothing here needs a GPU.

What a mat-vec workgroup does depends on nb = ceil(N / 64) alone.  The rule, restated from packed.hpp (strip_len_for,
row_strip_count, kRows64 = kRows32 = 8, kMaxStrip = kMaxStrip32 = 12):
  strip length S(nb) = 1, 2, 4, 12 column tiles for nb < 4, < 8, < 16, >= 16;
  block rows I, I + 1 .. I + 7 (I a multiple of 8) form one group; a short last group runs with the rows it has;
  a group is cut on its FIRST row's column grid: strips J0 = I, I + S, ..., each one workgroup; row I + r starts at max(J0, I + r);
  the last tile has N mod 64 live rows (64 when N is a multiple of 64), the rest is zero.
`workgroups(nb)` counts the strips this rule gives; `assert_build_constants` compares it with the loaded library's
scint_sweep_workgroups for both element types, so a changed build constant fails the coverage claim instead of shrinking it.

The matrix is one in which every tile matters: the conjugate spectrum (npad = 1) of 256 x 256 Gaussian noise plus a weak separable
cosine term (amplitude 0.5: enough to open the spectral gap, too little to concentrate the eigenvector), gathered on a theta grid
of N centres inside +-fd_max / 2 -- up to six times denser than the Doppler grid -- at a curvature that keeps every centre
(eta theta_max^2 = 0.9 tau_max), so that N = len(edges) - 1.  Symmetric edges need an even number of them (an odd number makes two
centres tie for the smallest |theta|), hence odd N; even N comes from a lopsided linspace.  The conditions these inputs have to
meet (tile sensitivity, spectral gap) are checked in tests/test_sweep_classes_emu_cpu.py from the oracle and LAPACK alone.

N = 1 (nb = 1, 'one live row in the last tile') has no eigenproblem: the reduced map is the 1 x 1 zero matrix, the reference's
thth_redmap raises on it (no reduced edges from one centre) and the sweep reports the crop as empty.  It stays in the list as a
case of its own kind (DEGENERATE): the checks assert that documented outcome for it instead of an eigenvalue."""
import functools

import numpy as np

from oracle import thth_oracle as to

TILE = 64
ROWS = 8                        # kRows64 = kRows32: block rows per mat-vec workgroup
MAX_STRIP = 12                  # kMaxStrip = kMaxStrip32
MAX_ITER = 300                  # ththmod.DEFAULT_MAX_ITER (asserted by the tests)
TOL = 1e-12                     # ththmod.DEFAULT_TOL

NS = 256                        # the dynamic spectrum is NS x NS, its conjugate spectrum 2 NS x 2 NS
NPAD = 1
SEED = 2
COHERENT = 0.5                  # amplitude of the separable cosine term, in units of the noise's standard deviation
ETA_FILL = 0.9                  # eta theta_max^2 / tau_max of the class cases: below the crop
LOPSIDED = 0.97                 # upper end of the lopsided edges, in units of fd_max / 2

# nb: why it is in the list
CLASS_NB = {1: "one tile", 3: "last nb with strips of one tile", 4: "first nb with strips of two", 7: "last nb with strips of two",
            8: "strips of four, one full row group", 9: "last group of one row", 12: "two groups, the second of four rows",
            13: "a first group of four strips, a last group of five rows", 15: "last group of seven rows",
            16: "strips of twelve: groups of two strips (16 tiles) and one (8 tiles)",
            17: "last group of one row behind a two-strip group", 19: "the production fit's nb",
            24: "first group exactly two strips", 25: "first group three strips, second two, third one row"}
FULL_TILE_NB = (1, 8, 17, 25)   # nb that also run N = 64 nb (no padding row)


def sizes():
    """Every N of the class cases: 64 (nb - 1) + 1 and 64 nb - 1 for every nb, 64 nb for FULL_TILE_NB."""
    out = []
    for nb in CLASS_NB:
        out += [TILE * (nb - 1) + 1, TILE * nb - 1]
        if nb in FULL_TILE_NB:
            out.append(TILE * nb)
    return out


DEGENERATE = (1,)               # see the module docstring
SIZES = tuple(sizes())
assert len(SIZES) == 14 * 2 + 4 and len(set(SIZES)) == len(SIZES)


def nb_of(n):
    return -(-n // TILE)


def strip_len(nb):
    return MAX_STRIP if nb >= 16 else (4 if nb >= 8 else (2 if nb >= 4 else 1))


def group_strips(nb):
    """[(first block row, rows, strips)] of every row group."""
    s = strip_len(nb)
    return [(i, min(ROWS, nb - i), -(-(nb - i) // s)) for i in range(0, nb, ROWS)]


def workgroups(nb):
    return sum(g[2] for g in group_strips(nb))


# the structure the table of cases claims, from the rule above
assert [strip_len(nb) for nb in CLASS_NB] == [1, 1, 2, 2, 4, 4, 4, 4, 4, 12, 12, 12, 12, 12]
assert group_strips(9) == [(0, 8, 3), (8, 1, 1)] and group_strips(15)[-1] == (8, 7, 2)
assert group_strips(13) == [(0, 8, 4), (8, 5, 2)]
assert group_strips(16) == [(0, 8, 2), (8, 8, 1)] and group_strips(17) == [(0, 8, 2), (8, 8, 1), (16, 1, 1)]
assert group_strips(19)[-1] == (16, 3, 1) and group_strips(24) == [(0, 8, 2), (8, 8, 2), (16, 8, 1)]
assert group_strips(25) == [(0, 8, 3), (8, 8, 2), (16, 8, 1), (24, 1, 1)]


def assert_build_constants(lib):
    """The loaded library (GPU build or host interpreter) cuts every nb of the list, and every nb the mixed-size calls pass
    through, into the workgroups the rule gives, for the complex128 and the complex64 strips."""
    for nb in sorted(set(CLASS_NB) | set(range(1, 26))):
        for c64 in (0, 1):
            got = int(lib.scint_sweep_workgroups(nb, c64))
            assert got == workgroups(nb), f"nb={nb} complex64={c64}: library {got} workgroups, rule {workgroups(nb)}"


# tiles whose first-order weight is structurally tiny: the last block column of the N = 1 (mod 64) cases holds ONE live row
# (its diagonal tile is the 1 x 1 zero block)
ONE_ROW_TILES = {n: tuple((i, nb_of(n) - 1) for i in range(nb_of(n))) for n in SIZES if n % TILE == 1 and n > 1}
assert ONE_ROW_TILES[129] == ((0, 2), (1, 2), (2, 2)) and len(ONE_ROW_TILES) == 13


@functools.lru_cache(maxsize=None)
def axes():
    """(tau, fd) of the padded conjugate spectrum."""
    tau = to.fft_axis(1400.0 + 0.1 * np.arange(NS), 1.0, NPAD)
    fd = to.fft_axis(30.0 * np.arange(NS), 1000.0, NPAD)
    for a in (tau, fd):
        a.setflags(write=False)
    return tau, fd


@functools.lru_cache(maxsize=None)
def spectrum(seed=SEED, coherent=COHERENT):
    """Conjugate spectrum [2 NS, 2 NS] of noise plus `coherent` x a separable cosine term (read-only)."""
    rng = np.random.default_rng(seed)
    dyn = rng.standard_normal((NS, NS)) + coherent * np.outer(np.cos(0.3 * np.arange(NS)), np.cos(0.2 * np.arange(NS)))
    CS = to.conjugate_spectrum(dyn - dyn.mean(), NPAD)
    CS.setflags(write=False)
    return CS


def eta_fill(scale=1.0):
    """The curvature with eta theta_max^2 = ETA_FILL tau_max on edges that end at scale fd_max / 2."""
    tau, fd = axes()
    return ETA_FILL * tau.max() / (scale * fd.max() / 2) ** 2


def edges_for(n, scale=1.0):
    """n + 1 edges inside +-scale fd_max / 2 whose n centres all survive the crop at eta_fill(scale)."""
    a = scale * axes()[1].max() / 2
    return np.linspace(-a, a if n % 2 else LOPSIDED * a, n + 1)


def case(n):
    """dict(CS, tau, fd, eta, edges) of the class case with N = n."""
    tau, fd = axes()
    return dict(CS=np.array(spectrum()), tau=tau, fd=fd, eta=eta_fill(), edges=edges_for(n))


@functools.lru_cache(maxsize=None)
def matrix(n):
    """The oracle's reduced theta-theta of case n (read-only, computed once)."""
    c = case(n)
    red = to.thth_redmap(c["CS"], c["tau"], c["fd"], c["eta"], c["edges"])[0]
    assert red.shape == (n, n), (red.shape, n)
    red.setflags(write=False)
    return red


@functools.lru_cache(maxsize=None)
def lapack_top(n):
    """LAPACK's largest algebraic eigenvalue of matrix(n)."""
    return float(np.linalg.eigvalsh(matrix(n))[-1])


# ---- several nb in one call ------------------------------------------------------------------------------------------------
MIXED_BATCH = 3
# kept sizes aimed at by the curvatures of the one-call check, on a grid of 1087 / 575 centres (GPU / host interpreter): at
# least twelve, every strip-length class the grid reaches
MIXED_TARGETS = {1087: (1087, 1020, 950, 820, 760, 570, 500, 440, 250, 180, 130, 100),
                 575: (575, 501, 441, 381, 301, 251, 190, 180, 150, 130, 110, 100)}


def mixed_case(full):
    """dict(CS, tau, fd, edges, etas): symmetric edges with `full` centres and one curvature per entry of MIXED_TARGETS[full],
    descending in N: the first keeps everything, curvature k crops to about the k-th target (theta^2 eta < tau_max)."""
    tau, fd = axes()
    edges = edges_for(full)
    th = to.theta_centres(edges)
    etas = [eta_fill()]
    for n in MIXED_TARGETS[full][1:]:
        bound = 0.5 * (th[full // 2 + n // 2] + th[full // 2 + n // 2 + 1])       # between the last kept centre and the next
        etas.append(tau.max() / bound ** 2)
    return dict(CS=np.array(spectrum()), tau=tau, fd=fd, edges=edges, etas=np.array(etas))


@functools.lru_cache(maxsize=None)
def mixed_reference(full):
    """(N[k], lambda_1[k]) of every curvature of mixed_case(full), from the oracle and LAPACK."""
    c = mixed_case(full)
    n, lam = [], []
    for e in c["etas"]:
        red = to.thth_redmap(c["CS"], c["tau"], c["fd"], e, c["edges"])[0]
        n.append(red.shape[0])
        lam.append(float(np.linalg.eigvalsh(red)[-1]))
    return np.array(n), np.array(lam)


# ---- a stack of spectra --------------------------------------------------------------------------------------------------------
STACK_CENTRES = 1087
STACK = ((2, 1.0, 1087), (3, 0.96, 620), (4, 0.92, 300))        # (seed, edge scale, kept size aimed at): strips of 12, 4 and 2


def stack_case():
    """(stack [3, 2 NS, 2 NS], grids [(tau, fd, edges)], etas [array of two]): three spectra with their own theta grids (one
    edge count, as eval_sweep_multi requires) and two curvatures each, whose crops fall in three strip-length classes."""
    tau, fd = axes()
    stack, grids, etas = [], [], []
    for seed, scale, n in STACK:
        edges = edges_for(STACK_CENTRES, scale)
        th = to.theta_centres(edges)
        if n == STACK_CENTRES:
            e = eta_fill(scale)
        else:
            e = tau.max() / (0.5 * (th[STACK_CENTRES // 2 + n // 2] + th[STACK_CENTRES // 2 + n // 2 + 1])) ** 2
        stack.append(spectrum(seed))
        grids.append((tau, fd, edges))
        etas.append(np.array([e, 1.07 * e]))
    return np.stack(stack), grids, etas
