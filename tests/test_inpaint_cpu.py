"""The biharmonic fill without a GPU: properties of the host oracle (tests/inpaint_oracle.py: scipy.ndimage.laplace, scipy.sparse,
spsolve -- no scikit-image), the test cases' records, and the host-made stencil table of scintools_amd.clean against the oracle."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import inpaint_cases as ic  # noqa: E402
import inpaint_oracle as io  # noqa: E402

EPS = np.finfo(float).eps


def test_a_constant_image_is_reproduced_exactly():
    """Every row of L L sums to zero exactly (integer coefficients), so b = A 1 c and the direct solve returns c."""
    _, bad = ic.case("a")
    for c in (1.0, 3.0, -0.625):
        out = io.fill(np.where(bad, np.nan, c), bad)
        assert np.abs(out - c).max() <= 64 * EPS * abs(c)
    m = io.rows(bad.shape, bad)
    assert np.array_equal(np.asarray(m.sum(axis=1)).ravel(), np.zeros(m.shape[0]))


def test_a_cubic_is_reproduced_away_from_the_edges():
    """L of a polynomial of degree <= 3 is linear, L of that is zero wherever both stencils stay inside the image: with every masked
    pixel at least 2 pixels from every edge the cubic itself solves the system, and the solution is unique."""
    nf, nt = 24, 20
    rng = np.random.default_rng(8)
    bad = np.zeros((nf, nt), bool)
    bad[2:-2, 2:-2] = rng.random((nf - 4, nt - 4)) < 0.15
    bad[9, 2:-2] = True
    bad[12:16, 5:9] = True
    f, t = np.meshgrid(np.arange(nf, dtype=float), np.arange(nt, dtype=float), indexing="ij")
    coef = rng.standard_normal(10)
    terms = [np.ones_like(f), f, t, f * f, f * t, t * t, f ** 3, f * f * t, f * t * t, t ** 3]
    cubic = sum(c * m for c, m in zip(coef, terms))
    out, a, b = io.fill(np.where(bad, np.nan, cubic), bad, return_system=True)
    kappa = np.linalg.cond(a.toarray())
    err = np.abs(out - cubic).max() / np.abs(cubic).max()
    print(f"cubic: error {err:.3g}, kappa {kappa:.3g}")
    assert err <= 16 * EPS * kappa


@pytest.mark.parametrize("name", ic.NAMES)
def test_the_matrix_is_symmetric_positive_definite_and_kappa_is_recorded(name):
    dyn, bad = ic.case(name)
    a = io.system(dyn, bad)[0].toarray()
    assert np.array_equal(a, a.T)
    w = np.linalg.eigvalsh(a)
    kappa = w[-1] / w[0]
    print(f"case {name}: {a.shape[0]} unknowns, eigenvalues {w[0]:.4g} .. {w[-1]:.4g}, kappa {kappa:.5g}")
    assert w[0] > 0.0
    assert kappa <= ic.KAPPA[name] <= 1.001 * kappa + 1e-3
    assert ic.KAPPA[name] < ic.KAPPA_LIMIT


def test_cases_reach_every_class_and_several_workgroups():
    for name in ("a", "b"):
        assert ic.classes(ic.case(name)[1]) == set(range(25))
    assert ic.case("b")[1].sum() > 3 * 256 and ic.case("b")[1].size > 4 * 1024


def test_the_host_table_holds_the_oracles_stencils():
    """Every pixel of a 7 x 6 image: the oracle's stencil (the rule of scikit-image's _get_neigh_coef) equals the table entry of
    the pixel's class, cropped to the image."""
    from scintools_amd import clean
    table = clean.stencil_table()
    assert table.shape == (25, 5, 5)
    nf, nt = 7, 6
    seen = set()
    for r in range(nf):
        for c in range(nt):
            k = 5 * ic.stencil_class(r, nf) + ic.stencil_class(c, nt)
            seen.add(k)
            r0, c0, st = io.stencil((nf, nt), r, c)
            full = np.zeros((5, 5))
            full[r0 - (r - 2):r0 - (r - 2) + st.shape[0], c0 - (c - 2):c0 - (c - 2) + st.shape[1]] = st
            assert np.array_equal(full, table[k]), (r, c)
    assert seen == set(range(25))
    assert np.array_equal(table[12], [[0, 0, 1, 0, 0], [0, 2, -8, 2, 0], [1, -8, 20, -8, 1], [0, 2, -8, 2, 0], [0, 0, 1, 0, 0]])
    assert np.array_equal(table[0][2:, 2:], [[6, -5, 1], [-5, 2, 0], [1, 0, 0]])
    assert np.array_equal(table[5 + 2][:, 2], [0, -7, 20, -8, 1])        # one row below the top edge: the centre column


def test_host_side_refusals_need_no_gpu():
    from scintools_amd import clean
    with pytest.raises(ValueError, match="every pixel is masked"):
        clean.biharmonic_fill_device(np.full((6, 6), np.nan))
    x = np.ones((4, 9))
    x[1, 1] = np.nan
    with pytest.raises(ValueError, match="5 x 5"):
        clean.biharmonic_fill_device(x)
    y = np.ones((6, 6))
    out = clean.biharmonic_fill_device(y)
    assert out is not y and np.array_equal(out, y)
    assert clean.INPAINT_TOL == clean.SVD_TOL


def test_entry_points_are_exported():
    from scintools_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "scint_inpaint_biharmonic") and hasattr(lib, "scint_inpaint_biharmonic_workspace_bytes")
    import ctypes
    need = ctypes.c_size_t()
    _lib.call("scint_inpaint_biharmonic_workspace_bytes", 1024, 1024, 18000, need)
    assert 4 * 1024 * 1024 + 52 * 18000 <= need.value <= 4 * 1024 * 1024 + 52 * 18000 + 32 * 1024
