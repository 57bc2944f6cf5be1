"""The mathematics of the line-block preconditioner of the biharmonic fill (``precond='lines'``) in NumPy, without a
GPU: the restatement of tests/inpaint_lines_oracle.py against the matrix of tests/inpaint_oracle.py, and the records of
tests/inpaint_lines_cases.py and tests/golden/inpaint_lines_tolerances.json."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import inpaint_lines_cases as lc  # noqa: E402
import inpaint_lines_checks as ck  # noqa: E402
import inpaint_lines_oracle as lo  # noqa: E402
import inpaint_oracle as io  # noqa: E402


@pytest.mark.parametrize("n", (5, 7, 16, 40))
def test_the_dct_diagonalises_the_second_difference(n):
    t, c, cinv = lo.neumann(n), lo.dct_matrix(n), lo.dct_inverse_matrix(n)
    assert np.abs(c @ cinv - np.eye(n)).max() <= 1e-14
    assert np.abs(c @ t @ cinv - np.diag(lo.eigenvalues(n))).max() <= 1e-13


def test_the_laplacian_is_the_kronecker_sum():
    """The rows of the oracle's L^2 are those of (L_f (x) I + I (x) L_t)^2."""
    nf, nt = 7, 6
    lap = np.kron(lo.neumann(nf), np.eye(nt)) + np.kron(np.eye(nf), lo.neumann(nt))
    rows = io.rows((nf, nt), np.ones((nf, nt), bool)).toarray()
    assert np.abs(rows - lap @ lap).max() <= 1e-12


@pytest.mark.parametrize("name", ("a", "b", "d", "g"))
def test_mode_blocks_are_the_dense_block(name):
    """DCT x identity takes the block of L^2 on the whole lines to the per-mode blocks, and those are the five bands."""
    dyn, bad = lc.case(name)
    a = io.system(dyn, bad)[0].toarray()
    pre = lo.Preconditioner(bad, np.diag(a))
    nf, nt = bad.shape
    for lines, blocks, n_across, n, index in ((pre.channels, pre.blocks_f, nf, nt, pre.index[pre.channels, :]),
                                              (pre.subints, pre.blocks_t, nt, nf, pre.index[:, pre.subints].T)):
        if not lines.size:
            continue
        block = a[np.ix_(index.ravel(), index.ravel())].reshape(lines.size, n, lines.size, n)     # [w][j][w'][j']
        c, cinv = lo.dct_matrix(n), lo.dct_inverse_matrix(n)
        hat = np.einsum("kj,wjvi,il->wkvl", c, block, cinv)
        for k in range(n):
            assert np.abs(hat[:, k, :, k] - blocks[k]).max() <= 1e-11
        off = hat.copy()
        for k in range(n):
            off[:, k, :, k] = 0.0
        assert np.abs(off).max() <= 1e-11, "the modes do not decouple"
        a0, b0, a1, b1, a2 = lo.bands(lines, n_across)
        for k, lam in enumerate(lo.eigenvalues(n)):
            m = np.diag(a0 + lam * b0 + lam * lam)
            for d, v in ((1, (a1 + lam * b1)[:-1]), (2, a2[:-2])):
                if lines.size > d:
                    m += np.diag(v, d) + np.diag(v, -d)
            assert np.abs(m - blocks[k]).max() <= 1e-12
            assert np.linalg.eigvalsh(blocks[k])[0] > 0.0


@pytest.mark.parametrize("name", ("d", "e", "f", "g"))
def test_the_preconditioner_is_symmetric_positive_definite(name):
    dyn, bad = lc.case(name)
    a = io.system(dyn, bad)[0]
    m = lo.Preconditioner(bad, a.diagonal()).dense()
    assert np.abs(m - m.T).max() <= 1e-12 * np.abs(m).max()
    assert np.linalg.eigvalsh(0.5 * (m + m.T))[0] > 0.0


@pytest.mark.parametrize("name", lc.NAMES)
def test_restated_pcg_reaches_the_direct_solve(name):
    dyn, bad = lc.case(name)
    ref, a, b, rho_ref = ck.reference(name)
    x, steps, res = lo.pcg(a, b, lo.Preconditioner(bad, a.diagonal()))
    err = np.linalg.norm(x - ref[bad]) / np.linalg.norm(ref[bad])
    print(f"restated pcg {name}: {steps} steps, residual {res:.3g}, error {err:.3g}, rho_ref {rho_ref:.3g}")
    assert res <= 1e-12 and err <= lc.KAPPA[name] * (res + rho_ref)
    assert lc.KAPPA[name] * rho_ref <= lc.RHO_REF_LIMIT
    assert steps == ck.recorded()[name]["pcg_steps"]
    if name in lc.DIRECT:
        assert steps == 0, "whole lines along one axis: x0 = M^-1 b is the solution"
    if name in lc.ITERATED:
        assert steps >= 1


@pytest.mark.parametrize("name", lc.NAMES)
def test_the_recorded_condition_numbers(name):
    dyn, bad = lc.case(name)
    ev = np.linalg.eigvalsh(io.system(dyn, bad)[0].toarray())
    kappa = ev[-1] / ev[0]
    assert kappa <= lc.KAPPA[name] <= 1.001 * kappa
    assert abs(ck.recorded()[name]["kappa"] / kappa - 1.0) <= 1e-6


def test_the_record_says_what_the_preconditioner_buys():
    rec = ck.recorded()
    for name in ("a", "b", "c"):
        assert rec[name]["cg_outcome"] == "NOCONV" and rec[name]["cg_steps"] == 2000 and rec[name]["cg_residual"] > 1e-12
    assert all(rec[name]["pcg_steps"] < rec[name]["cg_steps"] for name in lc.NAMES)


def test_keyword_is_checked_before_the_device():
    from scintools_amd import clean
    with pytest.raises(ValueError, match="precond"):
        clean.biharmonic_fill_device(np.ones((6, 6)), precond="jacobi")
    assert clean.lines_length_ok(5) and clean.lines_length_ok(4096) and clean.lines_length_ok(8192)
    assert not clean.lines_length_ok(4) and not clean.lines_length_ok(4097)
