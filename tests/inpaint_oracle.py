"""Host oracle of the biharmonic fill (Dynspec.inpaint, scintools_amd.clean.biharmonic_fill_device): the linear system of
scikit-image's ``inpaint_biharmonic`` (split_into_regions=False), assembled with scipy.ndimage.laplace and scipy.sparse exactly by
the rule of its ``_get_neigh_coef`` and solved directly.  scikit-image itself is not needed.

For a pixel p: a zero array over p's radius-2 neighbourhood clipped to the image, 1 at p, ``laplace(laplace(.))`` (default
mode='reflect').  That is column p of L @ L, L the 5-point Laplacian with reflecting edges, and, L being symmetric, row p too.
With m the masked and k the known pixels the fill solves A u_m = b, A = (L L)_mm, b = -(L L)_mk u_k."""
import numpy as np
import scipy.sparse as sp
from scipy.ndimage import laplace
from scipy.sparse.linalg import spsolve


def stencil(shape, r, c):
    """(r0, c0, coefficients): the stencil of pixel (r, c) over rows r0.. and columns c0.. of an image of ``shape``."""
    nf, nt = shape
    r0, r1, c0, c1 = max(r - 2, 0), min(r + 3, nf), max(c - 2, 0), min(c + 3, nt)
    delta = np.zeros((r1 - r0, c1 - c0))
    delta[r - r0, c - c0] = 1.0
    return r0, c0, laplace(laplace(delta))


def rows(shape, bad):
    """The rows of L @ L that belong to the masked pixels (row-major order): sparse [nmask][nf nt]."""
    nf, nt = shape
    pix = np.flatnonzero(bad.ravel())
    ii, jj, vv = [], [], []
    for i, p in enumerate(pix):
        r0, c0, st = stencil(shape, p // nt, p % nt)
        rr, cc = np.nonzero(st)
        ii.append(np.full(rr.size, i))
        jj.append((r0 + rr) * nt + c0 + cc)
        vv.append(st[rr, cc])
    return sp.csr_matrix((np.concatenate(vv), (np.concatenate(ii), np.concatenate(jj))), shape=(pix.size, nf * nt))


def system(dyn, bad):
    """(A, b) of the fill: A sparse [nmask][nmask], b [nmask]; the pixels of ``dyn`` under the mask are not read."""
    m = rows(dyn.shape, bad)
    flat = bad.ravel()
    known = np.where(flat, 0.0, dyn.ravel())
    return m[:, np.flatnonzero(flat)].tocsc(), -(m @ known)


def fill(dyn, bad, return_system=False):
    """``dyn`` with the pixels of ``bad`` replaced by the direct solution."""
    a, b = system(dyn, bad)
    u = np.atleast_1d(spsolve(a, b))
    out = np.array(dyn, dtype=float)
    out[bad] = u
    return (out, a, b) if return_system else out


def residual(a, b, u):
    """The true relative residual |b - A u|_2 / |b|_2."""
    return float(np.linalg.norm(b - a @ u) / np.linalg.norm(b))
