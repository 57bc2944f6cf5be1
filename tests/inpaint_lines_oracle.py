"""NumPy restatement of the line-block preconditioner of the biharmonic fill (``precond='lines'``, csrc/inpaint.hpp) and
of the preconditioned conjugate gradients around it.  The matrix is the one of tests/inpaint_oracle.py.

L = L_f (x) I + I (x) L_t, L_n the (1, -2, 1) matrix of size n with corner entries -1.  Its eigenvectors are the DCT-II basis
cos(pi k (j + 1/2) / n) with eigenvalues 2 cos(pi k / n) - 2.  For the set W_f of channels whose every pixel is masked the block
of L^2 on W_f x (all times) decouples, after a DCT along time, into one matrix ((L_f + lam_k I)^2)[W_f, W_f] per time mode k: a
principal submatrix of a pentadiagonal matrix, so pentadiagonal in the compressed numbering too.  The same with the axes
exchanged for the set W_t of whole sub-integrations.  The preconditioner is

    M^-1 r = R_f^T A_ff^-1 R_f r + R_t^T A_tt^-1 R_t r + D^-1 r_rest,

r_rest the part of r on masked pixels in no whole line, D the diagonal of A there.  Unknowns are numbered in pixel order."""
import numpy as np


def neumann(n):
    """The second difference of n points with reflecting ends."""
    t = -2.0 * np.eye(n) + np.eye(n, k=1) + np.eye(n, k=-1)
    t[0, 0] = t[-1, -1] = -1.0
    return t


def eigenvalues(n):
    return 2.0 * np.cos(np.pi * np.arange(n) / n) - 2.0


def dct_matrix(n):
    """C[k][j] = cos(pi k (j + 1/2) / n): X = C x is the (unnormalised) DCT-II, x = C^-1 X with C^-1 = (2 / n) C^T, its column 0
    halved."""
    k, j = np.arange(n)[:, None], np.arange(n)[None, :]
    return np.cos(np.pi * k * (j + 0.5) / n)


def dct_inverse_matrix(n):
    inv = (2.0 / n) * dct_matrix(n).T
    inv[:, 0] *= 0.5
    return inv


def whole_lines(bad):
    """(channels, sub-integrations) whose every pixel is masked."""
    return np.flatnonzero(bad.all(axis=1)), np.flatnonzero(bad.all(axis=0))


def mode_blocks(lines, n_across, n_along):
    """[n_along][len(lines)][len(lines)]: ((L + lam_k I)^2)[lines, lines] for every mode k of the axis of n_along points, L the
    second difference of the axis of n_across points that ``lines`` number."""
    t = neumann(n_across)
    out = np.empty((n_along, lines.size, lines.size))
    for k, lam in enumerate(eigenvalues(n_along)):
        s = t + lam * np.eye(n_across)
        out[k] = (s @ s)[np.ix_(lines, lines)]
    return out


def bands(lines, n_across):
    """The pentadiagonal blocks as five vectors over the compressed lines: entry (i, i + d) of mode k is
    a[d][i] + lam_k b[d][i] (+ lam_k^2 for d = 0).  Returns (a0, b0, a1, b1, a2): what the device's factorisation reads."""
    t = neumann(n_across)
    t2 = t @ t
    m = lines.size
    a0, b0 = t2[lines, lines], 2.0 * t[lines, lines]
    a1, b1, a2 = np.zeros(m), np.zeros(m), np.zeros(m)
    for d, (a, b) in ((1, (a1, b1)), (2, (a2, None))):
        for i in range(m - d):
            if lines[i + d] - lines[i] <= 2:
                a[i] = t2[lines[i], lines[i + d]]
                if b is not None:
                    b[i] = 2.0 * t[lines[i], lines[i + d]]
    return a0, b0, a1, b1, a2


class Preconditioner:
    def __init__(self, bad, diagonal):
        """``diagonal``: the diagonal of A (the centre coefficient of every unknown's stencil), in pixel order."""
        self.bad = np.asarray(bad, dtype=bool)
        nf, nt = self.bad.shape
        self.channels, self.subints = whole_lines(self.bad)
        self.index = np.full(self.bad.shape, -1)
        self.index[self.bad] = np.arange(int(self.bad.sum()))
        self.blocks_f = mode_blocks(self.channels, nf, nt)      # [nt][|W_f|][|W_f|]
        self.blocks_t = mode_blocks(self.subints, nt, nf)       # [nf][|W_t|][|W_t|]
        self.ct, self.ct_inv = dct_matrix(nt), dct_inverse_matrix(nt)
        self.cf, self.cf_inv = dct_matrix(nf), dct_inverse_matrix(nf)
        rest = self.bad.copy()
        rest[self.channels, :] = False
        rest[:, self.subints] = False
        self.rest = self.index[rest]
        self.diagonal = np.asarray(diagonal, dtype=float)

    def __call__(self, r):
        z = np.zeros_like(r)
        if self.channels.size:
            idx = self.index[self.channels, :]                  # [|W_f|][nt]
            rhat = r[idx] @ self.ct.T                           # DCT along time: [w][k]
            sol = np.linalg.solve(self.blocks_f, rhat.T[:, :, None])[:, :, 0].T
            np.add.at(z, idx, sol @ self.ct_inv.T)
        if self.subints.size:
            idx = self.index[:, self.subints].T                 # [|W_t|][nf]
            rhat = r[idx] @ self.cf.T
            sol = np.linalg.solve(self.blocks_t, rhat.T[:, :, None])[:, :, 0].T
            np.add.at(z, idx, sol @ self.cf_inv.T)
        z[self.rest] = r[self.rest] / self.diagonal[self.rest]
        return z

    def dense(self):
        n = self.diagonal.size
        return np.stack([self(e) for e in np.eye(n)], axis=1)


def pcg(a, b, apply, tol=1e-12, max_iter=2000):
    """Preconditioned conjugate gradients from x0 = M^-1 b, stopped by the true residual |b - A x| <= tol |b| (formed when the
    recurrence's residual passes, as the device does).  Returns (x, steps, true relative residual); steps = 0: x0 was enough."""
    bnorm = np.linalg.norm(b)
    x = apply(b)
    r = b - a @ x
    steps = 0
    while np.linalg.norm(r) > tol * bnorm and steps < max_iter:
        z = apply(r)
        p = z.copy()
        rz = r @ z
        while steps < max_iter:
            steps += 1
            q = a @ p
            alpha = rz / (p @ q)
            x = x + alpha * p
            r = r - alpha * q
            if np.linalg.norm(r) <= tol * bnorm:
                break
            z = apply(r)
            rz, rz_old = r @ z, rz
            p = z + (rz / rz_old) * p
        r = b - a @ x
    return x, steps, float(np.linalg.norm(r) / bnorm)


def cg(a, b, tol=1e-12, max_iter=2000):
    """Plain conjugate gradients from zero (the default route), the same stopping rule."""
    bnorm = np.linalg.norm(b)
    x = np.zeros_like(b)
    r = b.copy()
    steps = 0
    while np.linalg.norm(r) > tol * bnorm and steps < max_iter:
        p = r.copy()
        rr = r @ r
        while steps < max_iter:
            steps += 1
            q = a @ p
            alpha = rr / (p @ q)
            x = x + alpha * p
            r = r - alpha * q
            rr, rr_old = r @ r, rr
            if np.sqrt(rr) <= tol * bnorm:
                break
            p = r + (rr / rr_old) * p
        r = b - a @ x
    return x, steps, float(np.linalg.norm(r) / bnorm)
