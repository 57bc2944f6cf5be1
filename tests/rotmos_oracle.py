"""NumPy restatement of the reference's fitted mosaics (scintools/ththmod.py:1708-2310), for the tests: the same operations on
the same operands in the same order -- so that the mosaics can be compared bit for bit -- written once around a shared taper and
window helper.  Every sum comes as (value, S, P):

S, the SCALE, is the same sum with each summand replaced by its absolute value; the tests' tolerance for a sum is 1e-13 * S.

P, the PRODUCT SCALE, is the same sum with every product inside a summand replaced by the product of the moduli of its factors
(the differences the reference forms first -- `|W|^2 - dspec`, `E - y exp(i rot)` -- enter as computed).  It is not part of the
tolerance of an ordinary sum.  It serves one degenerate situation only: with tapers of length 1 (the 2 x 2 x 2 x 2 case) every
pixel belongs to one chunk alone, whole summands such as `8 Im(tM) Im(tN) + 4 w Re(conj(yM) yN) - 4 w Re(tN)` cancel to rounding
noise, S itself is of the size of one rounding, and the reference's own Hessian then differs from this restatement of it, on one
host, by 0.1 S (NumPy multiplies contiguous and strided operands in different loops).  Where S has fallen to that level
(S < 1e-6 P: no ordinary sum comes near) the tests add the rounding floor 8 eps P -- a dozen roundings of eps / 2 per summand,
rounded up -- to the tolerance (tests/rotmos_cases.py: close_in_scale)."""
import numpy as np


def _ramp(w):
    x = np.linspace(0, w - 1, w)
    return np.sin((np.pi / 2) * x / w) ** 2


def taper(shape, cf, ct):
    ncf, nct, cwf, cwt = shape
    mask = np.ones((cwf, cwt))
    if cf > 0:
        mask[: cwf // 2, :] *= _ramp(cwf // 2)[:, np.newaxis]
    if cf < ncf - 1:
        mask[cwf // 2:, :] *= 1 - _ramp(cwf // 2)[:, np.newaxis]
    if ct > 0:
        mask[:, : cwt // 2] *= _ramp(cwt // 2)
    if ct < nct - 1:
        mask[:, cwt // 2:] *= 1 - _ramp(cwt // 2)
    return mask


def window(shape, cf, ct):
    _, _, cwf, cwt = shape
    return (slice(cf * cwf // 2, cf * cwf // 2 + cwf), slice(ct * cwt // 2, ct * cwt // 2 + cwt))


def _extent(shape):
    ncf, nct, cwf, cwt = shape
    return ((ncf - 1) * (cwf // 2) + cwf, (nct - 1) * (cwt // 2) + cwt)


def _each(shape):
    for cf in range(shape[0]):
        for ct in range(shape[1]):
            yield cf, ct, cf * shape[1] + ct


def rot_mosaic(chunks, x):
    shape = chunks.shape
    E = np.zeros(_extent(shape), dtype=complex)
    for cf, ct, k in _each(shape):
        rot = x[k - 1] if k > 0 else 0
        E[window(shape, cf, ct)] += np.copy(chunks[cf, ct]) * taper(shape, cf, ct) * np.exp(1j * rot)
    return E


def rot_init(chunks):
    shape = chunks.shape
    E = np.zeros(_extent(shape), dtype=complex)
    x = np.zeros(shape[0] * shape[1] - 1)
    for cf, ct, k in _each(shape):
        new, mask, sl = np.copy(chunks[cf, ct]), taper(shape, cf, ct), window(shape, cf, ct)
        old = E[sl]
        rot = np.angle((old * np.conjugate(new) * mask).mean())
        E[sl] += new * mask * np.exp(1j * rot)
        if k > 0:
            x[k - 1] = rot
    return x


def rot_fit(x, chunks):
    """(value, S, P)"""
    s = np.sum(np.abs(rot_mosaic(chunks, x)) ** 2)
    return -s, s, s


def rot_der(x, chunks):
    """(gradient [n - 1], S, P)"""
    shape = chunks.shape
    E = rot_mosaic(chunks, x)
    g, S, P = np.zeros(x.shape), np.zeros(x.shape), np.zeros(x.shape)
    for cf, ct, k in _each(shape):
        if k == 0:
            continue
        y = np.copy(chunks[cf, ct])
        y *= taper(shape, cf, ct)
        rest = np.copy(E[window(shape, cf, ct)])
        rest -= y * np.exp(1j * x[k - 1])
        terms = 2 * np.imag(np.conjugate(rest) * y * np.exp(1j * x[k - 1]))
        g[k - 1], S[k - 1], P[k - 1] = np.sum(terms), np.sum(np.abs(terms)), np.sum(2 * np.abs(rest) * np.abs(y))
    return g, S, P


def full_mosaic(chunks, p):
    shape = chunks.shape
    n = shape[0] * shape[1]
    E = np.zeros(_extent(shape), dtype=complex)
    for cf, ct, k in _each(shape):
        phi = p[k - 1] if k > 0 else 0
        A = p[k + n - 1]
        E[window(shape, cf, ct)] += A * np.copy(chunks[cf, ct]) * taper(shape, cf, ct) * np.exp(1j * phi)
    return E


def full_fit(p, chunks, dspec, N):
    """(value, S, P): the summands are squares, both scales are the value"""
    M = np.abs(full_mosaic(chunks, p)) ** 2
    v = np.nansum(np.power((M - dspec[: M.shape[0], : M.shape[1]]) / N[: M.shape[0], : M.shape[1]], 2))
    return v, v, v


def full_grad(p, chunks, dspec, N):
    """(gradient [2 n - 1], S, P): the scale of a complex sum's part is the sum of that part's absolute values"""
    shape = chunks.shape
    n = shape[0] * shape[1]
    W = full_mosaic(chunks, p)
    weight = 4 * (np.abs(W) ** 2 - dspec)
    g, S, P = np.zeros(p.shape[0]), np.zeros(p.shape[0]), np.zeros(p.shape[0])
    for cf, ct, k in _each(shape):
        sl = window(shape, cf, ct)
        y = np.copy(chunks[cf, ct])
        y *= taper(shape, cf, ct)
        phi = p[k - 1] if k > 0 else 0
        A = p[k + n - 1]
        terms = weight[sl] * y * np.exp(1j * phi) * np.conjugate(W[sl]) / N[sl] ** 2
        total = np.conjugate(np.nansum(terms))
        keep = ~np.isnan(terms)
        with np.errstate(invalid="ignore", divide="ignore"):
            prod = np.sum((np.abs(weight[sl]) * np.abs(y) * np.abs(W[sl]) / N[sl] ** 2)[keep])
        if k > 0:
            g[k - 1], S[k - 1], P[k - 1] = A * total.imag, abs(A) * np.sum(np.abs(terms.imag[keep])), abs(A) * prod
        g[k + n - 1], S[k + n - 1], P[k + n - 1] = total.real, np.sum(np.abs(terms.real[keep])), prod
    return g, S, P


def _overlap(d, w):
    """(rows of N, rows of M) that chunk N shares with its neighbour M = N + d along an axis of chunk size w"""
    if d == -1:
        return slice(0, w // 2), slice(w // 2, 2 * (w // 2))
    if d == 0:
        return slice(0, w), slice(0, w)
    return slice(w // 2, 2 * (w // 2)), slice(0, w // 2)


def full_hess(p, chunks, dspec, N):
    """(Hessian [2 n - 1, 2 n - 1], S, P)"""
    shape = chunks.shape
    ncf, nct, cwf, cwt = shape
    n = ncf * nct
    W = full_mosaic(chunks, p)
    Ws = np.conjugate(W)
    weight = np.abs(W) ** 2 - dspec
    H, S, P = (np.zeros((p.shape[0], p.shape[0])) for _ in range(3))

    def rotated(cf, ct, k):
        y = np.copy(chunks[cf, ct])
        y *= taper(shape, cf, ct)
        y *= np.exp(1j * (p[k - 1] if k > 0 else 0))
        return y, y * Ws[window(shape, cf, ct)]

    def put(i, j, terms, prod):
        with np.errstate(invalid="ignore", divide="ignore"):
            H[i, j] = H[j, i] = np.sum(terms)
            S[i, j] = S[j, i] = np.sum(np.abs(terms))
            P[i, j] = P[j, i] = np.sum(prod)
    for cfN, ctN, kN in _each(shape):
        wt, ns = weight[window(shape, cfN, ctN)], N[window(shape, cfN, ctN)]
        yN, tN = rotated(cfN, ctN, kN)
        AN, iAN, ipN = p[kN + n - 1], kN + n - 1, kN - 1
        for dt in (-1, 0, 1):
            for df in (-1, 0, 1):
                cfM, ctM = cfN + df, ctN + dt
                if not (0 <= cfM < ncf and 0 <= ctM < nct):
                    continue
                kM = cfM * nct + ctM
                yM, tM = rotated(cfM, ctM, kM)
                AM, iAM, ipM = p[kM + n - 1], kM + n - 1, kM - 1
                (rN, rM), (cN, cM) = _overlap(df, cwf), _overlap(dt, cwt)
                a, b, w, n2 = tM[rM, cM], tN[rN, cN], wt[rN, cN], ns[rN, cN] ** 2
                yy = np.conjugate(yM[rM, cM]) * yN[rN, cN]
                with np.errstate(invalid="ignore", divide="ignore"):
                    ab, wyy, wb = 8 * np.abs(a) * np.abs(b) / n2, 4 * np.abs(w) * np.abs(yM[rM, cM]) * np.abs(yN[rN, cN]) / n2, 4 * np.abs(w) * np.abs(b) / n2
                    put(iAN, iAM, (8 * np.real(a) * np.real(b) + 4 * w * np.real(yy)) / n2, ab + wyy)
                    if kM > 0:
                        t = -8 * AM * np.imag(a) * np.real(b) + 4 * w * AM * np.imag(yy)
                        if kM == kN:
                            t -= 4 * w * np.imag(b)
                        put(iAN, ipM, t / n2, abs(AM) * (ab + wyy) + (wb if kM == kN else 0))
                        if kN > 0:
                            t = 8 * AN * AM * np.imag(a) * np.imag(b) + 4 * AN * AM * w * np.real(yy)
                            if kM == kN:
                                t -= 4 * AN * w * np.real(b)
                            put(ipM, ipN, t / n2, abs(AN * AM) * (ab + wyy) + (abs(AN) * wb if kM == kN else 0))
    return H, S, P
