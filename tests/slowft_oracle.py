"""Two restatements of scint_utils.slow_FT (scint_utils.py:655-703) in NumPy.

slow_ft        float64, the reference's arithmetic channel by channel: the memory is nt * nt, never nt^2 * nf.
slow_ft_ld     np.longdouble, the phase s_j k' t / nt reduced modulo one cycle before the 2 pi: the truth the device is measured
               against (64-bit significand on x86: its own error is about 2^-11 of float64's).
stage1_ld      the first stage alone (natural order of np.fft.fftfreq), for the column check."""
import numpy as np


def fscale(freqs, fref=None):
    freqs = np.asarray(freqs)
    if fref is None:
        fref = freqs[len(freqs) // 2]
    return (freqs / fref).astype('float64')


def slow_ft(dynspec, freqs, fref=None):
    dynspec = np.asarray(dynspec).astype(np.float64)
    ntime, nfreq = dynspec.shape
    src = np.arange(ntime).astype('float64')
    fs = fscale(freqs, fref)
    ft = np.fft.fftfreq(ntime, 1)
    SS = np.empty((ntime, nfreq), dtype=np.complex128)
    for j in range(nfreq):
        tscale = src * fs[j]
        FTphase = -2j * np.pi * tscale[:, np.newaxis] * ft[np.newaxis, :]
        SS[:, j] = np.sum(dynspec[:, j, np.newaxis] * np.exp(FTphase), axis=0)
    SS = np.fft.fftshift(SS, axes=0)
    SS = np.fft.fft(SS, axis=1)
    return np.fft.fftshift(SS, axes=1)


def _kprime(n):
    """Integer frequency index of np.fft.fftfreq(n, 1) * n, natural order."""
    return np.rint(np.fft.fftfreq(n, 1) * n).astype(np.int64)


def _cis_cycles(x):
    """exp(-2 pi i x) for long-double x in cycles, reduced modulo 1 first."""
    x = x - np.rint(x)
    two_pi = 2 * np.arctan2(np.longdouble(0), np.longdouble(-1))
    return np.cos(two_pi * x), -np.sin(two_pi * x)


def stage1_ld(dynspec, freqs, fref=None):
    """(real, imag) long-double parts of S1[k, j] in natural order of k."""
    ld = np.longdouble
    d = np.asarray(dynspec, dtype=np.float64).astype(ld)
    nt, nf = d.shape
    fs = fscale(freqs, fref).astype(ld)
    kt = (_kprime(nt)[:, None] * np.arange(nt, dtype=np.int64)[None, :]).astype(ld)      # exact integers k' t
    re, im = np.empty((nt, nf), dtype=ld), np.empty((nt, nf), dtype=ld)
    for j in range(nf):
        c, s = _cis_cycles(kt * fs[j] / ld(nt))
        re[:, j] = c @ d[:, j]
        im[:, j] = s @ d[:, j]
    return re, im


def slow_ft_ld(dynspec, freqs, fref=None):
    """The long-double truth, rounded to complex128 once at the end."""
    ld = np.longdouble
    re, im = stage1_ld(dynspec, freqs, fref)
    nt, nf = re.shape
    re, im = np.fft.fftshift(re, axes=0), np.fft.fftshift(im, axes=0)
    jm = (np.arange(nf, dtype=np.int64)[:, None] * _kprime(nf)[None, :]) % nf            # (j m) mod nf, exact
    c, s = _cis_cycles(jm.astype(ld) / ld(nf))
    out_re = re @ c - im @ s
    out_im = re @ s + im @ c
    out = np.empty((nt, nf), dtype=np.complex128)
    out.real = np.fft.fftshift(out_re, axes=1).astype(np.float64)
    out.imag = np.fft.fftshift(out_im, axes=1).astype(np.float64)
    return out
