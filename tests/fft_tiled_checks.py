"""Checks of the tiled column route of run_cols_fft (csrc/fft.hpp), shared by the host-interpreted tests
(tests/test_fft_tiled_emu_cpu.py, a build with -DSCINT_COLS_CACHE_BYTES=0.0) and the GPU tests (tests/test_gpu_fft_tiled.py, the
product at its 300 MiB threshold).  The cases, and what each is there for: tests/fft_tiled_cases.py.

Reference: a long-double DFT, applied separably (rows, then columns) to the padded input the entry point defines; no np.fft.
Its twiddles are exp(-2 pi i m / n) of the index product REDUCED mod n in integers, m = j k mod n, evaluated in np.longdouble.
Up to 256 points the DFT is the n x n matrix product.  Longer ones are split once, n = n1 n2 (Cooley-Tukey, an exact identity:
X[k1 + n1 k2] = sum_j2 W_n2^{j2 k2} W_n^{j2 k1} sum_j1 W_n1^{j1 k1} x[n2 j1 + j2]), into matrix products of n1 and n2 points with
the same exactly reduced twiddles -- n (n1 + n2) long-double products instead of n^2, which 16384 points would not allow in a test;
check_reference_split holds the split to the unsplit product.  Its rounding, a few 1e-19 log2 n of the maximum, is seven orders
below the bound.

Tolerance: the project's own for these entry points, |got - ref| <= 1e-12 max|ref| (test_fft2_matches_numpy,
test_conjugate_spectrum).  The stacks are held to the BITS of the single call in the same build.  The two routes add in different
orders: nothing here compares the bits of the two builds.

Largest |got - ref| / max|ref| observed, interpreted build (every case prints its own):
    scint_fft2, 21 shapes            8.4e-16   (16384 x 48)
    conjugate spectrum, npad = 0     1.2e-16   (256 x 16; the peak is the sum of the chunk, hence the small ratio)
    conjugate spectrum, padded       7.6e-17   (256 x 16, npad 1)
    scint_fft2, chirp-z columns      7.2e-16   (3000 x 17)
    scint_cs_batch, last problem     1.4e-16   (B = 3)
    scint_acf_batch, last problem    4.2e-16   (B = 3)
the largest of all: 8.4e-16, three orders inside the bound.

That the cases can fail was shown once on copies of fft.hpp with one line changed each (threshold-0 build, this module):
    `if (!s.ok) return;` removed from ColsBStore          every real-input case fails (21 + 3 conjugate spectra, both stacks)
    tw[s.inner * k1] -> tw[s.inner * (k1 ^ 1)] in pass A   every transform case fails (51 of 53 tests)
    batch = q >> lbits -> batch = 0 in tile_slot            scint_acf_batch B = 3 fails, alone: scint_cs_batch queues one-problem
                                                            passes, so only a truly stacked launch has batch bits to lose
"""
import ctypes

import numpy as np

import fft_tiled_cases as tc

TOL = 1e-12          # of max|ref|: tests/test_gpu_parity.py (FFT / CS)

LD, CLD = np.longdouble, np.clongdouble
_PI = 4 * np.arctan(LD(1))
_tables = {}


# ---- the long-double reference ----------------------------------------------------------------------------------------------------
def _w(n):
    """W_n^m = exp(-2 pi i m / n), m = 0 .. n-1, in long double."""
    if n not in _tables:
        a = 2 * _PI * np.arange(n, dtype=LD) / LD(n)
        _tables[n] = (np.cos(a) - 1j * np.sin(a)).astype(CLD)
    return _tables[n]


def _dft_matrix(n):
    j = np.arange(n, dtype=np.int64)
    return _w(n)[(j[:, None] * j[None, :]) % n]


def _split(n):
    """n = n1 * n2 with n1 <= n2 as close as the divisors allow; (1, n) for a prime."""
    n1 = int(np.sqrt(n))
    while n % n1:
        n1 -= 1
    return n1, n // n1


def dft_ld(x, axis, split=True):
    """Forward DFT (NumPy's sign) of x along `axis` in long double."""
    x = np.moveaxis(np.asarray(x).astype(CLD), axis, 0)
    n = x.shape[0]
    n1, n2 = _split(n)
    if n <= 256 or n1 == 1 or not split:
        out = np.tensordot(_dft_matrix(n), x, axes=(1, 0))
    else:
        rest = x.shape[1:]
        a = x.reshape((n1, n2) + rest)                                  # a[j1, j2] = x[n2 j1 + j2]
        y = np.tensordot(_dft_matrix(n1), a, axes=(1, 0))               # y[k1, j2]
        k1, j2 = np.arange(n1, dtype=np.int64), np.arange(n2, dtype=np.int64)
        y *= _w(n)[(k1[:, None] * j2[None, :]) % n].reshape((n1, n2) + (1,) * len(rest))
        z = np.tensordot(_dft_matrix(n2), y, axes=(1, 1))               # z[k2, k1]: X[k1 + n1 k2]
        out = z.reshape((n,) + rest)
    return np.moveaxis(out, 0, axis)


def fft2_ld(x):
    return dft_ld(dft_ld(x, 1), 0)


def shift2(a):
    """np.fft.fftshift of both axes (an index rotation by n // 2)."""
    return np.roll(a, (a.shape[0] // 2, a.shape[1] // 2), axis=(0, 1))


def cs_ld(dyn, npad, pad_value):
    """The conjugate spectrum (oracle/thth_oracle.py: conjugate_spectrum, no delay mask) in long double."""
    nf, nt = dyn.shape
    pad = np.full(((npad + 1) * nf, (npad + 1) * nt), pad_value, dtype=LD)
    pad[:nf, :nt] = dyn
    return shift2(fft2_ld(pad))


def check_reference_split():
    """The split DFT equals the unsplit matrix product to long-double rounding, at a power of two and at 300 = 15 * 20."""
    for n in (1024, 300):
        x = tc.complex_input((n, 3))
        a, b = dft_ld(x, 0), dft_ld(x, 0, split=False)
        err = float(np.abs(a - b).max() / np.abs(b).max())
        print(f"long-double DFT, n = {n}: split against unsplit {err:.2e}")
        assert err <= 64 * float(np.finfo(LD).eps)


def rel_err(got, ref):
    return float(np.abs(got.astype(CLD) - ref).max() / np.abs(ref).max())


# ---- the device side --------------------------------------------------------------------------------------------------------------
def fft2_device(x):
    """scint_fft2 as tests/test_gpu_parity.py::test_fft2_matches_numpy calls it."""
    import torch
    from scintools_amd import _lib
    from scintools_amd.device import empty, ptr, stream_ptr, to_device
    lib = _lib.load()
    need = ctypes.c_size_t()
    _lib.check(lib.scint_fft2_workspace_bytes(x.shape[0], x.shape[1], ctypes.byref(need)))
    ws = empty((need.value,), torch.uint8)
    xt = to_device(x, torch.complex128)
    out = empty(x.shape, torch.complex128)
    _lib.check(lib.scint_fft2(ptr(xt), ptr(out), x.shape[0], x.shape[1], ptr(ws), ws.numel(), stream_ptr()))
    return out.cpu().numpy()


def check_fft2(shape):
    x = tc.complex_input(shape)
    err = rel_err(fft2_device(x), fft2_ld(x))
    print(f"scint_fft2 {shape}: |got - ref| / max|ref| = {err:.3e}")
    assert err <= TOL, (shape, err)
    return err


def cs_with_workspace(dyn, npad):
    """scint_cs on a workspace that was filled with 0xff bytes: (CS, the workspace afterwards, pad_value)."""
    import torch
    from scintools_amd import _lib
    from scintools_amd.device import empty, ptr, stream_ptr, to_device
    lib = _lib.load()
    nf, nt = dyn.shape
    need = ctypes.c_size_t()
    _lib.check(lib.scint_cs_workspace_bytes(nf, nt, npad, ctypes.byref(need)))
    ws = empty((need.value,), torch.uint8)
    ws.fill_(0xff)
    pad_value = float(dyn.mean())
    out = empty(((npad + 1) * nf, (npad + 1) * nt), torch.complex128)
    _lib.check(lib.scint_cs(ptr(to_device(dyn, torch.float64)), nf, nt, npad, pad_value, 0, 0, 0, ptr(out), ptr(ws), ws.numel(),
                            stream_ptr()))
    return out.cpu().numpy(), ws.cpu().numpy(), pad_value


def check_pad_columns(ws, nf, R, C):
    """The half-width route keeps its column working array in rows of ChL = Ch rounded up to 8 elements (fft2_general, make_plan:
    the row result [nf][C] first, then, 256-byte aligned, the working array [R][ChL]).  The pad columns Ch .. ChL-1 belong to no
    column: the radix route never writes them (its lanes stop at ncols), so the tiled route -- whose last tile reaches across
    them -- must leave the 0xff bytes the workspace was filled with.  The live columns next to them must all have been written:
    that ties the offsets used here to the layout."""
    Ch = C // 2 + 1
    ChL = (Ch + 7) & ~7
    off = (nf * C * 16 + 255) & ~255
    work = ws[off:off + R * ChL * 16].reshape(R, ChL, 16)
    assert ChL > Ch
    untouched = (work == 0xff).all(axis=2)
    assert not untouched[:, :Ch].any(), "the working array is not where this check looks for it"
    assert untouched[:, Ch:].all(), f"{int((~untouched[:, Ch:]).sum())} pad elements of the column working array were written"


def check_cs_partial_tile(nf, nt):
    dyn = tc.real_input(nf, nt)
    got, ws, pad_value = cs_with_workspace(dyn, 0)
    err = rel_err(got, cs_ld(dyn, 0, pad_value))
    print(f"conjugate spectrum ({nf}, {nt}), npad 0, Ch = {nt // 2 + 1}: |got - ref| / max|ref| = {err:.3e}")
    assert err <= TOL, (nf, nt, err)
    check_pad_columns(ws, nf, nf, nt)
    return err


def check_cs_padded(thth, nf, nt, npad):
    """Through the wrapper (ththmod.conjugate_spectrum: the mean is the pad value), then the pad columns as above."""
    dyn = tc.real_input(nf, nt, seed=npad)
    got = thth.conjugate_spectrum(dyn, npad).cpu().numpy()
    err = rel_err(got, cs_ld(dyn, npad, float(dyn.mean())))
    print(f"conjugate spectrum ({nf}, {nt}), npad {npad}: |got - ref| / max|ref| = {err:.3e}")
    assert err <= TOL, (nf, nt, npad, err)
    got2, ws, _ = cs_with_workspace(dyn, npad)
    assert np.array_equal(got2.view(np.uint64), got.view(np.uint64))
    check_pad_columns(ws, nf, (npad + 1) * nf, (npad + 1) * nt)
    return err


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def check_cs_batch(thth, B, nf, nt):
    """scint_cs_batch as ththmod calls it: every problem has the bits of conjugate_spectrum alone, and is the transform."""
    import torch
    from scintools_amd import _lib
    from scintools_amd.device import empty, stream_ptr, to_device, workspace_for
    x = np.stack([tc.real_input(nf, nt, seed=10 + k) for k in range(B)])
    pads = np.ascontiguousarray([x[k].mean() for k in range(B)], dtype=np.float64)
    lohi = np.zeros((B, 2), dtype=np.int64)
    stack = empty((B, nf, nt), torch.complex128)
    ws = workspace_for("scint_cs", nf, nt, 0)
    _lib.call("scint_cs_batch", to_device(x, torch.float64), B, nf, nt, 0, pads, lohi, 0, stack, ws, ws.numel(), stream_ptr())
    got = stack.cpu().numpy()
    for k in range(B):
        one = thth.conjugate_spectrum(x[k], 0).cpu().numpy()
        assert np.array_equal(bits(got[k]), bits(one)), (k, int((bits(got[k]) != bits(one)).sum()))
    err = rel_err(got[B - 1], cs_ld(x[B - 1], 0, pads[B - 1]))
    print(f"scint_cs_batch B = {B} ({nf}, {nt}): last problem |got - ref| / max|ref| = {err:.3e}")
    assert err <= TOL
    return err


def acf_ld(x):
    """The ACF (dynspec.py:3780-3797; subtract_mean and normalise off) in long double: the inverse transform of the real, even
    power spectrum is its forward transform over R C."""
    nf, nt = x.shape
    pad = np.zeros((2 * nf, 2 * nt), dtype=LD)
    pad[:nf, :nt] = x
    power = np.abs(fft2_ld(pad)) ** 2
    return shift2(fft2_ld(power).real) / LD(4 * nf * nt)


def check_acf_batch(sp, B, nf, nt):
    """scint_acf_batch: B problems in ONE tiled launch per pass.  Every problem has the bits of acf_device alone (the same build),
    and the last one is the ACF to the single call's tolerance (tests/acf_batch_checks.py: 1e-12 of the maximum).  acf_device is
    the B = 1 of the same route (csrc/fft.hip: acf_stack), which decodes no problem: the bit check guards the problem decode of
    that one route -- the stacked rows, the tile slots' batch bits, the per-problem partials -- not two implementations."""
    import torch
    x = np.stack([tc.real_input(nf, nt, seed=20 + k) for k in range(B)])
    xt = sp.device.to_device(x, torch.float64)
    got = sp.acf_stack_device(xt, subtract_mean=False, normalise=False).cpu().numpy()
    assert got.shape == (B, 2 * nf, 2 * nt)
    for k in range(B):
        one = sp.acf_device(xt[k], subtract_mean=False, normalise=False).cpu().numpy()
        assert np.array_equal(bits(got[k]), bits(one)), (k, int((bits(got[k]) != bits(one)).sum()))
    ref = acf_ld(x[B - 1])
    err = float(np.abs(got[B - 1].astype(LD) - ref).max() / np.abs(ref).max())
    print(f"scint_acf_batch B = {B} ({nf}, {nt}): last problem |got - ref| / max|ref| = {err:.3e}")
    assert err <= TOL
    return err
