"""The checks of scint_utils.slow_FT, shared by the GPU tests (tests/test_gpu_slowft.py) and the host-interpreter tests
(tests/test_slowft_emu_cpu.py).  `U` is scintools_amd.scint_utils bound to a GPU or to the interpreter.  The truth is the long-double
restatement of tests/slowft_oracle.py, computed once per shape and shared read-only; tests/test_slowft_cpu.py pins both restatements
to the unmodified reference's outputs (tests/golden/slowft.npz).

Tolerance (derived, not tuned).  eps = 2^-52, E = max |out - truth| / sum |dyn|: every output is a sum of nt * nf terms of modulus
|dyn|.  A float64 phase of magnitude up to pi nt s_max carries a few eps of relative error, accumulation adds at most nt eps in
stage 1 and nf eps in stage 2, hence  E <= 16 eps (s_max nt + nf),  s_max = max |fscale|.  Against the goldens (the reference's own
float64 result) twice that.  Every check prints the E it measured."""
import functools

import numpy as np

import slowft_cases as sc
import slowft_oracle as so

EPS = 2.0 ** -52

TAILS = [(1, 1), (2, 1), (1, 16), (3, 5), (17, 16), (250, 37)]
# around the table block B, two blocks and a tail, one block past a group of G blocks, and past two workgroups of 256 |k'|
BLOCKS = [(sc.B - 1, 16), (sc.B, 16), (sc.B + 1, 16), (2 * sc.B + 1, 16), (2 * sc.B + 3, 33), (sc.B * sc.G + 1, 16), (1027, 3)]
# stage 2: direct sum below, row FFT at, direct sum above the first FFT length; an FFT length with a split exchange; no power of two
ROUTES = [(20, 15), (20, 16), (20, 17), (20, 64), (20, 100)]
EMU_LIMIT = 65 * 16          # the interpreter runs the shapes of at most this many pixels


def emu_shapes(shapes):
    return [s for s in shapes if s[0] * s[1] <= EMU_LIMIT]


def bound(nt, nf, fs):
    return 16.0 * EPS * (float(np.max(np.abs(fs))) * nt + nf)


def measure(out, truth, dyn):
    return float(np.max(np.abs(out - truth)) / np.sum(np.abs(dyn)))


def assert_close(tag, out, truth, dyn, fs, factor=1.0):
    nt, nf = dyn.shape
    assert out.shape == (nt, nf) and out.dtype == np.complex128
    e, b = measure(out, truth, dyn), factor * bound(nt, nf, fs)
    print(f"slowft: {tag} {nt}x{nf} E = {e:.3e} bound = {b:.3e}")
    assert e <= b


@functools.lru_cache(maxsize=None)
def truth(nt, nf, kind, lo=1200.0, hi=1600.0, fref_index=None):
    d, f = sc.dyn(nt, nf), sc.freqs(nf, kind, lo, hi)
    out = so.slow_ft_ld(d, f, None if fref_index is None else f[fref_index])
    out.setflags(write=False)
    return out


def check_golden(U, gold, case):
    d, f = sc.golden_inputs(case)
    nt, nf, kind = sc.GOLDEN[case]
    out = U.slow_FT(d, f)
    fs = so.fscale(f)
    assert_close(f"{case} vs truth", out, truth(nt, nf, kind), d, fs)
    assert_close(f"{case} vs reference", out, gold[case], d, fs, factor=2.0)


def check_shape(U, nt, nf, kind="asc"):
    d, f = sc.dyn(nt, nf), sc.freqs(nf, kind)
    assert_close(f"{kind}", U.slow_FT(d, f), truth(nt, nf, kind), d, so.fscale(f))


def check_phase_accuracy(U):
    """1024 x 16 with freqs spanning 2:1: phases up to 2 pi * 0.67 * 512 * 1023 / 1024 before reduction."""
    d, f = sc.dyn(1024, 16), sc.freqs(16, "asc", 1000.0, 2000.0)
    assert_close("2:1 band", U.slow_FT(d, f), truth(1024, 16, "asc", 1000.0, 2000.0), d, so.fscale(f))


def check_constant_freqs(U, nt, nf):
    """All s_j = 1: the plain shifted 2-D FFT."""
    d, f = sc.dyn(nt, nf), sc.freqs(nf, "const")
    assert_close("constant freqs vs fft2", U.slow_FT(d, f), np.fft.fftshift(np.fft.fft2(d)), d, np.ones(nf))


def check_reference_column(U, nt=33, nf=16):
    """Column nf // 2 of stage 1 is a plain DFT whatever freqs are.  Stage 1 is recovered by undoing the frequency transform (an
    average of nf outputs with unit-modulus weights: its error is at most the largest output error)."""
    d, f = sc.dyn(nt, nf), sc.freqs(nf, "uneven")
    out = U.slow_FT(d, f)
    s1 = np.fft.ifftshift(np.fft.ifft(np.fft.ifftshift(out, axes=1), axis=1), axes=0)
    want = np.fft.fft(d[:, nf // 2])
    e, b = float(np.max(np.abs(s1[:, nf // 2] - want)) / np.sum(np.abs(d))), bound(nt, nf, so.fscale(f))
    print(f"slowft: stage-1 column {nf // 2} vs np.fft.fft {nt}x{nf} E = {e:.3e} bound = {b:.3e}")
    assert e <= b


def check_fref(U, nt=33, nf=16):
    d, f = sc.dyn(nt, nf), sc.freqs(nf, "desc")
    base = U.slow_FT(d, f)
    assert np.array_equal(base, U.slow_FT(d, f, fref=f[len(f) // 2]))
    out0 = U.slow_FT(d, f, fref=f[0])
    assert not np.array_equal(out0, base)
    assert_close("fref = freqs[0]", out0, truth(nt, nf, "desc", fref_index=0), d, so.fscale(f, f[0]))


def check_device_paths(U, nt=33, nf=16):
    """A device tensor in, the device tensor out, float32 input: the bits of the host path."""
    import torch
    from scintools_amd import device
    d, f = sc.dyn(nt, nf), sc.freqs(nf, "asc")
    base = U.slow_FT(d, f)
    d_t = device.to_device(d, torch.float64)
    assert np.array_equal(U.slow_FT(d_t, f), base)
    out_t = U.slow_FT(d_t, f, out_device=True)
    assert isinstance(out_t, torch.Tensor) and out_t.dtype == torch.complex128 and out_t.device == d_t.device
    assert np.array_equal(out_t.cpu().numpy(), base)
    d32 = d.astype(np.float32)
    assert np.array_equal(U.slow_FT(d32, f), U.slow_FT(d32.astype(np.float64), f))
    assert np.array_equal(U.slow_FT(torch.from_numpy(d32), f), U.slow_FT(d32.astype(np.float64), f))


def check_nan(U):
    """One NaN pixel makes every output NaN, through both stage-2 routes."""
    for nt, nf in ((33, 16), (20, 15)):
        d = np.array(sc.dyn(nt, nf))
        d[nt // 3, nf - 2] = np.nan
        out = U.slow_FT(d, sc.freqs(nf, "asc"))
        assert out.shape == (nt, nf) and np.all(np.isnan(out.real)) and np.all(np.isnan(out.imag))


def check_deterministic(U, nt=65, nf=16):
    d, f = sc.dyn(nt, nf), sc.freqs(nf, "uneven")
    a, b = U.slow_FT(d, f), U.slow_FT(d, f)
    assert a is not b and np.array_equal(a, b)


def check_eval_sweep(U):
    """The transposed device result is a conjugate spectrum [tau, fd] for the theta-theta sweep, without a host round trip."""
    import torch
    from scintools_amd import ththmod
    from scintools_amd.synth import arc_dynspec
    dyn, freqs, times, eta_true = arc_dynspec(32, 32, seed=1, nimg=8)            # [frequency, time]
    dyn = dyn - dyn.mean()
    ss = U.slow_FT(dyn.T, freqs, out_device=True)                                 # [time, frequency]
    assert isinstance(ss, torch.Tensor) and tuple(ss.shape) == (32, 32)
    fd = ththmod.fft_axis(times, 1000.0, 0)
    tau = ththmod.fft_axis(freqs, 1.0, 0)
    edges = np.linspace(-fd.max() / 2, fd.max() / 2, 16)
    etas = np.array([0.7, 1.0, 1.4]) * eta_true
    eigs = ththmod.eval_sweep(ththmod.to_device(ss.T), tau, fd, etas, edges)
    print("slowft: eval_sweep on the NuT spectrum:", eigs)
    assert eigs.shape == (3,)


def check_errors(U, pytest):
    from scintools_amd import _lib
    with pytest.raises(_lib.ScintHipError, match="bad shape"):
        U.slow_FT(np.zeros((0, 4)), np.arange(4.0) + 1)
    with pytest.raises(ValueError, match="frequencies for"):
        U.slow_FT(np.zeros((4, 4)), np.arange(5.0) + 1)
    with pytest.raises(ValueError, match="time, frequency"):
        U.slow_FT(np.zeros(4), np.arange(4.0) + 1)
