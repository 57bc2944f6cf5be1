"""scintools.scint_utils on the device: slow_FT, the scaled-time ("NuT") conjugate spectrum of the theta-theta papers
(scint_utils.py:655-703), and the helpers of that module this package already has.

slow_FT transforms the time axis of every channel at t * f / fref, so that an arc's Doppler frequency no longer scales with the
observing frequency across a wide band, and applies a plain FFT along frequency.  The reference forms an [ntime, ntime, nfreq]
complex array (16 nt^2 nf bytes); here the exponentials are generated inside the kernel (csrc/slowft.hpp)
and the memory is 40 nt nf bytes.  There is no CPU fallback.
"""
import numpy as np
import torch

from . import _lib, device
from .clean import is_valid, svd_model          # noqa: F401  (scint_utils.py:75, 622)
from .dynspec import get_window                 # noqa: F401  (scint_utils.py:431)

__all__ = ["slow_FT", "svd_model", "is_valid", "get_window"]


def _bare(x):
    """A Quantity's numbers (in its own unit), anything else unchanged."""
    return x.value if hasattr(x, "unit") and hasattr(x, "value") else x


def slow_FT(dynspec, freqs, *, fref=None, out_device=False):
    """Slow FT of a dynamic spectrum along t * (f / fref), then an FFT along frequency (scint_utils.py:655-703).

    dynspec : [time, frequency] array (the TRANSPOSE of Dynspec.dyn) -- NumPy array, Quantity or device tensor; cast to float64.
    freqs   : frequencies of the channels (any unit: only freqs / fref enters).
    fref    : reference frequency; None = freqs[len(freqs) // 2], the reference's hard-coded choice.
    Returns fftshift(fft(fftshift(S1, axes=0), axis=1), axes=1) with S1[k, j] = sum_t dynspec[t, j] exp(-2 pi i t (f_j / fref) ft[k]),
    ft = np.fft.fftfreq(ntime, 1): a complex128 ndarray [time, frequency], or the device tensor with out_device=True (its
    transpose is a conjugate spectrum [tau, fd] for ththmod.to_device / eval_sweep)."""
    dev = device.require_gpu()
    freqs = np.asarray(_bare(freqs))
    if freqs.ndim != 1:
        raise ValueError("slow_FT: freqs must be one-dimensional")
    if fref is None:
        fref = freqs[len(freqs) // 2]                        # scint_utils.py:683-684
    fscale = (freqs / _bare(fref)).astype('float64')         # scint_utils.py:685-686
    dyn_t = device.to_device(_bare(dynspec), torch.float64)
    if dyn_t.dim() != 2:
        raise ValueError("slow_FT: dynspec must be [time, frequency]")
    nt, nf = (int(v) for v in dyn_t.shape)
    if fscale.shape[0] != nf:
        raise ValueError(f"slow_FT: {fscale.shape[0]} frequencies for {nf} channels")
    ws = device.workspace_for("scint_slow_ft", nt, nf)
    fs_t = device.to_device(fscale, torch.float64)
    out = torch.empty((nt, nf), dtype=torch.complex128, device=dev)
    _lib.call("scint_slow_ft", dyn_t, nt, nf, fs_t, out, ws, ws.numel(), device.stream_ptr())
    return out if out_device else out.cpu().numpy()
