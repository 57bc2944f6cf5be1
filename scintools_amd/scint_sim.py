"""Split-step electromagnetic screen simulator on the device: ``scint_sim.Simulation`` of the reference
(scint_sim.py:23-311, after Coles et al. 2010) with its constructor signature and its attributes.

    from scintools_amd.scint_sim import Simulation
    from scintools_amd.dynspec import Dynspec
    d = Dynspec(dyn=Simulation(mb2=20, ar=10, nx=4096, ny=128, nf=4096, seed=1), verbose=False)

The screen weights, both screen transforms and, per frequency, ``ifft2(frfilt3(fft2(exp(1j * xyp * scale))))`` run in
HIP kernels (csrc/sim.hpp; entry points scint_sim_screen / scint_sim_field / scint_sim_pulse).  Only column ``ny/2`` of
every inverse transform is kept by the reference, so only that column is computed ("The screen simulator").
The scalars and axes are host arithmetic restated operation by operation.  There is no CPU fallback.

Random numbers: the reference seeds NumPy's legacy global generator and draws ``randn(nx, ny)`` twice; the same numbers
are drawn here on the host from ``np.random.RandomState(seed)`` in the same order and uploaded, so a seed gives the
reference's screen.

Sizes: ``nx`` a power of two in [16, 131072] (the strided axis: the column passes of the FFT, run_cols_fft, each with at
most 65535 butterflies in its grid -- 2**18 would end on a radix-4 pass of 65536), ``ny`` a
power of two in [16, 8192] (the contiguous axis: the row kernel, launch_fft_rows), ``nx * ny <= 2**28``, ``nf >= 2``
arbitrary; anything else raises ``ValueError``.  ``pulsewin`` needs ``2 * nf`` to be a power of two in [16, 8192] and
raises ``NotImplementedError`` otherwise.

``ACF`` is the reference's theoretical 2-D intensity ACF (scint_sim.py:417-766; Rickett et al. 2014, Appendix A), the model of
``scint_models.scint_acf_model_2d``:

    from scintools_amd.scint_sim import ACF
    model = ACF(ar=3, psi=30, phasegrad=0.5, theta=40, taumax=4, dnumax=4, nt=51, nf=51).acf

Its Fresnel sums run as one float64 matrix-core contraction per frequency lag (csrc/acf.hpp, entry point scint_acf_model;
DESIGN.md, "The 2-D ACF model"); the axes, the ``dnun = 0`` column and the mirroring are the reference's NumPy lines on the host.
"""
import ctypes
import warnings

import numpy as np
import scipy.constants as sc
import torch
from scipy.special import gamma

from . import _lib, device

NX_MIN, NX_MAX = 16, 1 << 17
NY_MIN, NY_MAX = 16, 8192
PLANE_MAX = 1 << 28
# Default bound of one group's working set: it stays inside the 256 MiB Infinity Cache, where the in-place column passes
# re-read what they have just written (fft.hpp, run_cols_fft).  Never more than half of the free device memory.
SIM_GROUP_BYTES = 128 << 20


def _pow2(n):
    return n > 0 and (n & (n - 1)) == 0


def last_route():
    """(column, groups) of the last field computation of the process: whether it took the column shortcut (False with
    SCINT_SIM_COLUMN=0) and the number of frequency groups it ran."""
    col, groups = ctypes.c_int32(), ctypes.c_int64()
    _lib.call("scint_sim_last_route", col, groups)
    return bool(col.value), int(groups.value)


class Simulation:
    """The reference's ``Simulation``: same arguments, same attributes (``xyp, w, spe, spi, dyn, xyi, x, lams, freqs,
    times, df, bw, dt, freq, tobs, mjd, nsub, nchan, name, header, eta, betaeta, ffconx, ffcony, consp, s0, sref,
    scnorm``; ``pulsewin`` and ``dm`` on first access).  ``group_bytes`` bounds the device memory of one group of
    frequencies (default: ``SIM_GROUP_BYTES``, at most half of the free memory).  The result does not depend on it while a
    group's planes stay below the 300 MiB at which run_cols_fft changes from radix passes to its tiled form (the default
    does); a larger ``group_bytes`` agrees to rounding, not bit for bit."""

    def __init__(self, mb2=2, rf=1, ds=0.01, alpha=5 / 3, ar=1, psi=0, inner=0.001, ns=256, nf=256, dlam=0.25,
                 lamsteps=False, seed=None, nx=None, ny=None, dx=None, dy=None, plot=False, verbose=False, freq=1400,
                 dt=30, mjd=60000, nsub=None, efield=False, noise=None, group_bytes=None):
        if plot:
            raise NotImplementedError("plotting is outside the accelerated hot path")
        self.mb2 = mb2
        self.rf = rf
        self.ds = ds
        self.dx = dx if dx is not None else ds
        self.dy = dy if dy is not None else ds
        self.alpha = alpha
        self.ar = ar
        self.psi = psi
        self.inner = inner
        self.nx = nx if nx is not None else ns
        self.ny = ny if ny is not None else ns
        self.nf = nf
        self.dlam = dlam
        self.lamsteps = lamsteps
        self.seed = seed
        for name, n, lo, hi in (("nx", self.nx, NX_MIN, NX_MAX), ("ny", self.ny, NY_MIN, NY_MAX)):
            if not (isinstance(n, (int, np.integer)) and _pow2(int(n)) and lo <= n <= hi):
                raise ValueError(f"{name}={n}: the device transforms need a power of two in [{lo}, {hi}]")
        if self.nx * self.ny > PLANE_MAX:
            raise ValueError(f"nx * ny = {self.nx * self.ny}: at most 2**28 screen points")
        if not (isinstance(nf, (int, np.integer)) and nf >= 2):
            raise ValueError(f"nf={nf}: at least 2 frequencies (the reference builds no dynamic spectrum from one)")
        if self.nx * nf >= 2 ** 31:
            raise ValueError(f"nx * nf = {self.nx * nf}: must stay below 2**31")
        self.nx, self.ny, self.nf = int(self.nx), int(self.ny), int(nf)

        self.set_constants()
        if verbose:
            print('Computing screen phase')
        self.get_screen()
        if verbose:
            print('Getting intensity...')
        self.get_intensity(group_bytes=group_bytes)
        if verbose:
            print('Computing dynamic spectrum')
        self.get_dynspec()

        # physical units (scint_sim.py:81-133)
        self.name = 'sim:mb2={0},ar={1},psi={2},dlam={3}'.format(self.mb2, self.ar, self.psi, self.dlam)
        if lamsteps:
            self.name += ',lamsteps'
        self.header = [self.name, 'MJD0: {}'.format(mjd)]
        dyn = np.real(self.spe) if efield else self.spi
        self.dt = dt
        self.freq = freq
        self.nsub = int(np.shape(dyn)[0]) if nsub is None else nsub
        self.nchan = int(np.shape(dyn)[1])
        if not lamsteps:
            self.df = self.freq * self.dlam / (self.nchan - 1)
            self.freqs = self.freq + np.arange(-self.nchan / 2, self.nchan / 2, 1) * self.df
        else:
            self.lam = sc.c / (self.freq * 10**6)
            self.dl = self.lam * self.dlam / (self.nchan - 1)
            self.lams = self.lam + np.arange(-self.nchan / 2, self.nchan / 2, 1) * self.dl
            self.freqs = sc.c / self.lams / 10**6
            self.freq = (np.max(self.freqs) - np.min(self.freqs)) / 2     # the reference's redefinition (scint_sim.py:113)
        self.bw = max(self.freqs) - min(self.freqs)
        self.times = self.dt * np.arange(0, self.nsub)
        self.df = self.bw / self.nchan
        self.tobs = float(self.times[-1] - self.times[0])
        self.mjd = mjd
        if nsub is not None:
            dyn = dyn[0:nsub, :]
        self.dyn = np.transpose(dyn)
        V = self.ds / self.dt
        lambda0 = self.freq
        k = 2 * np.pi / lambda0
        L = self.rf**2 * k
        self.eta = L / (2 * V**2) / 10**6 / np.cos(psi * np.pi / 180)**2
        c = 299792458.0
        beta_to_eta = c * 1e6 / ((self.freq * 10**6)**2)
        self.betaeta = self.eta / beta_to_eta

    def set_constants(self):                                            # scint_sim.py:137-167
        ns = 1
        lenx = self.nx * self.dx
        leny = self.ny * self.dy
        self.ffconx = (2.0 / (ns * lenx * lenx)) * (np.pi * self.rf)**2
        self.ffcony = (2.0 / (ns * leny * leny)) * (np.pi * self.rf)**2
        dqx = 2 * np.pi / lenx
        dqy = 2 * np.pi / leny
        a2 = self.alpha * 0.5
        aa = 1.0 + a2
        ab = 1.0 - a2
        cdrf = 2.0**(self.alpha) * np.cos(self.alpha * np.pi * 0.25) * gamma(aa) / self.mb2
        self.s0 = self.rf * cdrf**(1.0 / self.alpha)
        cmb2 = self.alpha * self.mb2 / (4 * np.pi * gamma(ab) * np.cos(self.alpha * np.pi * 0.25) * ns)
        self.consp = cmb2 * dqx * dqy / (self.rf**self.alpha)
        self.scnorm = 1.0 / (self.nx * self.ny)
        self.sref = self.rf**2 / self.s0

    def get_screen(self):
        """w and xyp = real(fft2(w (z1 + 1j z2))) (scint_sim.py:169-207); the normals are the reference's for the seed."""
        dev = device.require_gpu()
        nx, ny = self.nx, self.ny
        rs = np.random.RandomState(self.seed)
        z1 = torch.from_numpy(rs.randn(nx, ny)).to(dev)
        z2 = torch.from_numpy(rs.randn(nx, ny)).to(dev)
        dqx = 2 * np.pi / (self.dx * nx)
        dqy = 2 * np.pi / (self.dy * ny)
        cs = np.cos(self.psi * np.pi / 180)                              # swdsp, scint_sim.py:277-285
        sn = np.sin(self.psi * np.pi / 180)
        r = self.ar
        con = np.sqrt(self.consp)
        alf = -(self.alpha + 2) / 4
        a = (cs**2) / r + r * sn**2
        b = r * cs**2 + sn**2 / r
        c = 2 * cs * sn * (1 / r - r)
        ws = device.workspace_for("scint_sim_screen", nx, ny)
        w = torch.empty((nx, ny), dtype=torch.float64, device=dev)
        xyp = torch.empty((nx, ny), dtype=torch.float64, device=dev)
        _lib.call("scint_sim_screen", z1, z2, nx, ny, dqx, dqy, a, b, c, con, alf, self.inner**2, w, xyp, ws, ws.numel(),
                  device.stream_ptr())
        self._xyp_t = xyp
        self.w = w.cpu().numpy()
        self.xyp = xyp.cpu().numpy()

    def _scales(self):
        out = np.empty(self.nf)
        for ifreq in range(0, self.nf):                                  # scint_sim.py:218-224
            if self.lamsteps:
                scale = 1.0 + self.dlam * (ifreq - 1 - (self.nf / 2)) / (self.nf)
            else:
                frfreq = 1.0 + self.dlam * (-0.5 + ifreq / self.nf)
                scale = 1 / frfreq
            out[ifreq] = scale
        return out

    def get_intensity(self, verbose=False, group_bytes=None):
        """spe [nx, nf] complex64, spi = |spe|^2 float32 and xyi [nx, ny] of the last frequency (scint_sim.py:209-244)."""
        dev = device.require_gpu()
        nx, ny, nf = self.nx, self.ny, self.nf
        if group_bytes is None:
            group_bytes = SIM_GROUP_BYTES
            if dev.type == "cuda":
                group_bytes = min(group_bytes, torch.cuda.mem_get_info(dev)[0] // 2)
        one, two, need = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        _lib.call("scint_sim_field_workspace_bytes", nx, ny, 1, one)
        _lib.call("scint_sim_field_workspace_bytes", nx, ny, 2, two)
        per = max(1, two.value - one.value)
        group = int(min(nf, max(1, 1 + (int(group_bytes) - one.value) // per)))
        _lib.call("scint_sim_field_workspace_bytes", nx, ny, group, need)
        ws = device.workspace.get(need.value)         # (the library sizes its groups by the BYTES it is told: need, not the buffer's)
        xyp = getattr(self, "_xyp_t", None)
        if xyp is None:
            xyp = device.to_device(self.xyp, torch.float64)
        scale = device.to_device(self._scales(), torch.float64)
        spe = torch.empty((nx, nf), dtype=torch.complex64, device=dev)
        spi = torch.empty((nx, nf), dtype=torch.float32, device=dev)
        xyi = torch.empty((nx, ny), dtype=torch.float64, device=dev)
        _lib.call("scint_sim_field", xyp, nx, ny, scale, nf, 0, nf, self.ffconx, self.ffcony, spe, spi, xyi, ws, need.value,
                  device.stream_ptr())
        self._xyp_t = None
        self.xyi = xyi.cpu().numpy()
        self.spe = spe.cpu().numpy()
        self.spi = spi.cpu().numpy()

    def get_dynspec(self):                                               # scint_sim.py:238-252 (spi: with spe, from the device)
        self.x = np.linspace(0, self.dx * (self.nx), (self.nx))
        ifreq = np.linspace(0, self.nf - 1, self.nf)
        lam_norm = 1.0 + self.dlam * (ifreq - 1 - (self.nf / 2)) / self.nf
        self.lams = lam_norm / np.mean(lam_norm)
        frfreq = 1.0 + self.dlam * (-0.5 + ifreq / self.nf)
        self.freqs = frfreq / np.mean(frfreq)

    def get_pulse(self):
        """pulsewin and dm (scint_sim.py:254-274): a device row FFT of length 2 nf, the Blackman window fused into its load,
        |.|^2 and the roll into its store."""
        nf = self.nf
        if not (_pow2(2 * nf) and 16 <= 2 * nf <= 8192):
            raise NotImplementedError(f"pulsewin: 2 * nf = {2 * nf} is not a power of two in [16, 8192] (the row transform's lengths)")
        dev = device.require_gpu()
        spe = torch.from_numpy(np.array(self.spe, dtype=np.complex64, order="C")).to(dev)
        win = device.to_device(np.blackman(nf), torch.float64)
        out = torch.empty((self.nx, 2 * nf), dtype=torch.float64, device=dev)
        _lib.call("scint_sim_pulse", spe, self.nx, nf, win, out, device.stream_ptr())
        self.__dict__["pulsewin"] = np.transpose(out.cpu().numpy())
        self.__dict__["dm"] = self.xyp[:, int(self.ny / 2)] * self.dlam / np.pi

    def __getattr__(self, name):                                         # pulsewin / dm: computed on first access
        if name == "dm" and "xyp" in self.__dict__:
            return self.xyp[:, int(self.ny / 2)] * self.dlam / np.pi
        if name == "pulsewin" and "spe" in self.__dict__:
            self.get_pulse()
            return self.__dict__[name]
        raise AttributeError(f"'{type(self).__name__}' object has no attribute '{name}'")


class ACF:
    """The reference's ``ACF``: same arguments, same attributes (``alpha, ar, psi, phasegrad, theta, amp, wn, taumax, dnumax, nf, nt,
    sp_fac, res_fac, core_fac, dsp, ddnun``; ``fn, tn, sn, snp, acf, acf_efield``; ``sspec`` after ``calc_sspec``).  The sums over the
    spatial grids -- every ``dnun > 0`` column of the field -- and ``acf_efield`` come from the device (scint_acf_model); the complex
    field before ``real(g * conj(g))`` is kept as ``gammitv``.  ``plot=True`` and the ``plot_*`` methods warn and draw nothing.  Sizes
    the reference cannot compute raise what it raises: ``nf = 1`` an ``IndexError`` (``dnun[1]``), ``nt = 1`` a
    ``ZeroDivisionError`` (``dsp``); 2 is made odd first, as every even size, and computes."""

    def __init__(self, psi=0, phasegrad=0, theta=0, ar=1, alpha=5 / 3, taumax=4, dnumax=4, nf=51, nt=51, amp=1, wn=0,
                 spatial_factor=2, resolution_factor=1, core_factor=2, auto_sampling=True, plot=False, display=True):
        self.alpha = alpha
        self.ar = ar
        self.psi = psi
        self.phasegrad = phasegrad
        self.theta = theta
        self.amp = amp
        self.wn = wn
        self.taumax = taumax
        spmax = taumax
        self.dnumax = dnumax
        if nf % 2 == 0:
            nf += 1
        if nt % 2 == 0:
            nt += 1
        self.nf = nf
        self.nt = nt
        if auto_sampling:                                                # scint_sim.py:471-481
            self.sp_fac = 6 * ar / spmax
            self.res_fac = 1 + ar / 3
            self.core_fac = 4
        else:
            self.sp_fac = spatial_factor
            self.res_fac = resolution_factor
            self.core_fac = core_factor
        self.dsp = 4 * spmax / (nt - 1)
        self.calc_acf()
        if plot:
            self.plot_acf(display=display)

    def calc_acf(self, plot=False):
        """The ACF of intensity against time and frequency lag (scint_sim.py:494-678).  Host: the axes (NumPy decides their lengths),
        the ``dnun = 0`` column, the white-noise spike, ``real(g * conj(g))``, the mirroring and ``amp``.  Device: ``acf_efield`` and
        every other column of the field."""
        alph2 = self.alpha / 2
        spmax = self.taumax
        dnumax = self.dnumax
        dsp = self.dsp
        phasegrad = self.phasegrad
        theta = self.theta
        amp = self.amp
        wn = self.wn
        xi = 90 - self.psi
        Vx = np.cos(xi * np.pi / 180)
        Vy = np.sin(xi * np.pi / 180)
        sigxn = phasegrad * np.cos((xi - theta) * np.pi / 180)
        sigyn = phasegrad * np.sin((xi - theta) * np.pi / 180)
        ar = self.ar
        sqrtar = np.sqrt(ar)
        dnun = np.linspace(0, dnumax, int(np.ceil(self.nf / 2)))
        ddnun = np.abs(dnun[1] - dnun[0])
        self.ddnun = ddnun
        ndnun = len(dnun)
        sp_fac = self.sp_fac
        res_fac = self.res_fac
        core_fac = self.res_fac * self.core_fac
        snp = np.arange(-sp_fac * spmax, sp_fac * spmax + dsp / res_fac, dsp / res_fac)
        snp2 = np.arange(-sp_fac * spmax, sp_fac * spmax + dsp / core_fac, dsp / core_fac)
        if phasegrad == 0:
            tn = np.linspace(0, (spmax), int(np.ceil(self.nt / 2)))
            snx = Vx * tn
            sny = Vy * tn
            sigxn = sigyn = 0.0                                          # this branch of the reference does not shift the centres
        else:
            tn = np.linspace(-(spmax), (spmax), self.nt)
            snx = np.cos(xi * np.pi / 180) * tn
            sny = np.sin(xi * np.pi / 180) * tn
        gammitv = np.zeros((int(len(snx)), int(ndnun)), dtype=np.complex128)
        gammitv[:, 0] = np.exp(-0.5 * ((snx / sqrtar)**2 + (sny * sqrtar)**2)**alph2)
        if phasegrad == 0:
            gammitv[0, 0] += wn / amp
        else:
            gammitv[np.argwhere(snx == 0), 0] += wn / amp
        field, gammes = self._device_field(snp, snp2, snx, sny, dnun, float(sigxn), float(sigyn), float(sqrtar), float(alph2),
                                           float(dsp / res_fac), float(dsp / core_fac))
        gammitv[:, 1:] = field[:, 1:]
        self.gammitv = gammitv
        # equation A1 convert ACF of E to ACF of I
        gammitv = np.real(gammitv * np.conj(gammitv))
        nr, nc = np.shape(gammitv)
        if phasegrad == 0:
            gam2 = np.zeros((nr, nc * 2 - 1))
            gam2[:, 0:nc - 1] = np.fliplr(gammitv[:, 1:])
            gam2[:, nc - 1:] = gammitv
            gam2 = gam2.squeeze()
            gam3 = np.zeros((nr * 2 - 1, nc * 2 - 1))
            gam3[0:nr - 1, :] = np.flipud(gam2[1:, :])
            gam3[nr - 1:, :] = gam2
            gam3 = np.transpose(gam3)
            t2 = np.concatenate((np.flip(-tn[1:]), tn)).squeeze()
            f2 = np.concatenate((np.flip(-dnun[1:]), dnun)).squeeze()
        else:
            gam3 = np.zeros((nr, nc * 2 - 1))
            gam3[:, 0:nc - 1] = np.fliplr(np.flipud(gammitv[:, 1:]))
            gam3[:, nc - 1:] = gammitv
            gam3 = np.transpose(gam3)
            f2 = np.concatenate((np.flip(-dnun[1:]), dnun)).squeeze()
            t2 = tn
        self.fn = f2
        self.tn = t2
        self.sn = t2
        self.snp = snp
        self.acf = amp * gam3
        self.acf_efield = gammes
        if plot:
            self.plot_acf()

    @staticmethod
    def _device_field(snp, snp2, snx, sny, dnun, sigxn, sigyn, sqrtar, alph2, step, step2):
        """(field [nsn, ndnun] complex128 with column 0 left at zero, acf_efield [m, m]) from scint_acf_model."""
        dev = device.require_gpu()
        m, m2, nsn, ndnun = len(snp), len(snp2), len(snx), len(dnun)
        need = ctypes.c_size_t()
        _lib.call("scint_acf_model_workspace_bytes", m, m2, nsn, ndnun, need)
        ws = device.workspace.get(need.value)
        d_snp, d_snp2, d_snx, d_sny, d_dnun = (device.to_device(a, torch.float64) for a in (snp, snp2, snx, sny, dnun))
        gammes = torch.empty((m, m), dtype=torch.float64, device=dev)
        gamma = torch.zeros((nsn, ndnun), dtype=torch.complex128, device=dev)
        _lib.call("scint_acf_model", d_snp, m, d_snp2, m2, d_snx, d_sny, nsn, d_dnun, ndnun, sigxn, sigyn, sqrtar, alph2, step, step2,
                  gammes, gamma, ws, need.value, device.stream_ptr())
        return gamma.cpu().numpy(), gammes.cpu().numpy()

    def calc_sspec(self, window='hanning', window_frac=1):
        """The secondary spectrum of the model ACF (scint_sim.py:728-742).  Host NumPy, as in the reference: an odd-length
        transform of the small ``nf x nt`` model array (at most a few hundred points a side), not a hot path."""
        from .dynspec import get_window
        nf, nt = np.shape(self.acf)
        chan_window, subint_window = get_window(nt, nf, window=window, frac=window_frac)
        arr = np.multiply(chan_window, self.acf)
        arr = np.transpose(np.multiply(subint_window, np.transpose(arr)))
        arr = np.fft.fftshift(arr)
        arr = np.fft.fft2(arr)
        arr = np.fft.fftshift(arr)
        arr = np.sqrt(np.real(arr * np.conj(arr)))
        self.sspec = 10 * np.log10(arr)

    def plot_acf(self, *args, **kwargs):
        warnings.warn("ACF.plot_acf: plotting is outside the accelerated hot path; nothing is drawn")

    def plot_acf_efield(self, *args, **kwargs):
        warnings.warn("ACF.plot_acf_efield: plotting is outside the accelerated hot path; nothing is drawn")

    def plot_sspec(self, *args, **kwargs):
        warnings.warn("ACF.plot_sspec: plotting is outside the accelerated hot path; nothing is drawn")
