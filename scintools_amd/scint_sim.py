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

``Brightness`` is the reference's brightness-distribution model of a secondary spectrum and its ACF (scint_sim.py:768-958; Yao et
al. 2020):

    from scintools_amd.scint_sim import Brightness
    b = Brightness(ar=2, psi=30, thetagx=0.5, thetarx=0.5)       # b.SS, b.acf, ...

The field ACF, the per-pixel map with both interpolations of the brightness, the fold and the ACF's normalisation are kernels of
csrc/bright.hpp; its transforms have whatever lengths ``np.arange`` gives and go through ``fft2_any`` (scint_fft2_any: Bluestein's
chirp-z where a length is not a power of two; DESIGN.md, "The brightness-distribution model").
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


FFT_ANY_MAX = 4096        # a Bluestein axis of n points runs at the power of two >= 2 n - 1; the row kernel ends at 8192


def fft2_any(a, in_shift=None, out_shift=None, out="complex"):
    """``np.fft.fft2`` of a 2-D float64 or complex128 array (NumPy or device tensor) of any lengths 2 .. 4096 on the device
    (scint_fft2_any: Bluestein's chirp-z where a length is not one the power-of-two kernels take).  ``in_shift`` / ``out_shift``:
    None, 'fftshift' or 'ifftshift' applied to the input / the result; ``out``: 'complex', 'abs' or 'real'.  Returns a device tensor."""
    dev = device.require_gpu()
    real = not (a.is_complex() if isinstance(a, torch.Tensor) else np.iscomplexobj(a))
    if len(a.shape) != 2:
        raise ValueError(f"fft2_any: a 2-D array is needed, got {len(a.shape)} dimensions")
    R, C = (int(n) for n in a.shape)
    for n in (R, C):
        if not 2 <= n <= FFT_ANY_MAX:
            raise ValueError(f"fft2_any: an axis of {n} points; the device transform takes 2 .. {FFT_ANY_MAX} "
                             f"(an arbitrary length n runs at the power of two >= 2 n - 1, at most 8192)")
    shifts = {None: 0, "fftshift": 1, "ifftshift": 2}
    what = {"complex": 0, "abs": 1, "real": 2}[out]
    src = device.to_device(a, torch.float64 if real else torch.complex128)
    res = torch.empty((R, C), dtype=torch.complex128 if what == 0 else torch.float64, device=dev)
    ws = device.workspace_for("scint_fft2_any", R, C)
    _lib.call("scint_fft2_any", src, int(real), R, C, shifts[in_shift], shifts[out_shift], what, res, ws, ws.numel(),
              device.stream_ptr())
    return res


def diagonals_from_simplices(simplices, n):
    """The one bit per cell of a triangulation of the regular ``n x n`` grid (point ``iy * n + ix``): bool ``[n-1, n-1]``, True where
    cell ``(iy, ix)`` is split along the diagonal from corner ``(ix, iy)`` to ``(ix+1, iy+1)``.  Raises ``ValueError`` unless every
    simplex lies inside one cell and every cell holds exactly two simplices that share one diagonal -- it does not guess."""
    s = np.asarray(simplices)
    if s.ndim != 2 or s.shape[1] != 3:
        raise ValueError(f"diagonals_from_simplices: simplices of shape {s.shape}, expected [ntri, 3]")
    iy, ix = np.divmod(s, n)
    y0, x0 = iy.min(axis=1), ix.min(axis=1)
    if np.any(s < 0) or np.any(s >= n * n) or np.any(iy.max(axis=1) - y0 != 1) or np.any(ix.max(axis=1) - x0 != 1):
        raise ValueError("diagonals_from_simplices: a simplex does not lie inside one grid cell")
    corner = 2 * (iy - y0[:, None]) + (ix - x0[:, None])                 # 0 .. 3: (0,0), (1,0), (0,1), (1,1) as (dx, dy)
    has = np.zeros((len(s), 4), dtype=bool)
    has[np.arange(len(s))[:, None], corner] = True
    if np.any(has.sum(axis=1) != 3):
        raise ValueError("diagonals_from_simplices: a simplex repeats a vertex")
    main = has[:, 0] & has[:, 3]                                          # otherwise it holds corners 1 and 2: the other diagonal
    cell = y0 * (n - 1) + x0
    count = np.bincount(cell, minlength=(n - 1) ** 2)
    nmain = np.bincount(cell, weights=main, minlength=(n - 1) ** 2)
    if len(count) != (n - 1) ** 2 or np.any(count != 2):
        raise ValueError("diagonals_from_simplices: not every cell holds exactly two simplices")
    if np.any((nmain != 0) & (nmain != 2)):
        raise ValueError("diagonals_from_simplices: the two simplices of a cell do not share a diagonal")
    return (nmain == 2).reshape(n - 1, n - 1)


def qhull_diagonals(x):
    """The diagonals of the triangulation ``scipy.interpolate.griddata(method='linear')`` builds for the grid ``meshgrid(x, x)``:
    ``scipy.spatial.Delaunay`` of the same points with the same (default) options."""
    from scipy.spatial import Delaunay
    X, Y = np.meshgrid(x, x)
    tri = Delaunay(np.column_stack((np.ravel(X), np.ravel(Y))))
    return diagonals_from_simplices(tri.simplices, len(x))


class Brightness:
    """The reference's ``Brightness`` (scint_sim.py:768-958; Yao et al. 2020): the secondary spectrum, and its ACF, of an anisotropic
    Kolmogorov brightness distribution with phase-gradient offsets.  Same arguments, methods (``calc_brightness``, ``calc_SS``,
    ``calc_acf``) and attributes (``x, X, Y, acf_efield, B, fd, td, thetax, thetay, jacobian, SS, LSS, acf``).

        b = Brightness(ar=2, psi=30, thetagx=0.5, thetarx=0.5)
        b.SS, b.acf

    The axes are ``np.arange`` on the host.  ``acf_efield, B, SS, LSS, acf, jacobian`` stay in device memory until first read;
    ``thetax`` and ``thetay`` (and ``X``, ``Y``) are produced on first access.  ``plot=True`` and the ``plot_*`` methods warn and draw nothing.

    The reference interpolates ``B`` with ``scipy.interpolate.griddata(method='linear')``: piecewise linear on a Delaunay
    triangulation that splits every grid cell along one of its diagonals -- which one is Qhull's tie-break.
    ``triangulation='qhull'`` (default) takes that bit per cell from ``scipy.spatial.Delaunay`` of the grid (the reference's result on the
    same scipy; the triangulation is the slow part); ``'main'`` splits every cell along the same diagonal and needs no scipy (for fits
    and large grids).  ``diagonals`` (bool ``[n-1, n-1]``, see ``diagonals_from_simplices``) overrides both.
    Every transform goes through ``fft2_any``: the grid and both axes of the spectrum hold at most 4096 points (``ValueError``)."""

    acf_efield = device.DeviceBacked("acf_efield")
    B = device.DeviceBacked("B")
    SS = device.DeviceBacked("SS")
    LSS = device.DeviceBacked("LSS")
    jacobian = device.DeviceBacked("jacobian")
    acf = device.DeviceBacked("acf")

    def __init__(self, ar=1.0, psi=0, alpha=1.67, thetagx=0, thetagy=0, thetarx=0, thetary=0, df=0.02, dt=0.08, dx=0.1, nf=10,
                 nt=80, nx=30, ncuts=5, plot=False, contour=True, figsize=(10, 8), calc_sspec=True, calc_acf=True,
                 triangulation="qhull", diagonals=None):
        if triangulation not in ("qhull", "main"):
            raise ValueError(f"triangulation={triangulation!r}: 'qhull' or 'main'")
        self.ar = ar
        self.alpha = alpha
        self.thetagx = thetagx
        self.thetagy = thetagy
        self.thetarx = thetarx
        self.thetary = thetary
        self.psi = psi
        self.df = df
        self.dt = dt
        self.dx = dx
        self.nf = nf
        self.nt = nt
        self.nx = nx
        self.ncuts = ncuts
        self.triangulation = triangulation
        self.diagonals = None if diagonals is None else np.asarray(diagonals)
        self.calc_brightness()
        if plot:
            self.plot_acf_efield(figsize=figsize)
            self.plot_brightness(figsize=figsize)
        if calc_sspec:
            self.calc_SS()
            if plot:
                self.plot_sspec(figsize=figsize)
                self.plot_cuts(figsize=figsize)
        if calc_acf:
            self.calc_acf()
            if plot:
                self.plot_acf(figsize=figsize, contour=contour)

    @staticmethod
    def _check_axis(name, n):
        if not 2 <= n <= FFT_ANY_MAX:
            raise ValueError(f"Brightness: {name} holds {n} points; the device transform takes 2 .. {FFT_ANY_MAX}")

    def calc_brightness(self):
        """``acf_efield`` and ``B = |ifftshift(fft2(fftshift(acf_efield)))|`` (scint_sim.py:838-869)."""
        dev = device.require_gpu()
        x = np.arange(-self.nx, self.nx, self.dx)
        n = len(x)
        self._check_axis("the grid x = arange(-nx, nx, dx)", n)
        if self.diagonals is not None and (self.diagonals.shape != (n - 1, n - 1) or self.diagonals.dtype != np.bool_):
            raise ValueError(f"diagonals: a bool array of shape {(n - 1, n - 1)} is needed for the grid of {n} points, "
                             f"got {self.diagonals.dtype} {self.diagonals.shape}")
        R = (self.ar**2 - 1) / (self.ar**2 + 1)
        cosa = np.cos(2 * (90 - self.psi) * np.pi / 180)
        sina = np.sin(2 * (90 - self.psi) * np.pi / 180)
        a = (1 - R * cosa) / np.sqrt(1 - R**2)
        b = (1 + R * cosa) / np.sqrt(1 - R**2)
        c = -2 * R * sina / np.sqrt(1 - R**2)
        self.x = x
        for stale in ("_bits", "X", "Y"):
            self.__dict__.pop(stale, None)
        self._x_t = device.to_device(x, torch.float64)
        rho = torch.empty((n, n), dtype=torch.float64, device=dev)
        _lib.call("scint_bright_efield", self._x_t, n, float(a), float(b), float(c), float(self.alpha / 2), rho, device.stream_ptr())
        type(self).acf_efield.park(self, rho)
        type(self).B.park(self, fft2_any(rho, in_shift="fftshift", out_shift="ifftshift", out="abs"))

    def _diagonal_bits(self):
        """The packed bitmap scint_bright_map reads (device uint8), or None for the same diagonal everywhere."""
        diag = self.diagonals
        if diag is None:
            if self.triangulation == "main":
                return None
            diag = qhull_diagonals(self.x)
        return device.to_device(np.packbits(np.ravel(diag), bitorder="little"), torch.uint8)

    def _map(self, want_theta):
        dev = device.require_gpu()
        fd, td = self.fd, self.td
        shape = (len(td), len(fd))
        n = len(self.x)
        if "_bits" not in self.__dict__:
            self._bits = self._diagonal_bits()
        par = np.array([self.thetagx, self.thetagy, self.thetarx, self.thetarx**2, self.thetary**2, 0.5 * self.df, 2 / self.df,
                        10**(-6), (n - 1) / (self.x[-1] - self.x[0])], dtype=np.float64)
        out = [torch.empty(shape, dtype=torch.float64, device=dev) for _ in range(4 if want_theta else 2)]
        _lib.call("scint_bright_map", type(self).B.tensor(self), self._x_t, n, self._bits, device.to_device(fd, torch.float64),
                  len(fd), device.to_device(td, torch.float64), len(td), par, out[0], out[1],
                  out[2] if want_theta else None, out[3] if want_theta else None, device.stream_ptr())
        return out

    def calc_SS(self):
        """``SS``, ``LSS`` and ``jacobian`` (scint_sim.py:871-951): the loop body, both interpolations and the fold on the device."""
        dev = device.require_gpu()
        self.fd = np.arange(-self.nf, self.nf, self.df)
        self.td = np.arange(-self.nt, self.nt, self.dt)
        ntd, nfd = len(self.td), len(self.fd)
        if ntd < 1 or nfd < 1:
            raise ValueError(f"Brightness: an empty spectrum ({ntd} x {nfd})")
        self.__dict__.pop("thetax", None)
        self.__dict__.pop("thetay", None)
        ss0, jac = self._map(False)
        ss = torch.empty_like(ss0)
        lss = torch.empty_like(ss0)
        _lib.call("scint_bright_fold", ss0, ntd, nfd, ss, lss, device.stream_ptr())
        type(self).jacobian.park(self, jac)
        type(self).SS.park(self, ss)
        type(self).LSS.park(self, lss)

    def calc_acf(self):
        """``acf = real(fftshift(fft2(fftshift(SS))))`` over its ``np.max`` (scint_sim.py:953-958)."""
        ntd, nfd = type(self).SS.shape(self)
        self._check_axis("the delay axis td = arange(-nt, nt, dt)", ntd)
        self._check_axis("the Doppler axis fd = arange(-nf, nf, df)", nfd)
        acf = fft2_any(type(self).SS.tensor(self), in_shift="fftshift", out_shift="fftshift", out="real")
        ws = device.workspace_for("scint_divide_by_max")
        _lib.call("scint_divide_by_max", acf, acf.numel(), ws, ws.numel(), device.stream_ptr())
        type(self).acf.park(self, acf)

    def __getattr__(self, name):                                         # thetax / thetay / X / Y: produced on first access
        if name in ("thetax", "thetay") and "fd" in self.__dict__:
            _, _, thx, thy = self._map(True)
            self.__dict__["thetax"], self.__dict__["thetay"] = thx.cpu().numpy(), thy.cpu().numpy()
            return self.__dict__[name]
        if name in ("X", "Y") and "x" in self.__dict__:
            self.__dict__["X"], self.__dict__["Y"] = np.meshgrid(self.x, self.x)
            return self.__dict__[name]
        raise AttributeError(f"'{type(self).__name__}' object has no attribute '{name}'")

    def plot_acf_efield(self, *args, **kwargs):
        warnings.warn("Brightness.plot_acf_efield: plotting is outside the accelerated hot path; nothing is drawn")

    def plot_brightness(self, *args, **kwargs):
        warnings.warn("Brightness.plot_brightness: plotting is outside the accelerated hot path; nothing is drawn")

    def plot_sspec(self, *args, **kwargs):
        warnings.warn("Brightness.plot_sspec: plotting is outside the accelerated hot path; nothing is drawn")

    def plot_acf(self, *args, **kwargs):
        warnings.warn("Brightness.plot_acf: plotting is outside the accelerated hot path; nothing is drawn")

    def plot_cuts(self, *args, **kwargs):
        warnings.warn("Brightness.plot_cuts: plotting is outside the accelerated hot path; nothing is drawn")
