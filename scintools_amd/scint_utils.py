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

__all__ = ["slow_FT", "svd_model", "is_valid", "get_window", "read_par", "get_true_anomaly", "get_ssb_delay",
           "get_earth_velocity"]


# ---- what Dynspec.scale_dyn(scale='velocity') asks of this module (dynspec.py:3963-3992): host NumPy / SciPy ----------------
def _astropy(what):
    try:
        import astropy  # noqa: F401
    except ImportError:
        raise ImportError(f"{what} needs astropy (the solar-system ephemeris); without it, pass your own velocities to "
                          "scintools_amd.arcfit.velocity_resample_device") from None


def get_ssb_delay(mjds, raj, decj, message=True):
    """Roemer delay to the solar-system barycentre in seconds, to be ADDED to site arrival times (scint_utils.py:286-311)."""
    _astropy("get_ssb_delay")
    from astropy import units as u
    from astropy.constants import au, c
    from astropy.coordinates import BarycentricTrueEcliptic, SkyCoord, get_body_barycentric
    from astropy.time import Time

    coord = SkyCoord('{0} {1}'.format(raj, decj), frame=BarycentricTrueEcliptic, unit=(u.hourangle, u.deg))
    psr_xyz = coord.cartesian.xyz.value
    t = []
    for mjd in mjds:
        earth_xyz = get_body_barycentric('earth', Time(mjd, format='mjd'))
        e_dot_p = np.dot(earth_xyz.xyz.value, psr_xyz)
        t.append(e_dot_p * au.value / c.value)
    if message:
        print('Returned SSB Roemer delays (in seconds) should be ADDED to site arrival times')
    return np.array(t)


def get_earth_velocity(mjds, raj, decj, radial=False):
    """The Earth's velocity transverse to the line of sight in RA and DEC, km/s (and the radial one) (scint_utils.py:349-395)."""
    _astropy("get_earth_velocity")
    from astropy import units as u
    from astropy.constants import au
    from astropy.coordinates import SkyCoord, get_body_barycentric_posvel
    from astropy.time import Time

    coord = SkyCoord('{0} {1}'.format(raj, decj), unit=(u.hourangle, u.deg))
    rarad = coord.ra.value * np.pi / 180
    decrad = coord.dec.value * np.pi / 180
    vearth_ra, vearth_dec, vearth_radial = [], [], []
    for mjd in mjds:
        pos_xyz, vel_xyz = get_body_barycentric_posvel('earth', Time(mjd, format='mjd'))
        vx, vy, vz = vel_xyz.x.value, vel_xyz.y.value, vel_xyz.z.value
        vearth_ra.append(- vx * np.sin(rarad) + vy * np.cos(rarad))
        vearth_dec.append(- vx * np.sin(decrad) * np.cos(rarad) - vy * np.sin(decrad) * np.sin(rarad) + vz * np.cos(decrad))
        vearth_radial.append(vx * np.cos(decrad) * np.cos(rarad) + vy * np.cos(decrad) * np.sin(rarad) + vz * np.sin(decrad))
    # AU/d -> km/s
    vearth_ra = vearth_ra * au / 1e3 / 86400
    vearth_dec = vearth_dec * au / 1e3 / 86400
    if radial:
        vearth_radial = vearth_radial * au / 1e3 / 86400
        return vearth_ra.value.squeeze(), vearth_dec.value.squeeze(), vearth_radial.value.squeeze()
    return vearth_ra.value.squeeze(), vearth_dec.value.squeeze()


_PAR_IGNORE = ('DMMODEL', 'DMOFF', "DM_", "CM_", 'CONSTRAIN', 'JUMP', 'NITS', 'NTOA', 'CORRECT_TROPOSPHERE', 'PLANET_SHAPIRO',
               'DILATEFREQ', 'TIMEEPH', 'MODE', 'TZRMJD', 'TZRSITE', 'TZRFRQ', 'EPHVER', 'T2CMETHOD')


def read_par(parfile):
    """A tempo2 .par file as a dictionary of names and values, with NAME_ERR and NAME_TYPE ('d' integer, 'f' float, 'e' float in
    exponent notation, 's' string) beside them (scint_utils.py:398-450)."""
    from decimal import Decimal, InvalidOperation
    par = {}
    with open(parfile, 'r') as fh:
        lines = fh.readlines()
    for line in lines:
        sline = line.split()
        if len(sline) == 0 or line[0] == "#" or line[0:2] == "C " or sline[0] in _PAR_IGNORE:
            continue
        param = "ECC" if sline[0] == "E" else sline[0]
        val, err, p_type = sline[1], None, None
        if len(sline) == 3 and sline[2] not in ['0', '1']:
            err = sline[2].replace('D', 'E')
        elif len(sline) == 4:
            err = sline[3].replace('D', 'E')
        try:
            val = int(val)
            p_type = 'd'
        except ValueError:
            try:
                val = float(Decimal(val.replace('D', 'E')))
                p_type = 'e' if ('e' in sline[1] or 'E' in sline[1].replace('D', 'E')) else 'f'
            except InvalidOperation:
                p_type = 's'
        par[param] = val
        if err:
            par[param + "_ERR"] = float(err)
        if p_type:
            par[param + "_TYPE"] = p_type
    return par


def get_true_anomaly(mjds, pars):
    """True anomalies for an array of barycentric MJDs and a parameter dictionary (scint_utils.py:509-554); the precision of
    `mjds` is kept (the reference hands over float128), Kepler's equation is solved in float64 by scipy's fsolve."""
    from scipy.optimize import fsolve
    if 'TASC' in pars.keys():
        T0 = pars['TASC']  # MJD
        ECC = np.sqrt(pars['EPS1']**2 + pars['EPS2']**2)
    else:
        T0 = pars['T0']  # MJD
        ECC = pars['ECC']
    PB = pars['PB']  # days
    PBDOT = 0 if 'PBDOT' not in pars.keys() else pars['PBDOT']
    if np.abs(PBDOT) > 1e-10:  # tempo format
        PBDOT *= 10**-12
    nb = 2 * np.pi / PB
    # mean anomaly
    M = nb * ((mjds - T0) - 0.5 * (PBDOT / PB) * (mjds - T0)**2)
    M = M.squeeze()
    # eccentric anomaly
    if ECC < 1e-4:
        E = M
    else:
        M = np.asarray(M, dtype=np.float64)
        E = []
        for m in M:
            E.append(fsolve(lambda E: E - ECC * np.sin(E) - m, m))
        E = np.asarray(E, dtype=np.longdouble)
    # true anomaly
    U = 2 * np.arctan2(np.sqrt(1 + ECC) * np.sin(E / 2), np.sqrt(1 - ECC) * np.cos(E / 2))
    if hasattr(U, "__len__"):
        U[np.argwhere(U < 0)] = U[np.argwhere(U < 0)] + 2 * np.pi
        U = U.squeeze()
    elif U < 0:
        U += 2 * np.pi
    return U


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
