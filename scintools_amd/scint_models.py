"""Models of the reference's scint_models.py that this package needs: ``effective_velocity_annual`` (scint_models.py:504-587, host
NumPy, for ``Dynspec.scale_dyn(scale='velocity')``) and ``scint_acf_model_2d`` (scint_models.py:164-215), the residual that
``get_scint_params(method='acf2d')`` hands to its optimiser: the theoretical 2-D ACF comes from the device
(``scint_sim.ACF``, a fresh one at every evaluation as in the reference), the triangle functions and the weights are the
reference's NumPy lines.  ``params`` is anything with ``valuesdict()`` (an ``lmfit.Parameters``) or a plain mapping; lmfit is not
needed."""
import numpy as np

from .scint_sim import ACF


def scint_acf_model_2d(params, ydata, weights):
    """Fit an analytical 2D ACF function: ``(ydata - model) * weights`` with the weight of the white-noise pixel zeroed."""
    parvals = params.valuesdict() if hasattr(params, "valuesdict") else params

    tau = np.abs(parvals['tau'])
    dnu = np.abs(parvals['dnu'])
    alpha = parvals['alpha']
    ar = np.abs(parvals['ar'])
    psi = parvals['psi']
    phasegrad = parvals['phasegrad']
    theta = parvals['theta']
    amp = parvals['amp']

    tobs = parvals['tobs']
    bw = parvals['bw']
    nt = parvals['nt']
    nf = parvals['nf']
    nf_crop, nt_crop = np.shape(ydata)

    dt, df = 2 * tobs / nt, 2 * bw / nf
    taumax = nt_crop * dt / tau
    dnumax = nf_crop * df / dnu

    acf = ACF(taumax=taumax, dnumax=dnumax, nt=nt_crop, nf=nf_crop, ar=ar, alpha=alpha, phasegrad=phasegrad, theta=theta,
              amp=amp, psi=psi)
    model = acf.acf

    triangle_t = 1 - np.divide(np.tile(np.abs(np.linspace(-taumax * tau, taumax * tau, nt_crop)), (nf_crop, 1)), tobs)
    triangle_f = np.transpose(1 - np.divide(np.tile(np.abs(np.linspace(-dnumax * dnu, dnumax * dnu, nf_crop)), (nt_crop, 1)), bw))
    triangle = np.multiply(triangle_t, triangle_f)
    model = np.multiply(model, triangle)  # multiply by triangle function

    if weights is None:
        weights = np.ones(np.shape(ydata))

    weights = np.fft.fftshift(weights)
    weights[-1, -1] = 0  # Not fitting for the white noise spike
    weights = np.fft.ifftshift(weights)

    return (ydata - model) * weights


def scint_acf_model_2d_approx(params, tdata, fdata, ydata, weights):
    """Fit an approximate 2D ACF function (scint_models.py:123-161): ``(ydata - model) * weights`` [nf, nt] with the weight of the
    white-noise pixel zeroed, evaluated on the device (``scint_acf2d_approx_model``) and returned as a host array.  ``params``
    holds ``amp, dnu, tau, alpha, phasegrad`` (min/MHz), ``tobs, bw``."""
    from . import scintpar
    parvals = params.valuesdict() if hasattr(params, "valuesdict") else params
    out = scintpar.acf2d_approx_model_device(tdata, fdata, ydata, weights, parvals['tau'], parvals['dnu'], parvals['amp'],
                                             parvals['alpha'], parvals['phasegrad'], parvals['tobs'], parvals['bw'])
    return out.cpu().numpy()


def effective_velocity_annual(params, true_anomaly, vearth_ra, vearth_dec, mjd=None):
    """Effective velocity with the annual and the pulsar's orbital and proper-motion terms, in RA and DEC, km/s
    (scint_models.py:504-587).  The ISM velocity is NOT included; the result is in the ISM's frame.  `params` is a dictionary
    with the tempo2 names in capitals (A1, PB, ECC, OM[, OMDOT, T0], KIN | COSI | SINI, KOM, PMRA, PMDEC) and ``s``
    (fractional screen distance), ``d`` (pulsar distance, kpc) in lower case.  Host NumPy: one number per sub-integration, in
    the precision of the inputs.  Returns (veff_ra, veff_dec, vp_ra, vp_dec)."""
    v_c = 299792.458  # km/s
    kmpkpc = 3.085677581e16
    secperyr = 86400 * 365.2425
    masrad = np.pi / (3600 * 180 * 1000)

    if 'PB' in params.keys():
        A1 = params['A1']  # projected semi-major axis in lt-s
        PB = params['PB']  # orbital period in days
        ECC = params['ECC']  # orbital eccentricity
        OM = params['OM'] * np.pi / 180  # longitude of periastron rad
        if 'OMDOT' in params.keys():
            if mjd is None:
                print('Warning, OMDOT present but no mjd for calculation')
                omega = OM
            else:
                omega = OM + params['OMDOT'] * np.pi / 180 * (mjd - params['T0']) / 365.2425
        else:
            omega = OM
        # (the fifth Keplerian parameter T0 went into the true anomaly)
        if 'KIN' in params.keys():
            INC = params['KIN'] * np.pi / 180  # inclination
        elif 'COSI' in params.keys():
            INC = np.arccos(params['COSI'])
        elif 'SINI' in params.keys():
            INC = np.arcsin(params['SINI'])
        else:
            print('Warning: inclination parameter (KIN, COSI, or SINI) not found')
        if 'sense' in params.keys():
            sense = params['sense']
            if sense < 0.5:  # KIN < 90
                if INC > np.pi / 2:
                    INC = np.pi - INC
            if sense >= 0.5:  # KIN > 90
                if INC < np.pi / 2:
                    INC = np.pi - INC
        KOM = params['KOM'] * np.pi / 180  # longitude ascending node
        # pulsar velocity along the line of nodes (x) and perpendicular to it in the plane of the sky (y)
        vp_0 = (2 * np.pi * A1 * v_c) / (np.sin(INC) * PB * 86400 * np.sqrt(1 - ECC**2))
        vp_x = -vp_0 * (ECC * np.sin(omega) + np.sin(true_anomaly + omega))
        vp_y = vp_0 * np.cos(INC) * (ECC * np.cos(omega) + np.cos(true_anomaly + omega))
    else:
        vp_x = 0
        vp_y = 0

    if 'PMRA' in params.keys():
        PMRA = params['PMRA']  # proper motion in RA
        PMDEC = params['PMDEC']  # proper motion in DEC
    else:
        PMRA = 0
        PMDEC = 0

    s = params['s']  # fractional screen distance
    d = params['d'] * kmpkpc  # pulsar distance in km
    pmra_v = PMRA * masrad * d / secperyr
    pmdec_v = PMDEC * masrad * d / secperyr

    # rotate the pulsar velocity into RA/DEC (KOM is defined with PB only, as in the reference)
    vp_ra = np.sin(KOM) * vp_x + np.cos(KOM) * vp_y
    vp_dec = np.cos(KOM) * vp_x - np.sin(KOM) * vp_y

    veff_ra = s * vearth_ra + (1 - s) * (vp_ra + pmra_v)
    veff_dec = s * vearth_dec + (1 - s) * (vp_dec + pmdec_v)
    return veff_ra, veff_dec, vp_ra, vp_dec
