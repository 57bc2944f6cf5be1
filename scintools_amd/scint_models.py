"""Model residuals for fitting (scint_models.py of the reference).  Only ``scint_acf_model_2d`` (scint_models.py:164-215), the
residual that ``get_scint_params(method='acf2d')`` hands to its optimiser: the theoretical 2-D ACF comes from the device
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
