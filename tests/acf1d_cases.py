"""Inputs of the 1-D ACF fit tests (tests/test_gpu_acf1d.py, tests/test_acf1d_emu_cpu.py, tests/test_acf1d_cpu.py) and of
tests/golden/make_acf1d_tolerances.py -- TEST INFRASTRUCTURE.  Everything is seeded and made with NumPy alone.

Two kinds of ACF stack:

  (a) known answers: the two central cuts are generated exactly from the model (scint_models.py:62-120) with chosen (tau, dnu, amp,
      alpha) over the samples the crop keeps, plus a white-noise spike at lag 0, embedded in a smooth ACF.  The crop length follows
      from the start values, which follow from the cut, so the builder iterates to the crop that reproduces itself;
  (b) realistic: ACFs (oracle/sspec_oracle.calc_acf) of small dynamic spectra |E|^2 of a complex Gaussian field with exponential
      correlations, plus white noise -- and one hand-made stack whose middle ACF decays so slowly that it never crosses 1/e.

The shapes are the smallest at which the kernel (one wavefront per problem, four problems per workgroup, lane j % 64 owns sample
j, the Bartlett scan runs 64 samples at a time) can still go wrong:

  floor5     (a) B = 5 (one more than a workgroup's four), 16 x 16, nscale=2: cuts of 8, the crop's floor of 6 samples
  wave65     (a) B = 2, 130 x 130, full_frame: cuts of 65 = one more than a wavefront; alpha varies (planted 2 and 1.5)
  odd        (a) B = 3, 37 x 51: odd R and C (cuts of 19 and 26), bartlett=False
  long       (a) B = 2, 20 x 6000, full_frame: a time cut of 3000 samples -- 47 chunks of the scan and of every pass
  real12     (b) B = 12, 64 x 96; also with alpha varying, weighted=False and bartlett=False
  real300    (b) B = 300, 48 x 64
  nocross    (b) B = 3, 24 x 40: no 1/e crossing in the middle problem (the tobs fallback, the whole cut kept) between ordinary ones
"""
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import acf1d_oracle as ao  # noqa: E402

DT, DF = 30.0, 0.5
FIT_KEYS = ("tau", "dnu", "amp", "alpha")
ERR_KEYS = ("tauerr", "dnuerr", "amperr", "alphaerr")


def _case(stack, kind, planted=None, bw=None, tobs=None, **kw):
    B, R, C = stack.shape
    return types.SimpleNamespace(stack=np.ascontiguousarray(stack), kind=kind, planted=planted, dt=DT, df=DF,
                                 bw=(R // 2) * DF if bw is None else bw, tobs=(C // 2) * DT if tobs is None else tobs, kw=kw)


# ---- kind (a) ---------------------------------------------------------------------------------------------------------------
def _model_cut(n_full, n, step, scale, amp, alpha, wn, half_power):
    """The model over the first n samples (triangle to the n-th), zero beyond, the white-noise spike at lag 0."""
    x = step * np.arange(n)
    y = np.zeros(n_full)
    arg = x * np.log(2) / scale if half_power else (x / scale) ** alpha
    y[:n] = amp * np.exp(-arg) * (1 - x / x.max())
    y[0] += wn
    return y


def planted_acf(R, C, tau, dnu, amp, alpha, wn, full_frame=False, nscale=5):
    """An ACF [R, C] whose central cuts are exactly the model at (tau, dnu, amp, alpha) over the samples the crop keeps."""
    r = DF * np.abs(np.arange(R) - R // 2)[:, None]
    c = DT * np.abs(np.arange(C) - C // 2)[None, :]
    acf = 0.5 * amp * np.exp(-(c / tau) ** alpha) * np.exp(-r * np.log(2) / dnu)          # the smooth surroundings
    ntc, nfc = C - C // 2, R - R // 2
    nt, nf = ntc, nfc
    for _ in range(20):
        acf[R // 2, C // 2:] = _model_cut(ntc, nt, DT, tau, amp, alpha, wn, False)
        acf[R // 2:, C // 2] = _model_cut(nfc, nf, DF, dnu, amp, alpha, wn, True)
        s = ao.setup(acf, DT, DF, (R // 2) * DF, (C // 2) * DT, nscale=nscale, full_frame=full_frame)
        if (len(s["x_t"]), len(s["x_f"])) == (nt, nf):
            return acf
        nt, nf = len(s["x_t"]), len(s["x_f"])
    raise AssertionError("planted_acf: the crop does not settle")


def _planted(R, C, params, **kw):
    fit_kw = {k: v for k, v in kw.items() if k in ("full_frame", "nscale")}
    stack = np.stack([planted_acf(R, C, *p, **fit_kw) for p in params])
    return _case(stack, "a", planted=np.array([p[:4] for p in params]), **kw)


# ---- kind (b) ---------------------------------------------------------------------------------------------------------------
def realistic_dyn(rng, nf, nt, lf, lt, noise):
    """|E|^2 of a complex Gaussian field with exponential correlations (lengths lf channels, lt samples), plus white noise."""
    pf, pt = 4 * nf, 4 * nt
    kf = 2 * np.pi * np.fft.fftfreq(pf)[:, None]
    kt = 2 * np.pi * np.fft.fftfreq(pt)[None, :]
    power = 1 / (1 + (kf * lf) ** 2) / (1 + (kt * lt) ** 2)
    white = rng.normal(size=(pf, pt)) + 1j * rng.normal(size=(pf, pt))
    field = np.fft.ifft2(white * np.sqrt(power))[:nf, :nt]
    dyn = np.abs(field) ** 2
    dyn /= dyn.mean()
    return dyn + noise * rng.normal(size=dyn.shape)


def _realistic(seed, B, nf, nt, lf, lt, noise, **kw):
    from oracle import sspec_oracle
    rng = np.random.default_rng(seed)
    stack = np.stack([sspec_oracle.calc_acf(realistic_dyn(rng, nf, nt, lf, lt, noise)) for _ in range(B)])
    return _case(stack, "b", **kw)


def _nocross():
    """Three ACFs whose cuts are the model over the whole cut plus 1e-3 noise; in the middle one the lag-1 samples are depressed
    (the start amplitude max(y_f[1], y_t[1]) is then 0.02) and nothing lies below 0.012, so neither cut crosses amp/e or amp/2:
    tau starts at tobs, dnu at bw, and the crop keeps everything."""
    R, C = 24, 40
    rng = np.random.default_rng(11)
    stack = np.stack([planted_acf(R, C, 150.0, 1.4, 0.8, 5/3, 0.2, full_frame=(b == 1)) for b in range(3)])
    stack += 1e-3 * rng.normal(size=stack.shape)
    yt, yf = stack[1, R // 2, C // 2:], stack[1, R // 2:, C // 2]        # views
    yt[1], yf[1] = 0.02, 0.015
    np.maximum(yt, 0.012, out=yt)
    np.maximum(yf, 0.012, out=yf)
    s = ao.setup(stack[1], DT, DF, (R // 2) * DF, (C // 2) * DT)
    assert s["tau"] == (C // 2) * DT and s["dnu"] == (R // 2) * DF and len(s["x_t"]) == C - C // 2
    return _case(stack, "b")


_BUILDERS = {
    "floor5": lambda: _planted(16, 16, [(25.0, 0.40, 0.8, 5/3, 0.2), (28.0, 0.45, 0.9, 5/3, 0.1), (20.0, 0.35, 0.7, 5/3, 0.3),
                                        (18.0, 0.30, 1.0, 5/3, 0.0), (22.0, 0.42, 0.6, 5/3, 0.4)], nscale=2),
    "wave65": lambda: _planted(130, 130, [(400.0, 6.0, 0.8, 2.0, 0.2), (300.0, 8.0, 0.9, 1.5, 0.1)], full_frame=True, alpha=None),
    "odd": lambda: _planted(37, 51, [(100.0, 1.5, 0.8, 5/3, 0.2), (75.0, 1.1, 0.9, 5/3, 0.1), (130.0, 2.0, 0.7, 5/3, 0.3)],
                            bartlett=False),
    "long": lambda: _planted(20, 6000, [(9000.0, 1.2, 0.8, 5/3, 0.2), (20000.0, 0.9, 0.9, 5/3, 0.1)], full_frame=True),
    "real12": lambda: _realistic(5, 12, 32, 48, 2.5, 3.5, 0.1),
    "real12_alpha": lambda: _realistic(5, 12, 32, 48, 2.5, 3.5, 0.1, alpha=None),
    "real12_unweighted": lambda: _realistic(5, 12, 32, 48, 2.5, 3.5, 0.1, weighted=False),
    "real12_nobartlett": lambda: _realistic(5, 12, 32, 48, 2.5, 3.5, 0.1, bartlett=False),
    "real300": lambda: _realistic(7, 300, 24, 32, 2.0, 3.0, 0.05),
    "nocross": _nocross,
}
CASES = tuple(_BUILDERS)
_cache = {}


def case(name):
    """The case `name` (built once, then shared: do not write into its arrays)."""
    if name not in _cache:
        _cache[name] = _BUILDERS[name]()
    return _cache[name]


def oracle(name):
    """(setups, fits) of the host oracle for every problem of the case (computed once)."""
    key = ("oracle", name)
    if key not in _cache:
        c = case(name)
        kw = dict(c.kw)
        alpha = kw.pop("alpha", 5/3)
        _cache[key] = ao.fit_stack(c.stack, c.dt, c.df, c.bw, c.tobs, alpha=alpha, **kw)
    return _cache[key]


def observation(rng_seed=21, nf=32, nt=48):
    """A kind (b) observation for Dynspec.fit_scint_params and fit_scint_params_cut."""
    import scintpar_cases
    dyn = realistic_dyn(np.random.default_rng(rng_seed), nf, nt, 2.5, 3.5, 0.1)
    return scintpar_cases.observation(dyn, 1400.0 + DF * np.arange(nf), DT * np.arange(nt), DF, DT, 1400.0 + DF * nf / 2, "acf1d")
