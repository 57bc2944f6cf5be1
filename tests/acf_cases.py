"""The 2-D ACF model's cases shared by tests/golden/make_golden_acf.py (which runs the unmodified reference on them), the host tests
(tests/test_acf_cpu.py), the host-interpreter tests (tests/test_acf_emu_cpu.py) and the GPU tests (tests/test_gpu_acf.py).
Parameters not listed keep the constructor's defaults.  Between them: nsn of 3, 7, 9, 11, 17 and 25 under the phase gradient and 26
without it (below one 16-column group, one past it, two groups), coarse grids of 21 to 76 points and core grids of 41 to 301 (none a
multiple of 16), several 64-row blocks per lag, both quadrant branches."""
CASES = {
    "a": dict(),                                                                                   # defaults: M = 51, M2 = 201
    "b": dict(ar=2, psi=30, nt=31, nf=21),
    "c": dict(phasegrad=0.5, theta=40, ar=1.5, psi=-20, nt=25, nf=25, taumax=3, dnumax=5),         # two quadrants
    "d": dict(auto_sampling=False, nt=20, nf=16, alpha=2, wn=0.3, amp=2.0),                        # the caller's sampling, even sizes
    "e": dict(ar=3, psi=60, alpha=1.2, nt=17, nf=9, phasegrad=1.0, theta=-70),
    "f": dict(nf=3, nt=5),                                                                         # the core lag only, no coarse loop
    "g": dict(ar=0.5, psi=90, taumax=2.7, dnumax=3.3, nt=13, nf=7),                                # non-integer extents, V along x
}

ARRAYS = ("acf", "acf_efield", "fn", "tn", "sn", "snp")
SCALARS = ("alpha", "ar", "psi", "phasegrad", "theta", "amp", "wn", "taumax", "dnumax", "nf", "nt", "sp_fac", "res_fac", "core_fac",
           "dsp", "ddnun")

# scint_acf_model_2d: the parameter set, the shape of ydata (nf_crop, nt_crop) and the seed of ydata / weights, per stored case
MODEL_CASES = {
    "a": (dict(tau=310.0, dnu=0.9, alpha=5 / 3, ar=1.4, psi=25.0, phasegrad=0.0, theta=0.0, amp=1.3, tobs=3600.0, bw=16.0, nt=120,
               nf=64), (11, 15), 11),
    "c": (dict(tau=-250.0, dnu=1.1, alpha=1.5, ar=2.0, psi=-35.0, phasegrad=0.4, theta=50.0, amp=0.8, tobs=3000.0, bw=20.0, nt=100,
               nf=80), (9, 13), 12),
}


def kwargs(case):
    return dict(CASES[case])


def model_inputs(case):
    """(parameter dict, ydata, weights) of a scint_acf_model_2d case: seeded, the same in the golden script and in the tests."""
    import numpy as np
    pars, shape, seed = MODEL_CASES[case]
    rs = np.random.RandomState(seed)
    ydata = rs.rand(*shape)
    weights = 0.5 + rs.rand(*shape)
    return dict(pars), ydata, weights


class Params:
    """Stand-in for lmfit.Parameters: all the model reads is valuesdict()."""

    def __init__(self, values):
        self._values = dict(values)

    def valuesdict(self):
        return dict(self._values)
