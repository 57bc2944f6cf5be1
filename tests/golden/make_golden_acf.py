#!/usr/bin/env python
"""Generate tests/golden/acf.npz by running the UNMODIFIED reference's theoretical 2-D ACF (scintools/scint_sim.py:417-766, ACF) and
its residual scint_models.scint_acf_model_2d (scintools/scint_models.py:164-215) with the stand-ins of tests/golden/refshim, as
make_golden_sim.py does.

    SCINTOOLS_REFERENCE=<checkout of the reference> python tests/golden/make_golden_acf.py

ACF uses np.complex_, which NumPy 2 removed: this process (only) sets np.complex_ = np.complex128 before importing the reference.
Inputs: the cases of tests/acf_cases.py.  Stored per case `<case>_<name>`: acf, acf_efield, fn, tn, sn, snp and the scalar
attributes; for the cases of acf_cases.MODEL_CASES also `<case>_resid`, the residual for the seeded ydata and weights of
acf_cases.model_inputs.  The reference's host timing is taken by tests/golden/time_reference_acf.py."""
import os
import sys
import time
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "refshim"))
sys.path.insert(0, os.environ["SCINTOOLS_REFERENCE"])
sys.path.insert(0, os.path.join(REPO, "tests"))

import matplotlib  # noqa: E402
matplotlib.use("Agg")
import numpy as np  # noqa: E402
if not hasattr(np, "complex_"):
    np.complex_ = np.complex128
from scintools.scint_sim import ACF  # noqa: E402
from scintools.scint_models import scint_acf_model_2d  # noqa: E402
import acf_cases as ac  # noqa: E402

warnings.simplefilter("ignore")


class Parameters:
    """What scint_acf_model_2d reads of an lmfit.Parameters."""

    def __init__(self, values):
        self.values = dict(values)

    def valuesdict(self):
        return dict(self.values)


if __name__ == "__main__":
    arrs = {}
    for case in ac.CASES:
        t0 = time.perf_counter()
        a = ACF(**ac.kwargs(case))
        secs = time.perf_counter() - t0
        for k in ac.ARRAYS + ac.SCALARS:
            arrs[f"{case}_{k}"] = np.asarray(getattr(a, k))
        print(case, f"{secs * 1e3:.1f} ms", "acf", a.acf.shape, "efield", a.acf_efield.shape, "max", a.acf.max())
    for case in ac.MODEL_CASES:
        pars, ydata, weights = ac.model_inputs(case)
        arrs[f"{case}_resid"] = scint_acf_model_2d(Parameters(pars), ydata, weights.copy())
        print(case, "residual", arrs[f"{case}_resid"].shape)
    path = os.path.join(HERE, "acf.npz")
    np.savez_compressed(path, **arrs)
    print(f"acf.npz: {os.path.getsize(path) / 1024:.0f} KiB, {len(arrs)} arrays")
