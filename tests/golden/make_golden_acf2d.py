#!/usr/bin/env python
"""Generate tests/golden/acf2d_approx.npz by running the UNMODIFIED reference's scint_models.scint_acf_model_2d_approx
(scintools/scint_models.py:123-161) with the stand-ins of tests/golden/refshim and a dict-like `params`.

    SCINTOOLS_REFERENCE=<checkout of the reference> python tests/golden/make_golden_acf2d.py

Inputs: the seeded windows of tests/acf2d_checks.golden_inputs (3 x 3, 21 x 31, 19 x 5).  Stored per window `<name>_w` (with
weights) and `<name>_n` (weights=None): the residual.  Only these outputs are stored; the inputs are regenerated from the seed."""
import os
import sys
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
from scintools.scint_models import scint_acf_model_2d_approx  # noqa: E402
import acf2d_checks as ck  # noqa: E402

warnings.simplefilter("ignore")


class Parameters:
    """What scint_acf_model_2d_approx reads of an lmfit.Parameters."""

    def __init__(self, values):
        self.values = dict(values)

    def valuesdict(self):
        return dict(self.values)


if __name__ == "__main__":
    arrs = {}
    for name in ck.GOLDEN_CASES:
        pars, tdata, fdata, ydata, weights = ck.golden_inputs(name)
        arrs[name + "_w"] = scint_acf_model_2d_approx(Parameters(pars), tdata, fdata, ydata, weights.copy())
        arrs[name + "_n"] = scint_acf_model_2d_approx(Parameters(pars), tdata, fdata, ydata, None)
        print(name, arrs[name + "_w"].shape)
    path = os.path.join(HERE, "acf2d_approx.npz")
    np.savez_compressed(path, **arrs)
    print(f"acf2d_approx.npz: {os.path.getsize(path) / 1024:.0f} KiB, {len(arrs)} arrays")
