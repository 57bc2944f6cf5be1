#!/usr/bin/env python
"""Generate tests/golden/scatim.npz by running the UNMODIFIED reference's Dynspec.calc_scattered_image (scintools/dynspec.py:
3412-3582) with the stand-ins of tests/golden/refshim, as the other make_golden_* scripts do.

    SCINTOOLS_REFERENCE=<checkout of the reference> python tests/golden/make_golden_scatim.py

Inputs: the seeded screen and field of tests/scatim_cases.py (regenerated here and by the tests, not stored).  Stored per case
`<case>_<name>`: scattered_image, scattered_image_ax, eta (the curvature the reference used: its input, its corner fallback, or
its own fit_arc's betaeta converted by its lines; for the latter also betaeta) and crop = (row0, row1, col0, col1), the reference's
crop lines applied to that curvature.  The reference draws the image when plot_log is True (its default): the Agg backend swallows it."""
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
from scintools.dynspec import Dynspec  # noqa: E402
import scatim_cases as sc  # noqa: E402
import scatim_oracle as so  # noqa: E402

warnings.simplefilter("ignore")

if __name__ == "__main__":
    arrs = {}
    for case in sc.CASES:
        kw = sc.call_kwargs(case)
        d = Dynspec(dyn=sc.sim(), process=False, verbose=False)
        d.dyn = np.array(d.dyn, dtype=np.float64)
        d.calc_scattered_image(plot_log=False, **kw)
        if "input_sspec" in kw:
            fdop, tdel, shape = kw["input_fdop"], kw["input_tdel"], kw["input_sspec"].shape
        else:
            fdop, tdel = d.fdop, d.tdel
            shape = (d.lamsspec if kw.get("lamsteps") else d.sspec).shape
        if "input_eta" in kw:
            eta = kw["input_eta"]
        elif kw.get("fit_arc", True):
            eta = so.beta_to_eta(d.betaeta, d.freq) if kw.get("lamsteps") else d.eta
            if kw.get("lamsteps"):
                arrs[f"{case}_betaeta"] = np.asarray(d.betaeta)
        else:
            eta = tdel[-1] / fdop[-1]**2
        rows, cols, _, _, flim = so.crop(np.asarray(fdop, dtype=float), np.asarray(tdel, dtype=float), eta)
        r, c = range(shape[0])[rows], range(shape[1])[cols]
        arrs[f"{case}_eta"] = np.asarray(eta, dtype=float)
        arrs[f"{case}_crop"] = np.array([r.start, r.stop, c.start, c.stop])
        for k in sc.STORED:
            arrs[f"{case}_{k}"] = np.asarray(getattr(d, k))
        im = d.scattered_image
        print(case, "eta", float(eta), "flim", flim, "crop", arrs[f"{case}_crop"], "image", im.shape, "max", np.nanmax(im),
              "finite", np.isfinite(im).all())
    path = os.path.join(HERE, "scatim.npz")
    np.savez_compressed(path, **arrs)
    print(f"scatim.npz: {os.path.getsize(path) / 1024:.0f} KiB, {len(arrs)} arrays")
