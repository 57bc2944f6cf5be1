#!/usr/bin/env python
"""Generate tests/golden/brightness_<case>.npz by running the UNMODIFIED reference's brightness-distribution model
(scintools/scint_sim.py:768-958, Brightness) with the stand-ins of tests/golden/refshim, as make_golden_acf.py does.

    SCINTOOLS_REFERENCE=<checkout of the reference> python tests/golden/make_golden_brightness.py

Inputs: the cases of tests/brightness_cases.py.  Stored per case: every constructor argument as `arg_<name>`, the reference's
B, SS, jacobian, thetax, thetay and acf, and `diagonals`: the bit per grid cell of the triangulation that scipy.spatial.Delaunay gave
for the grid points IN THE SAME RUN (the call, with its defaults, that the reference's griddata makes; Qhull is deterministic), so
that a test can pass it to Brightness(diagonals=...) whatever scipy it runs on.  Data only.  `--time-defaults` instead times the
reference once at its default sizes (grid 600 x 600, spectrum 2000 x 1000) and writes nothing."""
import os
import sys
import time
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "refshim"))
sys.path.insert(0, os.environ["SCINTOOLS_REFERENCE"])
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)

import matplotlib  # noqa: E402
matplotlib.use("Agg")
import numpy as np  # noqa: E402
if not hasattr(np, "complex_"):
    np.complex_ = np.complex128
import scipy  # noqa: E402
from scintools.scint_sim import Brightness  # noqa: E402
import brightness_cases as bc  # noqa: E402
from scintools_amd.scint_sim import qhull_diagonals  # noqa: E402

warnings.simplefilter("ignore")

if __name__ == "__main__":
    if "--time-defaults" in sys.argv:
        t0 = time.perf_counter()
        b = Brightness()
        print(f"reference Brightness() at the defaults: {time.perf_counter() - t0:.1f} s, grid {b.B.shape}, spectrum {b.SS.shape}")
        sys.exit(0)
    for case in bc.CASES:
        kw = bc.kwargs(case)
        t0 = time.perf_counter()
        b = Brightness(**kw)
        secs = time.perf_counter() - t0
        arrs = {f"arg_{k}": np.asarray(v) for k, v in kw.items()}
        for k in bc.ARRAYS:
            arrs[k] = np.asarray(getattr(b, k))
        arrs["diagonals"] = qhull_diagonals(b.x)
        arrs["scipy_version"] = np.asarray(scipy.__version__)
        assert (len(b.x), len(b.td), len(b.fd)) == bc.SHAPES[case]
        path = os.path.join(HERE, f"brightness_{case}.npz")
        np.savez_compressed(path, **arrs)
        print(case, f"{secs:.1f} s", "grid", b.B.shape, "spectrum", b.SS.shape, "NaN", int(np.isnan(b.SS).sum()),
              "main-diagonal cells", float(arrs["diagonals"].mean()), f"{os.path.getsize(path) / 1024:.0f} KiB")
