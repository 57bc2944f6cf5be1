#!/usr/bin/env python
"""Generate tests/golden/sim.npz by running the UNMODIFIED reference's screen simulator
(scintools/scint_sim.py:23-311, Simulation) with the stand-ins of tests/golden/refshim, as make_golden_rotmos.py does.

    SCINTOOLS_REFERENCE=<checkout of the reference> python tests/golden/make_golden_sim.py

Inputs: the cases of tests/sim_cases.py (seed 7).  Stored per case `<case>_<name>`: xyp, w, spe, spi, xyi, dyn, pulsewin, dm, freqs, times,
x, lams, the scalar attributes, and `<case>_name` (the object's name).  The reference's host timing is taken by
tests/golden/time_reference_sim.py."""
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
from scintools.scint_sim import Simulation  # noqa: E402
import sim_cases as sc  # noqa: E402

warnings.simplefilter("ignore")


if __name__ == "__main__":
    arrs = {}
    for case in sc.CASES:
        t0 = time.perf_counter()
        s = Simulation(**sc.kwargs(case))
        secs = time.perf_counter() - t0
        for k in sc.ARRAYS:
            arrs[f"{case}_{k}"] = np.asarray(getattr(s, k))
        for k in sc.SCALARS:
            arrs[f"{case}_{k}"] = np.asarray(getattr(s, k))
        arrs[f"{case}_name"] = np.asarray(s.name)
        print(case, f"{secs * 1e3:.1f} ms", "max|xyp|", np.abs(s.xyp).max(), "dyn", s.dyn.shape, s.dyn.dtype, "spe", s.spe.dtype)
    path = os.path.join(HERE, "sim.npz")
    np.savez_compressed(path, **arrs)
    print(f"sim.npz: {os.path.getsize(path) / 1024:.0f} KiB, {len(arrs)} arrays")
