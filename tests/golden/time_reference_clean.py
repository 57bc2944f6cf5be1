#!/usr/bin/env python
"""How long do the UNMODIFIED reference's Dynspec.zap, refill(method='median') and correct_dyn() (scintools/dynspec.py:3856-3870,
3273-3323, 3325-3410) take on the host?

    SCINTOOLS_REFERENCE=<checkout of the reference> python tests/golden/time_reference_clean.py [--sizes 1024 4096]

Wall time of each method on a seeded positive 1024^2 and 4096^2 dynamic spectrum (the generator of tools/time_clean.py: 2 % of the
pixels flagged NaN for refill, 0.1 % spikes for zap), one run each, with the stand-ins of tests/golden/refshim.  correct_dyn() is
the default svd=True, nmodes=1: a full numpy.linalg.svd.  Writes tests/golden/clean_timing.json, which DESIGN.md quotes beside the
device figures."""
import argparse
import json
import os
import sys
import time
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "refshim"))
sys.path.insert(0, os.environ["SCINTOOLS_REFERENCE"])
sys.path.insert(0, os.path.join(REPO, "tools"))

import matplotlib  # noqa: E402
matplotlib.use("Agg")
from scintools.dynspec import Dynspec  # noqa: E402
from time_clean import workload  # noqa: E402

warnings.simplefilter("ignore")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    args = ap.parse_args()
    out = {"what": "wall time in seconds of the unmodified reference's zap(), refill(method='median', kernel_size=5) and "
                   "correct_dyn() on the host (refshim stand-ins), one process, one run each", "host_cores": os.cpu_count(),
           "cases": {}}
    for size in args.sizes:
        rec = {}
        for name, call in (("zap", lambda d: d.zap()), ("refill_median", lambda d: d.refill(method="median", kernel_size=5)),
                           ("correct_dyn", lambda d: d.correct_dyn())):
            d = Dynspec.__new__(Dynspec)
            d.dyn = workload(size, name)
            t0 = time.perf_counter()
            call(d)
            rec[name] = round(time.perf_counter() - t0, 3)
            print(size, name, rec[name], flush=True)
        out["cases"][str(size)] = rec
    with open(os.path.join(HERE, "clean_timing.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
