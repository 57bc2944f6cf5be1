#!/usr/bin/env python
"""How long does the UNMODIFIED reference's theoretical 2-D ACF (scintools/scint_sim.py:417-766, ACF) take on the host?

    SCINTOOLS_REFERENCE=<checkout of the reference> python tests/golden/time_reference_acf.py [--samples 3] [--big-limit 300]

Wall time of the constructor for the cases of tools/time_acf.py -- the default size, ar=3, and ar=3 with a phase gradient: the median
of `--samples` runs in one process -- with the stand-ins of tests/golden/refshim and np.complex_ = np.complex128 set in this process
(the reference does not run on NumPy 2 otherwise).  ar=10 (1626^2 / 6501^2 grid points, about 2e9 complex exponentials) runs once in a
child process under `--big-limit` seconds and is recorded as not run if it does not finish.  Writes tests/golden/acf_timing.json,
which DESIGN.md quotes beside the device figures of tools/time_acf.py."""
import argparse
import json
import os
import subprocess
import sys
import time
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "refshim"))
sys.path.insert(0, os.environ["SCINTOOLS_REFERENCE"])

import matplotlib  # noqa: E402
matplotlib.use("Agg")
import numpy as np  # noqa: E402
if not hasattr(np, "complex_"):
    np.complex_ = np.complex128
from scintools.scint_sim import ACF  # noqa: E402

warnings.simplefilter("ignore")

CASES = {"default": dict(), "ar3": dict(ar=3), "ar3_phasegrad": dict(ar=3, phasegrad=0.5, theta=30)}
BIG = dict(ar=10)


def once(kw):
    t0 = time.perf_counter()
    ACF(**kw)
    return round(time.perf_counter() - t0, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--big-limit", type=float, default=300.0)
    ap.add_argument("--child-big", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child_big:
        print(json.dumps(once(BIG)))
        return
    out = {"what": "wall time of the unmodified reference's scint_sim.ACF on the host (refshim stand-ins, np.complex_ restored), one process",
           "host_cores": os.cpu_count(), "cases": {}}
    for name, kw in CASES.items():
        secs = [once(kw) for _ in range(args.samples)]
        out["cases"][name] = {"kwargs": kw, "seconds": round(float(np.median(secs)), 3), "samples": secs}
        print(name, secs, flush=True)
    try:
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-big"], capture_output=True, text=True,
                             timeout=args.big_limit)
        if res.returncode == 0:
            out["cases"]["ar10"] = {"kwargs": BIG, "seconds": json.loads(res.stdout.strip().splitlines()[-1]), "samples": 1}
        else:
            out["cases"]["ar10"] = {"kwargs": BIG, "not_run": "the reference failed (exit status %d), most likely for memory" % res.returncode}
    except subprocess.TimeoutExpired:
        out["cases"]["ar10"] = {"kwargs": BIG, "not_run": "did not finish within %.0f s" % args.big_limit}
    print("ar10", out["cases"]["ar10"], flush=True)
    with open(os.path.join(HERE, "acf_timing.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
