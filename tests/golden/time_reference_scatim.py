#!/usr/bin/env python
"""How long does the UNMODIFIED reference's Dynspec.calc_scattered_image (scintools/dynspec.py:3412-3582) take on the host?

    SCINTOOLS_REFERENCE=<checkout of the reference> python tests/golden/time_reference_scatim.py [--sizes 1024 4096] [--samples 3]

Wall time of the method at the spectrum of a 1024^2 and of a 4096^2 dynamic spectrum (1024 x 2048 and 4096 x 8192 float64 in dB: a
seeded field spanning four decades, the axes and the curvature of tools/time_scattered_image.py), sampling = 64, plot_log=False,
with the stand-ins of tests/golden/refshim: the median of `--samples` runs; at sizes above 2048 ONE run is made and recorded as such.
clean=True is the reference's default and is timed as it stands (scipy griddata over the whole spectrum, whose result it never uses);
the time with clean=False -- the spline alone -- is recorded beside it.  Writes tests/golden/scatim_timing.json, which DESIGN.md
quotes beside the device figures."""
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
import numpy as np  # noqa: E402
from scintools.dynspec import Dynspec  # noqa: E402
from time_scattered_image import axes  # noqa: E402

warnings.simplefilter("ignore")


def once(d, sspec, fdop, tdel, eta, clean):
    t0 = time.perf_counter()
    d.calc_scattered_image(input_sspec=sspec, input_fdop=fdop, input_tdel=tdel, input_eta=eta, sampling=64, plot_log=False, clean=clean)
    return round(time.perf_counter() - t0, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--with-clean", action="store_true", help="also time the default clean=True (griddata over the whole spectrum)")
    args = ap.parse_args()
    out = {"what": "wall time of the unmodified reference's Dynspec.calc_scattered_image on the host (refshim stand-ins), one process; "
                   "'seconds' is clean=False (the spline and the evaluation alone)", "host_cores": os.cpu_count(), "cases": {}}
    for size in args.sizes:
        nr, nc, fdop, tdel, eta = axes(size)
        sspec = 40.0 * (np.random.default_rng(size).random((nr, nc)) - 1.0)
        d = Dynspec.__new__(Dynspec)
        n = args.samples if size <= 2048 else 1
        secs = [once(d, sspec, fdop, tdel, eta, False) for _ in range(n)]
        rec = {"spectrum": [nr, nc], "seconds": round(float(np.median(secs)), 3), "samples": secs, "runs": n}
        if args.with_clean:
            rec["seconds_clean_true"] = once(d, sspec, fdop, tdel, eta, True)
        else:
            rec["seconds_clean_true"] = "not run"
        out["cases"][str(size)] = rec
        print(size, rec, flush=True)
    with open(os.path.join(HERE, "scatim_timing.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
