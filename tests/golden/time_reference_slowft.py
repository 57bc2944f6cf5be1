#!/usr/bin/env python
"""How long does the UNMODIFIED reference's scint_utils.slow_FT (scintools/scint_utils.py:655-703) take on the host?

    SCINTOOLS_REFERENCE=<checkout of the reference> python tests/golden/time_reference_slowft.py [--samples 3]

Wall time at 256 x 256 and 512 x 256 [time, frequency] -- the reference forms an [nt, nt, nf] complex128 array and its phase (about
50 nt^2 nf bytes live at the peak), so 512 x 256 is the largest it can hold -- with the stand-ins of tests/golden/refshim and, in this
process only, np.fft.fftshift accepting `axis=` (see make_golden_slowft.py).  The median of `--samples` runs.  Writes
tests/golden/slowft_timing.json, which DESIGN.md quotes beside the device figures."""
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
sys.path.insert(0, os.path.join(REPO, "tests"))

import matplotlib  # noqa: E402
matplotlib.use("Agg")
import numpy as np  # noqa: E402

_fftshift = np.fft.fftshift
np.fft.fftshift = lambda x, axes=None, axis=None: _fftshift(x, axes=axis if axes is None else axes)
from scintools.scint_utils import slow_FT  # noqa: E402
import slowft_cases as sc  # noqa: E402

warnings.simplefilter("ignore")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=3)
    args = ap.parse_args()
    out = {"what": "wall time of the unmodified reference's scint_utils.slow_FT on the host (refshim stand-ins, fftshift(axis=) "
                   "accepted), one process", "host_cores": os.cpu_count(), "cases": {}}
    for nt, nf in ((256, 256), (512, 256)):
        d, f = np.array(sc.dyn(nt, nf)), sc.freqs(nf, "asc")
        secs = []
        for _ in range(args.samples):
            t0 = time.perf_counter()
            slow_FT(d, f)
            secs.append(round(time.perf_counter() - t0, 3))
        rec = {"shape": [nt, nf], "seconds": round(float(np.median(secs)), 3), "samples": secs}
        out["cases"][f"{nt}x{nf}"] = rec
        print(nt, nf, rec, flush=True)
    with open(os.path.join(HERE, "slowft_timing.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
