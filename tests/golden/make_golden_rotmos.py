#!/usr/bin/env python
"""Generate tests/golden/rotmos.npz and rotmos_timing.json by running the UNMODIFIED reference's fitted mosaics
(scintools/ththmod.py:1708-2310: rotMos, rotFit, rotInit, rotDer, fullMos, fullMosFit, fullMosGrad, fullMosHess) with the
stand-ins of tests/golden/refshim, as make_golden_vlbi.py does.

    SCINTOOLS_REFERENCE=<checkout of the reference> python tests/golden/make_golden_rotmos.py [--no-timing]

Inputs: the seeded stacks of tests/rotmos_cases.py (GOLDEN_SHAPES, and the 3 x 3 stack once more with NaNs in dspec and a NaN and
a zero in N).  Stored per case: the inputs and all eight outputs at the case's random x / p (`_r`) and at rotInit with amplitudes 1
(`_i`; the two mosaics at `_r` only).  rotmos_timing.json: the reference's host seconds per call at 256 chunks of 64 x 64 (median of three) and one sample of
each at 961 chunks of 256 x 256."""
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
import scintools.ththmod as thth  # noqa: E402
import rotmos_cases as rc  # noqa: E402

warnings.simplefilter("ignore")


def outputs(c, x, p):
    ch, d, N = c["chunks"], c["dspec"], c["N"]
    return dict(rotMos=thth.rotMos(ch, x), rotFit=np.array(thth.rotFit(x, ch)), rotDer=thth.rotDer(x, ch),
                fullMos=thth.fullMos(ch, p), fullMosFit=np.array(thth.fullMosFit(p, ch, d, N)),
                fullMosGrad=thth.fullMosGrad(p, ch, d, N), fullMosHess=thth.fullMosHess(p, ch, d, N))


def timed(fn, repeats):
    secs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        secs.append(time.perf_counter() - t0)
    return round(float(np.median(secs)), 5)


def timing(shape, repeats):
    c = rc.case(shape, seed=7)
    ch, d, N, x, p = c["chunks"], c["dspec"], c["N"], c["x"], c["p"]
    calls = dict(rotMos=lambda: thth.rotMos(ch, x), rotFit=lambda: thth.rotFit(x, ch), rotDer=lambda: thth.rotDer(x, ch),
                 fullMosFit=lambda: thth.fullMosFit(p, ch, d, N), fullMosGrad=lambda: thth.fullMosGrad(p, ch, d, N),
                 fullMosHess=lambda: thth.fullMosHess(p, ch, d, N))
    out = {"shape": list(shape), "chunks": shape[0] * shape[1], "repeats": repeats}
    for name, fn in calls.items():
        out[name] = timed(fn, repeats)
        print(shape, name, out[name], flush=True)
    return out


if __name__ == "__main__":
    arrs = {}
    cases = [(rc.name_of(s), rc.case(s)) for s in rc.GOLDEN_SHAPES] + [("nan3x3", rc.case((3, 3, 8, 12), seed=1, nans=True))]
    for nm, c in cases:
        for k in ("chunks", "dspec", "N", "x", "p"):
            arrs[f"{nm}_{k}"] = c[k]
        n = c["chunks"].shape[0] * c["chunks"].shape[1]
        xi = thth.rotInit(c["chunks"])
        arrs[f"{nm}_rotInit"] = xi
        for tag, x, p in (("r", c["x"], c["p"]), ("i", xi, np.concatenate((xi, np.ones(n))))):
            for k, v in outputs(c, x, p).items():
                if tag == "r" or k not in ("rotMos", "fullMos"):      # (the mosaics once: they are the bulk of the file)
                    arrs[f"{nm}_{tag}_{k}"] = np.asarray(v)
        print(nm, "rotFit", arrs[f"{nm}_r_rotFit"], "fullMosFit", arrs[f"{nm}_r_fullMosFit"])
    path = os.path.join(HERE, "rotmos.npz")
    np.savez_compressed(path, **arrs)
    print(f"rotmos.npz: {os.path.getsize(path) / 1024:.0f} KiB, {len(arrs)} arrays")
    if "--no-timing" not in sys.argv:
        t = {"what": "reference rotMos ... fullMosHess on the host with the refshim stand-ins: seconds per call",
             "tutorial": timing((16, 16, 64, 64), 3), "headline_one_sample": timing((31, 31, 256, 256), 1),
             "host_cores": os.cpu_count()}
        with open(os.path.join(HERE, "rotmos_timing.json"), "w") as fh:
            json.dump(t, fh, indent=1)
            fh.write("\n")
