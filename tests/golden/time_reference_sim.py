#!/usr/bin/env python
"""How long does the UNMODIFIED reference's screen simulator (scintools/scint_sim.py: Simulation) take on the host for the BASELINE
screen (oracle/sim_oracle.py: BASELINE_SCREEN) at nx = nf = 1024, ny = 128?

    SCINTOOLS_REFERENCE=<checkout of the reference> python tests/golden/time_reference_sim.py [--samples 3]

Wall time of the whole constructor in one process, as tests/golden/time_reference_workloads.py takes its figures, with the stand-ins
of tests/golden/refshim; every sample and their median go into tests/golden/sim_timing.json, which DESIGN.md quotes beside the device
figures of tools/time_simulation.py."""
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
sys.path.insert(0, REPO)

import matplotlib  # noqa: E402
matplotlib.use("Agg")
import numpy as np  # noqa: E402
from scintools.scint_sim import Simulation  # noqa: E402
from oracle.sim_oracle import BASELINE_SCREEN  # noqa: E402

warnings.simplefilter("ignore")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=3)
    args = ap.parse_args()
    secs = []
    for _ in range(args.samples):
        t0 = time.perf_counter()
        Simulation(nx=1024, ny=128, nf=1024, seed=1, **BASELINE_SCREEN)
        secs.append(round(time.perf_counter() - t0, 3))
        print(secs[-1], flush=True)
    out = {"what": "wall time of the unmodified reference's scint_sim.Simulation on the host (refshim stand-ins), one process",
           "baseline_1024": {"nx": 1024, "ny": 128, "nf": 1024, "seed": 1, "seconds": round(float(np.median(secs)), 3), "samples": secs},
           "host_cores": os.cpu_count()}
    with open(os.path.join(HERE, "sim_timing.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
