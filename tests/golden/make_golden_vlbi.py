#!/usr/bin/env python
"""Generate tests/golden/vlbi.npz (and vlbi_timing.json) by running the UNMODIFIED reference's VLBI_chunk_retrieval
(scintools/ththmod.py:1223-1387) with the stand-ins of tests/golden/refshim, as make_golden_thin.py does.

    python tests/golden/make_golden_vlbi.py

Inputs: the seeded multi-station fields of tests/vlbi_cases.py (GOLDEN).  Stored per case: the inputs, the output of every
thth_redmap call the reference function itself makes (recorded through a pass-through wrapper of the reference's own
thth_redmap, with the `hermetian` flag of each call), edges_red, and the returned model_E.  ARPACK starts from a random vector,
so model_E is reproduced up to ONE phase common to all stations (two runs agree to ~3e-15 of the peak after removing it);
everything else is reproduced bit for bit.  Also recorded: what the reference does when the crop keeps fewer than two centres."""
import json
import os
import sys
import time
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "refshim"))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import matplotlib  # noqa: E402
matplotlib.use("Agg")
import numpy as np  # noqa: E402
import astropy.units as u  # noqa: E402  (the shim)
import scintools.ththmod as thth  # noqa: E402
import vlbi_cases  # noqa: E402

warnings.simplefilter("ignore")


def V(q):
    return np.array(getattr(q, "value", q))


def run_reference(c, eta=None):
    """(model_E list, recorded thth_redmap calls [(thth_red, edges_red, hermetian)], seconds)."""
    calls = []
    orig = thth.thth_redmap

    def recorder(CS, tau, fd, eta_, edges, hermetian=True):
        red, er = orig(CS, tau, fd, eta_, edges, hermetian=hermetian)
        calls.append((np.array(red), V(er), bool(hermetian)))
        return red, er
    thth.thth_redmap = recorder
    try:
        params = (c["dlist"], c["edges"] * u.mHz, c["time"] * u.s, c["freq"] * u.MHz, (c["eta"] if eta is None else eta) * u.s**3,
                  0, 0, c["npad"], c["n_dish"], c["tauMask"] * u.us, False)
        t0 = time.perf_counter()
        model_E, _, _ = thth.VLBI_chunk_retrieval(params)
        secs = time.perf_counter() - t0
    finally:
        thth.thth_redmap = orig
    return model_E, calls, secs


if __name__ == "__main__":
    arrs, timing = {}, {}
    for name in vlbi_cases.GOLDEN:
        c = vlbi_cases.golden_case(name)
        model_E, calls, secs = run_reference(c)
        run_reference(c)
        _, _, secs = run_reference(c)            # the third run's seconds (imports and caches warm)
        nspec = c["n_dish"] * (c["n_dish"] + 1) // 2
        assert len(calls) == nspec
        for i in range(nspec):
            arrs[f"{name}_in{i}"] = np.asarray(c["dlist"][i])
            arrs[f"{name}_red{i}"] = calls[i][0]
            arrs[f"{name}_herm{i}"] = np.array(calls[i][2])
        arrs[f"{name}_edges_red"] = calls[0][1]
        arrs[f"{name}_edges"], arrs[f"{name}_time"], arrs[f"{name}_freq"] = c["edges"], c["time"], c["freq"]
        arrs[f"{name}_eta"] = np.array(c["eta"])
        arrs[f"{name}_par"] = np.array([c["npad"], c["n_dish"]])
        arrs[f"{name}_tauMask"] = np.array(c["tauMask"])
        arrs[f"{name}_model_E"] = np.array(model_E)
        timing[name] = {"shape": list(np.asarray(c["dlist"][0]).shape), "npad": c["npad"], "n_dish": c["n_dish"],
                        "N": int(calls[0][0].shape[0]), "seconds": round(secs, 5)}
        print(name, "N =", calls[0][0].shape[0], "seconds", secs)
    # a curvature whose crop keeps ONE centre: what does the reference do?
    c = vlbi_cases.golden_case("n2")
    try:
        run_reference(c, eta=c["eta"] * 1e6)
        arrs["small_crop_raises"] = np.array("")
    except Exception as exc:  # noqa: BLE001
        arrs["small_crop_raises"] = np.array(type(exc).__name__)
    arrs["small_crop_eta_factor"] = np.array(1e6)
    print("crop of one centre:", arrs["small_crop_raises"])
    # edges wider than 1.5 times the Doppler span: does the reference's fancy index raise?
    c = vlbi_cases.wide_case()
    try:
        run_reference(c)
        arrs["wide_raises"] = np.array("")
    except Exception as exc:  # noqa: BLE001
        arrs["wide_raises"] = np.array(type(exc).__name__)
    arrs["wide_in1"] = np.asarray(c["dlist"][1])
    print("edges of 1.8 Doppler spans:", arrs["wide_raises"])
    path = os.path.join(HERE, "vlbi.npz")
    np.savez_compressed(path, **arrs)
    print(f"vlbi.npz: {os.path.getsize(path) / 1024:.0f} KiB, {len(arrs)} arrays")
    with open(os.path.join(HERE, "vlbi_timing.json"), "w") as fh:
        json.dump({"what": "reference VLBI_chunk_retrieval, one chunk per call, with the refshim stand-ins (third run of each case)",
                   "cases": timing, "host_cores": os.cpu_count()}, fh, indent=1)
        fh.write("\n")
