#!/usr/bin/env python
"""Time the fitted mosaics (ththmod.MosaicStack) on the GPU and print one JSON line.

    python tests/tools/time_rotmos.py [--repeats 7] [--small-only] [--profile-once]

Stacks: 256 chunks of 64 x 64 (the tutorial's size) and 961 chunks of 256 x 256 (the headline retrieval), seeded random chunks.
Per stack `rot_value_and_grad`, `full_value_and_grad` and `full_hess`: two warm-up calls, then `repeats` timed calls bracketed by
device synchronisation; median and spread (min, max).  Beside each time the bytes the evaluation must move -- the stack read once
by the gather and once by the window sums, the mosaic written once and read once, dspec and N read by both passes of the chi^2
fit; for the Hessian every overlap's two chunks, W, dspec and N, and the dense matrix written -- and the rate that gives.  The
speed-up is against tests/golden/rotmos_timing.json (the reference on the host).  Also one whole fit_mosaic("rot") on the small
stack.  --profile-once: one call of each after one warm-up, for a kernel trace."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def bytes_moved(shape):
    ncf, nct, cwf, cwt = shape
    n, cw = ncf * nct, cwf * cwt
    FT = ((ncf - 1) * (cwf // 2) + cwf) * ((nct - 1) * (cwt // 2) + cwt)
    rot = 2 * 16 * n * cw + 2 * 16 * FT
    full = rot + 16 * FT + 16 * n * cw                         # dspec, N: once per pixel in the gather, once per window element
    pairs = (n * cw + 2 * ((ncf - 1) * nct + (nct - 1) * ncf) * cw // 2 + 4 * (ncf - 1) * (nct - 1) * cw // 4)
    hess = 16 * n * cw + 16 * FT + (16 + 16 + 16 + 8 + 8) * pairs + 8 * (2 * n - 1) ** 2
    return {"rot_value_and_grad": rot, "full_value_and_grad": full, "full_hess": hess}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--profile-once", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    from scintools_amd import ththmod
    with open(os.path.join(os.path.dirname(HERE), "golden", "rotmos_timing.json")) as fh:
        ref = json.load(fh)
    out = {"tool": "time_rotmos", "repeats": 1 if a.profile_once else a.repeats, "device": torch.cuda.get_device_name(0), "stacks": {}}
    for key, shape in (("tutorial", (16, 16, 64, 64)), ("headline_one_sample", (31, 31, 256, 256))):
        if a.small_only and key != "tutorial":
            continue
        ncf, nct, cwf, cwt = shape
        n = ncf * nct
        g = torch.Generator(device="cuda").manual_seed(n)
        chunks_t = torch.randn(shape + (2,), dtype=torch.float64, device="cuda", generator=g)
        chunks_t = torch.view_as_complex(chunks_t)
        F, T = (ncf - 1) * (cwf // 2) + cwf, (nct - 1) * (cwt // 2) + cwt
        dspec_t = torch.rand((F, T), dtype=torch.float64, device="cuda", generator=g) + 0.5
        N_t = torch.full((F, T), 0.5, dtype=torch.float64, device="cuda")
        stack = ththmod.MosaicStack(chunks_t, dspec_t, N_t)
        rng = np.random.default_rng(n)
        x = rng.uniform(-np.pi, np.pi, n - 1)
        p = np.concatenate((x, rng.uniform(0.5, 2.0, n)))
        calls = {"rot_value_and_grad": lambda: stack.rot_value_and_grad(x), "full_value_and_grad": lambda: stack.full_value_and_grad(p),
                 "full_hess": lambda: stack.full_hess(p)}
        ref_s = {"rot_value_and_grad": ref[key]["rotFit"] + ref[key]["rotDer"], "full_value_and_grad": ref[key]["fullMosFit"] + ref[key]["fullMosGrad"],
                 "full_hess": ref[key]["fullMosHess"]}
        nbytes = bytes_moved(shape)
        res = {"shape": list(shape), "chunks": n}
        for name, fn in calls.items():
            def run():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3
            run()
            if not a.profile_once:
                run()
            ms = [run() for _ in range(1 if a.profile_once else a.repeats)]
            med = statistics.median(ms)
            res[name] = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "bytes": nbytes[name],
                         "TB_per_s": round(nbytes[name] / (med * 1e-3) / 1e12, 3), "reference_host_s": round(ref_s[name], 4),
                         "speedup": round(ref_s[name] / (med * 1e-3), 1)}
        if key == "tutorial":
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, _, r = ththmod.fit_mosaic(stack, mode="rot", out_device=True)
            torch.cuda.synchronize()
            res["fit_mosaic_rot"] = {"ms": round((time.perf_counter() - t0) * 1e3, 2), "iterations": int(r.nit), "evaluations": int(r.nfev)}
        out["stacks"][key] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
