#!/usr/bin/env python
"""Time the biharmonic fill with the line-block preconditioner on the GPU; print one JSON line and write
inpaint_lines_timing.json.

    python tests/tools/time_inpaint_lines.py [--repeats 7] [--warmups 2] [--sizes 1024 4096] [--plain-sizes 1024] [--out profiles]

Input: the seeded pattern of tests/inpaint_cases.py, n x n, with 1 % isolated pixels, one band of 200 whole channels, eight single
whole channels and three whole sub-integrations masked.  After `warmups` runs, `repeats` timed ones; median, min and max of

  call_ms     HIP events around ONE scint_inpaint_biharmonic_lines call on resident arrays: compaction, line detection, tables and
              factors, x0 = M^-1 b, every step (two launches, the transforms and solves of M^-1 r, the combination), the host's
              looks at the state (every 8 steps) and the scatter

and `iters`, the true relative `residual`, `per_step_us` = call_ms / max(iters, 1) (an upper bound: the call holds the set-up and
the start vector too), the whole lines found.  For `plain-sizes` the plain route (scint_inpaint_biharmonic, 2000 steps) runs ONCE
on the same mask beside it: `plain_status` (expected: NOCONV), `plain_iters`, `plain_residual` (what it reached) and
`plain_call_ms`.  No threshold: the figures are recorded."""
import argparse
import ctypes
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def observation(n, seed=12):
    import numpy as np
    import inpaint_cases as ic
    rng = np.random.default_rng(seed)
    bad = rng.random((n, n)) < 0.01
    start = n // 3
    bad[start:start + 200, :] = True
    free = np.setdiff1d(np.arange(8, n - 8), np.arange(start - 8, start + 208))
    bad[rng.choice(free, size=8, replace=False), :] = True
    bad[:, rng.choice(np.arange(8, n - 8), size=3, replace=False)] = True
    return np.where(bad, np.nan, ic.image(n, n, seed=seed)), bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--plain-sizes", type=int, nargs="*", default=[1024])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(HERE)), "profiles"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from scintools_amd import _lib, clean, device
    out = {"tool": "time_inpaint_lines", "repeats": a.repeats, "warmups": a.warmups, "device": torch.cuda.get_device_name(0),
           "tol": clean.INPAINT_TOL, "cases": {}}
    for n in a.sizes:
        dyn, bad = observation(n)
        nmask, nchan, nsub = int(bad.sum()), int(bad.all(axis=1).sum()), int(bad.all(axis=0).sum())
        src = device.to_device(np.where(bad, 0.0, dyn), torch.float64)
        work = torch.empty_like(src)
        m = device.to_device(bad, torch.uint8)
        table = device.to_device(clean.stencil_table(), torch.float64)
        residual, iters = ctypes.c_double(), ctypes.c_int32()

        def call(entry, *counts):
            ws = device.workspace_for(entry, n, n, nmask, *counts)
            work.copy_(src)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            status = "ok"
            try:
                _lib.call(entry, work, n, n, m, nmask, *counts, table, clean.INPAINT_TOL, clean.INPAINT_MAX_ITER, residual, iters,
                          ws, ws.numel(), device.stream_ptr())
            except _lib.ScintHipError as err:
                if err.status != _lib.SCINT_E_NOCONV:
                    raise
                status = "NOCONV"
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1), status

        for _ in range(a.warmups):
            call("scint_inpaint_biharmonic_lines", nchan, nsub)
        runs = [call("scint_inpaint_biharmonic_lines", nchan, nsub) for _ in range(a.repeats)]
        assert all(s == "ok" for _, s in runs) and torch.isfinite(work).all()
        ct = [t for t, _ in runs]
        res = {"shape": [n, n], "nmask": nmask, "line_channels": nchan, "line_subints": nsub, "iters": iters.value,
               "residual": residual.value, "call_ms": spread(ct),
               "per_step_us": round(statistics.median(ct) * 1e3 / max(iters.value, 1), 2)}
        if n in a.plain_sizes:
            ms, status = call("scint_inpaint_biharmonic")
            res.update(plain_status=status, plain_iters=iters.value, plain_residual=residual.value, plain_call_ms=round(ms, 3))
        out["cases"][f"{n}x{n}"] = res
        print(f"{n}x{n}", json.dumps(res), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "inpaint_lines_timing.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
