#!/usr/bin/env python
"""Time the biharmonic fill on the GPU; print one JSON line and write inpaint_timing.json.

    python tests/tools/time_inpaint.py [--repeats 7] [--warmups 2] [--sizes 1024 4096] [--oracle-size 1024] [--out profiles]

Input: the seeded pattern of tests/inpaint_cases.py, n x n, with 1 % isolated pixels and eight whole channels masked.  After
`warmups` runs, `repeats` timed ones; median, min and max of

  call_ms     HIP events around ONE scint_inpaint_biharmonic call on resident arrays: compaction, right-hand side, every
              conjugate-gradient step, the host's looks at the state (every 8 steps) and the scatter
  whole_ms    clean.biharmonic_fill_device: mask count, uploads, the call, the download (host clock around a synchronise)

and `iters`, the true relative `residual`, `per_step_us` = call_ms / iters (an upper bound: the call holds the set-up too),
`bytes_per_step` = 84 bytes streamed per unknown (list, r, p_old read, p, q written; x, r, p, q read, x, r written) plus the 13
index reads of 4 bytes, and `gbps` = bytes_per_step / per_step.  For `oracle-size` the host oracle (tests/inpaint_oracle.py) solves
the same mask once: `oracle_assemble_s`, `oracle_spsolve_s`, and the relative difference of the two fills.  No threshold: the
figures are recorded."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

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
    bad[rng.choice(np.arange(8, n - 8), size=8, replace=False), :] = True
    return np.where(bad, np.nan, ic.image(n, n, seed=seed)), bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--oracle-size", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(HERE)), "profiles"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import inpaint_oracle as io
    from scintools_amd import _lib, clean, device
    out = {"tool": "time_inpaint", "repeats": a.repeats, "warmups": a.warmups, "device": torch.cuda.get_device_name(0),
           "tol": clean.INPAINT_TOL, "cases": {}}
    for n in a.sizes:
        dyn, bad = observation(n)
        nmask = int(bad.sum())
        src = device.to_device(np.where(bad, 0.0, dyn), torch.float64)
        work = torch.empty_like(src)
        m = device.to_device(bad, torch.uint8)
        table = device.to_device(clean.stencil_table(), torch.float64)
        ws = device.workspace_for("scint_inpaint_biharmonic", n, n, nmask)
        residual, iters = ctypes.c_double(), ctypes.c_int32()

        def call():
            work.copy_(src)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.call("scint_inpaint_biharmonic", work, n, n, m, nmask, table, clean.INPAINT_TOL, clean.INPAINT_MAX_ITER, residual,
                      iters, ws, ws.numel(), device.stream_ptr())
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        def whole():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            filled = clean.biharmonic_fill_device(dyn)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, filled

        for _ in range(a.warmups):
            call()
            whole()
        ct = [call() for _ in range(a.repeats)]
        runs = [whole() for _ in range(a.repeats)]
        filled = runs[-1][1]
        assert np.array_equal(filled, work.cpu().numpy()) and np.isfinite(filled).all()
        per_step_us = statistics.median(ct) * 1e3 / iters.value
        bytes_per_step = (84 + 52) * nmask
        res = {"shape": [n, n], "nmask": nmask, "iters": iters.value, "residual": residual.value, "call_ms": spread(ct),
               "whole_ms": spread([r[0] for r in runs]), "per_step_us": round(per_step_us, 2), "bytes_per_step": bytes_per_step,
               "gbps": round(bytes_per_step / per_step_us * 1e-3, 1)}
        if n == a.oracle_size:
            t0 = time.perf_counter()
            mat, b = io.system(dyn, bad)
            t1 = time.perf_counter()
            from scipy.sparse.linalg import spsolve
            u = spsolve(mat, b)
            t2 = time.perf_counter()
            res.update(oracle_assemble_s=round(t1 - t0, 3), oracle_spsolve_s=round(t2 - t1, 3),
                       oracle_residual=io.residual(mat, b, u), residual_by_oracle_matrix=io.residual(mat, b, filled[bad]),
                       rel_diff_to_oracle=float(np.linalg.norm(filled[bad] - u) / np.linalg.norm(u)))
        out["cases"][f"{n}x{n}"] = res
        print(f"{n}x{n}", json.dumps(res), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "inpaint_timing.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
