#!/usr/bin/env python
"""Time the batched 1-D ACF fit on the GPU; print one JSON line and write acf1d_fit_timing.json.

    python tests/tools/time_acf1d.py [--repeats 7] [--warmups 2] [--sizes 1024 4096] [--out profiles]

Input: the seeded correlated field of tests/tools/time_scintpar.py, n x n.  Per size, `fit_scint_params_cut(63, 63)`: 4096 segments
of n/64 x n/64, their ACFs in one stack, one fit launch.  After `warmups` runs, `repeats` timed ones bracketed by device
synchronisation; median, min and max of

  whole_call    Dynspec.fit_scint_params_cut(63, 63): upload, segment cut, 4096 ACFs, the fit launch, the downloads (host clock)
  fit_kernel    scint_acf1d_fit alone on the prepared stack, outputs preallocated (events on the stream)

and, beside them, `oracle_s`: the host oracle (tests/acf1d_oracle.py, one scipy.optimize.least_squares call per problem) on the
same 4096 ACFs, once, with the number of problems on which both converge and the largest relative difference of tau and dnu
between the two on those.  No threshold: the figures are recorded."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(HERE)), "profiles"))
    ap.add_argument("--no-oracle", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    import acf1d_oracle as ao
    from time_scintpar import field
    from scintools_amd import _lib, device, scintpar
    from scintools_amd.dynspec import Dynspec
    out = {"tool": "time_acf1d", "repeats": a.repeats, "warmups": a.warmups, "device": torch.cuda.get_device_name(0), "cases": {}}
    for n in a.sizes:
        o = field(n, n)
        fnum = tnum = n // 64

        def whole():
            d = Dynspec(dyn=o, verbose=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d.fit_scint_params_cut(tcuts=63, fcuts=63)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, d

        for _ in range(a.warmups):
            whole()
        runs = [whole() for _ in range(a.repeats)]
        d = runs[-1][1]
        # the same stack, for the kernel alone and for the oracle
        segs = scintpar.segment_cut_device(device.to_device(o.dyn, torch.float64), fnum, tnum, 64, 64)
        B = 4096
        acfs = device.empty((B, 2 * fnum, 2 * tnum), torch.float64)
        for k in range(B):
            scintpar.acf_device(segs[k], subtract_mean=False, out=acfs[k])
        R, C = 2 * fnum, 2 * tnum
        bw = device.to_device(np.full(B, fnum * o.df), torch.float64)
        tobs = device.to_device(np.full(B, tnum * o.dt), torch.float64)
        values, errors = device.empty((B, 4), torch.float64), device.empty((B, 4), torch.float64)
        stats, setup = device.empty((B, 2), torch.float64), device.empty((B, 6), torch.float64)
        niter, status = device.empty((B,), torch.int32), device.empty((B,), torch.int32)
        ws = device.workspace_for("scint_acf1d_fit", B, R, C)

        def kernel():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.call("scint_acf1d_fit", acfs, B, R, C, float(o.dt), float(o.df), bw, tobs, 5.0, 0, 1, 1, 5/3, 0, 200, values, errors,
                      stats, niter, status, setup, ws, ws.numel(), device.stream_ptr())
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        for _ in range(a.warmups):
            kernel()
        kt = [kernel() for _ in range(a.repeats)]
        st, it = status.cpu().numpy(), niter.cpu().numpy()
        assert np.array_equal(st.reshape(64, 64), d.cut_fit_status)
        res = {"shape": [n, n], "problems": B, "acf_shape": [R, C], "whole_call_ms": spread([r[0] for r in runs]),
               "fit_kernel_ms": spread(kt), "converged": int((st == 0).sum()), "status_counts": np.bincount(st, minlength=5).tolist(),
               "niter_median": float(np.median(it)), "niter_max": int(it.max()),
               "bytes_per_problem": {"acf_read": 8 * (R - R // 2 + C - C // 2), "workspace": 16 * (R - R // 2 + C - C // 2),
                                     "outputs": 8 * 16 + 8}}
        if not a.no_oracle:
            host = acfs.cpu().numpy()
            warnings.simplefilter("ignore", RuntimeWarning)
            t0 = time.perf_counter()
            _, fits = ao.fit_stack(host, o.dt, o.df, fnum * o.df, tnum * o.dt)
            res["oracle_s"] = round(time.perf_counter() - t0, 3)
            vals = values.cpu().numpy()
            both = [b for b in range(B) if st[b] == 0 and fits[b]["success"]]
            res["oracle_converged"] = int(sum(f["success"] for f in fits))
            res["both_converged"] = len(both)
            res["max_rel_diff_tau_dnu"] = float(max(max(abs(vals[b, 0] / fits[b]["tau"] - 1), abs(vals[b, 1] / fits[b]["dnu"] - 1))
                                                    for b in both)) if both else None
        out["cases"][f"{n}x{n}"] = res
        print(f"{n}x{n}", json.dumps(res), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "acf1d_fit_timing.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
