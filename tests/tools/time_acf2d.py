#!/usr/bin/env python
"""Time the batched approximate 2-D ACF fit on the GPU; print one JSON line and write acf2d_fit_timing.json.

    python tests/tools/time_acf2d.py [--repeats 7] [--warmups 2] [--sizes 1024 4096] [--oracle-sample 64] [--out profiles]

Input: the seeded correlated field of tests/tools/time_scintpar.py, n x n, with its mean removed (cut_dyn subtracts none, and with a
mean no segment's ACF falls to half power: every window would be FIT_BAD_WINDOW).  Per size, `fit_scint_params_2d_cut(63, 63)`: 4096
segments of n/64 x n/64.  After `warmups` runs, `repeats` timed ones bracketed by device synchronisation; median, min and max of

  whole_call    Dynspec.fit_scint_params_2d_cut(63, 63): upload, cut, 4096 ACFs, the three launches, the downloads (host clock)
  fit_kernel    scint_acf2d_approx_fit alone on the prepared stack with the windows and start values of the whole call (events)

`oracle_s`: the host oracle (tests/acf2d_oracle.py) on the first `oracle-sample` problems whose window is good, once, scaled to 4096
in `oracle_s_for_4096`.  `full_frame`: one fit of the whole ACF of the 1024^2 observation on one workgroup (whole call, host
clock, and the kernel alone).  No threshold: the figures are recorded."""
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


def kernel_timer(stack, fit, o, bw, tobs, nsub, nchan, max_iter=200):
    """A function that launches scint_acf2d_approx_fit alone with the rectangles and start values of `fit`; returns ms."""
    import numpy as np
    import torch
    from scintools_amd import _lib, device
    B, R, C = (int(v) for v in stack.shape)
    rect = device.to_device(np.stack([fit[k] for k in ("f0", "nfw", "t0", "ntw")], axis=1).astype(np.int32), torch.int32)
    start = device.to_device(np.stack([fit[k + "_start"] for k in ("tau", "dnu", "amp", "alpha", "phasegrad")], axis=1),
                             torch.float64)
    status_in = device.to_device(np.where(fit["status"] == 3, 3, 0).astype(np.int32), torch.int32)
    bw_t, tobs_t = device.to_device(np.full(B, bw), torch.float64), device.to_device(np.full(B, tobs), torch.float64)
    values, errors = device.empty((B, 5), torch.float64), device.empty((B, 5), torch.float64)
    stats = device.empty((B, 2), torch.float64)
    niter, status, nnz = (device.empty((B,), torch.int32) for _ in range(3))
    ws = device.workspace_for("scint_acf2d_approx_fit", B, R, C, 0)

    def kernel():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.call("scint_acf2d_approx_fit", stack, B, R, C, rect, start, status_in, bw_t, tobs_t, float(nsub), float(nchan), 1, 1, 0,
                  max_iter, values, errors, stats, niter, status, nnz, 0, ws, ws.numel(), device.stream_ptr())
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    return kernel, status, niter


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--oracle-sample", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(HERE)), "profiles"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import acf2d_oracle as ao
    from time_scintpar import field
    from scintools_amd import device, scintpar
    from scintools_amd.dynspec import Dynspec
    warnings.simplefilter("ignore")
    out = {"tool": "time_acf2d", "repeats": a.repeats, "warmups": a.warmups, "device": torch.cuda.get_device_name(0), "cases": {}}
    for n in a.sizes:
        o = field(n, n)
        o.dyn = o.dyn - o.dyn.mean()
        fnum = tnum = n // 64

        def whole():
            d = Dynspec(dyn=o, verbose=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d.fit_scint_params_2d_cut(tcuts=63, fcuts=63)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, d

        for _ in range(a.warmups):
            whole()
        runs = [whole() for _ in range(a.repeats)]
        d = runs[-1][1]
        segs = scintpar.segment_cut_device(device.to_device(o.dyn, torch.float64), fnum, tnum, 64, 64)
        B, R, C = 4096, 2 * fnum, 2 * tnum
        acfs = device.empty((B, R, C), torch.float64)
        for k in range(B):
            scintpar.acf_device(segs[k], subtract_mean=False, out=acfs[k])
        bw, tobs = fnum * o.df, tnum * o.dt
        fit = scintpar.acf2d_approx_fit_device(acfs, o.dt, o.df, bw, tobs, nsub=tnum, nchan=fnum)
        assert np.array_equal(fit["status"].reshape(64, 64), d.cut_fit_status)
        kernel, status, niter = kernel_timer(acfs, fit, o, bw, tobs, tnum, fnum)
        for _ in range(a.warmups):
            kernel()
        kt = [kernel() for _ in range(a.repeats)]
        st, it = status.cpu().numpy(), niter.cpu().numpy()
        assert np.array_equal(st, fit["status"])
        pts = (fit["nfw"] * fit["ntw"])[st != 5]
        res = {"shape": [n, n], "problems": B, "acf_shape": [R, C], "whole_call_ms": spread([r[0] for r in runs]),
               "fit_kernel_ms": spread(kt), "converged": int((st == 0).sum()), "status_counts": np.bincount(st, minlength=6).tolist(),
               "niter_median": float(np.median(it)), "niter_max": int(it.max()),
               "window_points_median": float(np.median(pts)) if pts.size else None,
               "window_points_max": int(pts.max()) if pts.size else None}
        host = acfs.cpu().numpy()
        sample, both, worst, secs = 0, 0, 0.0, 0.0
        for b in range(B):
            if sample >= a.oracle_sample:
                break
            if st[b] == 5:
                continue
            sample += 1
            t0 = time.perf_counter()
            try:
                f = ao.fit(ao.setup(host[b], o.dt, o.df, bw, tobs, nsub=tnum, nchan=fnum))
            except Exception:
                f = dict(success=False)
            secs += time.perf_counter() - t0
            if f["success"] and st[b] == 0:
                both += 1
                worst = max(worst, abs(fit["tau"][b] / f["tau"] - 1), abs(fit["dnu"][b] / f["dnu"] - 1))
        res.update(oracle_sample=sample, oracle_s=round(secs, 3), oracle_s_for_4096=round(secs * B / max(sample, 1), 1),
                   both_converged=both, max_rel_diff_tau_dnu=float(worst))
        out["cases"][f"{n}x{n}"] = res
        print(f"{n}x{n}", json.dumps(res), flush=True)

    # one full_frame fit of a whole 1024^2 observation's ACF: one workgroup
    n = 1024
    o = field(n, n)
    dd = Dynspec(dyn=o, verbose=False)
    dd.calc_acf()
    acf = type(dd).acf.tensor(dd)[None]

    def single():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f = scintpar.acf2d_approx_fit_device(acf, o.dt, o.df, o.bw, o.tobs, nsub=n, nchan=n, full_frame=True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, f

    single()
    runs = [single() for _ in range(3)]
    f = runs[-1][1]
    kernel, status, niter = kernel_timer(acf, f, o, o.bw, o.tobs, n, n)
    kernel()
    kt = [kernel() for _ in range(3)]
    out["full_frame_1024"] = {"acf_shape": [2 * n, 2 * n], "window": [int(f["nfw"][0]), int(f["ntw"][0])], "runs": 3,
                              "whole_call_ms": spread([r[0] for r in runs]), "fit_kernel_ms": spread(kt),
                              "status": int(f["status"][0]), "niter": int(f["niter"][0]), "nnz": int(f["nnz"][0])}
    print("full_frame_1024", json.dumps(out["full_frame_1024"]), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "acf2d_fit_timing.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
