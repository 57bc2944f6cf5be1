#!/usr/bin/env python
"""Device times of the cleaning calls -- scint_zap, scint_refill_median (5 x 5), scint_svd_model (one mode) -- on a 1024^2 and a
4096^2 dynamic spectrum, with the upload and the download shown apart from the call:

    python tools/time_clean.py [--sizes 1024 4096] [--repeats 20] [--out FILE.json]

Call time: HIP events around ONE library call (all its launches; for scint_svd_model also the host's waits for the status every
fourth step), `--repeats` calls after one warm-up: median, minimum and maximum.  This is not per-kernel time (no kernel trace is
taken here).  scint_zap works in place, so every repeat first restores the array with a device-to-device copy inside the timed
window; that copy is timed alone the same way and both figures are recorded (`call_ms` has the copy's median subtracted).
Upload / download: wall time of ONE host-to-device and device-to-host copy of the float64 array from pageable memory, synchronised.  tests/golden/
time_reference_clean.py times the reference's methods on the same arrays (`workload`)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def workload(size, name):
    """Seeded positive size x size array: a rank-one bandpass x gain pattern times (1 + 0.3 noise); 0.1 % spikes for 'zap',
    2 % NaN for 'refill_median'."""
    rng = np.random.default_rng(size)
    a = np.outer(1.0 + 0.3 * np.cos(np.linspace(0, 3, size)), 1.0 + 0.2 * np.sin(np.linspace(0, 9, size)))
    a = a * (1.0 + 0.3 * rng.random((size, size)))
    if name == "zap":
        a[rng.random(a.shape) < 1e-3] = 50.0
    if name == "refill_median":
        a[rng.random(a.shape) < 0.02] = np.nan
    return a


def main():
    import torch
    from scintools_amd import _lib, clean, device
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.load()
    device.require_gpu()
    out = {"what": "milliseconds: one library call between HIP events (median [min, max] of the repeats), one upload and one "
                   "download (wall, pageable memory)", "repeats": args.repeats,
           "gpu": torch.cuda.get_device_name(0), "cases": {}}

    def timed(fn):
        ms = []
        for r in range(args.repeats + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return [round(float(f(ms[1:])), 3) for f in (np.median, np.min, np.max)]

    for size in args.sizes:
        rec = {}
        for name in ("zap", "refill_median", "correct_dyn"):
            a = workload(size, name)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t = device.to_device(a, torch.float64)
            torch.cuda.synchronize()
            up = (time.perf_counter() - t0) * 1e3
            n = size
            if name == "zap":
                need = ctypes.c_size_t()
                lib.scint_zap_workspace_bytes(ctypes.byref(need))
                ws = device.workspace.get(need.value)
                src = t.clone()

                def fn():
                    t.copy_(src)
                    _lib.check(lib.scint_zap(device.ptr(t), n * n, 7.0, None, device.ptr(ws), ws.numel(), device.stream_ptr()))
                copy_ms = timed(lambda: t.copy_(src))
                with_copy = timed(fn)
                rec["zap_restore_copy_ms"], rec["zap_with_copy_ms"] = copy_ms, with_copy
                k = [round(v - copy_ms[0], 3) for v in with_copy]
            elif name == "refill_median":
                o = device.empty((n, n), torch.float64)
                fill = float(np.mean(a[np.isfinite(a)]))
                k = timed(lambda: _lib.check(lib.scint_refill_median(device.ptr(t), n, n, 5, 5, fill, device.ptr(o), device.stream_ptr())))
                t = o
            else:
                need = ctypes.c_size_t()
                lib.scint_svd_model_workspace_bytes(n, n, ctypes.byref(need))
                ws = device.workspace.get(need.value)
                v0 = device.to_device(clean._start_basis(n, 1), torch.float64)
                m, c = device.empty((n, n), torch.float64), device.empty((n, n), torch.float64)
                it = ctypes.c_int32()
                k = timed(lambda: _lib.check(lib.scint_svd_model(device.ptr(t), n, n, 1, device.ptr(v0), clean.SVD_TOL, clean.SVD_MAX_ITER,
                                                                 device.ptr(m), device.ptr(c), None, ctypes.byref(it), device.ptr(ws),
                                                                 ws.numel(), device.stream_ptr())))
                rec["correct_dyn_iterations"] = it.value
                t = c
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t.cpu()
            down = (time.perf_counter() - t0) * 1e3
            rec[name] = {"call_ms": k[0], "call_ms_min_max": k[1:], "upload_ms": round(up, 3), "download_ms": round(down, 3)}
            print(size, name, rec[name], flush=True)
        out["cases"][str(size)] = rec
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
