#!/usr/bin/env python
"""Time the velocity and trapezoid rescalings on the GPU; print one JSON line and write scale_timing.json / scale_gpu.txt.

    python tests/tools/time_scale.py [--repeats 5] [--sizes 1024 4096] [--out profiles]

Per size n (an n x n seeded spectrum resident on the device, the effective velocity of tests/scale_cases.contrast_veff at 3 : 1):
(a) the row resample `arcfit.spline_resample_rows_device` against the same result from what the package had before it: device
    transpose, `arcfit.spline_resample_device` (scint_spline_resample: the recurrences down the strided axis), flip and transpose
    back; wall time of the whole call (host factors, uploads, kernels; synchronised) and the device time of the kernels alone
    (the entry point called directly on resident tables, timed by device events);
(b) the bytes a pass moves (one read of dyn + the tile overlap + one write of the result, 8 bytes each) and the fraction of the
    plain-read rate of DESIGN.md section 9 (5.85 TB/s) the kernels reach;
(c) the trapezoid pass `scint_trap_scale` against one read plus one write of the array;
(d) the reference's host time of scale_dyn('velocity') from tests/golden/scale_timing.json where the size is there.
Two warm-up calls, then `repeats` timed ones; medians, minimum and maximum.  No pass/fail threshold."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

PLAIN_READ = 5.85e12


def timed(fn, repeats):
    import torch
    for _ in range(2):
        fn()
    wall, dev = [], []
    for _ in range(repeats):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(a.elapsed_time(b))
    stat = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    return {"wall_ms": stat(wall), "device_ms": stat(dev)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(HERE)), "profiles"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import scale_cases as sc
    import scale_oracle as so
    from scintools_amd import _lib, arcfit
    from scintools_amd.device import empty, stream_ptr, to_device, workspace_for
    from scintools_amd.dynspec import get_window
    try:
        with open(os.path.join(os.path.dirname(HERE), "golden", "scale_timing.json")) as fh:
            ref = json.load(fh)["results"]
    except OSError:
        ref = {}
    out = {"tool": "time_scale", "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "plain_read_bytes_per_s": PLAIN_READ,
           "cases": {}}
    lines = []
    for n in a.sizes:
        g = torch.Generator(device="cuda").manual_seed(n)
        dyn_t = torch.rand((n, n), dtype=torch.float64, device="cuda", generator=g) + 1.0
        x, xnew = (np.asarray(v, dtype=float) for v in so.velocity_grid(sc.contrast_veff(n, 3.0)))
        route = arcfit.spline_rows_route(x)
        arcfit._ROWS_TRANSPOSE_MIN = float("inf")            # time the row kernel itself at every size, not the route the helper picks
        new = lambda: arcfit.spline_resample_rows_device(dyn_t, x, xnew)
        # the same result with the column kernel: its output rows are flipped (np.flipud), so ask for the targets reversed
        old = lambda: arcfit.spline_resample_device(dyn_t.t().contiguous(), x, xnew[::-1]).t().contiguous()
        diff = float((new() - old()).abs().max() / new().abs().max())
        res = {"route": list(route), "new_vs_transpose_route_rel": diff, "rows": timed(new, a.repeats),
               "transpose_route": timed(old, a.repeats)}
        # the kernels alone
        h, sub, inv, sup, end = arcfit._spline_system(x)
        idx = np.clip(np.searchsorted(x, xnew, side="right") - 1, 0, n - 2)
        hk = h[idx]
        A, B = (x[idx + 1] - xnew) / hk, (xnew - x[idx]) / hk
        coef = np.stack([A, B, (A**3 - A) * hk**2 / 6.0, (B**3 - B) * hk**2 / 6.0], axis=1)
        dev = lambda v: to_device(np.ascontiguousarray(v, dtype=float), torch.float64)
        tabs = [dev(h), dev(sub), dev(inv), dev(sup)]
        idx_t, coef_t, end = to_device(idx.astype(np.int32), torch.int32), dev(coef), np.ascontiguousarray(end, dtype=float)
        o_t = empty((n, n), torch.float64)
        block, warm = route[1], route[2]
        ws = workspace_for("scint_spline_resample_rows", n, n, block, warm)
        kern = lambda: _lib.call("scint_spline_resample_rows", dyn_t, n, n, *tabs, end, block, warm, idx_t, coef_t, n, o_t, ws,
                                 ws.numel(), stream_ptr())
        res["rows_kernel"] = timed(kern, a.repeats)
        span = min(block + 2 * warm + 4, n) if block else n
        moved = 8.0 * n * n * ((span / block if block else 1.0) + 1.0 + 1.0)      # tile loads + the evaluation's y + the result
        res["rows_kernel"]["bytes"] = moved
        res["rows_kernel"]["fraction_of_plain_read"] = round(moved / (res["rows_kernel"]["device_ms"]["median"] * 1e-3) / PLAIN_READ, 4)
        ws2 = torch.empty(2 * 8 * n * n, dtype=torch.uint8, device="cuda")
        dyn_tr = dyn_t.t().contiguous()
        o2 = empty((n, n), torch.float64)
        blk2, warm2 = arcfit._spline_blocks(sub, inv, sup, n)
        col = lambda: _lib.call("scint_spline_resample", dyn_tr, n, n, 0, *tabs, end, blk2, warm2, idx_t, coef_t, n, o2, ws2,
                                ws2.numel(), stream_ptr())
        res["column_kernel_without_transposes"] = timed(col, a.repeats)
        # the trapezoid pass
        freqs = np.linspace(1300.0, 1500.0, n)
        times = 100.0 + 200.0 * np.arange(n)
        cw, sw = (dev(v) for v in get_window(n, n))
        t_t, keep_t = dev(times), to_device(arcfit.trapezoid_keep(freqs, times), torch.int32)
        trap = lambda: _lib.call("scint_trap_scale", dyn_t, n, n, 1.5, cw, sw, t_t, keep_t, o_t, stream_ptr())
        res["trapezoid_kernel"] = timed(trap, a.repeats)
        res["trapezoid_kernel"]["bytes"] = 16.0 * n * n
        res["trapezoid_kernel"]["fraction_of_plain_read"] = round(
            16.0 * n * n / (res["trapezoid_kernel"]["device_ms"]["median"] * 1e-3) / PLAIN_READ, 4)
        copy = lambda: o_t.copy_(dyn_t)
        res["copy_read_plus_write"] = timed(copy, a.repeats)
        r = ref.get(f"{n}x{n}")
        if r:
            res["reference_cpu_s"] = round(r["scale_dyn_velocity_s"], 3)
        out["cases"][f"{n}x{n}"] = res
        lines.append(f"{n}x{n}: rows {route} call {res['rows']['wall_ms']['median']} ms wall, kernel "
                     f"{res['rows_kernel']['device_ms']['median']} ms ({res['rows_kernel']['fraction_of_plain_read']} of plain read); "
                     f"transpose route call {res['transpose_route']['wall_ms']['median']} ms wall "
                     f"({res['transpose_route']['device_ms']['median']} ms device), its column kernels alone "
                     f"{res['column_kernel_without_transposes']['device_ms']['median']} ms; trapezoid kernel "
                     f"{res['trapezoid_kernel']['device_ms']['median']} ms ({res['trapezoid_kernel']['fraction_of_plain_read']} of "
                     f"plain read), a device copy {res['copy_read_plus_write']['device_ms']['median']} ms; reference on the host "
                     f"{res.get('reference_cpu_s', 'n/a')} s; new vs transpose route {diff:.2e}; medians of {a.repeats}, {out['device']}")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "scale_timing.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    with open(os.path.join(a.out, "scale_gpu.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
