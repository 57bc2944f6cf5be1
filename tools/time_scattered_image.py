#!/usr/bin/env python
"""Time Dynspec.calc_scattered_image on the device at the spectra of a 1024^2 and a 4096^2 dynamic spectrum (1024 x 2048 and
4096 x 8192 float64 in dB), sampling = 64, beside the unmodified reference's host times (tests/golden/scatim_timing.json,
tests/golden/time_reference_scatim.py).

    python tools/time_scattered_image.py [--sizes 1024 4096] [--warmup 2] [--reps 7]

The spectrum is a seeded bounded field already resident on the device (what calc_sspec leaves parked); the curvature puts the arc's
edge at 60 % of the Doppler range, as tests/golden/time_reference_scatim.py does, so both crop the same columns.  Timed: the whole
method (host tables, uploads, the five launches, the read-back of the 129^2 image) and the device call alone on resident tensors,
synchronised around the timed region: two warm-up calls, then the median and the min-max spread of seven.  Beside each: the bytes
of one read of the cropped spectrum (the floor of the row pass), the rate the device call achieves on them, and the speed-up over
the reference.  Not a test and not part of bench.py.  Writes profiles/scatim_timing.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def stats(secs):
    return {"median_ms": round(1e3 * float(np.median(secs)), 4), "min_ms": round(1e3 * min(secs), 4), "max_ms": round(1e3 * max(secs), 4),
            "reps": len(secs)}


def axes(size):
    nr, nc = size, 2 * size
    fdop = (np.arange(nc) - nc // 2) * (1e3 / (nc * 30.0))
    tdel = np.arange(nr) / (2 * nr * 0.05)
    eta = tdel[-1] / (0.6 * fdop[-1])**2
    return nr, nc, fdop, tdel, eta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--sampling", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "scatim_timing.json"))
    args = ap.parse_args()
    import torch
    from scintools_amd import arcfit, device
    from scintools_amd.dynspec import Dynspec
    dev = device.require_gpu()
    try:
        with open(os.path.join(REPO, "tests", "golden", "scatim_timing.json")) as fh:
            ref = json.load(fh)["cases"]
    except OSError:
        ref = {}
    out = {"what": "Dynspec.calc_scattered_image; times in ms", "device": torch.cuda.get_device_name(dev), "sampling": args.sampling,
           "cases": {}}

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        secs = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        return stats(secs)

    for size in args.sizes:
        nr, nc, fdop, tdel, eta = axes(size)
        gen = torch.Generator(device=dev).manual_seed(size)
        sspec_t = 40.0 * (torch.rand((nr, nc), dtype=torch.float64, device=dev, generator=gen) - 1.0)     # 4 decades, in dB
        d = Dynspec.__new__(Dynspec)
        d.fdop, d.tdel = fdop, tdel
        Dynspec.sspec.park(d, sspec_t)
        seen = {}
        inner = arcfit.scattered_image_device

        def capture(*a):
            seen["args"] = a
            return inner(*a)

        arcfit.scattered_image_device = capture
        try:
            d.calc_scattered_image(input_eta=eta, sampling=args.sampling, plot_log=False)
        finally:
            arcfit.scattered_image_device = inner
        _, rows, cols, tdel_c, fdop_c, _, _ = seen["args"]
        crop_bytes = 8.0 * (rows[1] - rows[0]) * (cols[1] - cols[0])
        rec = {"spectrum": [nr, nc], "crop_rows": list(rows), "crop_cols": list(cols), "crop_bytes": crop_bytes,
               "image": list(d.scattered_image.shape), "finite": bool(np.isfinite(d.scattered_image).all())}
        rec["method"] = timed(lambda: d.calc_scattered_image(input_eta=eta, sampling=args.sampling, plot_log=False))
        rec["device_call"] = timed(lambda: inner(sspec_t, rows, cols, tdel_c, fdop_c, eta, args.sampling))
        sec = rec["device_call"]["min_ms"] * 1e-3
        rec["note"] = "device_call includes the host tables, their upload and the image read-back: an upper bound on the kernels"
        rec["crop_read_GBps_at_min"] = round(crop_bytes / sec / 1e9, 1)
        rec["floor_ms_at_6.3TBps"] = round(crop_bytes / 6.3e12 * 1e3, 4)
        host = ref.get(str(size), {}).get("seconds")
        rec["reference_seconds"] = host if host is not None else "not recorded"
        if host is not None:
            rec["speedup_method"] = round(host / (rec["method"]["median_ms"] * 1e-3), 1)
        print(json.dumps({size: rec}), flush=True)
        out["cases"][str(size)] = rec
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
