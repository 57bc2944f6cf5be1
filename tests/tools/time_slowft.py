#!/usr/bin/env python
"""Time scint_utils.slow_FT on the GPU and print one JSON line.

    python tests/tools/time_slowft.py [--repeats 5] [--sizes 1024 4096]

Per size n (an n x n [time, frequency] seeded spectrum, freqs spanning 1200-1600 MHz, everything resident on the device): two warm-up
calls, then `repeats` calls timed by device events; median and spread.  Arithmetic as DESIGN.md section 4l counts it: stage 1 runs
(nt / 2 + 1) * nf * nt_padded real-by-complex terms of two FP64 FMAs (4 flop) each; the fraction is that count over the median time
against the FP64 vector peak of 78.6 TFLOP/s (half the FP32 vector peak of the microarchitecture guide: 256 CUs x 4 SIMDs x 16 lanes
x 2 flop x 2.4 GHz).  The part of the time that grows linearly in nt -- the transpose, stage 2 and the launches -- is separated from
the quadratic stage 1 with a second measurement at nt / 2: linear = 4 T(nt / 2) - T(nt), reported as `linear_share` (stage 2 is its
bulk; it is not timed on its own).  The speed-up is against tests/golden/slowft_timing.json (the reference on the host) where the
sizes match; the reference cannot hold 1024^2."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

PEAK_FP64_VECTOR = 78.6e12


def timed(fn, repeats):
    import torch
    for _ in range(2):
        fn()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    a = ap.parse_args()
    import torch
    import slowft_cases as sc
    from scintools_amd import scint_utils
    with open(os.path.join(os.path.dirname(HERE), "golden", "slowft_timing.json")) as fh:
        ref = json.load(fh)
    out = {"tool": "time_slowft", "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "peak_fp64_vector": PEAK_FP64_VECTOR,
           "reference_host_seconds": {k: v["seconds"] for k, v in ref["cases"].items()}, "sizes": {}}
    for n in a.sizes:
        f = sc.freqs(n, "asc")
        g = torch.Generator(device="cuda").manual_seed(n)
        d = torch.randn((n, n), dtype=torch.float64, device="cuda", generator=g) + 1.0
        full = timed(lambda: scint_utils.slow_FT(d, f, out_device=True), a.repeats)
        half = timed(lambda: scint_utils.slow_FT(d[:n // 2], f, out_device=True), a.repeats)
        t, th = statistics.median(full), statistics.median(half)
        ntp = -(-n // sc.B) * sc.B
        flop = 4.0 * (n // 2 + 1) * n * ntp
        linear = max(4 * th - t, 0.0)
        out["sizes"][str(n)] = {"ms": round(t, 3), "ms_min_max": [round(min(full), 3), round(max(full), 3)], "ms_half_nt": round(th, 3),
                                "stage1_flop": flop, "fp64_vector_fraction": round(flop / (t * 1e-3) / PEAK_FP64_VECTOR, 4),
                                "linear_share": round(linear / t, 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
