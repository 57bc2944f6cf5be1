#!/usr/bin/env python
"""Time scint_sim.Brightness on the GPU; print one JSON line and write brightness_timing.json / brightness_gpu.txt.

    python tests/tools/time_brightness.py [--repeats 5] [--sizes default large] [--out profiles] [--no-deviations]

Per size -- `default`: the reference's defaults, grid 600 x 600 and spectrum 2000 x 1000; `large`: grid 2048 x 2048 and spectrum
4000 x 4000 -- the wall time of a whole `Brightness(...)` with every device array complete (synchronised, nothing copied to the
host), for triangulation='main' and for 'qhull' (whose host Delaunay is timed on its own as well; at the large size it is run once),
and of its three steps with 'main'.  The vectorised NumPy oracle (tests/brightness_oracle.py, main diagonal) is timed once per size
on the same machine for context; the reference itself is not timed here (tests/golden/make_golden_brightness.py --time-defaults).
brightness_gpu.txt also lists, per golden case, the device's deviation from the reference's golden relative to each array's peak,
beside the oracle's own (tests/brightness_checks.py: ORACLE_DEV and TOL).  Two warm-up calls, then `repeats` timed ones; median,
minimum and maximum.  No pass/fail threshold."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

SIZES = {"default": dict(), "large": dict(nx=128, dx=0.125, nf=10, df=0.005, nt=80, dt=0.04)}


def timed(fn, repeats, warm=2):
    import torch
    for _ in range(warm):
        fn()
    wall = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(statistics.median(wall), 3), "min": round(min(wall), 3), "max": round(max(wall), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", nargs="+", default=["default", "large"], choices=list(SIZES))
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(HERE)), "profiles"))
    ap.add_argument("--no-deviations", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    import brightness_cases as bc
    import brightness_checks as ck
    import brightness_oracle as bo
    from scintools_amd import scint_sim as S
    out = {"tool": "time_brightness", "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "cases": {}}
    lines = []
    for size in a.sizes:
        kw = SIZES[size]
        b = S.Brightness(triangulation="main", **kw)
        res = {"grid": list(S.Brightness.B.shape(b)), "spectrum": list(S.Brightness.SS.shape(b))}
        res["main_ms"] = timed(lambda: S.Brightness(triangulation="main", **kw), a.repeats)
        res["calc_brightness_ms"] = timed(b.calc_brightness, a.repeats)
        res["calc_SS_ms"] = timed(b.calc_SS, a.repeats)
        res["calc_acf_ms"] = timed(b.calc_acf, a.repeats)
        few = a.repeats if size == "default" else 1
        res["qhull_ms"] = timed(lambda: S.Brightness(triangulation="qhull", **kw), few, warm=0 if few == 1 else 1)
        res["qhull_host_delaunay_ms"] = timed(lambda: S.qhull_diagonals(b.x), few, warm=0)
        t0 = time.perf_counter()
        bo.model(diagonals="main", **kw)
        res["numpy_oracle_s"] = round(time.perf_counter() - t0, 3)
        out["cases"][size] = res
        lines.append(f"{size}: grid {res['grid']}, spectrum {res['spectrum']}: Brightness(triangulation='main') "
                     f"{res['main_ms']['median']} ms (calc_brightness {res['calc_brightness_ms']['median']}, calc_SS "
                     f"{res['calc_SS_ms']['median']}, calc_acf {res['calc_acf_ms']['median']}); 'qhull' {res['qhull_ms']['median']} ms "
                     f"of which the host Delaunay {res['qhull_host_delaunay_ms']['median']} ms; NumPy oracle {res['numpy_oracle_s']} s; "
                     f"medians of {a.repeats} ('qhull': of {few}), {out['device']}")
    if not a.no_deviations:
        dev = {}
        for case in bc.CASES:
            g = ck.load_golden(case)
            r = ck.run(S, "gpu", case, "golden")
            dev[case] = {k: ck.peak_dev(r[k], g[k]) for k in ("B", "SS", "acf")}
        worst = {k: float(np.nanmax([dev[c][k] for c in dev])) for k in ("B", "SS", "acf")}
        out["deviation_from_golden_over_peak"] = {"per_case": dev, "worst": worst, "oracle": ck.ORACLE_DEV, "asserted": ck.TOL}
        lines.append(f"deviation from the reference's goldens / peak, worst over the cases: device {worst}; the oracle's own "
                     f"{ck.ORACLE_DEV}; asserted (ten times the oracle's) {ck.TOL}")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "brightness_timing.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    with open(os.path.join(a.out, "brightness_gpu.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
