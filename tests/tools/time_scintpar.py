#!/usr/bin/env python
"""Time the no-fit scintillation measurements on the GPU; print one JSON line and write scintpar_timing.json / scintpar_gpu.txt.

    python tests/tools/time_scintpar.py [--repeats 5] [--sizes 1024 4096] [--out profiles]

Input: a seeded correlated random field n x n (white noise low-pass filtered to ~n/64 pixels, plus 1), so that the ACF has a
ridge and every fitted row's maximum is inside.  Per size, after one warm-up each, `repeats` runs bracketed by device
synchronisation (wall: host clock; device: events on the stream, copies included); median, min and max:

  device_route   a fresh Dynspec: calc_acf(); get_scint_params(method='nofit'); get_acf_tilt(method='nofit') -- the ACF stays in
                 HBM, the host receives two half-cuts, three moments and 7 samples per fitted row
  parent_route   what the parent commit offered: calc_acf() with its download of the whole ACF, then the same measurements
                 with NumPy on the host (tests/scintpar_oracle.py)
  cut_dyn_3_3    cut_dyn(tcuts=3, fcuts=3): 16 segments, secondary spectrum and ACF of each

with the bytes each route copies up and down (from the shapes) and the reference's own CPU seconds for the same calls
(tests/golden/scintpar_timing.json).  The two routes' results are compared (equal attributes) before anything is timed."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def field(n, seed):
    import numpy as np
    import scintpar_cases as cc
    rng = np.random.default_rng(seed)
    k = np.fft.fftfreq(n)
    filt = np.exp(-0.5 * (k[:, None] ** 2 + k[None, :] ** 2) * (2 * np.pi * n / 64.0) ** 2)
    x = np.real(np.fft.ifft2(np.fft.fft2(rng.standard_normal((n, n))) * filt))
    dyn = 1.0 + 0.5 * x / x.std()
    return cc.observation(dyn, 1400.0 + 0.05 * np.arange(n), 10.0 * np.arange(n), 0.05, 10.0, 1400.0 + 0.025 * n, f"field{n}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(HERE)), "profiles"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import scintpar_cases as cc
    import scintpar_oracle as so
    from scintools_amd import scintpar
    from scintools_amd.device import to_device
    from scintools_amd.dynspec import Dynspec
    try:
        with open(os.path.join(os.path.dirname(HERE), "golden", "scintpar_timing.json")) as fh:
            ref = json.load(fh)["cases"]
    except OSError:
        ref = {}
    out = {"tool": "time_scintpar", "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "cases": {}}
    lines = []
    for n in a.sizes:
        o = field(n, n)

        def device_route():
            d = Dynspec(dyn=o, verbose=False)
            d.calc_acf()
            d.get_scint_params(method='nofit')
            d.get_acf_tilt(method='nofit')
            return d

        def parent_route():
            acf = scintpar.acf_device(to_device(o.dyn, torch.float64)).cpu().numpy()     # the parent's calc_acf: upload, ACF, download
            p = so.nofit(acf, o.dyn, o)
            p["tilt"] = so.acf_tilt(acf, o, p["tau"], p["dnu"])
            return p

        def cut_route():
            d = Dynspec(dyn=o, verbose=False)
            d.cut_dyn(tcuts=3, fcuts=3)
            return d

        d, p = device_route(), parent_route()
        assert (d.tau, d.dnu, d.amp, d.wn, d.nscint) == (p["tau"], p["dnu"], p["amp"], p["wn"], p["nscint"])
        assert (d.acf_tilt, d.acf_tilt_err, d.fse_tilt) == p["tilt"]
        np.testing.assert_allclose(d.modulation_index, p["modulation_index"], rtol=1e-12)
        rows = len(so.tilt_rows((2 * n, 2 * n), o, d.dnu))
        res = {"shape": [n, n], "tau": d.tau, "dnu": d.dnu, "tilt_rows": rows}
        nbytes = 8 * n * n
        copied = {"device_route": {"up": 2 * nbytes + 4 * rows, "down": 8 * 2 * n + 8 * 3 + rows * (4 + 4 + 56)},
                  "parent_route": {"up": nbytes, "down": 4 * nbytes},
                  # cutdyn + cutacf (4 x the pixels) + cutsspec [nrfft, ncfft] of 16 segments of n/4 x n/4
                  "cut_dyn_3_3": {"up": nbytes, "down": 8 * 16 * (5 * (n // 4) ** 2 + 2 * (2 ** int(np.ceil(np.log2(n // 4)))) ** 2)}}
        for name, fn in (("device_route", device_route), ("parent_route", parent_route), ("cut_dyn_3_3", cut_route)):
            def run():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)
            run()
            t = [run() for _ in range(a.repeats)]
            wall, dev = [x[0] for x in t], [x[1] for x in t]
            res[name] = {"wall_ms_median": round(statistics.median(wall), 3), "wall_ms_min": round(min(wall), 3),
                         "wall_ms_max": round(max(wall), 3), "device_ms_median": round(statistics.median(dev), 3),
                         "device_ms_min": round(min(dev), 3), "device_ms_max": round(max(dev), 3),
                         "bytes_up": int(copied[name]["up"]), "bytes_down": int(copied[name]["down"])}
        r = ref.get(f"{n}x{n}")
        if r:
            res["reference_cpu_s"] = {"scales_total": round(r["scales_total_s"], 3), "cut_dyn_3_3": round(r["cut_dyn_3_3_s"], 3)}
        out["cases"][f"{n}x{n}"] = res
        lines.append(f"{n}x{n}: device route {res['device_route']['wall_ms_median']} ms wall "
                     f"({res['device_route']['device_ms_median']} ms device, {res['device_route']['bytes_down']} B down), "
                     f"parent route {res['parent_route']['wall_ms_median']} ms wall ({res['parent_route']['device_ms_median']} ms "
                     f"device, {res['parent_route']['bytes_down']} B down), cut_dyn(3, 3) {res['cut_dyn_3_3']['wall_ms_median']} ms "
                     f"wall; medians of {a.repeats}, {out['device']}")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "scintpar_timing.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    with open(os.path.join(a.out, "scintpar_gpu.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
