#!/usr/bin/env python
"""Time scintools_amd.scint_sim.Simulation on the BASELINE screen (oracle/sim_oracle.py: BASELINE_SCREEN), nx = nf = 1024, 2048, 4096
with ny = 128, beside the host restatement (oracle/sim_oracle.py) on one core and with its worker pool on the same machine.

    python tools/time_simulation.py [--sizes 1024 2048 4096] [--reps 5] [--oracle-serial-max 4096] [--oracle-pool-max 4096]

Per size: the host draw of the 2 nx ny normals and their upload (timed apart from the device work), the screen call, the field call
(scint_sim_field on resident tensors, synchronised around the timed region; one warm-up, then the median and the min-max spread of
`--reps` repetitions), the field call again with SCINT_SIM_COLUMN=0 (full inverse transforms) and with a 1 GiB group, the whole
constructor, and the bytes the field moves per frequency against the plain-read rate README.md quotes (6.0 TB/s).  Not a test and not
part of bench.py.  Writes profiles/sim_timing.json."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PLAIN_READ = 6.0e12      # bytes/s, README.md: the sweep's dominant kernel at 5.7-5.9 TB/s is 0.96-0.97 of a plain read


def stats(secs):
    return {"median_ms": round(1e3 * float(np.median(secs)), 4), "min_ms": round(1e3 * min(secs), 4), "max_ms": round(1e3 * max(secs), 4),
            "reps": len(secs)}


def col_passes(n):
    l = int(np.log2(n))
    p, r = l // 4, l % 4
    return p if (r == 0 or (r == 1 and p > 0)) else p + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048, 4096])
    ap.add_argument("--ny", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--oracle-serial-max", type=int, default=4096)
    ap.add_argument("--oracle-pool-max", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sim_timing.json"))
    args = ap.parse_args()
    import torch
    from oracle import sim_oracle
    from scintools_amd import _lib, device, scint_sim
    dev = device.require_gpu()
    lib = _lib.load()
    out = {"what": "scint_sim.Simulation, BASELINE screen, ny = %d; times in ms" % args.ny, "device": torch.cuda.get_device_name(dev),
           "plain_read_bytes_per_s": PLAIN_READ, "sizes": {}}

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        secs = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        return stats(secs)

    for n in args.sizes:
        nx = nf = n
        ny = args.ny
        kw = dict(nx=nx, ny=ny, nf=nf, seed=1, **sim_oracle.BASELINE_SCREEN)
        rec = {"nx": nx, "ny": ny, "nf": nf}
        t0 = time.perf_counter()
        rs = np.random.RandomState(1)
        z = [rs.randn(nx, ny), rs.randn(nx, ny)]
        rec["host_draw_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
        rec["upload"] = timed(lambda: [torch.from_numpy(a).to(dev) for a in z], args.reps)
        rec["constructor_total"] = timed(lambda: scint_sim.Simulation(**kw), max(2, args.reps // 2))
        s = scint_sim.Simulation(**kw)
        rec["screen_and_readback"] = timed(s.get_screen, args.reps)
        xyp = device.to_device(s.xyp, torch.float64)
        scale = device.to_device(s._scales(), torch.float64)
        spe = torch.empty((nx, nf), dtype=torch.complex64, device=dev)
        spi = torch.empty((nx, nf), dtype=torch.float32, device=dev)
        xyi = torch.empty((nx, ny), dtype=torch.float64, device=dev)

        def field(group_bytes):
            one, two, need = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
            lib.scint_sim_field_workspace_bytes(nx, ny, 1, ctypes.byref(one))
            lib.scint_sim_field_workspace_bytes(nx, ny, 2, ctypes.byref(two))
            group = int(min(nf, max(1, 1 + (group_bytes - one.value) // (two.value - one.value))))
            _lib.check(lib.scint_sim_field_workspace_bytes(nx, ny, group, ctypes.byref(need)), "workspace_bytes")
            ws = device.workspace.get(need.value)

            def call():
                _lib.check(lib.scint_sim_field(device.ptr(xyp), nx, ny, device.ptr(scale), nf, 0, nf, float(s.ffconx), float(s.ffcony),
                                               device.ptr(spe), device.ptr(spi), device.ptr(xyi), device.ptr(ws), need.value,
                                               device.stream_ptr()), "scint_sim_field")
            return call, group

        call, group = field(scint_sim.SIM_GROUP_BYTES)
        rec["field"] = dict(timed(call, args.reps), group=group, route=scint_sim.last_route())
        per_freq = nx * ny * (40 + 32 * (col_passes(nx) - 1)) + 3 * 16 * nx
        sec = rec["field"]["median_ms"] * 1e-3 / nf
        rec["field"].update(bytes_per_frequency=per_freq, us_per_frequency=round(1e6 * sec, 3),
                            fraction_of_plain_read=round(per_freq / sec / PLAIN_READ, 4),
                            sincos_per_s=round(2.0 * nx * ny / sec, 1))
        call, group = field(1 << 30)
        rec["field_group_1GiB"] = dict(timed(call, args.reps), group=group)
        os.environ["SCINT_SIM_COLUMN"] = "0"
        call, group = field(scint_sim.SIM_GROUP_BYTES)
        rec["field_full_transform"] = dict(timed(call, max(2, args.reps // 2)), group=group, route=scint_sim.last_route())
        del os.environ["SCINT_SIM_COLUMN"]
        okw = dict(nx=nx, ny=ny, nf=nf, seed=1, **sim_oracle.BASELINE_SCREEN)
        if n <= args.oracle_pool_max:
            w = sim_oracle.default_workers()
            t0 = time.perf_counter()
            o = sim_oracle.Simulation(workers=w, **okw)
            rec["oracle_pool"] = {"seconds": round(time.perf_counter() - t0, 3), "workers": w}
            rec["spe_not_bit_identical_to_oracle"] = float(np.mean(o.spe != s.spe))
            rec["spe_max_rel_diff_to_oracle"] = float((np.abs(o.spe - s.spe) / np.abs(o.spe).max()).max())
        else:
            rec["oracle_pool"] = {"skipped": "size above --oracle-pool-max %d" % args.oracle_pool_max}
        if n <= args.oracle_serial_max:
            t0 = time.perf_counter()
            sim_oracle.Simulation(workers=1, **okw)
            rec["oracle_one_core"] = {"seconds": round(time.perf_counter() - t0, 3)}
        else:
            rec["oracle_one_core"] = {"skipped": "size above --oracle-serial-max %d" % args.oracle_serial_max}
        print(json.dumps({n: rec}), flush=True)
        out["sizes"][str(n)] = rec
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
