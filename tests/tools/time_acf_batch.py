#!/usr/bin/env python
"""Time the batched ACF and the per-segment products that run on it; print one JSON line and write acf_batch_timing.json.

    python tests/tools/time_acf_batch.py [--repeats 7] [--warmups 2] [--sizes 1024 4096] [--out profiles] [--parent FILE]

Input: the seeded correlated field of tests/tools/time_scintpar.py, n x n, cut with tcuts = fcuts = 63 into 4096 segments of
n/64 x n/64.  After `warmups` runs, `repeats` timed ones bracketed by device synchronisation; median, min and max of

  acf_stack_ms          scintpar.acf_stack_device on the prepared stack of segments, output preallocated (events on the stream)
  fit_cut_ms            Dynspec.fit_scint_params_cut(63, 63), the whole call (host clock)
  fit_2d_cut_ms         Dynspec.fit_scint_params_2d_cut(63, 63), the whole call (host clock)
  cut_dyn_ms            Dynspec.cut_dyn(63, 63) without reading a stack (host clock)
  cut_dyn_read_ms       ... and reading cutdyn, cutsspec and cutacf (host clock)

With acf_stack_ms: the bytes one problem moves by the count of DESIGN 4s (the segment read, the complex intermediate of
16 * 2nf * 2nt bytes written and read twice, the ACF written), the rate that makes, and its fraction of `plain_read_GBps`, a sum over
1 GiB of float64 timed the same way.  The tool also runs on a tree without acf_stack_device (the parent of the change that added
it): it then leaves acf_stack_ms out.  `--parent FILE` folds such a run's figures in under "parent".  No threshold: the figures
are recorded."""
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
sys.path.insert(0, HERE)


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(HERE)), "profiles"))
    ap.add_argument("--parent", default=None)
    a = ap.parse_args()
    import torch
    from time_scintpar import field
    from scintools_amd import device, scintpar
    from scintools_amd.dynspec import Dynspec
    warnings.simplefilter("ignore")
    batched = hasattr(scintpar, "acf_stack_device")
    out = {"tool": "time_acf_batch", "repeats": a.repeats, "warmups": a.warmups, "device": torch.cuda.get_device_name(0),
           "batched": batched, "cases": {}}

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def host(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def timed(clock, fn):
        for _ in range(a.warmups):
            clock(fn)
        return spread([clock(fn) for _ in range(a.repeats)])

    big = torch.ones(1 << 27, dtype=torch.float64, device="cuda")
    ms = timed(events, lambda: torch.sum(big))
    out["plain_read_GBps"] = round(big.numel() * 8 / (ms["median"] * 1e-3) / 1e9, 1)
    del big
    for n in a.sizes:
        o = field(n, n)
        fnum = tnum = n // 64
        B = 4096
        res = {"shape": [n, n], "problems": B, "segment": [fnum, tnum]}
        if batched:
            segs = scintpar.segment_cut_device(device.to_device(o.dyn, torch.float64), fnum, tnum, 64, 64)
            acfs = device.empty((B, 2 * fnum, 2 * tnum), torch.float64)
            res["acf_stack_ms"] = timed(events, lambda: scintpar.acf_stack_device(segs, out=acfs))
            per = 8 * fnum * tnum + 2 * 2 * 16 * 4 * fnum * tnum + 8 * 4 * fnum * tnum
            rate = B * per / (res["acf_stack_ms"]["median"] * 1e-3) / 1e9
            res["bytes_per_problem"] = {"segment_read": 8 * fnum * tnum, "complex_intermediate": 16 * 4 * fnum * tnum,
                                        "intermediate_written_and_read": 2, "acf_written": 8 * 4 * fnum * tnum, "total": per}
            res["acf_stack_GBps"] = round(rate, 1)
            res["fraction_of_plain_read"] = round(rate / out["plain_read_GBps"], 3)
            del segs, acfs

        def read_all():
            d = Dynspec(dyn=o, verbose=False)
            d.cut_dyn(tcuts=63, fcuts=63)
            return d.cutdyn.shape, d.cutsspec.shape, d.cutacf.shape

        res["fit_cut_ms"] = timed(host, lambda: Dynspec(dyn=o, verbose=False).fit_scint_params_cut(tcuts=63, fcuts=63))
        res["fit_2d_cut_ms"] = timed(host, lambda: Dynspec(dyn=o, verbose=False).fit_scint_params_2d_cut(tcuts=63, fcuts=63))
        res["cut_dyn_ms"] = timed(host, lambda: Dynspec(dyn=o, verbose=False).cut_dyn(tcuts=63, fcuts=63))
        res["cut_dyn_read_ms"] = timed(host, read_all)
        out["cases"][f"{n}x{n}"] = res
        print(f"{n}x{n}", json.dumps(res), flush=True)
    if a.parent:
        with open(a.parent) as fh:
            out["parent"] = json.load(fh)["cases"]
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "acf_batch_timing.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
