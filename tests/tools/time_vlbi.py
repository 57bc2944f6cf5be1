#!/usr/bin/env python
"""Time ththmod.vlbi_retrieval_batch on a stack of tutorial-sized chunks and print one JSON line.

    python tests/tools/time_vlbi.py [--chunks 64] [--n-dish 2] [--size 64] [--npad 1] [--nedge 128] [--repeats 7] [--profile-once]

The chunks are the seeded multi-station fields of tests/vlbi_cases.py (size x size pixels, n_dish stations).  Two warm-up calls
(library load, workspace growth, FFT tables), then `repeats` timed calls bracketed by device synchronisation; the median and the
spread (min, max) are reported, per call and per chunk.  --profile-once: a single call after one warm-up, for a kernel trace."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=64)
    ap.add_argument("--n-dish", type=int, default=2)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--npad", type=int, default=1)
    ap.add_argument("--nedge", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--profile-once", action="store_true")
    a = ap.parse_args()
    import torch
    import vlbi_cases as vc
    from scintools_amd import ththmod

    cases = [vc.case(a.size, a.size, a.npad, a.n_dish, a.nedge, 0.8 + 0.01 * (k % 8), 500 + k) for k in range(a.chunks)]
    chunks = [(c["dlist"], c["edges"], c["time"], c["freq"], c["eta"]) for c in cases]

    def run(info=None):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ththmod.vlbi_retrieval_batch(chunks, a.npad, a.n_dish, 0.0, info=info)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    info = {}
    run(info)
    if a.profile_once:
        ms = [run()]
    else:
        run()
        ms = [run() for _ in range(a.repeats)]
    med = statistics.median(ms)
    print(json.dumps({"tool": "time_vlbi", "chunks": a.chunks, "n_dish": a.n_dish, "shape": [a.size, a.size], "npad": a.npad,
                      "nedge": a.nedge, "composite_n": int(info["composites"][0].shape[0]),
                      "lanczos_steps_median": int(statistics.median(info["iters"])), "repeats": len(ms),
                      "ms_per_call_median": round(med, 3), "ms_per_call_min": round(min(ms), 3), "ms_per_call_max": round(max(ms), 3),
                      "ms_per_chunk_median": round(med / a.chunks, 4), "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
