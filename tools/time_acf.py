#!/usr/bin/env python
"""Time scintools_amd.scint_sim.ACF -- the theoretical 2-D ACF model -- at the default size, ar=3, ar=10 and ar=3 with a phase gradient,
beside the unmodified reference's host times (tests/golden/acf_timing.json, tests/golden/time_reference_acf.py).

    python tools/time_acf.py [--cases default ar3 ar10 ar3_phasegrad] [--warmup 2] [--reps 7]

Per case: the whole constructor (host axes, uploads, the five launches, the read-back and the host mirroring) and the device call
alone (scint_acf_model on resident tensors, synchronised around the timed region): two warm-up calls, then the median and the min-max
spread of seven.  Beside each: the GEMM flops 4 nsn (M2^2 + (ndnun - 2) M^2), the sincos count 2 nsn (M2 + (ndnun - 2) M), the
achieved float64 rate of the device call and the speed-up of the constructor over the reference.  Not a test and not part of
bench.py.  Writes profiles/acf_timing.json."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
CASES = {"default": dict(), "ar3": dict(ar=3), "ar10": dict(ar=10), "ar3_phasegrad": dict(ar=3, phasegrad=0.5, theta=30)}


def stats(secs):
    return {"median_ms": round(1e3 * float(np.median(secs)), 4), "min_ms": round(1e3 * min(secs), 4), "max_ms": round(1e3 * max(secs), 4),
            "reps": len(secs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=list(CASES), choices=list(CASES))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "acf_timing.json"))
    args = ap.parse_args()
    import torch
    from scintools_amd import _lib, device, scint_sim
    dev = device.require_gpu()
    lib = _lib.load()
    try:
        with open(os.path.join(REPO, "tests", "golden", "acf_timing.json")) as fh:
            ref = json.load(fh)["cases"]
    except OSError:
        ref = {}
    out = {"what": "scint_sim.ACF; times in ms", "device": torch.cuda.get_device_name(dev), "cases": {}}

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

    for name in args.cases:
        kw = CASES[name]
        captured = {}
        inner = scint_sim.ACF._device_field

        def capture(*a):
            captured["args"] = a
            return inner(*a)

        scint_sim.ACF._device_field = staticmethod(capture)
        try:
            scint_sim.ACF(**kw)
        finally:
            scint_sim.ACF._device_field = staticmethod(inner)
        snp, snp2, snx, sny, dnun, sigxn, sigyn, sqrtar, alph2, step, step2 = captured["args"]
        m, m2, nsn, ndnun = len(snp), len(snp2), len(snx), len(dnun)
        rec = {"kwargs": kw, "M": m, "M2": m2, "nsn": nsn, "ndnun": ndnun,
               "gemm_flops": 4.0 * nsn * (m2 ** 2 + (ndnun - 2) * m ** 2), "sincos": 2.0 * nsn * (m2 + (ndnun - 2) * m)}
        rec["constructor"] = timed(lambda: scint_sim.ACF(**kw))
        need = ctypes.c_size_t()
        _lib.check(lib.scint_acf_model_workspace_bytes(m, m2, nsn, ndnun, ctypes.byref(need)), "workspace_bytes")
        ws = device.workspace.get(need.value)
        d = [device.to_device(a, torch.float64) for a in (snp, snp2, snx, sny, dnun)]
        gammes = torch.empty((m, m), dtype=torch.float64, device=dev)
        gamma = torch.zeros((nsn, ndnun), dtype=torch.complex128, device=dev)

        def call():
            _lib.check(lib.scint_acf_model(device.ptr(d[0]), m, device.ptr(d[1]), m2, device.ptr(d[2]), device.ptr(d[3]), nsn,
                                           device.ptr(d[4]), ndnun, sigxn, sigyn, sqrtar, alph2, step, step2, device.ptr(gammes),
                                           device.ptr(gamma), device.ptr(ws), need.value, device.stream_ptr()), "scint_acf_model")
        rec["device_call"] = timed(call)
        rec["workspace_MiB"] = round(need.value / 2 ** 20, 2)
        sec = rec["device_call"]["median_ms"] * 1e-3
        rec["gemm_tflops"] = round(rec["gemm_flops"] / sec / 1e12, 3)
        rec["sincos_per_s"] = round(rec["sincos"] / sec, 1)
        host = ref.get(name, {}).get("seconds")
        rec["reference_seconds"] = host if host is not None else ref.get(name, {}).get("not_run", "not recorded")
        if host is not None:
            rec["speedup_constructor"] = round(host / (rec["constructor"]["median_ms"] * 1e-3), 1)
        print(json.dumps({name: rec}), flush=True)
        out["cases"][name] = rec
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
