#!/usr/bin/env python
"""Time the batched arc fit beside the loop of single calls it replaces; print one JSON line and write arcfit_batch_timing.json.

    python tests/tools/time_arcfit_batch.py [--repeats 7] [--warmups 2] [--sizes 1024 4096] [--out profiles]

Input: the seeded correlated field of tests/tools/time_scintpar.py, n x n, cut into 64 x 64 and into 8 x 8 segments.  After `warmups`
runs, `repeats` timed ones bracketed by device synchronisation; median, min and max of

  fit_arc_cut_ms        Dynspec.fit_arc_cut(tcuts, fcuts) on an object whose cut_dyn has run (host clock): the batched call
  loop_ms               the single-call chain of fit_arc over the same segments of cutsspec, one after the other -- scint_block_std,
                        scint_norm_sspec, scint_masked_colavg, their read-backs and arcfit._arc_peak on the host --, which is what the
                        tree offered before fit_arc_cut (host clock, the same warm-ups and repeats; a pass over 4096 segments takes two seconds)
  speedup               loop_ms / fit_arc_cut_ms of the medians
  profile_ms            scint_arc_profile_batch alone on the stack (events on the stream), with the bytes it moves by the count of
                        DESIGN (B nr nc 8 read once, B nx 9 written), the rate that makes and its fraction of `plain_read_GBps`, a sum
                        over 1 GiB of float64 timed the same way
  peak_fit_ms           scint_arc_peak_fit alone on the profiles (events on the stream)

A segment whose loop fit raises (the reference's exceptions) counts as done.  No threshold: the figures are recorded."""
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
    a = ap.parse_args()
    import numpy as np
    import torch
    from time_scintpar import field
    from scintools_amd import arcfit as af
    from scintools_amd.dynspec import Dynspec
    warnings.simplefilter("ignore")
    out = {"tool": "time_arcfit_batch", "repeats": a.repeats, "warmups": a.warmups,
           "device": torch.cuda.get_device_name(0), "cases": {}}

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
    dev = lambda v: af.to_device(np.ascontiguousarray(v, dtype=float), torch.float64)
    for n in a.sizes:
        o = field(n, n)
        for cuts in (63, 7):
            d = Dynspec(dyn=o, verbose=False)
            d.cut_dyn(tcuts=cuts, fcuts=cuts)
            st = Dynspec.cutsspec.tensor(d)
            B, R, nc = (cuts + 1)**2, int(st.shape[2]), int(st.shape[3])
            st = st.view(B, R, nc)
            fdop = np.arange(-nc // 2, nc // 2) * (1e3 / (nc * d.dt))
            tdel = np.arange(R) / (2 * R * d.df)
            res = {"shape": [n, n], "problems": B, "spectrum": [R, nc]}
            res["fit_arc_cut_ms"] = timed(host, lambda: d.fit_arc_cut(tcuts=cuts, fcuts=cuts))
            # the same parameters as the batched call forms them (fit_arc's defaults)
            startbin, cutmid, ind = 3, 3, R - 1
            etamax = tdel[ind] / ((fdop[1] - fdop[0]) * cutmid)**2
            etamin = (tdel[1] - tdel[0]) * startbin / max(fdop)**2
            sq = np.linspace(np.sqrt(etamin), np.sqrt(etamax), 10000)
            nx = len(sq[(sq <= np.sqrt(etamax)) * (sq >= np.sqrt(etamin))])
            nx += nx % 2
            x = np.linspace(-1, 1, nx)
            nr = ind - startbin
            c_lo, c_hi, n_hi = nc // 2 - 1, nc // 2 + 1, nc // 2 + 2
            fd_t, y_t, x_t, w_t = dev(fdop), dev(tdel), dev(x), dev(np.ones(nr))
            div = float(np.sqrt(2 * ind))

            def loop():
                norm = af.empty((nr, nx), torch.float64)
                mask = af.empty((nr, nx), torch.uint8)
                pw = af.empty((nr,), torch.float64)
                avg = af.empty((nx,), torch.float64)
                none = af.empty((nx,), torch.uint8)
                std = af.empty((1,), torch.float64)
                for k in range(B):
                    ws = af.workspace.get(8 * 1032)
                    af._lib.call("scint_block_std", st[k], nc, nc, R // 2, R, c_lo, n_hi, std, ws, ws.numel(), af.stream_ptr())
                    noise = float(std.cpu().numpy()[0]) / div
                    af._lib.call("scint_norm_sspec", st[k], nc, nc, fd_t, y_t, startbin, nr, etamin, 1.0, c_lo, c_hi, None, x_t, None,
                                 nx, norm, mask, pw, af.stream_ptr())
                    pw.cpu()                                   # norm_sspec reads the power spectrum back
                    ws = af.workspace_for("scint_masked_colavg", nr, nx)
                    af._lib.call("scint_masked_colavg", norm, mask, nr, nx, w_t, None, avg, none, ws, ws.numel(), af.stream_ptr())
                    prof = np.ma.array(avg.cpu().numpy(), mask=none.cpu().numpy().astype(bool))
                    spec = np.array(np.add(prof[nx // 2:], np.flip(prof[:nx // 2], axis=0)) / 2).squeeze()
                    try:
                        af._arc_peak(spec, 1 / x[nx // 2:], etamin, etamax, noise=noise)
                    except (ValueError, IndexError, TypeError, np.linalg.LinAlgError):
                        pass

            res["loop_ms"] = timed(host, loop)
            res["speedup"] = round(res["loop_ms"]["median"] / res["fit_arc_cut_ms"]["median"], 1)
            res["profile_ms"] = timed(events, lambda: af.arc_profile_stack_device(st, fd_t, y_t, startbin, nr, etamin, 1.0, c_lo, c_hi,
                                                                                   c_lo, n_hi, x_t))
            per = 8 * nr * nc + 9 * nx
            rate = B * per / (res["profile_ms"]["median"] * 1e-3) / 1e9
            res["bytes_per_problem"] = {"spectrum_read": 8 * nr * nc, "profile_written": 9 * nx, "total": per}
            res["nx"] = nx
            res["profile_GBps"] = round(rate, 2)
            res["fraction_of_plain_read"] = round(rate / out["plain_read_GBps"], 4)
            avg_t, _, noise_t = af.arc_profile_stack_device(st, fd_t, y_t, startbin, nr, etamin, 1.0, c_lo, c_hi, c_lo, n_hi, x_t)
            res["peak_fit_ms"] = timed(events, lambda: af.arc_peak_fit_device(avg_t, noise_t, div, x_t, etamin, etamax))
            res["statuses"] = {str(k): int(v) for k, v in zip(*np.unique(d.cut_arc_status, return_counts=True))}
            out["cases"][f"{n}x{n}/{cuts}"] = res
            print(f"{n}x{n} cuts {cuts}", json.dumps(res), flush=True)
            del d, st, avg_t, noise_t
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "arcfit_batch_timing.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
