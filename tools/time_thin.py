"""Time the thin-screen curvature search (fitting_proc='thin') on one GPU and print ONE JSON line.

    python tools/time_thin.py [--skip-cpu] [--out profiles/thin_line.json]

Workloads:
  tutorial   the tutorial recipe (Sample_Data via tests/golden/fit_thetatheta.npz: cwf=64, edges_lim=.3, eta 30..50,
             arclet_lim=.15, center_cut=.02), Dynspec.fit_thetatheta (16 chunks x 52 curvatures);
  obs4096    arc_dynspec(4096, 4096, seed=3, nimg=64), cwf = cwt = 256, npad = 3, eta 0.5..2 eta_true,
             fitting_proc='thin' -- the observation of bench.py --workload fit_thetatheta.  Its thin maps are ~4700 x 4700
             (edges to fd.max()), 140 per chunk and 256 chunks: 13 TB per Lanczos step in all, so only the first
             --obs-chunks chunks (default 1) of the observation are fitted, with the observation's own parameters, and
             the whole observation is extrapolated from them.
Per workload: seconds (median of the timed repeats after one warm-up), curvatures per second, Lanczos steps per
curvature, the algorithmic bytes sum(16 n1 n2 steps) of the mat-vecs and that over the seconds as a fraction of the 8 TB/s
HBM peak.  For obs4096 also (unless --skip-cpu) the seconds of the host oracle's singularvalue_calc (tests/thin_oracle.py, a
dense np.linalg.svd as the reference) at one curvature of the first chunk, scaled to the whole observation, as context.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

HBM_PEAK = 8.0e12


def _instrument(thth):
    """Record the per-curvature (n1, n2, steps) of every sv_sweep_multi call."""
    log = []
    orig = thth.sv_sweep_multi

    def wrapped(*a, **k):
        k = dict(k, return_info=True)
        out, info = orig(*a, **k)
        r = info["ranges"]
        log.append((r[:, 3].astype(np.int64), r[:, 1].astype(np.int64), np.asarray(info["iters"], dtype=np.int64)))
        return out
    thth.sv_sweep_multi = wrapped
    return log, orig


def _run(make, reps):
    import torch
    from scintools_amd import ththmod as thth
    log, orig = _instrument(thth)
    try:
        d = make()
        d.fit_thetatheta()                        # warm-up (library load, workspace, first launches)
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            log.clear()
            d = make()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d.fit_thetatheta()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
    finally:
        thth.sv_sweep_multi = orig
    n1 = np.concatenate([x[0] for x in log])
    n2 = np.concatenate([x[1] for x in log])
    it = np.concatenate([x[2] for x in log])
    s = float(np.median(times))
    nbytes = float(np.sum(16.0 * n1 * n2 * it))
    return d, {"seconds": round(s, 5), "seconds_all": [round(t, 5) for t in times], "neta_total": int(n1.size),
               "eta_per_s": round(n1.size / s, 1), "steps_per_eta_mean": round(float(it.mean()), 2),
               "steps_per_eta_max": int(it.max()), "n1_mean": round(float(n1.mean()), 1), "n2_mean": round(float(n2.mean()), 1),
               "matvec_bytes": nbytes, "hbm_fraction": round(nbytes / s / HBM_PEAK, 4), "ththeta": float(d.ththeta)}


def tutorial(reps):
    from scintools_amd.dynspec import Dynspec
    f = np.load(os.path.join(REPO, "tests", "golden", "fit_thetatheta.npz"))

    class B:
        dyn, freqs, times, dt, df = f["dspec"], f["freq"], f["time"], float(f["dt"]), float(f["df"])

    def make():
        d = Dynspec(dyn=B(), verbose=False)
        d.prep_thetatheta(cwf=64, edges_lim=.3, eta_min=30, eta_max=50, fitting_proc='thin', arclet_lim=.15, center_cut=.02)
        return d
    return _run(make, reps)[1]


def obs4096(reps, skip_cpu, nchunks):
    from scintools_amd.dynspec import Dynspec
    from scintools_amd.synth import arc_dynspec
    dyn, freqs, times, eta_true = arc_dynspec(4096, 4096, seed=3, nimg=64)

    class B:
        pass
    B.dyn, B.freqs, B.times = dyn, freqs, times
    B.dt, B.df = float(times[1] - times[0]), float(freqs[1] - freqs[0])

    def make():
        d = Dynspec(dyn=B(), verbose=False)
        d.prep_thetatheta(cwf=256, cwt=256, npad=3, eta_min=0.5 * eta_true, eta_max=2.0 * eta_true, fitting_proc='thin')
        d.ncf_fit, d.nct_fit = 1, nchunks          # the first chunks of frequency row 0, everything else as prepared
        return d
    full = Dynspec(dyn=B(), verbose=False)
    full.prep_thetatheta(cwf=256, cwt=256, npad=3, eta_min=0.5 * eta_true, eta_max=2.0 * eta_true, fitting_proc='thin')
    nall = int(full.ncf_fit * full.nct_fit)
    d, res = _run(make, reps)
    res["chunks_timed"] = nchunks
    res["chunks_in_observation"] = nall
    res["neta_per_chunk"] = int(d.neta)
    res["nedge"] = int(d.edges.shape[0])
    res["whole_observation_s_est"] = round(res["seconds"] * nall / nchunks, 2)
    if not skip_cpu:
        import thin_oracle
        p = d._search_params_thin(0, 0)
        fd, tau = thin_oracle.fft_axis(p[2], 1000.0, 3), thin_oracle.fft_axis(p[1], 1.0, 3)
        pad = np.pad(p[0], ((0, 3 * 256), (0, 3 * 256)), mode="constant", constant_values=p[0].mean())
        CS = np.fft.fftshift(np.fft.fft2(pad))
        e = p[3][len(p[3]) // 2]
        t0 = time.perf_counter()
        thin_oracle.singularvalue_calc(CS, tau, fd, e, p[4], e, p[11], p[12])
        one = time.perf_counter() - t0
        res["cpu_oracle_one_eta_s"] = round(one, 2)
        res["cpu_oracle_whole_obs_s_est"] = round(one * d.neta * nall, 0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--obs-chunks", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    line = {"what": "thin-screen fit_thetatheta (sv_sweep_multi: gather + Lanczos on A^H A), one GPU",
            "device": torch.cuda.get_device_name(0), "tutorial": tutorial(a.reps), "obs4096": obs4096(a.reps, a.skip_cpu, a.obs_chunks)}
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
