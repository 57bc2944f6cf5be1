#!/usr/bin/env python
"""Generate tests/golden/scintpar.npz, tests/golden/scintpar_cut.npz (the cut_dyn stacks) and tests/golden/scintpar_tolerances.json by running the UNMODIFIED reference's
Dynspec.get_scint_params(method='nofit') / get_acf_tilt(method='nofit') / cut_dyn / calc_acf(method='sspec')
(scintools/dynspec.py:2470-2648, 2283-2413, 3158-3271, 3798-3807) with the stand-ins of tests/golden/refshim, as the other
make_golden_* scripts do (lmfit's stand-in raises: method='nofit' returns before it is touched).

    SCINTOOLS_REFERENCE=<checkout of the reference> python tests/golden/make_golden_scintpar.py [--timing [sizes ...]]

Inputs: the seeded observations and synthetic ACFs of tests/scintpar_cases.py.  Stored: the inputs (`in_<case>_*`; the
simulator's float32 dynamic spectra as float32), per observation and variant `<case>_<variant>_<attribute>`, the tilt
`<case>_tilt_<attribute>`, `holes_<attribute>`, the tie fixture `tie_acf` with `tie_<attribute>`, `<case>_cutdyn` /
`<case>_cutsspec` and `<case>_acf_sspec` as float64.

The fixture conditions are CHECKED here, on the reference's own ACF: every threshold crossing (amp/e, amp/2, argmin|y - amp/2|)
has a margin of at least 1e-9, at least two samples lie below each threshold, every fitted row's maximum is at least 3 columns
from an edge and leads the row's second-largest sample by more than 1e-9 (the tie fixture's tied rows excepted: they tie
exactly).  scintpar_tolerances.json: per observation the largest change of acf_tilt / acf_tilt_err / fse_tilt when the
reference's ACF is perturbed by +-1e-12 (the bound of the calc_acf parity test) over 32 seeded draws, measured with
tests/scintpar_oracle.py on the REFERENCE's ACF; and the bound of the 'sspec' ACF, 1e-10 of its maximum unless the CPU oracle
already differs from the reference by more (then 10 x that worst case).
--timing also writes tests/golden/scintpar_timing.json: the reference's CPU time of calc_acf + get_scint_params + get_acf_tilt
and of cut_dyn(3, 3) at the sizes tests/tools/time_scintpar.py runs on the device."""
import json
import os
import sys
import time
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "refshim"))
sys.path.insert(0, os.environ["SCINTOOLS_REFERENCE"])
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)

import matplotlib  # noqa: E402
matplotlib.use("Agg")
import numpy as np  # noqa: E402
from scintools.dynspec import Dynspec  # noqa: E402
import scintpar_cases as cc  # noqa: E402
import scintpar_oracle as so  # noqa: E402

warnings.simplefilter("ignore")
MARGIN = 1e-9
PERTURB = 1e-12
DRAWS = 32


def ref(obs):
    return Dynspec(dyn=obs, process=False, verbose=False)


def check_fixture(case, acf, o, dnu, tied_rows=()):
    cross, gap, below_t, below_f = so.nofit_margins(acf, o)
    assert cross >= MARGIN and gap >= 2 * MARGIN, (case, cross, gap)
    assert below_t >= 2 and below_f >= 2, (case, below_t, below_f)
    inds = so.tilt_rows(acf.shape, o, dnu)
    edge, _ = so.tilt_peak_margins(acf, inds)
    free = np.array([ii for ii in inds if int(ii[0]) not in tied_rows])
    _, lead = so.tilt_peak_margins(acf, free)
    assert edge >= 3 and lead > MARGIN, (case, edge, lead)
    print(f"  fixture {case}: crossing margin {cross:.2e}, half-power gap {gap:.2e}, below 1/e {below_t}, below 1/2 {below_f}, "
          f"rows {len(inds)}, peak to edge {edge}, peak lead {lead:.2e}")


def timing():
    from oracle import sim_oracle
    out = {"what": "CPU seconds of the unmodified reference (one run each; calc_acf + get_scint_params(method='nofit') + "
                   "get_acf_tilt(method='nofit'), and cut_dyn(3, 3)) on seeded simulations", "cases": {}}
    sizes = [int(v) for v in sys.argv[sys.argv.index("--timing") + 1:]] or [1024, 4096]
    for n in sizes:
        s = sim_oracle.Simulation(mb2=2, ar=1, dlam=0.25, dt=30, freq=1400, ns=n, nf=n, seed=n)
        o = cc.observation(np.asarray(s.dyn, dtype=np.float64), s.freqs, s.times, s.df, s.dt, s.freq)
        d = ref(o)
        t0 = time.perf_counter()
        d.calc_acf()
        t1 = time.perf_counter()
        d.get_scint_params(method='nofit')
        t2 = time.perf_counter()
        d.get_acf_tilt(method='nofit')
        t3 = time.perf_counter()
        d.cut_dyn(3, 3)
        t4 = time.perf_counter()
        out["cases"][f"{n}x{n}"] = {"calc_acf_s": t1 - t0, "get_scint_params_s": t2 - t1, "get_acf_tilt_s": t3 - t2,
                                    "scales_total_s": t3 - t0, "cut_dyn_3_3_s": t4 - t3}
        print(n, out["cases"][f"{n}x{n}"], flush=True)
    with open(os.path.join(HERE, "scintpar_timing.json"), "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    if "--timing" in sys.argv:
        timing()
        sys.exit(0)
    arrs, tol = {}, {"perturbation": PERTURB, "draws": DRAWS, "tilt_spread": {}}
    obs = cc.build_all()
    cc.store(obs, arrs)
    for case in cc.OBS:
        o = obs[case]
        acf = None
        for variant, kw in cc.VARIANTS.items():
            d = ref(o)
            d.get_scint_params(method='nofit', **kw)
            for name in cc.NOFIT_ATTRS:
                arrs[f"{case}_{variant}_{name}"] = np.asarray(getattr(d, name), dtype=float)
            assert d.scint_param_method == 'nofit'
            acf = d.acf
        d = ref(o)
        d.get_acf_tilt(method='nofit')
        for name in cc.TILT_ATTRS:
            arrs[f"{case}_tilt_{name}"] = np.asarray(getattr(d, name), dtype=float)
        print(case, o.dyn.shape, "tau", d.tau, "dnu", d.dnu, "nscint", d.nscint, "tilt", d.acf_tilt, d.acf_tilt_err, d.fse_tilt)
        check_fixture(case, acf, o, d.dnu)
        # the oracle on the reference's ACF is the reference, bit for bit
        p = so.nofit(acf, o.dyn, o)
        assert all(p[k] == arrs[f"{case}_default_{k}"] for k in cc.NOFIT_ATTRS), case
        base = so.acf_tilt(acf, o, d.tau, d.dnu)
        assert base == (d.acf_tilt, d.acf_tilt_err, d.fse_tilt), case
        rng = np.random.default_rng(20241019)
        spread = np.zeros(3)
        for _ in range(DRAWS):
            got = so.acf_tilt(acf + PERTURB * rng.uniform(-1, 1, acf.shape), o, d.tau, d.dnu)
            spread = np.maximum(spread, np.abs(np.array(got) - np.array(base)))
        tol["tilt_spread"][case] = dict(zip(cc.TILT_ATTRS, spread.tolist()))
        print("  tilt spread under +-1e-12:", tol["tilt_spread"][case])

    # the moments skip NaN, inf and zero pixels: poked in after the ACF was taken (calc_acf of a NaN is all NaN)
    d = ref(obs["even"])
    d.calc_acf()
    d.dyn = cc.poke_holes(d.dyn)
    d.get_scint_params(method='nofit')
    for name in cc.NOFIT_ATTRS:
        arrs[f"holes_{name}"] = np.asarray(getattr(d, name), dtype=float)
    print("holes", "dnu_est", d.dnu_est, "m", d.modulation_index)

    # exact ties of the row maximum
    o = cc.synthetic_observation()
    d = ref(o)
    d.acf = cc.tie_acf()
    for row in cc.tie_rows():
        assert (d.acf[row] == d.acf[row].max()).sum() == 2, row
    d.get_acf_tilt(method='nofit')
    arrs["tie_acf"] = np.array(d.acf, dtype=np.float64)
    for name in cc.NOFIT_ATTRS + cc.TILT_ATTRS:
        arrs[f"tie_{name}"] = np.asarray(getattr(d, name), dtype=float)
    print("tie", "tau", d.tau, "dnu", d.dnu, "tilt", d.acf_tilt, d.acf_tilt_err, d.fse_tilt)
    check_fixture("tie", d.acf, o, d.dnu, tied_rows=tuple(cc.tie_rows()))
    assert set(cc.tie_rows()) <= set(int(i[0]) for i in so.tilt_rows(d.acf.shape, o, d.dnu))

    for case, (tcuts, fcuts) in cc.CUTS.items():
        d = ref(obs[case])
        d.cut_dyn(tcuts=tcuts, fcuts=fcuts)
        arrs[f"{case}_cutdyn"] = np.array(d.cutdyn, dtype=np.float64)
        arrs[f"{case}_cutsspec"] = np.array(d.cutsspec, dtype=np.float64)
        print(case, "cut_dyn", d.cutdyn.shape, d.cutsspec.shape)

    tol["acf_sspec_bound"] = {}
    for case in cc.SSPEC_ACF:
        d = ref(obs[case])
        d.calc_acf(method='sspec')
        arrs[f"{case}_acf_sspec"] = np.array(d.acf, dtype=np.float64)
        worst = float(np.abs(so.acf_sspec(obs[case].dyn) - d.acf).max() / np.abs(d.acf).max())
        tol["acf_sspec_bound"][case] = {"oracle_vs_reference": worst, "bound": 1e-10 if worst <= 1e-10 else 10 * worst}
        print(case, "acf(sspec)", d.acf.shape, "oracle vs reference", worst, "finite", np.isfinite(d.acf).all())

    # the segment stacks go into a file of their own: float64 spectra do not compress, and a committed file stays below 1 MiB
    cuts = {k: arrs.pop(k) for k in [k for k in arrs if k.endswith(("_cutdyn", "_cutsspec"))]}
    for fname, part in (("scintpar.npz", arrs), ("scintpar_cut.npz", cuts)):
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **part)
        print(f"{fname}: {os.path.getsize(path) / 1024:.0f} KiB, {len(part)} arrays")
        assert os.path.getsize(path) < (1 << 20)
    with open(os.path.join(HERE, "scintpar_tolerances.json"), "w") as fh:
        json.dump(tol, fh, indent=1)
