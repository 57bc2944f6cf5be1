#!/usr/bin/env python
"""Generate tests/golden/thin.npz (and thin_timing.json) by running the UNMODIFIED reference's thin-screen
search (/root/reference/scintools) with the stand-ins of tests/golden/refshim, as make_golden.py does.

    python tests/golden/make_golden_thin.py

Every array is produced by the reference's own functions: ``ththmod.two_curve_map``, ``singularvalue_calc``,
``fft_axis`` and ``Dynspec.prep_thetatheta / thetatheta_single / fit_thetatheta`` with ``fitting_proc='thin'``.
Re-running it reproduces every array of thin.npz bit for bit; the reference's wall-clock seconds go to
thin_timing.json.  The tutorial dynamic spectrum itself is not copied (fit_thetatheta.npz holds it).
"""
import json
import os
import sys
import time
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "refshim"))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, REPO)

import matplotlib  # noqa: E402
matplotlib.use("Agg")
import numpy as np  # noqa: E402
import astropy.units as u  # noqa: E402  (the shim)
import scintools.ththmod as thth  # noqa: E402
from scintools.dynspec import Dynspec, BasicDyn  # noqa: E402
from scintools_amd.synth import arc_dynspec  # noqa: E402

warnings.simplefilter("ignore")


def V(q):
    return np.array(getattr(q, "value", q))


def small_case():
    """two_curve_map and singularvalue_calc on a small analytic arc (npad = 0, thin edges out to fd.max())."""
    dyn, freqs, times, eta_true = arc_dynspec(64, 64, seed=3, nimg=10)
    dyn = dyn - dyn.mean()
    fd = thth.fft_axis(times * u.s, u.mHz, 0)
    tau = thth.fft_axis(freqs * u.MHz, u.us, 0)
    CS = np.fft.fftshift(np.fft.fft2(dyn))
    fdm = V(fd).max()
    edges = np.linspace(-fdm, fdm, 64)
    arclet = edges[np.abs(edges) < 0.6 * fdm]
    out = dict(dyn=dyn, freqs=freqs, times=times, fd=V(fd), tau=V(tau), eta_true=eta_true, edges=edges, arclet=arclet)
    # two_curve_map: equal curvatures (the wrap region reached at 0.5 eta_true), unequal curvatures, and an arclet grid past
    # the Doppler range, where NumPy's fancy index raises IndexError
    maps = [("eq_lo", 0.5, 0.5, edges, edges), ("eq", 1.0, 1.0, edges, arclet), ("ne", 0.8, 1.3, edges, arclet),
            ("eq_hi", 2.0, 2.0, edges, edges)]
    for tag, f1, f2, e1, e2 in maps:
        red, er1, er2 = thth.two_curve_map(CS, tau, fd, f1 * eta_true * u.s**3, e1 * u.mHz, f2 * eta_true * u.s**3, e2 * u.mHz)
        out[f"map_{tag}"], out[f"er1_{tag}"], out[f"er2_{tag}"] = np.asarray(red), V(er1), V(er2)
        out[f"fac_{tag}"] = np.array([f1, f2])
    wide = np.linspace(-2.2 * fdm, 2.2 * fdm, 48)
    try:
        thth.two_curve_map(CS, tau, fd, 0.3 * eta_true * u.s**3, wide * u.mHz, 0.3 * eta_true * u.s**3, wide * u.mHz)
        out["wide_raises"] = np.array(False)
    except IndexError:
        out["wide_raises"] = np.array(True)
    out["wide"] = wide
    # singularvalue_calc at 8 curvatures, centre cut 0 and > 0, and one cut wider than every column
    etas = np.geomspace(0.5, 2.0, 8) * eta_true
    out["sv_etas"] = etas
    for tag, cut in (("cut0", 0.0), ("cut1", 0.1 * fdm), ("cutall", 10 * fdm)):
        out[f"sv_{tag}"] = np.array([thth.singularvalue_calc(CS, tau, fd, e * u.s**3, edges * u.mHz, e * u.s**3,
                                                             arclet * u.mHz, cut * u.mHz) for e in etas])
        out[f"cutval_{tag}"] = np.array(cut)
    return out


def tutorial():
    d = np.load("/root/reference/scintools/examples/data/ththsims/Sample_Data.npz")
    dspec = np.abs(d["Espec"]) ** 2
    freq, tme = d["f_MHz"], d["t_s"]

    def dyn_obj():
        b = BasicDyn(name="Sample Data", header=["Sample Data"], times=tme, freqs=freq, dyn=dspec,
                     nsub=tme.shape[0], nchan=freq.shape[0], dt=(tme[1] - tme[0]), df=(freq[1] - freq[0]))
        return Dynspec(dyn=b, process=False, verbose=False)
    dyn = dyn_obj()
    dyn.prep_thetatheta(verbose=False, cwf=64, edges_lim=.3, eta_min=30 * u.s**3, eta_max=50 * u.s**3,
                        fitting_proc='thin', arclet_lim=.15, center_cut=.02)
    t0 = time.perf_counter()
    etas0, eigs0, popt0 = dyn.thetatheta_single(cf=0, ct=0, plot=False, arrays=True)
    t1 = time.perf_counter()
    dyn.fit_thetatheta(verbose=False)
    t2 = time.perf_counter()
    out = dict(edges=V(dyn.edges), arclet_lim=V(dyn.arclet_lim), center_cut=V(dyn.center_cut), neta=dyn.neta,
               eta_min=V(dyn.eta_min), eta_max=V(dyn.eta_max), single_etas=V(etas0), single_eigs=np.asarray(eigs0),
               single_popt=np.array(popt0), eta_evo=V(dyn.eta_evo), eta_evo_err=V(dyn.eta_evo_err), f0s=V(dyn.f0s),
               ththeta=V(dyn.ththeta), ththetaerr=V(dyn.ththetaerr))
    out = {f"tut_{k}": v for k, v in out.items()}
    # the defaults of arclet_lim (edges_lim) and center_cut (0)
    dd = dyn_obj()
    dd.prep_thetatheta(verbose=False, cwf=64, edges_lim=.3, eta_min=30 * u.s**3, eta_max=50 * u.s**3, fitting_proc='thin')
    out.update(def_edges=V(dd.edges), def_arclet_lim=V(dd.arclet_lim), def_center_cut=V(dd.center_cut), def_neta=dd.neta)
    return out, [t1 - t0, t2 - t1]


if __name__ == "__main__":
    arrs = small_case()
    tut, secs = tutorial()
    arrs.update(tut)
    path = os.path.join(HERE, "thin.npz")
    np.savez_compressed(path, **arrs)
    print(f"thin.npz: {os.path.getsize(path) / 1024:.0f} KiB, {len(arrs)} arrays")
    with open(os.path.join(HERE, "thin_timing.json"), "w") as fh:
        json.dump({"what": "reference thetatheta_single and fit_thetatheta, fitting_proc='thin', tutorial recipe "
                           "(cwf=64, edges_lim=.3, eta 30..50, arclet_lim=.15, center_cut=.02), with the refshim stand-ins",
                   "thetatheta_single_s": round(secs[0], 3), "fit_thetatheta_s": round(secs[1], 3),
                   "host_cores": os.cpu_count()}, fh, indent=1)
        fh.write("\n")
    print("reference seconds:", secs)
