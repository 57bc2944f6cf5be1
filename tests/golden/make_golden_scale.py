#!/usr/bin/env python
"""Generate tests/golden/scale.npz and tests/golden/scale_tolerances.json by running the UNMODIFIED reference's
Dynspec.scale_dyn(scale='velocity' / 'trapezoid') and calc_sspec(velocity=True / trap=True) (scintools/dynspec.py:3872-4128,
3584-3748) with the stand-ins of tests/golden/refshim, as the other make_golden_* scripts do.

    SCINTOOLS_REFERENCE=<checkout of the reference> python tests/golden/make_golden_scale.py [--timing]

Two process-local stand-ins, nothing of the reference is edited:

* scintools.scint_utils.get_ssb_delay / get_earth_velocity (astropy's solar-system ephemeris) are replaced by functions that
  return the seeded arrays of tests/scale_cases.ephemeris; scale_dyn imports them when it is called, so replacing the module
  attributes is enough.  The arrays are stored, and the tests feed the port the same ones.
* As shipped, scale_dyn(scale='trapezoid') raises "ValueError: setting an array element with a sequence. The requested array has
  an inhomogeneous shape after 1 dimensions." at dynspec.py:4127 for every row that gets trailing zeros:
  list(np.zeros(np.shape(indzeros))) is a list of 1-element arrays, because np.argwhere returns [k, 1].  The scintools.dynspec
  module is given a global `list` that turns 1-element arrays into floats and is the builtin otherwise, so that line 4126 builds the
  k zeros it means to.

With a parameter dictionary without PB the reference raises KeyError('PB') in get_true_anomaly (scint_utils.py:522); the text is
stored.  The tolerance of the device row spline is measured here (see `tolerance`).  --timing: the reference's CPU time of
scale_dyn('velocity') at 1024^2 and 4096^2 with the seeded ephemerides, into tests/golden/scale_timing.json."""
import builtins
import json
import os
import sys
import tempfile
import time
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "refshim"))
sys.path.insert(0, os.environ["SCINTOOLS_REFERENCE"])
sys.path.insert(0, os.path.join(REPO, "tests"))

import matplotlib  # noqa: E402
matplotlib.use("Agg")
import numpy as np  # noqa: E402

import scintools.dynspec as ref_dynspec  # noqa: E402
import scintools.scint_models as ref_models  # noqa: E402
import scintools.scint_utils as ref_utils  # noqa: E402
from scintools.dynspec import BasicDyn, Dynspec  # noqa: E402
import scale_cases as sc  # noqa: E402
import scale_oracle as so  # noqa: E402

warnings.simplefilter("ignore")


def _list(x=()):
    return [float(v[0]) if isinstance(v, np.ndarray) and v.shape == (1,) else v for v in builtins.list(x)]


ref_dynspec.list = _list


def reference(o):
    b = BasicDyn(np.array(o.dyn), name=o.name, header=o.header, times=np.array(o.times), freqs=np.array(o.freqs), nchan=o.nchan,
                 nsub=o.nsub, bw=o.bw, df=o.df, freq=o.freq, tobs=o.tobs, dt=o.dt, mjd=o.mjd)
    return Dynspec(dyn=b, process=False, verbose=False)


def seed_ephemeris(nt):
    ssb, vra, vdec = sc.ephemeris(nt)
    ref_utils.get_ssb_delay = lambda mjds, raj, decj, message=True: np.array(ssb)
    ref_utils.get_earth_velocity = lambda mjds, raj, decj, radial=False: (np.array(vra), np.array(vdec))
    return ssb, vra, vdec


def quiet(fn, *a, **kw):
    out, sys.stdout = sys.stdout, open(os.devnull, "w")
    try:
        return fn(*a, **kw)
    finally:
        sys.stdout.close()
        sys.stdout = out


def velocity_goldens(arrs):
    o = sc.observation()
    ssb, vra, vdec = seed_ephemeris(o.nsub)
    arrs["eph_ssb"], arrs["eph_vra"], arrs["eph_vdec"] = ssb, vra, vdec
    worst = 0.0
    for name, (pars, kw, lam) in sc.VELOCITY.items():
        d = reference(o)
        if lam:
            d.scale_dyn(scale='lambda')
            arrs[f"v_{name}_lamdyn"] = np.array(d.lamdyn)
        p = dict(pars)
        quiet(d.scale_dyn, scale='velocity', pars=p, **dict(kw))
        arrs[f"v_{name}_vdyn"] = d.vdyn
        arrs[f"v_{name}_veff_ra"], arrs[f"v_{name}_veff_dec"] = np.array(d.veff_ra), np.array(d.veff_dec)
        # the host functions on their own, with the barycentred MJDs scale_dyn forms (dynspec.py:3982-3987)
        mjd = np.asarray(o.mjd, dtype=np.float128) + np.asarray(o.times, dtype=np.float128) / 86400
        mjd += np.divide(ssb, 86400)
        ta = quiet(ref_utils.get_true_anomaly, mjd, dict(p))
        arrs[f"v_{name}_true_anomaly"] = np.array(ta)
        eva = ref_models.effective_velocity_annual(dict(p), ta, np.array(vra), np.array(vdec), mjd=mjd)
        for tag, v in zip(("eva_ra", "eva_dec", "vp_ra", "vp_dec"), eva):
            arrs[f"v_{name}_{tag}"] = np.array(v)
        if lam:
            arrs[f"v_{name}_vlamdyn"] = d.vlamdyn
        if name == "ecc":
            d.calc_sspec(velocity=True)
            arrs["v_ecc_vsspec"], arrs["v_ecc_fdop"], arrs["v_ecc_tdel"] = d.vsspec, d.fdop, d.tdel
            d.calc_sspec(velocity=True, lamsteps=True)
            arrs["v_ecc_vlamsspec"], arrs["v_ecc_beta"] = d.vlamsspec, d.beta
        # the tolerance: the float64 moment algorithm of the kernel against the reference's vdyn
        veff = np.sqrt(veff2(d, p, kw))
        vc_orig, vc_new = so.velocity_grid(veff)
        assert np.array_equal(so.spline_rows(o.dyn, vc_orig, vc_new), d.vdyn), name
        mine = so.moments_rows(o.dyn, np.asarray(vc_orig, dtype=float), np.asarray(vc_new, dtype=float))
        e = np.abs(mine - d.vdyn).max() / np.abs(d.vdyn).max()
        print(f"{name}: veff {float(veff.min()):.2f} .. {float(veff.max()):.2f} km/s, moment algorithm vs reference {e:.3e}")
        worst = max(worst, e)
    # the orbit keyword, the parfile and the refused dictionary
    d = reference(o)
    quiet(d.scale_dyn, scale='orbit', pars=dict(sc.BINARY))
    assert np.array_equal(d.vdyn, arrs["v_ecc_vdyn"])
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "test.par")
        with open(path, "w") as fh:
            fh.write(sc.PARFILE)
        arrs["par_json"] = np.array(json.dumps(ref_utils.read_par(path), sort_keys=True))
        d = reference(o)
        quiet(d.scale_dyn, scale='velocity', parfile=path, **sc.PARFILE_KW)
        arrs["v_parfile_vdyn"] = d.vdyn
    try:
        quiet(reference(o).scale_dyn, scale='velocity', pars=dict(sc.NO_PB))
        raise SystemExit("the reference ran without PB")
    except KeyError as err:
        arrs["no_pb_error"] = np.array(f"{type(err).__name__}: {err}")
    return worst


def veff2(d, p, kw):
    """veff**2 from what the reference left behind: veff_ra / veff_dec after the ISM terms (dynspec.py:4018-4053)."""
    zeta = p.get('zeta', kw.get('zeta'))
    if zeta is None:
        return d.veff_ra**2 + d.veff_dec**2
    zeta = zeta * (np.pi / 180)                              # `zeta *= np.pi / 180` on a float rebinds the local name only
    vz = p.get('vism_zeta', kw.get('vism_zeta'))
    return (d.veff_ra * np.sin(zeta) + d.veff_dec * np.cos(zeta) - (0 if vz is None else vz))**2


def trapezoid_goldens(arrs):
    for name, (okw, kw) in sc.TRAPEZOID.items():
        o = sc.observation(**okw)
        d = reference(o)
        d.scale_dyn(scale='trapezoid', **kw)
        arrs[f"t_{name}_trapdyn"] = d.trapdyn
        assert np.array_equal(so.trapezoid(o.dyn, o.freqs, o.times, **kw), d.trapdyn), name
        print(f"{name}: keeps {so.trapezoid_keep(o.freqs, o.times).tolist()}")
    d = reference(sc.observation())
    d.calc_sspec(trap=True)
    arrs["t_default_trapsspec"] = d.trapsspec


def timing():
    out = {}
    for n in (1024, 4096):
        o = sc.observation(nf=n, nt=n)
        seed_ephemeris(n)
        d = reference(o)
        t0 = time.perf_counter()
        quiet(d.scale_dyn, scale='velocity', pars=dict(sc.BINARY))
        out[f"{n}x{n}"] = {"scale_dyn_velocity_s": time.perf_counter() - t0, "samples": 1}
        print(n, out[f"{n}x{n}"])
    with open(os.path.join(HERE, "scale_timing.json"), "w") as fh:
        json.dump({"tool": "make_golden_scale --timing", "what": "the reference's Dynspec.scale_dyn(scale='velocity') on the host, "
                   "seeded ephemerides, one run per size", "results": out}, fh, indent=1)


if __name__ == "__main__":
    if "--timing" in sys.argv:
        timing()
        raise SystemExit(0)
    arrs = {}
    worst = velocity_goldens(arrs)
    trapezoid_goldens(arrs)
    path = os.path.join(HERE, "scale.npz")
    np.savez_compressed(path, **arrs)
    print(f"scale.npz: {os.path.getsize(path) / 1024:.0f} KiB, {len(arrs)} arrays")
    with open(os.path.join(HERE, "scale_tolerances.json"), "w") as fh:
        json.dump({"what": "worst |float64 moment algorithm - reference vdyn| / max |vdyn| over the velocity cases "
                   "(tests/scale_oracle.moments_rows); the GPU bound is max(10 x this, 1e-12)",
                   "moment_algorithm_vs_reference": worst}, fh, indent=1)
    print("tolerance", worst)
