"""Inputs of the no-fit scintillation-scale tests (tests/test_scintpar_cpu.py, tests/test_gpu_scintpar.py) and of
tests/golden/make_golden_scintpar.py -- TEST INFRASTRUCTURE.

Observations come from the seeded screen simulator of oracle/sim_oracle.py; the generator stores them in
tests/golden/scintpar.npz (as float32, which is what the simulator produces), the tests read them back from there.  The shapes
are the smallest at which each kernel can still go wrong:

  even    64 x 96     a simulation of its own
  big     192 x 256   moments and the ACF's maximum span more than one workgroup
  odd     75 x 101    a crop of `big`: odd lengths (centre indices, odd ACF halves)
  cut     130 x 203   a crop of `big` for cut_dyn(tcuts=3, fcuts=2): 43 x 50 segments, remainders dropped, ACF lengths that are
                      no powers of two, spectrum lengths padded to powers of two
  small   24 x 40     a crop of `even` whose 'sspec' ACF (64 x 128) is small enough to store
  holes   = even with a NaN block and a block of zeros poked in AFTER the ACF was taken (the moments skip both)

and two synthetic ACFs for the row maxima: `tie` (exact ties inside a wavefront, across wavefronts and across a thread's
strides) and `edge` (a selected row whose maximum sits in column 1)."""
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SIMS = {"even": dict(ns=96, nf=64, seed=64), "big": dict(ns=256, nf=192, seed=192)}
CROPS = {"odd": ("big", 7, 75, 11, 101), "cut": ("big", 0, 130, 0, 203), "small": ("even", 3, 24, 5, 40)}
OBS = ("even", "big", "odd", "small")                  # get_scint_params + get_acf_tilt run on these
CUTS = {"cut": (3, 2), "small": (0, 0)}                # case -> (tcuts, fcuts)
SSPEC_ACF = ("small",)                                 # calc_acf(method='sspec') stored for these
NOFIT_ATTRS = ("tau", "dnu", "amp", "wn", "dnuerr", "tauerr", "amperr", "wnerr", "tscat", "nscint", "dnu_est", "dnu_esterr",
               "tscat_est", "modulation_index")
GRID_ATTRS = ("tau", "dnu")                            # multiples of dt / df: equal, not close
TILT_ATTRS = ("acf_tilt", "acf_tilt_err", "fse_tilt")
VARIANTS = {"default": {}, "full": dict(full_frame=True), "nscale1": dict(nscale=1)}
AXIS_KEYS = ("freqs", "times", "df", "dt", "bw", "tobs", "freq")


def simulate(name):
    """The seeded simulation `name` with a float64 copy of its (float32-valued) dynamic spectrum."""
    from oracle import sim_oracle
    s = sim_oracle.Simulation(mb2=2, ar=1, dlam=0.25, dt=30, freq=1400, **SIMS[name])
    return observation(np.asarray(s.dyn, dtype=np.float64), s.freqs, s.times, s.df, s.dt, s.freq, name)


def observation(dyn, freqs, times, df, dt, freq, name="obs"):
    """An object with the attribute set Dynspec.load_dyn_obj copies; bw and tobs as the reference's loaders form them."""
    o = types.SimpleNamespace()
    o.name, o.header, o.mjd = name, [name], 60000.0
    o.dyn, o.freqs, o.times = np.array(dyn, dtype=np.float64), np.array(freqs, dtype=float), np.array(times, dtype=float)
    o.nchan, o.nsub = o.dyn.shape
    o.df, o.dt, o.freq = float(df), float(dt), float(freq)
    o.bw = float(np.ptp(o.freqs) + o.df)
    o.tobs = float(np.ptp(o.times) + o.dt)
    return o


def crop(parent, r0, nr, c0, nc, name):
    return observation(parent.dyn[r0:r0 + nr, c0:c0 + nc], parent.freqs[r0:r0 + nr], parent.times[c0:c0 + nc] - parent.times[c0],
                       parent.df, parent.dt, float(np.mean(parent.freqs[r0:r0 + nr])), name)


def build_all():
    """Every observation, generated from the seeds (the generator script; the tests use `from_golden`)."""
    obs = {name: simulate(name) for name in SIMS}
    for name, (parent, r0, nr, c0, nc) in CROPS.items():
        obs[name] = crop(obs[parent], r0, nr, c0, nc, name)
    return obs


def store(obs, arrs):
    for name, o in obs.items():
        assert np.array_equal(o.dyn.astype(np.float32).astype(np.float64), o.dyn), name
        if name in SIMS:
            arrs[f"in_{name}_dyn"] = o.dyn.astype(np.float32)
        for k in AXIS_KEYS:
            arrs[f"in_{name}_{k}"] = np.asarray(getattr(o, k))


def from_golden(g, name):
    """Observation `name` from tests/golden/scintpar.npz (a crop is cut from its parent's stored array)."""
    if name in SIMS:
        dyn = g[f"in_{name}_dyn"].astype(np.float64)
    else:
        parent, r0, nr, c0, nc = CROPS[name]
        dyn = g[f"in_{parent}_dyn"].astype(np.float64)[r0:r0 + nr, c0:c0 + nc]
    o = types.SimpleNamespace(name=name, header=[name], mjd=60000.0, dyn=np.ascontiguousarray(dyn))
    for k in AXIS_KEYS:
        v = g[f"in_{name}_{k}"]
        setattr(o, k, v if v.ndim else float(v))
    o.nchan, o.nsub = o.dyn.shape
    return o


def poke_holes(dyn):
    """`dyn` with a NaN block, an inf pixel and a block of exact zeros: the pixels the moments must skip."""
    d = np.array(dyn, dtype=np.float64)
    d[5:9, 10:31] = np.nan
    d[20, 3] = np.inf
    d[40:44, 50:70] = 0.0
    return d


# ---- synthetic ACFs for the row maxima -----------------------------------------------------------------------------------
TIE_SHAPE = (16, 640)      # 640 columns: a thread of the 256-wide workgroup walks up to three of them


def _ridge(R, C, slope, width):
    """A smooth tilted ridge, 1 at the centre: row r peaks near column C/2 + slope (r - R/2)."""
    r = np.arange(R)[:, None] - R // 2
    c = np.arange(C)[None, :] - C // 2
    return np.exp(-0.5 * ((c - slope * r) / width) ** 2) * np.exp(-0.5 * (r / (0.35 * R)) ** 2)


def tie_acf():
    """Rows with an exact tie of the maximum: np.argmax takes the lowest column.  Row 6: neighbours (one wavefront); row 7: 40
    columns apart (two wavefronts of one stride); row 9: 256 apart (the same thread, two strides); row 10: 300 apart (another
    wavefront AND another stride, the later stride in the lower lane).  The first of the tied columns is where the ridge
    peaks anyway, so its 7-sample window is the ridge's and the parabola has a maximum."""
    R, C = TIE_SHAPE
    a = _ridge(R, C, 2.5, 9.0)
    a[:, 1::2] -= 1e-4                                    # (no accidental ties between a peak's neighbours)
    for row, gap in ((6, 1), (7, 40), (9, 256), (10, 300)):
        c0 = int(np.argmax(a[row]))
        a[row, c0 + gap] = a[row, c0]
        if gap > 1:                                       # a later copy must not look like a better peak to a wrong rule
            a[row, c0 + gap - 1] = a[row, c0 + gap + 1] = a[row, c0] * 0.5
    return a


def tie_rows():
    return np.array([6, 7, 9, 10])


def edge_acf():
    """`tie`-shaped ridge whose centre row's neighbour (row R/2 + 1, always selected by get_acf_tilt) has its maximum in
    column 1: no 7-sample window."""
    R, C = TIE_SHAPE
    a = _ridge(R, C, 2.5, 9.0)
    a[R // 2 + 1, 1] = 2.0
    return a


def synthetic_observation(R=TIE_SHAPE[0], C=TIE_SHAPE[1]):
    """An observation whose ACF has the synthetic fixtures' shape ([R / 2, C / 2] pixels); its dyn only feeds the moments."""
    rng = np.random.default_rng(7)
    nf, nt = R // 2, C // 2
    return observation(1.0 + 0.5 * rng.random((nf, nt)), 1400.0 + 0.5 * np.arange(nf), 30.0 * np.arange(nt), 0.5, 30.0, 1402.0,
                       "synthetic")
