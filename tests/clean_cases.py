"""Seeded inputs of the cleaning tests (tests/test_clean_cpu.py, test_clean_emu_cpu.py, test_gpu_clean.py) and of
tests/golden/make_golden_clean.py.  Nothing is stored but the reference's outputs: the inputs are regenerated from these seeds."""
import types

import numpy as np

NF, NT = 48, 40
ATTRS = ("dyn", "freqs", "times", "nchan", "nsub", "bw", "df", "freq", "dt", "tobs", "mjd")


def intensity(nf=NF, nt=NT, seed=5):
    """Positive 'intensity x bandpass x gain': a smooth bandpass times a slow gain times a scintillation pattern with two
    strong separable components, so that the singular values fall off by more than a factor 1.5 per mode."""
    rng = np.random.default_rng(seed)
    f, t = np.linspace(-1, 1, nf)[:, None], np.linspace(0, 1, nt)[None, :]
    bandpass = 1.0 + 0.4 * np.cos(1.3 * f) - 0.2 * f
    gain = 1.0 + 0.3 * np.sin(2.1 * np.pi * t)
    scint = 1.0 + 0.45 * np.sin(5.0 * f + 1.0) * np.cos(7.0 * t) + 0.2 * np.cos(11.0 * f) * np.sin(13.0 * t + 0.5) \
        + 0.08 * np.sin(17.0 * f + 2.0) * np.cos(3.0 * t + 1.0)
    return bandpass * gain * scint * (1.0 + 0.004 * rng.standard_normal((nf, nt)))


def observation(kind="channels"):
    """The 48 x 40 observation of the golden cases as an object with the reference's attribute set: two zeroed edge channels,
    one zeroed leading sub-integration, three interior flagged lines (two adjacent: channels or sub-integrations), four spikes."""
    dyn = intensity()
    dyn[0, :] = 0.0
    dyn[-1, :] = 0.0
    dyn[:, 0] = 0.0
    if kind == "channels":
        dyn[[10, 25, 26], :] = 0.0
    else:
        dyn[:, [8, 20, 21]] = 0.0
    for (i, j), v in zip(((5, 7), (17, 30), (33, 12), (40, 35)), (60.0, 35.0, 90.0, 45.0)):
        dyn[i, j] = v
    o = types.SimpleNamespace()
    o.name, o.header = "clean_case", ["clean_case"]
    o.dyn = dyn
    o.df, o.dt = 0.5, 8.0
    o.freqs = 1300.0 + o.df * np.arange(NF)
    o.times = o.dt * np.arange(NT, dtype=float)
    o.nchan, o.nsub = NF, NT
    o.bw = round(NF * o.df, 3)
    o.freq = round(float(np.mean(o.freqs)), 3)
    o.tobs = round(NT * o.dt, 3)
    o.mjd = 59000.25
    return o


# the golden cases: name -> (observation kind, [(method, kwargs), ...]); the attributes are stored after every step
CASES = {
    "chan_linear": ("channels", [("trim_edges", {}), ("refill", dict(method="linear"))]),
    "sub_linear": ("subints", [("trim_edges", {}), ("refill", dict(method="linear"))]),
    "chan_biharmonic": ("channels", [("trim_edges", {}), ("refill", {})]),
    "chan_zap": ("channels", [("trim_edges", {}), ("zap", {})]),
    "sub_zap3": ("subints", [("trim_edges", {}), ("zap", dict(sigma=3))]),
    "chan_median": ("channels", [("refill", dict(method="median", kernel_size=3))]),
    "sub_median5": ("subints", [("refill", dict(method="median"))]),
    "sub_meanfill": ("subints", [("refill", dict(method="cubic", linear=False))]),
    "chain": ("channels", [("trim_edges", {}), ("zap", {}), ("refill", dict(method="median", kernel_size=(3, 5))),
                           ("correct_dyn", {})]),
    "chain_sub_n2": ("subints", [("trim_edges", {}), ("zap", {}), ("refill", dict(method="median", kernel_size=(3, 5))),
                                 ("correct_dyn", dict(nmodes=2))]),
    "crop": ("channels", [("trim_edges", {}), ("crop_dyn", dict(fmin=1305.2, fmax=1318.0, tmin=0.5, tmax=4.0))]),
    "nosvd": ("channels", [("trim_edges", {}), ("correct_dyn", dict(svd=False))]),
    "nosvd_smooth": ("subints", [("trim_edges", {}), ("correct_dyn", dict(svd=False, nsmooth=5))]),
    "nosvd_time": ("channels", [("trim_edges", {}), ("correct_dyn", dict(svd=False, frequency=False))]),
    "nosvd_freq": ("channels", [("trim_edges", {}), ("correct_dyn", dict(svd=False, time=False))]),
}
SVD_CASES = {"chain": 1, "chain_sub_n2": 2}               # case -> nmodes of its correct_dyn step


def svd_matrix(nf, nt, nmodes, seed, nans=False):
    """A positive nf x nt array whose singular values fall by a factor 2 from mode to mode down to mode nmodes + 1 (relative gap
    1 - (s[k+1]/s[k])**2 = 0.75 at every k <= nmodes, s[nmodes]/s[0] >= 1/8) over a noise floor 30 times lower still."""
    rng = np.random.default_rng(seed)
    r = min(nf, nt, nmodes + 1)
    u = np.linalg.qr(np.column_stack([np.ones(nf) + 0.2 * rng.random(nf)] + [rng.standard_normal(nf) for _ in range(r - 1)]))[0]
    v = np.linalg.qr(np.column_stack([np.ones(nt) + 0.2 * rng.random(nt)] + [rng.standard_normal(nt) for _ in range(r - 1)]))[0]
    s = np.sqrt(nf * nt) * 0.5 ** np.arange(r)
    a = (u * s) @ v.T
    a = a * np.sign(a.sum())
    if min(nf, nt) > r:
        a = a + (s[-1] / 60.0) / (np.sqrt(nf) + np.sqrt(nt)) * rng.standard_normal((nf, nt))
    if nans:
        a[rng.random(a.shape) < 0.02] = np.nan
        a[rng.random(a.shape) < 0.02] = 0.0
    return a


def complex_matrix(nf=40, nt=24, seed=9):
    """40 x 24 complex, singular values 1, 1/2, 1/4 times 30 over a small floor."""
    rng = np.random.default_rng(seed)
    u = np.linalg.qr(rng.standard_normal((nf, 3)) + 1j * rng.standard_normal((nf, 3)))[0]
    v = np.linalg.qr(rng.standard_normal((nt, 3)) + 1j * rng.standard_normal((nt, 3)))[0]
    s = 30.0 * 0.5 ** np.arange(3)
    return (u * s) @ v.conj().T + 0.01 * (rng.standard_normal((nf, nt)) + 1j * rng.standard_normal((nf, nt)))


def zap_inputs():
    """name -> array of the zap kernel shapes: counts 1, 2, 255, 256, 257 and 1031 x 517, and the special values."""
    rng = np.random.default_rng(11)
    out = {}
    for n in (1, 2, 255, 256, 257):
        x = rng.standard_normal((1, n))
        if n > 2:
            x[0, n // 3] = 40.0
        out[f"n{n}"] = x
    big = rng.standard_normal((1031, 517))
    big[rng.random(big.shape) < 1e-3] = 25.0
    out["big"] = big
    out["big_even"] = big[:1030].copy()
    out["all_equal"] = np.full((9, 7), 3.25)
    nan30 = rng.standard_normal((40, 33))
    nan30[rng.random(nan30.shape) < 0.3] = np.nan
    nan30[3, 3] = -30.0
    out["nan30"] = nan30
    inf = rng.standard_normal((20, 21))
    inf[2, 2], inf[5, 6], inf[7, 7] = np.inf, -np.inf, np.inf
    out["inf"] = inf
    dup = np.repeat(np.array([1.0, 2.0, 2.0, 2.0, 2.0, 2.0, 3.0, 500.0]), 16).reshape(8, 16)
    out["dup_straddle"] = dup
    dup_even = np.concatenate([np.full(50, 1.0), np.full(50, 2.0), [9.0, -9.0]]).reshape(6, 17)
    out["dup_even_split"] = dup_even                                    # the middle pair is (1, 2): median 1.5
    sz = rng.standard_normal((10, 10))
    sz[sz > 0.3] = 0.0
    sz[sz < -0.3] = -0.0
    sz[0, 0] = -7.0
    out["signed_zero"] = sz
    out["mdev_zero"] = np.concatenate([np.full(60, 2.0), [2.5, 1.0, np.nan]]).reshape(7, 9)   # x/0 -> inf zapped, 0/0 not
    out["neg"] = -np.abs(rng.standard_normal((13, 11))) - 1.0
    out["all_nan"] = np.full((3, 4), np.nan)
    return out


def holes(nf, nt, seed, frac=0.12):
    """Unit-scale positive data with NaN pixels scattered, NaN runs and a NaN in every corner."""
    rng = np.random.default_rng(seed)
    x = 0.5 + rng.random((nf, nt))
    x[rng.random(x.shape) < frac] = np.nan
    x[nf // 2, :] = np.nan
    x[0, 0] = x[0, -1] = x[-1, 0] = x[-1, -1] = np.nan
    return x


def gaps(nf, nt, axis, seed):
    """Unit-scale data with whole-line gaps of width 1, 2 and 9 along ``axis`` (where the axis is long enough) and, for odd seeds,
    a gap touching the first or the last line."""
    rng = np.random.default_rng(seed)
    x = 0.5 + rng.random((nf, nt))
    n = x.shape[axis]
    lines = []
    if n >= 40:
        lines = [3, 7, 8] + list(range(20, 29))
    elif n >= 5:
        lines = [2]
    if seed % 2:
        lines += [0] if seed % 4 == 1 else [n - 1, n - 2]
    idx = [slice(None)] * 2
    idx[axis] = sorted(set(lines))
    x[tuple(idx)] = np.nan
    return x
