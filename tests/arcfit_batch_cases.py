"""Seeded stacks of small secondary spectra (dB) for the batched arc fit -- scint_arc_profile_batch, scint_arc_peak_fit,
arcfit.fit_arc_stack_device, Dynspec.fit_arc_cut; the checks are tests/arcfit_batch_checks.py.  A case is a stack [B, R, nc] of
arcs plus noise on shared axes, the delay rows [row0, row0 + nr), the normalising curvature and the grid x[nx]:

  one       B 1,  nc 8,    nr 1,  nx 2,   cutmid 0   the smallest of everything; one row, one selected column in it or few
  r31       B 2,  nc 64,   nr 31, nx 254, cutmid 3   one partial of 32 rows not full; x shorter than a workgroup
  r32       B 2,  nc 64,   nr 32, nx 256, cutmid 3   exactly one partial, exactly one workgroup
  r33       B 2,  nc 64,   nr 33, nx 514, cutmid 0   a second partial of one row; a third workgroup of two columns
  b37       B 37, nc 130,  nr 65, nx 258, cutmid 4   three partials, a B and an nc that are multiples of nothing, NaN and -inf pixels
  norows    B 2,  nc 64,   nr 33, nx 256, cutmid 0   a curvature so large that the first rows select no column (c1 < c0): the
                                                     Doppler axis is offset by half a bin, so no bin sits at zero
  empty     B 2,  nc 64,   nr 31, nx 258, cutmid 3   a curvature so small that the outer x columns are empty in every row
                                                     (empty_out = 1, 0.0 in avg_out)
  long      B 2,  nc 2050, nr 2,  nx 256, cutmid 3   one row selects 2050 columns, beyond the 2048 a workgroup stages in LDS: the
                                                     global-memory route at its real limit; the other row selects fewer and is staged

The peak-fit profiles (`peak_profiles`) are made on the host alone: a bump in power against curvature plus noise, and synthetic
ones that force each status and the flat-top tie."""
import numpy as np

#            B   R   nc   row0 nr  nx   cutmid
SHAPES = {
    "one": (1, 8, 8, 3, 1, 2, 0),
    "r31": (2, 40, 64, 3, 31, 254, 3),
    "r32": (2, 40, 64, 3, 32, 256, 3),
    "r33": (2, 40, 64, 3, 33, 514, 0),
    "b37": (37, 70, 130, 3, 65, 258, 4),
    "norows": (2, 40, 64, 1, 33, 256, 0),
    "empty": (2, 40, 64, 3, 31, 258, 3),
    "long": (2, 4, 2050, 1, 2, 256, 3),
}
CASES = tuple(SHAPES)
DFD, DY = 0.25, 0.125
_cache = {}


class Case:
    pass


def case(name):
    """The case (built once, then shared: do not write into it)."""
    if name in _cache:
        return _cache[name]
    B, R, nc, row0, nr, nx, cutmid = SHAPES[name]
    rng = np.random.default_rng(4000 + CASES.index(name))
    c = Case()
    c.name, c.B, c.R, c.nc, c.row0, c.nr, c.nx, c.cutmid = name, B, R, nc, row0, nr, nx, cutmid
    off = 0.5 if name == "norows" else 0.0
    c.fdop = (np.arange(nc) - nc // 2 + off) * DFD
    c.yaxis = np.arange(R) * DY
    ylast = c.yaxis[row0 + nr - 1]
    fmax = np.max(np.abs(c.fdop))
    c.eta = ylast / fmax**2                                       # the last row just selects every column
    if name == "norows":
        c.eta = c.yaxis[row0 + 2] / (0.5 * DFD)**2                # rows row0 and row0 + 1 select nothing, the last one 8 bins
    if name == "empty":
        c.eta = 0.25 * c.yaxis[row0] / fmax**2                    # max |fdop| / scale <= 0.5 from the first row on: |x| > 0.5 is empty
    if name == "long":
        c.eta = c.yaxis[row0 + 1] / fmax**2                       # row 1 selects all 2050 columns, row 0 about 0.71 of them
    c.maxnormfac = 1.0
    c.cut_lo = int(nc / 2 - np.floor(cutmid / 2))
    c.cut_hi = int(nc / 2 + np.floor(cutmid / 2))
    c.noise_lo = c.cut_lo
    c.noise_hi = int(nc / 2 + np.ceil(cutmid / 2))
    c.x = np.linspace(-1.0, 1.0, nx)
    # arcs: power along tdel = eta_b fdop^2, eta_b between 6 and 20 times the normalising curvature (|x| = 0.22 to 0.41 of the
    # normalised axis, where every case has data), over a noise floor averaged as 16 looks are
    f, y = np.meshgrid(c.fdop, c.yaxis)
    stack = np.empty((B, R, nc))
    for b in range(B):
        eta_b = c.eta * rng.uniform(6.0, 20.0)
        width = 1.5 * DY + 0.05 * y
        power = 30.0 * np.exp(-0.5 * ((y - eta_b * f**2) / width)**2) / (1.0 + y) + rng.gamma(16.0, 1.0 / 16.0, (R, nc))
        stack[b] = 10 * np.log10(power)
    if name == "b37":
        holes = rng.integers(0, stack.size, 200)
        stack.reshape(-1)[holes[:100]] = np.nan
        stack.reshape(-1)[holes[100:]] = -np.inf
        stack[5, :R // 2] = np.nan                                # a problem whose inner half is gone: nothing finite in its profile
    c.stack = np.ascontiguousarray(stack)
    _cache[name] = c
    return c


# ---- peak-fit profiles, host only ---------------------------------------------------------------------------------------------------
PEAK_NX = 400                      # x = linspace(-1, 1, PEAK_NX): 200 curvatures per folded profile
PEAK_ETAMIN, PEAK_ETAMAX = 1.0, 2000.0


def peak_x():
    return np.linspace(-1.0, 1.0, PEAK_NX)


def _eta_of_x():
    x = peak_x()
    return PEAK_ETAMIN / x[PEAK_NX // 2:]**2


def bump_profiles(count=24, seed=7):
    """avg [count, PEAK_NX] (both sides, different noise on each) of a parabola-topped bump in log eta, 8 dB over a sloping floor,
    noise of 0.15 dB: what a normalised, scrunched arc looks like."""
    rng = np.random.default_rng(seed)
    eta = _eta_of_x()
    out = np.empty((count, PEAK_NX))
    for k in range(count):
        centre = rng.uniform(np.log(8.0), np.log(300.0))
        w = rng.uniform(0.25, 0.6)
        base = -0.4 * np.log(eta) + 8.0 * np.exp(-0.5 * ((np.log(eta) - centre) / w)**2)
        out[k, PEAK_NX // 2:] = base + 0.15 * rng.standard_normal(eta.size)
        out[k, :PEAK_NX // 2] = np.flip(base + 0.15 * rng.standard_normal(eta.size))
    return out


def _from_flipped(spec_flipped):
    """avg [PEAK_NX] whose folded, flipped profile is `spec_flipped` [PEAK_NX / 2] (index 0 = the smallest curvature kept)."""
    pos = np.flip(np.asarray(spec_flipped, dtype=float))
    return np.concatenate((np.flip(pos), pos))


def synthetic_profiles():
    """{name: (avg [PEAK_NX], keywords, expected status)}: one profile for every status and the flat-top tie.  Every curvature of
    the grid is below PEAK_ETAMAX except the first few x, so `kept` is the same for all but `short`."""
    half = PEAK_NX // 2
    j = np.arange(half, dtype=float)
    out = {}
    hill = -0.002 * (j - 90.0)**2
    out["ok"] = (_from_flipped(hill + 0.01 * np.sin(1.7 * j)), {}, 0)
    short = np.full(half, np.nan)
    short[10:14] = 1.0                                             # 4 finite points, nsmooth = 5
    out["short"] = (_from_flipped(short), {}, 1)
    out["norange"] = (_from_flipped(hill), {"constraint": (5000.0, 6000.0)}, 2)
    edge = -0.07 * j                                               # the maximum is the first point: the window would start at -1
    out["window"] = (_from_flipped(edge), {}, 3)
    eta_f = np.flip(_eta_of_x())                                   # the curvature of flipped index j (the largest few are not kept)
    decay = 5.0 * np.exp(-j / 40.0)                                # convex and falling: with the peak forced to j = 50 by the constraint
    out["forward"] = (_from_flipped(decay), {"constraint": (eta_f[49], eta_f[52]), "low_power_diff": 0.0}, 4)   # and no low side
    out["nonfinite"] = (_from_flipped(1e200 * hill), {"low_power_diff": -2e198, "high_power_diff": -1e198}, 5)
    flat = np.minimum(hill, hill[80])                              # a flat top from 80 to 100
    out["flat"] = (_from_flipped(flat), {}, 0)
    return out
