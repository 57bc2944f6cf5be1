"""Seeded multi-station geometries for the VLBI phase retrieval (ththmod.VLBI_chunk_retrieval / vlbi_retrieval_batch), shared by
tests/golden/make_golden_vlbi.py, tests/test_vlbi_cpu.py, tests/test_vlbi_emu_cpu.py and tests/test_gpu_vlbi.py.

A chunk of nf x nt pixels (10 s time steps, 0.1 MHz channels, as tests/retrieval_cases.py) sees `nimg` images on ONE parabola
tau = eta theta^2: station a's field is E_a(f, t) = sum_k mu_k exp(i a slope theta_k) exp(2 pi i (theta_k t + tau_k (f - f0))),
i.e. station b's images carry an extra phase linear in theta against station a's.  The dynamic spectra are I_a = |E_a|^2 and the
visibilities V_ab = E_a conj(E_b), in the reference's order [I1, V12, ..., V1N, I2, V23, ..., IN]."""
import numpy as np

from retrieval_cases import geometry


def station_fields(nf, nt, n_dish, eta, th_lim, seed, nimg=12, slope=0.35):
    """[n_dish, nf, nt] complex fields: a bright image at theta = 0 and nimg - 1 fainter ones within |theta| < th_lim (mHz)."""
    rng = np.random.default_rng(seed)
    time = np.arange(nt) * 10.0
    freq = 0.1 * np.arange(nf)
    th = np.concatenate(([0.0], rng.uniform(-th_lim, th_lim, nimg - 1)))
    mu = np.concatenate(([1.0], 0.25 * (rng.standard_normal(nimg - 1) + 1j * rng.standard_normal(nimg - 1))))
    tau = eta * th ** 2
    phase = 2 * np.pi * (th[:, None, None] * 1e-3 * time[None, None, :] + tau[:, None, None] * freq[None, :, None])
    E = np.empty((n_dish, nf, nt), dtype=complex)
    for a in range(n_dish):
        E[a] = ((mu * np.exp(1j * a * slope * th))[:, None, None] * np.exp(1j * phase)).sum(0)
    return E


def spectra(E):
    """[I1, V12, ..., V1N, I2, V23, ..., IN] of the stations' fields."""
    out = []
    for a in range(E.shape[0]):
        out.append(np.abs(E[a]) ** 2)
        for b in range(a + 1, E.shape[0]):
            out.append(E[a] * np.conjugate(E[b]))
    return out


def case(nf, nt, npad, n_dish, nedge, factor, seed, span=0.45):
    """One chunk: dict(dlist, edges, time, freq, eta, E).  `factor` < 1: the crop of thth_redmap keeps every centre; > 1: it
    crops the theta grid (retrieval_cases.geometry)."""
    time, freq, tau, fd, edges, eta = geometry(nf, nt, npad, nedge, factor, span)
    th_lim = 0.8 * min(span * fd.max(), np.sqrt(np.abs(tau).max() / eta))
    E = station_fields(nf, nt, n_dish, eta, th_lim, seed)
    return dict(dlist=spectra(E), edges=edges, time=time, freq=freq, eta=float(eta), E=E)


# name: (nf, nt, npad, n_dish, nedge, factor, seed, tauMask in us) -- the golden cases (tests/golden/vlbi.npz)
GOLDEN = {
    "n1": (32, 32, 1, 1, 32, 0.8, 11, 0.0),           # one station: single_chunk_retrieval's arithmetic
    "n2": (48, 40, 1, 2, 40, 0.8, 12, 0.0),           # nothing cropped
    "n3crop": (32, 32, 0, 3, 36, 1.7, 13, 0.2),       # npad = 0, a curvature that crops the grid, a delay mask
    "odd": (33, 27, 3, 2, 30, 1.3, 14, 0.0),          # odd chunk, npad = 3
    "n2mask": (40, 48, 1, 2, 44, 0.7, 15, 0.3),       # delay mask, nothing cropped
}


def golden_case(name):
    nf, nt, npad, n_dish, nedge, factor, seed, mask = GOLDEN[name]
    c = case(nf, nt, npad, n_dish, nedge, factor, seed)
    c.update(npad=npad, n_dish=n_dish, tauMask=mask)
    return c


def fuzz_cases(count=24, seed=2024):
    """Seeded fuzz geometries: theta grids from sparse to dense -- centres per Doppler bin 0.3 .. 60, the range of the retrieval
    tail's fuzz (tests/test_gpu_retrieval.py); 10 of the 24 cases are drawn from 10 .. 60, where many (theta1, theta2) pairs
    share one CS pixel -- npad 0 / 1 / 3, 1-4 stations, odd and even chunks, curvatures on both sides of the crop.  The dense cases
    use short time axes so that the composite stays below ~2000 rows (n_dish nedge <= 2000): the oracle's eigsh and its N^2
    histograms then take seconds, and every case completes (tests/test_vlbi_cpu.py::test_fuzz_cases_complete_in_the_oracle)."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        npad = (0, 1, 3)[k % 3]
        n_dish = 1 + (k % 4)
        dense = (k % 5) in (0, 3)
        nf = int(rng.integers(16, 41))
        nt = int(rng.integers(16, 25 if dense else 41))
        if k % 2:
            nf, nt = nf | 1, nt | 1
        else:
            nf, nt = nf & ~1, nt & ~1
        lo, hi = (10.0, 60.0) if dense else (0.3, 6.0)
        cpb = float(np.exp(rng.uniform(np.log(lo), np.log(hi))))
        nedge = int(0.45 * nt * (npad + 1) * cpb) + 1         # edges span 0.45 of the nt (npad + 1) Doppler bins
        nedge = min(max(nedge + (nedge & 1), 12), min(800, (2000 // n_dish) & ~1))
        factor = float(rng.uniform(0.5, 2.0))
        mask = float(rng.choice([0.0, 0.0, 0.25]))
        c = case(nf, nt, npad, n_dish, nedge, factor, 1000 + k)
        c.update(npad=npad, n_dish=n_dish, tauMask=mask, dense=dense,
                 id="k%02d_%dx%d_p%d_d%d_e%d" % (k, nf, nt, npad, n_dish, nedge))
        out.append(c)
    return out


def fuzz_centres_per_bin(c):
    """Theta centres per Doppler bin of a fuzz case (retrieval_cases.centres_per_bin)."""
    from oracle import thth_oracle as to
    from retrieval_cases import centres_per_bin
    return centres_per_bin(to.fft_axis(c["time"], 1000.0, c["npad"]), c["edges"])


def align_joint(got, ref):
    """`got` [n_dish, nf, nt] rotated by ONE phase, common to all stations, onto `ref`."""
    got, ref = np.asarray(got), np.asarray(ref)
    return got * np.exp(-1j * np.angle(np.vdot(ref.ravel(), got.ravel())))


def align_on_first(got, ref):
    """`got` rotated by the phase that aligns station 1 ALONE: the other stations then test the phases between stations."""
    got, ref = np.asarray(got), np.asarray(ref)
    return got * np.exp(-1j * np.angle(np.vdot(ref[0].ravel(), got[0].ravel())))


def rel_err(got, ref):
    return float(np.abs(np.asarray(got) - np.asarray(ref)).max() / np.abs(np.asarray(ref)).max())


# ---- helpers shared by tests/test_vlbi_emu_cpu.py and tests/test_gpu_vlbi.py ---------------------------------------------------
def stored_case(gold, name):
    """A golden case as tests/golden/vlbi.npz stores it."""
    npad, n_dish = (int(v) for v in gold[f"{name}_par"])
    nspec = n_dish * (n_dish + 1) // 2
    return dict(dlist=[gold[f"{name}_in{i}"] for i in range(nspec)], edges=gold[f"{name}_edges"], time=gold[f"{name}_time"],
                freq=gold[f"{name}_freq"], eta=float(gold[f"{name}_eta"]), npad=npad, n_dish=n_dish, tauMask=float(gold[f"{name}_tauMask"]))


def chunk_of(c):
    return (c["dlist"], c["edges"], c["time"], c["freq"], c["eta"])


def params_of(c):
    """The reference's parameter tuple, idx_t = 3, idx_f = 5."""
    return (c["dlist"], c["edges"], c["time"], c["freq"], c["eta"], 3, 5, c["npad"], c["n_dish"], c["tauMask"], False)


def numpy_stack(c):
    """The conjugate spectra of a chunk as the reference forms them (ththmod.py:1293-1325, NumPy's own transform)."""
    from oracle import thth_oracle as to
    import vlbi_oracle as vo
    tau = to.fft_axis(c["freq"], 1.0, c["npad"])
    herm = [vo.spectrum_index(c["n_dish"], d, 0) for d in range(c["n_dish"])]
    out = []
    for i, x in enumerate(c["dlist"]):
        pad = np.pad(x, ((0, c["npad"] * x.shape[0]), (0, c["npad"] * x.shape[1])), mode="constant",
                     constant_values=x.mean() if i in herm else 0)
        CS = np.fft.fftshift(np.fft.fft2(pad))
        CS[np.abs(tau) < c["tauMask"]] = 0
        out.append(CS)
    return np.array(out), tau


def check_composite(thth, gold, name):
    """The gather on the reference's own conjugate spectra: every block of the composite equals the reference's thth_redmap
    output bit for bit, in both mirrored positions.  Returns (case, composite)."""
    from oracle import thth_oracle as to
    import vlbi_oracle as vo
    c = stored_case(gold, name)
    n_dish = c["n_dish"]
    nspec = n_dish * (n_dish + 1) // 2
    stack, tau = numpy_stack(c)
    grid = thth._Grid(tau, to.fft_axis(c["time"], 1000.0, c["npad"]), c["edges"])
    keep = grid.keep(c["eta"])
    n = gold[f"{name}_red0"].shape[0]
    assert keep.shape[0] == n
    # the spectra in REVERSED slots: the slot table, not the list position, names a spectrum's conjugate spectrum
    comp_t = thth._vlbi_composites_dev(thth.to_device(stack[::-1].copy()), np.arange(nspec)[::-1][None], [grid], [c["eta"]], [keep], n_dish)
    comp = comp_t.cpu().numpy()[0].reshape(n_dish * n, n_dish * n)
    for d1 in range(n_dish):
        for d2 in range(n_dish - d1):
            ref = gold[f"{name}_red{vo.spectrum_index(n_dish, d1, d2)}"]
            lower = comp[(d1 + d2) * n:(d1 + d2 + 1) * n, d1 * n:(d1 + 1) * n]
            upper = comp[d1 * n:(d1 + 1) * n, (d1 + d2) * n:(d1 + d2 + 1) * n]
            assert int((lower != ref).sum()) == 0, (d1, d2)
            assert int((upper != np.conjugate(ref.T)).sum()) == 0, (d1, d2)
            # the diagonal is zero everywhere (its weight sqrt|2 eta (th2 - th1)| is); the ANTI-diagonal is zeroed by the
            # Hermitian forcing (ththmod.py:113) on the dynamic spectra, and only there: a visibility keeps its own
            assert not np.diag(lower).any()
            if d2 == 0:
                assert not np.diag(lower[::-1]).any() and bool(gold[f"{name}_herm{vo.spectrum_index(n_dish, d1, d2)}"])
            elif c["tauMask"] == 0:                     # (the anti-diagonal reads the tau = 0 row: a delay mask zeroes it anyway)
                assert np.diag(lower[::-1]).any() and np.diag(upper[::-1]).any()
    assert np.array_equal(comp, vo.composite([gold[f"{name}_red{i}"] for i in range(nspec)], n_dish))
    return c, comp


def wide_case():
    """Edges 1.8 times the Doppler span: theta pairs whose Doppler index falls below -len(fd), where NumPy's fancy index in
    thth_map raises IndexError (ththmod.py:104)."""
    c = case(24, 24, 0, 2, 40, 0.3, 77, span=1.8)
    c.update(npad=0, n_dish=2, tauMask=0.0)
    return c
