"""The chunk-preparation helpers every theta-theta entry point shares (scintools_amd/ththmod.py, "small host helpers":
_chunk_axes, _chunk_grid, _tau_mask_rows, _reduced_centres_cached, _group_size) and the retrieval-chunk iterator of Dynspec:
host NumPy only, no GPU and no interpreter build."""
import numpy as np
import pytest

from scintools_amd import ththmod as T

MASK_ERROR = "tau mask is not a contiguous block of delays"


def inlined_mask_rows(tau, mask):
    """The block as conjugate_spectrum and the two batch functions each wrote it out."""
    lo = hi = 0
    sel = np.nonzero(np.abs(tau) < mask)[0]
    if sel.size:
        lo, hi = int(sel[0]), int(sel[-1]) + 1
        if hi - lo != sel.size:
            raise ValueError(MASK_ERROR)
    return lo, hi


@pytest.mark.parametrize("nf", [8, 9])
@pytest.mark.parametrize("npad", [0, 1])
def test_tau_mask_rows_is_the_inlined_expression(nf, npad):
    freq = 1400.0 + 0.1 * np.arange(nf)
    tau = T.fft_axis(freq, 1.0, npad)
    n, step = tau.shape[0], tau[1] - tau[0]
    assert n == (npad + 1) * nf
    assert T._tau_mask_rows(tau, 0.0) == inlined_mask_rows(tau, 0.0) == (0, 0)                     # nothing selected
    assert T._tau_mask_rows(tau, 2 * np.abs(tau).max()) == inlined_mask_rows(tau, 2 * np.abs(tau).max()) == (0, n)
    inner = T._tau_mask_rows(tau, 1.5 * step)                                                       # |tau| in {0, step}: three rows
    assert inner == inlined_mask_rows(tau, 1.5 * step) == (n // 2 - 1, n // 2 + 2) and 0 < inner[0] and inner[1] < n
    natural = np.fft.ifftshift(tau)                                                                 # 0, +step, ..., -step: two blocks
    with pytest.raises(ValueError) as err:
        T._tau_mask_rows(natural, 1.5 * step)
    assert str(err.value) == MASK_ERROR
    with pytest.raises(ValueError, match=MASK_ERROR):
        inlined_mask_rows(natural, 1.5 * step)


def chunk_inputs(nf=16, nt=12, nedge=14):
    time, freq = np.arange(nt) * 10.0, 1400.0 + 0.1 * np.arange(nf)
    fd = T.fft_axis(time, 1000.0, 1)
    return time, freq, np.linspace(-fd.max() / 2, fd.max() / 2, nedge)


def test_chunk_axes_are_the_stripped_inputs_and_their_conjugate_axes():
    time, freq, edges = chunk_inputs()
    time_v, freq_v, edges_v, tau, fd = T._chunk_axes(list(time), freq, edges, 1)
    assert np.array_equal(time_v, time) and np.array_equal(freq_v, freq) and np.array_equal(edges_v, edges)
    assert np.array_equal(tau, T.fft_axis(freq, 1.0, 1)) and np.array_equal(fd, T.fft_axis(time, 1000.0, 1))
    assert tau.shape == (32,) and fd.shape == (24,)


def test_chunk_grid_is_shared_by_equal_axes_and_edges_only():
    time, freq, edges = chunk_inputs()
    cache = {}
    a = T._chunk_grid(time, freq, edges, 1, cache)
    assert T._chunk_grid(time.copy(), freq.copy(), edges.copy(), 1, cache) is a and len(cache) == 1
    assert T._chunk_grid(time + 500.0, freq, edges, 1, cache) is a        # the key holds the step and the length of an axis, as fft_axis reads them
    ulp = edges.copy()
    ulp[3] = np.nextafter(ulp[3], np.inf)
    b = T._chunk_grid(time, freq, ulp, 1, cache)
    assert b is not a and len(cache) == 2 and b.edges[3] != a.edges[3]
    assert T._chunk_grid(time, freq, ulp, 1, cache) is b
    assert T._chunk_grid(time[:-1], freq, edges, 1, cache) is not a and T._chunk_grid(time, freq * 2, edges, 1, cache) is not a
    assert len(cache) == 4


def test_chunk_grid_cache_serves_one_npad():
    """The key does not hold npad (the callers make a cache per call, and a call has one npad): each npad gets a cache of its
    own, and the grids of two of them differ in their padded lengths."""
    time, freq, edges = chunk_inputs()
    caches = {0: {}, 1: {}}
    g0, g1 = (T._chunk_grid(time, freq, edges, npad, caches[npad]) for npad in (0, 1))
    assert g0 is not g1 and list(caches[0].values()) == [g0] and list(caches[1].values()) == [g1]
    assert list(caches[0]) == list(caches[1])
    assert (g0.geom.ntau, g0.geom.nfd) == (16, 12) and (g1.geom.ntau, g1.geom.nfd) == (32, 24)


def test_chunk_grid_without_a_cache_is_a_fresh_equal_grid():
    time, freq, edges = chunk_inputs()
    a, b = T._chunk_grid(time, freq, edges, 1), T._chunk_grid(time, freq, edges, 1, None)
    assert a is not b and bytes(a.geom) == bytes(b.geom) and np.array_equal(a.th_cents, b.th_cents)
    ref = T._Grid(T.fft_axis(freq, 1.0, 1), T.fft_axis(time, 1000.0, 1), edges)
    assert bytes(a.geom) == bytes(ref.geom) and np.array_equal(a.th_cents, ref.th_cents) and np.array_equal(a.tau, ref.tau)


def test_reduced_centres_are_cached_for_a_run_of_centres_only():
    time, freq, edges = chunk_inputs(nedge=22)
    grid = T._chunk_grid(time, freq, edges, 1)
    cache = {}
    run = np.arange(4, 4 + 11, dtype=np.int32)
    first = T._reduced_centres_cached(grid, run, cache)
    assert np.array_equal(first, T._theta_centres(grid.edges_red(run))) and list(cache) == [(id(grid), 4, 11)]
    assert T._reduced_centres_cached(grid, run.copy(), cache) is first and len(cache) == 1
    other = T._chunk_grid(time, freq, edges, 1)                                   # an equal grid that is another object: its own entry
    assert T._reduced_centres_cached(other, run, cache) is not first and len(cache) == 2
    holes = np.array([2, 3, 5, 6, 9, 10, 11], dtype=np.int32)
    got = T._reduced_centres_cached(grid, holes, cache)
    assert np.array_equal(got, T._theta_centres(grid.edges_red(holes))) and len(cache) == 2
    assert T._reduced_centres_cached(grid, holes, cache) is not got


def test_group_size():
    default = T.RETRIEVAL_GROUP_BYTES
    assert default == 8 << 30
    assert T._group_size(16 * 128 * 300) == T._group_size(16 * 128 * 300, None) == T._group_size(16 * 128 * 300, 0) == default // (16 * 128 * 300)
    assert T._group_size(1000, 2500) == 2 and T._group_size(1000, 2500.0) == 2 and isinstance(T._group_size(1000, 2500.0), int)
    assert T._group_size(default + 1) == 1 and T._group_size(1000, 1) == 1                       # a chunk larger than the budget
    assert T._group_size(1, None, cap=65535) == 65535 and T._group_size(1, 65534, cap=65535) == 65534
    assert T._group_size(1000, 1, cap=65535) == 1


class Observation:
    """8 channels x 12 sub-integrations."""
    rng = np.random.default_rng(3)
    dyn = rng.standard_normal((8, 12)) + 5.0
    freqs, times, df, dt = 1400.0 + 0.5 * np.arange(8), 10.0 * np.arange(12), 0.5, 10.0


def test_retrieval_chunks_of_dynspec_are_what_both_routes_build(monkeypatch):
    """Dynspec._retrieval_chunks on an 8 x 12 observation with cwf = 4, cwt = 6 (3 x 3 half-overlapping chunks) against the
    slicing rule written out (dynspec.py:1777-1800); then the parameter lists of both routes of thetatheta_chunks -- what a
    pool receives for single_chunk_retrieval, and what chunk_retrieval_batch and chunk_cut_device receive -- element for element."""
    import torch
    from scintools_amd.dynspec import Dynspec
    d = Dynspec(dyn=Observation(), process=False, verbose=False)
    d.prep_thetatheta(cwf=4, cwt=6, eta_min=0.5, eta_max=2.0, nedge=6, npad=1, tau_mask=0.1)
    d.ththeta = 1.25
    assert (d.ncf_ret, d.nct_ret) == (3, 3)
    expected = []
    for cf in range(3):
        for ct in range(3):
            freq2 = d.freqs[2 * cf:2 * cf + 4]
            expected.append((cf, ct, slice(2 * cf, 2 * cf + 4), slice(3 * ct, 3 * ct + 6), freq2,
                             1.25 * (d.fref / freq2.mean()) ** 2, d.edges * (freq2.mean() / d.fref)))
    got = list(d._retrieval_chunks())
    assert len(got) == 9
    for g, e in zip(got, expected):
        assert g[:4] == e[:4] and np.array_equal(g[4], e[4]) and g[5] == e[5] and np.array_equal(g[6], e[6])

    class RecordingPool:
        def map(self, fn, pars):
            assert fn is T.single_chunk_retrieval
            self.pars = list(pars)
            return [(np.full((4, 6), 10.0 * p[6] + p[5], dtype=complex), p[6], p[5]) for p in self.pars]
    pool = RecordingPool()
    d.thetatheta_chunks(pool=pool, verbose=True)
    assert len(pool.pars) == 9
    for p, (cf, ct, fs, ts, freq2, eta, edges) in zip(pool.pars, expected):
        dspec2 = np.copy(d.dyn[fs, ts])
        dspec2 -= np.nanmean(dspec2)
        assert len(p) == 10 and np.array_equal(p[0], np.nan_to_num(dspec2)) and np.array_equal(p[1], edges)
        assert np.array_equal(p[2], d.times[ts]) and np.array_equal(p[3], freq2) and p[4] == eta
        assert p[5:] == (ct, cf, 1, 0.1, True)
        assert d.chunks[cf, ct, 0, 0] == 10.0 * cf + ct

    seen = {}

    def cut(dyn_t, origins, cwf, cwt, fortran_order=False):
        seen["origins"], seen["cw"] = list(origins), (cwf, cwt)
        return torch.zeros((len(origins), cwf, cwt), dtype=torch.float64), torch.zeros(len(origins), dtype=torch.float64)

    def batch(pars, npad, tau_mask, **kw):
        seen["pars"], seen["args"] = list(pars), (npad, tau_mask)
        return torch.zeros((len(pars), 4, 6), dtype=torch.complex128)
    monkeypatch.setattr(T, "to_device", lambda a, dtype: torch.from_numpy(np.ascontiguousarray(a)))
    monkeypatch.setattr(T, "chunk_cut_device", cut)
    monkeypatch.setattr(T, "chunk_retrieval_batch", batch)
    d.thetatheta_chunks()
    assert seen["origins"] == [(2 * cf, 3 * ct) for cf in range(3) for ct in range(3)] and seen["cw"] == (4, 6)
    assert seen["args"] == (1, 0.1) and len(seen["pars"]) == 9
    for p, (cf, ct, fs, ts, freq2, eta, edges) in zip(seen["pars"], expected):
        assert len(p) == 5 and p[0] is None and np.array_equal(p[1], edges) and np.array_equal(p[2], d.times[ts])
        assert np.array_equal(p[3], freq2) and p[4] == eta
