"""The tail of phase retrieval on an MI355X (ththmod._retrieval_tail_dev -> scint_retrieval_tail: the one-row back-map
rev_row_kernel and the shifted inverse FFT) against the oracle, on theta grids from far sparser to far denser than the Doppler
step; the batched retrieval against the pool route on dense grids; the odd single-chunk mosaic.  Geometry: tests/retrieval_cases.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import retrieval_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def thth():
    from scintools_amd import ththmod
    from scintools_amd.device import require_gpu
    require_gpu()
    return ththmod


@pytest.fixture(scope="module")
def to():
    from oracle import thth_oracle
    return thth_oracle


class SerialPool:
    def map(self, fn, it):
        return [fn(x) for x in it]


def test_retrieval_tail_fuzz_vs_oracle(thth):
    """30 seeded random chunks: odd and even sizes, npad 0 / 1 / 3, 0.3 to 60 theta centres per Doppler bin, curvatures 0.2 to 50
    times the one that fills the arc -- long runs of j per pixel, and mirrored pairs (-x, +x) of the zero-Doppler column far apart
    in j.  Each chunk's tail of one random row against the oracle's tail of single_chunk_retrieval: 1e-12 of the peak; a second
    call gives the same bits."""
    rng = np.random.default_rng(20261016)
    worst, most = 0.0, 0.0
    for trial in range(30):
        nf, nt = int(rng.integers(12, 160)), int(rng.integers(12, 160))
        npad = int(rng.choice([0, 1, 3]))
        if trial % 3 == 0:                                   # short unpadded time axes: the densest grids within ~800 centres
            nt, npad = int(rng.integers(12, 32)), 0
        cpb = float(10 ** rng.uniform(np.log10(0.3), np.log10(60)))
        factor = float(10 ** rng.uniform(np.log10(0.2), np.log10(50)))
        _, _, _, fd = rc.axes(nf, nt, npad)
        nedge = 2 * max(3, min(int(cpb * fd.max() / (fd[1] - fd[0]) / 2), 400))
        time, freq, tau, fd, edges, eta = rc.geometry(nf, nt, npad, nedge, factor)
        if thth._Grid(tau, fd, edges).keep(eta).shape[0] < 3:           # (a coarse grid cropped to nothing: the arc-filling curvature)
            time, freq, tau, fd, edges, eta = rc.geometry(nf, nt, npad, nedge, 1.0)
        grid, keep, th_red, edges_red = rc.tail_inputs(thth, tau, fd, edges, eta)
        n = keep.shape[0]
        row = rc.random_row(rng, n)
        args = (row[None], th_red[None], [n], None, [grid], [eta], nf, nt)
        got = thth._retrieval_tail_dev(*args).cpu().numpy()[0]
        ref = rc.oracle_tail(row, tau, fd, eta, edges_red, nf, nt)
        err = np.abs(got - ref).max() / np.abs(ref).max()
        key = (trial, nf, nt, npad, nedge, factor, n, rc.centres_per_bin(fd, edges))
        assert err <= 1e-12, (err, key)
        assert np.array_equal(thth._retrieval_tail_dev(*args).cpu().numpy()[0], got), key
        worst, most = max(worst, err), max(most, rc.centres_per_bin(fd, edges))
    print(f"\nretrieval tail fuzz: largest error {worst:.2e} of the peak, up to {most:.1f} centres per Doppler bin")


@pytest.mark.parametrize("nf,nt,npad,nedge,factor", [(48, 40, 0, 400, 1.0), (48, 40, 0, 400, 0.2), (48, 40, 1, 400, 50.0),
                                                     (48, 40, 0, 180, 0.5), (33, 41, 3, 40, 1.0)])
def test_retrieval_tail_named_cases_vs_oracle(thth, nf, nt, npad, nedge, factor):
    """The interpreter's cases where an 8-position window dropped weights (tests/test_retrieval_emu_cpu.py), on the GPU."""
    time, freq, tau, fd, edges, eta = rc.geometry(nf, nt, npad, nedge, factor)
    grid, keep, th_red, edges_red = rc.tail_inputs(thth, tau, fd, edges, eta)
    row = rc.random_row(np.random.default_rng(nedge), keep.shape[0])
    got = thth._retrieval_tail_dev(row[None], th_red[None], [keep.shape[0]], None, [grid], [eta], nf, nt).cpu().numpy()[0]
    ref = rc.oracle_tail(row, tau, fd, eta, edges_red, nf, nt)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


def test_retrieval_tail_classes_groups_and_skipped_chunks(thth):
    """Two classes back to back: nine chunks of one grid and curvature (more than the eight of one launch) with a skipped chunk
    (keep_n < 2) in the middle that keeps what the caller put there, then two of a second curvature; 21 centres per Doppler bin."""
    import torch
    from scintools_amd.device import require_gpu
    nf, nt, npad = 48, 40, 0
    rng = np.random.default_rng(78)
    chunks = []
    for factor, count in ((0.2, 9), (1.0, 2)):
        time, freq, tau, fd, edges, eta = rc.geometry(nf, nt, npad, 400, factor)
        grid, keep, th_red, edges_red = rc.tail_inputs(thth, tau, fd, edges, eta)
        for _ in range(count):
            chunks.append((grid, eta, th_red, edges_red, rc.random_row(rng, keep.shape[0])))
    M, n = max(c[2].shape[0] for c in chunks), len(chunks)
    rows, th_all, keep_n = np.zeros((n, M), dtype=complex), np.zeros((n, M)), np.zeros(n, dtype=np.int32)
    for k, (grid, eta, th_red, edges_red, row) in enumerate(chunks):
        rows[k, :row.shape[0]], th_all[k, :row.shape[0]], keep_n[k] = row, th_red, row.shape[0]
    skipped = 4
    keep_n[skipped] = 0
    init = torch.full((n, nf, nt), 3.0 - 2.0j, dtype=torch.complex128, device=require_gpu())
    out = thth._retrieval_tail_dev(rows, th_all, keep_n, np.array([0] * 9 + [1] * 2), [c[0] for c in chunks],
                                   [c[1] for c in chunks], nf, nt, out_t=init.clone()).cpu().numpy()
    assert np.array_equal(out[skipped], init[skipped].cpu().numpy())
    for k, (grid, eta, th_red, edges_red, row) in enumerate(chunks):
        if k != skipped:
            ref = rc.oracle_tail(row, grid.tau, grid.fd, eta, edges_red, nf, nt)
            assert np.abs(out[k] - ref).max() <= 1e-12 * np.abs(ref).max(), k


@pytest.mark.parametrize("npad,nedge", [(0, 400), (1, 400), (0, 760)])
def test_chunk_retrieval_batch_on_dense_grids_vs_oracle(thth, to, npad, nedge):
    """chunk_retrieval_batch of a 48 x 40 chunk on theta grids with 10 to 40 centres per Doppler bin against the oracle's
    single_chunk_retrieval: 1e-9 of the peak after removing the global phase."""
    from scintools_amd.synth import arc_dynspec
    dyn, freqs, times, eta_true = arc_dynspec(48, 40, seed=41 + npad, nimg=8)
    dyn = dyn - dyn.mean()
    fd = to.fft_axis(times, 1000.0, npad)
    edges = np.linspace(-fd.max() / 2, fd.max() / 2, nedge)
    assert rc.centres_per_bin(fd, edges) >= 10
    got = thth.chunk_retrieval_batch([(dyn, edges, times, freqs, eta_true)], npad, 0.0)[0]
    ref = to.single_chunk_retrieval(dyn, edges, times, freqs, eta_true, npad)
    assert np.abs(rc.align(got, ref) - ref).max() <= 1e-9 * np.abs(ref).max()


def test_grouped_retrieval_with_a_failing_chunk_shares_grids(thth, capsys, monkeypatch):
    """Four 16 x 12 chunks of one frequency row at npad = 1 in two groups of two.  Chunk 2 carries a single edge, a grid that
    cannot be built: it is reported and left zero, and chunk 3 takes its slot of the second group's stack.  The other three
    equal their own single_chunk_retrieval to 1e-9 of the peak after removing the global phase.  Grids are shared within a group:
    three constructions -- one for chunks 0 and 1 together, the failing one of chunk 2, one for chunk 3."""
    from scintools_amd.synth import arc_dynspec
    npad = 1
    time, freq, tau, fd, edges, eta = rc.geometry(16, 12, npad, 14, 1.0)
    chunks = []
    for k in range(4):
        dyn = arc_dynspec(16, 12, seed=70 + k, nimg=6)[0]
        chunks.append((dyn - dyn.mean(), edges.copy(), time.copy(), freq.copy(), eta))
    chunks[2] = (chunks[2][0], edges[:1]) + chunks[2][2:]
    built = []
    init = thth._Grid.__init__

    def counting(self, tau, fd, edges):
        built.append(np.shape(edges)[0])
        init(self, tau, fd, edges)
    with monkeypatch.context() as m:
        m.setattr(thth._Grid, "__init__", counting)
        got = thth.chunk_retrieval_batch(chunks, npad, 0.0, group_bytes=2 * 16 * (2 * 16) * (2 * 12))
    assert built == [14, 1, 14]          # (the count before the chunk preparation moved into ththmod._chunk_grid: the same three)
    assert "Chunk 2: " in capsys.readouterr().out
    assert got.shape == (4, 16, 12) and not got[2].any()
    for k in (0, 1, 3):
        ref = thth.single_chunk_retrieval(chunks[k] + (0, 0, npad, 0.0, False))[0]
        assert np.abs(ref).max() > 0
        err = np.abs(rc.align(got[k], ref) - ref).max() / np.abs(ref).max()
        print(f"chunk {k}: batch against single_chunk_retrieval {err:.2e} of the peak")
        assert err <= 1e-9, k


def test_dense_grid_wavefield_batched_route_equals_pool_route(thth, golden):
    """A Dynspec of several chunks with a dense nedge (about 17 centres per Doppler bin at npad = 1): calc_wavefield (batched
    route, retrieval tail) against thetatheta_chunks(pool=...) (single_chunk_retrieval per chunk, the general back-map), each
    chunk to 1e-9 of its peak after phase alignment."""
    from scintools_amd.dynspec import Dynspec
    f = golden("fit_thetatheta.npz")

    class B:
        dyn, freqs, times, dt, df = f["dspec"][:128], f["freq"][:128], f["time"], float(f["dt"]), float(f["df"])
    d = Dynspec(dyn=B(), verbose=False)
    d.prep_thetatheta(cwf=64, cwt=100, edges_lim=.3, eta_min=30, eta_max=50, nedge=600, npad=1)
    fd = thth.fft_axis(d.times[:d.cwt], 1000.0, d.npad)
    assert rc.centres_per_bin(fd, d.edges) >= 10 and d.ncf_ret * d.nct_ret >= 4
    d.calc_wavefield()
    batched = d.chunks.copy()
    d.thetatheta_chunks(pool=SerialPool())
    for cf in range(d.ncf_ret):
        for ct in range(d.nct_ret):
            b = d.chunks[cf, ct]
            assert np.abs(b).max() > 0
            assert np.abs(rc.align(batched[cf, ct], b) - b).max() <= 1e-9 * np.abs(b).max(), (cf, ct)


@pytest.mark.parametrize("shape", [(1, 1, 33, 41), (1, 3, 33, 40), (3, 1, 32, 41)])
def test_device_mosaic_of_odd_single_chunk_axes(thth, to, shape):
    """An axis with one chunk has no taper: odd sizes there give the host loop's and the oracle's mosaic bit for bit."""
    import torch
    from scintools_amd.device import require_gpu
    rng = np.random.default_rng(sum(shape))
    ch = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    got = thth.mosaic_device(torch.from_numpy(ch).to(require_gpu())).cpu().numpy()
    assert np.array_equal(got, thth.mosaic(ch)) and np.array_equal(got, to.mosaic(ch))


def test_device_mosaic_of_odd_chunks_on_a_tapered_axis_raises(thth):
    import torch
    from scintools_amd.device import require_gpu
    with pytest.raises(ValueError):
        thth.mosaic_device(torch.ones((2, 1, 33, 40), dtype=torch.complex128, device=require_gpu()))


def test_odd_single_chunk_observation_wavefield(thth):
    """prep_thetatheta without cwf / cwt: one chunk of the observation's odd shape; calc_wavefield completes and equals the pool
    route to 1e-9 of the peak after phase alignment."""
    from scintools_amd.dynspec import Dynspec
    from scintools_amd.synth import arc_dynspec
    dyn, freqs, times, eta_true = arc_dynspec(65, 81, seed=9, nimg=12)

    class B:
        pass
    B.dyn, B.freqs, B.times, B.dt, B.df = dyn, freqs, times, float(times[1] - times[0]), float(freqs[1] - freqs[0])
    d = Dynspec(dyn=B(), process=False, verbose=False)
    d.prep_thetatheta(eta_min=0.5 * eta_true, eta_max=2.0 * eta_true)
    assert (d.cwf, d.cwt, d.ncf_ret, d.nct_ret) == (65, 81, 1, 1)
    d.calc_wavefield()
    wf = d.wavefield.copy()
    d.thetatheta_chunks(pool=SerialPool())
    ref = d.chunks[0, 0]
    assert wf.shape == ref.shape and np.abs(ref).max() > 0
    assert np.abs(rc.align(wf, ref) - ref).max() <= 1e-9 * np.abs(ref).max()
