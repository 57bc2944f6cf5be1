"""The tail of phase retrieval (ththmod._retrieval_tail_dev -> scint_retrieval_tail: the one-row back-map rev_row_kernel and the
shifted inverse FFT) and the odd single-chunk mosaic, interpreted on the host (tests/emu) against the oracle -- runs without a GPU.

The theta grids here are dense against the Doppler step (up to ~45 centres per Doppler bin; the product's default grids hold one
to three): a pixel then collects the weights of long runs of j, and in the Doppler bin of theta_j = theta_i the pixel of -x recurs
after those of smaller |x|.  See tests/retrieval_cases.py for the geometry."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)
import retrieval_cases as rc  # noqa: E402


@pytest.fixture()
def emu(monkeypatch):
    import subprocess
    import emulated
    try:
        emulated.install(monkeypatch)
    except (RuntimeError, OSError, subprocess.CalledProcessError) as exc:    # no usable clang++ on this machine
        pytest.skip(f"host interpreter could not be built: {exc}")
    from scintools_amd import ththmod
    return ththmod


@pytest.fixture(scope="module")
def to():
    from oracle import thth_oracle
    return thth_oracle


def _tail_vs_oracle(emu, rng, nf, nt, npad, nedge, factor):
    time, freq, tau, fd, edges, eta = rc.geometry(nf, nt, npad, nedge, factor)
    grid, keep, th_red, edges_red = rc.tail_inputs(emu, tau, fd, edges, eta)
    n = keep.shape[0]
    row = rc.random_row(rng, n)
    args = (row[None], th_red[None], [n], None, [grid], [eta], nf, nt)
    got = emu._retrieval_tail_dev(*args).cpu().numpy()[0]
    ref = rc.oracle_tail(row, tau, fd, eta, edges_red, nf, nt)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    assert np.array_equal(emu._retrieval_tail_dev(*args).cpu().numpy()[0], got)          # the same bits twice
    return err, rc.centres_per_bin(fd, edges), n


# (nf, nt, npad, nedge, curvature / the arc-filling one): centres per Doppler bin in the comment
TAIL_CASES = [
    (48, 40, 0, 160, 1.0),     # 8.4: the 8-position window still sufficed here
    (48, 40, 0, 180, 0.5),     # 9.5: the first dropped weights
    (48, 40, 0, 400, 1.0),     # 21
    (48, 40, 0, 400, 0.2),     # 21, long runs of j per pixel
    (48, 40, 1, 400, 50.0),    # 10.5, mirrored pairs of the zero-Doppler column more than 8 positions apart
    (33, 41, 3, 40, 1.0),      # 0.5, odd chunk
    (47, 40, 1, 76, 3.0),      # 1.9
    (48, 39, 0, 324, 1.0),     # 17
    (48, 40, 3, 170, 8.0),     # 2.1 at npad 3
    (32, 24, 0, 496, 0.5),     # 45
]


@pytest.mark.parametrize("nf,nt,npad,nedge,factor", TAIL_CASES)
def test_retrieval_tail_vs_oracle(emu, nf, nt, npad, nedge, factor):
    """scint_retrieval_tail of one random row against the oracle's tail of single_chunk_retrieval (zero N x N matrix with row N/2
    set, rev_map(hermetian=False), ifft2(ifftshift(.))[:nf, :nt] nf nt / 4): 1e-12 of the peak, where one dropped weight of a unit
    row is orders of magnitude above; a second call gives the same bits."""
    rng = np.random.default_rng(nf * 1000 + nt * 10 + npad + nedge)
    err, cpb, n = _tail_vs_oracle(emu, rng, nf, nt, npad, nedge, factor)
    assert err <= 1e-12, (err, cpb, n)


def test_retrieval_tail_classes_groups_and_skipped_chunks(emu):
    """Two classes back to back (the pair counts are formed per class): nine chunks of one grid and curvature -- more than the
    eight of one launch (kTailGroup) -- with a skipped chunk (keep_n < 2) in the middle that keeps what the caller put there,
    then two chunks of a second curvature.  Dense grid (21 centres per Doppler bin), every chunk against the oracle."""
    import torch
    nf, nt, npad = 48, 40, 0
    rng = np.random.default_rng(77)
    chunks = []
    for factor, count in ((0.2, 9), (1.0, 2)):
        time, freq, tau, fd, edges, eta = rc.geometry(nf, nt, npad, 400, factor)
        grid, keep, th_red, edges_red = rc.tail_inputs(emu, tau, fd, edges, eta)
        for _ in range(count):
            chunks.append((grid, eta, th_red, edges_red, rc.random_row(rng, keep.shape[0])))
    M = max(c[2].shape[0] for c in chunks)
    n = len(chunks)
    rows, th_all, keep_n = np.zeros((n, M), dtype=complex), np.zeros((n, M)), np.zeros(n, dtype=np.int32)
    for k, (grid, eta, th_red, edges_red, row) in enumerate(chunks):
        rows[k, :row.shape[0]], th_all[k, :row.shape[0]], keep_n[k] = row, th_red, row.shape[0]
    skipped = 4
    keep_n[skipped] = 1
    class_id = np.array([0] * 9 + [1] * 2, dtype=np.int32)
    init = torch.full((n, nf, nt), 3.0 - 2.0j, dtype=torch.complex128)
    out = emu._retrieval_tail_dev(rows, th_all, keep_n, class_id, [c[0] for c in chunks], [c[1] for c in chunks], nf, nt,
                                  out_t=init.clone()).cpu().numpy()
    assert np.array_equal(out[skipped], init[skipped].numpy())
    for k, (grid, eta, th_red, edges_red, row) in enumerate(chunks):
        if k == skipped:
            continue
        ref = rc.oracle_tail(row, grid.tau, grid.fd, eta, edges_red, nf, nt)
        assert np.abs(out[k] - ref).max() <= 1e-12 * np.abs(ref).max(), k
    # the classes taken from the inputs (what chunk_retrieval_batch does) give the same bits
    auto = emu._retrieval_tail_dev(rows, th_all, keep_n, None, [c[0] for c in chunks], [c[1] for c in chunks], nf, nt,
                                   out_t=init.clone()).cpu().numpy()
    assert np.array_equal(auto, out)


@pytest.mark.parametrize("npad,nedge", [(0, 180), (0, 400), (1, 400)])
def test_chunk_retrieval_batch_on_dense_grids_vs_oracle(emu, to, npad, nedge):
    """chunk_retrieval_batch (eigenpair sweep + retrieval tail) of a 48 x 40 chunk on theta grids with 10 to 21 centres per
    Doppler bin against the oracle's single_chunk_retrieval: 1e-9 of the peak after removing the global phase."""
    from scintools_amd.synth import arc_dynspec
    dyn, freqs, times, eta_true = arc_dynspec(48, 40, seed=41 + npad, nimg=8)
    dyn = dyn - dyn.mean()
    fd = to.fft_axis(times, 1000.0, npad)
    edges = np.linspace(-fd.max() / 2, fd.max() / 2, nedge)
    assert rc.centres_per_bin(fd, edges) >= 9
    got = emu.chunk_retrieval_batch([(dyn, edges, times, freqs, eta_true)], npad, 0.0)[0]
    ref = to.single_chunk_retrieval(dyn, edges, times, freqs, eta_true, npad)
    assert np.abs(rc.align(got, ref) - ref).max() <= 1e-9 * np.abs(ref).max()


@pytest.mark.parametrize("shape", [(1, 1, 33, 41), (1, 3, 33, 40), (3, 1, 32, 41)])
def test_device_mosaic_of_odd_single_chunk_axes(emu, to, shape):
    """An axis with ONE chunk has no taper, so its chunk size may be odd (prep_thetatheta without cwf / cwt makes the whole
    observation one chunk): mosaic_device equals the host loop and the oracle's mosaic bit for bit."""
    import torch
    rng = np.random.default_rng(sum(shape))
    ch = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    got = emu.mosaic_device(torch.from_numpy(ch)).numpy()
    assert np.array_equal(got, emu.mosaic(ch)) and np.array_equal(got, to.mosaic(ch))


@pytest.mark.parametrize("shape", [(2, 1, 33, 40), (1, 2, 32, 41)])
def test_device_mosaic_of_odd_chunks_on_a_tapered_axis_raises(emu, to, shape):
    """Several chunks along an odd axis: the reference's half tapers do not broadcast (neither does the oracle's); nor does this."""
    import torch
    ch = np.ones(shape, dtype=complex)
    with pytest.raises(ValueError):
        to.mosaic(ch)
    with pytest.raises(ValueError):
        emu.mosaic_device(torch.from_numpy(ch))


def test_odd_single_chunk_observation_wavefield(emu):
    """prep_thetatheta without cwf / cwt makes the whole observation ONE chunk of its own, odd, shape: calc_wavefield (batched
    retrieval, device mosaic) completes and equals the pool route (single_chunk_retrieval per chunk) to 1e-9 of the peak after
    removing the global phase."""
    from scintools_amd.dynspec import Dynspec
    from scintools_amd.synth import arc_dynspec
    dyn, freqs, times, eta_true = arc_dynspec(33, 41, seed=9, nimg=8)

    class B:
        pass
    B.dyn, B.freqs, B.times, B.dt, B.df = dyn, freqs, times, float(times[1] - times[0]), float(freqs[1] - freqs[0])

    class SerialPool:
        def map(self, fn, it):
            return [fn(x) for x in it]
    d = Dynspec(dyn=B(), process=False, verbose=False)
    d.prep_thetatheta(eta_min=0.8 * eta_true, eta_max=1.25 * eta_true, fw=0.3, npad=1)
    assert (d.cwf, d.cwt, d.ncf_ret, d.nct_ret) == (33, 41, 1, 1)
    d.calc_wavefield()
    wf = d.wavefield.copy()
    d.thetatheta_chunks(pool=SerialPool())
    ref = d.chunks[0, 0]
    assert wf.shape == ref.shape and np.abs(ref).max() > 0
    assert np.abs(rc.align(wf, ref) - ref).max() <= 1e-9 * np.abs(ref).max()
