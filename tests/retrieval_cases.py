"""Geometries and the oracle for the tail of phase retrieval (ththmod._retrieval_tail_dev -> scint_retrieval_tail), shared by
tests/test_retrieval_emu_cpu.py and tests/test_gpu_retrieval.py.

A chunk of nf x nt pixels (10 s time steps, 0.1 MHz channels), zero-padded npad times, has the Doppler step 1000 / (nt (npad+1)
10) mHz.  Edges that span half the Doppler range put `centres_per_bin` theta centres in one Doppler bin; `factor` scales the
curvature that fills the arc (eta max(theta^2) = max|tau|).  Small factors put many centres of a Doppler bin into one delay
bin, large ones crop the grid and make the zero-Doppler column hold mirrored pairs (-x, +x) far apart in j."""
import numpy as np


def axes(nf, nt, npad):
    from oracle import thth_oracle as to
    time = np.arange(nt) * 10.0
    freq = 1400.0 + 0.1 * np.arange(nf)
    return time, freq, to.fft_axis(freq, 1.0, npad), to.fft_axis(time, 1000.0, npad)


def geometry(nf, nt, npad, nedge, factor, span=0.5):
    """(time, freq, tau, fd, edges, eta) of one chunk."""
    from oracle import thth_oracle as to
    time, freq, tau, fd = axes(nf, nt, npad)
    edges = np.linspace(-span * fd.max(), span * fd.max(), nedge)
    th = to.theta_centres(edges)
    eta = factor * np.abs(tau).max() / (th ** 2).max()
    return time, freq, tau, fd, edges, eta


def centres_per_bin(fd, edges):
    return float((fd[1] - fd[0]) / (edges[1] - edges[0]))


def tail_inputs(thth, tau, fd, edges, eta):
    """The reduced grid a retrieval of this chunk uses: (_Grid, kept indices, reduced centres, reduced edges); the crop checked
    against the oracle's."""
    from oracle import thth_oracle as to
    grid = thth._Grid(tau, fd, edges)
    keep = grid.keep(eta)
    mask, th = to.reduced_keep(tau, fd, eta, edges)
    assert np.array_equal(np.nonzero(mask)[0], keep)
    edges_red = to.reduced_edges(th[mask])
    th_red = thth._theta_centres(grid.edges_red(keep))
    assert np.array_equal(th_red, to.theta_centres(edges_red))
    return grid, keep, th_red, edges_red


def oracle_tail(row, tau, fd, eta, edges_red, nf, nt):
    """single_chunk_retrieval's tail (oracle/thth_oracle.py): theta-theta of the E field zero but for row N/2, non-Hermitian
    back-map, shifted inverse FFT cropped to the chunk and scaled (the centre pixel's NaN becomes 0 in rev_map)."""
    from oracle import thth_oracle as to
    n = row.shape[0]
    E = np.zeros((n, n), dtype=complex)
    E[n // 2] = row
    with np.errstate(all="ignore"):
        recov = to.rev_map(E, tau, fd, eta, edges_red, hermetian=False)
    return np.fft.ifft2(np.fft.ifftshift(recov))[:nf, :nt] * (nf * nt / 4)


def random_row(rng, n):
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def align(a, ref):
    """a rotated onto ref's global phase."""
    return a * np.exp(-1j * np.angle(np.vdot(ref, a)))

