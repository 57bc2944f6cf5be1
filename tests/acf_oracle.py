"""Host restatement of the reference's theoretical 2-D ACF (scint_sim.py:494-678, ACF.calc_acf): the DIRECT sums over the M x M grids
with the summed phase argument, one np.sum per (time-lag sample, frequency lag) -- not the factorisation the device uses.  Pinned bit
for bit to the unmodified reference's outputs (tests/golden/acf.npz) by tests/test_acf_cpu.py; it also returns the complex field, which
the reference discards, and the rounding scale of every lag."""
import numpy as np


def sampling(taumax=4, nt=51, ar=1, spatial_factor=2, resolution_factor=1, core_factor=2, auto_sampling=True):
    """(nt made odd, sp_fac, res_fac, core_fac, dsp) as the constructor sets them."""
    if nt % 2 == 0:
        nt += 1
    if auto_sampling:
        sp_fac, res_fac, core_fac = 6 * ar / taumax, 1 + ar / 3, 4
    else:
        sp_fac, res_fac, core_fac = spatial_factor, resolution_factor, core_factor
    return nt, sp_fac, res_fac, core_fac, 4 * taumax / (nt - 1)


def efield_plane(grid, sqrtar, alph2):
    X, Y = np.meshgrid(grid, grid)
    return X, Y, np.exp(-0.5 * ((X / sqrtar)**2 + (Y * sqrtar)**2)**alph2)


def acf_model(psi=0, phasegrad=0, theta=0, ar=1, alpha=5 / 3, taumax=4, dnumax=4, nf=51, nt=51, amp=1, wn=0, spatial_factor=2,
              resolution_factor=1, core_factor=2, auto_sampling=True):
    """dict(acf, acf_efield, fn, tn, snp, snp2, field [nsn, ndnun] complex, scale [ndnun], dnun)."""
    if nf % 2 == 0:
        nf += 1
    nt, sp_fac, res_fac, core_fac0, dsp = sampling(taumax, nt, ar, spatial_factor, resolution_factor, core_factor, auto_sampling)
    alph2 = alpha / 2
    xi = 90 - psi
    Vx, Vy = np.cos(xi * np.pi / 180), np.sin(xi * np.pi / 180)
    sigxn = phasegrad * np.cos((xi - theta) * np.pi / 180)
    sigyn = phasegrad * np.sin((xi - theta) * np.pi / 180)
    sqrtar = np.sqrt(ar)
    dnun = np.linspace(0, dnumax, int(np.ceil(nf / 2)))
    ndnun = len(dnun)
    core_fac = res_fac * core_fac0
    snp = np.arange(-sp_fac * taumax, sp_fac * taumax + dsp / res_fac, dsp / res_fac)
    snp2 = np.arange(-sp_fac * taumax, sp_fac * taumax + dsp / core_fac, dsp / core_fac)
    X, Y, G = efield_plane(snp, sqrtar, alph2)
    X2, Y2, G2 = efield_plane(snp2, sqrtar, alph2)
    shifted = phasegrad != 0
    if shifted:
        tn = np.linspace(-taumax, taumax, nt)
    else:
        tn = np.linspace(0, taumax, int(np.ceil(nt / 2)))
    snx, sny = Vx * tn, Vy * tn
    field = np.zeros((len(snx), ndnun), dtype=np.complex128)
    field[:, 0] = np.exp(-0.5 * ((snx / sqrtar)**2 + (sny * sqrtar)**2)**alph2)
    if shifted:
        field[np.argwhere(snx == 0), 0] += wn / amp
    else:
        field[0, 0] += wn / amp
    scale = np.zeros(ndnun)
    for idn in range(1, ndnun):
        gx, gy, g, step = (X2, Y2, G2, dsp / core_fac) if idn == 1 else (X, Y, G, dsp / res_fac)
        cx = snx - 2 * sigxn * dnun[idn] if shifted else snx
        cy = sny - 2 * sigyn * dnun[idn] if shifted else sny
        scale[idn] = step**2 * np.sum(g) / ((2 * np.pi) * dnun[idn])
        for isn in range(len(snx)):
            arg = ((gx - cx[isn])**2 + (gy - cy[isn])**2) / (2 * dnun[idn])
            field[isn, idn] = -1j * (step**2 * np.sum(g * np.exp(1j * arg)) / ((2 * np.pi) * dnun[idn]))
    inten = np.real(field * np.conj(field))
    nr, nc = inten.shape
    fn = np.concatenate((np.flip(-dnun[1:]), dnun)).squeeze()
    if shifted:
        full = np.zeros((nr, nc * 2 - 1))
        full[:, 0:nc - 1] = np.fliplr(np.flipud(inten[:, 1:]))
        full[:, nc - 1:] = inten
        t2 = tn
    else:
        half = np.zeros((nr, nc * 2 - 1))
        half[:, 0:nc - 1] = np.fliplr(inten[:, 1:])
        half[:, nc - 1:] = inten
        full = np.zeros((nr * 2 - 1, nc * 2 - 1))
        full[0:nr - 1, :] = np.flipud(half[1:, :])
        full[nr - 1:, :] = half
        t2 = np.concatenate((np.flip(-tn[1:]), tn)).squeeze()
    return dict(acf=amp * np.transpose(full), acf_efield=G, fn=fn, tn=t2, snp=snp, snp2=snp2, field=field, scale=scale, dnun=dnun)


def scint_acf_model_2d(parvals, ydata, weights, acf):
    """The residual's arithmetic (scint_models.py:164-215) around a given model array `acf` [nf_crop, nt_crop]."""
    tau, dnu = np.abs(parvals['tau']), np.abs(parvals['dnu'])
    tobs, bw, nt, nf = parvals['tobs'], parvals['bw'], parvals['nt'], parvals['nf']
    nf_crop, nt_crop = np.shape(ydata)
    dt, df = 2 * tobs / nt, 2 * bw / nf
    taumax, dnumax = nt_crop * dt / tau, nf_crop * df / dnu
    tri_t = 1 - np.divide(np.tile(np.abs(np.linspace(-taumax * tau, taumax * tau, nt_crop)), (nf_crop, 1)), tobs)
    tri_f = np.transpose(1 - np.divide(np.tile(np.abs(np.linspace(-dnumax * dnu, dnumax * dnu, nf_crop)), (nt_crop, 1)), bw))
    triangle = np.multiply(tri_t, tri_f)
    model = np.multiply(acf, triangle)
    if weights is None:
        weights = np.ones(np.shape(ydata))
    weights = np.fft.fftshift(weights)
    weights[-1, -1] = 0
    weights = np.fft.ifftshift(weights)
    return (ydata - model) * weights, triangle, weights, dict(taumax=taumax, dnumax=dnumax)
