"""The checks of the fitted mosaics, shared by the GPU tests (tests/test_gpu_rotmos.py) and the host-interpreter tests
(tests/test_rotmos_emu_cpu.py): `T` is scintools_amd.ththmod bound to a GPU or to the interpreter.  The oracle's results are
computed once per case and shared.

Tolerance of every sum: 1e-13 * S, S the sum of the summands' absolute values (tests/rotmos_oracle.py).  Derived, not measured:
two tree summations of up to 2^20 terms each err by at most about (log2 n + a few) * eps * S; with a dozen roundings per summand
that is about 1e-14 * S, and the tolerance is ten times that.  Only where S itself has fallen to rounding level (tapers of
length 1: whole summands cancel) a rounding floor is added: rotmos_cases.close_in_scale, rotmos_oracle's docstring."""
import functools

import numpy as np

import rotmos_cases as rc
import rotmos_oracle as ro

TOL_SUM = 1e-13
FD_STEP, TOL_FD = 1e-6, 1e-5


@functools.lru_cache(maxsize=None)
def _case(shape, seed, noise, nans):
    c = rc.case(shape, seed=seed, noise=noise, nans=nans)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def case(shape, seed=0, noise=0.1, nans=False):
    return _case(tuple(shape), seed, noise, nans)


@functools.lru_cache(maxsize=None)
def oracle_at(shape, seed, nans, point):
    """Every oracle output of the case at its random x / p ('r') or at rotInit with amplitudes 1 ('i')."""
    c = case(shape, seed, 0.1, nans)
    ch, d, N = c["chunks"], c["dspec"], c["N"]
    n = shape[0] * shape[1]
    xi = ro.rot_init(ch)
    x, p = (c["x"], c["p"]) if point == "r" else (xi, np.concatenate((xi, np.ones(n))))
    with np.errstate(all="ignore"):
        out = dict(x=x, p=p, rotInit=xi, rotMos=ro.rot_mosaic(ch, x), rotFit=ro.rot_fit(x, ch), rotDer=ro.rot_der(x, ch),
                   fullMos=ro.full_mosaic(ch, p), fullMosFit=ro.full_fit(p, ch, d, N), fullMosGrad=ro.full_grad(p, ch, d, N),
                   fullMosHess=ro.full_hess(p, ch, d, N))
    return out


def check_mosaics_and_init(T, shape, seed=0, gold=None):
    """rotMos / fullMos equal the oracle's loops bit for bit on this host (when its NumPy's products are understood); rotInit
    is the oracle's, and rotMos at rotInit is the greedy mosaic_device."""
    c, o = case(shape, seed), oracle_at(tuple(shape), seed, False, "r")
    stack = T.MosaicStack(c["chunks"])
    got_r, got_f = T.rotMos(stack, c["x"]), T.fullMos(stack, c["p"])
    assert isinstance(got_r, np.ndarray) and got_r.dtype == np.complex128 and got_r.shape == rc.extent(shape)
    if T._numpy_mosaic_modes(shape[2], shape[3]) is not None:
        assert np.array_equal(got_r, o["rotMos"]) and np.array_equal(got_f, o["fullMos"])
    else:
        assert np.abs(got_r - o["rotMos"]).max() <= 1e-14 * np.abs(o["rotMos"]).max()
        assert np.abs(got_f - o["fullMos"]).max() <= 1e-14 * np.abs(o["fullMos"]).max()
    if gold is not None:                       # the reference's own mosaics came from another host's NumPy: to rounding
        for got, ref in ((got_r, gold[rc.name_of(shape) + "_r_rotMos"]), (got_f, gold[rc.name_of(shape) + "_r_fullMos"])):
            assert np.abs(got - ref).max() <= 1e-14 * np.abs(ref).max()
    xi = T.rotInit(stack)
    assert xi.shape == (shape[0] * shape[1] - 1,)
    if T._numpy_mosaic_modes(shape[2], shape[3]) is not None:
        assert np.array_equal(xi, o["rotInit"])
    greedy = T.mosaic_device(stack.chunks_t).cpu().numpy()
    assert np.array_equal(T.rotMos(stack, xi), greedy)
    assert np.array_equal(T.rotMos(c["chunks"], c["x"]), got_r)           # a NumPy stack, uploaded by the call


def device_sums(T, c, x, p):
    stack = T.MosaicStack(c["chunks"], c["dspec"], c["N"])
    return dict(rotFit=T.rotFit(x, stack), rotDer=T.rotDer(x, stack), fullMosFit=T.fullMosFit(p, stack, None, None),
                fullMosGrad=T.fullMosGrad(p, stack, None, None), fullMosHess=T.fullMosHess(p, stack, None, None))


def check_sums(T, shape, seed=0, nans=False, gold=None, gold_name=None):
    """Every sum within TOL_SUM * S of the oracle (and of the reference's stored outputs); the Hessian's NaN pattern, symmetry
    and band."""
    c = case(shape, seed, 0.1, nans)
    worst = {}
    for point in ("r", "i"):
        o = oracle_at(tuple(shape), seed, nans, point)
        got = device_sums(T, c, o["x"], o["p"])
        for k, v in got.items():
            want, S, P = o[k]
            assert np.shape(v) == np.shape(want), k
            worst[k + "_" + point] = rc.close_in_scale(v, want, S, TOL_SUM, P)
            if gold is not None:
                worst[k + "_" + point + "_ref"] = rc.close_in_scale(v, gold[f"{gold_name}_{point}_{k}"], S, TOL_SUM, P)
        H = got["fullMosHess"]
        assert np.array_equal(np.isnan(H), np.isnan(o["fullMosHess"][0]))
        assert np.array_equal(H, H.T, equal_nan=True)
        assert not H[~rc.neighbour_band(shape)].any()
    print(shape, "nans" if nans else "", {k: f"{v:.1e}" for k, v in worst.items()})
    return worst


def check_derivatives(T, shape, seed=0):
    """Central differences of the device objective against the device gradient, and of the device gradient against the device
    Hessian's columns."""
    c = case(shape, seed)
    stack = T.MosaicStack(c["chunks"], c["dspec"], c["N"])
    n = shape[0] * shape[1]

    def central(f, v, k):
        e = np.zeros(v.size)
        e[k] = FD_STEP
        return (f(v + e) - f(v - e)) / (2 * FD_STEP)
    # A central difference cannot resolve less than its own rounding: the differenced function carries about eps of its size,
    # so the quotient about eps * |f| / h (2e-10 |f| here).  Where the criterion's 1e-5 of the largest entry lies below that
    # floor -- tapers of length 1 make the objective independent of the phases: the gradient is exactly 0 and the Hessian's
    # phase columns are rounding noise -- the floor (with a factor 4) is what the comparison can ask.  Everywhere else the
    # tolerance is the criterion's own: the larger of the two is taken, they are not added.
    eps = np.finfo(float).eps

    def agree(fd, exact, size):
        err, tol = np.abs(fd - exact).max(initial=0.0), max(TOL_FD * np.abs(exact).max(initial=0.0), 4 * eps * size / FD_STEP)
        assert err <= tol, (err, tol)
        big = np.abs(exact).max(initial=0.0)
        return err / big if TOL_FD * big > 4 * eps * size / FD_STEP else 0.0      # (reported where the criterion is the binding one)
    if n > 1:
        f0, g = stack.rot_value_and_grad(c["x"])
        fd = np.array([central(lambda v: stack.rot_value_and_grad(v)[0], c["x"], k) for k in range(n - 1)])
        print(shape, "rot   fd", agree(fd, g, abs(f0)))
    f0, g = stack.full_value_and_grad(c["p"])
    fd = np.array([central(lambda v: stack.full_value_and_grad(v)[0], c["p"], k) for k in range(2 * n - 1)])
    print(shape, "full  fd", agree(fd, g, abs(f0)))
    H = stack.full_hess(c["p"])
    worst = 0.0
    for k in range(2 * n - 1):
        col = central(lambda v: stack.full_value_and_grad(v)[1], c["p"], k)
        worst = max(worst, agree(col, H[:, k], np.abs(g).max()))
    print(shape, "hess  fd", worst)


def check_deterministic(T, shape):
    c = case(shape)
    stack = T.MosaicStack(c["chunks"], c["dspec"], c["N"])
    a, b = (stack.rot_value_and_grad(c["x"]), stack.rot_value_and_grad(c["x"]))
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    a, b = (stack.full_value_and_grad(c["p"]), stack.full_value_and_grad(c["p"]))
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    assert np.array_equal(stack.full_hess(c["p"]), stack.full_hess(c["p"]))
    assert np.array_equal(stack.full_mosaic(c["p"]), stack.full_mosaic(c["p"]))


def check_errors(T, pytest):
    c = case((2, 3, 34, 50))
    with pytest.raises(ValueError):
        T.MosaicStack(np.zeros((2, 1, 5, 4), dtype=complex))                   # odd along an axis of several chunks
    with pytest.raises(ValueError):
        T.rotMos(np.zeros((1, 2, 4, 5), dtype=complex), np.zeros(1))
    T.MosaicStack(np.zeros((1, 2, 5, 4), dtype=complex))                        # odd along an axis of one: fine
    F, T_ = rc.extent((2, 3, 34, 50))
    big_d, big_N = np.pad(c["dspec"], ((0, 2), (0, 3)), constant_values=1.0), np.pad(c["N"], ((0, 2), (0, 3)), constant_values=1.0)
    stack = T.MosaicStack(c["chunks"])
    # fullMosFit crops dspec and N to the mosaic ...
    assert T.fullMosFit(c["p"], stack, big_d, big_N) == T.fullMosFit(c["p"], stack, c["dspec"], c["N"])
    # ... fullMosGrad and fullMosHess do not
    for fn in (T.fullMosGrad, T.fullMosHess):
        with pytest.raises(ValueError):
            fn(c["p"], stack, big_d, big_N)
        with pytest.raises(ValueError):
            fn(c["p"], stack, c["dspec"][:-1], c["N"][:-1])
    with pytest.raises(ValueError):
        T.fullMosFit(c["p"], stack, c["dspec"][:-1], c["N"])
    with pytest.raises(ValueError):
        stack.full_value_and_grad(c["p"])                                      # no dspec / N at all
    with pytest.raises(ValueError):
        T.fit_mosaic(stack, mode="neither")


def check_driver(T, mode, seed):
    """fit_mosaic against the same SciPy call on the oracle's own functions, judged by the oracle's objective."""
    from scipy.optimize import minimize
    shape = rc.DRIVER_SHAPE
    c = case(shape, seed, 0.5)
    ch, d, N = c["chunks"], c["dspec"], c["N"]
    n = shape[0] * shape[1]
    x0 = ro.rot_init(ch)
    if mode == "rot":
        f = lambda v: ro.rot_fit(v, ch)[0]                                     # noqa: E731
        g = lambda v: ro.rot_der(v, ch)[0]                                     # noqa: E731
        ref = minimize(f, x0, jac=g, method="L-BFGS-B")
        stack = T.MosaicStack(ch)
    else:
        x0 = np.concatenate((x0, np.ones(n)))
        f = lambda v: ro.full_fit(v, ch, d, N)[0]                              # noqa: E731
        g = lambda v: ro.full_grad(v, ch, d, N)[0]                             # noqa: E731
        ref = minimize(f, x0, jac=g, hess=lambda v: ro.full_hess(v, ch, d, N)[0], method="Newton-CG")
        stack = T.MosaicStack(ch, d, N)
    wf, params, res = T.fit_mosaic(stack, mode=mode)
    assert wf.shape == rc.extent(shape) and params.shape == x0.shape
    gain_ref, gain = f(x0) - f(ref.x), f(x0) - f(params)
    g0, g1 = np.abs(g(x0)).max(), np.abs(g(params)).max()
    print(mode, seed, "start", f(x0), "oracle", f(ref.x), ref.nit, "device", f(params), res.nit, "gradient", g0, "->", g1)
    assert gain_ref > 0 and gain >= 0.9 * gain_ref
    assert g1 <= g0 / 10
    assert np.array_equal(wf, (T.rotMos(stack, params) if mode == "rot" else T.fullMos(stack, params)))
