"""The fitted mosaics on the GPU: rotMos / rotFit / rotDer / rotInit, fullMos / fullMosFit / fullMosGrad / fullMosHess,
MosaicStack, fit_mosaic and Dynspec.refine_wavefield against the oracle (tests/rotmos_oracle.py) and the reference's stored
outputs (tests/golden/rotmos.npz).  The checks and their tolerances are in tests/rotmos_checks.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rotmos_cases as rc  # noqa: E402
import rotmos_checks as ck  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    from scintools_amd import ththmod
    from scintools_amd.device import require_gpu
    require_gpu()
    return ththmod


@pytest.fixture(scope="module")
def gold(golden):
    return golden("rotmos.npz")


@pytest.mark.parametrize("shape", rc.SHAPES)
def test_mosaics_equal_the_host_loops_bit_for_bit_and_rotinit_is_the_greedy_mosaic(T, gold, shape):
    ck.check_mosaics_and_init(T, shape, gold=gold if shape in rc.GOLDEN_SHAPES else None)


@pytest.mark.parametrize("shape", rc.SHAPES)
def test_every_sum_within_1e13_of_its_scale(T, gold, shape):
    stored = shape in rc.GOLDEN_SHAPES
    ck.check_sums(T, shape, gold=gold if stored else None, gold_name=rc.name_of(shape))


def test_sums_and_hessian_pattern_with_nans_and_a_zero_noise(T, gold):
    ck.check_sums(T, (3, 3, 8, 12), seed=1, nans=True, gold=gold, gold_name="nan3x3")


@pytest.mark.parametrize("shape", rc.SHAPES)
def test_central_differences_agree_with_gradient_and_hessian(T, shape):
    ck.check_derivatives(T, shape)


@pytest.mark.parametrize("shape", [(3, 3, 8, 12), (2, 3, 34, 50), (5, 5, 32, 32)])
def test_two_calls_return_equal_bits(T, shape):
    ck.check_deterministic(T, shape)


def test_shape_errors(T):
    ck.check_errors(T, pytest)


def test_wavefield_stays_on_the_device_when_asked(T):
    import torch
    c = ck.case((3, 3, 8, 12))
    stack = T.MosaicStack(c["chunks"])
    w, params, _ = T.fit_mosaic(stack, mode="rot", out_device=True, options={"maxiter": 2})
    assert isinstance(w, torch.Tensor) and w.is_cuda and np.array_equal(w.cpu().numpy(), T.rotMos(stack, params))
    on_dev = T.MosaicStack(torch.from_numpy(c["chunks"].copy()).cuda())
    assert np.array_equal(on_dev.full_mosaic(c["p"]), T.fullMos(c["chunks"], c["p"]))


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("mode", ["rot", "full"])
def test_fit_mosaic_reaches_the_oracles_optimum(T, mode, seed):
    ck.check_driver(T, mode, seed)


def test_refine_wavefield_is_no_less_coherent_than_the_greedy_mosaic(T, golden):
    from scintools_amd.dynspec import Dynspec
    g, f = golden("retrieval.npz"), golden("fit_thetatheta.npz")
    n = int(g["nchan"])

    class B:
        dyn, freqs, times, dt, df = f["dspec"][:n], f["freq"][:n], f["time"], float(f["dt"]), float(f["df"])
    d = Dynspec(dyn=B(), verbose=False)
    d.prep_thetatheta(cwf=64, edges_lim=.3, eta_min=30, eta_max=50, nedge=128)
    d.calc_wavefield()
    greedy = -np.sum(np.abs(d.wavefield) ** 2)
    chunks = d.chunks.copy()
    d.refine_wavefield("rot")
    refined = -np.sum(np.abs(d.wavefield) ** 2)
    print("greedy", greedy, "refined", refined, "iterations", d.mosaic_result.nit)
    assert d.wavefield.shape == rc.extent(chunks.shape)
    assert d.mosaic_params.shape == (chunks.shape[0] * chunks.shape[1] - 1,)
    assert refined <= greedy
    assert np.array_equal(d.wavefield, T.rotMos(chunks, d.mosaic_params))
