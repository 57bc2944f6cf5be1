"""The NumPy oracle of the fitted mosaics (tests/rotmos_oracle.py) against the reference's stored outputs
(tests/golden/rotmos.npz, written by tests/golden/make_golden_rotmos.py), and the stored inputs against the seeded generator
(tests/rotmos_cases.py).  Runs without a GPU."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rotmos_cases as rc  # noqa: E402
import rotmos_checks as ck  # noqa: E402

CASES = [(rc.name_of(s), s, 0, False) for s in rc.GOLDEN_SHAPES] + [("nan3x3", (3, 3, 8, 12), 1, True)]


@pytest.fixture(scope="module")
def gold(golden):
    return golden("rotmos.npz")


@pytest.mark.parametrize("name,shape,seed,nans", CASES)
def test_stored_inputs_are_the_generators(gold, name, shape, seed, nans):
    c = ck.case(shape, seed, 0.1, nans)
    for k in ("chunks", "dspec", "N", "x", "p"):
        assert np.array_equal(gold[f"{name}_{k}"], c[k], equal_nan=True), k


@pytest.mark.parametrize("name,shape,seed,nans", CASES)
def test_oracle_vs_reference(gold, name, shape, seed, nans):
    """The mosaics and rotInit to rounding (the goldens came from another host's NumPy, whose complex products may round
    differently); every sum within 1e-13 of its scale (plus the rounding floor where the scale itself is rounding noise); the Hessian's NaN pattern, symmetry and band exactly."""
    for point in ("r", "i"):
        o = ck.oracle_at(tuple(shape), seed, nans, point)
        assert np.abs(o["rotInit"] - gold[f"{name}_rotInit"]).max(initial=0.0) <= 1e-12
        if point == "r":
            for k in ("rotMos", "fullMos"):
                ref = gold[f"{name}_r_{k}"]
                assert np.abs(o[k] - ref).max() <= 1e-14 * np.abs(ref).max()
        for k in ("rotFit", "rotDer", "fullMosFit", "fullMosGrad", "fullMosHess"):
            # at 'i' the oracle's own rotInit is the point: it may differ from the reference's in the last bits, which moves a
            # sum by about (its gradient) x 1e-16 -- far inside the tolerance
            rc.close_in_scale(o[k][0], gold[f"{name}_{point}_{k}"], o[k][1], ck.TOL_SUM, o[k][2])
        H = o["fullMosHess"][0]
        ref = gold[f"{name}_{point}_fullMosHess"]
        assert np.array_equal(np.isnan(H), np.isnan(ref)) and np.array_equal(H, H.T, equal_nan=True)
        assert np.array_equal(ref, ref.T, equal_nan=True) and not ref[~rc.neighbour_band(shape)].any()
        assert not H[~rc.neighbour_band(shape)].any()


def test_the_nan_case_has_its_nans(gold):
    assert np.isnan(gold["nan3x3_dspec"]).sum() == 3 and np.isnan(gold["nan3x3_N"]).sum() == 1 and (gold["nan3x3_N"] == 0).sum() == 1
    assert np.isnan(gold["nan3x3_r_fullMosHess"]).any()


def test_reference_timing_is_recorded():
    with open(os.path.join(HERE, "golden", "rotmos_timing.json")) as fh:
        t = json.load(fh)
    assert t["tutorial"]["chunks"] == 256 and t["tutorial"]["shape"][2:] == [64, 64]
    assert t["headline_one_sample"]["chunks"] == 961 and t["headline_one_sample"]["shape"][2:] == [256, 256]
    for k in ("rotFit", "rotDer", "fullMosGrad", "fullMosHess"):
        assert t["tutorial"][k] > 0 and t["headline_one_sample"][k] > 0
