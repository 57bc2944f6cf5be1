"""The NumPy oracle of the multi-station retrieval (tests/vlbi_oracle.py) against the reference's own outputs
(tests/golden/vlbi.npz, written by tests/golden/make_golden_vlbi.py) -- runs without a GPU and without the package's library."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vlbi_cases as vc  # noqa: E402
import vlbi_oracle as vo  # noqa: E402

TOL = 1e-9     # of the peak: the project's figure for retrieval parity (tests/test_gpu_retrieval.py)


@pytest.fixture(scope="module")
def gold(golden):
    return golden("vlbi.npz")


def _inputs(gold, name):
    npad, n_dish = (int(v) for v in gold[f"{name}_par"])
    nspec = n_dish * (n_dish + 1) // 2
    dlist = [gold[f"{name}_in{i}"] for i in range(nspec)]
    return dlist, gold[f"{name}_edges"], gold[f"{name}_time"], gold[f"{name}_freq"], float(gold[f"{name}_eta"]), npad, n_dish, \
        float(gold[f"{name}_tauMask"])


@pytest.mark.parametrize("name", list(vc.GOLDEN))
def test_generator_reproduces_golden_inputs(gold, name):
    c = vc.golden_case(name)
    dlist = _inputs(gold, name)[0]
    for a, b in zip(c["dlist"], dlist):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", list(vc.GOLDEN))
def test_oracle_blocks_equal_reference(gold, name):
    dlist, edges, time, freq, eta, npad, n_dish, mask = _inputs(gold, name)
    reds, flags, edges_red, _, _ = vo.reduced_maps(dlist, edges, time, freq, eta, npad, n_dish, mask)
    for i, (red, flag) in enumerate(zip(reds, flags)):
        ref = gold[f"{name}_red{i}"]
        assert flag == bool(gold[f"{name}_herm{i}"])
        assert red.shape == ref.shape
        assert int((red != ref).sum()) == 0
    assert np.array_equal(edges_red, gold[f"{name}_edges_red"])
    # the flags: the dynamic spectra (station pair (d, d)) are the Hermitian ones
    assert [i for i, f in enumerate(flags) if f] == [vo.spectrum_index(n_dish, d, 0) for d in range(n_dish)]


@pytest.mark.parametrize("name", list(vc.GOLDEN))
def test_oracle_model_equals_reference(gold, name):
    dlist, edges, time, freq, eta, npad, n_dish, mask = _inputs(gold, name)
    got = vo.vlbi_chunk_retrieval(dlist, edges, time, freq, eta, npad, n_dish, mask)
    ref = gold[f"{name}_model_E"]
    err = vc.rel_err(vc.align_joint(got, ref), ref)
    print(name, "oracle vs reference:", err)
    assert err <= TOL


def test_one_station_is_single_chunk_retrieval(gold):
    from oracle import thth_oracle as to
    dlist, edges, time, freq, eta, npad, n_dish, mask = _inputs(gold, "n1")
    got = vo.vlbi_chunk_retrieval(dlist, edges, time, freq, eta, npad, 1, mask)
    ref = to.single_chunk_retrieval(dlist[0], edges, time, freq, eta, npad, mask)
    err = vc.rel_err(vc.align_joint(got, ref[None]), ref[None])
    print("n_dish = 1 vs single_chunk_retrieval:", err)
    assert err <= TOL


def test_reference_raises_on_a_crop_of_one_centre(gold):
    assert str(gold["small_crop_raises"]) == "IndexError"


def test_fuzz_cases_complete_in_the_oracle():
    """Every fuzz geometry of tests/test_gpu_vlbi.py goes through the oracle (none may be skipped there), covers the promised
    ranges, and recovers the injected station phases up to the one common phase."""
    cases = vc.fuzz_cases()
    assert len(cases) >= 20
    assert {c["npad"] for c in cases} == {0, 1, 3} and {c["n_dish"] for c in cases} == {1, 2, 3, 4}
    shapes = [np.asarray(c["dlist"][0]).shape for c in cases]
    assert any(s[0] % 2 for s in shapes) and any(not s[0] % 2 for s in shapes)
    cpb = np.array([vc.fuzz_centres_per_bin(c) for c in cases])
    print("centres per Doppler bin:", np.round(np.sort(cpb), 2))
    assert cpb.min() <= 0.5 and cpb.max() >= 30 and (cpb >= 10).sum() >= 8       # sparse to dense, as retrieval_cases' fuzz
    for c in cases:
        out = vo.vlbi_chunk_retrieval(c["dlist"], c["edges"], c["time"], c["freq"], c["eta"], c["npad"], c["n_dish"], c["tauMask"])
        assert np.isfinite(out).all() and np.abs(out).max() > 0, c["id"]
