"""The multi-station (VLBI) phase retrieval on an MI355X: ththmod.VLBI_chunk_retrieval / vlbi_retrieval_batch against the
reference's outputs (tests/golden/vlbi.npz) and the oracle (tests/vlbi_oracle.py).  Reads only tests/golden and the repository."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vlbi_cases as vc  # noqa: E402
import vlbi_oracle as vo  # noqa: E402

_case, _chunk, _params, check_composite = vc.stored_case, vc.chunk_of, vc.params_of, vc.check_composite

pytestmark = pytest.mark.gpu
TOL = 1e-9        # retrieval parity, of the peak (tests/test_gpu_retrieval.py)
FUZZ = vc.fuzz_cases()


@pytest.fixture(scope="module")
def thth():
    from scintools_amd import ththmod
    from scintools_amd.device import require_gpu
    require_gpu()
    return ththmod


@pytest.fixture(scope="module")
def gold(golden):
    return golden("vlbi.npz")


@pytest.mark.parametrize("name", list(vc.GOLDEN))
def test_composite_blocks_equal_reference(thth, gold, name):
    check_composite(thth, gold, name)


@pytest.mark.parametrize("name", list(vc.GOLDEN))
def test_retrieval_vs_reference_and_oracle(thth, gold, name):
    c = _case(gold, name)
    model_E, idx_f, idx_t = thth.VLBI_chunk_retrieval(_params(c))
    assert (idx_f, idx_t) == (5, 3) and len(model_E) == c["n_dish"]
    got = np.array(model_E)
    ref = gold[f"{name}_model_E"]
    orc = vo.vlbi_chunk_retrieval(c["dlist"], c["edges"], c["time"], c["freq"], c["eta"], c["npad"], c["n_dish"], c["tauMask"])
    e_ref, e_orc = vc.rel_err(vc.align_joint(got, ref), ref), vc.rel_err(vc.align_joint(got, orc), orc)
    e_first = vc.rel_err(vc.align_on_first(got, ref), ref)      # the phases BETWEEN stations
    print(name, "vs reference", e_ref, "vs oracle", e_orc, "aligned on station 1", e_first)
    assert e_ref <= TOL and e_orc <= TOL and e_first <= TOL


@pytest.mark.parametrize("c", FUZZ, ids=[c["id"] for c in FUZZ])
def test_fuzz_vs_oracle(thth, c):
    got = np.array(thth.VLBI_chunk_retrieval(_params(c))[0])
    orc = vo.vlbi_chunk_retrieval(c["dlist"], c["edges"], c["time"], c["freq"], c["eta"], c["npad"], c["n_dish"], c["tauMask"])
    err = vc.rel_err(vc.align_joint(got, orc), orc)
    print(c["id"], "vs oracle", err)
    assert err <= TOL


def test_fuzz_has_twenty_cases():
    assert len(FUZZ) >= 20


def test_one_station_is_single_chunk_retrieval(thth, gold):
    c = _case(gold, "n1")
    got = np.array(thth.VLBI_chunk_retrieval(_params(c))[0])
    one = thth.single_chunk_retrieval((c["dlist"][0], c["edges"], c["time"], c["freq"], c["eta"], 0, 0, c["npad"], c["tauMask"], False))[0]
    assert np.abs(one).max() > 0
    err = vc.rel_err(vc.align_joint(got, one[None]), one[None])
    print("n_dish = 1 vs single_chunk_retrieval", err)
    assert err <= TOL


def test_groups_and_out_device(thth):
    """A batch that spans several `group_bytes` groups gives the same chunks as one group; out_device returns the same values."""
    cs = [vc.case(32, 24, 1, 3, 30, f, 70 + k) for k, f in enumerate((0.6, 0.9, 1.2, 1.5, 1.9))]
    chunks = [_chunk(c) for c in cs]
    i1, i2 = {}, {}
    one = thth.vlbi_retrieval_batch(chunks, 1, 3, 0.0, info=i1)
    per_chunk = 16 * 6 * 64 * 48
    many = thth.vlbi_retrieval_batch(chunks, 1, 3, 0.0, group_bytes=2 * per_chunk, info=i2)
    assert i1["groups"] == 1 and i2["groups"] > 1
    assert one.shape == (5, 3, 32, 24) and np.array_equal(one, many)
    dev = thth.vlbi_retrieval_batch(chunks, 1, 3, 0.0, out_device=True)
    assert hasattr(dev, "device") and np.array_equal(dev.cpu().numpy(), one)
    for k, c in enumerate(cs):
        orc = vo.vlbi_chunk_retrieval(c["dlist"], c["edges"], c["time"], c["freq"], c["eta"], 1, 3, 0.0)
        assert vc.rel_err(vc.align_joint(one[k], orc), orc) <= TOL


def test_crop_of_one_centre_raises_like_the_reference(thth, gold):
    c = _case(gold, "n2")
    bad = dict(c, eta=c["eta"] * float(gold["small_crop_eta_factor"]))
    with pytest.raises(IndexError):
        thth.VLBI_chunk_retrieval(_params(bad))


def test_edges_wider_than_the_doppler_span_raise_like_the_reference(thth, gold):
    assert str(gold["wide_raises"]) == "IndexError"
    with pytest.raises(IndexError):
        thth.VLBI_chunk_retrieval(_params(vc.wide_case()))
