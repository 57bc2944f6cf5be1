"""The multi-station (VLBI) retrieval -- scint_cs_complex_batch, scint_vlbi_composite, scint_eigh_top_batch and the shared
retrieval tail -- interpreted on the host (tests/emu) through the same C ABI and Python wrappers as on a GPU, against the
reference's outputs (tests/golden/vlbi.npz) and the oracle (tests/vlbi_oracle.py).  Runs without a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)
import vlbi_cases as vc  # noqa: E402
import vlbi_oracle as vo  # noqa: E402

TOL = 1e-9        # retrieval parity, of the peak (tests/test_gpu_retrieval.py)
TOL_FFT = 1e-12   # the transforms, of the peak (the retrieval-tail tests' figure)


@pytest.fixture()
def emu(monkeypatch):
    import emulated
    emulated.install(monkeypatch)
    from scintools_amd import ththmod
    return ththmod


@pytest.fixture(scope="module")
def gold(golden):
    return golden("vlbi.npz")


_case, _chunk, _params, check_composite = vc.stored_case, vc.chunk_of, vc.params_of, vc.check_composite


def test_symbols_exist(emu):
    assert callable(emu.VLBI_chunk_retrieval) and callable(emu.vlbi_retrieval_batch)


@pytest.mark.parametrize("name", list(vc.GOLDEN))
def test_composite_blocks_equal_reference(emu, gold, name):
    c, comp = check_composite(emu, gold, name)
    # and the composite the whole device path forms (its own transforms feed the gather): the same matrix to the transforms' rounding
    info = {}
    emu.vlbi_retrieval_batch([_chunk(c)], c["npad"], c["n_dish"], c["tauMask"], info=info)
    assert info["composites"][0].shape == comp.shape
    assert np.abs(info["composites"][0] - comp).max() <= TOL_FFT * np.abs(comp).max()


@pytest.mark.parametrize("nf,nt,npad,lo,hi", [(16, 16, 1, 14, 19), (12, 20, 0, 0, 0), (9, 7, 3, 16, 21), (8, 16, 3, 0, 0)])
def test_complex_zero_padded_conjugate_spectrum(emu, nf, nt, npad, lo, hi):
    import torch
    from scintools_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(nf * 100 + nt)
    n = 3
    x = rng.standard_normal((n, nf, nt)) + 1j * rng.standard_normal((n, nf, nt))
    R, C = (npad + 1) * nf, (npad + 1) * nt
    x_t = torch.from_numpy(x.copy())
    out_t = torch.full((n, R, C), complex(np.nan, np.nan), dtype=torch.complex128)
    need = ctypes.c_size_t()
    assert lib.scint_cs_workspace_bytes(nf, nt, npad, ctypes.byref(need)) == 0
    ws = torch.empty(need.value, dtype=torch.uint8)
    lohi = np.ascontiguousarray([[lo, hi]] * n, dtype=np.int64)
    rc = lib.scint_cs_complex_batch(x_t.data_ptr(), n, nf, nt, npad, lohi.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                    out_t.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert rc == 0
    got = out_t.numpy()
    for k in range(n):
        ref = np.fft.fftshift(np.fft.fft2(np.pad(x[k], ((0, npad * nf), (0, npad * nt)), mode="constant", constant_values=0)))
        assert not got[k, lo:hi].any() and not np.signbit(got[k, lo:hi].real).any() and not np.signbit(got[k, lo:hi].imag).any()
        ref[lo:hi] = 0
        err = np.abs(got[k] - ref).max() / np.abs(ref).max()
        print("complex CS", (nf, nt, npad), err)
        assert err <= TOL_FFT


@pytest.mark.parametrize("name", list(vc.GOLDEN))
def test_retrieval_vs_reference_and_oracle(emu, gold, name):
    c = _case(gold, name)
    model_E, idx_f, idx_t = emu.VLBI_chunk_retrieval(_params(c))
    assert (idx_f, idx_t) == (5, 3) and isinstance(model_E, list) and len(model_E) == c["n_dish"]
    got = np.array(model_E)
    ref = gold[f"{name}_model_E"]
    orc = vo.vlbi_chunk_retrieval(c["dlist"], c["edges"], c["time"], c["freq"], c["eta"], c["npad"], c["n_dish"], c["tauMask"])
    e_ref, e_orc = vc.rel_err(vc.align_joint(got, ref), ref), vc.rel_err(vc.align_joint(got, orc), orc)
    # the phases BETWEEN stations: aligned on station 1 alone, the others must still agree
    e_first = vc.rel_err(vc.align_on_first(got, ref), ref)
    print(name, "vs reference", e_ref, "vs oracle", e_orc, "aligned on station 1", e_first)
    assert e_ref <= TOL and e_orc <= TOL and e_first <= TOL


def test_one_station_is_single_chunk_retrieval(emu, gold):
    c = _case(gold, "n1")
    got = np.array(emu.VLBI_chunk_retrieval(_params(c))[0])
    one = emu.single_chunk_retrieval((c["dlist"][0], c["edges"], c["time"], c["freq"], c["eta"], 0, 0, c["npad"], c["tauMask"], False))[0]
    err = vc.rel_err(vc.align_joint(got, one[None]), one[None])
    print("n_dish = 1 vs single_chunk_retrieval", err)
    assert err <= TOL


def test_batch_equals_single_calls(emu):
    """Chunks of one shape with different curvatures (one of them cropping the grid) in one batch, in one group and in groups of
    one: the same chunks as the one-chunk calls."""
    cs = [vc.case(24, 20, 1, 2, 28, f, 40 + k) for k, f in enumerate((0.7, 1.0, 1.6))]
    chunks = [_chunk(c) for c in cs]
    info = {}
    both = emu.vlbi_retrieval_batch(chunks, 1, 2, 0.0, info=info)
    assert both.shape == (3, 2, 24, 20) and info["groups"] == 1
    info1 = {}
    split = emu.vlbi_retrieval_batch(chunks, 1, 2, 0.0, group_bytes=1, info=info1)
    assert info1["groups"] == 3
    assert len({m.shape for m in info["composites"]}) > 1          # different crops in one batch
    for k, c in enumerate(cs):
        one = np.array(emu.VLBI_chunk_retrieval((c["dlist"], c["edges"], c["time"], c["freq"], c["eta"], 0, 0, 1, 2, 0.0, False))[0])
        assert np.array_equal(both[k], one) and np.array_equal(split[k], one)
        orc = vo.vlbi_chunk_retrieval(c["dlist"], c["edges"], c["time"], c["freq"], c["eta"], 1, 2, 0.0)
        assert vc.rel_err(vc.align_joint(one, orc), orc) <= TOL


def test_crop_of_one_centre_raises_like_the_reference(emu, gold):
    """The reference raises IndexError when the crop keeps fewer than two centres (recorded by make_golden_vlbi.py); so does the
    port, for the one-chunk call and for a batch that holds such a chunk."""
    assert str(gold["small_crop_raises"]) == "IndexError"
    c = _case(gold, "n2")
    bad = dict(c, eta=c["eta"] * float(gold["small_crop_eta_factor"]))
    with pytest.raises(IndexError):
        emu.VLBI_chunk_retrieval(_params(bad))
    with pytest.raises(IndexError):
        emu.vlbi_retrieval_batch([_chunk(c), _chunk(bad)], c["npad"], c["n_dish"], c["tauMask"])


def test_edges_wider_than_the_doppler_span_raise_like_the_reference(emu, gold):
    """Edges of 1.8 times the Doppler span reach Doppler indices below -len(fd) at kept delays: the reference's thth_map raises
    IndexError there (recorded by make_golden_vlbi.py), and so does the port -- before anything is queued."""
    assert str(gold["wide_raises"]) == "IndexError"
    c = vc.wide_case()
    assert np.array_equal(c["dlist"][1], gold["wide_in1"])
    with pytest.raises(IndexError):
        emu.VLBI_chunk_retrieval(_params(c))
