"""scint_utils.slow_FT without a GPU: the two NumPy restatements (tests/slowft_oracle.py) against the unmodified reference's outputs
(tests/golden/slowft.npz), the identities the device tests rely on, and the host side of the port up to the device call."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import slowft_cases as sc  # noqa: E402
import slowft_checks as ck  # noqa: E402
import slowft_oracle as so  # noqa: E402


@pytest.fixture(scope="module")
def gold(golden):
    return golden("slowft.npz")


@pytest.mark.parametrize("case", list(sc.GOLDEN))
def test_oracles_against_reference(gold, case):
    """The reference within the bound of the long-double truth (this measures the reference's own E), and the channel-by-channel
    float64 restatement within twice the bound of the reference."""
    d, f = sc.golden_inputs(case)
    nt, nf, kind = sc.GOLDEN[case]
    fs = so.fscale(f)
    ck.assert_close(f"{case} reference vs truth", gold[case], ck.truth(nt, nf, kind), d, fs)
    ck.assert_close(f"{case} float64 oracle vs reference", so.slow_ft(d, f), gold[case], d, fs, factor=2.0)


def test_golden_cases_cover_the_orderings():
    assert {v[:2] for v in sc.GOLDEN.values()} == {(64, 48), (256, 64), (250, 37)}
    assert {v[2] for v in sc.GOLDEN.values()} == set(sc.FREQ_KINDS)
    assert np.all(np.diff(sc.freqs(37, "asc")) > 0) and np.all(np.diff(sc.freqs(37, "desc")) < 0)
    steps = np.diff(sc.freqs(37, "uneven"))
    assert np.all(steps > 0) and steps.max() > 2 * steps.min()


def test_truth_identities():
    """Constant freqs: the shifted fft2.  Column nf // 2 of stage 1: a plain DFT.  A wrong element exceeds the bound."""
    d = sc.dyn(48, 20)
    out = so.slow_ft_ld(d, sc.freqs(20, "const"))
    ck.assert_close("truth, constant freqs vs fft2", out, np.fft.fftshift(np.fft.fft2(d)), d, np.ones(20))
    d, f = sc.dyn(33, 16), sc.freqs(16, "uneven")
    re, im = so.stage1_ld(d, f)
    col = (re[:, 8] + 1j * im[:, 8]).astype(np.complex128)
    assert np.max(np.abs(col - np.fft.fft(d[:, 8]))) <= ck.bound(33, 16, so.fscale(f)) * np.sum(np.abs(d))
    bad = np.array(ck.truth(33, 16, "asc"))
    bad[5, 7] = bad[5, 8]
    with pytest.raises(AssertionError):
        ck.assert_close("one wrong element", bad, ck.truth(33, 16, "asc"), sc.dyn(33, 16), so.fscale(sc.freqs(16, "asc")))


def test_module_mirrors_the_reference():
    import inspect
    from scintools_amd import clean, dynspec, scint_utils
    sig = inspect.signature(scint_utils.slow_FT)
    assert list(sig.parameters) == ["dynspec", "freqs", "fref", "out_device"]
    assert [p.kind for p in sig.parameters.values()][2:] == [inspect.Parameter.KEYWORD_ONLY] * 2
    assert sig.parameters["fref"].default is None and sig.parameters["out_device"].default is False
    assert scint_utils.svd_model is clean.svd_model and scint_utils.is_valid is clean.is_valid
    assert scint_utils.get_window is dynspec.get_window


def test_library_exports_and_argument_errors():
    import ctypes
    from scintools_amd import _lib
    names = ("scint_slow_ft", "scint_slow_ft_workspace_bytes")
    assert set(names) <= set(_lib.header_symbols()) and set(names) <= set(_lib._SIGNATURES)
    lib = _lib.load()
    n = ctypes.c_size_t()
    assert lib.scint_slow_ft_workspace_bytes(4096, 4096, ctypes.byref(n)) == 0
    assert 24 * 4096 * 4096 <= n.value <= 24 * 4096 * 4096 + 1024
    assert lib.scint_slow_ft_workspace_bytes(33, 5, ctypes.byref(n)) == 0 and n.value >= 8 * 64 * 5 + 16 * 33 * 5
    for nt, nf in ((0, 4), (4, 0), (-1, 4), ((1 << 20) + 1, 1), (1, (1 << 20) + 1), (1 << 20, 1 << 11)):
        assert lib.scint_slow_ft_workspace_bytes(nt, nf, ctypes.byref(n)) == _lib.SCINT_E_ARG, (nt, nf)
        assert "slow_ft" in _lib.last_error()
    assert lib.scint_slow_ft(None, 4, 4, None, None, None, 0, None) == _lib.SCINT_E_ARG
    assert "slow_ft: null pointer" in _lib.last_error()


def test_no_gpu_no_fallback():
    import torch
    from scintools_amd import _lib, scint_utils
    if not torch.cuda.is_available():
        with pytest.raises(_lib.ScintHipError):
            scint_utils.slow_FT(sc.dyn(3, 5), sc.freqs(5, "asc"))
