"""scint_utils.slow_FT -- scint_slow_ft and its Python wrapper -- interpreted on the host (tests/emu) through the same C ABI as on a
GPU, against the long-double oracle (tests/slowft_oracle.py) and the unmodified reference's outputs (tests/golden/slowft.npz).  The
checks are those of the GPU tests (tests/slowft_checks.py) at the shapes of at most 65 x 16 pixels.  Runs without a GPU."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)
import slowft_checks as ck  # noqa: E402


@pytest.fixture()
def U(monkeypatch):
    import emulated
    emulated.install(monkeypatch)
    from scintools_amd import scint_utils
    return scint_utils


@pytest.mark.parametrize("shape", ck.emu_shapes(ck.TAILS + ck.BLOCKS + ck.ROUTES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes(U, shape):
    ck.check_shape(U, *shape)


@pytest.mark.parametrize("kind", ["desc", "uneven"])
def test_freq_orderings(U, kind):
    ck.check_shape(U, 33, 16, kind)


def test_constant_freqs_is_fft2(U):
    ck.check_constant_freqs(U, 48, 20)


def test_reference_column_is_plain_dft(U):
    ck.check_reference_column(U)


def test_fref(U):
    ck.check_fref(U)


def test_device_tensor_out_device_float32(U):
    ck.check_device_paths(U)


def test_nan_pixel_gives_nan_everywhere(U):
    ck.check_nan(U)


def test_deterministic(U):
    ck.check_deterministic(U)


def test_transposed_result_feeds_eval_sweep(U):
    ck.check_eval_sweep(U)


def test_errors(U):
    ck.check_errors(U, pytest)
