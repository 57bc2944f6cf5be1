"""scint_utils.slow_FT on the GPU against the long-double oracle (tests/slowft_oracle.py) and the unmodified reference's outputs
(tests/golden/slowft.npz).  The checks, their shapes and the derived tolerance are in tests/slowft_checks.py, shared with the
host-interpreter run (tests/test_slowft_emu_cpu.py); every check prints the E it measured."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import slowft_cases as sc  # noqa: E402
import slowft_checks as ck  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def U():
    from scintools_amd import scint_utils
    return scint_utils


@pytest.fixture(scope="module")
def gold(golden):
    return golden("slowft.npz")


@pytest.mark.parametrize("case", list(sc.GOLDEN))
def test_against_reference(U, gold, case):
    ck.check_golden(U, gold, case)


@pytest.mark.parametrize("shape", ck.TAILS + ck.BLOCKS + ck.ROUTES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes(U, shape):
    ck.check_shape(U, *shape)


@pytest.mark.parametrize("kind", ["desc", "uneven"])
def test_freq_orderings(U, kind):
    ck.check_shape(U, 67, 33, kind)


def test_phase_accuracy_wide_band(U):
    ck.check_phase_accuracy(U)


@pytest.mark.parametrize("shape", [(64, 64), (48, 20)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_constant_freqs_is_fft2(U, shape):
    ck.check_constant_freqs(U, *shape)


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
