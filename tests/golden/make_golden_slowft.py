#!/usr/bin/env python
"""Generate tests/golden/slowft.npz by running the UNMODIFIED reference's scint_utils.slow_FT (scintools/scint_utils.py:655-703)
with the stand-ins of tests/golden/refshim, as the other make_golden_* scripts do.

    SCINTOOLS_REFERENCE=<checkout of the reference> python tests/golden/make_golden_slowft.py

slow_FT calls np.fft.fftshift(SS, axis=0) (line 695); the keyword is `axes`, so as shipped it raises TypeError in every NumPy.  This
process (only) lets np.fft.fftshift accept `axis=` as `axes=` before the reference runs -- the same kind of stand-in as
make_golden_acf.py's np.complex_.  Nothing else of the reference is touched.
Inputs: the seeded cases of tests/slowft_cases.py (regenerated here and by the tests, not stored).  Stored per case: the output."""
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "refshim"))
sys.path.insert(0, os.environ["SCINTOOLS_REFERENCE"])
sys.path.insert(0, os.path.join(REPO, "tests"))

import matplotlib  # noqa: E402
matplotlib.use("Agg")
import numpy as np  # noqa: E402

_fftshift = np.fft.fftshift


def _fftshift_axis(x, axes=None, axis=None):
    return _fftshift(x, axes=axis if axes is None else axes)


np.fft.fftshift = _fftshift_axis
from scintools.scint_utils import slow_FT  # noqa: E402
import slowft_cases as sc  # noqa: E402

warnings.simplefilter("ignore")

if __name__ == "__main__":
    arrs = {}
    for case in sc.GOLDEN:
        d, f = sc.golden_inputs(case)
        out = slow_FT(np.array(d), np.array(f))
        assert out.shape == d.shape and out.dtype == np.complex128
        arrs[case] = out
        print(case, out.shape, "max |SS|", np.abs(out).max())
    path = os.path.join(HERE, "slowft.npz")
    np.savez_compressed(path, **arrs)
    print(f"slowft.npz: {os.path.getsize(path) / 1024:.0f} KiB, {len(arrs)} arrays")
