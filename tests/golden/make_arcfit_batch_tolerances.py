"""Writes tests/golden/arcfit_batch_tolerances.json: how far the HOST's float64 parabola fits (arcfit.fit_parabola /
fit_log_parabola, i.e. np.polyfit) lie from the same least-squares parabola solved in np.longdouble, on the seeded profiles of
tests/arcfit_batch_cases.py; per kind of fit the tolerance is 4 x the largest relative deviation, at least 64 eps, for the peak and
for its error.  Both are float64 solves of one problem and a centred solve should do no worse than np.polyfit: the factor covers the
spread between cases, not another algorithm's error.  Runs on the host alone (no GPU, no kernel): nothing the device computes enters
the file.

    python tests/golden/make_arcfit_batch_tolerances.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import arcfit_batch_cases as cc  # noqa: E402
import arcfit_batch_checks as ck  # noqa: E402
from scintools_amd import arcfit as af  # noqa: E402

EPS = np.finfo(float).eps


def main():
    x = cc.peak_x()
    out = {}
    for kind, log_parabola in (("plain", False), ("log_parabola", True)):
        worst = {"peak": 0.0, "error": 0.0}
        count = 0
        for seed in (7, 8, 9):
            for avg in cc.bump_profiles(seed=seed):
                for side in (-1, 0, 1):
                    ref = ck.oracle(af, avg, x, 0.2, cc.PEAK_ETAMIN, cc.PEAK_ETAMAX, side=side, log_parabola=log_parabola)
                    if ref["status"] != 0:
                        continue
                    eta_t, err_t = ck.truth(ref["xdata"], ref["ydata"], log_parabola)
                    worst["peak"] = max(worst["peak"], abs(ref["eta"] - eta_t) / abs(eta_t))
                    worst["error"] = max(worst["error"], abs(ref["etaerr2"] - err_t) / abs(err_t))
                    count += 1
        out[kind] = {"peak": max(4 * worst["peak"], 64 * EPS), "error": max(4 * worst["error"], 64 * EPS),
                     "host_peak_deviation": worst["peak"], "host_error_deviation": worst["error"], "profiles": count}
    path = os.path.join(HERE, "arcfit_batch_tolerances.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
