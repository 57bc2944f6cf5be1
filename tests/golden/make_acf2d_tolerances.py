"""Write tests/golden/acf2d_fit_tolerances.json: the bounds of the approximate 2-D ACF fit tests, measured on the host oracle alone
(tests/acf2d_oracle.py: scipy.optimize.least_squares at ftol = xtol = gtol = 1e-15) over the case list of tests/acf2d_cases.py.

    python tests/golden/make_acf2d_tolerances.py

No output of the code under test enters.  Per kind of case ("a": the ACF is the model, "b": realistic), as the 1-D maker's:

  stationarity   10 x the largest max_i |J^T r|_i / chi^2 (gradient in log tau, log dnu, log amp, phasegrad[, alpha]) at the oracle's
                 own solutions, from both of its starts;
  values_rtol    10 x the largest relative difference of tau, dnu, amp, alpha between the oracle's two starts, or 10 x 64 eps;
  phasegrad_tol  the same for the phase gradient, on the scale max(|phasegrad|, phasegraderr): it is often near 0;
  errors_rtol    the same for the standard errors.

The script refuses a case list on which the oracle does not converge from both starts to one minimum (values within 1e-3)."""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import acf2d_cases as cc  # noqa: E402
import acf2d_oracle as ao  # noqa: E402

FLOOR = 64 * np.finfo(float).eps
SAME_MINIMUM = 1e-3
SLOTS = ("stationarity", "values_rtol", "phasegrad_tol", "errors_rtol")


def main():
    warnings.simplefilter("ignore", RuntimeWarning)
    worst = {k: dict.fromkeys(SLOTS, 0.0) for k in ("a", "b")}
    per_case = {}
    for name in cc.FIT_CASES:
        c = cc.case(name)
        alpha = c.kw.get("alpha", 5/3)
        vary = alpha is None
        setups, fits = cc.oracle(name)
        m = dict.fromkeys(SLOTS, 0.0)
        for b, (s, f) in enumerate(zip(setups, fits)):
            if s is None:
                raise SystemExit(f"{name}[{b}]: bad window {f['rect']}; choose another seed")
            f2 = ao.fit(s, alpha=alpha, start=ao.second_start(s, vary))
            if not (f["success"] and f2["success"]):
                raise SystemExit(f"{name}[{b}]: the oracle does not converge from both starts; choose another seed")
            for r in (f, f2):
                g, chi = ao.stationarity([r[k] for k in cc.FIT_KEYS], s, vary)
                m["stationarity"] = max(m["stationarity"], g / chi if chi > 0 else 0.0)
            for k in cc.FIT_KEYS + cc.ERR_KEYS:
                if k == "phasegrad":
                    d = abs(f[k] - f2[k]) / max(abs(f[k]), f["phasegraderr"])
                    slot = "phasegrad_tol"
                elif f[k] == 0:
                    continue
                else:
                    d = abs(f[k] - f2[k]) / abs(f[k])
                    slot = "errors_rtol" if k.endswith("err") else "values_rtol"
                if slot != "errors_rtol" and d > SAME_MINIMUM:
                    raise SystemExit(f"{name}[{b}]: two minima ({k}: {f[k]} and {f2[k]}); choose another seed")
                m[slot] = max(m[slot], d)
        per_case[name] = dict(kind=c.kind, problems=len(fits), **m)
        for k, v in m.items():
            worst[c.kind][k] = max(worst[c.kind][k], v)
        print(name, per_case[name], flush=True)
    out = {"_made_by": "tests/golden/make_acf2d_tolerances.py", "_factor": 10, "_floor": FLOOR, "_oracle_per_case": per_case}
    for kind, m in worst.items():
        out[kind] = {k: 10 * (v if k == "stationarity" else max(v, FLOOR)) for k, v in m.items()}
    with open(os.path.join(HERE, "acf2d_fit_tolerances.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print({k: out[k] for k in ("a", "b")})


if __name__ == "__main__":
    main()
