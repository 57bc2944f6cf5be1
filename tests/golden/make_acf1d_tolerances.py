"""Write tests/golden/acf1d_fit_tolerances.json: the bounds of the 1-D ACF fit tests, measured on the host oracle alone
(tests/acf1d_oracle.py: scipy.optimize.least_squares at ftol = xtol = gtol = 1e-15) over the case list of tests/acf1d_cases.py.

    python tests/golden/make_acf1d_tolerances.py

No output of the code under test enters.  Per kind of case ("a": cuts generated exactly from the model, "b": realistic):

  stationarity   10 x the largest max_i |J^T r|_i / chi^2 (gradient in log tau, log dnu, log amp[, alpha]) at the oracle's own
                 solutions, from both of its starts;
  values_rtol    10 x the largest relative difference of tau, dnu, amp, alpha between the oracle's two starts -- or, where the two
                 agree more closely than that, 10 x 64 eps: a parameter passes through exp, log and pow on its way out, each good to
                 a few units in the last place, so two correct programs cannot be asked to agree below some tens of eps;
  errors_rtol    the same for the standard errors.

The kinds are kept apart because a kind (a) chi^2 is rounding noise (~1e-31): the ratio |J^T r| / chi^2 and the standard errors,
which scale with sqrt(chi^2), mean nothing there, and one bound over both kinds would let that noise excuse the realistic cases.
Each kind's bound is at most the bound over all cases.  The script also refuses a case list on which the oracle does not
converge from both starts: the GPU tests allow no unconverged problem."""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import acf1d_cases as cc  # noqa: E402
import acf1d_oracle as ao  # noqa: E402

FLOOR = 64 * np.finfo(float).eps


def main():
    warnings.simplefilter("ignore", RuntimeWarning)
    worst = {k: dict(stationarity=0.0, values_rtol=0.0, errors_rtol=0.0) for k in ("a", "b")}
    per_case = {}
    for name in cc.CASES:
        c = cc.case(name)
        alpha = c.kw.get("alpha", 5/3)
        vary = alpha is None
        setups, fits = cc.oracle(name)
        m = dict(stationarity=0.0, values_rtol=0.0, errors_rtol=0.0)
        for b, (s, f) in enumerate(zip(setups, fits)):
            f2 = ao.fit(s, alpha=alpha, start=ao.second_start(s, vary))
            if not (f["success"] and f2["success"]):
                raise SystemExit(f"{name}[{b}]: the oracle does not converge from both starts; choose another seed")
            for r in (f, f2):
                g, chi = ao.stationarity([r[k] for k in cc.FIT_KEYS], s, vary)
                m["stationarity"] = max(m["stationarity"], g / chi if chi > 0 else 0.0)
            for keys, slot in ((cc.FIT_KEYS, "values_rtol"), (cc.ERR_KEYS, "errors_rtol")):
                for k in keys:
                    if f[k] != 0:
                        m[slot] = max(m[slot], abs(f[k] - f2[k]) / abs(f[k]))
        per_case[name] = dict(kind=c.kind, problems=len(fits), **m)
        for k, v in m.items():
            worst[c.kind][k] = max(worst[c.kind][k], v)
        print(name, per_case[name], flush=True)
    out = {"_made_by": "tests/golden/make_acf1d_tolerances.py", "_factor": 10, "_floor": FLOOR, "_oracle_per_case": per_case}
    for kind, m in worst.items():
        out[kind] = dict(stationarity=10 * m["stationarity"], values_rtol=10 * max(m["values_rtol"], FLOOR),
                         errors_rtol=10 * max(m["errors_rtol"], FLOOR))
    with open(os.path.join(HERE, "acf1d_fit_tolerances.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print({k: out[k] for k in ("a", "b")})


if __name__ == "__main__":
    main()
