"""Writes tests/golden/sspec_class_tolerances.json: how far the float64 ORACLE (oracle/sspec_oracle.calc_sspec, NumPy's pocketfft)
lies from the same secondary spectrum evaluated in np.longdouble (tests/sspec_class_checks.sspec_ld), on every case of
tests/sspec_class_cases.py, in the metric of the class tests -- max |A - A_ld| / max A_ld with A = sqrt(P D), the transform's
modulus before post-darkening.  Per group (axis, class, prewhite) the bound is 8 x the largest such error of the group's cases,
at least 64 eps.  The device's radix-16 stages and pocketfft's mixed radix factor the transform differently, so equal errors are
not expected; the factor covers that spread, not an error of another kind (a misplaced or dropped element is at least 1e-3 here).
No bound may reach 1e-10: the script refuses to write such a file, because the case is then too ill-conditioned to test a kernel
and the input, not the factor, has to change.  Runs on the host alone (no GPU, no kernel, no interpreter): nothing the device
computes enters the file.

    python tests/golden/make_sspec_class_tolerances.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import sspec_class_cases as cc  # noqa: E402
import sspec_class_checks as ck  # noqa: E402


def main():
    out = {}
    for shape in cc.EMU_CASES:
        for prewhite in cc.PREWHITE:
            c = ck.Case(shape, prewhite)
            amp, lin = c.errors(c.sec_oracle)
            g = out.setdefault(cc.group(shape, prewhite), {"oracle_amplitude_error": 0.0, "oracle_linear_power_error": 0.0, "cases": []})
            g["oracle_amplitude_error"] = max(g["oracle_amplitude_error"], amp)
            g["oracle_linear_power_error"] = max(g["oracle_linear_power_error"], lin)
            g["cases"].append(cc.case_id(shape))
            print(f"{cc.case_id(shape)} prewhite={int(prewhite)} {cc.group(shape, prewhite)}: oracle amplitude error {amp:.3e}, "
                  f"linear power {lin:.3e}", flush=True)
    for key, g in out.items():
        g["bound"] = max(ck.FACTOR * g["oracle_amplitude_error"], ck.FLOOR)
        assert g["bound"] < ck.CEILING, f"{key}: bound {g['bound']:.3e} reaches {ck.CEILING:g}: change the input of the case, not the factor"
    with open(ck.TOLERANCES, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
