"""Writes tests/golden/inpaint_lines_tolerances.json: for the cases of tests/inpaint_lines_cases.py, the steps that the NumPy
restatement of the preconditioned conjugate gradients (tests/inpaint_lines_oracle.py: the reference algorithm, not the library)
takes to a true relative residual of 1e-12, the steps of plain NumPy conjugate gradients on the same system (capped at 2000, with
the residual reached and NOCONV noted), and the condition number of the matrix.  The tests bound the device's step count by
1.25 x the restatement's + 2 for the cases in COUNTED.

    python tests/golden/make_inpaint_lines_tolerances.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import inpaint_lines_cases as lc  # noqa: E402
import inpaint_lines_oracle as lo  # noqa: E402
import inpaint_oracle as io  # noqa: E402

TOL, MAX_ITER = 1e-12, 2000


def main():
    out = {}
    for name in lc.NAMES:
        dyn, bad = lc.case(name)
        a, b = io.system(dyn, bad)
        _, steps, res = lo.pcg(a, b, lo.Preconditioner(bad, a.diagonal()), TOL, MAX_ITER)
        _, cg_steps, cg_res = lo.cg(a, b, TOL, MAX_ITER)
        ev = np.linalg.eigvalsh(a.toarray())
        out[name] = dict(shape=list(bad.shape), nmask=int(bad.sum()), pcg_steps=steps, pcg_residual=res, cg_steps=cg_steps,
                         cg_residual=cg_res, cg_outcome="ok" if cg_res <= TOL else "NOCONV", kappa=float(ev[-1] / ev[0]))
        print(name, out[name], flush=True)
    with open(os.path.join(HERE, "inpaint_lines_tolerances.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
