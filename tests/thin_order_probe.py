"""TEST INFRASTRUCTURE ONLY: run the thin-screen kernels on the host interpreter and save their results (argv[1] = .npz).
tests/test_thin_emu_cpu.py runs it with SCINT_EMU_ORDER unset and =rev (waves, lanes and blocks in the opposite order) and
demands identical bits, as tests/emu/order_probe.py does for the other kernels."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)


def main(out_path):
    from _pytest.monkeypatch import MonkeyPatch
    import emulated
    patch = MonkeyPatch()
    emulated.install(patch)
    from scintools_amd import ththmod
    g = np.load(os.path.join(HERE, "golden", "thin.npz"))
    CS = np.fft.fftshift(np.fft.fft2(g["dyn"]))
    tau, fd, eta = g["tau"], g["fd"], float(g["eta_true"])
    res = {}
    res["map"] = ththmod.two_curve_map(CS, tau, fd, 0.5 * eta, g["edges"], 0.5 * eta, g["edges"])[0]
    sv, info = ththmod.sv_sweep_multi(CS[None], [(tau, fd, g["edges"], g["arclet"])], [g["sv_etas"]], 0.02, return_info=True)
    res["sv"], res["iters"] = sv[0], info["iters"]
    rng = np.random.default_rng(2)
    cs = rng.standard_normal(CS.shape) + 1j * rng.standard_normal(CS.shape)
    res["sv_rand"] = ththmod.sv_sweep_multi(cs[None], [(tau, fd, g["edges"], g["edges"])], [np.array([0.6, 1.4]) * eta])[0]
    # few-row and odd-strip members of the MI355X case list (tests/thin_cases.py), and a zero middle row
    import thin_cases as tc
    tau, fd = tc.axes()
    e0 = tc.eta0(tau, fd)
    for n1, n2, kind, cutf in [c for c in tc.small_class_cases() if c[1] in (1, 3, 5)] + [(257, 300, "gauss", 0.0)]:
        sv, info = ththmod.sv_sweep_multi(tc.spectrum(kind)[None], [tc.grid(n1, n2, tau, fd)], [np.array([e0])], cutf * fd.max(),
                                          return_info=True)
        res[f"sv_{n1}_{n2}"], res[f"iters_{n1}_{n2}"] = sv[0], info["iters"]
    g = tc.grid(200, 9, tau, fd)
    res["sv_zero_row"] = ththmod.sv_sweep_multi(tc.zero_middle_row(tc.spectrum("gauss"), tau, fd, e0, g[2], g[3])[None], [g],
                                                [np.array([e0])])[0]
    np.savez(out_path, **res)
    patch.undo()


if __name__ == "__main__":
    main(sys.argv[1])
