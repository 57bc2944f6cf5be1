"""The screen-simulator cases shared by tests/golden/make_golden_sim.py (which runs the unmodified reference on them), the GPU tests
(tests/test_gpu_sim.py) and the host-interpreter tests (tests/test_sim_emu_cpu.py).  All use seed 7; parameters not listed keep the
constructor's defaults."""
SEED = 7

CASES = {
    "a": dict(nx=16, ny=16, nf=2, mb2=200, ds=0.2),                                     # smallest legal transform on both axes
    "b": dict(nx=64, ny=32, nf=5, mb2=200, ds=0.1),                                     # odd nf, rectangular, phases wrap (23 rad)
    "c": dict(nx=128, ny=16, nf=3, mb2=200, ds=0.05, ar=10, psi=30),                    # cross term of the anisotropy, nx >> ny
    "d": dict(nx=32, ny=64, nf=6, mb2=100, ds=0.1, ar=3, psi=-20, lamsteps=True),       # wavelength steps, ny > nx
    "e": dict(nx=64, ny=32, nf=4, mb2=200, ds=0.1, efield=True, nsub=40),               # case b's screen, the two output options
    "f": dict(nx=256, ny=64, nf=8, dx=0.02, dy=0.05, mb2=20),                           # dx != dy, two column passes on x, pulsewin
}

ARRAYS = ("xyp", "w", "spe", "spi", "xyi", "dyn", "pulsewin", "dm", "freqs", "times", "x", "lams")
SCALARS = ("df", "bw", "dt", "freq", "tobs", "mjd", "nsub", "nchan", "eta", "betaeta", "ffconx", "ffcony", "consp", "s0", "sref", "scnorm")


def kwargs(case):
    return dict(CASES[case], seed=SEED)
