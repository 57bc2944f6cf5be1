// sim.hpp -- the split-step screen simulator (scint_sim.py: Simulation.get_screen / get_intensity / get_pulse) as
// loaders and storers of the two FFT kernels in fft.hpp.  The entry points are at the end of fft.hip.
//
//   screen   w (the weights of get_screen / swdsp, from the index alone)  ->  xyp = real(fft2(w (z1 + i z2)))
//            rows (y): load w * (z1 + i z2)            cols (x): last pass stores the real part
//   field    per frequency f:  E = ifft2(frfilt3(fft2(exp(i xyp scale_f))))  and only column ny/2 of E is kept
//            cols (x): the first pass loads exp(i xyp scale) -- sincos in the loader, the phase field is never written
//            rows (y): the storer multiplies by the Fresnel filter and (-1)^ky and REDUCES the row to g[kx]:
//                      E[x, ny/2] = (1/ny) sum_ky ifft_x(F)[x, ky] e^{+2 pi i ky (ny/2) / ny} = (1/ny) sum_ky (-1)^ky ifft_x(F)[x, ky]
//                      so column ny/2 is the inverse transform along x of g[kx] = sum_ky (-1)^ky F[kx, ky]
//            cols (x): one inverse transform of g for the whole group, lanes along frequency, stored as complex64 into
//                      spe[x, f] together with spi = |spe|^2 (float32)
//   pulse    pulsewin: rows of spe times the Blackman window, zero-padded to 2 nf; |.|^2 and the roll in the storer
//
// Inverse transforms are conj-forward-conj, as everywhere in fft.hip.  Functions whose results must round like NumPy's
// (a product feeding a sum, pow or exp) switch contraction off locally: this unit is built with the default (fast).
#pragma once
#include <math.h>

#include "fft.hpp"

namespace scint {

// ---- screen weights -------------------------------------------------------------------------------------
struct SimScreenPar {
    int nx, ny;
    double dqx, dqy;      // 2 pi / (dx nx), 2 pi / (dy ny)
    double a, b, c;       // anisotropy coefficients of swdsp (scint_sim.py:283-285)
    double con, alf;      // sqrt(consp), -(alpha + 2) / 4
    double inner2;        // inner ** 2
};

// swdsp(kx = p dqx, ky = q dqy), operation by operation (scint_sim.py:286-291)
__host__ __device__ inline double sim_swdsp(const SimScreenPar& s, int p, int q) {
#pragma clang fp contract(off)
    const double kx = (double)p * s.dqx, ky = (double)q * s.dqy;
    const double kx2 = kx * kx, ky2 = ky * ky;
    const double q2 = (s.a * kx2 + s.b * ky2) + s.c * (kx * ky);
    const double e = exp(((-(kx2 + ky2)) * s.inner2) / 2.0);
    return s.con * (pow(q2, s.alf) * e);
}

// The value get_screen leaves at w[i, j] (scint_sim.py:182-198), its fill order restated: the ky = 0 line copies from
// row k, not k - 1 (line 185: w[nx/2, 0] receives the still-zero w[nx/2 + 1, 0], the rows above it are shifted by one);
// the mirrored half of column ny/2 is overwritten by the loop's own last iteration; w[0, 0] is never written.
__host__ __device__ inline double sim_weight(const SimScreenPar& s, int i, int j) {
    const int nx = s.nx, ny = s.ny, hx = nx / 2, hy = ny / 2;
    if (i == 0) {
        if (j == 0) return 0.0;
        return sim_swdsp(s, 0, j <= hy ? j : ny - j);
    }
    if (j == 0) {
        if (i < hx) return sim_swdsp(s, i, 0);
        if (i == hx) return 0.0;
        return sim_swdsp(s, nx + 1 - i, 0);
    }
    if (j < hy) return sim_swdsp(s, i <= hx ? i : i - nx, j);
    if (j == hy) return sim_swdsp(s, i < hx ? i : nx - i, hy);
    return sim_swdsp(s, i < hx ? -i : nx - i, ny - j);
}

__global__ void __launch_bounds__(256) sim_weights_kernel(SimScreenPar s, double* __restrict__ w) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)s.nx * s.ny) return;
    const int i = (int)(idx / s.ny), j = (int)(idx - (int64_t)i * s.ny);
    w[idx] = sim_weight(s, i, j);
}

// rows (y) of the screen transform: w (z1 + i z2)
struct SimScreenLoad {
    const double* w; const double* z1; const double* z2; int ny;
    struct Slot {
        const double* w; const double* z1; const double* z2;
        __device__ inline cplx operator()(int j) const { return mk(w[j] * z1[j], w[j] * z2[j]); }
    };
    __device__ inline Slot open(int64_t s) const { return Slot{w + s * ny, z1 + s * ny, z2 + s * ny}; }
};
struct SimRowLoad {          // plain rows of a [slots][n] complex array
    const cplx* a; int n;
    struct Slot {
        const cplx* row;
        __device__ inline cplx operator()(int j) const { return row[j]; }
    };
    __device__ inline Slot open(int64_t s) const { return Slot{a + s * n}; }
};
struct SimRowStore {
    static constexpr bool kPair = false;
    cplx* a; int n;
    struct Slot {
        cplx* row;
        __device__ inline void operator()(int k, cplx v) const { row[k] = v; }
    };
    __device__ inline Slot open(int64_t s) const { return Slot{a + s * n}; }
};
struct SimRealStore {        // last column pass of the screen: xyp = real(.)
    double* out; int ld;
    __device__ inline void operator()(int64_t, int r, int c, cplx v) const { out[(int64_t)r * ld + c] = v.x; }
};

// ---- field --------------------------------------------------------------------------------------------
// first column pass: exp(i xyp[r, c] scale[batch])
struct SimPhaseLoad {
    const double* xyp; const double* scale; int ld;
    __device__ inline cplx operator()(int64_t bt, int r, int c) const {
        double sn, cs;
        sincos(xyp[(int64_t)r * ld + c] * scale[bt], &sn, &cs);
        return mk(cs, sn);
    }
};

// frfilt3 (scint_sim.py:294-311) builds its filter in complex64: q2 in double in the reference's operation order,
// cos and -sin in double, each rounded to float, and THEN the product with the complex128 spectrum.
struct SimFilter {
    const double* scale; double ffconx, ffcony; int nx, ny, lognx; int64_t nslots;
    struct Row { double q2x, scale; };
    __device__ inline Row row(int64_t slot) const {
#pragma clang fp contract(off)
        const int kx = (int)(slot & (nx - 1));
        const double sc = slot < nslots ? scale[slot >> lognx] : 0.0;      // (slots past the end are opened too, never stored)
        const double kf = (double)(kx <= nx - kx ? kx : nx - kx);
        return Row{((kf * kf) * sc) * ffconx, sc};
    }
    __device__ inline cplx apply(const Row& r, int ky, cplx v) const {
#pragma clang fp contract(off)
        const int kf = ky <= ny - ky ? ky : ny - ky;
        const double q2 = r.q2x + (ffcony * (double)(kf * kf)) * r.scale;
        double sn, cs;
        sincos(q2, &sn, &cs);
        const double fr = (double)(float)cs, fi = (double)(float)(-sn);
        return mk(v.x * fr - v.y * fi, v.x * fi + v.y * fr);
    }
};
// rows (y), the column shortcut: g[kx][batch] = conj(sum_ky (-1)^ky F[kx, ky] filt[kx, ky])
struct SimFilterReduce {
    static constexpr bool kPair = false;
    static constexpr bool kSlotReduce = true;
    SimFilter f; cplx* g; int group;       // g[kx * group + batch]
    struct Slot {
        const SimFilterReduce& p; SimFilter::Row r; cplx* out;
        __device__ inline void operator()(int ky, cplx v, cplx& acc) const {
            const cplx t = p.f.apply(r, ky, v);
            acc = (ky & 1) ? acc - t : acc + t;
        }
        __device__ inline void finish(cplx total) const { *out = conj(total); }
    };
    __device__ inline Slot open(int64_t slot) const {
        const int64_t bt = slot >> f.lognx, kx = slot & (f.nx - 1);
        return Slot{*this, f.row(slot), g + kx * group + bt};
    }
};
// rows (y), the full route: conj(F filt) in place, ready for the conj-forward inverse
struct SimFilterStore {
    static constexpr bool kPair = false;
    SimFilter f; cplx* a;
    struct Slot {
        const SimFilterStore& p; SimFilter::Row r; cplx* row;
        __device__ inline void operator()(int ky, cplx v) const { row[ky] = conj(p.f.apply(r, ky, v)); }
    };
    __device__ inline Slot open(int64_t slot) const { return Slot{*this, f.row(slot), a + slot * f.ny}; }
};

// complex64 value and its intensity as the reference rounds them: spi = real(spe * conj(spe)) in complex64
__device__ inline void sim_store_spe(float* spe, float* spi, int64_t o, double re, double im) {
#pragma clang fp contract(off)
    const float fr = (float)re, fi = (float)im;
    spe[2 * o] = fr;
    spe[2 * o + 1] = fi;
    const float rr = fr * fr, ii = fi * fi;
    spi[o] = rr + ii;
}
// last pass of the inverse transform of g: column c is frequency f0 + c
struct SimSpeStore {
    float* spe; float* spi; int nf; int f0; double norm;     // norm = 1 / (nx ny)
    __device__ inline void operator()(int64_t, int x, int c, cplx v) const {
        sim_store_spe(spe, spi, (int64_t)x * nf + f0 + c, v.x * norm, -(v.y * norm));
    }
};
// last pass of the full inverse transform: column ny/2 goes to spe, the last frequency's plane to xyi
struct SimFullStore {
    float* spe; float* spi; double* xyi; int nf, ny; int f0; double norm;
    __device__ inline void operator()(int64_t bt, int x, int c, cplx v) const {
        const double re = v.x * norm, im = -(v.y * norm);
        const int f = f0 + (int)bt;
        if (spe && c == ny / 2) sim_store_spe(spe, spi, (int64_t)x * nf + f, re, im);
        if (xyi && f == nf - 1) xyi[(int64_t)x * ny + c] = re * re + im * im;
    }
};

// ---- pulse ----------------------------------------------------------------------------------------------
// get_pulse (scint_sim.py:267-270): fft(spe * blackman(nf), 2 nf), |.|^2, np.roll(., nf) -- of the FLATTENED array,
// so the upper half of a row's transform lands in the next row.
struct SimPulseLoad {
    const float* spe; const double* win; int nf;
    struct Slot {
        const float* row; const double* win; int nf;
        __device__ inline cplx operator()(int j) const {
            if (j >= nf) return mk(0.0, 0.0);
            return mk((double)row[2 * j] * win[j], (double)row[2 * j + 1] * win[j]);
        }
    };
    __device__ inline Slot open(int64_t s) const { return Slot{spe + 2 * s * nf, win, nf}; }
};
struct SimPulseStore {
    static constexpr bool kPair = false;
    double* out; int nf; int64_t total;       // total = nx * 2 nf
    struct Slot {
        double* out; int64_t base, total;
        __device__ inline void operator()(int k, cplx v) const {
            int64_t o = base + k;
            if (o >= total) o -= total;
            out[o] = v.x * v.x + v.y * v.y;
        }
    };
    __device__ inline Slot open(int64_t s) const { return Slot{out, s * 2 * nf + nf, total}; }
};

}  // namespace scint
