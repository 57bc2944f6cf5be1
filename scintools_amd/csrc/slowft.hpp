// slowft.hpp -- the scaled-time ("NuT") conjugate spectrum, scint_utils.slow_FT (scint_utils.py:655-703): per channel j a DFT of the
// time axis at t * s_j (s_j = f_j / f_ref), then a plain FFT along frequency, both fftshifts folded into the store indices.
// Included from fft.hip (the entry points are at its end); stage 2 re-uses fft_rows_kernel where nf is one of its lengths.
//
//   S1[k', j] = sum_t dyn[t, j] exp(-2 pi i s_j k' t / nt),   k' = -nt/2 .. ceil(nt/2) - 1,   stored at row k' + nt/2
//
//   pre      slowft_transpose_kernel   dyn[t][j] -> dynT[j][ntp] (ntp = nt rounded up to kSlowB, the tail zero): coalesced along j
//            on the way in, and every channel becomes one contiguous row
//   stage 1  slowft_stage1_kernel      a workgroup owns one channel (blockIdx.x) and 256 values of |k'| (lanes); dyn is REAL, so
//            S1[-k'] = conj(S1[k']) and only k' = 0 .. nt/2 are computed: nt^2 nf / 2 terms of two FMAs each.
//            t = t1 B + t0 (B = kSlowB):  exp(-2 pi i phi t) = P[t1] Q[t0], phi = s_j k' / nt.  Q (B entries) lives in registers;
//            P is formed once per GROUP of kSlowG blocks, from the group's own phase, and inside a group the blocks are chained last
//            to first by the one constant exp(-2 pi i phi B) (at most kSlowG - 1 products, whatever nt is).  Every table entry comes
//            straight from its own phase, nothing rotates along the row: B + 1 + nt / (B kSlowG) sincos per (k', j) instead of nt.
//            The channel's row is wave-uniform: it arrives through the scalar cache and feeds the FMAs as a scalar operand, so the
//            inner loop holds no vector memory or LDS instruction.  256 VGPRs, nothing spilled.
//   stage 2  nf a power of two in 16..8192: fft_rows_kernel on the rows of S1, the shift in the storer (SlowShiftStore);
//            any other nf: slowft_dft_kernel, the direct sum with W_nf^((j m) mod nf) from the long-double table of fft.hip, the
//            index advanced in exact integers.
//
// Phase.  x = s m / nt cycles with the integer m = k' t (exact in float64: below 2^41).  s m is carried as hi + lo (one FMA), the
// quotient is corrected by its exact remainder, and the integer part is dropped BEFORE the 2 pi: the angle handed to sincos is in
// [-pi, pi] with an absolute error of a few 2^-53 whatever nt is.  (DESIGN.md section 4l has the error budget.)
#pragma once
#include <math.h>

#include "fft.hpp"

namespace scint {

constexpr int kSlowB = 32;                  // table block: t = t1 * kSlowB + t0
constexpr int kSlowG = 8;                   // blocks that share one outer phase
constexpr int kSlowThreads = 256;           // values of |k'| per workgroup

// (cos, sin) of 2 pi frac(s m / nt); inv_nt = 1 / nt rounded (the remainder r makes up for its rounding)
__device__ inline void slowft_cis(double s, double m, double nt, double inv_nt, double* c, double* sn) {
#pragma clang fp contract(off)
    const double hi = s * m, lo = fma(s, m, -hi);
    const double y = hi * inv_nt;
    const double r = fma(-y, nt, hi);                       // hi - y nt, exact
    const double f = (y - rint(y)) + (r + lo) * inv_nt;    // the difference is exact
    sincos(6.283185307179586476925 * f, sn, c);
}

__global__ void __launch_bounds__(256)
slowft_transpose_kernel(const double* __restrict__ dyn, int64_t nt, int64_t nf, int64_t ntp, double* __restrict__ dynT) {
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t t0 = (int64_t)blockIdx.x * 32, j0 = (int64_t)blockIdx.y * 32;
    for (int i = ty; i < 32; i += 8) {
        const int64_t t = t0 + i, j = j0 + tx;
        tile[i][tx] = (t < nt && j < nf) ? dyn[t * nf + j] : 0.0;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int64_t j = j0 + i, t = t0 + tx;
        if (j < nf && t < ntp) dynT[j * ntp + t] = tile[tx][i];
    }
}

__global__ void __launch_bounds__(kSlowThreads)
slowft_stage1_kernel(const double* __restrict__ dynT, const double* __restrict__ fscale, cplx* __restrict__ s1, int64_t nt,
                     int64_t ntp, int64_t nf, double inv_nt) {
    const int64_t j = blockIdx.x, half = nt / 2;
    const int64_t kq = (int64_t)blockIdx.y * kSlowThreads + threadIdx.x;       // |k'|
    const double kd = (double)(kq < half ? kq : half);                         // (lanes past the end redo the last one, store nothing)
    const double s = fscale[j], dnt = (double)nt;
    // a sum over t of dyn exp(-i a_t) is kept as the pair (sum dyn cos a_t, sum dyn sin a_t); times exp(-i b) it becomes
    // (A cos b - S sin b, A sin b + S cos b)
    double qc[kSlowB], qs[kSlowB];
#pragma unroll
    for (int t0 = 0; t0 < kSlowB; ++t0) slowft_cis(s, kd * (double)t0, dnt, inv_nt, &qc[t0], &qs[t0]);
    double bc, bs;                                          // one block further: exp(-2 pi i phi kSlowB)
    slowft_cis(s, kd * (double)kSlowB, dnt, inv_nt, &bc, &bs);
    const double* __restrict__ row = dynT + j * ntp;
    double accr = 0.0, acci = 0.0;
    for (int64_t t = 0; t < ntp; t += kSlowB * kSlowG) {
        const int64_t left = (ntp - t) / kSlowB;
        const int ng = (int)(left < kSlowG ? left : kSlowG);
        double hr = 0.0, hs = 0.0;                          // the group, last block first: h = block + exp(-2 pi i phi kSlowB) h
        for (int g = ng - 1; g >= 0; --g) {
            const double* __restrict__ blk = row + t + (int64_t)g * kSlowB;
            double ar0 = 0.0, ar1 = 0.0, as0 = 0.0, as1 = 0.0;         // two chains each: the FMAs of one chain depend on each other
#pragma unroll
            for (int t0 = 0; t0 < kSlowB; t0 += 2) {
                const double d0 = blk[t0], d1 = blk[t0 + 1];
                ar0 = fma(d0, qc[t0], ar0);
                as0 = fma(d0, qs[t0], as0);
                ar1 = fma(d1, qc[t0 + 1], ar1);
                as1 = fma(d1, qs[t0 + 1], as1);
            }
            const double nr = (ar0 + ar1) + (hr * bc - hs * bs);
            hs = (as0 + as1) + (hr * bs + hs * bc);
            hr = nr;
        }
        double pc, ps;                                      // the group's own phase, from t
        slowft_cis(s, kd * (double)t, dnt, inv_nt, &pc, &ps);
        accr += hr * pc - hs * ps;
        acci += hr * ps + hs * pc;
    }
    if (kq > half) return;
    if (half + kq < nt) s1[(half + kq) * nf + j] = mk(accr, -acci);            // k' = +kq (not for the lone -nt/2 of an even nt)
    if (kq > 0) s1[(half - kq) * nf + j] = mk(accr, acci);                     // k' = -kq: the conjugate
}

// stage 2, nf one of the row-transform lengths: natural frequency k goes to column (k + nf/2) mod nf
struct SlowShiftStore {
    static constexpr bool kPair = false;
    cplx* out; int n;
    struct Slot {
        cplx* row; int n;
        __device__ inline void operator()(int k, cplx v) const {
            int c = k + n / 2;
            if (c >= n) c -= n;
            row[c] = v;
        }
    };
    __device__ inline Slot open(int64_t s) const { return Slot{out + s * n, n}; }
};

// stage 2, any other nf: out[r, (m + nf/2) mod nf] = sum_j S1[r, j] W_nf^((j m) mod nf).  Lanes along m; the row is wave-uniform.
__global__ void __launch_bounds__(256)
slowft_dft_kernel(const cplx* __restrict__ s1, const cplx* __restrict__ tw, cplx* __restrict__ out, int64_t nf) {
    const int64_t r = blockIdx.x, m = (int64_t)blockIdx.y * 256 + threadIdx.x;
    if (m >= nf) return;
    const cplx* __restrict__ row = s1 + r * nf;
    int64_t idx = 0;                                        // (j m) mod nf
    cplx acc = mk(0.0, 0.0);
    for (int64_t j = 0; j < nf; ++j) {
        acc = acc + row[j] * gload(tw + idx);
        idx += m;
        if (idx >= nf) idx -= nf;
    }
    int64_t c = m + nf / 2;
    if (c >= nf) c -= nf;
    out[r * nf + c] = acc;
}

}  // namespace scint
