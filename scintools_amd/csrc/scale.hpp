// scale.hpp -- the velocity and trapezoid rescalings of Dynspec.scale_dyn (dynspec.py:3961-4128), DESIGN.md section 4n.
//
//   scint_spline_resample_rows   not-a-knot cubic spline along the contiguous TIME axis of every channel (dynspec.py:4062-4074)
//     spline_rows_kernel         a workgroup owns up to kRowsMax rows x one block of knots: the tile is loaded coalesced into LDS
//                                (row stride odd), one lane per row runs the two Thomas sweeps in place there, all lanes evaluate
//                                the block's targets from the moments in LDS and store them coalesced.  No workspace.
//     spline_rows_seq_kernel     one sequential sweep per row through a workspace of nf*nt doubles, for a single block that does not
//     + spline_rows_eval_kernel  fit the LDS tile (an axis too uneven to block AND longer than kRowsLds - 4 knots)
//   scint_trap_scale             the trapezoid rescale in one pass (dynspec.py:4081-4128): mean, windows, np.linspace, np.interp
//
// Everything below is compiled without floating-point contraction: np.interp's slope*(x - xp[j]) + fp[j], np.linspace's
// j*step + start and the two window products must round like NumPy.
#pragma once
#pragma clang fp contract(off)
#include <math.h>

#include <algorithm>

#include "common.hpp"

namespace scint {

constexpr int kRowsThreads = 256;
constexpr int kRowsLds = 7680;        // doubles of LDS one workgroup of spline_rows_kernel holds (60 KiB: two workgroups per CU)
constexpr int kRowsMax = 64;          // rows of one workgroup: one lane each in the sweeps, so one wavefront at the most

struct RowSpline {
    const double* h;    // [nt-1] knot spacings
    const double* sub;  // [nt] sub-diagonal of the interior rows 1..nt-2
    const double* inv;  // [nt] 1 / pivot
    const double* sup;  // [nt] Thomas c'
    double e0, e1, e2, e3;
};

// first target j in [0, nout) with idx[j] >= k (idx is non-decreasing)
__device__ inline int64_t first_target(const int32_t* idx, int64_t nout, int64_t k) {
    int64_t lo = 0, hi = nout;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)gload(idx + mid) < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// blockIdx.x = block of `block` interior knots [first, last), blockIdx.y = group of `rt` rows.  The block evaluates the targets
// whose interval starts at a knot in [first-1, last-1) (the last block also the last interval), so it needs the moments of the
// knots [first-1, last]: the forward sweep starts `warm` knots before that range from zero, the backward sweep `warm` knots
// after it, and by then either has forgotten its start (the caller sizes `warm` from the factors).  tile[r*stride + (i - base)]
// holds y[i], then d[i], then M[i] of row r; stride is odd, so the lanes of a sweep (one row each) hit distinct banks.
__global__ void __launch_bounds__(kRowsThreads)
spline_rows_kernel(const double* __restrict__ dyn, int64_t nf, int64_t nt, RowSpline s, int64_t block, int64_t warm, int rt,
                   int stride, const int32_t* __restrict__ idx, const double* __restrict__ coef, int64_t nout,
                   double* __restrict__ out) {
    __shared__ double tile[kRowsLds];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.y * rt;
    const int nrows = (int)min((int64_t)rt, nf - r0);
    const int64_t first = 1 + (int64_t)blockIdx.x * block;
    const int64_t last = min(first + block, nt - 1);
    const int64_t lo = max((int64_t)1, first - 1), hi = min(nt - 2, last);      // moments wanted on the interior knots [lo, hi]
    const int64_t i0 = max((int64_t)1, lo - warm), i1 = min(nt - 2, hi + warm);
    const int64_t base = i0 - 1;
    const int span = (int)(i1 - i0 + 3);                                        // knots [i0-1, i1+1]; span <= stride
    // ---- the tile, coalesced along time
    for (int e = tid; e < nrows * span; e += kRowsThreads) {
        const int r = e / span, j = e - r * span;
        tile[r * stride + j] = gload(dyn + (r0 + r) * nt + base + j);
    }
    __syncthreads();
    // ---- the two sweeps, one lane per row, in place
    if (tid < nrows) {
        double* t = tile + tid * stride;
        double y_prev = t[0], y_cur = t[1], d = 0.0;
        for (int64_t i = i0; i <= i1; ++i) {
            const int j = (int)(i - base);
            const double y_next = t[j + 1];
            const double r = 6.0 * ((y_next - y_cur) / gload(s.h + i) - (y_cur - y_prev) / gload(s.h + i - 1));
            d = (r - gload(s.sub + i) * d) * gload(s.inv + i);
            t[j] = d;
            y_prev = y_cur; y_cur = y_next;
        }
        double m = 0.0;          // exact at i1 == nt-2 (sup[nt-2] == 0), decayed away otherwise
        for (int64_t i = i1; i >= lo; --i) {
            const int j = (int)(i - base);
            m = t[j] - gload(s.sup + i) * m;
            t[j] = m;
        }
        if (first == 1) t[0] = s.e0 * t[1] + s.e1 * t[2];                                    // M[0]   (base == 0)
        if (last == nt - 1) t[span - 1] = s.e2 * t[span - 2] + s.e3 * t[span - 3];           // M[nt-1] (i1 == nt-2)
    }
    __syncthreads();
    // ---- the block's targets
    const int64_t k0 = first - 1, k1 = (last == nt - 1) ? nt - 1 : last - 1;    // intervals [k0, k1)
    const int64_t j0 = first_target(idx, nout, k0), j1 = first_target(idx, nout, k1);
    const int64_t ntar = j1 - j0;
    for (int64_t e = tid; e < (int64_t)nrows * ntar; e += kRowsThreads) {
        const int r = (int)(e / ntar);
        const int64_t j = j0 + (e - r * ntar);
        const int64_t k = gload(idx + j);
        if (k < k0 || k >= k1) continue;                    // (only an idx that is not non-decreasing: nothing is read out of range)
        const double c0 = gload(coef + 4 * j), c1 = gload(coef + 4 * j + 1), c2 = gload(coef + 4 * j + 2), c3 = gload(coef + 4 * j + 3);
        const double* y = dyn + (r0 + r) * nt + k;
        const double* m = tile + r * stride + (k - base);
        const double v = c0 * gload(y) + c1 * gload(y + 1) + c2 * m[0] + c3 * m[1];
        gstore(out + (r0 + r) * nout + j, v);
    }
}

// One lane per row, the whole axis in one sweep, moments into W[nf][nt]: the rare route of an axis that can neither be blocked
// nor held in LDS.  The accesses of a wavefront are nt doubles apart.
__global__ void __launch_bounds__(64)
spline_rows_seq_kernel(const double* __restrict__ dyn, int64_t nf, int64_t nt, RowSpline s, double* __restrict__ W) {
    const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (r >= nf) return;
    const double* y = dyn + r * nt;
    double* w = W + r * nt;
    double y_prev = gload(y), y_cur = gload(y + 1), d = 0.0;
    for (int64_t i = 1; i <= nt - 2; ++i) {
        const double y_next = gload(y + i + 1);
        const double q = 6.0 * ((y_next - y_cur) / gload(s.h + i) - (y_cur - y_prev) / gload(s.h + i - 1));
        d = (q - gload(s.sub + i) * d) * gload(s.inv + i);
        gstore(w + i, d);
        y_prev = y_cur; y_cur = y_next;
    }
    double m = 0.0, m1 = 0.0, m2 = 0.0;
    for (int64_t i = nt - 2; i >= 1; --i) {
        m = gload(w + i) - gload(s.sup + i) * m;
        gstore(w + i, m);
        if (i == 2) m2 = m;
        if (i == 1) m1 = m;
    }
    gstore(w, s.e0 * m1 + s.e1 * m2);
    gstore(w + nt - 1, s.e2 * gload(w + nt - 2) + s.e3 * gload(w + nt - 3));
}

// blockIdx.y = row, threads along the targets
__global__ void __launch_bounds__(256)
spline_rows_eval_kernel(const double* __restrict__ dyn, const double* __restrict__ W, int64_t nt, const int32_t* __restrict__ idx,
                        const double* __restrict__ coef, int64_t nout, double* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t r = blockIdx.y;
    if (j >= nout) return;
    const int64_t k = min(max((int64_t)gload(idx + j), (int64_t)0), nt - 2);
    const double c0 = gload(coef + 4 * j), c1 = gload(coef + 4 * j + 1), c2 = gload(coef + 4 * j + 2), c3 = gload(coef + 4 * j + 3);
    const double* y = dyn + r * nt + k;
    const double* m = W + r * nt + k;
    gstore(out + r * nout + j, c0 * gload(y) + c1 * gload(y + 1) + c2 * gload(m) + c3 * gload(m + 1));
}

// Rows one workgroup of spline_rows_kernel takes and their LDS stride for blocks of `block` knots with `warm` knots of warm-up
// (block <= 0: one block of all nt-2 interior knots); rt == 0: the tile does not fit, the sequential route runs.
inline void spline_rows_tile(int64_t nt, int64_t block, int64_t warm, int64_t* block_out, int* rt, int* stride) {
    const int64_t rows = nt - 2;
    if (block <= 0 || block >= rows) { block = rows; warm = 0; }
    const int64_t span = std::min(block + 2 * warm + 4, nt);
    *block_out = block;
    *stride = (int)(span | 1);
    *rt = span + 1 > kRowsLds ? 0 : (int)std::min<int64_t>(kRowsMax, kRowsLds / (span | 1));
}

// ------------------------------------------------------------------------------------------------------------------------
// trapezoid
// ------------------------------------------------------------------------------------------------------------------------
struct TrapRow {
    const double* row;      // dyn[f][:]
    const double* cw;       // [nt] or null
    const double* times;
    double mean, sw;
    bool windowed;
    // the windowed pixel in the reference's order: dyn -= mean; chan_window * dyn; subint_window * (.)  (dynspec.py:4083, 4106-4108)
    __device__ inline double fp(int64_t t) const {
        const double v = gload(row + t) - mean;
        return windowed ? (v * gload(cw + t)) * sw : v;
    }
    // np.interp(x, times, fp) for one finite x (numpy/_core/src/multiarray/compiled_base.c, arr_interp); times ascending
    __device__ inline double interp(double x, int64_t n, double inv_step) const {
        const double x_lo = gload(times), x_hi = gload(times + n - 1);
        if (n == 1) return fp(0);
        if (x > x_hi) return fp(n - 1);
        if (x < x_lo) return fp(0);
        // j = largest index with times[j] <= x: uniform-axis guess, a short walk, bisection otherwise
        const double g = floor((x - x_lo) * inv_step);
        int64_t j = (int64_t)fmin(fmax(g, 0.0), (double)(n - 1));
        int walk = 0;
        while (j > 0 && gload(times + j) > x && walk < 4) { --j; ++walk; }
        while (j < n - 1 && gload(times + j + 1) <= x && walk < 4) { ++j; ++walk; }
        if (gload(times + j) > x || (j < n - 1 && gload(times + j + 1) <= x)) {
            int64_t lo = 0, hi = n;             // first index with times > x is in [lo, hi]
            while (lo < hi) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                if (x >= gload(times + mid)) lo = mid + 1; else hi = mid;
            }
            j = lo - 1;
        }
        const double fj = fp(j);
        if (j == n - 1) return fj;
        const double xj = gload(times + j);
        if (xj == x) return fj;
        const double xj1 = gload(times + j + 1), fj1 = fp(j + 1);
        const double slope = (fj1 - fj) / (xj1 - xj);
        double r = slope * (x - xj) + fj;
        if (r != r) {
            r = slope * (x - xj1) + fj1;
            if (r != r && fj == fj1) r = fj;
        }
        return r;
    }
};

// blockIdx.y = channel, threads along the output samples.  np.linspace(tmin, tmax, n) as NumPy forms it (function_base.py):
// step = (tmax - tmin)/(n - 1); y = j*step (or (j/(n-1))*(tmax - tmin) when step == 0); y += tmin; y[n-1] = tmax.
__global__ void __launch_bounds__(256)
trap_scale_kernel(const double* __restrict__ dyn, int64_t nf, int64_t nt, double mean, const double* __restrict__ cw,
                  const double* __restrict__ sw, const double* __restrict__ times, const int32_t* __restrict__ nkeep,
                  double* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t f = blockIdx.y;
    if (j >= nt) return;
    const int64_t n = min((int64_t)max(gload(nkeep + f), 0), nt);
    double v = 0.0;
    if (j < n) {
        const double tmin = gload(times), tmax = gload(times + nt - 1);
        double x = tmin;
        if (n > 1) {
            const double delta = tmax - tmin, div = (double)(n - 1);
            const double step = delta / div;
            double y = (double)j;
            y = (step == 0.0) ? (y / div) * delta : y * step;
            x = (j == n - 1) ? tmax : y + tmin;
        }
        TrapRow row{dyn + f * nt, cw, times, mean, (cw && sw) ? gload(sw + f) : 1.0, cw && sw};
        const double inv_step = (nt > 1 && tmax > tmin) ? (double)(nt - 1) / (tmax - tmin) : 0.0;
        v = row.interp(x, nt, inv_step);
    }
    gstore(out + f * nt + j, v);
}

}  // namespace scint
