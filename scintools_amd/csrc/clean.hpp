// clean.hpp -- dynamic-spectrum cleaning: Dynspec.zap, refill, correct_dyn (dynspec.py:3856-3870, 3273-3323, 3325-3410) and
// ththmod.svd_model.  Included from arcnorm.hip (-ffp-contract=off: x - median, slope * dx + v0 and a / b round as NumPy's do).
//
//   zap       exact order statistics of float64 by radix select on the order-preserving 64-bit key, NaN excluded: eight passes
//             of 8 bits, most significant first.  zap_hist_kernel counts the byte under the already fixed prefix (LDS histogram,
//             one integer atomic per non-empty bin and workgroup: integer sums, so the result does not depend on their order);
//             zap_pick_kernel (one thread) walks the 256 bins to the bin that holds the wanted rank and extends the prefix.  The
//             two middle ranks of an even count are selected side by side in the same passes.  The second median is that of
//             |x - median|, formed on the fly.  zap_apply_kernel writes NaN where |x - median| / mdev > sigma.
//             Traffic: 17 reads of the array and one sparse write; no copy of the array, no sort.
//   refill    refill_median_kernel: a 16 x 16 tile with its halo in LDS (zero padding, NaN -> fill); only tiles that hold a NaN
//             load the halo, and only NaN pixels select: the element of rank kf kt / 2 by counting, no sorting network, any odd
//             kf x kt <= 225.  refill_linear_kernel: a pixel of an invalid line walks the validity flags to the bracketing valid
//             lines and interpolates with np.interp's arithmetic; a gap that touches the edge stays NaN.
//   svd       top-p right singular subspace of the real nf x nt array by block iteration on A^T A: svd_av_kernel T = A V (one
//             wave per row), svd_aty_kernel Y = A^T T (one thread per column, row blocks into partial sums that svd_reduce_kernel adds
//             in a fixed order: no atomics), svd_step_kernel (one workgroup): H = V^T Y, the residual |Y - V H|_F, the eigenvalues of
//             H by Jacobi, and V <- orth(Y) by two passes of modified Gram-Schmidt; a column that vanishes is deflated (rank
//             < p).  The model sum_k sigma_k u_k v_k^T equals (A V) V^T: svd_model_kernel forms it from T = A V and divides.
//             STOPPING RULE: |A^T A V - V H|_F <= tol * lambda_p with lambda_p the smallest eigenvalue of H among the columns
//             not deflated (the Ritz-residual rule of the eigenvalue sweeps, residual <= tol lambda on A^T A; the Python side
//             passes ththmod.DEFAULT_TOL = 1e-12).  Two reads of A per iteration, two more for the model pass.
//   nanmean   clean_row_nanmean_kernel / clean_col_nanmean_kernel + clean_col_final_kernel, clean_divide_kernel (svd=False).
#pragma once

namespace scint {

constexpr int kZapMaxBlocks = 1024;
constexpr int kMedTile = 16;
constexpr int kMedMaxWindow = 225;
constexpr int kMedLds = 3840;                       // max (15 + kf)(15 + kt) over odd kf kt <= 225
constexpr int kSvdMaxP = 8;
constexpr int kSvdMaxRowBlocks = 64;

// ------------------------------------------------------------------------------
// zap
// ------------------------------------------------------------------------------
struct ZapState {
    unsigned long long prefix[2];   // key bits fixed so far, of the lower and the upper middle element
    unsigned long long rank[2];     // wanted rank among the keys under that prefix
    unsigned long long count;       // non-NaN elements
    double value[2];                // [0] median of x, [1] median of |x - median|
    unsigned long long hist[2][256];
};

__device__ inline unsigned long long zap_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double zap_unkey(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

// mode 0: keys of x; mode 1: keys of |x - value[0]|.  shift = 56, 48, ..., 0.
__global__ void __launch_bounds__(256) zap_hist_kernel(const double* x, int64_t n, int mode, int shift, ZapState* st) {
    __shared__ unsigned int h[2][256];
    const int t = threadIdx.x;
    h[0][t] = 0; h[1][t] = 0;
    __syncthreads();
    const double med = mode ? st->value[0] : 0.0;
    const bool first = shift == 56;
    const unsigned long long p0 = first ? 0 : st->prefix[0] >> (shift + 8), p1 = first ? 0 : st->prefix[1] >> (shift + 8);
    for (int64_t i = (int64_t)blockIdx.x * 256 + t; i < n; i += (int64_t)gridDim.x * 256) {
        double v = gload(x + i);
        if (mode) v = fabs(v - med);
        if (v != v) continue;
        const unsigned long long k = zap_key(v), hi = first ? 0 : k >> (shift + 8);
        const int digit = (int)((k >> shift) & 255);
        if (hi == p0) atomicAdd(&h[0][digit], 1u);
        if (hi == p1) atomicAdd(&h[1][digit], 1u);
    }
    __syncthreads();
    if (h[0][t]) atomicAdd(&st->hist[0][t], (unsigned long long)h[0][t]);
    if (h[1][t]) atomicAdd(&st->hist[1][t], (unsigned long long)h[1][t]);
}

__global__ void zap_pick_kernel(int mode, int shift, ZapState* st) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (shift == 56) {
        unsigned long long total = 0;
        for (int b = 0; b < 256; ++b) total += st->hist[0][b];
        st->count = total;
        st->prefix[0] = st->prefix[1] = 0;
        st->rank[0] = total ? (total - 1) / 2 : 0;
        st->rank[1] = total / 2;
    }
    const unsigned long long total = st->count;
    if (total == 0) {                                   // np.median of nothing: NaN
        st->value[mode] = __longlong_as_double(0x7ff8000000000000ll);
    } else {
        for (int s = 0; s < 2; ++s) {
            unsigned long long r = st->rank[s], cum = 0;
            int digit = 255;
            for (int b = 0; b < 256; ++b) {
                const unsigned long long c = st->hist[s][b];
                if (r < cum + c) { digit = b; break; }
                cum += c;
            }
            st->rank[s] = r - cum;
            st->prefix[s] |= (unsigned long long)digit << shift;
        }
        if (shift == 0) {
            const double a = zap_unkey(st->prefix[0]), b = zap_unkey(st->prefix[1]);
            st->value[mode] = (total & 1) ? a : (a + b) / 2.0;      // np.mean of the middle pair
        }
    }
    for (int b = 0; b < 256; ++b) { st->hist[0][b] = 0; st->hist[1][b] = 0; }
}

__global__ void __launch_bounds__(256) zap_apply_kernel(double* x, int64_t n, double sigma, const ZapState* st) {
    const double med = st->value[0], mdev = st->value[1];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double d = fabs(gload(x + i) - med);
        if (d / mdev > sigma) gstore(x + i, __longlong_as_double(0x7ff8000000000000ll));
    }
}

// ------------------------------------------------------------------------------
// refill
// ------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
refill_median_kernel(const double* in, int64_t nf, int64_t nt, int kf, int kt, double fill, double* out) {
    __shared__ double tile[kMedLds];
    __shared__ int any;
    const int t = threadIdx.x, ty = t / kMedTile, tx = t % kMedTile;
    const int64_t r0 = (int64_t)blockIdx.y * kMedTile, c0 = (int64_t)blockIdx.x * kMedTile;
    const int64_t r = r0 + ty, c = c0 + tx;
    const bool inside = r < nf && c < nt;
    if (t == 0) any = 0;
    __syncthreads();
    double own = 0.0;
    if (inside) own = gload(in + r * nt + c);
    const bool hole = inside && own != own;
    if (hole) any = 1;                                  // every writer stores the same value
    if (inside && !hole) gstore(out + r * nt + c, own);
    __syncthreads();
    if (!any) return;                                   // uniform over the workgroup
    const int hf = kf / 2, ht = kt / 2, H = kMedTile + kf - 1, W = kMedTile + kt - 1;
    for (int e = t; e < H * W; e += 256) {
        const int64_t rr = r0 - hf + e / W, cc = c0 - ht + e % W;
        double v = 0.0;                                 // medfilt pads with zeros
        if (rr >= 0 && rr < nf && cc >= 0 && cc < nt) {
            v = gload(in + rr * nt + cc);
            if (v != v) v = fill;
        }
        tile[e] = v;
    }
    __syncthreads();
    if (!hole) return;
    const int want = (kf * kt) / 2;
    double res = fill;
    for (int a = 0; a < kf * kt; ++a) {
        const double va = tile[(ty + a / kt) * W + tx + a % kt];
        int less = 0, eq = 0;
        for (int i = 0; i < kf; ++i) {
            const double* row = tile + (ty + i) * W + tx;
            for (int j = 0; j < kt; ++j) {
                const double vb = row[j];
                less += vb < va;
                eq += vb == va;
            }
        }
        if (less <= want && want < less + eq) { res = va; break; }
    }
    gstore(out + r * nt + c, res);
}

// axis 0: the lines are rows (channels), a gap is filled along the column; axis 1: the lines are columns.
__global__ void __launch_bounds__(256)
refill_linear_kernel(double* a, int64_t nf, int64_t nt, int axis, const uint8_t* valid) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= nt) return;
    for (int64_t r = blockIdx.y; r < nf; r += gridDim.y) {
        const int64_t line = axis == 0 ? r : c, nline = axis == 0 ? nf : nt;
        if (gload(valid + line)) continue;
        int64_t lo = line - 1, hi = line + 1;
        while (lo >= 0 && !gload(valid + lo)) --lo;
        while (hi < nline && !gload(valid + hi)) ++hi;
        if (lo < 0 || hi >= nline) continue;            // no bracket: stays NaN
        const double v0 = axis == 0 ? gload(a + lo * nt + c) : gload(a + r * nt + lo);
        const double v1 = axis == 0 ? gload(a + hi * nt + c) : gload(a + r * nt + hi);
        const double slope = (v1 - v0) / (double)(hi - lo);
        gstore(a + r * nt + c, slope * (double)(line - lo) + v0);
    }
}

// ------------------------------------------------------------------------------
// truncated SVD by block iteration on A^T A.  V, Y: [kSvdMaxP][nt]; T: [nf][kSvdMaxP].
// ------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
svd_av_kernel(const double* a, int64_t nf, int64_t nt, const double* V, int p, double* T) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nf) return;                              // a whole wave leaves together
    double acc[kSvdMaxP];
#pragma unroll
    for (int k = 0; k < kSvdMaxP; ++k) acc[k] = 0.0;
    for (int64_t j = lane; j < nt; j += 64) {
        const double x = gload(a + row * nt + j);
#pragma unroll
        for (int k = 0; k < kSvdMaxP; ++k)
            if (k < p) acc[k] += x * gload(V + k * nt + j);
    }
#pragma unroll
    for (int k = 0; k < kSvdMaxP; ++k) {
        const double s = wave_sum(acc[k]);
        if (lane == 0) gstore(T + row * kSvdMaxP + k, k < p ? s : 0.0);
    }
}

__global__ void __launch_bounds__(256)
svd_aty_kernel(const double* a, int64_t nf, int64_t nt, const double* T, int p, int64_t rows_per_block, double* part) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nt) return;
    const int64_t i0 = (int64_t)blockIdx.y * rows_per_block, i1 = min(i0 + rows_per_block, nf);
    double acc[kSvdMaxP];
#pragma unroll
    for (int k = 0; k < kSvdMaxP; ++k) acc[k] = 0.0;
    for (int64_t i = i0; i < i1; ++i) {
        const double x = gload(a + i * nt + j);
#pragma unroll
        for (int k = 0; k < kSvdMaxP; ++k)
            if (k < p) acc[k] += x * T[i * kSvdMaxP + k];
    }
#pragma unroll
    for (int k = 0; k < kSvdMaxP; ++k)
        if (k < p) gstore(part + ((int64_t)blockIdx.y * kSvdMaxP + k) * nt + j, acc[k]);
}

// Y[k][j] = sum of the row blocks' partial sums, in block order (blockIdx.y = k)
__global__ void __launch_bounds__(256) svd_reduce_kernel(const double* part, int nblk, int64_t nt, double* Y) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y;
    if (j >= nt) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += gload(part + ((int64_t)b * kSvdMaxP + k) * nt + j);
    gstore(Y + k * nt + j, s);
}

struct SvdStatus {
    double res;        // |Y - V H|_F of the V this step started from
    double lam_min;    // smallest eigenvalue of H among the active columns
    double lam_max;
    double active;     // columns of the new V that are not deflated
    double lam[kSvdMaxP];
};

// eigenvalues of the symmetric p x p matrix h (row-major, stride kSvdMaxP), descending, by cyclic Jacobi
__device__ inline void svd_jacobi(double* h, int p, double* lam) {
    for (int sweep = 0; sweep < 12; ++sweep) {
        for (int i = 0; i < p - 1; ++i) {
            for (int j = i + 1; j < p; ++j) {
                const double hij = h[i * kSvdMaxP + j];
                if (hij == 0.0) continue;
                const double theta = (h[j * kSvdMaxP + j] - h[i * kSvdMaxP + i]) / (2.0 * hij);
                const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
                for (int k = 0; k < p; ++k) {           // columns i, j
                    const double hki = h[k * kSvdMaxP + i], hkj = h[k * kSvdMaxP + j];
                    h[k * kSvdMaxP + i] = c * hki - s * hkj;
                    h[k * kSvdMaxP + j] = s * hki + c * hkj;
                }
                for (int k = 0; k < p; ++k) {           // rows i, j
                    const double hik = h[i * kSvdMaxP + k], hjk = h[j * kSvdMaxP + k];
                    h[i * kSvdMaxP + k] = c * hik - s * hjk;
                    h[j * kSvdMaxP + k] = s * hik + c * hjk;
                }
            }
        }
    }
    for (int i = 0; i < p; ++i) lam[i] = h[i * kSvdMaxP + i];
    for (int i = 1; i < p; ++i) {                       // insertion sort, descending
        const double v = lam[i];
        int j = i - 1;
        while (j >= 0 && lam[j] < v) { lam[j + 1] = lam[j]; --j; }
        lam[j + 1] = v;
    }
}

__global__ void __launch_bounds__(256)
svd_step_kernel(int64_t nt, int p, double* V, double* Y, SvdStatus* status) {
    __shared__ double red[4];
    __shared__ double H[kSvdMaxP * kSvdMaxP];
    __shared__ double lam[kSvdMaxP];
    const int t = threadIdx.x;
    // H = V^T Y
    for (int k = 0; k < p; ++k)
        for (int l = 0; l < p; ++l) {
            double s = 0.0;
            for (int64_t j = t; j < nt; j += 256) s += V[k * nt + j] * Y[l * nt + j];
            s = block_sum(s, red);
            if (t == 0) H[k * kSvdMaxP + l] = s;
        }
    __syncthreads();
    // residual of the old basis
    double r2 = 0.0;
    for (int l = 0; l < p; ++l)
        for (int64_t j = t; j < nt; j += 256) {
            double v = Y[l * nt + j];
            for (int k = 0; k < p; ++k) v -= V[k * nt + j] * H[k * kSvdMaxP + l];
            r2 += v * v;
        }
    r2 = block_sum(r2, red);
    __syncthreads();
    if (t == 0) {
        for (int k = 0; k < p; ++k)
            for (int l = k + 1; l < p; ++l) {
                const double m = 0.5 * (H[k * kSvdMaxP + l] + H[l * kSvdMaxP + k]);
                H[k * kSvdMaxP + l] = m; H[l * kSvdMaxP + k] = m;
            }
        svd_jacobi(H, p, lam);
    }
    __syncthreads();
    // V <- orth(Y): modified Gram-Schmidt, twice; a column that vanishes against its predecessors is deflated
    int active = 0;
    for (int l = 0; l < p; ++l) {
        double n0 = 0.0;
        for (int64_t j = t; j < nt; j += 256) n0 += Y[l * nt + j] * Y[l * nt + j];
        n0 = block_sum(n0, red);
        for (int pass = 0; pass < 2; ++pass)
            for (int k = 0; k < l; ++k) {
                double s = 0.0;
                for (int64_t j = t; j < nt; j += 256) s += V[k * nt + j] * Y[l * nt + j];
                s = block_sum(s, red);
                for (int64_t j = t; j < nt; j += 256) Y[l * nt + j] -= s * V[k * nt + j];
            }
        double n1 = 0.0;
        for (int64_t j = t; j < nt; j += 256) n1 += Y[l * nt + j] * Y[l * nt + j];
        n1 = block_sum(n1, red);
        const bool dead = !(n1 > 1e-26 * n0);            // also n0 == 0 and NaN
        const double scale = dead ? 0.0 : 1.0 / sqrt(n1);
        __syncthreads();
        for (int64_t j = t; j < nt; j += 256) V[l * nt + j] = dead ? 0.0 : Y[l * nt + j] * scale;
        __syncthreads();
        active += dead ? 0 : 1;
    }
    if (t == 0) {
        status->res = sqrt(r2);
        status->lam_max = lam[0];
        status->lam_min = active > 0 ? lam[active - 1] : 0.0;
        status->active = (double)active;
        for (int k = 0; k < kSvdMaxP; ++k) status->lam[k] = k < p ? lam[k] : 0.0;
    }
}

// model = T V (T = A V), corrected = a / |model|; either output may be null
__global__ void __launch_bounds__(256)
svd_model_kernel(const double* a, int64_t nf, int64_t nt, const double* T, const double* V, int p, double* model,
                 double* corrected) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nt) return;
    for (int64_t i = blockIdx.y; i < nf; i += gridDim.y) {
        double m = 0.0;
        for (int k = 0; k < p; ++k) m += T[i * kSvdMaxP + k] * gload(V + k * nt + j);
        if (model) gstore(model + i * nt + j, m);
        if (corrected) gstore(corrected + i * nt + j, gload(a + i * nt + j) / fabs(m));
    }
}

// ------------------------------------------------------------------------------
// nanmean along an axis, divide along an axis (correct_dyn, svd=False)
// ------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) clean_row_nanmean_kernel(const double* a, int64_t nf, int64_t nt, double* out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nf) return;
    double s = 0.0, cnt = 0.0;
    for (int64_t j = lane; j < nt; j += 64) {
        const double x = gload(a + row * nt + j);
        if (x == x) { s += x; cnt += 1.0; }
    }
    s = wave_sum(s); cnt = wave_sum(cnt);
    if (lane == 0) gstore(out + row, s / cnt);
}

__global__ void __launch_bounds__(256)
clean_col_nanmean_kernel(const double* a, int64_t nf, int64_t nt, int64_t rows_per_block, double* part) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nt) return;
    const int64_t i0 = (int64_t)blockIdx.y * rows_per_block, i1 = min(i0 + rows_per_block, nf);
    double s = 0.0, cnt = 0.0;
    for (int64_t i = i0; i < i1; ++i) {
        const double x = gload(a + i * nt + j);
        if (x == x) { s += x; cnt += 1.0; }
    }
    gstore(part + (int64_t)blockIdx.y * 2 * nt + j, s);
    gstore(part + ((int64_t)blockIdx.y * 2 + 1) * nt + j, cnt);
}

__global__ void __launch_bounds__(256) clean_col_final_kernel(const double* part, int nblk, int64_t nt, double* out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nt) return;
    double s = 0.0, cnt = 0.0;
    for (int b = 0; b < nblk; ++b) {
        s += gload(part + (int64_t)b * 2 * nt + j);
        cnt += gload(part + ((int64_t)b * 2 + 1) * nt + j);
    }
    gstore(out + j, s / cnt);
}

// a[i][j] /= v[i] (axis 0) or v[j] (axis 1)
__global__ void __launch_bounds__(256) clean_divide_kernel(double* a, int64_t nf, int64_t nt, int axis, const double* v) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nt) return;
    for (int64_t i = blockIdx.y; i < nf; i += gridDim.y)
        gstore(a + i * nt + j, gload(a + i * nt + j) / gload(v + (axis == 0 ? i : j)));
}

}  // namespace scint
