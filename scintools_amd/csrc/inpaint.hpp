// inpaint.hpp -- biharmonic inpainting of flagged pixels (Dynspec.inpaint; the method of Dynspec.refill(method='biharmonic'),
// dynspec.py:3301-3307, scikit-image's inpaint_biharmonic without a split into regions).  Included from arcnorm.hip.  float64.
//
//   system    L = the 5-point Laplacian of the [nf][nt] image with reflecting edges (scipy.ndimage.laplace, mode='reflect'), a
//             symmetric matrix.  With m the masked and k the known pixels the fill solves A u_m = b, A = (L^2)_mm,
//             b = -(L^2)_mk u_k.  A is a principal submatrix of L^2: symmetric, and positive definite once a pixel is known.
//             Row p of L^2 is one of 25 stencils of 5 x 5 (13 non-zero in the interior: 20, -8, 2, 1): each axis has the classes
//             "0 or 1 from the near edge, interior, 1 or 0 from the far edge", so nf, nt >= 5.  The host makes the table once.
//   compact   inpaint_count_kernel (masked pixels per 1024-pixel block), inpaint_scan_kernel (one workgroup: exclusive scan of
//             the block counts, the total), inpaint_fill_kernel (index image pixel -> unknown or -1, list unknown -> pixel):
//             unknowns are numbered in pixel order, whatever the launch shape.
//   stencil   inpaint_row<F>: the at most 13 neighbours of one unknown through the index image, coefficients from the table in
//             LDS.  The same body forms b (known neighbours), q = A p (unknown neighbours) and the true residual b - A x.
//   CG        two launches a step.  inpaint_ap_kernel: beta = rho / rho_prev from the partial sums of the last step (every
//             workgroup adds the same partials in the same order), p = r + beta p_old written to the other p buffer and formed
//             on the fly at the neighbours, q = A p, partial sums of p.q.  inpaint_update_kernel: alpha = rho / p.q, x += alpha p,
//             r -= alpha q, partial sums of r.r.  No atomics, one fixed order of every sum: equal inputs give equal bits.
//             STOPPING RULE: when |r|_2 <= tol |b|_2 the step kernels stop doing work (two flags, each written by one launch and
//             read by later ones only); the host, which reads the state every kCgCheck steps, then has inpaint_true_kernel
//             form r = b - A x and either accepts it or continues from it with p = r.
//   traffic   per step and unknown: 84 bytes streamed (list, r, p_old, p, q; x, r, p, q read, x, r written) and 13 index reads
//             of 4 bytes plus the neighbours' r and p_old, which come from the caches (the vectors of a 1 % mask fit the L2).
#pragma once

namespace scint {

constexpr int kInpaintChunk = 1024;         // pixels per workgroup of the compaction: 256 threads x 4
constexpr int kCgMaxBlocks = 1024;          // workgroups of a CG launch = partial sums of a dot product
constexpr int kCgCheck = 8;                 // the host reads the state every kCgCheck steps

struct InpaintState {
    double bnorm2;       // b.b
    double thresh2;      // tol^2 b.b
    double rho;          // r.r as the last step (or probe) saw it
    double true_rho;     // r.r of the last true residual b - A x
    int32_t count;       // masked pixels found by the compaction
    int32_t iters;       // steps done
    int32_t done_a;      // written by inpaint_ap_kernel / inpaint_probe_kernel: rho <= thresh2 (or not finite)
    int32_t done_b;      // written by inpaint_update_kernel: done_a of the launch before
};

// ---- compaction ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) inpaint_count_kernel(const uint8_t* mask, int64_t n, int32_t* counts) {
    __shared__ int red[4];
    const int64_t base = (int64_t)blockIdx.x * kInpaintChunk + threadIdx.x * 4;
    int c = 0;
    for (int e = 0; e < 4; ++e)
        if (base + e < n) c += gload(mask + base + e) != 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// exclusive scan of counts[nblk] in place, one workgroup; the total goes to st->count
__global__ void __launch_bounds__(256) inpaint_scan_kernel(int32_t* counts, int64_t nblk, InpaintState* st) {
    __shared__ int s[256];
    __shared__ int carry;
    const int t = threadIdx.x;
    if (t == 0) carry = 0;
    __syncthreads();
    for (int64_t b0 = 0; b0 < nblk; b0 += 256) {
        const int own = b0 + t < nblk ? counts[b0 + t] : 0;
        s[t] = own;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const int add = t >= o ? s[t - o] : 0;
            __syncthreads();
            s[t] += add;
            __syncthreads();
        }
        const int before = carry;
        if (b0 + t < nblk) counts[b0 + t] = before + s[t] - own;
        __syncthreads();
        if (t == 255) carry = before + s[255];
        __syncthreads();
    }
    if (t == 0) st->count = carry;
}

// index[pixel] = its number among the masked pixels or -1; list[number] = pixel.  `cap` bounds the list (the caller's nmask).
__global__ void __launch_bounds__(256)
inpaint_fill_kernel(const uint8_t* mask, int64_t n, const int32_t* offsets, int64_t cap, int32_t* index, int32_t* list) {
    __shared__ int s[256];
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * kInpaintChunk + t * 4;
    bool m[4];
    int own = 0;
    for (int e = 0; e < 4; ++e) {
        m[e] = base + e < n && gload(mask + base + e) != 0;
        own += m[e];
    }
    s[t] = own;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int add = t >= o ? s[t - o] : 0;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    int64_t k = (int64_t)offsets[blockIdx.x] + s[t] - own;
    for (int e = 0; e < 4; ++e) {
        if (base + e >= n) break;
        int32_t v = -1;
        if (m[e]) {
            if (k < cap) { list[k] = (int32_t)(base + e); v = (int32_t)k; }
            ++k;
        }
        index[base + e] = v;
    }
}

// ---- the stencil -----------------------------------------------------------------------------------------------------------------
__device__ inline int inpaint_class(int64_t i, int64_t n) { return i < 2 ? (int)i : (i >= n - 2 ? (int)(4 - (n - 1 - i)) : 2); }

__device__ inline void inpaint_load_table(const double* table, double* tab) {
    for (int e = threadIdx.x; e < 625; e += blockDim.x) tab[e] = gload(table + e);
    __syncthreads();
}

// sum over the neighbours q of pixel `pix` of coefficient * f(q, index[q]); f sees every in-range pixel of the 13-point diamond
template <class F>
__device__ inline double inpaint_row(const double* tab, const int32_t* index, int64_t nf, int64_t nt, int64_t pix, F&& f) {
    const int64_t r = pix / nt, c = pix - r * nt;
    const double* st = tab + (inpaint_class(r, nf) * 5 + inpaint_class(c, nt)) * 25;
    double acc = 0.0;
#pragma unroll
    for (int dr = -2; dr <= 2; ++dr) {
        const int w = 2 - (dr < 0 ? -dr : dr);
#pragma unroll
        for (int dc = -2; dc <= 2; ++dc) {
            if (dc < -w || dc > w) continue;
            const int64_t rr = r + dr, cc = c + dc;
            if (rr < 0 || rr >= nf || cc < 0 || cc >= nt) continue;
            const int64_t q = rr * nt + cc;
            acc += st[(dr + 2) * 5 + dc + 2] * f(q, gload(index + q));
        }
    }
    return acc;
}

// the sum of part[0 .. n) in one fixed order, the same in every workgroup (256 threads)
__device__ inline double inpaint_total(const double* part, int n, double* red) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += gload(part + i);
    return block_sum(s, red);
}

// b = -(L^2)_mk u_k, r = b, x = 0; partial sums of b.b
__global__ void __launch_bounds__(256)
inpaint_rhs_kernel(const double* dyn, int64_t nf, int64_t nt, const double* table, const int32_t* index, const int32_t* list,
                   int64_t n, double* b, double* r, double* x, double* part) {
    __shared__ double tab[625];
    __shared__ double red[4];
    inpaint_load_table(table, tab);
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double v = -inpaint_row(tab, index, nf, nt, gload(list + i),
                                      [&](int64_t q, int32_t j) { return j < 0 ? gload(dyn + q) : 0.0; });
        gstore(b + i, v); gstore(r + i, v); gstore(x + i, 0.0);
        acc += v * v;
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// one workgroup: the state from the partial sums of b.b
__global__ void __launch_bounds__(256) inpaint_init_kernel(const double* part, int nparts, double tol, InpaintState* st) {
    __shared__ double red[4];
    const double bb = inpaint_total(part, nparts, red);
    if (threadIdx.x == 0) {
        st->bnorm2 = bb; st->thresh2 = tol * tol * bb; st->rho = bb; st->true_rho = bb;
        st->iters = 0; st->done_a = 0; st->done_b = 0;
    }
}

// r = b - A x; partial sums of r.r; the flags are cleared (no other launch runs beside this one)
__global__ void __launch_bounds__(256)
inpaint_true_kernel(int64_t nf, int64_t nt, const double* table, const int32_t* index, const int32_t* list, int64_t n,
                    const double* b, const double* x, double* r, double* part, InpaintState* st) {
    __shared__ double tab[625];
    __shared__ double red[4];
    inpaint_load_table(table, tab);
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double ax = inpaint_row(tab, index, nf, nt, gload(list + i),
                                      [&](int64_t, int32_t j) { return j >= 0 ? gload(x + j) : 0.0; });
        const double v = gload(b + i) - ax;
        gstore(r + i, v);
        acc += v * v;
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
    if (blockIdx.x == 0 && threadIdx.x == 0) { st->done_a = 0; st->done_b = 0; }
}

// one workgroup: rho = the sum of the partial r.r; done_a when it is within the bound (or not finite)
__global__ void __launch_bounds__(256) inpaint_probe_kernel(const double* rr, int nparts, int is_true, InpaintState* st) {
    __shared__ double red[4];
    if (st->done_a) return;                             // a step has stopped already: rho is the one it saw
    const double rho = inpaint_total(rr, nparts, red);
    if (threadIdx.x == 0) {
        st->rho = rho;
        if (is_true) st->true_rho = rho;
        if (!(rho > st->thresh2)) st->done_a = 1;
    }
}

// p = r + beta p_old, q = A p, partial sums of p.q.  rr: the partial r.r of the last step, rr_prev: of the one before.
__global__ void __launch_bounds__(256)
inpaint_ap_kernel(int64_t nf, int64_t nt, const double* table, const int32_t* index, const int32_t* list, int64_t n,
                  const double* r, const double* p_old, double* p, double* q, const double* rr, const double* rr_prev,
                  int nparts, int first, int step, double* pq, InpaintState* st) {
    __shared__ double tab[625];
    __shared__ double red[4];
    if (st->done_b) return;                             // (written by an earlier launch)
    const double rho = inpaint_total(rr, nparts, red);
    if (!(rho > st->thresh2)) {                         // the same sum in every workgroup: they all leave
        if (blockIdx.x == 0 && threadIdx.x == 0) { st->rho = rho; st->done_a = 1; }
        return;
    }
    double beta = 0.0;
    if (!first) {
        __syncthreads();
        beta = rho / inpaint_total(rr_prev, nparts, red);
    }
    inpaint_load_table(table, tab);
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double pi = first ? gload(r + i) : gload(r + i) + beta * gload(p_old + i);
        const double qi = inpaint_row(tab, index, nf, nt, gload(list + i), [&](int64_t, int32_t j) {
            if (j < 0) return 0.0;
            return first ? gload(r + j) : gload(r + j) + beta * gload(p_old + j);
        });
        gstore(p + i, pi); gstore(q + i, qi);
        acc += pi * qi;
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) pq[blockIdx.x] = acc;
    if (blockIdx.x == 0 && threadIdx.x == 0) { st->rho = rho; st->iters = step; }
}

// alpha = rho / p.q, x += alpha p, r -= alpha q, partial sums of the new r.r into rr_next
__global__ void __launch_bounds__(256)
inpaint_update_kernel(int64_t n, const double* p, const double* q, const double* pq, int nparts, double* x, double* r,
                      double* rr_next, InpaintState* st) {
    __shared__ double red[4];
    if (st->done_a) {                                   // (written by the launch before this one)
        if (blockIdx.x == 0 && threadIdx.x == 0) st->done_b = 1;
        return;
    }
    const double alpha = st->rho / inpaint_total(pq, nparts, red);
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double ri = gload(r + i) - alpha * gload(q + i);
        gstore(x + i, gload(x + i) + alpha * gload(p + i));
        gstore(r + i, ri);
        acc += ri * ri;
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) rr_next[blockIdx.x] = acc;
}

__global__ void __launch_bounds__(256) inpaint_scatter_kernel(const double* x, const int32_t* list, int64_t n, double* dyn) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        gstore(dyn + gload(list + i), gload(x + i));
}

}  // namespace scint
