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
//
//   precond='lines' (scint_inpaint_biharmonic_lines): preconditioned conjugate gradients with the exact inverses of the
//             blocks of A on the whole channels and on the whole sub-integrations of the mask -- the kernels after
//             inpaint_scatter_kernel below.  The kernels of the plain route above are shared and unchanged.
#pragma once

#include "fft.hpp"

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

// ==================================================================================================================================
// The line-block preconditioner (precond='lines', scint_inpaint_biharmonic_lines).  float64; no atomics, every sum in one order.
//
//   M^-1 r = R_f^T A_ff^-1 R_f r + R_t^T A_tt^-1 R_t r + D^-1 r_rest.  W_f: the channels whose every pixel is masked, A_ff the block
//   of A on W_f x (all times).  L = L_f (x) I + I (x) L_t and the DCT-II along time diagonalises L_t (eigenvalues lam_k =
//   2 cos(pi k / nt) - 2), so A_ff is, per time mode k, ((L_f + lam_k I)^2)[W_f, W_f]: symmetric positive definite and pentadiagonal
//   in the compressed channel number.  W_t: the same with the axes exchanged.  D: the centre coefficient of the stencil of a masked
//   pixel that lies in no whole line.
//   lines     lines_row_count_kernel / lines_col_count_kernel (integer counts: is the line whole?), lines_list_kernel (one
//             workgroup: position of a line among the whole ones or -1, the list, the number).
//   "axis"    one set of whole lines: line l, point j is pixel lines[l] * line_stride + j * elem_stride (channels: nt, 1;
//             sub-integrations: 1, nt).  Both sets run the same kernels.
//   DCT       of n points through ONE complex row FFT (fft_rows_kernel) of the even-odd reordered line (v_j = x_2j,
//             v_(n-1-j) = x_(2j+1)): X_k = Re(e^(-i pi k / 2n) V_k); backwards V_k = e^(i pi k / 2n) (X_k - i X_(n-k)).  n a power of
//             two from 16: the row FFT itself.  Any other n: the chirp-z identity at m = the power of two >= 2 n - 1 (two row
//             FFTs; tables by lines_tables_kernel).  m <= 8192: n <= 4096, or n = 8192.  LinesLoad / LinesStore are the row FFT's
//             functors: they gather the unknowns of a line through the index image, apply the chirps and the half-sample
//             twiddles, and leave the coefficients as hat[line][mode] -- a wavefront's 64 modes read and write whole lines.
//   solve     lines_factor_kernel: one thread a mode, L D L^T without pivoting of the mode's pentadiagonal block, once per call
//             (1/d, l1, l2 as [line][mode]).  lines_solve_kernel: forward and back substitution in place on hat.
//   PCG       x0 = M^-1 b (the whole solve when the mask is whole lines along one axis).  A step: lines_ap_kernel (p = z + beta p_old
//             formed on the fly at the neighbours, q = A p, p.q), lines_update_kernel (x, r, r.r), the transforms and solves of
//             M^-1 r, lines_combine_kernel (z and r.z).  Flags, the host's look every kCgCheck steps and the true residual by
//             inpaint_true_kernel as in the plain route.
// ==================================================================================================================================
constexpr int kLinesMaxFft = 8192;          // the row FFT's longest transform
constexpr double kLinesPi = 3.141592653589793238462643;

struct InpaintLinesState {
    InpaintState s;      // first: the kernels of the plain route write it
    double rz;           // r.z of the step (written by lines_ap_kernel, read by lines_update_kernel)
    int32_t nlines[2];   // whole channels, whole sub-integrations found
};

// one set of whole lines and its buffers
struct LineAxis {
    int L;               // lines
    int n;               // points of a line = modes
    int m;               // length of the row FFT: n, or the chirp-z length
    int blue;            // chirp-z
    int64_t n_across;    // lines of the image along the other axis (the size of L_f for channels)
    int64_t line_stride, elem_stride;
    int32_t* lines;      // [L] ascending
    int32_t* pos;        // [n_across] position in `lines` or -1
    cplx* half;          // [n] e^(-i pi k / 2n)
    cplx* chirp;         // [n] e^(-i pi j^2 / n)
    cplx* bhat;          // [m] FFT_m of the conjugate chirp, wrapped
    cplx* buf;           // [L][m] between the two FFTs of the chirp-z route
    double* hat;         // [L][n] coefficients: [line][mode]
    double* val;         // [L][n] M^-1 r on the lines: [line][point]
    double* fac;         // [3][L][n]: 1 / d, l1, l2
};

__global__ void __launch_bounds__(256) lines_row_count_kernel(const uint8_t* mask, int64_t nt, int32_t* whole) {
    __shared__ int red[4];
    const uint8_t* row = mask + (int64_t)blockIdx.x * nt;
    int c = 0;
    for (int64_t j = threadIdx.x; j < nt; j += 256) c += gload(row + j) != 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) whole[blockIdx.x] = (int64_t)(red[0] + red[1] + red[2] + red[3]) == nt;
}

// lanes along the contiguous axis
__global__ void __launch_bounds__(256) lines_col_count_kernel(const uint8_t* mask, int64_t nf, int64_t nt, int32_t* whole) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= nt) return;
    int64_t cnt = 0;
    for (int64_t r = 0; r < nf; ++r) cnt += gload(mask + r * nt + c) != 0;
    whole[c] = cnt == nf;
}

// one workgroup: pos[i] = the number of line i among the whole ones or -1, list[number] = i (`cap` bounds the list), *count
__global__ void __launch_bounds__(256)
lines_list_kernel(const int32_t* whole, int64_t n, int64_t cap, int32_t* pos, int32_t* list, int32_t* count) {
    __shared__ int s[256];
    __shared__ int carry;
    const int t = threadIdx.x;
    if (t == 0) carry = 0;
    __syncthreads();
    for (int64_t b0 = 0; b0 < n; b0 += 256) {
        const int own = b0 + t < n ? whole[b0 + t] : 0;
        s[t] = own;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const int add = t >= o ? s[t - o] : 0;
            __syncthreads();
            s[t] += add;
            __syncthreads();
        }
        const int k = carry + s[t] - own;
        if (b0 + t < n) {
            pos[b0 + t] = own && k < cap ? k : -1;
            if (own && k < cap) list[k] = (int32_t)(b0 + t);
        }
        __syncthreads();
        if (t == 255) carry += s[255];
        __syncthreads();
    }
    if (t == 0) *count = carry;
}

// half[k] = e^(-i pi k / 2n); chirp-z: chirp[j] = e^(-i pi j^2 / n) (j^2 reduced modulo 2 n exactly) and, into b[m], its conjugate
// wrapped: b[j] = b[m - j] = conj(chirp[j]), zero elsewhere
__global__ void __launch_bounds__(256) lines_tables_kernel(int n, int m, int blue, cplx* half, cplx* chirp, cplx* b) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    double sn, cs;
    if (i < n) {
        sincos(kLinesPi * ((double)i / (2.0 * (double)n)), &sn, &cs);
        gstore(half + i, mk(cs, -sn));
    }
    if (!blue || i >= m) return;
    const int j = i < n ? i : (m - i < n ? m - i : -1);
    if (j < 0) { gstore(b + i, mk(0.0, 0.0)); return; }
    sincos(kLinesPi * ((double)(((int64_t)j * j) % (2 * (int64_t)n)) / (double)n), &sn, &cs);
    gstore(b + i, mk(cs, sn));
    if (i < n) gstore(chirp + i, mk(cs, -sn));
}

// the even-odd reordering of the one-FFT DCT: point j of v is point lines_perm(j, n) of the line
__device__ inline int lines_perm(int j, int n) { return 2 * j < n ? 2 * j : 2 * n - 2 * j - 1; }

enum { LINES_LD_PLAIN = 0, LINES_LD_VALUES = 1, LINES_LD_COEFFS = 2 };
enum { LINES_ST_PLAIN = 0, LINES_ST_MULB = 1, LINES_ST_COEFFS = 2, LINES_ST_VALUES = 3 };

// input of a row FFT.  PLAIN: src[slot][m].  VALUES: the unknowns r of line `slot`, reordered, zero from n on.  COEFFS:
// conj(V_k) = e^(-i pi k / 2n) (X_k + i X_(n-k)) from hat[slot][.].  The last two times chirp[j] on the chirp-z route.
struct LinesLoad {
    int mode, n, m, L, blue;
    const cplx* src;
    const double* r; const int32_t* index; const int32_t* lines; int64_t line_stride, elem_stride;
    const double* hat; const cplx* half; const cplx* chirp;
    struct Slot {
        const LinesLoad& p; int64_t base; int64_t s;
        __device__ inline cplx operator()(int j) const {
            if (p.mode == LINES_LD_PLAIN) return gload(p.src + s * p.m + j);
            if (j >= p.n) return mk(0.0, 0.0);
            cplx v;
            if (p.mode == LINES_LD_VALUES) {
                const int64_t pix = base + (int64_t)lines_perm(j, p.n) * p.elem_stride;
                v = mk(gload(p.r + gload(p.index + pix)), 0.0);
            } else {
                const double* h = p.hat + s * p.n;
                v = gload(p.half + j) * mk(gload(h + j), j > 0 ? gload(h + (p.n - j)) : 0.0);
            }
            if (p.blue) v = v * gload(p.chirp + j);
            return v;
        }
    };
    __device__ inline Slot open(int64_t slot) const {
        const int64_t s = slot < L ? slot : 0;          // (a slot beyond the last one is opened, never read)
        return Slot{*this, mode == LINES_LD_VALUES ? (int64_t)gload(lines + s) * line_stride : 0, s};
    }
};

// output of a row FFT.  PLAIN: dst[slot][m].  MULB: conj(v bhat[k]) (between the two FFTs of the chirp-z route).  COEFFS:
// hat[slot][k] = Re(e^(-i pi k / 2n) V_k).  VALUES: val[slot][point] = Re(v) / n, the reordering undone.  On the chirp-z route
// the last two first undo the chirp: V = chirp[k] conj(v) / m.
struct LinesStore {
    static constexpr bool kPair = false;
    int mode, n, m, blue;
    double inv_m, inv_n;
    cplx* dst; const cplx* bhat; const cplx* chirp; const cplx* half;
    double* hat; double* val;
    struct Slot {
        const LinesStore& p; int64_t s;
        __device__ inline void operator()(int k, cplx v) const {
            if (p.mode == LINES_ST_PLAIN) { gstore(p.dst + s * p.m + k, v); return; }
            if (p.mode == LINES_ST_MULB) { gstore(p.dst + s * p.m + k, conj(v * gload(p.bhat + k))); return; }
            if (k >= p.n) return;
            if (p.blue) v = (gload(p.chirp + k) * conj(v)) * p.inv_m;
            if (p.mode == LINES_ST_COEFFS) {
                const cplx h = gload(p.half + k);
                gstore(p.hat + s * p.n + k, v.x * h.x - v.y * h.y);
            } else {
                gstore(p.val + s * p.n + lines_perm(k, p.n), v.x * p.inv_n);
            }
        }
    };
    __device__ inline Slot open(int64_t slot) const { return Slot{*this, slot}; }
};

// entries (i, i), (i + 1, i), (i + 2, i) of ((T + lam I)^2)[lines, lines], T the (1, -2, 1) matrix of n_across points with corner
// entries -1: T^2 has the diagonal 6 (2 at the ends), the first off-diagonal -4 (-3 at the ends) and the second 1
struct LinesBand { double a0, a1, a2; };
__device__ inline LinesBand lines_band(const int32_t* lines, int L, int64_t n_across, int i, double lam) {
    const int64_t w = gload(lines + i);
    const int64_t g1 = i + 1 < L ? gload(lines + i + 1) - w : 0, g2 = i + 2 < L ? gload(lines + i + 2) - w : 0;
    const bool end = w == 0 || w == n_across - 1;
    LinesBand b;
    b.a0 = (end ? 2.0 : 6.0) + lam * (end ? -2.0 : -4.0) + lam * lam;
    b.a1 = g1 == 1 ? ((w == 0 || w + 1 == n_across - 1) ? -3.0 : -4.0) + 2.0 * lam : (g1 == 2 ? 1.0 : 0.0);
    b.a2 = g2 == 2 ? 1.0 : 0.0;
    return b;
}

// one thread a mode: L D L^T of the mode's block.  fac[0][i][k] = 1 / d_i, fac[1][i][k] = L(i+1, i), fac[2][i][k] = L(i+2, i)
__global__ void __launch_bounds__(256) lines_factor_kernel(const int32_t* lines, int L, int64_t n_across, int n, double* fac) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const double sh = sin(kLinesPi * ((double)k / (2.0 * (double)n)));
    const double lam = -4.0 * sh * sh;                   // 2 cos(pi k / n) - 2 without the cancellation
    const int64_t plane = (int64_t)L * n;
    double d1 = 0.0, d2 = 0.0, e1 = 0.0, f1 = 0.0, f2 = 0.0;   // d(i-1), d(i-2), l1(i-1), l2(i-1), l2(i-2)
    for (int i = 0; i < L; ++i) {
        const LinesBand b = lines_band(lines, L, n_across, i, lam);
        const double d = b.a0 - e1 * e1 * d1 - f2 * f2 * d2;
        const double l1 = (b.a1 - f1 * d1 * e1) / d, l2 = b.a2 / d;
        const int64_t o = (int64_t)i * n + k;
        gstore(fac + o, 1.0 / d); gstore(fac + plane + o, l1); gstore(fac + 2 * plane + o, l2);
        d2 = d1; d1 = d; f2 = f1; f1 = l2; e1 = l1;
    }
}

// one thread a mode: hat[.][k] <- the solution of the mode's system, in place
__global__ void __launch_bounds__(256)
lines_solve_kernel(const double* fac, int L, int n, double* hat, const InpaintLinesState* st) {
    if (st->s.done_a) return;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int64_t plane = (int64_t)L * n;
    double y1 = 0.0, y2 = 0.0, e1 = 0.0, f2 = 0.0, f1 = 0.0;
    for (int i = 0; i < L; ++i) {
        const int64_t o = (int64_t)i * n + k;
        const double y = gload(hat + o) - e1 * y1 - f2 * y2;
        gstore(hat + o, y);
        y2 = y1; y1 = y; f2 = f1; f1 = gload(fac + 2 * plane + o); e1 = gload(fac + plane + o);
    }
    double x1 = 0.0, x2 = 0.0;
    for (int i = L - 1; i >= 0; --i) {
        const int64_t o = (int64_t)i * n + k;
        const double x = gload(hat + o) * gload(fac + o) - gload(fac + plane + o) * x1 - gload(fac + 2 * plane + o) * x2;
        gstore(hat + o, x);
        x2 = x1; x1 = x;
    }
}

// z = M^-1 r from the two sets of lines (val_f[line][time], val_t[line][channel]) and the diagonal part; partial sums of r.z
__global__ void __launch_bounds__(256)
lines_combine_kernel(int64_t nf, int64_t nt, const double* table, const int32_t* list, int64_t n, const int32_t* pos_f,
                     const int32_t* pos_t, const double* val_f, const double* val_t, const double* r, double* z, double* part,
                     const InpaintLinesState* st) {
    __shared__ double centre[25];
    __shared__ double red[4];
    if (st->s.done_a) return;
    if (threadIdx.x < 25) centre[threadIdx.x] = gload(table + threadIdx.x * 25 + 12);
    __syncthreads();
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t pix = gload(list + i), row = pix / nt, col = pix - row * nt;
        const int32_t pf = gload(pos_f + row), pt = gload(pos_t + col);
        const double ri = gload(r + i);
        double zi = 0.0;
        if (pf >= 0) zi += gload(val_f + (int64_t)pf * nt + col);
        if (pt >= 0) zi += gload(val_t + (int64_t)pt * nf + row);
        if (pf < 0 && pt < 0) zi = ri / centre[inpaint_class(row, nf) * 5 + inpaint_class(col, nt)];
        gstore(z + i, zi);
        acc += ri * zi;
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// inpaint_ap_kernel with p = z + beta p_old, beta from the partial sums of r.z (rz: this step's, rz_prev: the last one's); rr: the
// partial r.r of the last step, for the stopping rule
__global__ void __launch_bounds__(256)
lines_ap_kernel(int64_t nf, int64_t nt, const double* table, const int32_t* index, const int32_t* list, int64_t n,
                const double* z, const double* p_old, double* p, double* q, const double* rr, const double* rz,
                const double* rz_prev, int nparts, int first, int step, double* pq, InpaintLinesState* st) {
    __shared__ double tab[625];
    __shared__ double red[4];
    if (st->s.done_b) return;
    const double rho = inpaint_total(rr, nparts, red);
    if (!(rho > st->s.thresh2)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { st->s.rho = rho; st->s.done_a = 1; }
        return;
    }
    __syncthreads();
    const double rzn = inpaint_total(rz, nparts, red);
    double beta = 0.0;
    if (!first) {
        __syncthreads();
        beta = rzn / inpaint_total(rz_prev, nparts, red);
    }
    inpaint_load_table(table, tab);
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double pi = first ? gload(z + i) : gload(z + i) + beta * gload(p_old + i);
        const double qi = inpaint_row(tab, index, nf, nt, gload(list + i), [&](int64_t, int32_t j) {
            if (j < 0) return 0.0;
            return first ? gload(z + j) : gload(z + j) + beta * gload(p_old + j);
        });
        gstore(p + i, pi); gstore(q + i, qi);
        acc += pi * qi;
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) pq[blockIdx.x] = acc;
    if (blockIdx.x == 0 && threadIdx.x == 0) { st->s.rho = rho; st->rz = rzn; st->s.iters = step; }
}

// inpaint_update_kernel with alpha = r.z / p.q
__global__ void __launch_bounds__(256)
lines_update_kernel(int64_t n, const double* p, const double* q, const double* pq, int nparts, double* x, double* r,
                    double* rr_next, InpaintLinesState* st) {
    __shared__ double red[4];
    if (st->s.done_a) {
        if (blockIdx.x == 0 && threadIdx.x == 0) st->s.done_b = 1;
        return;
    }
    const double alpha = st->rz / inpaint_total(pq, nparts, red);
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

}  // namespace scint
