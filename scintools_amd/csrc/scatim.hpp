// scatim.hpp -- the scattered image, Dynspec.calc_scattered_image (dynspec.py:3553-3570): the tensor-product
// not-a-knot cubic spline of the linear-power secondary spectrum (scipy RectBivariateSpline, kx = ky = 3, s = 0),
// evaluated on the (theta_x, theta_y) grid.  Included from arcnorm.hip (after its spline kernels, which pass B re-uses).
//
//   pass A  scat_rows_kernel   every delay row: spline along the contiguous Doppler axis, evaluated at the nx abscissae
//                              fdop_x -> A[nrow][nx].  10**(dB/10) is formed in the loader; the linear spectrum is never stored.
//   pass B  spline_forward / backward / ends kernels on A (knots: the delay axis, lanes across the nx columns), then
//           scat_image_kernel: every column's own delays (fdop_x[j]^2 + fdop_y[i]^2) eta, times fdop_y, both mirrored halves.
//
// Pass A geometry.  A workgroup of 256 threads owns one CHUNK of interior knots (at most kScatRegion = 2048 columns, warm-up
// included) and walks row groups of kScatRows rows with it.  Thread t owns kScatSeg = 8 consecutive knots; its Thomas factors stay in
// registers for every row.  Per row: coalesced 16-byte loads -> 10**(v/10) -> LDS (rows of 8 doubles padded to 9: conflict-free
// 8-byte accesses at a lane stride of 8 knots); each thread runs the forward recurrence d_i = alpha_i + beta_i d_(i-1) over its
// segment from zero, the 256 affine maps (d_out = A + B d_in) are composed by a wave scan + 4 wave totals, the thread adds the carry;
// the backward recurrence M_i = d_i - sup_i M_(i+1) the same way from the right.  Inside a chunk nothing is approximated; a row longer
// than one chunk is cut into chunks that start `warm` knots early from zero on both sides (the factors contract by >= 2 per knot; the
// host sizes `warm` from the actual factors for a 1e-22 start-up error), so a spectrum element is read once plus that overlap.
// LDS: (2050 + 2048) * 9/8 * 8 B = 36.9 KB per workgroup (4 would fit a CU); the compiler allots 208 VGPRs (the factors, two inlined
// pow), so 2 workgroups = 8 waves per CU are resident: register-bound, nothing spilled to scratch.
#pragma once

namespace scint {

constexpr int kScatSeg = 8;                         // knots per thread
constexpr int kScatRegion = 256 * kScatSeg;         // knots per chunk, warm-up included
constexpr int kScatRows = 4;                        // rows per row group
constexpr int kScatMaxGroups = 512;                 // row groups per launch (grid.y); the rest is strided
constexpr int kScatMaxWarm = 256;

__host__ __device__ inline int scat_pad(int e) { return e + (e >> 3); }

struct ScatRows {
    const double* sspec; int64_t ld, row0, col0;    // dB spectrum, crop origin
    int64_t nrow, n;                                // cropped rows, cropped columns (= knots of a row)
    const double* ih;      // [n] 1 / h_i
    const double* finv6;   // [n] 6 / pivot_i
    const double* fbeta;   // [n] -sub_i / pivot_i
    const double* bsup;    // [n] Thomas c'_i
    double e0, e1, e2, e3; // not-a-knot ends: M[0] = e0 M[1] + e1 M[2], M[n-1] = e2 M[n-2] + e3 M[n-3]
    int64_t valid, warm;   // interior knots a chunk owns; warm-up knots on either side
    const int32_t* idx;    // [nx] interval of abscissa j
    const double* coef;    // [nx][4] weights of y[k], y[k+1], M[k], M[k+1]
    int64_t nx;
    double* A;             // [nrow][nx]
    int32_t* nonfinite;    // set to 1 when 10**(v/10) is NaN or inf anywhere
};

// Carry into every thread's segment of a first-order recurrence whose segment maps are v_out = A + B v_in.  DIR > 0: the
// recurrence runs towards higher threads, DIR < 0 towards lower ones; the chain starts from 0.  red: 8 doubles of LDS.
template <int DIR>
__device__ inline double scat_carry(double A, double B, double* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double A1 = DIR > 0 ? __shfl_up(A, o, 64) : __shfl_down(A, o, 64);
        const double B1 = DIR > 0 ? __shfl_up(B, o, 64) : __shfl_down(B, o, 64);
        if (DIR > 0 ? lane >= o : lane + o < 64) { A = A + B * A1; B = B * B1; }
    }
    __syncthreads();
    if (lane == (DIR > 0 ? 63 : 0)) { red[2 * w] = A; red[2 * w + 1] = B; }
    __syncthreads();
    double c = 0.0;                                 // carry into this wave
    if (DIR > 0) { for (int k = 0; k < w; ++k) c = red[2 * k] + red[2 * k + 1] * c; }
    else { for (int k = 3; k > w; --k) c = red[2 * k] + red[2 * k + 1] * c; }
    double Ae = DIR > 0 ? __shfl_up(A, 1, 64) : __shfl_down(A, 1, 64);
    double Be = DIR > 0 ? __shfl_up(B, 1, 64) : __shfl_down(B, 1, 64);
    if (lane == (DIR > 0 ? 0 : 63)) { Ae = 0.0; Be = 1.0; }
    return Ae + Be * c;
}

__global__ void __launch_bounds__(256) scat_rows_kernel(ScatRows p) {
    __shared__ double Y[kScatRegion + 2 + (kScatRegion + 2) / 8 + 1];   // y[lo-1 .. hi], padded
    __shared__ double M[kScatRegion + kScatRegion / 8 + 1];            // M[lo .. hi-1], padded
    __shared__ double red[8];
    const int t = threadIdx.x;
    const int64_t n = p.n;
    // this workgroup's chunk: it owns the interior knots [vlo, vhi) and solves [lo, hi)
    const int64_t vlo = 1 + (int64_t)blockIdx.x * p.valid;
    const int64_t vhi = min(vlo + p.valid, n - 1);
    const int64_t lo = max((int64_t)1, vlo - p.warm);
    const int64_t hi = min(n - 1, vhi + 1 + p.warm);
    const int len = (int)(hi - lo);                 // <= kScatRegion (checked by the host side)
    const int cnt = len + 2;                        // elements y[lo-1 .. hi]
    // the factors of this thread's knots
    double ih[kScatSeg + 1], finv6[kScatSeg], fbeta[kScatSeg], bsup[kScatSeg];
#pragma unroll
    for (int j = 0; j <= kScatSeg; ++j) {
        const int e = t * kScatSeg + j;             // knot lo + e; ih[j] = 1 / h[lo + e - 1]
        ih[j] = e <= len ? gload(p.ih + lo + e - 1) : 0.0;
        if (j < kScatSeg) {
            const bool in = e < len;
            finv6[j] = in ? gload(p.finv6 + lo + e) : 0.0;
            fbeta[j] = in ? gload(p.fbeta + lo + e) : 0.0;
            bsup[j] = in ? gload(p.bsup + lo + e) : 0.0;
        }
    }
    const int64_t ngroup = (p.nrow + kScatRows - 1) / kScatRows;
    for (int64_t g = blockIdx.y; g < ngroup; g += gridDim.y) {
        for (int64_t r = g * kScatRows; r < min((g + 1) * kScatRows, p.nrow); ++r) {
            // ---- load y[lo-1 .. hi] of this row: aligned 16-byte pairs, 8-byte loads where a pair crosses the range
            const double* src = p.sspec + (p.row0 + r) * p.ld + p.col0 + (lo - 1);
            const int s = (int)(((uintptr_t)src >> 3) & 1);             // 1: src is the upper half of an aligned pair
            bool bad = false;
            for (int q = t; 2 * q - s < cnt; q += 256) {
                const int ea = 2 * q - s, eb = ea + 1;
                double va = 0.0, vb = 0.0;
                if (ea >= 0 && eb < cnt) {
                    const v2d v = *(const SCINT_GLOBAL v2d*)(src + ea);
                    va = v.x; vb = v.y;
                } else {
                    if (ea >= 0) va = gload(src + ea);
                    if (eb < cnt) vb = gload(src + eb);
                }
                if (ea >= 0) { va = pow(10.0, va / 10.0); bad |= !isfinite(va); Y[scat_pad(ea)] = va; }
                if (eb < cnt) { vb = pow(10.0, vb / 10.0); bad |= !isfinite(vb); Y[scat_pad(eb)] = vb; }
            }
            if (bad) *(SCINT_GLOBAL int32_t*)p.nonfinite = 1;           // every writer stores the same value
            __syncthreads();
            // ---- forward: d_i = (6 r_i - sub_i d_(i-1)) / pivot_i over this thread's knots, from zero
            double d[kScatSeg];
            {
                const int e0 = t * kScatSeg;                            // Y index of y[knot - 1] of the first knot
                double ym = Y[scat_pad(e0 < cnt ? e0 : 0)], yc = Y[scat_pad(e0 + 1 < cnt ? e0 + 1 : 0)];
                double acc = 0.0, prod = 1.0;
#pragma unroll
                for (int j = 0; j < kScatSeg; ++j) {
                    const int e = e0 + j;
                    if (e < len) {
                        const double yp = Y[scat_pad(e + 2)];
                        const double rr = (yp - yc) * ih[j + 1] - (yc - ym) * ih[j];
                        acc = rr * finv6[j] + fbeta[j] * acc;
                        prod = prod * fbeta[j];
                        ym = yc; yc = yp;
                    }
                    d[j] = acc;
                }
                double carry = scat_carry<1>(acc, prod, red);
#pragma unroll
                for (int j = 0; j < kScatSeg; ++j) { carry = carry * fbeta[j]; d[j] = d[j] + carry; }
            }
            // ---- backward: M_i = d_i - sup_i M_(i+1), from zero at the right
            {
                double acc = 0.0, prod = 1.0;
#pragma unroll
                for (int j = kScatSeg - 1; j >= 0; --j) {
                    if (t * kScatSeg + j < len) {
                        acc = d[j] - bsup[j] * acc;
                        prod = prod * (-bsup[j]);
                        d[j] = acc;
                    }
                }
                double carry = scat_carry<-1>(acc, prod, red);
#pragma unroll
                for (int j = kScatSeg - 1; j >= 0; --j) {
                    const int e = t * kScatSeg + j;
                    if (e < len) { carry = carry * (-bsup[j]); M[scat_pad(e)] = d[j] + carry; }
                }
            }
            __syncthreads();
            // ---- evaluate the abscissae whose interval this chunk owns
            for (int64_t j = t; j < p.nx; j += 256) {
                const int64_t k = gload(p.idx + j);
                const int64_t kk = min(max(k, (int64_t)1), n - 2);
                if (kk < vlo || kk >= vhi) continue;
                auto mom = [&](int64_t i) {                             // M[i], the not-a-knot ends included
                    if (i == 0) return p.e0 * M[scat_pad((int)(1 - lo))] + p.e1 * M[scat_pad((int)(2 - lo))];
                    if (i == n - 1) return p.e2 * M[scat_pad((int)(n - 2 - lo))] + p.e3 * M[scat_pad((int)(n - 3 - lo))];
                    return M[scat_pad((int)(i - lo))];
                };
                const double* c = p.coef + 4 * j;
                const double v = gload(c) * Y[scat_pad((int)(k - (lo - 1)))] + gload(c + 1) * Y[scat_pad((int)(k + 1 - (lo - 1)))] +
                                 gload(c + 2) * mom(k) + gload(c + 3) * mom(k + 1);
                gstore(p.A + r * p.nx + j, v);
            }
            __syncthreads();                                            // Y and M are re-used by the next row
        }
    }
}

// Pass B: pixel (i, j) of the upper half.  Column j of A is a spline in delay with moments Mc; its abscissa is
// (fx[j]^2 + fy[i]^2) eta clamped to the knots (FITPACK's bispev clamps), found by bisection: the interval k with
// knot[k] <= x < knot[k+1], the right end point in the last one (numpy.searchsorted(side='right') - 1, clipped).
__global__ void __launch_bounds__(256)
scat_image_kernel(const double* A, const double* Mc, const double* knot, int64_t nrow, const double* fx, const double* fy,
                  double eta, int64_t nx, int64_t ny, double* image) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= nx) return;
    const double fxj = gload(fx + j), fyi = gload(fy + i);
    double x = (fxj * fxj + fyi * fyi) * eta;
    const double x_lo = gload(knot), x_hi = gload(knot + nrow - 1);
    if (x < x_lo) x = x_lo;
    if (x > x_hi) x = x_hi;
    int64_t lo = 0, hi = nrow;                      // first knot > x
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (x >= gload(knot + mid)) lo = mid + 1; else hi = mid;
    }
    const int64_t k = min(max(lo - 1, (int64_t)0), nrow - 2);
    const double xk = gload(knot + k), xk1 = gload(knot + k + 1), h = xk1 - xk;
    const double a = (xk1 - x) / h, b = (x - xk) / h;
    const double c = (a * a * a - a) * (h * h) / 6.0, e = (b * b * b - b) * (h * h) / 6.0;
    double v = a * gload(A + k * nx + j) + b * gload(A + (k + 1) * nx + j) + c * gload(Mc + k * nx + j) +
               e * gload(Mc + (k + 1) * nx + j);
    v = v * fyi;
    gstore(image + (ny - 1 + i) * nx + j, v);       // scat_im[ny-1:nx, :] = image
    if (i > 0) gstore(image + (ny - 1 - i) * nx + j, v);   // scat_im[0:ny-1, :] = image[ny-1:0:-1, :]
}

}  // namespace scint
