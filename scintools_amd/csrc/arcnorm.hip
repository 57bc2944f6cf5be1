// arcnorm.hip -- arc normalisation of the secondary spectrum (gfx950).
//
//   scint_spline_resample  Dynspec.scale_dyn(scale='lambda')   dynspec.py:3948-3957
//   scint_norm_sspec       the row loop of Dynspec.norm_sspec   dynspec.py:2093-2127
//   scint_masked_colavg    np.ma.average(..., axis=0, weights)  dynspec.py:2171-2181
//   scint_row_nanmean      delay response of subtract_artefacts dynspec.py:2060-2061
//   scint_block_std        fit_arc's noise estimate             dynspec.py:1097-1101
//   scint_scattered_image  Dynspec.calc_scattered_image        dynspec.py:3553-3570 (kernels: scatim.hpp)
//   scint_zap, scint_refill_median / _linear, scint_svd_model, scint_nanmean_axis, scint_divide_axis
//                          Dynspec.zap / refill / correct_dyn   dynspec.py:3856-3870, 3273-3410 (kernels: clean.hpp)
//   scint_inpaint_biharmonic  Dynspec.inpaint: the biharmonic fill of refill   dynspec.py:3301-3307 (kernels: inpaint.hpp)
//   scint_inpaint_biharmonic_lines  the same fill by preconditioned CG (precond='lines': wide bands of whole lines; inpaint.hpp)
//
// Everything here is HBM-bound streaming work (a gather along each delay row, column and row
// reductions).  Compiled with -ffp-contract=off: the interpolation must round like NumPy's
// arr_interp (slope*(x - xp[j]) + fp[j], no fused multiply-add).
#include <math.h>

#include <algorithm>

#include "common.hpp"

namespace scint {

// ------------------------------------------------------------------------------
// cubic-spline resample down the frequency axis
// ------------------------------------------------------------------------------
struct SplineSys {
    const double* h;    // [nf-1] knot spacings
    const double* sub;  // [nf] sub-diagonal a_i of the interior rows 1..nf-2
    const double* inv;  // [nf] 1 / pivot
    const double* sup;  // [nf] Thomas c'_i
    double e0, e1, e2, e3;
};

// Thomas sweeps of the moment system, one thread per (time column, frequency block); loads
// coalesce across the wavefront along time.  Both recurrences contract (|sub*inv|, |sup| are
// about 0.27 on a uniform axis), so a block does not wait for its neighbour: it starts `warm`
// rows early from zero and the start-up error has decayed below rounding (the host sizes `warm`
// from the actual factors) by the first row it stores.  blockIdx.y = frequency block.
__global__ void __launch_bounds__(64)
spline_forward_kernel(const double* dyn, int64_t nf, int64_t nt, int reverse, SplineSys s,
                      int64_t block_rows, int64_t warm, double* D) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= nt) return;
    const int64_t first = 1 + (int64_t)blockIdx.y * block_rows;       // rows [first, last) are stored
    const int64_t last = min(first + block_rows, nf - 1);
    const int64_t i0 = max((int64_t)1, first - warm);
    auto row = [&](int64_t i) { return (reverse ? nf - 1 - i : i) * nt + t; };
    double y_prev = gload(dyn + row(i0 - 1)), y_cur = gload(dyn + row(i0));
    double dp = 0.0;
    for (int64_t i = i0; i < last; ++i) {
        const double y_next = gload(dyn + row(i + 1));
        const double r = 6.0 * ((y_next - y_cur) / gload(s.h + i) - (y_cur - y_prev) / gload(s.h + i - 1));
        dp = (r - gload(s.sub + i) * dp) * gload(s.inv + i);
        if (i >= first) gstore(D + i * nt + t, dp);
        y_prev = y_cur; y_cur = y_next;
    }
}

__global__ void __launch_bounds__(64)
spline_backward_kernel(const double* D, int64_t nf, int64_t nt, SplineSys s, int64_t block_rows,
                       int64_t warm, double* M) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= nt) return;
    const int64_t first = 1 + (int64_t)blockIdx.y * block_rows;
    const int64_t last = min(first + block_rows, nf - 1);
    const int64_t i1 = min(nf - 2, last - 1 + warm);
    double m_next = 0.0;   // exact at i1 == nf-2 (sup[nf-2] == 0), decayed away otherwise
    for (int64_t i = i1; i >= first; --i) {
        m_next = gload(D + i * nt + t) - gload(s.sup + i) * m_next;
        if (i < last) gstore(M + i * nt + t, m_next);
    }
}

// not-a-knot ends: M[0] and M[nf-1] follow from their two neighbours
__global__ void __launch_bounds__(256) spline_ends_kernel(int64_t nf, int64_t nt, SplineSys s, double* M) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    gstore(M + t, s.e0 * gload(M + nt + t) + s.e1 * gload(M + 2 * nt + t));
    gstore(M + (nf - 1) * nt + t, s.e2 * gload(M + (nf - 2) * nt + t) + s.e3 * gload(M + (nf - 3) * nt + t));
}

__global__ void __launch_bounds__(256)
spline_eval_kernel(const double* dyn, int64_t nf, int64_t nt, int reverse, const double* M,
                   const int32_t* idx, const double* coef, int64_t nout, double* out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t k = blockIdx.y;
    if (t >= nt) return;
    const int64_t i = idx[k];
    const int64_t r0 = reverse ? nf - 1 - i : i, r1 = reverse ? nf - 2 - i : i + 1;
    const double c0 = coef[4 * k], c1 = coef[4 * k + 1], c2 = coef[4 * k + 2], c3 = coef[4 * k + 3];
    const double v = c0 * gload(dyn + r0 * nt + t) + c1 * gload(dyn + r1 * nt + t) +
                     c2 * gload(M + i * nt + t) + c3 * gload(M + (i + 1) * nt + t);
    gstore(out + (nout - 1 - k) * nt + t, v);  // np.flipud
}

// ------------------------------------------------------------------------------
// norm_sspec rows
// ------------------------------------------------------------------------------
struct NormRow {
    const double* row;     // sspec row
    const double* fdop;
    double scale, offset;
    int64_t c0, c1;        // selected columns [c0, c1]
    int64_t cut_lo, cut_hi;
    bool has_offset;
    __device__ inline double xp(int64_t c) const { return gload(fdop + c) / scale; }
    __device__ inline double fp(int64_t c) const {
        if (c >= cut_lo && c < cut_hi) return NAN;
        const double v = gload(row + c);
        return has_offset ? v - offset : v;
    }
    __device__ inline double interp(double x, double x_lo, double x_hi, double inv_step) const;
};

// np.interp(x, xp, fp) for one x (numpy/_core/src/multiarray/compiled_base.c, arr_interp) over the selected columns [c0, c1] of a
// row: `Row` gives c0, c1, the abscissa xp(c) and the value fp(c) (NormRow from global memory; the batched profile's tile from LDS)
template <class Row>
__device__ inline double interp_row(const Row& row, double x, double x_lo, double x_hi, double inv_step) {
    const int64_t c0 = row.c0, c1 = row.c1;
    auto xp = [&](int64_t c) { return row.xp(c); };
    auto fp = [&](int64_t c) { return row.fp(c); };
    const int64_t n = c1 - c0 + 1;
    if (n == 1) return fp(c0);
    if (x != x) return x;
    if (x > x_hi) return fp(c1);
    if (x < x_lo) return fp(c0);
    // j = largest column with xp(j) <= x: uniform-axis guess, short walk, bisection fallback.
    // xp(j) and xp(j+1) are carried along so that the usual case costs two divisions.
    const double g = floor((x - x_lo) * inv_step);
    int64_t j = c0 + (int64_t)fmin(fmax(g, 0.0), (double)(n - 1));
    double xj = xp(j), xj1 = 0.0;
    bool have1 = false;
    int walk = 0;
    while (xj > x && j > c0 && walk < 6) { xj1 = xj; have1 = true; --j; xj = xp(j); ++walk; }
    if (!(xj > x)) {
        while (j < c1 && walk < 6) {
            if (!have1) { xj1 = xp(j + 1); have1 = true; }
            if (xj1 > x) break;
            ++j; xj = xj1; have1 = false; ++walk;
        }
    }
    if (xj > x || (j < c1 && (have1 ? xj1 : xp(j + 1)) <= x)) {
        int64_t lo = c0, hi = c1 + 1;  // first column with xp > x is in (lo, hi]
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (x >= xp(mid)) lo = mid + 1; else hi = mid;
        }
        j = lo - 1;
        xj = xp(j);
        have1 = false;
    }
    if (j == c1) return fp(j);
    const double fj = fp(j);
    if (xj == x) return fj;
    if (!have1) xj1 = xp(j + 1);
    const double fj1 = fp(j + 1);
    const double slope = (fj1 - fj) / (xj1 - xj);
    double r = slope * (x - xj) + fj;
    if (r != r) {
        r = slope * (x - xj1) + fj1;
        if (r != r && fj == fj1) r = fj;
    }
    return r;
}

__device__ inline double NormRow::interp(double x, double x_lo, double x_hi, double inv_step) const {
    return interp_row(*this, x, x_lo, x_hi, inv_step);
}

struct NormParams {
    const double* sspec; int64_t ld, nc;
    const double* fdop; const double* yaxis;
    int64_t row0, nr;
    double eta, maxnormfac;
    int64_t cut_lo, cut_hi;
    const double* row_offset;
    const double* x; const double* xlin; int64_t nx;
    double* norm; uint8_t* mask; double* pow;
};

// one workgroup per delay row
__global__ void __launch_bounds__(256) norm_sspec_kernel(NormParams p) {
    __shared__ double red[4];
    const int64_t r = blockIdx.x;
    const double scale = sqrt(gload(p.yaxis + p.row0 + r) / p.eta);
    const double lim = p.maxnormfac * scale;
    // sel = |fdop| <= lim on an ascending axis: first column >= -lim .. last column <= lim
    int64_t lo = 0, hi = p.nc;
    while (lo < hi) { const int64_t m = (lo + hi) >> 1; if (gload(p.fdop + m) >= -lim) hi = m; else lo = m + 1; }
    const int64_t c0 = lo;
    lo = 0; hi = p.nc;
    while (lo < hi) { const int64_t m = (lo + hi) >> 1; if (gload(p.fdop + m) <= lim) lo = m + 1; else hi = m; }
    const int64_t c1 = lo - 1;
    NormRow row;
    row.row = p.sspec + (p.row0 + r) * p.ld;
    row.fdop = p.fdop; row.scale = scale;
    row.has_offset = p.row_offset != nullptr;
    row.offset = row.has_offset ? gload(p.row_offset + r) : 0.0;
    row.c0 = c0; row.c1 = c1; row.cut_lo = p.cut_lo; row.cut_hi = p.cut_hi;
    const bool empty = c1 < c0 || !(lim == lim);
    double x_lo = 0.0, x_hi = 0.0, inv_step = 0.0, x_abs = 0.0;
    if (!empty) {
        x_lo = row.xp(c0); x_hi = row.xp(c1);
        inv_step = (c1 > c0 && x_hi > x_lo) ? (double)(c1 - c0) / (x_hi - x_lo) : 0.0;
        x_abs = fmax(fabs(x_lo), fabs(x_hi));
    }
    double acc = 0.0, cnt = 0.0;
    for (int64_t k = threadIdx.x; k < p.nx; k += 256) {
        const double x = gload(p.x + k);
        double v = NAN, vp = NAN;
        bool m = true;
        if (!empty) {
            v = row.interp(x, x_lo, x_hi, inv_step);
            m = (fabs(x) > x_abs) || (v != v);
            vp = p.xlin ? row.interp(gload(p.xlin + k), x_lo, x_hi, inv_step) : v;
        }
        p.norm[r * p.nx + k] = v;
        p.mask[r * p.nx + k] = m ? 1 : 0;
        // the masked division normSspec/10 masks every non-finite entry (dynspec.py:2118-2127)
        if (!m && isfinite(vp)) { acc += pow(10.0, vp / 10.0); cnt += 1.0; }
    }
    acc = block_sum(acc, red);
    cnt = block_sum(cnt, red);
    if (threadIdx.x == 0) p.pow[r] = cnt > 0.0 ? acc / cnt : NAN;
}

// ------------------------------------------------------------------------------
// masked weighted column average
// ------------------------------------------------------------------------------
constexpr int kAvgRows = 32;  // rows per partial

__global__ void __launch_bounds__(256)
colavg_partial_kernel(const double* norm, const uint8_t* mask, int64_t nr, int64_t nx, const double* w,
                      const uint8_t* rowsel, double* part /*[nchunk][3][nx]*/) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nx) return;
    const int64_t r0 = (int64_t)blockIdx.y * kAvgRows, r1 = min(r0 + kAvgRows, nr);
    double num = 0.0, den = 0.0, cnt = 0.0;
    for (int64_t r = r0; r < r1; ++r) {
        if (rowsel && !rowsel[r]) continue;
        if (mask[r * nx + k]) continue;
        const double wr = w[r];
        num += norm[r * nx + k] * wr;
        den += wr;
        cnt += 1.0;
    }
    part[((int64_t)blockIdx.y * 3) * nx + k] = num;
    part[((int64_t)blockIdx.y * 3 + 1) * nx + k] = den;
    part[((int64_t)blockIdx.y * 3 + 2) * nx + k] = cnt;
}

__global__ void __launch_bounds__(256)
colavg_final_kernel(const double* part, int64_t nchunk, int64_t nx, double* avg, uint8_t* empty) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nx) return;
    double num = 0.0, den = 0.0, cnt = 0.0;
    for (int64_t c = 0; c < nchunk; ++c) {
        num += part[(c * 3) * nx + k];
        den += part[(c * 3 + 1) * nx + k];
        cnt += part[(c * 3 + 2) * nx + k];
    }
    // a column with no entry is masked in the reference, with 0.0 left under the mask
    avg[k] = cnt > 0.0 ? num / den : 0.0;
    empty[k] = cnt > 0.0 ? 0 : 1;
}

// ------------------------------------------------------------------------------
// row nanmean, block std
// ------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
row_nanmean_kernel(const double* sspec, int64_t ld, int64_t nc, int64_t row0, const uint8_t* colsel,
                   int64_t cut_lo, int64_t cut_hi, double* out) {
    __shared__ double red[4];
    const double* row = sspec + (row0 + blockIdx.x) * ld;
    double acc = 0.0, cnt = 0.0;
    for (int64_t c = threadIdx.x; c < nc; c += 256) {
        if (!colsel[c] || (c >= cut_lo && c < cut_hi)) continue;
        const double v = row[c];
        if (v == v) { acc += v; cnt += 1.0; }
    }
    acc = block_sum(acc, red);
    cnt = block_sum(cnt, red);
    if (threadIdx.x == 0) out[blockIdx.x] = acc / cnt;
}

constexpr int kStdBlocks = 1024;

// pass 0: sum(x); pass 1: sum((x - mean)^2), mean = mean_p[problem].  blockIdx.y = the problem of a stack (array `stride`, partials
// `pstride` apart; one problem: grid.y = 1)
__global__ void __launch_bounds__(256)
block_moment_kernel(const double* a, int64_t stride, int64_t ld, int64_t r0, int64_t rows, int64_t c_lo, int64_t c_hi,
                    int64_t nc, const double* mean_p, double* partial, int64_t pstride) {
    __shared__ double red[4];
    const int64_t b = blockIdx.y;
    a += b * stride;
    const int64_t width = c_lo + (nc - c_hi);
    const int64_t total = rows * width;
    const double mean = mean_p ? mean_p[b] : 0.0;
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / width, q = i - r * width;
        const int64_t c = q < c_lo ? q : q - c_lo + c_hi;
        const double v = a[(r0 + r) * ld + c];
        acc += mean_p ? (v - mean) * (v - mean) : v;
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) partial[b * pstride + blockIdx.x] = acc;
}

// blockIdx.x = the problem
__global__ void __launch_bounds__(256)
block_moment_final_kernel(const double* partial, int64_t pstride, int np, double inv_n, int take_sqrt, double* out) {
    __shared__ double red[4];
    const int64_t b = blockIdx.x;
    double acc = 0.0;
    for (int i = threadIdx.x; i < np; i += 256) acc += partial[b * pstride + i];
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) out[b] = take_sqrt ? sqrt(acc * inv_n) : acc * inv_n;
}

}  // namespace scint

#include "scatim.hpp"
#include "clean.hpp"
#include "inpaint.hpp"
#include "arcbatch.hpp"

using namespace scint;

extern "C" int32_t scint_spline_resample(const double* dyn, int64_t nf, int64_t nt, int32_t reverse,
                                         const double* h, const double* sub, const double* inv,
                                         const double* sup, const double* end, int64_t block_rows,
                                         int64_t warm, const int32_t* idx, const double* coef,
                                         int64_t nout, double* out, void* workspace,
                                         size_t workspace_bytes, void* stream_) {
    SCINT_REQUIRE(dyn && h && sub && inv && sup && end && idx && coef && out && workspace,
                  "spline_resample: null pointer");
    SCINT_REQUIRE(nf >= 4 && nt >= 1 && nout >= 1, "spline_resample: need at least 4 channels");
    SCINT_REQUIRE(nout <= 65535, "spline_resample: too many output rows");
    SCINT_REQUIRE(warm >= 0, "spline_resample: bad warm-up length");
    if (workspace_bytes < 2 * sizeof(double) * (size_t)nf * (size_t)nt) {
        set_error("scint: spline_resample workspace too small");
        return SCINT_E_WORKSPACE;
    }
    hipStream_t stream = (hipStream_t)stream_;
    SplineSys s{h, sub, inv, sup, end[0], end[1], end[2], end[3]};
    double* D = (double*)workspace;
    double* M = D + nf * nt;
    const int64_t rows = nf - 2;                       // interior rows 1..nf-2
    if (block_rows <= 0 || block_rows > rows) block_rows = rows;   // one block = the plain sweep
    const int64_t nblk = ceil_div(rows, block_rows);
    SCINT_REQUIRE(nblk <= 65535, "spline_resample: too many frequency blocks");
    const dim3 grid((unsigned)ceil_div(nt, 64), (unsigned)nblk);
    hipLaunchKernelGGL(spline_forward_kernel, grid, dim3(64), 0, stream, dyn, nf, nt, (int)reverse, s,
                       block_rows, warm, D);
    SCINT_LAUNCH_CHECK();
    hipLaunchKernelGGL(spline_backward_kernel, grid, dim3(64), 0, stream, D, nf, nt, s, block_rows, warm, M);
    SCINT_LAUNCH_CHECK();
    hipLaunchKernelGGL(spline_ends_kernel, dim3((unsigned)ceil_div(nt, 256)), dim3(256), 0, stream, nf, nt, s, M);
    SCINT_LAUNCH_CHECK();
    hipLaunchKernelGGL(spline_eval_kernel, dim3((unsigned)ceil_div(nt, 256), (unsigned)nout), dim3(256), 0,
                       stream, dyn, nf, nt, (int)reverse, M, idx, coef, nout, out);
    SCINT_LAUNCH_CHECK();
    return SCINT_OK;
}

extern "C" int32_t scint_norm_sspec(const double* sspec, int64_t ld, int64_t nc, const double* fdop,
                                    const double* yaxis, int64_t row0, int64_t nr, double eta,
                                    double maxnormfac, int64_t cut_lo, int64_t cut_hi,
                                    const double* row_offset, const double* x, const double* xlin,
                                    int64_t nx, double* norm_out, uint8_t* mask_out, double* pow_out,
                                    void* stream_) {
    SCINT_REQUIRE(sspec && fdop && yaxis && x && norm_out && mask_out && pow_out, "norm_sspec: null pointer");
    SCINT_REQUIRE(nc >= 1 && ld >= nc && row0 >= 0 && nr >= 0 && nx >= 1, "norm_sspec: bad sizes");
    if (nr == 0) return SCINT_OK;
    NormParams p;
    p.sspec = sspec; p.ld = ld; p.nc = nc; p.fdop = fdop; p.yaxis = yaxis;
    p.row0 = row0; p.nr = nr; p.eta = eta; p.maxnormfac = maxnormfac;
    p.cut_lo = cut_lo; p.cut_hi = cut_hi; p.row_offset = row_offset;
    p.x = x; p.xlin = xlin; p.nx = nx;
    p.norm = norm_out; p.mask = mask_out; p.pow = pow_out;
    hipLaunchKernelGGL(norm_sspec_kernel, dim3((unsigned)nr), dim3(256), 0, (hipStream_t)stream_, p);
    SCINT_LAUNCH_CHECK();
    return SCINT_OK;
}

extern "C" int32_t scint_masked_colavg_workspace_bytes(int64_t nr, int64_t nx, size_t* bytes) {
    SCINT_REQUIRE(bytes && nr >= 0 && nx >= 1, "masked_colavg_workspace_bytes: bad arguments");
    *bytes = sizeof(double) * 3 * (size_t)std::max<int64_t>(1, ceil_div(nr, kAvgRows)) * (size_t)nx;
    return SCINT_OK;
}

extern "C" int32_t scint_masked_colavg(const double* norm, const uint8_t* mask, int64_t nr, int64_t nx,
                                       const double* weights, const uint8_t* rowsel, double* avg_out,
                                       uint8_t* empty_out, void* workspace, size_t workspace_bytes,
                                       void* stream_) {
    SCINT_REQUIRE(norm && mask && weights && avg_out && empty_out && workspace, "masked_colavg: null pointer");
    SCINT_REQUIRE(nr >= 1 && nx >= 1, "masked_colavg: bad sizes");
    size_t need = 0;
    scint_masked_colavg_workspace_bytes(nr, nx, &need);
    if (workspace_bytes < need) { set_error("scint: masked_colavg workspace too small"); return SCINT_E_WORKSPACE; }
    const int64_t nchunk = ceil_div(nr, kAvgRows);
    SCINT_REQUIRE(nchunk <= 65535, "masked_colavg: too many rows");
    hipStream_t stream = (hipStream_t)stream_;
    double* part = (double*)workspace;
    hipLaunchKernelGGL(colavg_partial_kernel, dim3((unsigned)ceil_div(nx, 256), (unsigned)nchunk), dim3(256), 0,
                       stream, norm, mask, nr, nx, weights, rowsel, part);
    SCINT_LAUNCH_CHECK();
    hipLaunchKernelGGL(colavg_final_kernel, dim3((unsigned)ceil_div(nx, 256)), dim3(256), 0, stream, part,
                       nchunk, nx, avg_out, empty_out);
    SCINT_LAUNCH_CHECK();
    return SCINT_OK;
}

extern "C" int32_t scint_row_nanmean(const double* sspec, int64_t ld, int64_t nc, int64_t row0, int64_t nr,
                                     const uint8_t* colsel, int64_t cut_lo, int64_t cut_hi, double* out,
                                     void* stream_) {
    SCINT_REQUIRE(sspec && colsel && out, "row_nanmean: null pointer");
    SCINT_REQUIRE(nc >= 1 && ld >= nc && row0 >= 0 && nr >= 0, "row_nanmean: bad sizes");
    if (nr == 0) return SCINT_OK;
    hipLaunchKernelGGL(row_nanmean_kernel, dim3((unsigned)nr), dim3(256), 0, (hipStream_t)stream_, sspec, ld, nc,
                       row0, colsel, cut_lo, cut_hi, out);
    SCINT_LAUNCH_CHECK();
    return SCINT_OK;
}

extern "C" int32_t scint_block_std(const double* a, int64_t ld, int64_t nc, int64_t r0, int64_t r1,
                                   int64_t c_lo, int64_t c_hi, double* out, void* workspace,
                                   size_t workspace_bytes, void* stream_) {
    SCINT_REQUIRE(a && out && workspace, "block_std: null pointer");
    SCINT_REQUIRE(nc >= 1 && ld >= nc && r0 >= 0 && r1 > r0 && c_lo >= 0 && c_hi >= c_lo && c_hi <= nc,
                  "block_std: bad ranges");
    const int64_t total = (r1 - r0) * (c_lo + nc - c_hi);
    SCINT_REQUIRE(total >= 1, "block_std: empty selection");
    if (workspace_bytes < sizeof(double) * (kStdBlocks + 8)) {
        set_error("scint: block_std workspace too small");
        return SCINT_E_WORKSPACE;
    }
    hipStream_t stream = (hipStream_t)stream_;
    double* partial = (double*)workspace;
    double* mean = partial + kStdBlocks;
    const int blocks = (int)std::min<int64_t>(kStdBlocks, std::max<int64_t>(1, ceil_div(total, 1024)));
    for (int pass = 0; pass < 2; ++pass) {
        hipLaunchKernelGGL(block_moment_kernel, dim3(blocks), dim3(256), 0, stream, a, (int64_t)0, ld, r0, r1 - r0, c_lo, c_hi,
                           nc, pass ? mean : (const double*)nullptr, partial, (int64_t)0);
        SCINT_LAUNCH_CHECK();
        hipLaunchKernelGGL(block_moment_final_kernel, dim3(1), dim3(256), 0, stream, (const double*)partial, (int64_t)0, blocks,
                           1.0 / (double)total, pass, pass ? out : mean);
        SCINT_LAUNCH_CHECK();
    }
    return SCINT_OK;
}

// ------------------------------------------------------------------------------
// scattered image
// ------------------------------------------------------------------------------
static size_t scat_plane_bytes(int64_t nrow, int64_t nx) { return align_up(sizeof(double) * (size_t)nrow * (size_t)nx, 256); }

extern "C" int32_t scint_scattered_image_workspace_bytes(int64_t nrow, int64_t sampling, size_t* bytes) {
    SCINT_REQUIRE(bytes && nrow >= 4 && sampling >= 1, "scattered_image_workspace_bytes: bad arguments");
    *bytes = 3 * scat_plane_bytes(nrow, 2 * sampling + 1) + 256;      // A, the forward values, the moments; the flag
    return SCINT_OK;
}

extern "C" int32_t scint_scattered_image(const double* sspec_db, int64_t ld, int64_t row0, int64_t row1, int64_t col0,
                                         int64_t col1, const double* tdel, const double* row_sys, const double* row_end,
                                         int64_t row_warm, const int32_t* row_idx, const double* row_coef,
                                         const double* col_sys, const double* col_end, int64_t col_block_rows,
                                         int64_t col_warm, const double* fdop_x, const double* fdop_y, double eta,
                                         int64_t sampling, double* image, int32_t* nonfinite, void* workspace,
                                         size_t workspace_bytes, void* stream_) {
    SCINT_REQUIRE(sspec_db && tdel && row_sys && row_end && row_idx && row_coef && col_sys && col_end && fdop_x && fdop_y &&
                  image && nonfinite && workspace, "scattered_image: null pointer");
    const int64_t nrow = row1 - row0, n = col1 - col0;
    SCINT_REQUIRE(row0 >= 0 && col0 >= 0 && col1 <= ld && nrow >= 4 && n >= 4, "scattered_image: the crop needs at least 4 x 4 pixels");
    SCINT_REQUIRE(sampling >= 1 && sampling <= 32767, "scattered_image: bad sampling");
    SCINT_REQUIRE(row_warm >= 0 && row_warm <= kScatMaxWarm && col_warm >= 0, "scattered_image: bad warm-up length");
    size_t need = 0;
    scint_scattered_image_workspace_bytes(nrow, sampling, &need);
    if (workspace_bytes < need) { set_error("scint: scattered_image workspace too small"); return SCINT_E_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t nx = 2 * sampling + 1, ny = sampling + 1;
    Carver carve(workspace, workspace_bytes);
    double* A = carve.take<double>((size_t)nrow * nx);
    double* D = carve.take<double>((size_t)nrow * nx);
    double* Mc = carve.take<double>((size_t)nrow * nx);
    SCINT_HIP(hipMemsetAsync(nonfinite, 0, sizeof(int32_t), stream));
    // pass A: rows.  One chunk when the interior knots fit a workgroup, else chunks with a warm-up on both sides.
    ScatRows p;
    p.sspec = sspec_db; p.ld = ld; p.row0 = row0; p.col0 = col0; p.nrow = nrow; p.n = n;
    p.ih = row_sys; p.finv6 = row_sys + n; p.fbeta = row_sys + 2 * n; p.bsup = row_sys + 3 * n;
    p.e0 = row_end[0]; p.e1 = row_end[1]; p.e2 = row_end[2]; p.e3 = row_end[3];
    if (n - 2 <= kScatRegion) { p.valid = n - 2; p.warm = 0; }
    else {
        SCINT_REQUIRE(row_warm >= 1, "scattered_image: a row longer than one chunk needs a warm-up length");
        p.warm = row_warm; p.valid = kScatRegion - 2 * row_warm - 1;
    }
    p.idx = row_idx; p.coef = row_coef; p.nx = nx; p.A = A; p.nonfinite = nonfinite;
    const int64_t nchunk = ceil_div(n - 2, p.valid);
    const int64_t ngroup = std::min<int64_t>(kScatMaxGroups, ceil_div(nrow, kScatRows));
    hipLaunchKernelGGL(scat_rows_kernel, dim3((unsigned)nchunk, (unsigned)ngroup), dim3(256), 0, stream, p);
    SCINT_LAUNCH_CHECK();
    // pass B: columns of A (knots: the delay axis), lanes across the nx columns
    SplineSys s{col_sys, col_sys + nrow, col_sys + 2 * nrow, col_sys + 3 * nrow, col_end[0], col_end[1], col_end[2], col_end[3]};
    const int64_t rows = nrow - 2;
    if (col_block_rows <= 0 || col_block_rows > rows) col_block_rows = rows;
    const int64_t nblk = ceil_div(rows, col_block_rows);
    SCINT_REQUIRE(nblk <= 65535, "scattered_image: too many delay blocks");
    const dim3 grid((unsigned)ceil_div(nx, 64), (unsigned)nblk);
    hipLaunchKernelGGL(spline_forward_kernel, grid, dim3(64), 0, stream, (const double*)A, nrow, nx, 0, s, col_block_rows,
                       col_warm, D);
    SCINT_LAUNCH_CHECK();
    hipLaunchKernelGGL(spline_backward_kernel, grid, dim3(64), 0, stream, (const double*)D, nrow, nx, s, col_block_rows, col_warm, Mc);
    SCINT_LAUNCH_CHECK();
    hipLaunchKernelGGL(spline_ends_kernel, dim3((unsigned)ceil_div(nx, 256)), dim3(256), 0, stream, nrow, nx, s, Mc);
    SCINT_LAUNCH_CHECK();
    hipLaunchKernelGGL(scat_image_kernel, dim3((unsigned)ceil_div(nx, 256), (unsigned)ny), dim3(256), 0, stream, (const double*)A,
                       (const double*)Mc, tdel, nrow, fdop_x, fdop_y, eta, nx, ny, image);
    SCINT_LAUNCH_CHECK();
    return SCINT_OK;
}

// ------------------------------------------------------------------------------
// cleaning: zap, refill, correct_dyn (kernels: clean.hpp)
// ------------------------------------------------------------------------------
extern "C" int32_t scint_zap_workspace_bytes(size_t* bytes) {
    SCINT_REQUIRE(bytes, "zap_workspace_bytes: null pointer");
    *bytes = align_up(sizeof(ZapState), 256);
    return SCINT_OK;
}

extern "C" int32_t scint_zap(double* dyn, int64_t n, double sigma, double* stats, void* workspace, size_t workspace_bytes,
                             void* stream_) {
    SCINT_REQUIRE(dyn && workspace, "zap: null pointer");
    SCINT_REQUIRE(n >= 1, "zap: empty array");
    if (workspace_bytes < sizeof(ZapState)) { set_error("scint: zap workspace too small"); return SCINT_E_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    ZapState* st = (ZapState*)workspace;
    SCINT_HIP(hipMemsetAsync(st, 0, sizeof(ZapState), stream));
    const int blocks = (int)std::min<int64_t>(kZapMaxBlocks, ceil_div(n, 256));
    for (int mode = 0; mode < 2; ++mode)
        for (int shift = 56; shift >= 0; shift -= 8) {
            hipLaunchKernelGGL(zap_hist_kernel, dim3(blocks), dim3(256), 0, stream, (const double*)dyn, n, mode, shift, st);
            SCINT_LAUNCH_CHECK();
            hipLaunchKernelGGL(zap_pick_kernel, dim3(1), dim3(64), 0, stream, mode, shift, st);
            SCINT_LAUNCH_CHECK();
        }
    hipLaunchKernelGGL(zap_apply_kernel, dim3(blocks), dim3(256), 0, stream, dyn, n, sigma, (const ZapState*)st);
    SCINT_LAUNCH_CHECK();
    if (stats) SCINT_HIP(hipMemcpyAsync(stats, st->value, 2 * sizeof(double), hipMemcpyDeviceToDevice, stream));
    return SCINT_OK;
}

extern "C" int32_t scint_refill_median(const double* in, int64_t nf, int64_t nt, int64_t kf, int64_t kt, double fill,
                                       double* out, void* stream_) {
    SCINT_REQUIRE(in && out && in != out, "refill_median: null or aliased pointer");
    SCINT_REQUIRE(nf >= 1 && nt >= 1, "refill_median: bad sizes");
    SCINT_REQUIRE(kf >= 1 && kt >= 1 && (kf & 1) && (kt & 1), "refill_median: each kernel size must be odd");
    SCINT_REQUIRE(kf * kt <= kMedMaxWindow, "refill_median: the window holds more than 225 elements");
    SCINT_REQUIRE(ceil_div(nf, kMedTile) <= 65535, "refill_median: more than 1048560 channels");
    hipLaunchKernelGGL(refill_median_kernel, dim3((unsigned)ceil_div(nt, kMedTile), (unsigned)ceil_div(nf, kMedTile)), dim3(256),
                       0, (hipStream_t)stream_, in, nf, nt, (int)kf, (int)kt, fill, out);
    SCINT_LAUNCH_CHECK();
    return SCINT_OK;
}

extern "C" int32_t scint_refill_linear(double* dyn, int64_t nf, int64_t nt, int32_t axis, const uint8_t* line_valid,
                                       void* stream_) {
    SCINT_REQUIRE(dyn && line_valid, "refill_linear: null pointer");
    SCINT_REQUIRE(nf >= 1 && nt >= 1 && (axis == 0 || axis == 1), "refill_linear: bad arguments");
    hipLaunchKernelGGL(refill_linear_kernel, dim3((unsigned)ceil_div(nt, 256), (unsigned)std::min<int64_t>(nf, 65535)), dim3(256),
                       0, (hipStream_t)stream_, dyn, nf, nt, (int)axis, line_valid);
    SCINT_LAUNCH_CHECK();
    return SCINT_OK;
}

static int64_t clean_row_blocks(int64_t nf) { return std::min<int64_t>(kSvdMaxRowBlocks, ceil_div(nf, 32)); }

extern "C" int32_t scint_svd_model_workspace_bytes(int64_t nf, int64_t nt, size_t* bytes) {
    SCINT_REQUIRE(bytes && nf >= 1 && nt >= 1, "svd_model_workspace_bytes: bad arguments");
    const size_t vec = align_up(sizeof(double) * kSvdMaxP * (size_t)nt, 256);
    *bytes = 2 * vec + (size_t)clean_row_blocks(nf) * vec + align_up(sizeof(double) * kSvdMaxP * (size_t)nf, 256) + 512;
    return SCINT_OK;
}

extern "C" int32_t scint_svd_model(const double* a, int64_t nf, int64_t nt, int32_t p, const double* v0, double tol,
                                   int32_t max_iter, double* model, double* corrected, double* status_out, int32_t* iters_out,
                                   void* workspace, size_t workspace_bytes, void* stream_) {
    SCINT_REQUIRE(a && v0 && workspace && (model || corrected), "svd_model: null pointer");
    SCINT_REQUIRE(nf >= 1 && nt >= 1, "svd_model: bad sizes");
    SCINT_REQUIRE(p >= 1 && p <= kSvdMaxP, "svd_model: 1 to 8 columns");
    SCINT_REQUIRE(tol > 0.0 && max_iter >= 1, "svd_model: bad tolerance or iteration limit");
    size_t need = 0;
    scint_svd_model_workspace_bytes(nf, nt, &need);
    if (workspace_bytes < need) { set_error("scint: svd_model workspace too small"); return SCINT_E_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t nblk = clean_row_blocks(nf), rows_per_block = ceil_div(nf, nblk);
    Carver carve(workspace, workspace_bytes);
    double* V = carve.take<double>((size_t)kSvdMaxP * nt);
    double* Y = carve.take<double>((size_t)kSvdMaxP * nt);
    double* part = carve.take<double>((size_t)nblk * kSvdMaxP * nt);
    double* T = carve.take<double>((size_t)kSvdMaxP * nf);
    SvdStatus* status = carve.take<SvdStatus>(1);
    SCINT_HIP(hipMemcpyAsync(V, v0, sizeof(double) * (size_t)p * nt, hipMemcpyDeviceToDevice, stream));
    const dim3 grid_av((unsigned)ceil_div(nf, 4)), grid_aty((unsigned)ceil_div(nt, 256), (unsigned)nblk);
    SvdStatus h;
    bool done = false;
    int it = 0;
    while (!done && it < max_iter) {
        ++it;
        hipLaunchKernelGGL(svd_av_kernel, grid_av, dim3(256), 0, stream, a, nf, nt, (const double*)V, (int)p, T);
        SCINT_LAUNCH_CHECK();
        hipLaunchKernelGGL(svd_aty_kernel, grid_aty, dim3(256), 0, stream, a, nf, nt, (const double*)T, (int)p, rows_per_block, part);
        SCINT_LAUNCH_CHECK();
        hipLaunchKernelGGL(svd_reduce_kernel, dim3((unsigned)ceil_div(nt, 256), (unsigned)p), dim3(256), 0, stream,
                           (const double*)part, (int)nblk, nt, Y);
        SCINT_LAUNCH_CHECK();
        hipLaunchKernelGGL(svd_step_kernel, dim3(1), dim3(256), 0, stream, nt, (int)p, V, Y, status);
        SCINT_LAUNCH_CHECK();
        if (it % 4 == 0 || it == max_iter) {            // the host looks at the residual every fourth step
            SCINT_HIP(hipMemcpyAsync(&h, status, sizeof(SvdStatus), hipMemcpyDeviceToHost, stream));
            SCINT_HIP(hipStreamSynchronize(stream));
            if (!(h.res == h.res)) { set_error("scint: svd_model: the array is not finite"); return SCINT_E_NONFINITE; }
            done = h.active == 0.0 || h.res <= tol * h.lam_min;
        }
    }
    if (iters_out) *iters_out = it;
    if (status_out) SCINT_HIP(hipMemcpyAsync(status_out, status, sizeof(SvdStatus), hipMemcpyDeviceToDevice, stream));
    if (!done) { set_error("scint: svd_model: the block iteration did not reach its residual"); return SCINT_E_NOCONV; }
    hipLaunchKernelGGL(svd_av_kernel, grid_av, dim3(256), 0, stream, a, nf, nt, (const double*)V, (int)p, T);
    SCINT_LAUNCH_CHECK();
    hipLaunchKernelGGL(svd_model_kernel, dim3((unsigned)ceil_div(nt, 256), (unsigned)std::min<int64_t>(nf, 65535)), dim3(256), 0,
                       stream, a, nf, nt, (const double*)T, (const double*)V, (int)p, model, corrected);
    SCINT_LAUNCH_CHECK();
    return SCINT_OK;
}

extern "C" int32_t scint_nanmean_axis_workspace_bytes(int64_t nf, int64_t nt, size_t* bytes) {
    SCINT_REQUIRE(bytes && nf >= 1 && nt >= 1, "nanmean_axis_workspace_bytes: bad arguments");
    *bytes = sizeof(double) * 2 * (size_t)clean_row_blocks(nf) * (size_t)nt;
    return SCINT_OK;
}

extern "C" int32_t scint_nanmean_axis(const double* a, int64_t nf, int64_t nt, int32_t axis, double* out, void* workspace,
                                      size_t workspace_bytes, void* stream_) {
    SCINT_REQUIRE(a && out, "nanmean_axis: null pointer");
    SCINT_REQUIRE(nf >= 1 && nt >= 1 && (axis == 0 || axis == 1), "nanmean_axis: bad arguments");
    hipStream_t stream = (hipStream_t)stream_;
    if (axis == 1) {                                    // over time: one value per channel
        hipLaunchKernelGGL(clean_row_nanmean_kernel, dim3((unsigned)ceil_div(nf, 4)), dim3(256), 0, stream, a, nf, nt, out);
        SCINT_LAUNCH_CHECK();
        return SCINT_OK;
    }
    size_t need = 0;
    scint_nanmean_axis_workspace_bytes(nf, nt, &need);
    SCINT_REQUIRE(workspace, "nanmean_axis: null workspace");
    if (workspace_bytes < need) { set_error("scint: nanmean_axis workspace too small"); return SCINT_E_WORKSPACE; }
    const int64_t nblk = clean_row_blocks(nf), rows_per_block = ceil_div(nf, nblk);
    double* part = (double*)workspace;
    hipLaunchKernelGGL(clean_col_nanmean_kernel, dim3((unsigned)ceil_div(nt, 256), (unsigned)nblk), dim3(256), 0, stream, a, nf, nt,
                       rows_per_block, part);
    SCINT_LAUNCH_CHECK();
    hipLaunchKernelGGL(clean_col_final_kernel, dim3((unsigned)ceil_div(nt, 256)), dim3(256), 0, stream, (const double*)part,
                       (int)nblk, nt, out);
    SCINT_LAUNCH_CHECK();
    return SCINT_OK;
}

extern "C" int32_t scint_divide_axis(double* a, int64_t nf, int64_t nt, int32_t axis, const double* v, void* stream_) {
    SCINT_REQUIRE(a && v, "divide_axis: null pointer");
    SCINT_REQUIRE(nf >= 1 && nt >= 1 && (axis == 0 || axis == 1), "divide_axis: bad arguments");
    hipLaunchKernelGGL(clean_divide_kernel, dim3((unsigned)ceil_div(nt, 256), (unsigned)std::min<int64_t>(nf, 65535)), dim3(256), 0,
                       (hipStream_t)stream_, a, nf, nt, (int)axis, v);
    SCINT_LAUNCH_CHECK();
    return SCINT_OK;
}

// ------------------------------------------------------------------------------
// biharmonic inpainting (kernels: inpaint.hpp)
// ------------------------------------------------------------------------------
extern "C" int32_t scint_inpaint_biharmonic_workspace_bytes(int64_t nf, int64_t nt, int64_t nmask, size_t* bytes) {
    SCINT_REQUIRE(bytes && nf >= 1 && nt >= 1 && nmask >= 0 && nmask <= nf * nt, "inpaint_biharmonic_workspace_bytes: bad arguments");
    const size_t npix = (size_t)nf * (size_t)nt, n = (size_t)std::max<int64_t>(nmask, 1);
    *bytes = align_up(sizeof(int32_t) * npix, 256) + align_up(sizeof(int32_t) * n, 256) +
             align_up(sizeof(int32_t) * (size_t)ceil_div((int64_t)npix, kInpaintChunk), 256) + 6 * align_up(sizeof(double) * n, 256) +
             align_up(sizeof(double) * 3 * kCgMaxBlocks, 256) + 512;
    return SCINT_OK;
}

extern "C" int32_t scint_inpaint_biharmonic(double* dyn, int64_t nf, int64_t nt, const uint8_t* mask, int64_t nmask,
                                            const double* stencils, double tol, int32_t max_iter, double* residual_out,
                                            int32_t* iters_out, void* workspace, size_t workspace_bytes, void* stream_) {
    SCINT_REQUIRE(dyn && mask && stencils && workspace, "inpaint_biharmonic: null pointer");
    SCINT_REQUIRE(nf >= 5 && nt >= 5, "inpaint_biharmonic: the 25 stencil classes need nf >= 5 and nt >= 5");
    SCINT_REQUIRE(nf * nt < (int64_t(1) << 31), "inpaint_biharmonic: more than 2^31 - 1 pixels");
    SCINT_REQUIRE(nmask >= 0 && nmask < nf * nt, "inpaint_biharmonic: every pixel is masked (or a negative count)");
    SCINT_REQUIRE(tol > 0.0 && tol < 1.0 && max_iter >= 1, "inpaint_biharmonic: bad tolerance or iteration limit");
    if (residual_out) *residual_out = 0.0;
    if (iters_out) *iters_out = 0;
    if (nmask == 0) return SCINT_OK;
    size_t need = 0;
    scint_inpaint_biharmonic_workspace_bytes(nf, nt, nmask, &need);
    if (workspace_bytes < need) { set_error("scint: inpaint_biharmonic workspace too small"); return SCINT_E_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t npix = nf * nt, nchunk = ceil_div(npix, kInpaintChunk), n = nmask;
    const int nb = (int)std::min<int64_t>(kCgMaxBlocks, ceil_div(n, 256));
    Carver carve(workspace, workspace_bytes);
    int32_t* index = carve.take<int32_t>((size_t)npix);
    int32_t* list = carve.take<int32_t>((size_t)n);
    int32_t* counts = carve.take<int32_t>((size_t)nchunk);
    double* x = carve.take<double>((size_t)n);
    double* r = carve.take<double>((size_t)n);
    double* b = carve.take<double>((size_t)n);
    double* q = carve.take<double>((size_t)n);
    double* P[2] = {carve.take<double>((size_t)n), carve.take<double>((size_t)n)};
    double* part = carve.take<double>((size_t)3 * kCgMaxBlocks);
    double* RR[2] = {part, part + kCgMaxBlocks};
    double* pq = part + 2 * kCgMaxBlocks;
    InpaintState* st = carve.take<InpaintState>(1);
    InpaintState h;
#define SCINT_INPAINT_READ()                                                                         \
    do {                                                                                             \
        SCINT_HIP(hipMemcpyAsync(&h, st, sizeof(InpaintState), hipMemcpyDeviceToHost, stream));      \
        SCINT_HIP(hipStreamSynchronize(stream));                                                     \
    } while (0)

    // the unknowns, in pixel order
    hipLaunchKernelGGL(inpaint_count_kernel, dim3((unsigned)nchunk), dim3(256), 0, stream, mask, npix, counts);
    SCINT_LAUNCH_CHECK();
    hipLaunchKernelGGL(inpaint_scan_kernel, dim3(1), dim3(256), 0, stream, counts, nchunk, st);
    SCINT_LAUNCH_CHECK();
    hipLaunchKernelGGL(inpaint_fill_kernel, dim3((unsigned)nchunk), dim3(256), 0, stream, mask, npix, (const int32_t*)counts, n, index,
                       list);
    SCINT_LAUNCH_CHECK();
    SCINT_HIP(hipMemcpyAsync(&h.count, &st->count, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    SCINT_HIP(hipStreamSynchronize(stream));
    SCINT_REQUIRE(h.count == n, "inpaint_biharmonic: nmask is not the number of non-zero elements of the mask");

    hipLaunchKernelGGL(inpaint_rhs_kernel, dim3(nb), dim3(256), 0, stream, (const double*)dyn, nf, nt, stencils, (const int32_t*)index,
                       (const int32_t*)list, n, b, r, x, RR[0]);
    SCINT_LAUNCH_CHECK();
    hipLaunchKernelGGL(inpaint_init_kernel, dim3(1), dim3(256), 0, stream, (const double*)RR[0], nb, tol, st);
    SCINT_LAUNCH_CHECK();
    SCINT_INPAINT_READ();
    if (!(h.bnorm2 - h.bnorm2 == 0.0)) {
        set_error("scint: inpaint_biharmonic: a known pixel next to a masked one is not finite");
        return SCINT_E_NONFINITE;
    }
    bool ok = h.bnorm2 == 0.0;                          // b = 0: the fill is zero
    int it = 0, par = 0, first = 1;
    while (!ok) {
        for (int s = 0; s < kCgCheck && it < max_iter; ++s) {
            ++it;
            hipLaunchKernelGGL(inpaint_ap_kernel, dim3(nb), dim3(256), 0, stream, nf, nt, stencils, (const int32_t*)index,
                               (const int32_t*)list, n, (const double*)r, (const double*)P[par], P[par ^ 1], q, (const double*)RR[par],
                               (const double*)RR[par ^ 1], nb, first, it, pq, st);
            SCINT_LAUNCH_CHECK();
            hipLaunchKernelGGL(inpaint_update_kernel, dim3(nb), dim3(256), 0, stream, n, (const double*)P[par ^ 1], (const double*)q,
                               (const double*)pq, nb, x, r, RR[par ^ 1], st);
            SCINT_LAUNCH_CHECK();
            par ^= 1;
            first = 0;
        }
        hipLaunchKernelGGL(inpaint_probe_kernel, dim3(1), dim3(256), 0, stream, (const double*)RR[par], nb, 0, st);
        SCINT_LAUNCH_CHECK();
        SCINT_INPAINT_READ();
        if (!(h.rho - h.rho == 0.0)) { set_error("scint: inpaint_biharmonic: the residual is not finite"); return SCINT_E_NONFINITE; }
        if (!h.done_a && it < max_iter) continue;
        // within the bound by the recurrence (or out of steps): the true residual b - A x decides
        hipLaunchKernelGGL(inpaint_true_kernel, dim3(nb), dim3(256), 0, stream, nf, nt, stencils, (const int32_t*)index,
                           (const int32_t*)list, n, (const double*)b, (const double*)x, r, RR[0], st);
        SCINT_LAUNCH_CHECK();
        hipLaunchKernelGGL(inpaint_probe_kernel, dim3(1), dim3(256), 0, stream, (const double*)RR[0], nb, 1, st);
        SCINT_LAUNCH_CHECK();
        SCINT_INPAINT_READ();
        ok = h.done_a != 0;
        it = h.iters;                                   // the steps that did work
        par = 0;
        first = 1;                                      // continue from the true residual: p = r
        if (it >= max_iter) break;
    }
#undef SCINT_INPAINT_READ
    if (iters_out) *iters_out = h.iters;
    if (residual_out) *residual_out = h.bnorm2 > 0.0 ? sqrt(h.true_rho / h.bnorm2) : 0.0;
    if (!ok) { set_error("scint: inpaint_biharmonic: conjugate gradients did not reach the residual"); return SCINT_E_NOCONV; }
    hipLaunchKernelGGL(inpaint_scatter_kernel, dim3(nb), dim3(256), 0, stream, (const double*)x, (const int32_t*)list, n, dyn);
    SCINT_LAUNCH_CHECK();
    return SCINT_OK;
}

// ------------------------------------------------------------------------------
// biharmonic inpainting with the line-block preconditioner (kernels: inpaint.hpp, second half)
// ------------------------------------------------------------------------------
// a line of n points transforms directly when n is a power of two from 16, else by the chirp-z identity at the power of two >= 2 n - 1
static bool lines_direct(int64_t n) { return is_pow2(n) && n >= 16; }
static int64_t lines_fft_len(int64_t n) { return lines_direct(n) ? n : std::max<int64_t>(16, next_pow2(2 * n - 1)); }
static bool lines_len_ok(int64_t n) { return n >= 5 && lines_fft_len(n) <= kLinesMaxFft; }

// the buffers of one set of L whole lines of n points (sizing with ax == nullptr, carving otherwise: one description of the layout)
static void lines_axis_layout(Carver& carve, int64_t L, int64_t n, int64_t n_across, LineAxis* ax) {
    const int64_t m = lines_fft_len(n);
    const bool blue = !lines_direct(n);
    int32_t* lines = carve.take<int32_t>((size_t)std::max<int64_t>(L, 1));
    int32_t* pos = carve.take<int32_t>((size_t)n_across);
    cplx *half = nullptr, *chirp = nullptr, *bhat = nullptr, *buf = nullptr;
    double *hat = nullptr, *val = nullptr, *fac = nullptr;
    if (L > 0) {
        half = carve.take<cplx>((size_t)n);
        if (blue) {
            chirp = carve.take<cplx>((size_t)n);
            bhat = carve.take<cplx>((size_t)m);
            buf = carve.take<cplx>((size_t)(L * m));
        }
        hat = carve.take<double>((size_t)(L * n));
        val = carve.take<double>((size_t)(L * n));
        fac = carve.take<double>((size_t)(3 * L * n));
    }
    if (ax) {
        ax->L = (int)L; ax->n = (int)n; ax->m = (int)m; ax->blue = blue; ax->n_across = n_across;
        ax->lines = lines; ax->pos = pos; ax->half = half; ax->chirp = chirp; ax->bhat = bhat; ax->buf = buf;
        ax->hat = hat; ax->val = val; ax->fac = fac;
    }
}

struct LinesLayout {
    int32_t *index, *list, *counts, *whole;
    double *x, *r, *b, *q, *z, *P[2], *part;
    InpaintLinesState* st;
    LineAxis ax[2];      // 0: whole channels (lines along time), 1: whole sub-integrations
    size_t bytes;
};
static LinesLayout lines_layout(void* workspace, int64_t nf, int64_t nt, int64_t nmask, int64_t nchan, int64_t nsub, bool carving) {
    LinesLayout l;
    const size_t npix = (size_t)nf * (size_t)nt, n = (size_t)std::max<int64_t>(nmask, 1);
    Carver carve(workspace, ~size_t(0));
    l.index = carve.take<int32_t>(npix);
    l.list = carve.take<int32_t>(n);
    l.counts = carve.take<int32_t>((size_t)ceil_div((int64_t)npix, kInpaintChunk));
    l.whole = carve.take<int32_t>((size_t)std::max(nf, nt));
    l.x = carve.take<double>(n); l.r = carve.take<double>(n); l.b = carve.take<double>(n); l.q = carve.take<double>(n);
    l.z = carve.take<double>(n); l.P[0] = carve.take<double>(n); l.P[1] = carve.take<double>(n);
    l.part = carve.take<double>((size_t)4 * kCgMaxBlocks);
    l.st = carve.take<InpaintLinesState>(1);
    lines_axis_layout(carve, nchan, nt, nf, carving ? &l.ax[0] : nullptr);
    lines_axis_layout(carve, nsub, nf, nt, carving ? &l.ax[1] : nullptr);
    l.bytes = align_up(carve.off, 256);
    return l;
}

static bool lines_args_ok(int64_t nf, int64_t nt, int64_t nmask, int64_t nchan, int64_t nsub) {
    return nf >= 1 && nt >= 1 && nf * nt < (int64_t(1) << 31) && nmask >= 0 && nmask <= nf * nt && nchan >= 0 && nchan <= nf &&
           nsub >= 0 && nsub <= nt;
}

extern "C" int32_t scint_inpaint_biharmonic_lines_workspace_bytes(int64_t nf, int64_t nt, int64_t nmask, int64_t nchan, int64_t nsub,
                                                                  size_t* bytes) {
    SCINT_REQUIRE(bytes && lines_args_ok(nf, nt, nmask, nchan, nsub), "inpaint_biharmonic_lines_workspace_bytes: bad arguments");
    SCINT_REQUIRE((nchan == 0 || lines_len_ok(nt)) && (nsub == 0 || lines_len_ok(nf)),
                  "inpaint_biharmonic_lines_workspace_bytes: a transformed axis must hold 5 .. 4096 points, or 8192");
    *bytes = lines_layout(nullptr, nf, nt, nmask, nchan, nsub, false).bytes;
    return SCINT_OK;
}

// the row FFTs of one transform of a set of lines: `values` -> coefficients (forward) or coefficients -> values
static int32_t lines_transform(const LineAxis& ax, bool forward, const double* r, const int32_t* index, hipStream_t stream) {
    LinesLoad ld{};
    ld.n = ax.n; ld.m = ax.m; ld.L = ax.L; ld.blue = ax.blue;
    ld.src = ax.buf; ld.r = r; ld.index = index; ld.lines = ax.lines; ld.line_stride = ax.line_stride; ld.elem_stride = ax.elem_stride;
    ld.hat = ax.hat; ld.half = ax.half; ld.chirp = ax.chirp;
    LinesStore st{};
    st.n = ax.n; st.m = ax.m; st.blue = ax.blue; st.inv_m = 1.0 / (double)ax.m; st.inv_n = 1.0 / (double)ax.n;
    st.dst = ax.buf; st.bhat = ax.bhat; st.chirp = ax.chirp; st.half = ax.half; st.hat = ax.hat; st.val = ax.val;
    ld.mode = forward ? LINES_LD_VALUES : LINES_LD_COEFFS;
    const int last = forward ? LINES_ST_COEFFS : LINES_ST_VALUES;
    if (ax.blue) {
        st.mode = LINES_ST_MULB;
        const int32_t rc = launch_fft_rows(ax.m, ax.L, ld, st, stream);
        if (rc != SCINT_OK) return rc;
        ld.mode = LINES_LD_PLAIN;
    }
    st.mode = last;
    return launch_fft_rows(ax.m, ax.L, ld, st, stream);
}

extern "C" int32_t scint_inpaint_biharmonic_lines(double* dyn, int64_t nf, int64_t nt, const uint8_t* mask, int64_t nmask,
                                                  int64_t nchan, int64_t nsub, const double* stencils, double tol, int32_t max_iter,
                                                  double* residual_out, int32_t* iters_out, void* workspace, size_t workspace_bytes,
                                                  void* stream_) {
    SCINT_REQUIRE(dyn && mask && stencils && workspace, "inpaint_biharmonic_lines: null pointer");
    SCINT_REQUIRE(nf >= 5 && nt >= 5, "inpaint_biharmonic_lines: the 25 stencil classes need nf >= 5 and nt >= 5");
    SCINT_REQUIRE(lines_args_ok(nf, nt, nmask, nchan, nsub), "inpaint_biharmonic_lines: bad sizes or counts (nf nt < 2^31)");
    SCINT_REQUIRE(nmask < nf * nt, "inpaint_biharmonic_lines: every pixel is masked");
    SCINT_REQUIRE(tol > 0.0 && tol < 1.0 && max_iter >= 1, "inpaint_biharmonic_lines: bad tolerance or iteration limit");
    SCINT_REQUIRE((nchan == 0 || lines_len_ok(nt)) && (nsub == 0 || lines_len_ok(nf)),
                  "inpaint_biharmonic_lines: a transformed axis must hold 5 .. 4096 points, or 8192");
    if (residual_out) *residual_out = 0.0;
    if (iters_out) *iters_out = 0;
    if (nmask == 0) return SCINT_OK;
    LinesLayout w = lines_layout(workspace, nf, nt, nmask, nchan, nsub, true);
    if (workspace_bytes < w.bytes) { set_error("scint: inpaint_biharmonic_lines workspace too small"); return SCINT_E_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t npix = nf * nt, nchunk = ceil_div(npix, kInpaintChunk), n = nmask;
    const int nb = (int)std::min<int64_t>(kCgMaxBlocks, ceil_div(n, 256));
    double *RR = w.part, *RZ[2] = {w.part + kCgMaxBlocks, w.part + 2 * kCgMaxBlocks}, *pq = w.part + 3 * kCgMaxBlocks;
    InpaintLinesState* st = w.st;
    InpaintLinesState h;
    w.ax[0].line_stride = nt; w.ax[0].elem_stride = 1;
    w.ax[1].line_stride = 1; w.ax[1].elem_stride = nt;
#define SCINT_LINES_READ()                                                                            \
    do {                                                                                              \
        SCINT_HIP(hipMemcpyAsync(&h, st, sizeof(InpaintLinesState), hipMemcpyDeviceToHost, stream));  \
        SCINT_HIP(hipStreamSynchronize(stream));                                                      \
    } while (0)

    // the unknowns, in pixel order, and the whole lines
    hipLaunchKernelGGL(inpaint_count_kernel, dim3((unsigned)nchunk), dim3(256), 0, stream, mask, npix, w.counts);
    SCINT_LAUNCH_CHECK();
    hipLaunchKernelGGL(inpaint_scan_kernel, dim3(1), dim3(256), 0, stream, w.counts, nchunk, &st->s);
    SCINT_LAUNCH_CHECK();
    hipLaunchKernelGGL(inpaint_fill_kernel, dim3((unsigned)nchunk), dim3(256), 0, stream, mask, npix, (const int32_t*)w.counts, n, w.index,
                       w.list);
    SCINT_LAUNCH_CHECK();
    hipLaunchKernelGGL(lines_row_count_kernel, dim3((unsigned)nf), dim3(256), 0, stream, mask, nt, w.whole);
    SCINT_LAUNCH_CHECK();
    hipLaunchKernelGGL(lines_list_kernel, dim3(1), dim3(256), 0, stream, (const int32_t*)w.whole, nf, nchan, w.ax[0].pos, w.ax[0].lines,
                       &st->nlines[0]);
    SCINT_LAUNCH_CHECK();
    hipLaunchKernelGGL(lines_col_count_kernel, dim3((unsigned)ceil_div(nt, 256)), dim3(256), 0, stream, mask, nf, nt, w.whole);
    SCINT_LAUNCH_CHECK();
    hipLaunchKernelGGL(lines_list_kernel, dim3(1), dim3(256), 0, stream, (const int32_t*)w.whole, nt, nsub, w.ax[1].pos, w.ax[1].lines,
                       &st->nlines[1]);
    SCINT_LAUNCH_CHECK();
    SCINT_LINES_READ();                                 // (before any kernel walks the lists: they are as long as the caller said)
    SCINT_REQUIRE(h.s.count == n, "inpaint_biharmonic_lines: nmask is not the number of non-zero elements of the mask");
    SCINT_REQUIRE(h.nlines[0] == nchan && h.nlines[1] == nsub,
                  "inpaint_biharmonic_lines: nchan / nsub are not the numbers of wholly masked channels / sub-integrations");
    hipLaunchKernelGGL(inpaint_rhs_kernel, dim3(nb), dim3(256), 0, stream, (const double*)dyn, nf, nt, stencils, (const int32_t*)w.index,
                       (const int32_t*)w.list, n, w.b, w.r, w.x, RR);
    SCINT_LAUNCH_CHECK();
    hipLaunchKernelGGL(inpaint_init_kernel, dim3(1), dim3(256), 0, stream, (const double*)RR, nb, tol, &st->s);
    SCINT_LAUNCH_CHECK();
    SCINT_LINES_READ();
    if (!(h.s.bnorm2 - h.s.bnorm2 == 0.0)) {
        set_error("scint: inpaint_biharmonic_lines: a known pixel next to a masked one is not finite");
        return SCINT_E_NONFINITE;
    }
    // tables and factors: once per call
    for (const LineAxis& ax : w.ax) {
        if (ax.L == 0) continue;
        hipLaunchKernelGGL(lines_tables_kernel, dim3((unsigned)ceil_div(ax.m, 256)), dim3(256), 0, stream, ax.n, ax.m, ax.blue, ax.half,
                           ax.chirp, ax.buf);
        SCINT_LAUNCH_CHECK();
        if (ax.blue) {
            LinesLoad ld{};
            ld.mode = LINES_LD_PLAIN; ld.n = ax.n; ld.m = ax.m; ld.L = 1; ld.src = ax.buf;
            LinesStore sx{};
            sx.mode = LINES_ST_PLAIN; sx.n = ax.n; sx.m = ax.m; sx.dst = ax.bhat;
            const int32_t rc = launch_fft_rows(ax.m, 1, ld, sx, stream);
            if (rc != SCINT_OK) return rc;
        }
        hipLaunchKernelGGL(lines_factor_kernel, dim3((unsigned)ceil_div(ax.n, 256)), dim3(256), 0, stream, (const int32_t*)ax.lines, ax.L,
                           ax.n_across, ax.n, ax.fac);
        SCINT_LAUNCH_CHECK();
    }
    // out = M^-1 r, partial sums of r.out into `part`
    auto precondition = [&](double* out, double* part) -> int32_t {
        for (const LineAxis& ax : w.ax) {
            if (ax.L == 0) continue;
            int32_t rc = lines_transform(ax, true, w.r, w.index, stream);
            if (rc != SCINT_OK) return rc;
            hipLaunchKernelGGL(lines_solve_kernel, dim3((unsigned)ceil_div(ax.n, 256)), dim3(256), 0, stream, (const double*)ax.fac, ax.L,
                               ax.n, ax.hat, (const InpaintLinesState*)st);
            SCINT_LAUNCH_CHECK();
            rc = lines_transform(ax, false, w.r, w.index, stream);
            if (rc != SCINT_OK) return rc;
        }
        hipLaunchKernelGGL(lines_combine_kernel, dim3(nb), dim3(256), 0, stream, nf, nt, stencils, (const int32_t*)w.list, n,
                           (const int32_t*)w.ax[0].pos, (const int32_t*)w.ax[1].pos, (const double*)w.ax[0].val,
                           (const double*)w.ax[1].val, (const double*)w.r, out, part, (const InpaintLinesState*)st);
        SCINT_LAUNCH_CHECK();
        return SCINT_OK;
    };
    auto true_residual = [&]() -> int32_t {
        hipLaunchKernelGGL(inpaint_true_kernel, dim3(nb), dim3(256), 0, stream, nf, nt, stencils, (const int32_t*)w.index,
                           (const int32_t*)w.list, n, (const double*)w.b, (const double*)w.x, w.r, RR, &st->s);
        SCINT_LAUNCH_CHECK();
        hipLaunchKernelGGL(inpaint_probe_kernel, dim3(1), dim3(256), 0, stream, (const double*)RR, nb, 1, &st->s);
        SCINT_LAUNCH_CHECK();
        SCINT_LINES_READ();
        return SCINT_OK;
    };
    bool ok = h.s.bnorm2 == 0.0;                        // b = 0: the fill is zero
    int it = 0;
    if (!ok) {                                          // x0 = M^-1 b: the whole solve when M = A
        int32_t rc = precondition(w.x, RZ[0]);
        if (rc != SCINT_OK) return rc;
        rc = true_residual();
        if (rc != SCINT_OK) return rc;
        if (!(h.s.true_rho - h.s.true_rho == 0.0)) { set_error("scint: inpaint_biharmonic_lines: the residual is not finite"); return SCINT_E_NONFINITE; }
        ok = h.s.done_a != 0;
    }
    while (!ok && it < max_iter) {
        int32_t rc = precondition(w.z, RZ[0]);          // (re)start from the true residual: p = z
        if (rc != SCINT_OK) return rc;
        int par = 0, first = 1;
        do {
            for (int s = 0; s < kCgCheck && it < max_iter; ++s) {
                ++it;
                hipLaunchKernelGGL(lines_ap_kernel, dim3(nb), dim3(256), 0, stream, nf, nt, stencils, (const int32_t*)w.index,
                                   (const int32_t*)w.list, n, (const double*)w.z, (const double*)w.P[par], w.P[par ^ 1], w.q,
                                   (const double*)RR, (const double*)RZ[par], (const double*)RZ[par ^ 1], nb, first, it, pq, st);
                SCINT_LAUNCH_CHECK();
                hipLaunchKernelGGL(lines_update_kernel, dim3(nb), dim3(256), 0, stream, n, (const double*)w.P[par ^ 1], (const double*)w.q,
                                   (const double*)pq, nb, w.x, w.r, RR, st);
                SCINT_LAUNCH_CHECK();
                rc = precondition(w.z, RZ[par ^ 1]);
                if (rc != SCINT_OK) return rc;
                par ^= 1;
                first = 0;
            }
            hipLaunchKernelGGL(inpaint_probe_kernel, dim3(1), dim3(256), 0, stream, (const double*)RR, nb, 0, &st->s);
            SCINT_LAUNCH_CHECK();
            SCINT_LINES_READ();
            if (!(h.s.rho - h.s.rho == 0.0)) { set_error("scint: inpaint_biharmonic_lines: the residual is not finite"); return SCINT_E_NONFINITE; }
        } while (!h.s.done_a && it < max_iter);
        // within the bound by the recurrence (or out of steps): the true residual b - A x decides
        rc = true_residual();
        if (rc != SCINT_OK) return rc;
        ok = h.s.done_a != 0;
        it = h.s.iters;                                 // the steps that did work
    }
#undef SCINT_LINES_READ
    if (iters_out) *iters_out = h.s.bnorm2 > 0.0 ? h.s.iters : 0;
    if (residual_out) *residual_out = h.s.bnorm2 > 0.0 ? sqrt(h.s.true_rho / h.s.bnorm2) : 0.0;
    if (!ok) { set_error("scint: inpaint_biharmonic_lines: conjugate gradients did not reach the residual"); return SCINT_E_NOCONV; }
    hipLaunchKernelGGL(inpaint_scatter_kernel, dim3(nb), dim3(256), 0, stream, (const double*)w.x, (const int32_t*)w.list, n, dyn);
    SCINT_LAUNCH_CHECK();
    return SCINT_OK;
}

// ------------------------------------------------------------------------------
// arc fits over a stack of spectra (kernels: arcbatch.hpp)
// ------------------------------------------------------------------------------
static int arc_std_blocks(int64_t total) { return (int)std::min<int64_t>(kStdBlocks, std::max<int64_t>(1, ceil_div(total, 1024))); }

extern "C" int32_t scint_arc_profile_batch_workspace_bytes(int64_t B, int64_t R, int64_t nc, int64_t nr, size_t* bytes) {
    SCINT_REQUIRE(bytes && B >= 1 && B <= 65535 && R >= 2 && nc >= 1 && nr >= 1 && nr <= R,
                  "arc_profile_batch_workspace_bytes: bad arguments");
    // the row table; per problem the partials of the widest possible noise selection
    const size_t pstride = (size_t)arc_std_blocks((R - R / 2) * nc);
    *bytes = align_up(sizeof(ArcRowInfo) * (size_t)nr, 256) + align_up(sizeof(double) * (size_t)B * pstride, 256);
    return SCINT_OK;
}

extern "C" int32_t scint_arc_profile_batch(const double* sspec, int64_t B, int64_t R, int64_t ld, int64_t nc, const double* fdop,
                                           const double* yaxis, int64_t row0, int64_t nr, double eta, double maxnormfac,
                                           int64_t cut_lo, int64_t cut_hi, int64_t noise_lo, int64_t noise_hi, const double* x,
                                           int64_t nx, double* avg_out, uint8_t* empty_out, double* noise_out, void* workspace,
                                           size_t workspace_bytes, void* stream_) {
    SCINT_REQUIRE(sspec && fdop && yaxis && x && avg_out && empty_out && noise_out && workspace, "arc_profile_batch: null pointer");
    SCINT_REQUIRE(B >= 1 && B <= 65535, "arc_profile_batch: 1 to 65535 problems");
    SCINT_REQUIRE(R >= 2 && nc >= 1 && ld >= nc && nx >= 1, "arc_profile_batch: bad sizes");
    SCINT_REQUIRE(row0 >= 0 && nr >= 1 && row0 + nr <= R, "arc_profile_batch: the delay rows leave the spectrum");
    SCINT_REQUIRE(noise_lo >= 0 && noise_hi >= noise_lo && noise_hi <= nc && noise_lo + nc - noise_hi >= 1,
                  "arc_profile_batch: bad noise columns");
    size_t need = 0;
    scint_arc_profile_batch_workspace_bytes(B, R, nc, nr, &need);
    if (workspace_bytes < need) { set_error("scint: arc_profile_batch workspace too small"); return SCINT_E_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    Carver carve(workspace, workspace_bytes);
    ArcRowInfo* table = carve.take<ArcRowInfo>((size_t)nr);
    const int64_t pstride = arc_std_blocks((R - R / 2) * nc);
    double* partial = carve.take<double>((size_t)B * pstride);
    hipLaunchKernelGGL(arc_row_table_kernel, dim3((unsigned)ceil_div(nr, 256)), dim3(256), 0, stream, fdop, nc, yaxis, row0, nr, eta,
                       maxnormfac, table);
    SCINT_LAUNCH_CHECK();
    ArcProfileParams p;
    p.sspec = sspec; p.stride = R * ld; p.ld = ld; p.fdop = fdop; p.row0 = row0; p.nr = nr; p.cut_lo = cut_lo; p.cut_hi = cut_hi;
    p.rows = table; p.x = x; p.nx = nx; p.avg = avg_out; p.empty = empty_out;
    hipLaunchKernelGGL(arc_profile_kernel, dim3((unsigned)ceil_div(nx, 256), (unsigned)B), dim3(256), 0, stream, p);
    SCINT_LAUNCH_CHECK();
    // the noise of every problem: the two passes of scint_block_std over rows [R/2, R)
    const int64_t r0 = R / 2, rows = R - r0, total = rows * (noise_lo + nc - noise_hi);
    const int blocks = arc_std_blocks(total);
    for (int pass = 0; pass < 2; ++pass) {
        // (between the passes noise_out[b] holds the mean of problem b)
        hipLaunchKernelGGL(block_moment_kernel, dim3(blocks, (unsigned)B), dim3(256), 0, stream, sspec, R * ld, ld, r0, rows, noise_lo,
                           noise_hi, nc, pass ? (const double*)noise_out : (const double*)nullptr, partial, pstride);
        SCINT_LAUNCH_CHECK();
        hipLaunchKernelGGL(block_moment_final_kernel, dim3((unsigned)B), dim3(256), 0, stream, (const double*)partial, pstride, blocks,
                           1.0 / (double)total, pass, noise_out);
        SCINT_LAUNCH_CHECK();
    }
    return SCINT_OK;
}

extern "C" int32_t scint_arc_peak_fit_workspace_bytes(int64_t P, int64_t nx, int32_t asymm, size_t* bytes) {
    SCINT_REQUIRE(bytes && P >= 1 && P * (asymm ? 2 : 1) <= 0x7fffffff && nx >= 2 && nx % 2 == 0,
                  "arc_peak_fit_workspace_bytes: bad arguments");
    *bytes = align_up(sizeof(double) * (size_t)P * (asymm ? 2 : 1) * (size_t)(nx / 2), 256);
    return SCINT_OK;
}

extern "C" int32_t scint_arc_peak_fit(const double* avg, int64_t P, int64_t nx, const double* noise, double noise_div,
                                      const double* x, double etamin, double etamax, const double* constraint, int32_t nsmooth,
                                      const double* coef, double low_power_diff, double high_power_diff, int32_t noise_error,
                                      int32_t log_parabola, int32_t asymm, double* profile_out, double* val_out, int32_t* dec_out,
                                      void* workspace, size_t workspace_bytes, void* stream_) {
    SCINT_REQUIRE(avg && noise && x && constraint && coef && profile_out && val_out && dec_out && workspace,
                  "arc_peak_fit: null pointer");
    SCINT_REQUIRE(P >= 1 && P <= 0x7fffffff && P * (asymm ? 2 : 1) <= 0x7fffffff, "arc_peak_fit: 1 to 2^31 - 1 profiles (two per problem with asymm)");
    SCINT_REQUIRE(nx >= 2 && nx % 2 == 0, "arc_peak_fit: x must hold as many negative as non-negative entries");
    SCINT_REQUIRE(nsmooth >= 3 && (nsmooth & 1), "arc_peak_fit: nsmooth must be odd and at least 3");
    SCINT_REQUIRE(noise_div > 0.0, "arc_peak_fit: bad noise divisor");
    size_t need = 0;
    scint_arc_peak_fit_workspace_bytes(P, nx, asymm, &need);
    if (workspace_bytes < need) { set_error("scint: arc_peak_fit workspace too small"); return SCINT_E_WORKSPACE; }
    ArcPeakParams p;
    p.avg = avg; p.nx = nx; p.noise = noise; p.noise_div = noise_div; p.x = x; p.etamin = etamin; p.etamax = etamax;
    p.con_lo = constraint[0]; p.con_hi = constraint[1]; p.nsmooth = nsmooth; p.coef = coef; p.low = low_power_diff;
    p.high = high_power_diff; p.noise_error = noise_error; p.log_parabola = log_parabola; p.asymm = asymm ? 1 : 0;
    p.prof = profile_out; p.etak = (double*)workspace; p.val = val_out; p.dec = dec_out; p.npp = P * (asymm ? 2 : 1);
    hipLaunchKernelGGL(arc_peak_fit_kernel, dim3((unsigned)p.npp), dim3(64), 0, (hipStream_t)stream_, p);
    SCINT_LAUNCH_CHECK();
    return SCINT_OK;
}
