// arcbatch.hpp -- arc-curvature fits over a stack of secondary spectra (included from arcnorm.hip, -ffp-contract=off).
//
//   scint_arc_profile_batch  per problem: scint_norm_sspec + scint_masked_colavg (unit weights) and scint_block_std, fused:
//                            the normalised spectrum norm[nr][nx] is never written
//   scint_arc_peak_fit       what Dynspec.fit_arc does on the host with each profile (dynspec.py:1190-1313): fold, smooth,
//                            peak, the two walks, the parabola and its errors; one wavefront per profile
//
// The profile kernel reads every selected pixel once (B nr nc 8 bytes) and writes B nx 9 bytes.  Its sums run in the order of
// colavg_partial_kernel / colavg_final_kernel, its interpolation is interp_row (arcnorm.hip), so problem b holds the bits of the
// single calls on problem b alone.  No atomics anywhere: equal inputs give equal bits.
#pragma once

namespace scint {

// ------------------------------------------------------------------------------
// what a delay row has in common for every problem of the stack (norm_sspec_kernel computes the same per row and problem)
// ------------------------------------------------------------------------------
struct ArcRowInfo {
    double scale, x_lo, x_hi, inv_step, x_abs;
    int64_t c0, c1;        // selected columns [c0, c1]
    int64_t empty;         // no column selected (or a NaN limit): every entry of the row is masked
};

__global__ void __launch_bounds__(256)
arc_row_table_kernel(const double* fdop, int64_t nc, const double* yaxis, int64_t row0, int64_t nr, double eta, double maxnormfac,
                     ArcRowInfo* table) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= nr) return;
    const double scale = sqrt(gload(yaxis + row0 + r) / eta);
    const double lim = maxnormfac * scale;
    int64_t lo = 0, hi = nc;
    while (lo < hi) { const int64_t m = (lo + hi) >> 1; if (gload(fdop + m) >= -lim) hi = m; else lo = m + 1; }
    const int64_t c0 = lo;
    lo = 0; hi = nc;
    while (lo < hi) { const int64_t m = (lo + hi) >> 1; if (gload(fdop + m) <= lim) lo = m + 1; else hi = m; }
    const int64_t c1 = lo - 1;
    ArcRowInfo t;
    t.scale = scale; t.c0 = c0; t.c1 = c1;
    t.empty = (c1 < c0 || !(lim == lim)) ? 1 : 0;
    t.x_lo = t.x_hi = t.inv_step = t.x_abs = 0.0;
    if (!t.empty) {
        t.x_lo = gload(fdop + c0) / scale; t.x_hi = gload(fdop + c1) / scale;
        t.inv_step = (c1 > c0 && t.x_hi > t.x_lo) ? (double)(c1 - c0) / (t.x_hi - t.x_lo) : 0.0;
        t.x_abs = fmax(fabs(t.x_lo), fabs(t.x_hi));
    }
    table[r] = t;
}

// ------------------------------------------------------------------------------
// the profile: one workgroup = one problem x 256 columns of x, walking the delay rows
// ------------------------------------------------------------------------------
// Selected columns of a row one workgroup stages: abscissae and values, 2 x 16 KiB of LDS.  Five workgroups (20 of 32 wavefronts)
// then share a compute unit's 160 KiB; a longer selection is read from global memory through NormRow.
constexpr int kArcLdsCols = 2048;

struct ArcTile {           // the Row of interp_row on the staged selection
    const double* xs; const double* fs;
    int64_t c0, c1;
    __device__ inline double xp(int64_t c) const { return xs[c - c0]; }
    __device__ inline double fp(int64_t c) const { return fs[c - c0]; }
};

struct ArcProfileParams {
    const double* sspec; int64_t stride, ld;     // problem b starts at sspec + b * stride
    const double* fdop;
    int64_t row0, nr, cut_lo, cut_hi;
    const ArcRowInfo* rows;
    const double* x; int64_t nx;
    double* avg; uint8_t* empty;
};

__global__ void __launch_bounds__(256) arc_profile_kernel(ArcProfileParams p) {
    __shared__ double tile_x[kArcLdsCols];
    __shared__ double tile_f[kArcLdsCols];
    const int64_t b = blockIdx.y, k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = k < p.nx;
    const double x = live ? gload(p.x + k) : 0.0;
    const double* prob = p.sspec + b * p.stride;
    double num = 0.0, den = 0.0, cnt = 0.0;
    for (int64_t r0 = 0; r0 < p.nr; r0 += kAvgRows) {           // one partial of colavg_partial_kernel, then its place in the final sum
        const int64_t r1 = min(r0 + kAvgRows, p.nr);
        double pnum = 0.0, pden = 0.0, pcnt = 0.0;
        for (int64_t r = r0; r < r1; ++r) {
            const ArcRowInfo t = p.rows[r];                      // the same for every lane
            if (t.empty) continue;
            const double* row = prob + (p.row0 + r) * p.ld;
            const int64_t n = t.c1 - t.c0 + 1;
            double v = NAN;
            if (n <= kArcLdsCols) {
                __syncthreads();                                 // the readers of the previous row are done
                for (int64_t i = threadIdx.x; i < n; i += 256) {
                    const int64_t c = t.c0 + i;
                    tile_x[i] = gload(p.fdop + c) / t.scale;
                    tile_f[i] = (c >= p.cut_lo && c < p.cut_hi) ? NAN : gload(row + c);
                }
                __syncthreads();
                ArcTile tile{tile_x, tile_f, t.c0, t.c1};
                if (live) v = interp_row(tile, x, t.x_lo, t.x_hi, t.inv_step);
            } else {
                NormRow g;
                g.row = row; g.fdop = p.fdop; g.scale = t.scale; g.offset = 0.0; g.has_offset = false;
                g.c0 = t.c0; g.c1 = t.c1; g.cut_lo = p.cut_lo; g.cut_hi = p.cut_hi;
                if (live) v = g.interp(x, t.x_lo, t.x_hi, t.inv_step);
            }
            const bool m = (fabs(x) > t.x_abs) || (v != v);
            if (live && !m) { pnum += v; pden += 1.0; pcnt += 1.0; }
        }
        num += pnum; den += pden; cnt += pcnt;
    }
    if (!live) return;
    p.avg[b * p.nx + k] = cnt > 0.0 ? num / den : 0.0;
    p.empty[b * p.nx + k] = cnt > 0.0 ? 0 : 1;
}

// ------------------------------------------------------------------------------
// the peak fit: one wavefront per profile
// ------------------------------------------------------------------------------
enum { kArcOk = 0, kArcShort = 1, kArcNoRange = 2, kArcWindow = 3, kArcForward = 4, kArcNonFinite = 5 };

struct ArcPeakParams {
    const double* avg; int64_t nx;
    const double* noise; double noise_div;
    const double* x;
    double etamin, etamax, con_lo, con_hi;
    int nsmooth; const double* coef;
    double low, high;
    int noise_error, log_parabola, asymm;
    double* prof; double* etak;                  // [PP][nx / 2]: the kept points, flipped (prof padded with NaN)
    double* val; int32_t* dec; int64_t npp;      // val[4][PP]: eta, etaerr, etaerr2, noise; dec[5][PP]: pk, i1, i2, kept, status
};

__device__ inline double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ inline double wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}

// scipy.signal.savgol_filter(s, w, 1) (mode='interp') at one index: the handed coefficients inside, the least-squares line over
// the first / last w points within half a window of an end
struct ArcSmooth {
    const double* s; int64_t n; int w, h;
    const double* coef;
    double tm, lmean, lslope, rmean, rslope;
    __device__ inline void edges() {
        tm = 0.5 * (double)(w - 1);
        const double stt = (double)w * ((double)w * (double)w - 1.0) / 12.0;
        double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
        for (int t = 0; t < w; ++t) {
            const double l = gload(s + t), r = gload(s + n - w + t);
            a0 += l; a1 += ((double)t - tm) * l;
            b0 += r; b1 += ((double)t - tm) * r;
        }
        lmean = a0 / (double)w; lslope = a1 / stt;
        rmean = b0 / (double)w; rslope = b1 / stt;
    }
    __device__ inline double at(int64_t i) const {
        if (i < h) return lmean + lslope * ((double)i - tm);
        if (i >= n - h) return rmean + rslope * ((double)(i - (n - w)) - tm);
        double acc = 0.0;
        for (int k = 0; k < w; ++k) acc += gload(coef + k) * gload(s + i + h - k);
        return acc;
    }
};

// smallest i in [lo, hi] at which stop(i) holds, 64 candidates at a time; hi if none does (the callers make stop(hi) hold)
template <class F>
__device__ inline int64_t arc_first_stop(int64_t lo, int64_t hi, F stop) {
    const int lane = threadIdx.x & 63;
    for (int64_t base = lo; base <= hi; base += 64) {
        const int64_t i = base + lane;
        const unsigned long long m = __ballot(i <= hi && stop(i));
        if (m) return base + __ffsll((long long)m) - 1;
    }
    return hi;
}

__global__ void __launch_bounds__(64) arc_peak_fit_kernel(ArcPeakParams p) {
    const int lane = threadIdx.x;
    const int64_t pp = blockIdx.x;
    const int64_t prob = p.asymm ? pp >> 1 : pp;
    const int side = p.asymm ? (int)(pp & 1) : -1;              // 0: x >= 0 (left), 1: x < 0 flipped (right)
    const int64_t half = p.nx / 2;
    const double* a = p.avg + prob * p.nx;
    double* s = p.prof + pp * half;
    double* e = p.etak + pp * half;
    const double noise = gload(p.noise + prob) / p.noise_div;
    const double qnan = NAN;

    // fold, drop what is not finite, flip, eta = etamin / x^2, keep eta < etamax: in the flipped order
    int64_t n = 0;
    for (int64_t base = half - 1; base >= 0; base -= 64) {
        const int64_t j = base - lane;
        bool keep = false;
        double sv = 0.0, ev = 0.0;
        if (j >= 0) {
            const double vp = gload(a + half + j), vn = gload(a + half - 1 - j);
            sv = side < 0 ? (vp + vn) / 2 : (side == 0 ? vp : vn);
            const double ef = 1 / gload(p.x + half + j);
            ev = p.etamin * (ef * ef);
            keep = isfinite(sv) && ev < p.etamax;
        }
        const unsigned long long m = __ballot(keep);
        if (keep) {
            const int64_t at = n + __popcll(m & ((1ull << lane) - 1ull));
            s[at] = sv; e[at] = ev;
        }
        n += __popcll(m);
    }
    for (int64_t i = n + lane; i < half; i += 64) s[i] = qnan;
    __syncthreads();                                             // the wave's stores before its loads of other lanes' points

    int status = kArcOk;
    int64_t pk = -1, i1 = -1, i2 = -1;
    double eta = qnan, etaerr = qnan, etaerr2 = qnan;
    ArcSmooth sm;
    sm.s = s; sm.n = n; sm.w = p.nsmooth; sm.h = p.nsmooth / 2; sm.coef = p.coef;
    double maxp = 0.0;
    if (n < max(p.nsmooth, 4)) status = kArcShort;
    if (status == kArcOk) {
        sm.edges();
        // the largest smoothed value inside the constraint, then its first occurrence anywhere (np.argmin(|smooth - max|))
        double mx = -INFINITY;
        bool any = false;
        for (int64_t i = lane; i < n; i += 64) {
            const double ev = gload(e + i);
            if (ev > p.con_lo && ev < p.con_hi) { any = true; mx = fmax(mx, sm.at(i)); }
        }
        if (!__ballot(any)) status = kArcNoRange;
        maxp = wave_max(mx);
    }
    if (status == kArcOk) {
        for (int64_t base = 0; base < n && pk < 0; base += 64) {
            const int64_t i = base + lane;
            const unsigned long long m = __ballot(i < n && sm.at(i) == maxp);
            if (m) pk = base + __ffsll((long long)m) - 1;
        }
        if (pk < 0) status = kArcNonFinite;                      // (a NaN maximum: cannot happen with finite points)
    }
    if (status == kArcOk) {
        const int64_t hi = max((int64_t)1, n - 1 - pk);          // pk + i >= n - 1 ends both walks
        const double thr_lo = maxp + p.low, thr_hi = maxp + p.high;
        i1 = arc_first_stop(1, hi, [&](int64_t i) {
            if (i >= 2 && pk - i < 0) return true;               // the reference reads smooth[pk - i] here, wrapped
            const double pw = i == 1 ? maxp : sm.at(pk - i);
            return !(pw > thr_lo) || pk + i >= n - 1;
        });
        i2 = arc_first_stop(1, hi, [&](int64_t i) {
            const double pw = i == 1 ? maxp : sm.at(pk + i);
            return !(pw > thr_hi) || pk + i >= n - 1;
        });
        if (pk - i1 < 0 || i1 + i2 < 4) status = kArcWindow;
    }
    if (status == kArcOk) {
        const int64_t m = i1 + i2, first = pk - i1;
        const double* xd = e + first;
        const double* yd = s + first;
        // the abscissa of fit_parabola: x 1000 / ptp(x); of fit_log_parabola: log x scaled so, then scaled so again inside
        double f1 = 1.0, ptp1 = 0.0;
        auto raw = [&](int64_t i) { const double v = gload(xd + i); return p.log_parabola ? log(v) : v; };
        double lo = INFINITY, hi = -INFINITY;
        for (int64_t i = lane; i < m; i += 64) { const double v = raw(i); lo = fmin(lo, v); hi = fmax(hi, v); }
        double ptp = wave_max(hi) - wave_min(lo);
        if (p.log_parabola) {
            ptp1 = ptp; f1 = 1000 / ptp1;
            lo = INFINITY; hi = -INFINITY;
            for (int64_t i = lane; i < m; i += 64) { const double v = raw(i) * f1; lo = fmin(lo, v); hi = fmax(hi, v); }
            ptp = wave_max(hi) - wave_min(lo);
        }
        const double f = 1000 / ptp;
        auto xs = [&](int64_t i) { return p.log_parabola ? (raw(i) * f1) * f : raw(i) * f; };
        // least squares in the centred abscissa u = xs - mean through the orthogonal basis 1, p1 = u - r01, p2 = u^2 - r02 - r12 p1
        // (a QR by Gram-Schmidt of the three columns: the condition number is never squared)
        double acc0 = 0.0;
        for (int64_t i = lane; i < m; i += 64) acc0 += xs(i);
        const double mean = wave_sum(acc0) / (double)m;
        double su = 0.0, suu = 0.0;
        for (int64_t i = lane; i < m; i += 64) { const double u = xs(i) - mean; su += u; suu += u * u; }
        const double r01 = wave_sum(su) / (double)m, r02 = wave_sum(suu) / (double)m;
        double s11 = 0.0, s12 = 0.0;
        for (int64_t i = lane; i < m; i += 64) {
            const double u = xs(i) - mean, p1 = u - r01;
            s11 += p1 * p1; s12 += p1 * (u * u - r02);
        }
        const double n1 = wave_sum(s11), r12 = wave_sum(s12) / n1;
        double s22 = 0.0, sy0 = 0.0, sy1 = 0.0, sy2 = 0.0;
        for (int64_t i = lane; i < m; i += 64) {
            const double u = xs(i) - mean, p1 = u - r01, p2 = (u * u - r02) - r12 * p1, y = gload(yd + i);
            s22 += p2 * p2; sy0 += y; sy1 += y * p1; sy2 += y * p2;
        }
        const double n2 = wave_sum(s22);
        const double d0 = wave_sum(sy0) / (double)m, d1 = wave_sum(sy1) / n1, d2 = wave_sum(sy2) / n2;
        auto fit = [&](int64_t i) {
            const double u = xs(i) - mean, p1 = u - r01, p2 = (u * u - r02) - r12 * p1;
            return d0 + d1 * p1 + d2 * p2;
        };
        double sr = 0.0;
        for (int64_t i = lane; i < m; i += 64) { const double d = gload(yd + i) - fit(i); sr += d * d; }
        const double var = wave_sum(sr) / (double)(m - 3);
        // y = pa u^2 + pb u + ..., so in xs: params[0] = pa, params[1] = pb - 2 pa mean; d1 and d2 are independent, hence
        // var(params[0]) = var / n2 and var(params[1]) = var / n1 + (r12 + 2 mean)^2 var / n2
        const double pa = d2, pb = d1 - d2 * r12;
        const double peak_u = -pb / (2 * pa);
        const double peak = mean + peak_u;
        const double par1 = -2 * pa * peak;
        const double g = r12 + 2 * mean;
        const double err0 = sqrt(fabs(var / n2)), err1 = sqrt(fabs(var / n1 + (var / n2) * (g * g)));
        const double h0 = 1 / (2 * pa), h1 = par1 / 2;
        const double peak_error = sqrt((err1 * err1) * (h0 * h0) + (err0 * err0) * (h1 * h1));
        // np.mean(np.gradient(np.diff(yfit))) > 0, the sum telescoped
        const double y0 = fit(0), y1 = fit(1), y2 = fit(2), z0 = fit(m - 1), z1 = fit(m - 2), z2 = fit(m - 3);
        const double da = y1 - y0, db = y2 - y1, dy = z0 - z1, dz = z1 - z2;
        const double grad = (db - da) + (dy - dz) + ((dy + dz) - (db + da)) / 2;
        if (grad > 0.0) status = kArcForward;
        else if (p.log_parabola) {
            const double pk2 = peak * (ptp / 1000), er2 = peak_error * (ptp / 1000);
            const double frac = er2 / pk2;
            eta = exp(pk2 * ptp1 / 1000);
            etaerr2 = frac * eta;
        } else {
            eta = peak * (ptp / 1000);
            etaerr2 = peak_error * (ptp / 1000);
        }
    }
    if (status == kArcOk) {
        etaerr = etaerr2;
        if (p.noise_error) {
            const double thr = maxp - noise;
            const int64_t e1 = arc_first_stop(1, max((int64_t)1, pk - 1), [&](int64_t i) {
                const double pw = i == 1 ? maxp : sm.at(pk - (i - 1));
                return !(pw > thr) || pk - i <= 1;
            });
            const int64_t e2 = arc_first_stop(1, max((int64_t)1, n - 1 - pk), [&](int64_t i) {
                const double pw = i == 1 ? maxp : sm.at(pk + i);
                return !(pw > thr) || pk + i >= n - 1;
            });
            etaerr = fabs(gload(e + pk - e1) - gload(e + pk + e2)) / 2;
        }
        if (!isfinite(eta) || !isfinite(etaerr) || !isfinite(etaerr2)) status = kArcNonFinite;
    }
    if (lane == 0) {
        const bool ok = status == kArcOk;
        p.val[pp] = ok ? eta : qnan;
        p.val[p.npp + pp] = ok ? etaerr / sqrt(2.0) : qnan;
        p.val[2 * p.npp + pp] = ok ? etaerr2 / sqrt(2.0) : qnan;
        p.val[3 * p.npp + pp] = noise;
        p.dec[pp] = (int32_t)pk;
        p.dec[p.npp + pp] = (int32_t)i1;
        p.dec[2 * p.npp + pp] = (int32_t)i2;
        p.dec[3 * p.npp + pp] = (int32_t)n;
        p.dec[4 * p.npp + pp] = status;
    }
}

}  // namespace scint
