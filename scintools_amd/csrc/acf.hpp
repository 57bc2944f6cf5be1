// acf.hpp -- the theoretical 2-D intensity ACF of strong scintillation (scint_sim.py:417-766, ACF.calc_acf; Rickett et al. 2014,
// Appendix A) as a float64 matrix-core contraction.  The entry points are at the end of mosaic.hip (built with -ffp-contract=off).
//
// The reference sums, per frequency lag nu and time-lag sample s, gammes[y][x] exp(i ((X - sx)^2 + (Y - sy)^2) / (2 nu)) over an
// M x M grid.  The phase separates, so per lag and for every s at once
//
//     P[y][s]  = sum_x G[y][x] Ex[x][s]                 G real M x M, Ex complex M x nsn: two real GEMMs sharing the A operand
//     gamma[s] = -i step^2 / (2 pi nu) sum_y Ey[y][s] P[y][s]
//
//   tables    Ex / Ey of every lag in one launch (float64 sincos with full range reduction: the arguments reach 1e4-1e5 rad),
//             as four real planes [M][nsnp] per lag (nsnp = nsn padded to a multiple of 16, the padding written as zero)
//   efield    the coarse plane G = acf_efield [m][m]: an OUTPUT, written once and re-read by every lag >= 2
//   contract  v_mfma_f64_16x16x4_f64: a wave owns 16 rows (y), a workgroup 64; A is 16 (y) x 4 (x) of G, B 4 (x) x 16 (s) of Re Ex
//             and of Im Ex; up to four 16-column groups share one A tile.  The core plane (lag 1, the grid core_fac times finer)
//             is GENERATED in the tile loader and never stored.  The epilogue multiplies by Ey, adds a wave's 16 rows and the
//             workgroup's four waves in a fixed order and writes one partial per (lag, y-block, s).
//   finish    adds the partials of the y-blocks in order and applies -i step^2 / (2 pi nu).
// No atomics: equal inputs give equal bits.
//
// f64 MFMA operand layout (tests/emu/include/hip/hip_runtime.h, tools/probes/mfma_f64_probe.hip): A[i][k] in lane 16 k + i,
// B[k][j] in lane 16 k + j, result register r of lane l = row (l >> 4) + 4 r, column l & 15.  The x index of k-step t of a
// 16-wide chunk is xb + 4 k + t, so that a lane's four A values are contiguous in memory; the sum over x has no preferred order.
#pragma once
#include <math.h>

#include "common.hpp"

namespace scint {

typedef double acf_v4d __attribute__((ext_vector_type(4)));

constexpr int kAcfRows = 64;        // y rows of a workgroup (4 waves x 16)
constexpr int kAcfGroups = 4;       // 16-column groups of s that share an A tile

struct AcfPar {
    const double* snp; const double* snp2;      // coarse grid [m], core grid [m2]
    const double* snx; const double* sny;       // time-lag samples [nsn]
    const double* dnun;                          // frequency lags [ndnun] (dnun[0] = 0 is not used)
    int m, m2, nsn, nsnp, ndnun;
    double sigxn, sigyn, sqrtar, alph2, step, step2;
    double* gammes;                              // [m][m]
    double* tab;                                 // phase tables, acf_tab_off
    cplx* part;                                  // partial sums, acf_part_off
    cplx* gamma;                                 // [nsn][ndnun]
};

__host__ __device__ inline int acf_len(const AcfPar& p, int lag) { return lag == 1 ? p.m2 : p.m; }
__host__ __device__ inline int acf_yblocks(int len) { return (len + kAcfRows - 1) / kAcfRows; }
// tables of lag l: four planes [len][nsnp] -- Re Ex, Im Ex, Re Ey, Im Ey
__host__ __device__ inline int64_t acf_tab_off(const AcfPar& p, int lag) {
    return lag == 1 ? 0 : 4 * (int64_t)p.nsnp * ((int64_t)p.m2 + (int64_t)(lag - 2) * p.m);
}
// partials of lag l: [yblocks][nsnp]
__host__ __device__ inline int64_t acf_part_off(const AcfPar& p, int lag) {
    return lag == 1 ? 0 : (int64_t)p.nsnp * ((int64_t)acf_yblocks(p.m2) + (int64_t)(lag - 2) * acf_yblocks(p.m));
}

// gammes (scint_sim.py:573-574), operation by operation
__host__ __device__ inline double acf_efield(double x, double y, double sqrtar, double alph2) {
#pragma clang fp contract(off)
    const double a = x / sqrtar, b = y * sqrtar;
    return exp(-0.5 * pow(a * a + b * b, alph2));
}

__global__ void __launch_bounds__(256) acf_efield_kernel(AcfPar p) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)p.m * p.m) return;
    const int y = (int)(idx / p.m), x = (int)(idx - (int64_t)y * p.m);
    p.gammes[idx] = acf_efield(p.snp[x], p.snp[y], p.sqrtar, p.alph2);
}

// One thread per (row of every lag's grid, axis, s): exp(i (grid[row] - centre[s])^2 / (2 nu)) with the reference's shifted
// centres snxt = snx - 2 sigxn dnun[idn] (scint_sim.py:639-650; sigxn = sigyn = 0 without a phase gradient).
__global__ void __launch_bounds__(256) acf_tables_kernel(AcfPar p, int64_t total) {
#pragma clang fp contract(off)
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int s = (int)(idx % p.nsnp);
    const int64_t t = idx / p.nsnp;
    const int axis = (int)(t & 1);
    const int64_t r = t >> 1;
    int lag, row;
    if (r < p.m2) { lag = 1; row = (int)r; }
    else { lag = 2 + (int)((r - p.m2) / p.m); row = (int)((r - p.m2) % p.m); }
    const int len = acf_len(p, lag);
    double re = 0.0, im = 0.0;
    if (s < p.nsn) {
        const double nu = p.dnun[lag];
        const double g = lag == 1 ? p.snp2[row] : p.snp[row];
        const double c = axis ? p.sny[s] - (2.0 * p.sigyn) * nu : p.snx[s] - (2.0 * p.sigxn) * nu;
        const double d = g - c;
        sincos((d * d) / (2.0 * nu), &im, &re);
    }
    double* plane = p.tab + acf_tab_off(p, lag) + (int64_t)(2 * axis) * len * p.nsnp;
    plane[(int64_t)row * p.nsnp + s] = re;
    plane[(int64_t)(len + row) * p.nsnp + s] = im;
}

// grid: x = y-block, y = chunk of kAcfGroups column groups, z = lag - lag0.  GEN: lag 1, A generated from snp2.
template <bool GEN>
__global__ void __launch_bounds__(256) acf_contract_kernel(AcfPar p, int lag0) {
    __shared__ cplx red[4][16 * kAcfGroups];
    const int lag = lag0 + (int)blockIdx.z;
    const int M = acf_len(p, lag), nsnp = p.nsnp;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int k = lane >> 4, i = lane & 15;
    const int y0 = (int)blockIdx.x * kAcfRows + 16 * w;
    const int s0 = (int)blockIdx.y * 16 * kAcfGroups;
    const int ng = min(kAcfGroups, (nsnp - s0) / 16);          // uniform over the workgroup
    const double* tab = p.tab + acf_tab_off(p, lag);
    const double* ex_re = tab;
    const double* ex_im = tab + (int64_t)M * nsnp;
    const double* ey_re = tab + 2 * (int64_t)M * nsnp;
    const double* ey_im = tab + 3 * (int64_t)M * nsnp;

    acf_v4d acc[kAcfGroups][2];
#pragma unroll
    for (int g = 0; g < kAcfGroups; ++g) acc[g][0] = acc[g][1] = (acf_v4d){0.0, 0.0, 0.0, 0.0};

    if (y0 < M) {                                             // uniform over the wave
        const int y = y0 + i;
        const bool yok = y < M;
        const double gy = GEN && yok ? p.snp2[y] : 0.0;
        const double* grow = GEN ? nullptr : p.gammes + (int64_t)(yok ? y : 0) * M;
        for (int xb = 0; xb < M; xb += 16) {
            double a[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int x = xb + 4 * k + t;
                a[t] = 0.0;
                if (yok && x < M) a[t] = GEN ? acf_efield(p.snp2[x], gy, p.sqrtar, p.alph2) : grow[x];
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int x = xb + 4 * k + t;
                const bool xok = x < M;
                const int64_t o = (int64_t)(xok ? x : 0) * nsnp + s0 + i;
#pragma unroll
                for (int g = 0; g < kAcfGroups; ++g) {
                    if (g < ng) {
                        const double br = xok ? ex_re[o + 16 * g] : 0.0;
                        const double bi = xok ? ex_im[o + 16 * g] : 0.0;
                        acc[g][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t], br, acc[g][0], 0, 0, 0);
                        acc[g][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t], bi, acc[g][1], 0, 0, 0);
                    }
                }
            }
        }
    }
    // epilogue: sum_y Ey[y][s] P[y][s] over the wave's 16 rows (register r of lane l: row (l >> 4) + 4 r, column l & 15)
#pragma unroll
    for (int g = 0; g < kAcfGroups; ++g) {
        if (g < ng) {
            cplx v = mk(0.0, 0.0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int y = y0 + k + 4 * r;
                if (y < M) {
                    const int64_t o = (int64_t)y * nsnp + s0 + 16 * g + i;
                    v = v + mk(ey_re[o], ey_im[o]) * mk(acc[g][0][r], acc[g][1][r]);
                }
            }
            v.x += __shfl_xor(v.x, 16, 64); v.y += __shfl_xor(v.y, 16, 64);
            v.x += __shfl_xor(v.x, 32, 64); v.y += __shfl_xor(v.y, 32, 64);
            if (lane < 16) red[w][16 * g + lane] = v;
        }
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (c < 16 * ng)
        p.part[acf_part_off(p, lag) + (int64_t)blockIdx.x * nsnp + s0 + c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
}

// gamma[s][lag] = -1j * (step^2 * sum / ((2 pi) nu)) (scint_sim.py:597-598, 605-606), one thread per (lag, s)
__global__ void __launch_bounds__(256) acf_finish_kernel(AcfPar p) {
#pragma clang fp contract(off)
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)(p.ndnun - 1) * p.nsn) return;
    const int lag = 1 + (int)(idx / p.nsn), s = (int)(idx % p.nsn);
    const int nyb = acf_yblocks(acf_len(p, lag));
    const cplx* part = p.part + acf_part_off(p, lag) + s;
    cplx sum = mk(0.0, 0.0);
    for (int b = 0; b < nyb; ++b) sum = sum + part[(int64_t)b * p.nsnp];
    const double st = lag == 1 ? p.step2 : p.step;
    const double den = (2.0 * M_PI) * p.dnun[lag];
    const double re = ((st * st) * sum.x) / den, im = ((st * st) * sum.y) / den;
    p.gamma[(int64_t)s * p.ndnun + lag] = mk(im, -re);
}

}  // namespace scint
