// eigen.hip -- dominant ('largest algebraic') eigenpair of a user-supplied dense Hermitian
// matrix (scint_eigh_top: the eigsh call of modeler).  The eta sweep itself runs on the
// tile-packed storage in eigen_packed.hip.
//
// Replaces scipy.sparse.linalg.eigsh(thth_red, 1, v0=v0, which="LA") of
// Eval_calc (ththmod.py:396-401) and modeler (ththmod.py:308).  theta-theta has a
// zero diagonal, so its spectrum is +/- mixed (lambda_min ~ -0.9 lambda_max): an
// un-shifted power iteration would chase |lambda|.  We run the Hermitian Lanczos
// three-term recurrence from the same start vector ARPACK is given (the middle row),
// take the top Ritz value of the tridiagonal T_k, and stop on the Ritz residual
// beta_k |s_k| <= tol |theta| -- the same quantity ARPACK tests, driven to ~1e-12
// so that |w| agrees with eigsh to better than 1e-9.
//
// Kernels per Lanczos step j (all batched over jobs in blockIdx.y):
//   lanczos_matvec_kernel   u = A q_j - beta_j q_{j-1}; partial q_j^H u     (HBM bound:
//                           16 N^2 B per job; one wavefront owns 8 rows, q_j in LDS,
//                           lanes stride the row -> 1 KiB coalesced per wave-load,
//                           wave-shuffle reduction of the 8 dot products)
//   lanczos_update_kernel   alpha_j = sum partials; w = u - alpha_j q_j; partial |w|^2
// and every `chunk` steps
//   lanczos_check_kernel    top eigenpair of T_k by 64-lane multisection on the Sturm
//                           count + backward recurrence for the eigenvector.
// All reductions use fixed trees / fixed partial order: results are bit-reproducible.
#include <math.h>

#include <algorithm>
#include <vector>

#include "prof.hpp"
#include "thth.hpp"

namespace scint {

constexpr int kRowsPerWave = 8;
constexpr int kRowsPerBlock = 32;      // 4 waves x 8 rows
constexpr int kXChunk = 8192;          // q_j elements staged in LDS at a time (128 KiB)
constexpr int kVecBlock = 256;

struct LanczosJob {
    const cplx* A;      // [n, ld]
    int64_t ld;
    int32_t n;
    int32_t max_steps;  // min(max_iter, n)
    cplx* W[2];         // ping-pong work vectors [n]
    cplx* Q;            // q vectors: [qslots][n]
    int32_t qslots;     // 2 (ring) or max_steps (kept for the eigenvector)
    int32_t rank;       // an upper bound of rank(A) if one is known (the Krylov space is exhausted after rank + 1 steps), or 0
    double* alpha;      // [max_steps]
    double* beta;       // [max_steps + 1]; beta[0] = |v0|, beta[j] = |w| after step j-1
    double* apart;      // [ceil(n/32)]   partial q_j^H u per matvec block
    double* npart;      // [ceil(n/256)]  partial |w|^2 per vector block
    double* svec;       // [max_steps]    eigenvector of T_k (when the Ritz vector is wanted)
    double* result;     // [4]: theta, resid, -, -
    int32_t* state;     // [2]: done flag, steps used
    double* eig_out;    // |theta| destination (device), may be null
    int32_t* status_out;
    int32_t* iters_out;
    const cplx* v0;     // start vector, or null = row n/2 of A
    double tol;
};

__device__ inline double sum_partials(const double* p, int n) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += p[i];
    return s;
}

// w0 = v0 (or the middle row of A, Eval_calc ththmod.py:398); partial |w0|^2
__global__ void __launch_bounds__(kVecBlock) lanczos_init_kernel(const LanczosJob* jobs) {
    __shared__ double red[kVecBlock / 64];
    const LanczosJob jb = jobs[blockIdx.y];
    const int n = jb.n;
    const int r = blockIdx.x * kVecBlock + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x == 0) { jb.state[0] = 0; jb.state[1] = 0; }
    if (blockIdx.x * kVecBlock >= n) return;
    double p = 0.0;
    if (r < n) {
        const cplx v = jb.v0 ? jb.v0[r] : jb.A[(int64_t)(n / 2) * jb.ld + r];
        jb.W[0][r] = v;
        p = norm2(v);
    }
    p = block_sum(p, red);
    if (threadIdx.x == 0) jb.npart[blockIdx.x] = p;
}

__global__ void __launch_bounds__(256) lanczos_matvec_kernel(const LanczosJob* jobs, int step) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    cplx* xs = reinterpret_cast<cplx*>(smem_raw);
    __shared__ double red[4];
    const LanczosJob jb = jobs[blockIdx.y];
    const int n = jb.n;
    const int row_base = blockIdx.x * kRowsPerBlock;
    if (n < 2 || row_base >= n || step >= jb.max_steps || jb.state[0]) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const cplx* __restrict__ win = (step & 1) ? jb.W[1] : jb.W[0];
    cplx* __restrict__ wout = (step & 1) ? jb.W[0] : jb.W[1];
    const int nvb = (n + kVecBlock - 1) / kVecBlock;
    const double beta = sqrt(sum_partials(jb.npart, nvb));   // |w| of the previous step
    const double inv = beta > 0.0 ? 1.0 / beta : 0.0;
    const int qs = jb.qslots;
    cplx* __restrict__ qcur = jb.Q + (int64_t)(step % qs) * n;
    const cplx* __restrict__ qprev = jb.Q + (int64_t)((step + qs - 1) % qs) * n;

    const int r0 = row_base + wave * kRowsPerWave;
    const cplx* rowp[kRowsPerWave];
#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r) {
        const int rr = (r0 + r < n) ? (r0 + r) : (n - 1);
        rowp[r] = jb.A + (int64_t)rr * jb.ld;
    }
    cplx acc[kRowsPerWave];
#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r) acc[r] = mk(0.0, 0.0);

    for (int c0 = 0; c0 < n; c0 += kXChunk) {
        const int cn = min(kXChunk, n - c0);
        __syncthreads();
        for (int c = threadIdx.x; c < cn; c += 256) {
            const cplx v = win[c0 + c];
            xs[c] = mk(v.x * inv, v.y * inv);
        }
        __syncthreads();
        int c = lane;
        for (; c + 64 < cn; c += 128) {
            const cplx x0 = xs[c], x1 = xs[c + 64];
            cplx a0[kRowsPerWave], a1[kRowsPerWave];
#pragma unroll
            for (int r = 0; r < kRowsPerWave; ++r) {
                a0[r] = gload_nt(rowp[r] + c0 + c);
                a1[r] = gload_nt(rowp[r] + c0 + c + 64);
            }
#pragma unroll
            for (int r = 0; r < kRowsPerWave; ++r) acc[r] = acc[r] + a0[r] * x0 + a1[r] * x1;
        }
        for (; c < cn; c += 64) {
            const cplx x0 = xs[c];
#pragma unroll
            for (int r = 0; r < kRowsPerWave; ++r) acc[r] = acc[r] + gload_nt(rowp[r] + c0 + c) * x0;
        }
    }
    // the normalised q_j rows owned by this block (needed by the update and by step j+1)
    double ap = 0.0;
#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r) {
        const cplx s = wave_sum(acc[r]);
        const int row = r0 + r;
        if (lane == 0 && row < n) {
            const cplx wv = win[row];
            const cplx q = mk(wv.x * inv, wv.y * inv);
            cplx u = s;
            if (step > 0) {
                const cplx qp = qprev[row];
                u = mk(u.x - beta * qp.x, u.y - beta * qp.y);
            }
            qcur[row] = q;
            wout[row] = u;
            ap += q.x * u.x + q.y * u.y;  // Re(conj(q) u)
        }
    }
    ap = block_sum(ap, red);
    if (threadIdx.x == 0) {
        jb.apart[blockIdx.x] = ap;
        if (blockIdx.x == 0) jb.beta[step] = beta;
    }
}

__global__ void __launch_bounds__(kVecBlock) lanczos_update_kernel(const LanczosJob* jobs, int step) {
    __shared__ double red[kVecBlock / 64];
    const LanczosJob jb = jobs[blockIdx.y];
    const int n = jb.n;
    if (n < 2 || blockIdx.x * kVecBlock >= n || step >= jb.max_steps || jb.state[0]) return;
    const int nmb = (n + kRowsPerBlock - 1) / kRowsPerBlock;
    const double alpha = sum_partials(jb.apart, nmb);
    cplx* __restrict__ w = (step & 1) ? jb.W[0] : jb.W[1];
    const cplx* __restrict__ q = jb.Q + (int64_t)(step % jb.qslots) * n;
    const int r = blockIdx.x * kVecBlock + threadIdx.x;
    double p = 0.0;
    if (r < n) {
        const cplx u = w[r], qv = q[r];
        const cplx v = mk(u.x - alpha * qv.x, u.y - alpha * qv.y);
        w[r] = v;
        p = norm2(v);
    }
    p = block_sum(p, red);
    if (threadIdx.x == 0) {
        jb.npart[blockIdx.x] = p;
        if (blockIdx.x == 0) jb.alpha[step] = alpha;
    }
}

// Number of eigenvalues of T_k (diag a[0..k), off-diagonal b[1..k)) below x.
__device__ inline int sturm_count(const double* a, const double* b, int k, double x, double tiny) {
    int cnt = 0;
    double d = a[0] - x;
    if (fabs(d) < tiny) d = -tiny;
    cnt += d < 0.0;
    for (int i = 1; i < k; ++i) {
        d = (a[i] - x) - b[i] * b[i] / d;
        if (fabs(d) < tiny) d = -tiny;
        cnt += d < 0.0;
    }
    return cnt;
}

// One wavefront per job: top Ritz pair of T_k after `k` completed steps.
__global__ void __launch_bounds__(64) lanczos_check_kernel(const LanczosJob* jobs, int k_done,
                                                           int final_pass) {
    const LanczosJob jb = jobs[blockIdx.x];
    if (jb.state[0]) return;
    const int lane = threadIdx.x;
    const int n = jb.n;
    if (n < 2) {
        if (lane == 0) {
            jb.state[0] = 1;
            if (jb.status_out) jb.status_out[0] = SCINT_E_EMPTY;
            if (jb.eig_out) jb.eig_out[0] = nan("");
            if (jb.iters_out) jb.iters_out[0] = 0;
        }
        return;
    }
    const int k = min(k_done, jb.max_steps);
    const double* a = jb.alpha;
    const double* b = jb.beta;  // b[i], i >= 1, couples i-1 and i
    const int nvb = (n + kVecBlock - 1) / kVecBlock;
    const double beta_k = sqrt(sum_partials(jb.npart, nvb));
    // Gershgorin bracket
    double lo = INFINITY, hi = -INFINITY, scale = 0.0;
    for (int i = lane; i < k; i += 64) {
        const double off = (i > 0 ? fabs(b[i]) : 0.0) + (i + 1 < k ? fabs(b[i + 1]) : 0.0);
        lo = fmin(lo, a[i] - off);
        hi = fmax(hi, a[i] + off);
        scale = fmax(scale, fabs(a[i]) + off);
    }
    for (int o = 32; o > 0; o >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, o, 64));
        hi = fmax(hi, __shfl_xor(hi, o, 64));
        scale = fmax(scale, __shfl_xor(scale, o, 64));
    }
    bool finite = isfinite(lo) && isfinite(hi) && isfinite(beta_k);
    // A job that knows rank(A) <= r (B = A^H A of a map with r rows) has exhausted its Krylov space after r + 1 steps: T_k
    // then holds lambda_1 exactly.  Past that point the recurrence restarts from rounding noise and grows a second copy of
    // lambda_1; until that copy has converged too, the top pair of T_k is a near-degenerate mix whose last component is not
    // small, and the residual rule alone would let the job wander for tens of steps.
    const bool exhausted = jb.rank > 0 && k > jb.rank;
    double theta = nan(""), resid = nan("");
    if (finite) {
        const double tiny = fmax(scale, 1e-300) * 1e-300 + 1e-300;
        hi = hi + 1e-15 * fabs(hi) + 1e-300;  // count(hi) == k guaranteed
        // multisection: shrink [lo, hi] around the largest eigenvalue (count(lo) < k, count(hi) == k)
        for (int round = 0; round < 40; ++round) {
            const double w = hi - lo;
            if (!(w > 0.0)) break;
            const double x = lo + w * ((double)(lane + 1) / 65.0);
            const int full = (x > lo && x < hi) ? (sturm_count(a, b, k, x, tiny) == k) : 0;
            const unsigned long long m = __ballot(full);
            double nlo, nhi;
            if (m == 0ull) { nlo = __shfl(x, 63, 64); nhi = hi; }
            else {
                const int first = __ffsll((long long)m) - 1;
                nhi = __shfl(x, first, 64);
                nlo = first > 0 ? __shfl(x, first - 1, 64) : lo;
            }
            if (nlo == lo && nhi == hi) break;
            lo = nlo > lo ? nlo : lo;
            hi = nhi < hi ? nhi : hi;
            if (hi - lo <= 4e-16 * fmax(fabs(lo), fabs(hi))) break;
        }
        theta = 0.5 * (lo + hi);
        // eigenvector of T_k for theta by the backward recurrence (stable for the top pair)
        if (lane == 0) {
            double* s = jb.svec;
            double sk = 1.0, skp1 = 0.0, nrm = 0.0, last = 1.0;
            // s[k-1] = 1; b[i] s[i-1] = (theta - a[i]) s[i] - b[i+1] s[i+1]
            if (s) s[k - 1] = 1.0;
            nrm = 1.0;
            for (int i = k - 1; i >= 1; --i) {
                const double bi = b[i];
                double sm1 = (bi != 0.0) ? ((theta - a[i]) * sk - (i + 1 < k ? b[i + 1] * skp1 : 0.0)) / bi : 0.0;
                if (!isfinite(sm1)) sm1 = 0.0;
                if (fabs(sm1) > 1e150) {  // rescale to avoid overflow
                    const double f = 1e-150;
                    sm1 *= f; sk *= f; last *= f; nrm *= f * f;
                    if (s) for (int t = i; t < k; ++t) s[t] *= f;
                }
                if (s) s[i - 1] = sm1;
                nrm += sm1 * sm1;
                skp1 = sk;
                sk = sm1;
            }
            const double inv = 1.0 / sqrt(nrm);
            if (s) for (int t = 0; t < k; ++t) s[t] *= inv;
            resid = beta_k * fabs(last) * inv;
        }
        resid = __shfl(resid, 0, 64);
    }
    if (lane == 0) {
        const bool conv = finite && (resid <= jb.tol * fmax(fabs(theta), 1e-300) || k >= n || beta_k == 0.0 || exhausted);
        const bool stop = conv || !finite || k >= jb.max_steps || final_pass;
        jb.result[0] = theta;
        jb.result[1] = resid;
        if (stop) {
            jb.state[0] = 1;
            jb.state[1] = k;
            if (jb.eig_out) jb.eig_out[0] = fabs(theta);
            if (jb.iters_out) jb.iters_out[0] = k;
            if (jb.status_out)
                jb.status_out[0] = !finite || !isfinite(theta) ? SCINT_E_NONFINITE
                                                                : (conv ? SCINT_OK : SCINT_E_NOCONV);
        }
    }
}

// Ritz vector y = sum_j s_j q_j (un-normalised) + partial |y|^2
// (out_stride: elements between the vectors of consecutive jobs, scint_eigh_top_batch)
__global__ void __launch_bounds__(kVecBlock) lanczos_ritz_kernel(const LanczosJob* jobs, cplx* out, int64_t out_stride) {
    __shared__ double red[kVecBlock / 64];
    const LanczosJob jb = jobs[blockIdx.y];
    out += (int64_t)blockIdx.y * out_stride;
    const int n = jb.n, k = jb.state[1];
    if (blockIdx.x * kVecBlock >= n) return;
    const int r = blockIdx.x * kVecBlock + threadIdx.x;
    double p = 0.0;
    if (r < n) {
        cplx y = mk(0.0, 0.0);
        for (int j = 0; j < k; ++j) {
            const cplx q = jb.Q[(int64_t)j * n + r];
            const double s = jb.svec[j];
            y = mk(y.x + s * q.x, y.y + s * q.y);
        }
        out[r] = y;
        p = norm2(y);
    }
    p = block_sum(p, red);
    if (threadIdx.x == 0) jb.npart[blockIdx.x] = p;
}

__global__ void __launch_bounds__(kVecBlock) lanczos_scale_kernel(const LanczosJob* jobs, cplx* out, int64_t out_stride,
                                                                  double* w_out) {
    const LanczosJob jb = jobs[blockIdx.y];
    out += (int64_t)blockIdx.y * out_stride;
    const int n = jb.n;
    const int r = blockIdx.x * kVecBlock + threadIdx.x;
    const int nvb = (n + kVecBlock - 1) / kVecBlock;
    const double nrm = sqrt(sum_partials(jb.npart, nvb));
    const double inv = nrm > 0.0 ? 1.0 / nrm : 0.0;
    if (r < n) out[r] = mk(out[r].x * inv, out[r].y * inv);
    if (r == 0 && w_out) w_out[blockIdx.y] = jb.result[0];
}

// ------------------------------------------------------------------------------
// host driver
// ------------------------------------------------------------------------------
struct JobLayout {   // byte offsets inside one job's slab
    size_t W0, W1, Q, alpha, beta, apart, npart, svec, result, state, total;
};

static JobLayout job_layout(int64_t nmax, int max_steps, int qslots, bool with_A, size_t* a_off) {
    JobLayout L;
    size_t off = 0;
    auto take = [&](size_t bytes) { off = align_up(off, 256); size_t o = off; off += bytes; return o; };
    if (a_off) *a_off = with_A ? take(sizeof(cplx) * (size_t)nmax * (size_t)nmax) : 0;
    L.W0 = take(sizeof(cplx) * nmax);
    L.W1 = take(sizeof(cplx) * nmax);
    L.Q = take(sizeof(cplx) * (size_t)nmax * (size_t)qslots);
    L.alpha = take(sizeof(double) * (max_steps + 1));
    L.beta = take(sizeof(double) * (max_steps + 2));
    L.apart = take(sizeof(double) * (size_t)ceil_div(nmax, kRowsPerBlock));
    L.npart = take(sizeof(double) * (size_t)ceil_div(nmax, kVecBlock));
    L.svec = take(sizeof(double) * (max_steps + 1));
    L.result = take(sizeof(double) * 4);
    L.state = take(sizeof(int32_t) * 4);
    L.total = align_up(off, 256);
    return L;
}

// Runs Lanczos on `njobs` jobs already uploaded to jobs_dev.  Synchronises the stream
// every `chunk` steps to read the done flags (4 bytes per job).
// Job s keeps its state words at states_dev[4*s .. 4*s+3].
static int32_t run_lanczos(const LanczosJob* jobs_dev, const int32_t* states_dev, int njobs, int nmax,
                           int max_iter, int32_t* flags_pinned, hipStream_t stream) {
    if (njobs == 0) return SCINT_OK;
    const dim3 vgrid((unsigned)ceil_div(nmax, kVecBlock), (unsigned)njobs);
    const dim3 mgrid((unsigned)ceil_div(nmax, kRowsPerBlock), (unsigned)njobs);
    const size_t lds = sizeof(cplx) * (size_t)std::min<int64_t>(nmax, kXChunk);
    if (lds > 64 * 1024)
        SCINT_HIP(hipFuncSetAttribute((const void*)lanczos_matvec_kernel,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(lanczos_init_kernel, vgrid, dim3(kVecBlock), 0, stream, jobs_dev);
    SCINT_LAUNCH_CHECK();
    const int steps_cap = std::min(max_iter, nmax);
    int step = 0;
    int chunk = 16;  // first look after 16 steps, then every 8
    while (step < steps_cap) {
        const int upto = std::min(steps_cap, step + chunk);
        for (; step < upto; ++step) {
            const int slot = profiler().begin(kProfMatvec, stream);
            hipLaunchKernelGGL(lanczos_matvec_kernel, mgrid, dim3(256), lds, stream, jobs_dev, step);
            profiler().end(kProfMatvec, slot, stream);
            hipLaunchKernelGGL(lanczos_update_kernel, vgrid, dim3(kVecBlock), 0, stream, jobs_dev, step);
        }
        SCINT_LAUNCH_CHECK();
        hipLaunchKernelGGL(lanczos_check_kernel, dim3((unsigned)njobs), dim3(64), 0, stream, jobs_dev,
                           step, step >= steps_cap ? 1 : 0);
        SCINT_LAUNCH_CHECK();
        SCINT_HIP(hipMemcpyAsync(flags_pinned, states_dev, sizeof(int32_t) * 4 * (size_t)njobs,
                                 hipMemcpyDeviceToHost, stream));
        SCINT_HIP(hipStreamSynchronize(stream));
        if (profiler().enabled) profiler().collect();
        bool all = true;
        for (int i = 0; i < njobs; ++i) all = all && flags_pinned[4 * i] != 0;
        if (all) break;
        chunk = 8;
    }
    return SCINT_OK;
}

}  // namespace scint

using namespace scint;

// ------------------------------------------------------------------------------
// scint_eigh_top
// ------------------------------------------------------------------------------
extern "C" int32_t scint_eigh_top_workspace_bytes(int64_t n, int32_t max_iter, size_t* bytes) {
    SCINT_REQUIRE(bytes && n >= 1 && max_iter >= 1, "eigh_top_workspace_bytes: bad arguments");
    const int steps = (int)std::min<int64_t>(max_iter, n);
    JobLayout L = job_layout(n, steps, steps, false, nullptr);
    *bytes = L.total + sizeof(LanczosJob) + 1024;
    return SCINT_OK;
}

extern "C" int32_t scint_eigh_top(const scint_c128* a, int64_t n, const scint_c128* v0, double tol,
                                  int32_t max_iter, double* w_out, scint_c128* vec_out,
                                  int32_t* status_out, int32_t* iters_out, void* workspace,
                                  size_t workspace_bytes, void* stream_) {
    SCINT_REQUIRE(a && w_out && status_out && workspace, "eigh_top: null pointer");
    SCINT_REQUIRE(n >= 1 && max_iter >= 1 && tol > 0, "eigh_top: bad arguments");
    hipStream_t stream = (hipStream_t)stream_;
    size_t need = 0;
    scint_eigh_top_workspace_bytes(n, max_iter, &need);
    if (workspace_bytes < need) { set_error("scint: eigh_top workspace too small"); return SCINT_E_WORKSPACE; }
    const int steps = (int)std::min<int64_t>(max_iter, n);
    JobLayout L = job_layout(n, steps, steps, false, nullptr);
    char* base = (char*)workspace;
    LanczosJob jb;
    jb.A = (const cplx*)a; jb.ld = n; jb.n = (int32_t)n; jb.max_steps = steps;
    jb.W[0] = (cplx*)(base + L.W0); jb.W[1] = (cplx*)(base + L.W1);
    jb.Q = (cplx*)(base + L.Q); jb.qslots = steps; jb.rank = 0;
    jb.alpha = (double*)(base + L.alpha); jb.beta = (double*)(base + L.beta);
    jb.apart = (double*)(base + L.apart); jb.npart = (double*)(base + L.npart);
    jb.svec = (double*)(base + L.svec); jb.result = (double*)(base + L.result);
    jb.state = (int32_t*)(base + L.state);
    jb.eig_out = nullptr; jb.status_out = status_out; jb.iters_out = iters_out;
    jb.v0 = (const cplx*)v0; jb.tol = tol;
    LanczosJob* jd = (LanczosJob*)(base + align_up(L.total, 256));
    SCINT_HIP(hipMemcpyAsync(jd, &jb, sizeof(jb), hipMemcpyHostToDevice, stream));
    int32_t* flags = nullptr;
    SCINT_HIP(hipHostMalloc(&flags, sizeof(int32_t) * 4));
    int32_t rc = run_lanczos(jd, jb.state, 1, (int)n, max_iter, flags, stream);
    (void)hipHostFree(flags);
    if (rc != SCINT_OK) return rc;
    if (vec_out) {
        const dim3 vgrid((unsigned)ceil_div(n, kVecBlock), 1);
        hipLaunchKernelGGL(lanczos_ritz_kernel, vgrid, dim3(kVecBlock), 0, stream, jd, (cplx*)vec_out, (int64_t)0);
        hipLaunchKernelGGL(lanczos_scale_kernel, vgrid, dim3(kVecBlock), 0, stream, jd, (cplx*)vec_out, (int64_t)0, w_out);
        SCINT_LAUNCH_CHECK();
    } else {
        SCINT_HIP(hipMemcpyAsync(w_out, jb.result, sizeof(double), hipMemcpyDeviceToDevice, stream));
    }
    SCINT_HIP(hipStreamSynchronize(stream));
    return SCINT_OK;
}


// ------------------------------------------------------------------------------
// scint_eigh_top_batch: scint_eigh_top of MANY dense Hermitian matrices in one set of launches (the composite theta-theta
// matrices of a group of VLBI chunks, ththmod.py:1365).  The Lanczos kernels above are batched over jobs in blockIdx.y; job j
// is the n[j] x n[j] matrix at a_stack + j * a_stride (row length n[j]), started from its row start_row[j] (its middle row when
// start_row is null).  A job's arithmetic does
// not depend on which jobs share the call.  n[j] < 2: status SCINT_E_EMPTY, the vector left as it was.
// ------------------------------------------------------------------------------
extern "C" int32_t scint_eigh_top_batch_workspace_bytes(int64_t nmax, int32_t max_iter, int64_t njobs, size_t* bytes) {
    SCINT_REQUIRE(bytes && nmax >= 1 && max_iter >= 1 && njobs >= 1, "eigh_top_batch_workspace_bytes: bad arguments");
    const int steps = (int)std::min<int64_t>(max_iter, nmax);
    JobLayout L = job_layout(nmax, steps, steps, false, nullptr);
    *bytes = L.total * (size_t)njobs + align_up(sizeof(LanczosJob) * (size_t)njobs, 256) + align_up(sizeof(int32_t) * 4 * (size_t)njobs, 256) + 1024;
    return SCINT_OK;
}

extern "C" int32_t scint_eigh_top_batch(const scint_c128* a_stack, int64_t a_stride, const int32_t* n, const int32_t* start_row,
                                        int64_t njobs, double tol, int32_t max_iter, double* w_out, scint_c128* vec_out, int64_t vec_stride,
                                        int32_t* status_out, int32_t* iters_out, void* workspace, size_t workspace_bytes,
                                        void* stream_) {
    SCINT_REQUIRE(a_stack && n && w_out && vec_out && status_out && iters_out && workspace, "eigh_top_batch: null pointer");
    SCINT_REQUIRE(njobs >= 1 && njobs <= 65535 && max_iter >= 1 && tol > 0, "eigh_top_batch: bad arguments");
    hipStream_t stream = (hipStream_t)stream_;
    int64_t nmax = 1;
    for (int64_t j = 0; j < njobs; ++j) {
        SCINT_REQUIRE(n[j] >= 0 && (int64_t)n[j] * n[j] <= a_stride && n[j] <= vec_stride, "eigh_top_batch: matrix larger than its slot");
        SCINT_REQUIRE(!start_row || n[j] == 0 || (start_row[j] >= 0 && start_row[j] < n[j]), "eigh_top_batch: start row outside the matrix");
        nmax = std::max<int64_t>(nmax, n[j]);
    }
    size_t need = 0;
    scint_eigh_top_batch_workspace_bytes(nmax, max_iter, njobs, &need);
    if (workspace_bytes < need) { set_error("scint: eigh_top_batch workspace too small"); return SCINT_E_WORKSPACE; }
    const int steps_max = (int)std::min<int64_t>(max_iter, nmax);
    const JobLayout L = job_layout(nmax, steps_max, steps_max, false, nullptr);
    std::vector<LanczosJob> jobs((size_t)njobs);
    LanczosJob* jd = (LanczosJob*)((char*)workspace + L.total * (size_t)njobs);
    // the done flags of all jobs in ONE array (run_lanczos reads 4 words per job back with one copy), not in the jobs' slabs
    int32_t* states = (int32_t*)((char*)jd + align_up(sizeof(LanczosJob) * (size_t)njobs, 256));
    for (int64_t j = 0; j < njobs; ++j) {
        char* base = (char*)workspace + L.total * (size_t)j;
        LanczosJob& jb = jobs[(size_t)j];
        const int steps = (int)std::min<int64_t>(max_iter, std::max<int64_t>(n[j], 1));
        jb.A = (const cplx*)a_stack + j * a_stride; jb.ld = n[j]; jb.n = n[j]; jb.max_steps = steps;
        jb.W[0] = (cplx*)(base + L.W0); jb.W[1] = (cplx*)(base + L.W1);
        jb.Q = (cplx*)(base + L.Q); jb.qslots = steps; jb.rank = 0;
        jb.alpha = (double*)(base + L.alpha); jb.beta = (double*)(base + L.beta);
        jb.apart = (double*)(base + L.apart); jb.npart = (double*)(base + L.npart);
        jb.svec = (double*)(base + L.svec); jb.result = (double*)(base + L.result);
        jb.state = states + 4 * j;
        jb.eig_out = nullptr; jb.status_out = status_out + j; jb.iters_out = iters_out + j;
        jb.v0 = (start_row && n[j] > 0) ? jb.A + (int64_t)start_row[j] * n[j] : nullptr; jb.tol = tol;
    }
    SCINT_HIP(hipMemcpyAsync(jd, jobs.data(), sizeof(LanczosJob) * jobs.size(), hipMemcpyHostToDevice, stream));
    int32_t* flags = nullptr;
    SCINT_HIP(hipHostMalloc(&flags, sizeof(int32_t) * 4 * (size_t)njobs));
    const int32_t rc = run_lanczos(jd, states, (int)njobs, (int)nmax, max_iter, flags, stream);
    if (rc != SCINT_OK) (void)hipStreamSynchronize(stream);     // `jobs` (the source of the copy above) and `flags` go away here
    (void)hipHostFree(flags);
    if (rc != SCINT_OK) return rc;
    const dim3 vgrid((unsigned)ceil_div(nmax, kVecBlock), (unsigned)njobs);
    hipLaunchKernelGGL(lanczos_ritz_kernel, vgrid, dim3(kVecBlock), 0, stream, jd, (cplx*)vec_out, vec_stride);
    hipLaunchKernelGGL(lanczos_scale_kernel, vgrid, dim3(kVecBlock), 0, stream, jd, (cplx*)vec_out, vec_stride, w_out);
    SCINT_LAUNCH_CHECK();
    SCINT_HIP(hipStreamSynchronize(stream));
    return SCINT_OK;
}


// ==============================================================================
// Largest singular value of rectangular theta-theta maps: the thin-screen search
// (singularvalue_calc, ththmod.py:496-513, swept by single_search_thin, :516-712)
// ==============================================================================
// The reference takes S[0] of a dense np.linalg.svd of every map.  Here: Lanczos on the Hermitian
// B = A^H A (n1 x n1, A = the n2 x n1 map), sigma_1 = sqrt(lambda_max(B)), with the same tridiagonal
// machinery (lanczos_check_kernel: Sturm-count multisection of T_k, Ritz residual beta_k |s_k| <= tol theta).
// Float64 only: the mixed-precision mode of the eigenvalue sweeps (scint_sweep_precision) does not apply.
//
// Per Lanczos step j (batched over the resident maps in blockIdx.y):
//   sv_matvec_kernel   a workgroup owns a strip of R rows: for each row (two at a time when the row is
//                      short) it loads the row into registers, forms y_r = A_r q_j (fixed-tree block
//                      reduction) and adds conj(A_r) y_r to its partial of z = A^H A q_j while the row is
//                      still in registers -- A is read from HBM once per step (16 n1 n2 bytes).  The
//                      partials [G][n1] are summed in block order by
//   sv_reduce_kernel   z = sum_b partial_b; u = z - beta_j q_{j-1}; partial q_j^H u
//   sv_update_kernel   alpha_j; w = u - alpha_j q_j; partial |w|^2
// and every 8 steps lanczos_check_kernel.  R and G depend on n2 only and every sum has a fixed order,
// so a map's result does not depend on which maps share its launches.
namespace scint {

constexpr int kSvMinRows = 4;

struct SvJob {
    const cplx* A;            // [n2][n1]
    int32_t n1, n2, max_steps, R, G, cls;
    cplx* W[2];               // ping-pong work vectors [n1]
    cplx* Q;                  // [2][n1] ring of q vectors
    cplx* zpart;              // [G][n1]
    double* alpha;            // [max_steps + 1]
    double* beta;             // [max_steps + 2]
    double* apart;            // [ceil(n1 / 256)]
    double* npart;            // [ceil(n1 / 256)]
    int32_t* state;           // [4] (shared with the check kernel's LanczosJob)
    double* lam;              // lambda_max(B) from the check kernel
    int32_t* status;          // from the check kernel
    int32_t* iters;
    const int32_t* raise;     // the gather's "NumPy would raise" word
};

__host__ __device__ inline int sv_rows_per_group(int n2) {
    const int r = (n2 + 255) / 256;
    return r > kSvMinRows ? r : kSvMinRows;
}

__device__ inline double sv_beta(const SvJob& jb) {
    return sqrt(sum_partials(jb.npart, (jb.n1 + kVecBlock - 1) / kVecBlock));
}

// q_j = w_j / beta_j; at j = 0 with a zero start vector the defined fallback is the constant unit vector
__device__ inline cplx sv_q(const SvJob& jb, const cplx* w, int c, int step, double beta) {
    if (step == 0 && beta == 0.0) return mk(1.0 / sqrt((double)jb.n1), 0.0);
    const double inv = beta > 0.0 ? 1.0 / beta : 0.0;
    const cplx v = w[c];
    return mk(v.x * inv, v.y * inv);
}

// w_0 = conj(row n2/2 of A) (the middle row, as Eval_calc starts from, ththmod.py:398); partial |w_0|^2.
// Maps the gather flagged, maps with an empty side and single-column maps take no Lanczos steps.
__global__ void __launch_bounds__(kVecBlock) sv_init_kernel(const SvJob* jobs) {
    __shared__ double red[kVecBlock / 64];
    const SvJob jb = jobs[blockIdx.y];
    const int n1 = jb.n1;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const bool skip = *jb.raise != 0 || n1 < 2 || jb.n2 < 1;
        jb.state[0] = skip ? 1 : 0;
        jb.state[1] = 0;
    }
    if (n1 < 2 || jb.n2 < 1 || (int)blockIdx.x * kVecBlock >= n1) return;
    const int c = blockIdx.x * kVecBlock + threadIdx.x;
    double p = 0.0;
    if (c < n1) {
        const cplx v = conj(jb.A[(int64_t)(jb.n2 / 2) * n1 + c]);
        jb.W[0][c] = v;
        p = norm2(v);
    }
    p = block_sum(p, red);
    if (threadIdx.x == 0) jb.npart[blockIdx.x] = p;
}

template <int NT, int K, int ROWS>
__global__ void __launch_bounds__(NT) sv_matvec_kernel(const SvJob* jobs, int step, int cls) {
    constexpr int NW = NT / 64;
    __shared__ cplx red[2][NW][ROWS];
    const SvJob jb = jobs[blockIdx.y];
    if (jb.cls != cls || (int)blockIdx.x >= jb.G || step >= jb.max_steps || jb.state[0]) return;
    const int n1 = jb.n1, n2 = jb.n2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const cplx* __restrict__ win = (step & 1) ? jb.W[1] : jb.W[0];
    const double beta = sv_beta(jb);
    cplx q[K], z[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int c = threadIdx.x + NT * k;
        q[k] = c < n1 ? sv_q(jb, win, c, step, beta) : mk(0.0, 0.0);
        z[k] = mk(0.0, 0.0);
    }
    const int r_begin = blockIdx.x * jb.R;
    const int r_end = min(r_begin + jb.R, n2);
    int par = 0;
    for (int r0 = r_begin; r0 < r_end; r0 += ROWS) {
        cplx a[ROWS][K];
#pragma unroll
        for (int rr = 0; rr < ROWS; ++rr) {
            const int row = r0 + rr;
            const cplx* __restrict__ rowp = jb.A + (int64_t)(row < r_end ? row : r0) * n1;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int c = threadIdx.x + NT * k;
                a[rr][k] = (row < r_end && c < n1) ? gload_nt(rowp + c) : mk(0.0, 0.0);
            }
        }
        cplx s[ROWS];
#pragma unroll
        for (int rr = 0; rr < ROWS; ++rr) {
            s[rr] = mk(0.0, 0.0);
#pragma unroll
            for (int k = 0; k < K; ++k) s[rr] = s[rr] + a[rr][k] * q[k];
            s[rr] = wave_sum(s[rr]);
        }
        if (lane == 0) {
#pragma unroll
            for (int rr = 0; rr < ROWS; ++rr) red[par][wave][rr] = s[rr];
        }
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < ROWS; ++rr) {
            cplx y = red[par][0][rr];
            for (int w = 1; w < NW; ++w) y = y + red[par][w][rr];
#pragma unroll
            for (int k = 0; k < K; ++k) z[k] = z[k] + conj(a[rr][k]) * y;
        }
        par ^= 1;
    }
    cplx* __restrict__ zp = jb.zpart + (int64_t)blockIdx.x * n1;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int c = threadIdx.x + NT * k;
        if (c < n1) zp[c] = z[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) jb.beta[step] = beta;
}

__global__ void __launch_bounds__(kVecBlock) sv_reduce_kernel(const SvJob* jobs, int step) {
    __shared__ double red[kVecBlock / 64];
    const SvJob jb = jobs[blockIdx.y];
    const int n1 = jb.n1;
    if (blockIdx.x * kVecBlock >= n1 || step >= jb.max_steps || jb.state[0]) return;
    const cplx* __restrict__ win = (step & 1) ? jb.W[1] : jb.W[0];
    cplx* __restrict__ wout = (step & 1) ? jb.W[0] : jb.W[1];
    const double beta = sv_beta(jb);
    const int c = blockIdx.x * kVecBlock + threadIdx.x;
    double p = 0.0;
    if (c < n1) {
        cplx z = jb.zpart[c];
        for (int b = 1; b < jb.G; ++b) z = z + jb.zpart[(int64_t)b * n1 + c];
        const cplx q = sv_q(jb, win, c, step, beta);
        cplx u = z;
        if (step > 0) {
            const cplx qp = jb.Q[(int64_t)((step + 1) & 1) * n1 + c];
            u = mk(u.x - beta * qp.x, u.y - beta * qp.y);
        }
        jb.Q[(int64_t)(step & 1) * n1 + c] = q;
        wout[c] = u;
        p = q.x * u.x + q.y * u.y;      // Re(conj(q) u)
    }
    p = block_sum(p, red);
    if (threadIdx.x == 0) jb.apart[blockIdx.x] = p;
}

__global__ void __launch_bounds__(kVecBlock) sv_update_kernel(const SvJob* jobs, int step) {
    __shared__ double red[kVecBlock / 64];
    const SvJob jb = jobs[blockIdx.y];
    const int n1 = jb.n1;
    if (blockIdx.x * kVecBlock >= n1 || step >= jb.max_steps || jb.state[0]) return;
    const int nvb = (n1 + kVecBlock - 1) / kVecBlock;
    const double alpha = sum_partials(jb.apart, nvb);
    cplx* __restrict__ w = (step & 1) ? jb.W[0] : jb.W[1];
    const cplx* __restrict__ q = jb.Q + (int64_t)(step & 1) * n1;
    const int c = blockIdx.x * kVecBlock + threadIdx.x;
    double p = 0.0;
    if (c < n1) {
        const cplx u = w[c], qv = q[c];
        const cplx v = mk(u.x - alpha * qv.x, u.y - alpha * qv.y);
        w[c] = v;
        p = norm2(v);
    }
    p = block_sum(p, red);
    if (threadIdx.x == 0) {
        jb.npart[blockIdx.x] = p;
        if (blockIdx.x == 0) jb.alpha[step] = alpha;
    }
}

// sigma_1 and the status of every map of the batch.  A breakdown right after the first step (B q_0 = alpha_0 q_0 exactly,
// the all-zero map among them) is exact: lambda = alpha_0.  A single column needs no iteration: sigma = its 2-norm (rows in order).
__global__ void __launch_bounds__(64) sv_finish_kernel(const SvJob* jobs, int njobs, double* sv_out, int32_t* status_out,
                                                       int32_t* iters_out) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= njobs) return;
    const SvJob jb = jobs[j];
    double sv;
    int32_t st, it;
    if (*jb.raise) { sv = nan(""); st = SCINT_E_ARG; it = 0; }
    else if (jb.n1 < 1 || jb.n2 < 1) { sv = nan(""); st = SCINT_E_EMPTY; it = 0; }
    else if (jb.n1 == 1) {
        double s = 0.0;
        for (int r = 0; r < jb.n2; ++r) s += norm2(jb.A[r]);
        sv = sqrt(s);
        st = isfinite(sv) ? SCINT_OK : SCINT_E_NONFINITE;
        it = 0;
    } else {
        st = *jb.status;
        it = *jb.iters;
        double lam = *jb.lam;
        if (st == SCINT_OK && it >= 1 && jb.beta[1] == 0.0 && isfinite(jb.alpha[0])) lam = jb.alpha[0];
        sv = st == SCINT_OK ? sqrt(fabs(lam)) : nan("");
    }
    sv_out[j] = sv;
    status_out[j] = st;
    iters_out[j] = it;
}

template <int NT, int K>
static void launch_sv_matvec(const SvJob* jobs_dev, dim3 grid, int step, int cls, hipStream_t stream) {
    constexpr int ROWS = K <= 8 ? 2 : 1;
    hipLaunchKernelGGL((sv_matvec_kernel<NT, K, ROWS>), grid, dim3(NT), 0, stream, jobs_dev, step, cls);
}

// class of a map by its row length: 256 threads x K columns each (K = 1, 2, 4, 8, 16), then 512 x 16 and 1024 x 16
// (a thread keeps K elements of the row, of q and of its z partial in registers: K = 16 is the most that fits)
static int sv_class(int n1) {
    if (n1 <= 256) return 0;
    if (n1 <= 512) return 1;
    if (n1 <= 1024) return 2;
    if (n1 <= 2048) return 3;
    if (n1 <= 4096) return 4;
    if (n1 <= 8192) return 5;
    return 6;
}
constexpr int kSvClasses = 7;
constexpr int64_t kSvMaxCols = 16384;

static void launch_sv_class(const SvJob* jobs_dev, int cls, unsigned gmax, unsigned nj, int step, hipStream_t stream) {
    const dim3 grid(gmax, nj);
    switch (cls) {
        case 0: launch_sv_matvec<256, 1>(jobs_dev, grid, step, cls, stream); break;
        case 1: launch_sv_matvec<256, 2>(jobs_dev, grid, step, cls, stream); break;
        case 2: launch_sv_matvec<256, 4>(jobs_dev, grid, step, cls, stream); break;
        case 3: launch_sv_matvec<256, 8>(jobs_dev, grid, step, cls, stream); break;
        case 4: launch_sv_matvec<256, 16>(jobs_dev, grid, step, cls, stream); break;
        case 5: launch_sv_matvec<512, 16>(jobs_dev, grid, step, cls, stream); break;
        default: launch_sv_matvec<1024, 16>(jobs_dev, grid, step, cls, stream); break;
    }
}

struct SvSlab {      // byte offsets inside one resident map's slab
    size_t A, W0, W1, Q, zpart, alpha, beta, apart, npart, result, lam, status, iters, total;
};
static SvSlab sv_slab(int64_t n1max, int64_t n2max, int max_steps) {
    SvSlab L;
    size_t off = 0;
    auto take = [&](size_t bytes) { off = align_up(off, 256); size_t o = off; off += bytes; return o; };
    const int64_t gmax = ceil_div(std::max<int64_t>(n2max, 1), sv_rows_per_group((int)std::max<int64_t>(n2max, 1)));
    L.A = take(sizeof(cplx) * (size_t)n1max * (size_t)n2max);
    L.W0 = take(sizeof(cplx) * n1max);
    L.W1 = take(sizeof(cplx) * n1max);
    L.Q = take(sizeof(cplx) * 2 * n1max);
    L.zpart = take(sizeof(cplx) * (size_t)gmax * n1max);
    L.alpha = take(sizeof(double) * (max_steps + 2));
    L.beta = take(sizeof(double) * (max_steps + 2));
    L.apart = take(sizeof(double) * ceil_div(n1max, kVecBlock));
    L.npart = take(sizeof(double) * ceil_div(n1max, kVecBlock));
    L.result = take(sizeof(double) * 4);
    L.lam = take(sizeof(double) * 2);
    L.status = take(sizeof(int32_t) * 2);
    L.iters = take(sizeof(int32_t) * 2);
    L.total = align_up(off, 256);
    return L;
}
// per batch: the slabs, the two job tables, the geometry table and the raise words
static size_t sv_batch_bytes(int64_t n1max, int64_t n2max, int max_steps, int64_t batch, int64_t ncs) {
    const SvSlab L = sv_slab(n1max, n2max, max_steps);
    return L.total * (size_t)batch + align_up(sizeof(SvJob) * batch, 256) + align_up(sizeof(LanczosJob) * batch, 256) +
           align_up(sizeof(ThinJob) * batch, 256) + align_up(sizeof(ThinGeomDev) * ncs, 256) +
           align_up(sizeof(int32_t) * batch, 256) + align_up(sizeof(int32_t) * 4 * batch, 256) + 4096;
}

}  // namespace scint

extern "C" int32_t scint_sv_sweep_multi_workspace_bytes(int64_t M1, int64_t M2, int64_t neta, int64_t batch,
                                                        int32_t max_iter, int64_t ncs, size_t* bytes) {
    SCINT_REQUIRE(bytes && M1 >= 1 && M2 >= 1 && neta >= 1 && batch >= 1 && max_iter >= 1 && ncs >= 1,
                  "sv_sweep_multi_workspace_bytes: bad arguments");
    SCINT_REQUIRE(M1 <= kSvMaxCols, "sv_sweep_multi_workspace_bytes: more than 16384 theta1 centres");
    const int steps = (int)std::min<int64_t>(max_iter, M1);
    *bytes = sv_batch_bytes(M1, M2, steps, std::min(batch, neta), ncs);
    return SCINT_OK;
}

extern "C" int32_t scint_sv_sweep_multi(const scint_c128* cs_stack, int64_t ncs, int64_t cs_stride,
                                        const int32_t* cs_index, const scint_thin_geom* geoms,
                                        const double* th1_stack, int64_t M1, const double* th2_stack, int64_t M2,
                                        const int32_t* ranges, const int32_t* check, const double* etas1,
                                        const double* etas2, int64_t neta, double tol, int32_t max_iter, int64_t batch,
                                        double* sv_out, int32_t* status_out, int32_t* iters_out, void* workspace,
                                        size_t workspace_bytes, void* stream_) {
    SCINT_REQUIRE(cs_stack && cs_index && geoms && th1_stack && th2_stack && ranges && check && etas1 && etas2 && sv_out &&
                  status_out && iters_out && workspace, "sv_sweep_multi: null pointer");
    SCINT_REQUIRE(ncs >= 1 && neta >= 1 && batch >= 1 && max_iter >= 1 && tol > 0, "sv_sweep_multi: bad arguments");
    SCINT_REQUIRE(M1 >= 1 && M2 >= 1 && M1 <= kSvMaxCols && M2 < (1 << 30), "sv_sweep_multi: bad grid sizes");
    for (int64_t c = 0; c < ncs; ++c)
        SCINT_REQUIRE(geoms[c].ntau >= 2 && geoms[c].nfd >= 2 && geoms[c].dtau > 0 && geoms[c].dfd > 0 &&
                      geoms[c].ntau * geoms[c].nfd <= cs_stride, "sv_sweep_multi: bad geometry");
    int64_t n1max = 1, n2max = 1;
    for (int64_t e = 0; e < neta; ++e) {
        const int32_t* r = ranges + 6 * e;
        SCINT_REQUIRE(cs_index[e] >= 0 && cs_index[e] < ncs, "sv_sweep_multi: cs_index out of range");
        SCINT_REQUIRE(r[0] >= 0 && r[1] >= 0 && r[0] + (int64_t)r[1] <= M2 && r[2] >= 0 && r[3] >= 0 &&
                      r[2] + (int64_t)r[3] <= M1 && r[4] >= 0 && r[4] <= r[5] && r[5] <= r[3],
                      "sv_sweep_multi: crop or cut outside the grids");
        n2max = std::max<int64_t>(n2max, r[1]);
        n1max = std::max<int64_t>(n1max, r[3]);
    }
    batch = std::min(batch, neta);
    const int steps_cap = (int)std::min<int64_t>(max_iter, M1);
    size_t need = 0;
    scint_sv_sweep_multi_workspace_bytes(M1, M2, neta, batch, max_iter, ncs, &need);
    if (workspace_bytes < need) { set_error("scint: sv_sweep_multi workspace too small"); return SCINT_E_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    // the slabs are laid out for the largest map of the call (M1 x M2 bounds every crop)
    const SvSlab L = sv_slab(M1, M2, steps_cap);
    Carver cv(workspace, workspace_bytes);
    char* slabs = cv.take<char>(L.total * (size_t)batch);
    SvJob* sv_dev = cv.take<SvJob>(batch);
    LanczosJob* lj_dev = cv.take<LanczosJob>(batch);
    ThinJob* tj_dev = cv.take<ThinJob>(batch);
    ThinGeomDev* g_dev = cv.take<ThinGeomDev>(ncs);
    int32_t* raise_dev = cv.take<int32_t>(batch);
    int32_t* states_dev = cv.take<int32_t>(4 * batch);     // [batch][4]: done flag, steps (one read-back per check)
    if (!cv.ok()) { set_error("scint: sv_sweep_multi workspace too small"); return SCINT_E_WORKSPACE; }
    std::vector<ThinGeomDev> gh(ncs);
    for (int64_t c = 0; c < ncs; ++c) gh[c] = to_dev(geoms[c]);
    SCINT_HIP(hipMemcpyAsync(g_dev, gh.data(), sizeof(ThinGeomDev) * ncs, hipMemcpyHostToDevice, stream));
    int32_t* flags = nullptr;
    SCINT_HIP(hipHostMalloc(&flags, sizeof(int32_t) * 4 * (size_t)batch));
    std::vector<SvJob> sv(batch);
    std::vector<LanczosJob> lj(batch);
    std::vector<ThinJob> tj(batch);
    int32_t rc = SCINT_OK;
    for (int64_t e0 = 0; e0 < neta && rc == SCINT_OK; e0 += batch) {
        const int nj = (int)std::min<int64_t>(batch, neta - e0);
        int64_t max_dom = 0, gmax = 1, n1b = 1;
        bool cls_used[kSvClasses] = {};
        int nmax_steps = 1;
        for (int j = 0; j < nj; ++j) {
            const int64_t e = e0 + j;
            const int32_t* r = ranges + 6 * e;
            char* s = slabs + L.total * (size_t)j;
            ThinJob& t = tj[j];
            const int c = cs_index[e];
            t.cs = (const cplx*)cs_stack + (int64_t)c * cs_stride;
            t.th1 = th1_stack + (int64_t)c * M1;
            t.th2 = th2_stack + (int64_t)c * M2;
            t.eta1 = etas1[e]; t.eta2 = etas2[e]; t.two_eta1 = 2 * etas1[e]; t.two_eta2 = 2 * etas2[e];
            t.r0 = r[0]; t.n2 = r[1]; t.c0 = r[2]; t.n1 = r[3]; t.cut0 = r[4]; t.cut1 = r[5];
            t.M1 = (int32_t)M1; t.M2 = (int32_t)M2; t.check = check[e] ? 1 : 0; t.geom = c;
            t.out = (cplx*)(s + L.A);
            t.raise = raise_dev + j;
            max_dom = std::max<int64_t>(max_dom, t.check ? M1 * M2 : (int64_t)r[1] * r[3]);
            SvJob& b = sv[j];
            b.A = t.out; b.n1 = r[3]; b.n2 = r[1];
            b.max_steps = (int)std::min<int64_t>(max_iter, std::max(r[3], 1));
            b.R = sv_rows_per_group(std::max(r[1], 1));
            b.G = (int)ceil_div(std::max(r[1], 1), b.R);
            b.cls = sv_class(std::max(r[3], 1));
            b.W[0] = (cplx*)(s + L.W0); b.W[1] = (cplx*)(s + L.W1); b.Q = (cplx*)(s + L.Q);
            b.zpart = (cplx*)(s + L.zpart);
            b.alpha = (double*)(s + L.alpha); b.beta = (double*)(s + L.beta);
            b.apart = (double*)(s + L.apart); b.npart = (double*)(s + L.npart);
            b.state = states_dev + 4 * j; b.lam = (double*)(s + L.lam);
            b.status = (int32_t*)(s + L.status); b.iters = (int32_t*)(s + L.iters);
            b.raise = t.raise;
            gmax = std::max<int64_t>(gmax, b.G);
            n1b = std::max<int64_t>(n1b, r[3]);
            if (b.n1 >= 2 && b.n2 >= 1) { cls_used[b.cls] = true; nmax_steps = std::max(nmax_steps, b.max_steps); }
            LanczosJob& l = lj[j];
            l = LanczosJob{};
            l.n = b.n1; l.max_steps = b.max_steps; l.qslots = 2; l.rank = b.n2;
            l.alpha = b.alpha; l.beta = b.beta; l.apart = b.apart; l.npart = b.npart;
            l.svec = nullptr; l.result = (double*)(s + L.result);
            l.state = b.state; l.eig_out = b.lam; l.status_out = b.status; l.iters_out = b.iters;
            l.tol = tol;
        }
        SCINT_HIP(hipMemsetAsync(raise_dev, 0, sizeof(int32_t) * nj, stream));
        SCINT_HIP(hipMemcpyAsync(tj_dev, tj.data(), sizeof(ThinJob) * nj, hipMemcpyHostToDevice, stream));
        SCINT_HIP(hipMemcpyAsync(sv_dev, sv.data(), sizeof(SvJob) * nj, hipMemcpyHostToDevice, stream));
        SCINT_HIP(hipMemcpyAsync(lj_dev, lj.data(), sizeof(LanczosJob) * nj, hipMemcpyHostToDevice, stream));
        const int slot = profiler().begin(kProfGather, stream);
        rc = launch_thin_gather(tj_dev, g_dev, nj, max_dom, stream);
        profiler().end(kProfGather, slot, stream);
        if (rc != SCINT_OK) break;
        const dim3 vgrid((unsigned)ceil_div(n1b, kVecBlock), (unsigned)nj);
        hipLaunchKernelGGL(sv_init_kernel, vgrid, dim3(kVecBlock), 0, stream, sv_dev);
        SCINT_LAUNCH_CHECK();
        int step = 0, chunk = 16;
        const int cap = nmax_steps;
        bool any = false;
        for (int k = 0; k < kSvClasses; ++k) any = any || cls_used[k];
        while (any && step < cap) {
            const int upto = std::min(cap, step + chunk);
            for (; step < upto; ++step) {
                const int ms = profiler().begin(kProfMatvec, stream);
                for (int k = 0; k < kSvClasses; ++k)
                    if (cls_used[k]) launch_sv_class(sv_dev, k, (unsigned)gmax, (unsigned)nj, step, stream);
                profiler().end(kProfMatvec, ms, stream);
                hipLaunchKernelGGL(sv_reduce_kernel, vgrid, dim3(kVecBlock), 0, stream, sv_dev, step);
                hipLaunchKernelGGL(sv_update_kernel, vgrid, dim3(kVecBlock), 0, stream, sv_dev, step);
            }
            SCINT_LAUNCH_CHECK();
            hipLaunchKernelGGL(lanczos_check_kernel, dim3((unsigned)nj), dim3(64), 0, stream, lj_dev, step,
                               step >= cap ? 1 : 0);
            SCINT_LAUNCH_CHECK();
            SCINT_HIP(hipMemcpyAsync(flags, states_dev, sizeof(int32_t) * 4 * (size_t)nj, hipMemcpyDeviceToHost, stream));
            SCINT_HIP(hipStreamSynchronize(stream));
            if (profiler().enabled) profiler().collect();
            bool all = true;
            for (int j = 0; j < nj && all; ++j) all = flags[4 * j] != 0;
            if (all) break;
            chunk = 8;
        }
        hipLaunchKernelGGL(sv_finish_kernel, dim3((unsigned)ceil_div(nj, 64)), dim3(64), 0, stream, sv_dev, nj,
                           sv_out + e0, status_out + e0, iters_out + e0);
        SCINT_LAUNCH_CHECK();
        SCINT_HIP(hipStreamSynchronize(stream));     // the job tables are rewritten for the next batch
    }
    (void)hipHostFree(flags);
    return rc;
}
