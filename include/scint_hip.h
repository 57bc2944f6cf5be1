/*
 * scint_hip.h -- C ABI of libscint_hip.so: the MI355X (gfx950) implementation of
 * scintools' secondary-spectrum + theta-theta hot path.
 *
 * The reference (danielreardon/scintools) is pure Python and has no FFI; the
 * boundary below is what a ctypes binding inside the reference would call in
 * place of the NumPy/SciPy lines cited on every entry point (paths relative to
 * /root/reference/scintools).  INTEGRATION.md shows that binding.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller unless marked SCINT_HOST;
 *   - arrays are C-contiguous; complex data is interleaved (re, im) float64,
 *     i.e. numpy complex128 / HIP double2;
 *   - sizes are int64_t, flags int32_t, the return value is an int32_t status:
 *     0 = ok, >0 = SCINT_E_*; the message is available from scint_last_error();
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  All
 *     work is enqueued on it; only entry points documented as synchronous
 *     wait for it.  The sweep entry points split the resident curvatures into two
 *     groups, one driven on `stream`, one on an internal stream, and queue each
 *     group's Lanczos steps two chunks ahead of the convergence flags they have
 *     read (so no stream waits for the host); scint_chisq_sweep additionally
 *     drives two internal streams for the model steps of retired curvatures.
 *     Internal streams are per host thread and device.  The sweep entry points
 *     return with every stream drained;
 *   - no function throws, allocates caller-visible memory, or keeps pointers to
 *     caller buffers after it returns.  Persistent library-owned state, all small
 *     and created on first use: a mutex-guarded cache of FFT twiddle tables per
 *     device; an 8 KiB reduction scratch per (device, stream) used by scint_mean /
 *     scint_chisq; per host thread a pinned flag buffer (4 int32 per resident
 *     curvature) and staging for the sweep's job tables, and, per device, the internal
 *     streams mentioned above and a note of which kernels' LDS-size attribute has been set.
 */
#ifndef SCINT_HIP_H
#define SCINT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Marks a pointer parameter that is read or written by the CPU during the call; every other pointer is device memory.
 * (Empty for the compiler; the Python binding derives its argument types from these prototypes: scintools_amd/_lib.py.) */
#define SCINT_HOST

/* The version of the argument lists below, returned by scint_version(): an argument added in the middle of a list shifts every
 * pointer after it, so a binding refuses a library of another version.  An entry point may be ADDED without a new version.
 *   101: scint_profile_end takes the length of the caller's arrays;
 *   102: scint_sweep_workgroups;
 *   103: scint_chisq_sweep takes crop_group;
 *   104: calc_sspec through persistent kernels (no signature change; the version binds library and package: _lib.load checks it);
 *   105: scint_mosaic_* / scint_chunk_cut;
 *   106: scint_retrieval_tail takes class_id (one-row back-map, pair counts per class);
 *   107: the rank-1 Hermitian back-map on a uniform theta grid is rev_diag_kernel (scint_rev_map leaves which kernel ran in word 9
 *        of its workspace; SCINT_REV_DIAG=0 keeps the general kernel);
 *   108: scint_two_curve_map / scint_sv_sweep_multi (the thin-screen search, scint_thin_geom);
 *   (the VLBI entry points -- scint_cs_complex_batch / scint_vlbi_composite / scint_eigh_top_batch -- and the batched 1-D ACF fit --
 *   scint_acf1d_fit -- and the approximate 2-D one -- scint_acf2d_approx_fit -- and the biharmonic fill -- scint_inpaint_biharmonic --
 *   and the ACFs and secondary spectra of a stack -- scint_acf_batch, scint_sspec_batch -- and the arc fits of a stack --
 *   scint_arc_profile_batch, scint_arc_peak_fit -- and the preconditioned biharmonic fill -- scint_inpaint_biharmonic_lines -- only ADD symbols: no bump; a build without them fails at load, which checks every declared symbol) */
#define SCINT_ABI_VERSION 108

#define SCINT_OK 0
#define SCINT_E_ARG 1        /* bad size / null pointer / unsupported option   */
#define SCINT_E_HIP 2        /* a HIP runtime call failed                      */
#define SCINT_E_WORKSPACE 3  /* workspace too small                            */
#define SCINT_E_NOCONV 4     /* eigen iteration hit max_iter (per-eta status)  */
#define SCINT_E_EMPTY 5      /* reduced theta-theta has < 2 points (per-eta)   */
#define SCINT_E_NONFINITE 6  /* non-finite eigenvalue (per-eta)                */

typedef struct { double re, im; } scint_c128;

/* Geometry of a conjugate spectrum CS[ntau, nfd] and of the theta grid, as the
 * reference derives it inside thth_map (ththmod.py:83-97) -- computed on the
 * host by the wrapper with the reference's exact NumPy expressions so that the
 * floor() in the gather sees bit-identical operands. */
typedef struct {
    int64_t ntau, nfd;     /* CS shape: tau is the slow axis                    */
    double tau0, dtau;     /* tau[0], np.diff(tau).mean()            [us]       */
    double fd0, dfd;       /* fd[0],  np.diff(fd).mean()             [mHz]      */
    double tau_max;        /* abs(tau.max())  (crop, ththmod.py:153)            */
    double fd_max;         /* abs(fd.max())   (crop, ththmod.py:154)            */
    double tau1_step;      /* tau[1]-tau[0]   (rev_map bin edges, :214-216)     */
    double fd1_step;       /* fd[1]-fd[0]     (rev_map bin edges, :211-213)     */
} scint_cs_geom;

/* Geometry of a conjugate spectrum for the thin-screen map two_curve_map (ththmod.py:1557-1636), which indexes from the
 * SECOND sample of each axis: tau_inv = ((eta1 th1^2 - eta2 th2^2) - tau[1] + dtau/2) // dtau and
 * fd_inv = ((th1 - th2) - fd[1] + dfd/2) // dfd.  Host-computed with the reference's NumPy expressions. */
typedef struct {
    int64_t ntau, nfd;     /* CS shape: tau is the slow axis                    */
    double tau1, dtau;     /* tau[1], np.diff(tau).mean()            [us]       */
    double fd1, dfd;       /* fd[1],  np.diff(fd).mean()             [mHz]      */
} scint_thin_geom;

/* ---- diagnostics -------------------------------------------------------- */
int32_t scint_version(void);
/* HOST buffer; copies the calling thread's last error text. */
int32_t scint_last_error(char* SCINT_HOST buf, size_t n);
/* Number of visible HIP devices (0 if none): lets the wrapper fail loudly. */
int32_t scint_device_count(void);

/* Optional per-kernel timing for the benchmark: between begin and end every launch of
 * the theta-theta gather kernel ([0]) and of the eigen mat-vec kernel ([1]) is bracketed
 * by hipEvents on its stream.  end() synchronises the device and returns, per kernel, the length
 * in milliseconds of the UNION of its launch intervals (the sweep drives two streams, so
 * launches may overlap), the plain SUM of the individual launch spans (sum / launches is the
 * average a kernel trace reports) and the launch counts.  HOST arrays of `count` entries; the
 * library fills min(count, 8) of them and never writes beyond `count` (since version 101: the
 * entry point wrote a fixed 2, then 3, entries before): [2] is the complex64 mat-vec of the
 * mixed-precision sweep (scint_sweep_precision), [3] the rank-1 back-map and [4] the model
 * transform + chi^2 of the model steps of scint_chisq_sweep; since version 102 [5], [6], [7] are the
 * three kernels of the two-trip scint_sspec (input copy + sums, strided axis, row transforms with
 * |.|^2 / dB).  Not thread-safe; off by default. */
int32_t scint_profile_begin(void);
int32_t scint_profile_end(double* SCINT_HOST ms_out /*[count]*/, double* SCINT_HOST ms_sum_out /*[count]*/,
                          int64_t* SCINT_HOST launches_out /*[count]*/, int32_t count);

/* ---- secondary spectrum: Dynspec.calc_sspec core (dynspec.py:3665-3721) -- */
/* dyn[nf,nt] -> sec[(halve? nrfft/2 : nrfft), ncfft] in dB, where
 * nrfft/ncfft = 2*nextpow2(nf/nt) (dynspec.py:3677-3678).
 * win_t[nt], win_f[nf]: tapers of scint_utils.get_window (:810-832) or NULL.
 * pd_fd[ncfft], pd_td[nrfft/2]: post-darkening sin^2 vectors (dynspec.py:3706-3711),
 * required iff prewhite.  Workspace: scint_sspec_workspace_bytes(). */
int32_t scint_sspec_workspace_bytes(int64_t nf, int64_t nt, size_t* SCINT_HOST bytes);
int32_t scint_sspec(const double* dyn, int64_t nf, int64_t nt,
                    const double* win_t, const double* win_f,
                    int32_t prewhite, int32_t halve,
                    const double* pd_fd, const double* pd_td,
                    double* sec_out, void* workspace, size_t workspace_bytes,
                    void* stream);

/* scint_sspec of every problem of a stack: sec_out[b][rows][ncfft] (rows = nrfft / 2 if halve, else nrfft) holds, BIT FOR BIT, what
 * scint_sspec writes for stack[b][nf][nt] with the same windows, prewhite, halve and post-darkening vectors (b < B, 1 <= B <=
 * 65535): each problem's own mean and windowed mean, then prewhitening, |.|^2, post-darkening, 10 log10 and fftshift as there.
 * Problems whose padded half-length is below 256 on either axis (nf <= 128 or nt <= 128, or halve = 0) go through scint_sspec's
 * generic transform as slots / grid.z of the same kernels and its reductions in their fixed order: the number of launches does
 * not depend on B, and the workspace grows with B.  Larger problems (both half-lengths 256 .. 8192, halve = 1) are scint_sspec's
 * persistent kernels, which take one problem at a time: they run problem after problem on ONE problem's workspace, and their
 * launches grow with B.  No atomics.  Asynchronous on `stream`. */
int32_t scint_sspec_batch_workspace_bytes(int64_t B, int64_t nf, int64_t nt, int32_t halve, size_t* SCINT_HOST bytes);
int32_t scint_sspec_batch(const double* stack, int64_t B, int64_t nf, int64_t nt,
                          const double* win_t, const double* win_f,
                          int32_t prewhite, int32_t halve,
                          const double* pd_fd, const double* pd_td,
                          double* sec_out, void* workspace, size_t workspace_bytes,
                          void* stream);

/* ---- conjugate spectrum: single_search lines ththmod.py:777-787 ---------- */
/* CS = fftshift(fft2(pad(dspec, right/bottom by npad*shape, pad_value)));
 * rows r with mask_lo <= r < mask_hi are zeroed (the |tau| < tauMask rows).
 * If `incoherent` != 0 the output is abs(CS) + 0j (ththmod.py:801).
 * cs_out[(npad+1)*nf, (npad+1)*nt].  Any sizes (non powers of two go through a
 * chirp-z pass).  Workspace: scint_cs_workspace_bytes(). */
int32_t scint_cs_workspace_bytes(int64_t nf, int64_t nt, int64_t npad, size_t* SCINT_HOST bytes);
int32_t scint_cs(const double* dspec, int64_t nf, int64_t nt, int64_t npad,
                 double pad_value, int64_t mask_lo, int64_t mask_hi, int32_t incoherent,
                 scint_c128* cs_out, void* workspace, size_t workspace_bytes, void* stream);

/* mean of a device array (np.mean of the chunk), synchronous, HOST result. */
int32_t scint_mean(const double* x, int64_t n, double* SCINT_HOST mean_out, void* stream);

/* ---- CS -> theta-theta: thth_map + thth_redmap (ththmod.py:56-173) ------- */
/* th_cents[M]: bin centres (ththmod.py:83-84).  keep_idx[N]: indices (into
 * th_cents, ascending) of the centres kept by the crop (:153-155); pass the
 * identity for plain thth_map.  thth_out[N,N].  hermitian: ththmod.py:108-114. */
int32_t scint_thth_map(const scint_c128* cs, const scint_cs_geom* SCINT_HOST geom,
                       const double* th_cents, int64_t M,
                       const int32_t* keep_idx, int64_t N,
                       double eta, int32_t hermitian,
                       scint_c128* thth_out, void* stream);

/* ---- eta sweep: the Eval_calc loop of single_search (ththmod.py:788-799) -- */
/* For each eta_i: reduced theta-theta (as above, hermitian) -> dominant
 * 'largest algebraic' eigenvalue seeded with the middle row (Eval_calc,
 * ththmod.py:396-401) -> eigs_out[i] = |w|.
 * keep_idx[neta*M] / keep_n[neta]: per-eta crop (host-computed, device arrays).
 * status_out[i] != 0 -> the wrapper stores NaN (ththmod.py:795-799).
 * iters_out[i]: Lanczos steps used (for the roofline accounting); may be NULL.
 * eigs_out/status_out/iters_out are DEVICE arrays and need no initialisation (the library presets status to a
 * failure code and the step counts to 0 on the caller's stream; eigenvector rows of the *_vec entry points are
 * zero beyond their N_i entries, chi^2 of a curvature whose crop leaves nothing stays NaN).
 * NOT asynchronous: like every *_sweep entry point this one drives the caller's stream AND the library's internal
 * streams from a host-side scheduler that reads convergence flags back, and returns with all of them drained -- results
 * are complete (in device memory) on return, and an asynchronous fault of any queued kernel is reported by this call. */
int32_t scint_eval_sweep_workspace_bytes(int64_t M, int64_t neta, int64_t batch,
                                         int32_t max_iter, size_t* SCINT_HOST bytes);
/* Operand precision of the ITERATION of the eigenvalue sweeps (scint_eval_sweep, scint_eval_sweep_multi), per process:
 *   0  float64 throughout (the default): every Lanczos pass streams the complex128 tiles;
 *   1  mixed: the passes stream a complex64 copy of theta-theta (float64 vectors and sums), and the eigenvalue that
 *      is returned is the Ritz value of a certificate pass on the complex128 tiles that satisfies the float64 sweep's
 *      own a-posteriori bound, evaluated in float64 on that matrix -- same tolerance, same status codes
 *      (csrc/eigen_packed.hip, "Mixed precision").  iters_out[i] then counts the passes of both phases (complex64 and
 *      complex128; scint_sweep_stats splits the bytes).  Eigenvector sweeps are not affected.
 *   2  mixed-all: as 1, and the eigenPAIR sweeps (scint_eigvec_sweep*, scint_chisq_sweep) iterate on the complex64 copy too,
 *      to the eigenvalue rule; the run that starts from the two Ritz vectors on the complex128 tiles then continues to
 *      the eigenvector rule of the float64 sweep (residual of the float64 matrix, in float64).
 *  -1  query.
 * Returns the previous mode.  Call it BEFORE the *_workspace_bytes of a sweep: the mixed sweep needs a larger
 * workspace.  The environment variable SCINT_SWEEP_PRECISION=mixed|mixed-all|f64 sets the initial mode. */
int32_t scint_sweep_precision(int32_t mode);
/* Scheduling of the sweeps, per process (the host-side scheduler of eigen_packed.hip; the reference has no counterpart --
 * its loop, ththmod.py:788-799, is sequential): chunks queued ahead of the convergence flags the host has seen (`depth`,
 * 1 or 2), Lanczos passes between convergence checks (`check_every`, 1..16), slot groups on separate streams (`groups`,
 * 1 or 2).  0 restores the measured default, -1 leaves a setting as it is.  Initial values: SCINT_SWEEP_DEPTH /
 * SCINT_CHECK_EVERY / SCINT_SWEEP_GROUPS in the environment, read once.  `depth` and `groups` change no bit of any result;
 * `check_every` decides after which passes the stopping rule is looked at, so a curvature may stop a pass earlier or later
 * -- a value inside the same tolerance, not the same bits (tests/test_gpu_edges.py).  They exist for that test and for
 * bench.py's one-slot-group leg. */
int32_t scint_sweep_schedule(int32_t depth, int32_t check_every, int32_t groups);
/* Diagnostics of the calling thread's last sweep (any of the sweep entry points), for the roofline accounting:
 * out[0] algorithmic bytes of its complex64 passes (4 n (n + 1) each), out[1] of its complex128 passes (8 n (n + 1)),
 * out[2] curvatures that went through a certificate, out[3] complex128 passes those certificates took. */
int32_t scint_sweep_stats(double* SCINT_HOST out /*[4]*/);
/* Mat-vec workgroups ONE theta-theta matrix of `nb` 64-row blocks contributes to a launch of the sweep (`complex64` != 0: of the
 * complex64 kernel of the mixed sweep) -- block rows per workgroup and column tiles per strip are build constants of the library
 * (csrc/packed.hpp).  For callers that size the `batch` argument of the sweeps: resident curvatures x this = workgroups per
 * launch (scintools_amd/ththmod.py: default_batch).  Returns the count (>= 1), or -SCINT_E_ARG for nb < 1. */
int32_t scint_sweep_workgroups(int32_t nb, int32_t complex64);
/* Environment variables the library reads (each ONCE per process unless said otherwise; none selects another kernel family or
 * changes a result beyond what is said here):
 *   SCINT_SWEEP_PRECISION = f64 | mixed | mixed-all   initial value of scint_sweep_precision();
 *   SCINT_SWEEP_DEPTH, SCINT_CHECK_EVERY, SCINT_SWEEP_GROUPS   initial values of scint_sweep_schedule();
 *   SCINT_STRIP_LEN = n   column tiles per mat-vec workgroup, at most the build's maximum (csrc/packed.hpp): for the test that
 *                         proves a sweep's values do not depend on the strip shape beyond rounding (tests/test_emu_cpu.py).
 *   SCINT_SSPEC_MAXGRID = n   (read per call) an upper bound on the workgroups of calc_sspec's persistent kernels, for the test
 *                         that runs several rows / column pairs per workgroup at small shapes; changes no bit of the result.
 * (SCINT_CHISQ_MODEL and SCINT_SSPEC_GENERIC of round 4 are gone: no test used them; the model route of the chi^2 sweep is
 *  reached with a mask or a non-finite dspec, the generic calc_sspec route with halve = 0 or lengths outside 256..8192.) */
/* Limits common to every sweep entry point below (eval / eigvec / chisq, single and _multi): a conjugate spectrum must hold
 * fewer than 2^31 elements (ntau * nfd; the packed gather indexes it with 32 bits) -- SCINT_E_ARG otherwise, before anything
 * is queued.  scint_thth_map / scint_rev_map / scint_modeler index with 64 bits and have no such limit. */
int32_t scint_eval_sweep(const scint_c128* cs, const scint_cs_geom* SCINT_HOST geom,
                         const double* th_cents, int64_t M,
                         const int32_t* keep_idx, const int32_t* SCINT_HOST keep_n,
                         const double* SCINT_HOST etas, int64_t neta,
                         double tol, int32_t max_iter, int64_t batch,
                         double* eigs_out, int32_t* status_out, int32_t* iters_out,
                         void* workspace, size_t workspace_bytes, void* stream);

/* The same sweep over MANY conjugate spectra of one shape in a single batched call -- the
 * chunk loop of Dynspec.fit_thetatheta (dynspec.py:1681-1719), where every chunk has its own
 * CS, eta grid and (frequency-scaled) edges.  cs_stack[ncs][ntau][nfd] with cs_stride elements
 * between spectra; geoms[ncs] (HOST); th_stack[ncs][M]; curvature e reads spectrum
 * cs_index[e] (HOST) and keeps keep_idx[e*M ..] of th_stack[cs_index[e]]. */
int32_t scint_eval_sweep_multi_workspace_bytes(int64_t M, int64_t neta, int64_t batch,
                                               int32_t max_iter, int64_t ncs, size_t* SCINT_HOST bytes);
int32_t scint_eval_sweep_multi(const scint_c128* cs_stack, int64_t ncs, int64_t cs_stride,
                               const int32_t* SCINT_HOST cs_index, const scint_cs_geom* SCINT_HOST geoms,
                               const double* th_stack, int64_t M,
                               const int32_t* keep_idx, const int32_t* SCINT_HOST keep_n,
                               const double* SCINT_HOST etas, int64_t neta,
                               double tol, int32_t max_iter, int64_t batch,
                               double* eigs_out, int32_t* status_out, int32_t* iters_out,
                               void* workspace, size_t workspace_bytes, void* stream);

/* Same sweep, but returning the eigenpair (signed w and unit eigenvector) of every eta: the
 * eigsh call of modeler (ththmod.py:308) for a whole curvature sweep.  vec_out[neta, vec_stride]
 * (vec_stride >= M; row i holds keep_n[i] entries).  Stops on the Ritz residual (tol). */
int32_t scint_eigvec_sweep_workspace_bytes(int64_t M, int64_t neta, int64_t batch,
                                           int32_t max_iter, size_t* SCINT_HOST bytes);
int32_t scint_eigvec_sweep(const scint_c128* cs, const scint_cs_geom* SCINT_HOST geom,
                           const double* th_cents, int64_t M,
                           const int32_t* keep_idx, const int32_t* SCINT_HOST keep_n,
                           const double* SCINT_HOST etas, int64_t neta,
                           double tol, int32_t max_iter, int64_t batch,
                           double* w_out, scint_c128* vec_out, int64_t vec_stride,
                           int32_t* status_out, int32_t* iters_out,
                           void* workspace, size_t workspace_bytes, void* stream);

/* The crop of thth_redmap (ththmod.py:153-155) for every curvature of a sweep, on the device:
 * keep_idx[e*M ..] = ascending indices i with th_cents[i]^2 * etas[e] < tau_max and |th_cents[i]| < fd_half
 * (NumPy's expression, same roundings), keep_n[e] their count -- the tables the sweeps take.  th_cents,
 * keep_idx, keep_n: DEVICE; etas: HOST.  Asynchronous. */
int32_t scint_sweep_keep(const double* th_cents, int64_t M, const double* SCINT_HOST etas, int64_t neta,
                         double tau_max, double fd_half, int32_t* keep_idx, int32_t* keep_n, void* stream);

/* The same for MANY conjugate spectra of one shape in one batched sweep (arguments as
 * scint_eval_sweep_multi): the eigenpairs of all chunks of Dynspec.thetatheta_chunks -- one
 * modeler() call per chunk in the reference, dynspec.py:1765-1826 / ththmod.py:1455 -- in ONE call. */
int32_t scint_eigvec_sweep_multi_workspace_bytes(int64_t M, int64_t neta, int64_t batch,
                                                 int32_t max_iter, int64_t ncs, size_t* SCINT_HOST bytes);
int32_t scint_eigvec_sweep_multi(const scint_c128* cs_stack, int64_t ncs, int64_t cs_stride,
                                 const int32_t* SCINT_HOST cs_index, const scint_cs_geom* SCINT_HOST geoms,
                                 const double* th_stack, int64_t M,
                                 const int32_t* keep_idx, const int32_t* SCINT_HOST keep_n,
                                 const double* SCINT_HOST etas, int64_t neta,
                                 double tol, int32_t max_iter, int64_t batch,
                                 double* w_out, scint_c128* vec_out, int64_t vec_stride,
                                 int32_t* status_out, int32_t* iters_out,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* ---- dominant eigenpair of a given Hermitian matrix (eigsh k=1 'LA') ----- */
/* a[n,n] row-major.  v0[n] start vector or NULL (then a fixed pseudo-random
 * start, as modeler's eigsh call has no v0, ththmod.py:308).  w_out[1],
 * vec_out[n] (unit 2-norm) device outputs; status_out[1], iters_out[1]. */
int32_t scint_eigh_top_workspace_bytes(int64_t n, int32_t max_iter, size_t* SCINT_HOST bytes);
int32_t scint_eigh_top(const scint_c128* a, int64_t n, const scint_c128* v0,
                       double tol, int32_t max_iter,
                       double* w_out, scint_c128* vec_out,
                       int32_t* status_out, int32_t* iters_out,
                       void* workspace, size_t workspace_bytes, void* stream);

/* The same for MANY dense Hermitian matrices in one set of launches: job j is the n[j] x n[j] row-major matrix at
 * a_stack + j * a_stride, started from its row start_row[j] (HOST [njobs]; NULL = the middle row n[j] / 2).  w_out[njobs],
 * vec_out[njobs][vec_stride] (row j holds n[j] entries, the rest is left as it was), status_out[njobs], iters_out[njobs]: device.
 * n, start_row: HOST.  A job with n[j] < 2 gets SCINT_E_EMPTY.  A job's arithmetic does not depend on which jobs share the call.
 * Synchronous (the done flags are read back every few steps, as in scint_eigh_top).  njobs <= 65535. */
int32_t scint_eigh_top_batch_workspace_bytes(int64_t nmax, int32_t max_iter, int64_t njobs, size_t* SCINT_HOST bytes);
int32_t scint_eigh_top_batch(const scint_c128* a_stack, int64_t a_stride, const int32_t* SCINT_HOST n,
                             const int32_t* SCINT_HOST start_row /*or NULL*/, int64_t njobs, double tol, int32_t max_iter,
                             double* w_out, scint_c128* vec_out, int64_t vec_stride,
                             int32_t* status_out, int32_t* iters_out,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ---- theta-theta -> CS: rev_map (ththmod.py:176-271) --------------------- */
/* thth[N,N] on centres th_cents[N] (already re-centred) -> recov[ntau,nfd].
 * If `rank1` != 0, thth is not read: thth = |w| V V^H with V = vec[N], w = *w
 * (device), which is modeler's thth2_red (ththmod.py:312-313).
 * Every pixel of recov_out is written (no zero-fill needed).  The per-pixel sums are
 * order-independent: each addend is split on a fixed binary grid so that the float64 LDS
 * accumulations are exact (thth.hip, RevSplit), hence the image is bit-reproducible from run
 * to run like np.histogram2d's.  Workspace: scint_rev_map_workspace_bytes() (a few words).
 * Version 107: the rank-1 Hermitian image (modeler's) on a UNIFORM theta grid -- theta_k = theta_0 + k step to 1e-9 of a
 * step, checked on the device for every call; the centres of linspace edges and any contiguous crop of them are one -- is
 * formed by another kernel (thth.hip, rev_diag_kernel: whole diagonals j = i + s of a Doppler column instead of a search for
 * every theta_i's partners; plain float64 sums in ONE fixed order, so equally bit-reproducible; the same pairs in the same
 * pixels, each pixel within its rounding of the split sums').  After the call word 9 (uint64) of the workspace is 1 if that
 * kernel formed the image, 0 if the general one did.  Environment: SCINT_REV_DIAG=0 keeps every image (also the chi^2 sweep's)
 * on the general kernel. */
int32_t scint_rev_map_workspace_bytes(size_t* SCINT_HOST bytes);
int32_t scint_rev_map(const scint_c128* thth, const scint_c128* vec, const double* w,
                      int32_t rank1, const double* th_cents, int64_t N,
                      const scint_cs_geom* SCINT_HOST geom, double eta, int32_t hermitian,
                      scint_c128* recov_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- model dynamic spectrum: ifft2(ifftshift(recov)).real (ththmod.py:322-324) ----------
 * recov[ntau, nfd] -> model_out[ntau, nfd].  Computed as a complex-to-real transform of the
 * Hermitian part of ifftshift(recov) when both lengths are powers of two (nfd in 32..8192): an
 * identity for any input, equal to the complex transform's real part up to rounding. */
int32_t scint_model_workspace_bytes(int64_t ntau, int64_t nfd, size_t* SCINT_HOST bytes);
int32_t scint_model_from_recov(const scint_c128* recov, int64_t ntau, int64_t nfd,
                               double* model_out, void* workspace, size_t workspace_bytes,
                               void* stream);

/* ---- complex inverse: scale * ifft2(ifftshift(x))[:crop_rows, :crop_cols] ----------------
 * The wavefield step of single_chunk_retrieval (ththmod.py:1465-1468).  out[crop_rows, crop_cols]. */
int32_t scint_ifft2_shifted(const scint_c128* in, int64_t rows, int64_t cols, double scale,
                            int64_t crop_rows, int64_t crop_cols, scint_c128* out,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ---- the mosaic of the retrieved chunks (ththmod.py:1492-1554) and the chunks themselves (dynspec.py:1782-1790) ----------
 * Replaces the host loop of `mosaic`: a chunk is rotated onto the sum of the chunks before it and added under its taper, with
 * NumPy's own summation order and product arithmetic restated on the device (csrc/mosaic.hip) so that the result equals the
 * host loop's bit for bit.  The reference's loop is sequential, but chunk (cf, ct) only meets its four predecessors
 * (cf, ct-1), (cf-1, ct-1 .. ct+1): chunks with equal 2 cf + ct are independent and their windows disjoint, so the wrapper walks
 * 2 (ncf - 1) + nct STEPS and hands each step's chunks to one launch -- every pixel still receives its addends in the
 * reference's order.  Per step: scint_mosaic_phase (sums_out[k][2] <- sum over chunk k's window of (E * conj(chunk)) * mask,
 * device memory), mean / numpy.angle / numpy.exp in NumPy on the host, scint_mosaic_add (E[window] += (chunk * mask) *
 * phases[k]).  jobs: device int64 [count][4] = (offset of the window's first element in E, chunk index in the stack `chunks`
 * [.][cwf][cwt], row taper, column taper), count <= 64; tapers rows[4][cwf], cols[4][cwt] (variant 2 * has-a-neighbour-before +
 * has-a-neighbour-after), mask[r][c] = rows[rv][r] * cols[cv][c]; ldE the wavefield's row length; phases: HOST [count][2].
 * numpy_fused, two properties of the HOST's NumPy that the wrapper measures: bit 0 = it multiplies complex arrays with fused
 * multiply-adds (re = fma(ar, br, -(ai bi)): its x86 SIMD loops) rather than the plain expressions; bit 1 = it evaluates
 * chunk_old * conj(chunk_new) with the operands swapped (temporary elision, chunks of 256 KiB and more).
 * The library keeps one small plan per window size in device memory (as it does FFT twiddle tables).
 * scint_chunk_cut: chunks_out[k] = nan_to_num(dyn[r0[k] : r0[k] + cwf, c0[k] : c0[k] + cwt] - nanmean(that window)),
 * pad_out[k] = mean(chunks_out[k]) (the padding value of the conjugate spectrum, ththmod.py:783); r0 / c0 device int32.
 * colmajor: the host array is Fortran-ordered (numpy.copy keeps the order, NumPy's sums then walk a window column by column);
 * `dyn` itself is row-major here either way.
 * Workspace for both: scint_mosaic_workspace_bytes(cwf, cwt, nchunk) (nchunk = count for scint_mosaic_phase). */
int32_t scint_mosaic_workspace_bytes(int64_t cwf, int64_t cwt, int64_t nchunk, size_t* SCINT_HOST bytes);
int32_t scint_mosaic_phase(const scint_c128* E, int64_t ldE, const scint_c128* chunks, int64_t cwf, int64_t cwt,
                           const int64_t* jobs, int64_t count, const double* rows, const double* cols, int32_t numpy_fused,
                           void* workspace, size_t workspace_bytes, double* sums_out, void* stream);
int32_t scint_mosaic_add(scint_c128* E, int64_t ldE, const scint_c128* chunks, int64_t cwf, int64_t cwt,
                         const int64_t* jobs, int64_t count, const double* rows, const double* cols, int32_t numpy_fused,
                         const double* SCINT_HOST phases, void* stream);
int32_t scint_chunk_cut(const double* dyn, int64_t nf, int64_t nt, const int32_t* r0, const int32_t* c0, int64_t nchunk,
                        int64_t cwf, int64_t cwt, int32_t colmajor, double* chunks_out, double* pad_out, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---- the fitted mosaics (ththmod.py:1708-2310: rotMos / rotFit / rotDer, fullMos / fullMosFit / fullMosGrad / fullMosHess) ----
 * W = sum_k A_k exp(i phi_k) mask_k (.) chunk_k over the stack `chunks` [ncf * nct][cwf][cwt] in half-overlapping windows (sizes
 * even along an axis of several chunks), tapers rows[4][cwf] / cols[4][cwt] as above.  coef: DEVICE [ncf * nct][3] = amplitude,
 * then real and imaginary part of exp(1j * phase) as the host's NumPy evaluated it (chunk 0: exp(0j)).  full = 0: rotMos (the
 * amplitudes are not read) with the objective -sum |W|^2; full = 1: fullMos with nansum(((|W|^2 - dspec) / noise)^2), dspec and
 * noise DEVICE [F][T] (the mosaic's extent, F = (ncf - 1) (cwf / 2) + cwf).
 * scint_mosaic_fit_eval: W [F][T] <- the mosaic, every pixel's 1-4 terms added in the reference's order and evaluated as NumPy
 * does (numpy_fused bit 0 as for scint_mosaic_add): equal to the host loop bit for bit.  want = 0: that is all (dspec, noise, out
 * and the workspace may be null); 1: out[0] <- the objective; 2: also out[1 + k] <- d/d phi_k and, full, out[1 + n + k] <-
 * d/d A_k for every chunk k (k = 0 included: the caller drops its phase).  out: DEVICE [1 + 2 n].  Three launches, fixed-order
 * sums, no floating-point atomics: equal inputs give equal bits.
 * scint_mosaic_fit_hess: H [2 n - 1][2 n - 1] <- fullMosHess at the W that scint_mosaic_fit_eval formed from the same coef
 * (parameters: phases of chunks 1 .. n - 1, then the n amplitudes); numpy.sum, so a NaN or zero of dspec / noise shows in the
 * entries it touches; zero outside the neighbour band; exactly symmetric (where the reference writes an entry from the visits
 * (N, M) and (M, N), the later one's value, as there). */
int32_t scint_mosaic_fit_workspace_bytes(int64_t ncf, int64_t nct, int64_t cwf, int64_t cwt, size_t* SCINT_HOST bytes);
int32_t scint_mosaic_fit_eval(const scint_c128* chunks, int64_t ncf, int64_t nct, int64_t cwf, int64_t cwt, const double* rows,
                              const double* cols, const double* coef, int32_t full, int32_t numpy_fused, const double* dspec,
                              const double* noise, scint_c128* W, int32_t want, double* out, void* workspace,
                              size_t workspace_bytes, void* stream);
int32_t scint_mosaic_fit_hess(const scint_c128* chunks, int64_t ncf, int64_t nct, int64_t cwf, int64_t cwt, const double* rows,
                              const double* cols, const double* coef, const double* dspec, const double* noise,
                              const scint_c128* W, double* H, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the per-chunk steps of Dynspec.thetatheta_chunks, a whole group of chunks per call (dynspec.py:1765-1826; the reference
 * maps single_chunk_retrieval, ththmod.py:1390-1476, over the chunks) --------------------------------------------------------
 * scint_cs_batch: scint_cs of every chunk of dstack [n][nf][nt] into cs_stack [n][R][C]; pads (HOST [n]) the padding values,
 * mask_lohi (HOST [n][2]) the masked delay rows of each.  scint_retrieval_tail: per chunk k with keep_n[k] >= 2 the theta-theta
 * of the E field (zeros with row N/2 = rows[k][:N] = conj(V) sqrt(w), ththmod.py:1459-1461), its non-Hermitian back-map on
 * geoms[k] / etas[k] / th_red[k][:N], and scale * ifft2(ifftshift(.))[:nf, :nt] -> out[k] (scint_ifft2_shifted); chunks with
 * keep_n[k] < 2 are left untouched.  The back-map is rev_map's arithmetic (ththmod.py:176-271, hermetian=False) without the N x N
 * matrix: a pixel is (sum of the row's weights that fall in it, in increasing j) x 1 / (number of ALL N^2 pairs that fall in it),
 * and those counts are formed once per CLASS -- class_id (HOST [n]): consecutive chunks with equal ids share theta grid, curvature
 * and axes (the chunks of one frequency row of an observation).  rows [n][M] complex, th_red [n][M], out [n][nf][nt]: device;
 * keep_n, class_id, geoms, etas: HOST. */
int32_t scint_cs_batch(const double* dstack, int64_t n, int64_t nf, int64_t nt, int64_t npad, const double* SCINT_HOST pads,
                       const int64_t* SCINT_HOST mask_lohi, int32_t incoherent, scint_c128* cs_stack, void* workspace,
                       size_t workspace_bytes, void* stream);
int32_t scint_retrieval_tail_workspace_bytes(int64_t M, int64_t ntau, int64_t nfd, size_t* SCINT_HOST bytes);
int32_t scint_retrieval_tail(const scint_c128* rows, const double* th_red, const int32_t* SCINT_HOST keep_n, const int32_t* SCINT_HOST class_id,
                             const scint_cs_geom* SCINT_HOST geoms, const double* SCINT_HOST etas, int64_t n, int64_t M, int64_t nf, int64_t nt,
                             double scale, scint_c128* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- multi-station (VLBI) phase retrieval: VLBI_chunk_retrieval (ththmod.py:1223-1387), a group of chunks per call
 * A chunk of n_dish stations has nspec = n_dish (n_dish + 1) / 2 spectra in the reference's order [I1, V12, .., V1N, I2, V23, .., IN]:
 * the dynamic spectra go through scint_cs_batch (mean-padded, real), the visibilities through
 * scint_cs_complex_batch: cs_stack[k] = fftshift(fft2(np.pad(xstack[k], right/bottom by npad * shape, 0))) of COMPLEX
 *   xstack [n][nf][nt], rows mask_lohi[k][0] <= r < mask_lohi[k][1] (HOST [n][2]) written as zero (ththmod.py:1313-1325).
 *   Workspace: scint_cs_workspace_bytes().
 * scint_vlbi_composite: the composite theta-theta of every chunk (ththmod.py:1292-1362).  Spectrum idx of chunk k is the
 *   conjugate spectrum at cs_stack + cs_slot[k * nspec + idx] * cs_stride (cs_slot: HOST) on geoms[k] (HOST); the chunk keeps the
 *   keep_n[k] (HOST) centres keep_idx[k * M ..] of th_stack[k * M ..] (the crop of thth_redmap: one per chunk) at curvature etas[k]
 *   (HOST).  With N = keep_n[k], the composite is the dense row-major [n_dish N][n_dish N] matrix at comp_out + k * comp_stride:
 *   for station pair (d1, d1 + d2) the reduced theta-theta T of spectrum idx(d1, d2) (ththmod.py:1345-1349) is block
 *   (d1 + d2, d1) and conj(T^T) block (d1, d1 + d2); T is thth_redmap with hermetian=True when d2 == 0 (ththmod.py:108-114) and
 *   hermetian=False otherwise (no forcing, no nan_to_num, nothing zeroed).  Every element of the composite is written; a CS pixel
 *   is read once for both blocks.  An element whose Doppler index lies below -nfd (NumPy raises IndexError) is NaN.
 *   Workspace: scint_vlbi_composite_workspace_bytes().  Synchronous.
 * The dominant eigenpair of the composites: scint_eigh_top_batch; the wavefields: scint_retrieval_tail with n_dish rows per chunk. */
int32_t scint_cs_complex_batch(const scint_c128* xstack, int64_t n, int64_t nf, int64_t nt, int64_t npad,
                               const int64_t* SCINT_HOST mask_lohi, scint_c128* cs_stack, void* workspace,
                               size_t workspace_bytes, void* stream);
int32_t scint_vlbi_composite_workspace_bytes(int64_t nchunk, int64_t n_dish, size_t* SCINT_HOST bytes);
int32_t scint_vlbi_composite(const scint_c128* cs_stack, int64_t cs_stride, const int64_t* SCINT_HOST cs_slot,
                             const scint_cs_geom* SCINT_HOST geoms, const double* th_stack, int64_t M,
                             const int32_t* keep_idx, const int32_t* SCINT_HOST keep_n, const double* SCINT_HOST etas,
                             int64_t nchunk, int64_t n_dish, scint_c128* comp_out, int64_t comp_stride,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ---- Gerchberg-Saxton iterations of Dynspec.gerchberg_saxton (dynspec.py:1868-1875) -------
 * wavefield[rows, cols] in place.  Per iteration: fft2, zero the natural-order delay rows
 * zero_lo <= k < zero_hi (the tau < 0 half), ifft2, then where pos != 0 replace the amplitude
 * by amp (= sqrt(dyn)) keeping the phase.  Workspace: scint_gs_workspace_bytes(). */
int32_t scint_gs_workspace_bytes(int64_t rows, int64_t cols, size_t* SCINT_HOST bytes);
int32_t scint_gerchberg_saxton(scint_c128* wavefield, int64_t rows, int64_t cols,
                               const double* amp, const uint8_t* pos,
                               int64_t zero_lo, int64_t zero_hi, int32_t niter,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ---- autocovariance: Dynspec.calc_acf(method='direct') (dynspec.py:3780-3797) ------------
 * acf_out[2nf, 2nt] = real(fftshift(ifft2(|fft2(dyn - mean, s=[2nf, 2nt])|^2))), / max if
 * normalise; the mean is subtracted only if subtract_mean (the reference skips it for
 * input_dyn).  dyn must be finite (the reference takes the mean of the valid pixels only). */
int32_t scint_acf_workspace_bytes(int64_t nf, int64_t nt, size_t* SCINT_HOST bytes);
int32_t scint_acf(const double* dyn, int64_t nf, int64_t nt, int32_t subtract_mean, int32_t normalise,
                  double* acf_out, void* workspace, size_t workspace_bytes, void* stream);

/* scint_acf of every problem of a stack: acf_out[b][2nf][2nt] holds, BIT FOR BIT, what scint_acf writes for stack[b][nf][nt]
 * (b < B, 1 <= B <= 65535) -- each problem's own mean when subtract_mean, its own maximum when normalise, and for a degenerate
 * problem (a constant one with subtract_mean: an all-zero ACF, then 0 / 0) what scint_acf gives.  The problems go through
 * scint_acf's row and column passes as slots / grid.z of the same kernels and through its reductions in their fixed order, so the
 * number of launches does not depend on B; no atomics.  The workspace grows with B (the complex intermediates: 16 * 2nf * 2nt
 * bytes per problem and array); a caller that has to bound it splits the stack and asks scint_acf_batch_workspace_bytes for each
 * part's need.  Asynchronous on `stream`. */
int32_t scint_acf_batch_workspace_bytes(int64_t B, int64_t nf, int64_t nt, size_t* SCINT_HOST bytes);
int32_t scint_acf_batch(const double* stack, int64_t B, int64_t nf, int64_t nt, int32_t subtract_mean, int32_t normalise,
                        double* acf_out, void* workspace, size_t workspace_bytes, void* stream);

/* Dynspec.calc_acf(method='sspec') (dynspec.py:3798-3807) from the full-frame (halve = 0, prewhite = 0) secondary spectrum in dB
 * sec_db[R][C] of scint_sspec: acf_out[R][C] = real(fftshift(fft2(10**(fftshift(sec_db) / 10)))), / max if normalise.  R >= 2 and
 * C >= 16 are powers of two (every full-frame spectrum's are).  -inf dB (an exact zero of power) counts as 0.  Asynchronous. */
int32_t scint_acf_sspec_workspace_bytes(int64_t R, int64_t C, size_t* SCINT_HOST bytes);
int32_t scint_acf_sspec(const double* sec_db, int64_t R, int64_t C, int32_t normalise, double* acf_out,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- what the no-fit scintillation measurements read from the device (csrc/scintpar.hpp) ---------------------------------
 * Dynspec.get_scint_params(method='nofit') (dynspec.py:2570-2648), get_acf_tilt (:2358-2413) and cut_dyn (:3158-3271): the ACF
 * stays in device memory and the reference's host arithmetic gets the few samples it reads.  All asynchronous on `stream`;
 * no atomics: equal inputs give equal bits.
 * scint_acf_cuts: cuts_out[0 .. R - R/2) = acf[R/2 + i][C/2] and cuts_out[R - R/2 .. R - R/2 + C - C/2) = acf[R/2][C/2 + j]
 *   (the integer halves of dynspec.py:2576-2578) for acf[R][C]: a gather, the bits of the ACF's own elements.
 * scint_dyn_moments: stats_out[3] = (count, mean, population variance) of the pixels of dyn[n] that are finite and non-zero
 *   (dynspec.py:2633-2635).  Two-stage sums in a fixed order; the variance is a second pass about the mean.  An empty selection
 *   gives count 0 and NaN, as NumPy.  Workspace: scint_dyn_moments_workspace_bytes().
 * scint_acf_row_peaks: for k < nrows, col_out[k] = the FIRST column at which acf[rows[k], :] has its maximum (np.argmax; a tie
 *   resolves to the lowest column, NaN samples are never the maximum), win_out[k][7] = acf[rows[k], col - 3 : col + 4],
 *   flag_out[k] = 0; a window that would cross column 0 or C is not read: flag_out[k] = 1 and win_out[k] = 0; a rows[k] outside
 *   [0, R) gives flag_out[k] = 2.  rows, col_out, flag_out: device int32.  1 <= nrows < 2^31, C < 2^31.
 * scint_segment_cut: segs_out[ii * ntseg + jj][r][c] = dyn[ii * fnum + r][jj * tnum + c] for dyn[nf][nt], ii < nfseg,
 *   jj < ntseg (dynspec.py:3201-3203); nfseg * fnum <= nf and ntseg * tnum <= nt (SCINT_E_ARG otherwise). */
int32_t scint_acf_cuts(const double* acf, int64_t R, int64_t C, double* cuts_out, void* stream);
int32_t scint_dyn_moments_workspace_bytes(size_t* SCINT_HOST bytes);
int32_t scint_dyn_moments(const double* dyn, int64_t n, double* stats_out, void* workspace, size_t workspace_bytes,
                          void* stream);
int32_t scint_acf_row_peaks(const double* acf, int64_t R, int64_t C, const int32_t* rows, int64_t nrows,
                            int32_t* col_out, double* win_out, int32_t* flag_out, void* stream);
int32_t scint_segment_cut(const double* dyn, int64_t nf, int64_t nt, int64_t fnum, int64_t tnum, int64_t nfseg,
                          int64_t ntseg, double* segs_out, void* stream);

/* ---- batched 1-D ACF fits of tau and dnu: Dynspec.get_scint_params(method='acf1d') of the reference, for a stack ----------
 * Replaces, per problem b < B of acf[B][R][C] (as scint_acf writes an ACF), dynspec.py:2575-2608 (the two half-cuts
 * acf[R/2:, C/2] and acf[R/2, C/2:], the start values wn, amp, tau, dnu and the crop to nscale scales or 5 samples), :2650-2687
 * (the weights; `bartlett`: Brockwell & Davis 7.2.5 on the CROPPED cut) and :2698-2702 with scint_models.py:62-120: the
 * least-squares fit of
 *   r_t = (y_t - amp exp(-(x_t / tau)^alpha) (1 - x_t / max x_t)) w_t,  r_f = (y_f - amp exp(-x_f ln2 / dnu) (1 - x_f / max x_f)) w_f
 * over (tau, dnu, amp), and alpha when alpha_varies (started at `alpha`), by Levenberg-Marquardt in (log tau, log dnu, log amp,
 * alpha) -- the scales stay positive, as the reference's min=0 -- with an analytic Jacobian.  One wavefront per problem, at most
 * max_iter (1 .. 100000) passes each: no problem can spin.  No atomics; equal inputs give equal bits, whatever the neighbours.
 *   dt, df      sample steps of the two cuts; bw[B], tobs[B] (device): the fallbacks for dnu and tau without a crossing;
 *   values_out [B][4]  tau, dnu, amp, alpha;  errors_out [B][4]: sqrt(diag((J^T J)^-1 chi^2 / (N - nvary))) in these external
 *               parameters, N = all residuals (the two zero-weighted first samples included); alpha and 0 when alpha is fixed;
 *   stats_out [B][2]   chi^2 = sum r^2 and chi^2 / (N - nvary);   niter_out[B] passes made;
 *   status_out[B]      0 converged (the last step moved no scale by more than 1e-12 of itself, alpha by 1e-12), 1 max_iter reached,
 *               2 singular normal matrix (or a start scale that is not positive), 3 non-finite sample in a half-cut,
 *               4 non-finite cost or step.  Every status but 0 leaves NaN in values_out, errors_out and stats_out;
 *   setup_out [B][6] or NULL: the start values wn, amp, tau, dnu and the crop lengths n_t, n_f (as doubles; NaN start values for
 *               status 3).
 * Workspace (scint_acf1d_fit_workspace_bytes), per problem 2 (n_tc + n_fc) doubles with n_tc = C - C/2, n_fc = R - R/2: the
 * half-cuts y_t[n_tc], y_f[n_fc], then their weights w_t, w_f (n_t and n_f of them valid).  R, C >= 6.  Asynchronous. */
int32_t scint_acf1d_fit_workspace_bytes(int64_t B, int64_t R, int64_t C, size_t* SCINT_HOST bytes);
int32_t scint_acf1d_fit(const double* acf, int64_t B, int64_t R, int64_t C, double dt, double df, const double* bw,
                        const double* tobs, double nscale, int32_t full_frame, int32_t weighted, int32_t bartlett,
                        double alpha, int32_t alpha_varies, int32_t max_iter, double* values_out, double* errors_out,
                        double* stats_out, int32_t* niter_out, int32_t* status_out, double* setup_out, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---- batched approximate 2-D ACF fits of tau, dnu and the phase gradient: get_scint_params(method='acf2d_approx') ---------
 * (dynspec.py:2710-2842 with scint_models.py:123-161; csrc/acf2d.hpp).  The host chooses per problem b < B of acf[B][R][C] a
 * window rect[b] = (f0, nfw, t0, ntw) (rows f0 .. f0 + nfw, columns t0 .. t0 + ntw; device int32) centred on the ACF's maximum
 * and the start values start[b] = (tau, dnu, amp, alpha, phasegrad); the fit minimises the sum of squares of
 *   r = (y - amp exp(-(|(t - 60 phasegrad f) / tau|^(3 alpha / 2) + |f ln2 / dnu|^(3/2))^(2/3)) (1 - |t| / tobs) (1 - |f| / bw)) w
 * over the window, t and f the ticks of np.linspace(-tobs, tobs, C + 1)[:-1] and np.linspace(-bw, bw, R + 1)[:-1], by
 * Levenberg-Marquardt in (log tau, log dnu, log amp, phasegrad, alpha) with an analytic Jacobian; tau leaves the problem when
 * !tau_varies, alpha when !alpha_varies.  The weights are computed in the kernel: W0 = sqrt(nsub nchan (T / max tticks)
 * (F / max fticks)) with T = tobs - |t|, F = bw - |f| (1 when !weighted), zero where not finite or where y - 1 / W0 < 0, rolled by
 * -1 in both axes (the reference's double fftshift on an odd window), zero at the window's centre.  One 256-thread workgroup per
 * problem, one launch, at most max_iter (1 .. 100000) passes each; no atomics, equal inputs give equal bits.
 *   scint_acf_argmax   idx_out[b] (device int32) = np.argmax(acf[b]): ties resolve to the lowest flat index, NaN is never the
 *               maximum.  R C < 2^31.
 *   status_in[B]       device int32; non-zero: the host gave up on the problem (its status is passed on, NaN outputs);
 *   values_out [B][5]  tau, dnu, amp, alpha, phasegrad;  errors_out [B][5]: sqrt(diag((J^T J)^-1 chi^2 / (N - nvary))) in these
 *               external parameters, N = nfw ntw (zero-weight points included), 0 for a parameter that does not vary;
 *   stats_out [B][2]   chi^2 and chi^2 / (N - nvary);  niter_out[B] passes made;  nnz_out[B] number of non-zero weights;
 *   status_out[B]      0 .. 4 as scint_acf1d_fit (3: passed on from status_in), 5 the rectangle has an even or empty side or
 *               leaves the ACF (nothing outside acf[b] is ever read).  Every status but 0 leaves NaN in values, errors, stats.
 * Workspace (scint_acf2d_approx_fit_workspace_bytes): 256 bytes, and with return_setup per problem 2 R C doubles: the window's y,
 * row-major in the first nfw ntw, then from R C on its weights.  R, C >= 6, R C < 2^31.  Asynchronous.
 * scint_acf2d_approx_model: out[nf][nt] = (ydata - model(tdata[j], fdata[i])) weights, ydata NULL = 0, weights NULL = 1, the
 *   weight at ((nf - 1) / 2, (nt - 1) / 2) zero (scint_models.py:156-158): scint_acf_model_2d_approx for device arrays. */
int32_t scint_acf_argmax(const double* acf, int64_t B, int64_t R, int64_t C, int32_t* idx_out, void* stream);
int32_t scint_acf2d_approx_fit_workspace_bytes(int64_t B, int64_t R, int64_t C, int32_t return_setup, size_t* SCINT_HOST bytes);
int32_t scint_acf2d_approx_fit(const double* acf, int64_t B, int64_t R, int64_t C, const int32_t* rect, const double* start,
                               const int32_t* status_in, const double* bw, const double* tobs, double nsub, double nchan,
                               int32_t weighted, int32_t tau_varies, int32_t alpha_varies, int32_t max_iter,
                               double* values_out, double* errors_out, double* stats_out, int32_t* niter_out,
                               int32_t* status_out, int32_t* nnz_out, int32_t return_setup, void* workspace,
                               size_t workspace_bytes, void* stream);
int32_t scint_acf2d_approx_model(const double* tdata, int64_t nt, const double* fdata, int64_t nf, const double* ydata,
                                 const double* weights, double tau, double dnu, double amp, double alpha, double phasegrad,
                                 double tobs, double bw, double* out, void* stream);

/* ---- chi^2: sum((model[:nf,:nt]-dspec)[mask]**2)/N (ththmod.py:364-367) --- */
/* mask: uint8[nf*nt] or NULL (= isfinite(dspec)).  out: DEVICE double[1].  Asynchronous. */
int32_t scint_chisq(const double* model, int64_t ld_model, const double* dspec,
                    int64_t nf, int64_t nt, const uint8_t* mask, double noise_n,
                    double* out, void* stream);

/* ---- modeler / chisq_calc sweep: [chisq_calc(dspec, CS, tau, fd, eta, edges, N, mask) for eta in etas]
 * (ththmod.py:330-368 over :274-327) in ONE call.  The dominant eigenPAIR of every curvature is found
 * by the batched Lanczos sweep (as scint_eigvec_sweep); as each curvature retires, its model step --
 * rank-1 rev_map of |w| V V^H, inverse FFT, chi^2 against dspec[nf, nt] -- is chained on an internal
 * stream beside the Lanczos steps of the curvatures still resident, without returning to the host.
 * When the model is not cropped (ntau == nf, nfd == nt), mask is NULL and dspec is finite, chi^2 is taken
 * from recov and fft2(dspec) by Parseval's identity instead (the same sum to rounding; no inverse FFT); on that route
 * the curvatures one chunk of the sweep retires go through their model step TOGETHER (<= 8 per set of launches), and
 * back-map and chi^2 touch only the delay rows |tau| <= |eta| max theta^2 a curvature can reach (recov is exactly 0
 * elsewhere; those rows contribute sum |fft2(dspec)|^2).  The workspace holds up to 8 images per internal stream for it.
 *   th_red   DEVICE [neta, M]: row e = the N_e centres of the reduced edges (ththmod.py:157-172 then
 *            :204-205), host-computed like the other grid quantities;
 *   crop_group HOST [neta] or NULL: curvatures with the same non-negative id keep the same theta centres (their th_red rows
 *            are equal element for element: the caller's promise); -1 = on its own.  Which theta_j pair with theta_i in a
 *            Doppler column does not depend on the curvature, so the back-maps of the two largest groups (>= 8 members)
 *            share one partner table per group instead of walking the centres per curvature (since version 103).  Version
 *            107: a curvature whose th_red row is a uniform grid (tested on the device before the sweep: every grid of the
 *            reference's path is one) takes the diagonal back-map of scint_rev_map instead, which has no partners to look
 *            up; tables are built only for groups of curvatures that are not;
 *   mask     DEVICE uint8[nf*nt] or NULL (= isfinite(dspec));
 *   chisq_out DEVICE [neta]: sum((model[:nf,:nt]-dspec)[mask]**2)/noise_n; NaN-filled by the call, and left NaN for a
 *            curvature whose crop keeps fewer than THREE centres (two have no mean edge step: the reference's
 *            rev_map raises there, ththmod.py:166) or whose eigen-solve failed (see status_out);
 *   w_out / vec_out / status_out / iters_out as in scint_eigvec_sweep.
 * Synchronous like the other sweep entry points (returns with all internal streams drained). */
/* Version 107: when, on that route, the axes are symmetric about 0 (even lengths, x0 = -(n / 2) step to 1e-7 of a step: every
 * fft_axis), chi^2 of a uniform-grid curvature comes from the back-map's accumulators -- the rank-1 Hermitian histogram is then
 * mirror-symmetric, fft2(model) at an interior pixel IS recov there, and the workgroup that holds the pixel adds |recov - D|^2
 * itself: the image is neither written nor read back (Doppler column 0 and delay row 0, whose mirrors are off the axes, still
 * are, and take the partner formula).  A pair that sits on a bin edge with its mirrored pair NOT in the mirrored pixel raises the
 * curvature's flag (the edges np.histogram2d computes mirror each other only to ~1e-9 of a step); flagged curvatures are done
 * again from a written image before the call returns.  SCINT_CHISQ_FUSE=0 (environment) keeps every image written.
 * scint_chisq_sweep_last_route: of the LAST scint_chisq_sweep of the process -- fused = 1 if it took chi^2 from the accumulators,
 * redone = the curvatures it did again (tests, bench.py). */
int32_t scint_chisq_sweep_last_route(int32_t* SCINT_HOST fused, int64_t* SCINT_HOST redone);
int32_t scint_chisq_sweep_workspace_bytes(int64_t M, int64_t neta, int64_t batch, int32_t max_iter,
                                          int64_t ntau, int64_t nfd, int64_t nf, int64_t nt,
                                          size_t* SCINT_HOST bytes);
int32_t scint_chisq_sweep(const scint_c128* cs, const scint_cs_geom* SCINT_HOST geom, const double* th_cents,
                          int64_t M, const int32_t* keep_idx, const int32_t* SCINT_HOST keep_n,
                          const double* SCINT_HOST etas, int64_t neta, double tol, int32_t max_iter,
                          int64_t batch, const double* th_red, const int32_t* SCINT_HOST crop_group /*[neta] or NULL*/,
                          const double* dspec, int64_t nf, int64_t nt,
                          const uint8_t* mask, double noise_n, double* chisq_out, double* w_out,
                          scint_c128* vec_out, int64_t vec_stride, int32_t* status_out, int32_t* iters_out,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ==== arc normalisation: scale_dyn / norm_sspec / fit_arc ==== */

/* ---- equal-wavelength resample: Dynspec.scale_dyn(scale='lambda') (dynspec.py:3948-3957) ----
 * Every time column of dyn[nf, nt] is interpolated with the not-a-knot cubic spline
 * (scipy interp1d(kind='cubic')) from the channel frequencies to nout target frequencies, and
 * the rows are written flipped (np.flipud): out[nout-1-k, :] = S(target k).
 * The spline is solved in second-derivative form (moments M[i]); the tridiagonal system
 * depends on the frequency axis only, so the caller passes its Thomas factors (DEVICE arrays):
 *   h[nf-1] knot spacings; interior rows i = 1..nf-2 with right-hand side
 *   r_i = 6*((y[i+1]-y[i])/h[i] - (y[i]-y[i-1])/h[i-1]):  forward  d_i = (r_i - sub[i]*d_{i-1})*inv[i],
 *   backward M[i] = d_i - sup[i]*M[i+1];  not-a-knot ends (HOST end[4]):
 *   M[0] = end[0]*M[1] + end[1]*M[2],  M[nf-1] = end[2]*M[nf-2] + end[3]*M[nf-3];
 *   per target k: interval idx[k] and coef[k][4]: S = c0*y[i] + c1*y[i+1] + c2*M[i] + c3*M[i+1].
 * `reverse` != 0: the frequency axis is descending and row i of the spline is dyn row nf-1-i.
 * Both sweeps contract, so they run in independent frequency blocks of `block_rows` rows, each
 * started `warm` rows early from zero; the caller sizes `warm` from the factors so that the
 * start-up error is below rounding (block_rows <= 0: one block, the plain sequential sweep).
 * workspace: 2*nf*nt doubles. */
int32_t scint_spline_resample(const double* dyn, int64_t nf, int64_t nt, int32_t reverse,
                              const double* h, const double* sub, const double* inv,
                              const double* sup, const double* SCINT_HOST end /*[4]*/,
                              int64_t block_rows, int64_t warm,
                              const int32_t* idx, const double* coef, int64_t nout,
                              double* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Dynspec.norm_sspec row loop (dynspec.py:2093-2127) ------------------------------------
 * For delay rows r = 0..nr-1 (row row0+r of sspec[., ld], nc columns, dB):
 *   scale = sqrt(yaxis[row0+r]/eta); sel = |fdop| <= maxnormfac*scale;
 *   norm_out[r, k] = np.interp(x[k], fdop[sel]/scale, sspec[row0+r, sel])   (exact NumPy
 *   branch structure and rounding: searchsorted bracket, slope*(x-xp[j])+fp[j], NaN retry);
 *   mask_out[r, k] = (|x[k]| > max|fdop[sel]/scale|) or isnan(norm_out[r, k]);
 *   pow_out[r]     = mean over unmasked finite entries of 10**(v/10), v = norm_out[r, k] or,
 *                    when xlin is given (logsteps), np.interp(xlin[k], ...)  (NaN if none).
 * Columns [cut_lo, cut_hi) read as NaN (cutmid); row_offset[nr] (or NULL) is subtracted from
 * the row first (subtract_artefacts).  fdop must be ascending.  All pointers DEVICE. */
int32_t scint_norm_sspec(const double* sspec, int64_t ld, int64_t nc, const double* fdop,
                         const double* yaxis, int64_t row0, int64_t nr, double eta,
                         double maxnormfac, int64_t cut_lo, int64_t cut_hi,
                         const double* row_offset, const double* x, const double* xlin,
                         int64_t nx, double* norm_out, uint8_t* mask_out, double* pow_out,
                         void* stream);

/* ---- np.ma.average(norm, axis=0, weights=w) (dynspec.py:2171-2181) --------------------------
 * avg_out[k] = sum_r w[r]*norm[r,k] / sum_r w[r] over rows with rowsel[r] != 0 (NULL = all) and
 * mask[r,k] == 0.  A column with no entry gets empty_out[k] = 1 and avg_out[k] = 0 (the value
 * numpy.ma leaves under the mask).  Fixed summation order (deterministic). */
int32_t scint_masked_colavg_workspace_bytes(int64_t nr, int64_t nx, size_t* SCINT_HOST bytes);
int32_t scint_masked_colavg(const double* norm, const uint8_t* mask, int64_t nr, int64_t nx,
                            const double* weights, const uint8_t* rowsel, double* avg_out,
                            uint8_t* empty_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- np.nanmean(sspec[rows, colsel], axis=1) (dynspec.py:2060-2061) ------------------------ */
int32_t scint_row_nanmean(const double* sspec, int64_t ld, int64_t nc, int64_t row0, int64_t nr,
                          const uint8_t* colsel, int64_t cut_lo, int64_t cut_hi, double* out,
                          void* stream);

/* ---- np.std over rows [r0, r1), columns [0, c_lo) + [c_hi, nc) (fit_arc noise, dynspec.py:1097-1101)
 * out: DEVICE double[1]; workspace: 1032 doubles. */
int32_t scint_block_std(const double* a, int64_t ld, int64_t nc, int64_t r0, int64_t r1,
                        int64_t c_lo, int64_t c_hi, double* out, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---- arc fits over a stack of spectra (scintools_amd/csrc/arcbatch.hpp) ----------------------------------------------------
 * scint_arc_profile_batch: for every problem b of sspec[B][R][ld] (dB, nc columns, 1 <= B <= 65535, SCINT_E_ARG otherwise) with
 * shared fdop[nc] (ascending), yaxis[R], delay rows [row0, row0 + nr) (row0 + nr <= R) and x[nx]:
 *   avg_out[b][nx], empty_out[b][nx]  the BITS of scint_norm_sspec(sspec_b, ..., row_offset = NULL, xlin = NULL) followed by
 *                                     scint_masked_colavg(..., weights = 1, rowsel = NULL); the normalised spectrum
 *                                     norm[nr][nx] in between is never written;
 *   noise_out[b]                      the BITS of scint_block_std(sspec_b, ld, nc, R / 2, R, noise_lo, noise_hi): fit_arc's
 *                                     noise before its division by sqrt(2 ind) (its columns are not norm_sspec's cut for an odd
 *                                     cutmid, hence the two pairs).
 * A workgroup owns one problem and 256 columns of x and walks the delay rows, summing in the order of scint_masked_colavg
 * (partials over 32 rows, then the partials in ascending order); a row's selected columns are staged in LDS when there are at most
 * 2048 of them and read from global memory otherwise.  Six launches for any B, no atomics, asynchronous on `stream`.
 * workspace: scint_arc_profile_batch_workspace_bytes(B, R, nc, nr) (a table of nr rows, the noise partials). */
int32_t scint_arc_profile_batch_workspace_bytes(int64_t B, int64_t R, int64_t nc, int64_t nr, size_t* SCINT_HOST bytes);
int32_t scint_arc_profile_batch(const double* sspec, int64_t B, int64_t R, int64_t ld, int64_t nc, const double* fdop,
                                const double* yaxis, int64_t row0, int64_t nr, double eta, double maxnormfac,
                                int64_t cut_lo, int64_t cut_hi, int64_t noise_lo, int64_t noise_hi, const double* x,
                                int64_t nx, double* avg_out, uint8_t* empty_out, double* noise_out, void* workspace,
                                size_t workspace_bytes, void* stream);

/* scint_arc_peak_fit: what Dynspec.fit_arc does with a profile after norm_sspec (dynspec.py:1190-1313), one wavefront per profile,
 * one launch.  avg[P][nx] (the profile kernel's avg_out; nx even, x[nx] ascending with x[nx/2 - 1] < 0 <= x[nx/2], shared),
 * noise[P] (its noise_out; the fit uses noise[p] / noise_div).  PP = P profiles, or 2 P with asymm: 2 p = the side x >= 0
 * ("left"), 2 p + 1 = the side x < 0 flipped ("right").  Per profile:
 *   fold (avg[x >= 0] + flip(avg[x < 0])) / 2 (or one side); drop non-finite entries (a column that empty_out marks carries 0.0
 *   and is kept); flip; eta = etamin / x^2, keep eta < etamax -> profile_out[PP][nx/2], the kept points, NaN after them;
 *   smooth: Savitzky-Golay of order 1, interior points with coef[nsmooth] (DEVICE; scipy.signal.savgol_coeffs(nsmooth, 1)), within
 *   nsmooth/2 of an end the least-squares line over the first / last nsmooth points (scipy's mode='interp'); nsmooth odd, >= 3;
 *   pk = the first index whose smoothed value equals the largest one with constraint[0] < eta < constraint[1] (HOST [2]);
 *   i1, i2 = the reference's walks down to low_power_diff / high_power_diff below the peak, bounded by the profile;
 *   the least-squares parabola through the UNSMOOTHED points [pk - i1, pk + i2) in x 1000 / ptp(x) (log_parabola: in log x,
 *   scaled twice as fit_log_parabola does), solved through an orthogonal basis on the centred abscissa; peak and peak error from
 *   the coefficient covariance as scint_models.fit_parabola / fit_log_parabola; noise_error: etaerr from the noise walk.
 * val_out[4][PP]: eta, etaerr, etaerr2 (both errors divided by sqrt 2, as the attributes are), the noise used.
 * dec_out[5][PP]: pk, i1, i2 (-1 where not reached), the number of points kept, status:
 *   0 ok; 1 fewer than max(nsmooth, 4) points kept; 2 no point inside constraint; 3 the window [pk - i1, pk + i2) leaves the
 *   profile (the reference wraps to negative indices there) or has fewer than 4 points; 4 forward parabola (the reference raises
 *   ValueError); 5 non-finite result.  Every status but 0 leaves NaN in eta, etaerr and etaerr2.
 * workspace: scint_arc_peak_fit_workspace_bytes(P, nx, asymm) (the kept curvatures, PP * nx/2 doubles).  No atomics. */
int32_t scint_arc_peak_fit_workspace_bytes(int64_t P, int64_t nx, int32_t asymm, size_t* SCINT_HOST bytes);
int32_t scint_arc_peak_fit(const double* avg, int64_t P, int64_t nx, const double* noise, double noise_div,
                           const double* x, double etamin, double etamax, const double* SCINT_HOST constraint /*[2]*/,
                           int32_t nsmooth, const double* coef, double low_power_diff, double high_power_diff,
                           int32_t noise_error, int32_t log_parabola, int32_t asymm, double* profile_out, double* val_out,
                           int32_t* dec_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- plain 2-D complex FFT (forward, numpy sign convention) -------------- */
/* Exposed for tests: out may alias in. */
int32_t scint_fft2_workspace_bytes(int64_t rows, int64_t cols, size_t* SCINT_HOST bytes);
int32_t scint_fft2(const scint_c128* in, scint_c128* out, int64_t rows, int64_t cols,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- split-step screen simulator: scint_sim.Simulation (scint_sim.py:23-311, Coles et al. 2010) -------------------
 * x (nx) is the strided axis of every array here, y (ny) the contiguous one.  Sizes: nx a power of two in [16, 2^17]
 * (the column passes of the FFT, at most 65535 butterflies each), ny a power of two in [16, 8192] (the row kernel), nx * ny <= 2^28.
 * scint_sim_screen: w[nx][ny], the weights of get_screen / swdsp from the index alone (the reference's fill order, its
 *   off-by-one on the ky = 0 line and the entries it leaves at zero included), and xyp = real(fft2(w (z1 + i z2))) for
 *   the two normal draws z1, z2[nx][ny].  a, b, c: the anisotropy coefficients of swdsp; con = sqrt(consp);
 *   alf = -(alpha + 2) / 4; inner2 = inner^2.
 * scint_sim_field: spe[:, f0:f1] (complex64 [nx][nf]) and spi = |spe|^2 (float32 [nx][nf], rounded as the reference's
 *   complex64 product) of E_f = ifft2(frfilt3(fft2(exp(i xyp scale[f])))), column ny/2, for the frequencies f0 <= f < f1;
 *   scale[nf] is a DEVICE array.  The frequencies go in groups of as many as the workspace holds
 *   (scint_sim_field_workspace_bytes(nx, ny, group)); the result does not depend on the grouping while a group's planes
 *   (16 nx ny bytes per frequency) stay below the 300 MiB at which the column transform changes from radix passes to its
 *   tiled form -- a larger group agrees to rounding, not bit for bit.  With xyi != NULL
 *   and f1 == nf the intensity |E|^2 [nx][ny] of the last frequency is written too.  Only column ny/2 of every inverse
 *   transform is computed (a row reduction and one 1-D inverse transform per frequency); SCINT_SIM_COLUMN=0
 *   (environment, read per call) takes the full inverse 2-D transform of every frequency and picks the column.
 * scint_sim_last_route: of the LAST scint_sim_field of the process -- column = 1 if it took the shortcut, groups = the
 *   groups it ran (tests).
 * scint_sim_pulse: get_pulse's pulsewin before its transpose, out[nx][2 nf] = roll(|fft(spe * window, 2 nf)|^2, nf)
 *   (the roll of the flattened array, as np.roll without an axis); 2 nf a power of two in [16, 8192]. */
int32_t scint_sim_screen_workspace_bytes(int64_t nx, int64_t ny, size_t* SCINT_HOST bytes);
int32_t scint_sim_screen(const double* z1, const double* z2, int64_t nx, int64_t ny, double dqx, double dqy,
                         double a, double b, double c, double con, double alf, double inner2, double* w,
                         double* xyp, void* workspace, size_t workspace_bytes, void* stream);
int32_t scint_sim_field_workspace_bytes(int64_t nx, int64_t ny, int64_t group, size_t* SCINT_HOST bytes);
int32_t scint_sim_field(const double* xyp, int64_t nx, int64_t ny, const double* scale, int64_t nf, int64_t f0,
                        int64_t f1, double ffconx, double ffcony, void* spe, float* spi, double* xyi,
                        void* workspace, size_t workspace_bytes, void* stream);
int32_t scint_sim_last_route(int32_t* SCINT_HOST column, int64_t* SCINT_HOST groups);
int32_t scint_sim_pulse(const void* spe, int64_t nx, int64_t nf, const double* window, double* out, void* stream);

/* ---- theoretical 2-D ACF model: scint_sim.ACF (scint_sim.py:417-766; Rickett et al. 2014, Appendix A) ---------------------
 * The strong-scintillation intensity ACF behind scint_models.scint_acf_model_2d.  For every frequency lag dnun[idn], idn >= 1,
 * and every time-lag sample s the reference sums gammes[y][x] exp(i ((X - sx)^2 + (Y - sy)^2) / (2 dnun[idn])) over a square
 * grid; here the phase is factorised into exp(i (X - sx)^2 / (2 nu)) exp(i (Y - sy)^2 / (2 nu)) and the sum over x becomes a
 * real x complex float64 matrix product on the matrix cores (csrc/acf.hpp).  Grid lengths are DATA: the host builds the axes
 * with NumPy (np.arange with a float step) and passes their lengths.
 * scint_acf_model: inputs (device) snp[m] the coarse grid, snp2[m2] the core grid (lag 1 only), snx[nsn], sny[nsn] the time-lag
 *   samples in the screen's coordinates, dnun[ndnun] the frequency lags (dnun[0] = 0 is not read); sigxn, sigyn the phase
 *   gradient (the centres of lag idn are snx - 2 sigxn dnun[idn], sny - 2 sigyn dnun[idn]); sqrtar = sqrt(ar), alph2 = alpha / 2;
 *   step = dsp / res_fac the coarse grid's step, step2 = dsp / core_fac the core grid's.
 *   Outputs (device): gammes[m][m] = exp(-0.5 ((x / sqrtar)^2 + (y sqrtar)^2)^alph2), x = snp[column], y = snp[row] (the
 *   reference's acf_efield), and the complex field gamma[nsn][ndnun], columns 1 .. ndnun - 1:
 *   gamma[s][idn] = -i step^2 / (2 pi dnun[idn]) sum_yx G exp(i ...) with the core grid for idn = 1.  Column 0 (dnun = 0) is NOT
 *   written: it is the e-field ACF at the samples, which the host computes.  Any m, m2, nsn >= 1 and ndnun >= 2 (m, m2 <= 2^24,
 *   nsn <= 64 * 65535, ndnun <= 65536).  Five launches (four when ndnun == 2); no atomics: results are bit-reproducible.
 *   Asynchronous on `stream`.  Workspace: scint_acf_model_workspace_bytes(m, m2, nsn, ndnun) -- the phase tables
 *   (32 nsnp (m2 + (ndnun - 2) m) bytes, nsnp = nsn rounded up to 16) and one partial per (lag, block of 64 rows, s). */
int32_t scint_acf_model_workspace_bytes(int64_t m, int64_t m2, int64_t nsn, int64_t ndnun, size_t* SCINT_HOST bytes);
int32_t scint_acf_model(const double* snp, int64_t m, const double* snp2, int64_t m2, const double* snx,
                        const double* sny, int64_t nsn, const double* dnun, int64_t ndnun, double sigxn, double sigyn,
                        double sqrtar, double alph2, double step, double step2, double* gammes, scint_c128* gamma,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- thin-screen curvature search: two_curve_map + singularvalue_calc (ththmod.py:496-513, 1557-1636) ----------------
 * The 'thin' fitting procedure of Dynspec.prep_thetatheta (dynspec.py:1480-1516) models only the region near the arclet apexes:
 * a RECTANGULAR theta-theta map thth[theta2, theta1] (rows: the arclet centres th2[M2], columns: the main-arc centres th1[M1],
 * both (edges[1:] + edges[:-1]) / 2 with no re-centring), cropped to |centre| < sqrt(tau.max() / eta) on each axis, with the
 * reduced columns |centre| < centerCut set to zero, and its largest singular value in place of np.linalg.svd(thth_red)[1][0].
 * ranges (HOST, 6 int32 per map): r0, n2 = the kept theta2 centres [r0, r0 + n2); c0, n1 = the kept theta1 centres
 * [c0, c0 + n1); cut0, cut1 = the reduced columns [cut0, cut1) that are zeroed.  The host computes them with the reference's
 * own masks (each must be one run of centres: edges from np.linspace).  check != 0: the grid may reach fd_inv < -nfd, where
 * NumPy's fancy index raises IndexError (the wrap of -nfd <= fd_inv < 0 is reproduced); the whole M2 x M1 grid is then tested.
 *
 * scint_two_curve_map: thth_out[n2][n1] (every element written); *raise_out (device int32) = 1 if NumPy would raise.
 *   Synchronous.  Workspace: scint_two_curve_map_workspace_bytes() (the job table).
 * scint_sv_sweep_multi: sigma_1 of every map of a fit_thetatheta -- the per-chunk loops of single_search_thin (ththmod.py:
 *   588-643) over every (chunk, eta) pair in one call, as scint_eval_sweep_multi does for 'standard'.  Map e is built from
 *   cs_stack + cs_index[e] * cs_stride with geoms[cs_index[e]], th1_stack[cs_index[e]][M1], th2_stack[cs_index[e]][M2], the
 *   curvatures etas1[e] (main arc) and etas2[e] (arclets), ranges[e][6] and check[e].  sigma_1 = sqrt(lambda_max(A^H A)) by
 *   float64 Lanczos with the Ritz-residual rule of the eigenvalue sweeps (residual <= tol lambda, on A^H A), from the conjugated
 *   middle row (the constant vector if that row is zero); a map whose Krylov space is complete first is exact (a single column:
 *   its 2-norm; the all-zero map: 0).  A is read from HBM once per Lanczos step (eigen.hip, sv_matvec_kernel).  The maps are
 *   built and resident `batch` at a time (each slab holds an M2 x M1 map).  Results are bit-reproducible and do not depend on
 *   `batch` or on which maps share a call.  Mixed precision (scint_sweep_precision) does not apply: always float64.
 *   Outputs (device): sv_out[neta] (NaN unless status 0), status_out[neta]: 0, SCINT_E_NOCONV, SCINT_E_EMPTY (no kept row or
 *   column), SCINT_E_NONFINITE, or SCINT_E_ARG = NumPy would raise IndexError in two_curve_map; iters_out[neta] Lanczos steps.
 *   At most 16384 theta1 centres.  Synchronous.  Workspace: scint_sv_sweep_multi_workspace_bytes(). */
int32_t scint_two_curve_map_workspace_bytes(size_t* SCINT_HOST bytes);
int32_t scint_two_curve_map(const scint_c128* cs, const scint_thin_geom* SCINT_HOST geom,
                            const double* th1, int64_t M1, const double* th2, int64_t M2,
                            double eta1, double eta2, const int32_t* SCINT_HOST ranges /*[6]*/, int32_t check,
                            scint_c128* thth_out, int32_t* raise_out, void* workspace, size_t workspace_bytes,
                            void* stream);
int32_t scint_sv_sweep_multi_workspace_bytes(int64_t M1, int64_t M2, int64_t neta, int64_t batch, int32_t max_iter,
                                             int64_t ncs, size_t* SCINT_HOST bytes);
int32_t scint_sv_sweep_multi(const scint_c128* cs_stack, int64_t ncs, int64_t cs_stride,
                             const int32_t* SCINT_HOST cs_index, const scint_thin_geom* SCINT_HOST geoms,
                             const double* th1_stack, int64_t M1, const double* th2_stack, int64_t M2,
                             const int32_t* SCINT_HOST ranges /*[neta][6]*/, const int32_t* SCINT_HOST check,
                             const double* SCINT_HOST etas1, const double* SCINT_HOST etas2, int64_t neta,
                             double tol, int32_t max_iter, int64_t batch,
                             double* sv_out, int32_t* status_out, int32_t* iters_out,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Scattered image: Dynspec.calc_scattered_image (dynspec.py:3553-3570) -- scipy's RectBivariateSpline(tdel, fdop, 10**(sspec/10))
 * (kx = ky = 3, s = 0: the tensor-product not-a-knot interpolating cubic spline), evaluated at ((fx[j]^2 + fy[i]^2) eta, fx[j]) with
 * both arguments clamped to the knots, times fy[i], mirrored into image[nx][nx] (nx = 2 sampling + 1, ny = sampling + 1 rows computed).
 * sspec_db: the dB spectrum with leading dimension ld; the crop is rows [row0, row1) x columns [col0, col1), at least 4 x 4.
 * Everything the host decides is data: tdel[nrow] the cropped row knots (strictly increasing, any spacing);
 *   row_sys[4][ncol] = 1/h, 6/pivot, -sub/pivot, sup of the column-axis (Doppler) not-a-knot system in second-derivative form and
 *   row_end[4] (HOST) its end rule M[0] = e0 M[1] + e1 M[2], M[n-1] = e2 M[n-2] + e3 M[n-3]; row_warm the warm-up length of a row
 *   chunk (rows of more than 2050 knots are solved in chunks; 1..256, unused for shorter rows); row_idx[nx], row_coef[nx][4] the
 *   interval and the weights of y[k], y[k+1], M[k], M[k+1] of the clamped abscissa fx[j] on the Doppler knots;
 *   col_sys[4][nrow] = h, sub, 1/pivot, sup of the delay-axis system, col_end[4] (HOST), col_block_rows / col_warm its blocking as in
 *   scint_spline_resample (0, 0: one sequential sweep); fx[nx], fy[ny] the image axes (not clamped).
 * Outputs (device): image[nx][nx]; *nonfinite = 1 if some 10**(v/10) of the crop is NaN or inf (scipy then returns NaN everywhere),
 *   else 0.  No atomics: equal inputs give equal bits.  Asynchronous on `stream`.
 * Workspace: scint_scattered_image_workspace_bytes(nrow, sampling): three nrow x nx planes. */
int32_t scint_scattered_image_workspace_bytes(int64_t nrow, int64_t sampling, size_t* SCINT_HOST bytes);
int32_t scint_scattered_image(const double* sspec_db, int64_t ld, int64_t row0, int64_t row1, int64_t col0, int64_t col1,
                              const double* tdel, const double* row_sys, const double* SCINT_HOST row_end /*[4]*/, int64_t row_warm,
                              const int32_t* row_idx, const double* row_coef, const double* col_sys,
                              const double* SCINT_HOST col_end /*[4]*/, int64_t col_block_rows, int64_t col_warm,
                              const double* fx, const double* fy, double eta, int64_t sampling, double* image,
                              int32_t* nonfinite, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Dynamic-spectrum cleaning: Dynspec.zap, refill, correct_dyn (dynspec.py:3856-3870, 3273-3323, 3325-3410) and
 * ththmod.svd_model (ththmod.py:18-35).  Arrays are row-major float64 [nf][nt] without padding, on the device.
 *
 * scint_zap: in place.  median = np.median of the non-NaN elements (radix select on the order-preserving 64-bit key; an even
 *   count gives (a + b) / 2 of the two middle elements; +-inf take part), mdev = the same of |x - median|; an element becomes
 *   NaN where |x - median| / mdev > sigma.  Bit-exact: integer counting only.  stats (device, may be NULL) = {median, mdev}.
 *   No non-NaN element: both NaN, nothing changes.  Asynchronous.  Workspace: scint_zap_workspace_bytes().
 * scint_refill_median: out = in with every NaN replaced by the median of its kf x kt window (both odd, kf kt <= 225) of
 *   `in with NaN -> fill`, zero padding beyond the edges (scipy.signal.medfilt); other elements are copied.  out != in.
 * scint_refill_linear: in place.  line_valid[nf] (axis 0) or [nt] (axis 1), 1 = the line holds data: every element of a line
 *   flagged 0 becomes slope * (i - i0) + v0, slope = (v1 - v0) / (i1 - i0), between the nearest valid lines i0 < i < i1 on
 *   either side (np.interp's arithmetic, not contracted); without a valid line on one side it is left as it is.
 * scint_svd_model: model = sum over the top p singular triplets of a = (a V) V^T with V [nt][p] the dominant right singular
 *   subspace, by block iteration on a^T a from the orthonormal start v0[p][nt] (a zero row is a deflated column);
 *   corrected = a / |model|.  Either output may be NULL.  1 <= p <= 8.  Stops when |a^T a V - V H|_F <= tol lambda_p, H = V^T a^T a V,
 *   lambda_p its smallest eigenvalue among the columns not deflated (checked every fourth step); SCINT_E_NOCONV after max_iter
 *   steps, SCINT_E_NONFINITE for a NaN or inf element.  status_out (device, may be NULL): 4 + 8 doubles {residual, lambda_p,
 *   lambda_1, active columns, the eigenvalues of H descending}; *iters_out (HOST, may be NULL).  No atomics.  Synchronous.
 *   Workspace: scint_svd_model_workspace_bytes(nf, nt).
 * scint_nanmean_axis: np.nanmean(a, axis): axis 1 -> out[nf], axis 0 -> out[nt] (needs the workspace of
 *   scint_nanmean_axis_workspace_bytes; fixed summation order, not NumPy's).  A line without data gives NaN.
 * scint_divide_axis: in place, a[i][j] /= v[i] (axis 0) or v[j] (axis 1).  Both asynchronous. */
int32_t scint_zap_workspace_bytes(size_t* SCINT_HOST bytes);
int32_t scint_zap(double* dyn, int64_t n, double sigma, double* stats, void* workspace, size_t workspace_bytes, void* stream);
int32_t scint_refill_median(const double* in, int64_t nf, int64_t nt, int64_t kf, int64_t kt, double fill, double* out,
                            void* stream);
int32_t scint_refill_linear(double* dyn, int64_t nf, int64_t nt, int32_t axis, const uint8_t* line_valid, void* stream);
int32_t scint_svd_model_workspace_bytes(int64_t nf, int64_t nt, size_t* SCINT_HOST bytes);
int32_t scint_svd_model(const double* a, int64_t nf, int64_t nt, int32_t p, const double* v0, double tol, int32_t max_iter,
                        double* model, double* corrected, double* status_out, int32_t* SCINT_HOST iters_out,
                        void* workspace, size_t workspace_bytes, void* stream);
int32_t scint_nanmean_axis_workspace_bytes(int64_t nf, int64_t nt, size_t* SCINT_HOST bytes);
int32_t scint_nanmean_axis(const double* a, int64_t nf, int64_t nt, int32_t axis, double* out, void* workspace,
                           size_t workspace_bytes, void* stream);
int32_t scint_divide_axis(double* a, int64_t nf, int64_t nt, int32_t axis, const double* v, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Biharmonic inpainting of flagged pixels: the method of Dynspec.refill(method='biharmonic') (dynspec.py:3301-3307, scikit-image's
 * inpaint_biharmonic with split_into_regions=False); kernels in csrc/inpaint.hpp, DESIGN.md 4r.
 *
 * scint_inpaint_biharmonic: in place on dyn[nf][nt] (float64, device).  mask[nf][nt] (device, uint8): non-zero = the pixel is
 *   unknown; nmask = the number of such pixels (the caller counts them: it sizes the workspace; SCINT_E_ARG if the device counts
 *   another number).  With L the 5-point Laplacian with reflecting edges (scipy.ndimage.laplace, mode='reflect'), m the masked
 *   and k the other pixels, the masked pixels become the solution of (L^2)_mm u_m = -(L^2)_mk u_k; every other pixel keeps its
 *   bits, and the values of dyn under the mask are never read (they may be NaN).  stencils[25][5][5] (device): for the class
 *   5 cf + ct of a pixel (cf, ct = 0, 1: that far from the first channel / sub-integration, 2: interior, 3, 4: one and zero
 *   from the last) the coefficients of L^2 at the offsets (-2..2, -2..2) around it, zero beyond the edge.
 *   Solver: conjugate gradients from zero, every scalar on the device, every sum in one fixed order and no atomics: equal inputs
 *   give equal bits.  It stops when |r|_2 <= tol |b|_2 for the TRUE residual r = b - A u: the recurrence's residual is tested
 *   every step on the device (the host looks every 8 steps), the true one is formed when that test passes, and the iteration goes
 *   on from it if it fails.  0 < tol < 1.  SCINT_E_NOCONV after max_iter steps (dyn is then left as it was), SCINT_E_NONFINITE
 *   if a known pixel within two pixels of a masked one is NaN or inf.  *residual_out (HOST, may be NULL) = the true relative
 *   residual |b - A u|_2 / |b|_2, *iters_out (HOST, may be NULL) = the steps taken; both are set on SCINT_E_NOCONV too.
 *   nmask = 0 returns at once.  Limits: nf, nt >= 5 (the 25 classes are distinct), nf nt < 2^31, nmask < nf nt.  Synchronous.
 *   Workspace: scint_inpaint_biharmonic_workspace_bytes(nf, nt, nmask): 4 nf nt + 52 nmask bytes and 25 KB. */
int32_t scint_inpaint_biharmonic_workspace_bytes(int64_t nf, int64_t nt, int64_t nmask, size_t* SCINT_HOST bytes);
int32_t scint_inpaint_biharmonic(double* dyn, int64_t nf, int64_t nt, const uint8_t* mask, int64_t nmask, const double* stencils,
                                 double tol, int32_t max_iter, double* SCINT_HOST residual_out, int32_t* SCINT_HOST iters_out,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* scint_inpaint_biharmonic_lines: the same system, arguments and results as scint_inpaint_biharmonic, solved by PRECONDITIONED
 *   conjugate gradients.  nchan / nsub = the numbers of channels / sub-integrations whose every pixel is masked (the
 *   caller counts them: they size the workspace; SCINT_E_ARG if the device finds other numbers).  The preconditioner inverts
 *   exactly the block of the matrix on the whole channels (a DCT along time, then one symmetric positive definite pentadiagonal
 *   system per time mode, L D L^T factors formed once per call) and the block on the whole sub-integrations (axes exchanged), and
 *   divides by the diagonal on the masked pixels in no whole line.  The start is x0 = M^-1 b: for a mask of whole channels only, or
 *   of whole sub-integrations only, the true residual passes there and *iters_out = 0.  Stopping rule, determinism (no atomics,
 *   equal inputs give equal bits), errors and the untouched dyn on SCINT_E_NOCONV as above.  A mask without a whole line is
 *   accepted and gains nothing.  Limits: as above, and an axis that is transformed (time if nchan > 0, frequency if nsub > 0) must
 *   hold 5 .. 4096 points, or 8192 (SCINT_E_ARG otherwise).  Synchronous.
 *   Workspace: scint_inpaint_biharmonic_lines_workspace_bytes(nf, nt, nmask, nchan, nsub): 4 nf nt + 60 nmask bytes and 35 KB, plus
 *   per set of L whole lines of n points 40 L n bytes, and 16 (L + 1) m + 32 n more when n is not a power of two from 16 (m = the
 *   power of two >= 2 n - 1). */
int32_t scint_inpaint_biharmonic_lines_workspace_bytes(int64_t nf, int64_t nt, int64_t nmask, int64_t nchan, int64_t nsub,
                                                       size_t* SCINT_HOST bytes);
int32_t scint_inpaint_biharmonic_lines(double* dyn, int64_t nf, int64_t nt, const uint8_t* mask, int64_t nmask, int64_t nchan,
                                       int64_t nsub, const double* stencils, double tol, int32_t max_iter,
                                       double* SCINT_HOST residual_out, int32_t* SCINT_HOST iters_out, void* workspace,
                                       size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Scaled-time (NuT) conjugate spectrum: scint_utils.slow_FT (scint_utils.py:655-703).  dyn[nt][nf] is [time][frequency], row-major
 * float64 on the device; fscale[nf] = freqs / fref (device; formed by the caller as the reference does, lines 683-686).
 *   S1[k][j] = sum_t dyn[t][j] exp(-2 pi i (t fscale[j]) ft[k]),  ft = np.fft.fftfreq(nt, 1)              (lines 688-694)
 *   out = fftshift(fft(fftshift(S1, axes=0), axis=1), axes=1)                                             (lines 695-700)
 * (line 695 as the reference means it: it spells the keyword `axis`, which NumPy rejects).  out[nt][nf] complex128.
 * The [nt][nt][nf] array of the reference is never formed: per (k, j) the exponentials are the product of two tables of 64 and
 * nt / 64 entries, each entry from its own float64 phase reduced modulo one cycle (no recurrence).  The frequency transform is the
 * row FFT when nf is a power of two in [16, 8192] and a direct sum with exactly reduced twiddle indices otherwise (nt nf^2 terms).
 * Non-finite input propagates as in NumPy (one NaN pixel makes every output NaN); there is no input scan.  No atomics: equal
 * inputs give equal bits.  Asynchronous on `stream`.
 * Limits: 1 <= nt, nf <= 2^20 and ceil(nt / 64) * 64 * nf <= 2^30 (SCINT_E_ARG otherwise): every index is formed in 64 bits,
 *   the launch grids stay below 65536 in y, and the integer k t of a phase stays exact in float64.
 * Workspace: scint_slow_ft_workspace_bytes(nt, nf): the zero-padded transpose of dyn and S1, about 24 nt nf bytes. */
int32_t scint_slow_ft_workspace_bytes(int64_t nt, int64_t nf, size_t* SCINT_HOST bytes);
int32_t scint_slow_ft(const double* dyn /*[nt][nf]*/, int64_t nt, int64_t nf, const double* fscale /*[nf] device*/,
                      scint_c128* out /*[nt][nf]*/, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The velocity and trapezoid rescalings of Dynspec.scale_dyn (dynspec.py:3961-4128); kernels in csrc/scale.hpp, DESIGN.md 4n.
 *
 * scint_spline_resample_rows: every ROW of dyn[nf, nt] is interpolated with the not-a-knot cubic spline (scipy
 *   interp1d(kind='cubic')) from the knots x[nt] (ascending, any spacing, shared by all rows) to nout targets: out[nf, nout],
 *   out[r, j] = S_r(target j), not flipped.  The mathematics and the arguments are scint_spline_resample's, with the time axis in
 *   the place of the frequency axis: h[nt-1], sub/inv/sup[nt] the Thomas factors (DEVICE), end[4] the not-a-knot ends (HOST),
 *   idx[nout] the interval of every target and coef[nout][4] its weights; idx must be NON-DECREASING (targets ascending), because
 *   a block of knots evaluates the contiguous range of targets that falls into it.
 *   A workgroup takes up to 64 rows and one block of `block` interior knots, started `warm` knots early from zero on either side
 *   (block <= 0 or >= nt-2: one block, the plain sequential sweep of every row; `warm` is then ignored); it stages its tile in
 *   LDS, solves there and evaluates its targets from LDS, so the moments never reach memory and no workspace is used.  Only when
 *   ONE block is asked for and min(block + 2 warm + 4, nt) exceeds 7679 knots the rows are swept through a workspace of nf*nt
 *   doubles (scint_spline_resample_rows_workspace_bytes says which: 256 bytes, which may be NULL, or nf*nt*8).
 *   A non-finite pixel spreads over what one sweep covers: its whole row with one block, its neighbourhood otherwise (the caller
 *   tests the mean and asks for one block).  float64, no atomics, equal inputs give equal bits.  Asynchronous on `stream`.
 *   Limits: 1 <= nf <= 65535, 4 <= nt < 2^31, 1 <= nout < 2^31.
 *
 * scint_trap_scale: out[nf, nt] of scale_dyn(scale='trapezoid').  v[f][t] = ((dyn[f][t] - mean) * cw[t]) * sw[f] in that order
 *   (cw == sw == NULL: v = dyn - mean; `mean` is the caller's np.mean of the host array); row f keeps nkeep[f] samples (DEVICE
 *   int32, clamped to [0, nt]): out[f][j] = np.interp(np.linspace(times[0], times[nt-1], nkeep[f])[j], times, v[f]) for
 *   j < nkeep[f] and +0.0 after.  times[nt] ascending, any spacing.  np.linspace and np.interp are reproduced operation by
 *   operation (step = (stop - start)/(n - 1), j*step + start, the last sample set to stop; the bracket j with times[j] <= x,
 *   slope*(x - times[j]) + v[j] without contraction and NumPy's NaN retries), so the result equals NumPy's bit for bit.
 *   Limits: 1 <= nf <= 65535, nt >= 1.  Asynchronous on `stream`. */
int32_t scint_spline_resample_rows_workspace_bytes(int64_t nf, int64_t nt, int64_t block, int64_t warm, size_t* SCINT_HOST bytes);
int32_t scint_spline_resample_rows(const double* dyn, int64_t nf, int64_t nt, const double* h, const double* sub,
                                   const double* inv, const double* sup, const double* SCINT_HOST end /*[4]*/,
                                   int64_t block, int64_t warm, const int32_t* idx, const double* coef, int64_t nout,
                                   double* out, void* workspace, size_t workspace_bytes, void* stream);
int32_t scint_trap_scale(const double* dyn, int64_t nf, int64_t nt, double mean, const double* cw, const double* sw,
                         const double* times, const int32_t* nkeep, double* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The any-length 2-D transform and the brightness-distribution model scint_sim.Brightness (scint_sim.py:768-958, after Yao et al.
 * 2020); kernels in csrc/bright.hpp, DESIGN.md 4o.  All asynchronous on `stream`; no atomics: equal inputs give equal bits.
 *
 * scint_fft2_any: the forward 2-D DFT (NumPy's sign) of in[R][C], 2 <= R, C <= 4096 (SCINT_E_ARG otherwise).  A power-of-two
 *   length the row / column kernels take (rows: 16 .. 8192, columns: >= 2) goes to them; any other length n goes through Bluestein's
 *   chirp-z at the power of two M >= 2 n - 1 (at least 16; so n <= 4096 with the row kernel's 8192): chirp, zero-pad, forward
 *   transform, times the chirp filter's transform (formed once per length and cached beside the twiddle tables), inverse transform,
 *   chirp, crop.  The chirp phase pi k^2 / n comes from k^2 mod 2 n in integers.
 *   real_input: `in` is float64 [R][C] (else complex128).  in_shift / out_shift: 0 none, 1 np.fft.fftshift, 2 np.fft.ifftshift of
 *   the input before / the result after the transform (they differ on odd lengths), folded into the index arithmetic.
 *   out_what: 0 out is complex128 [R][C]; 1 float64 [R][C] = the modulus; 2 float64 [R][C] = the real part.
 *   Non-finite input propagates as in NumPy.  Workspace: scint_fft2_any_workspace_bytes(R, C).
 * scint_bright_efield: rho[n][n] = exp(-0.5 * (a X^2 + b Y^2 + c X Y)**alpha2), X = x[column], Y = x[row] (calc_brightness,
 *   :855-857); a, b, c are the host's (the kernel does not divide by 1 - R^2).
 * scint_bright_map: per pixel (itd, ifd) of the [ntd][nfd] spectrum the loop body of calc_SS (:911-925) and
 *   ss0 = B(thetax, thetay) * amp + B(thetax, -thetay) * amp (:933-938), jacobian = amp; thetax / thetay are written when not NULL.
 *   B(.,.) is scipy's griddata(method='linear') of B[n][n] on the grid x[n] x x[n] (ascending): piecewise linear on the two
 *   triangles of a cell, NaN outside the grid.  diagonals: bit iy (n - 1) + ix (bit b of byte b / 8 is (byte >> (b % 8)) & 1) says
 *   that the cell with corners (ix, iy) .. (ix + 1, iy + 1) is split along the diagonal through those two corners, 0 along the
 *   other; NULL = 1 everywhere.  par (HOST [9]): thetagx, thetagy, thetarx, thetarx**2, thetary**2, 0.5 * df, 2 / df, 10**(-6) and
 *   (n - 1) / (x[n-1] - x[0]).
 * scint_bright_fold: ss = ss0 with ss[1:, 1:] += flip(flip(ss0[1:, 1:])), lss = 10 log10(ss) (:947-950); ss must not be ss0.
 * scint_divide_by_max: x /= np.max(x) in place (calc_acf, :956): NaN if any element is NaN.  Two fixed-order stages.
 *   Workspace: scint_divide_by_max_workspace_bytes(). */
int32_t scint_fft2_any_workspace_bytes(int64_t R, int64_t C, size_t* SCINT_HOST bytes);
int32_t scint_fft2_any(const void* in, int32_t real_input, int64_t R, int64_t C, int32_t in_shift, int32_t out_shift,
                       int32_t out_what, void* out, void* workspace, size_t workspace_bytes, void* stream);
int32_t scint_bright_efield(const double* x, int64_t n, double a, double b, double c, double alpha2, double* rho, void* stream);
int32_t scint_bright_map(const double* B, const double* x, int64_t n, const uint8_t* diagonals, const double* fd, int64_t nfd,
                         const double* td, int64_t ntd, const double* SCINT_HOST par /*[9]*/, double* ss0, double* jacobian,
                         double* thetax, double* thetay, void* stream);
int32_t scint_bright_fold(const double* ss0, int64_t ntd, int64_t nfd, double* ss, double* lss, void* stream);
int32_t scint_divide_by_max_workspace_bytes(size_t* SCINT_HOST bytes);
int32_t scint_divide_by_max(double* x, int64_t n, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCINT_HIP_H */
