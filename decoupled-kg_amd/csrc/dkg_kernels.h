// Kernel argument blocks and launch helpers shared by the kernels TU and the C ABI TU.
#pragma once

#include "dkg_common.h"

namespace dkg {

// Line records: the posterior means mu_D and a candidate's covariance row are
// kept [N][cov_rec(m)] (all outputs of a line side by side, zero-padded to a
// power of two), in global memory and staged as is, so a lane reads two
// outputs of a line with one 16-byte ds_read_b128 (256 B/clk) instead of
// per-output 8-byte reads the compiler pairs into ds_read2st64_b64 (128 B/clk).
__host__ __device__ constexpr int cov_rec(int m) { return m <= 1 ? 1 : m <= 2 ? 2 : m <= 4 ? 4 : 8; }

// Groups of 8 scalarisation pairs: the envelope stage's fixed summation order (envelope_body).
__host__ __device__ constexpr int pair_groups(int S) { return (S + 7) >> 3; }
// Plan::dup: no discretisation point coincides with the candidate.
constexpr int DUP_NONE = 0x7fffffff;

// Stage ablations (empty cross / covariance / envelope launches selected by
// DKG_DEBUG_COV_FLAGS 2 / 1 and DKG_DEBUG_ENV_FLAGS 2; cross_big_kernel's means alone / Q_X blocks alone by
// DKG_DEBUG_COV_FLAGS 16 / 32) exist only in builds
// with -DDKG_ABLATIONS=1: the check is a dependent scalar load at kernel entry.
#ifndef DKG_ABLATIONS
#define DKG_ABLATIONS 0
#endif

// Everything a forward needs besides the candidates, resident in device memory
// (written once per (model, discretisation, weights) by dkg_plan_init): the
// kernels take a pointer to it, so each launch carries ~40 bytes of arguments
// instead of a ~1 KiB by-value block (measured ~1.5 us of launch cost).
// Large n: K(x, X) is filled once per forward by its own kernel (cross_kfill_kernel) and the cross
// workgroups load their slab of it.  Every column-pair group of a row tile otherwise evaluates the
// kernel over the columns its wider tile needs: at n = 1024 (64 tiles, 32 groups) each entry ~24 times,
// which took most of the stage.  At the headline's n = 256 the extra launch costs more than it saves
// (profiles/r02/r02zz).
__host__ __device__ inline bool cross_kfill(int np) { return np >= 512; }
// Launches over many candidates (a launch of several forward batches, dkg_plan_forward_batches) fill K(x, X)
// once with the separate kernel at any n: the fill replicated over the column-pair groups of a row tile (~4.5x
// at n = 256) is then work the whole device waits on, not latency one forward hides.  Same bits either way.
// fp64 plans at n_pad <= 256 take cross_tall_kernel there instead (dkg_stages.h: K(x, X) once per row tile, in LDS);
// the fill by candidate count remains for fp32 plans (Plan::kx32).
#ifndef DKG_KFILL_MIN_B
#define DKG_KFILL_MIN_B 512
#endif
constexpr int KFILL_MIN_B = DKG_KFILL_MIN_B;
__host__ __device__ inline bool cross_kfill_launch(int np, int B) {
  return np >= 512 || B >= KFILL_MIN_B;
}

// Register slots per lane for a staged (non-streaming) line set of `lines`
// lines: the envelope_kernel instantiation launch_env_bucket picks.
__host__ __device__ inline int env_slots(int lines) {
  return lines <= 64 * 2 ? 2 : lines <= 64 * 8 ? 8 : lines <= 64 * 17 ? 17 : 33;
}

struct Plan {
  dkg_output o[DKG_MAX_OUTPUTS];
  int32_t m, d, N, S, target;       // target < 0: all outputs observed
  int32_t max_B, max_np;            // workspace sized for max_B candidates; max n_pad over outputs
  int32_t sw, split;                // envelope geometry: waves per workgroup, workgroups per candidate
  int32_t debug_env, debug_cov;     // test / ablation switches (0 in production)
  int32_t debug_stamp;              // 1: per-workgroup phase stamps into g_kstamps (0 in production)
  int32_t grad;                     // workspace holds the gradient buffers (DKG_PLAN_GRAD)
  int32_t bpad;                     // pad16(max_B): rows of the fragment-packed candidate buffers
  int32_t stream;                   // envelope streams the lines from global memory (large N)
  int32_t f32;                      // DKG_PLAN_F32: fp32 contractions (q32 / root32 / disc32)
  const double* disc;               // [N x d]
  const double* weights;            // [S x m]
  double* q[DKG_MAX_OUTPUTS];       // fragment-packed K(x, X) R per output (workspace)
  double* kx[DKG_MAX_OUTPUTS];      // large n (cross_kfill): K(x, X) per output in the cross stage's B-operand
                                    // order [B_pad / 16][n_pad / 4][64], filled once per forward (else null)
  double* mux[DKG_MAX_OUTPUTS];     // posterior mean at the candidates per output (workspace)
  double* var[DKG_MAX_OUTPUTS];     // noiseless posterior variance s - |Q_X[b]|^2 per output (workspace)
  double* jq[DKG_MAX_OUTPUTS];      // GRAD: J_g = dK(x,X)/dx_g R, row-major [d][bpad][n_pad] per output
  double* qxrm[DKG_MAX_OUTPUTS];    // GRAD: Q_X = K(x,X) R row-major [bpad][n_pad] per output
  double* qdrm[DKG_MAX_OUTPUTS];    // GRAD: Q_D = K(D,X) R row-major [N][n_pad] per output (written at plan init)
  double* gmu[DKG_MAX_OUTPUTS];     // GRAD: [d][bpad] model-space mean gradients
  unsigned long long* kstamps;      // debug_stamp: [3][KST_WG][8] phase stamps (device)
  double* mux_all;                  // [m][bpad]  = mux[0..m)
  double* var_all;                  // [m][bpad]  = var[0..m)
  double* cov_all;                  // [max_B][N][cov_rec(m)] posterior covariance rows, line records (workspace)
  double* mu_all;                   // [N][cov_rec(m)] the outputs' disc_mean, line records
  int64_t cov_stride;               // N * cov_rec(m): doubles per candidate in cov_all
  double* wg_part;                  // [B][S + ng] pair values, then group terms (ng = ceil(S / 8); split > 1 only)
  int* tickets;                     // [B][ng + 1] group and candidate arrival counters (zeroed by the cross stage)
  // [B]: the lowest record k with z_k == x_b exactly (DUP_NONE: none), from the covariance stage (r^2 = 0).
  // The reference's joint posterior over [x_b; D] makes line 0 and line k + 1 exact copies there (same rows
  // of one covariance matrix), and the walk then takes line 0 (lowest index) while torch.max splits the
  // gradient of max a between them; the envelope builds line 0 from record k so it is the same copy.
  int* dup;
  double* wg_gpart;                 // GRAD: [B][S + ng][d] as wg_part, for dKG/dx (split > 1 only)
  float* q32[DKG_MAX_OUTPUTS];      // F32: quad-packed K(x, X) R per output (workspace)
  float* root32[DKG_MAX_OUTPUTS];   // F32: quad-packed R^T (fp32 copy of root_frag, plan init)
  float* disc32[DKG_MAX_OUTPUTS];   // F32: quad-packed Q_D (fp32 copy of disc_frag, plan init)
  int* hull_pairs;                  // [max_B x S] upper-envelope lines per pair (written with kg_pairs)
  int32_t fused;                    // dkg_plan_forward runs the fused one-launch forward (dkg_fused.h)
  unsigned long long* sync;         // fused hand-off counters: cnt1 [m][rt], cnt2 [nrb], done (zeroed)
  int* sync_err;                    // fused waits that gave up (bits), after the counters
  size_t sync_bytes;                // bytes of the counter block (sync .. sync_err), a multiple of 16
  // Staged forward: the intercepts of lines k >= 1 depend on the weights and mu_D only, not on the
  // candidates -- a_k = a_off + sum_i w_i sd_i mu_i(z_k), discretekg.py:201-213 -- so the plan keeps each
  // scalarisation's largest (itop / itopk; dkg_plan_init, the envelope's own arithmetic: bit-identical lines).
  // icpt is intercepts_kernel's scratch: it writes every a_k there and reads them back to find itop and itopk;
  // no other kernel reads it (the envelope stages mu_D and forms its intercepts itself).
  double* icpt;                     // [S][icpt_stride]: slot k = a_k for 1 <= k <= N, NaN at k = 0 and k > N
  int32_t icpt_stride;              // 64 * env_slots(N + 1): doubles per scalarisation in icpt
  double* itop;                     // [S]: max_{k >= 1} a_k (-inf when N = 0)
  int* itopk;                       // [S][2]: the first k >= 1 attaining it, and how many lines do
  float* kx32[DKG_MAX_OUTPUTS];     // F32 with the K(x, X) fill: kx's entries quad-packed in fp32 (frag32_index),
                                    // the B operand of cross_big32_kernel (kx itself still feeds the fp64 means)
  // Several targets on one plan (dkg_plan_init_targets): the cross and covariance stages do not depend on the
  // target, so one call runs them once and the envelope once per item (tau, b), target tlist[tau]
  // (envelope_targets_kernel; a plan of one target launches envelope_kernel, which knows nothing of items).  The
  // per-candidate result buffers (kg accumulators, wg_part, wg_gpart, tickets, hull_pairs) are carved per item,
  // workspace item tau * bpad + b; the caller's kg / dkg_dx / kg_pairs rows are item tau * B + b.
  // ntgt = 1, tlist[0] = target: the single-target plan.
  int32_t ntgt;
  int32_t tlist[DKG_MAX_OUTPUTS + 1];
  // tlist for the envelope kernel's arguments: 4 bits per target, tlist[tau] + 1 at bits 4 tau (target_of), so
  // a workgroup has its target with the argument load instead of a dependent load through the plan
  unsigned long long tpack;
  // DKG_PLAN_GRAD_GLOBAL_ROWS / DKG_PLAN_FORCE_GLOBAL_ROWS: the (streaming) gradient envelope reads the
  // candidate's q_i / J_i rows from qxrm / jq instead of staging them in LDS (envelope_rows_kernel)
  int32_t grad_rows;
};

__host__ __device__ inline int target_of(unsigned long long tpack, int tau) {
  return (int)((tpack >> (4 * tau)) & 15) - 1;
}
static_assert(DKG_MAX_OUTPUTS + 1 <= 15 && 4 * (DKG_MAX_OUTPUTS + 1) <= 64, "Plan::tpack holds every target in 4 bits");

// By-value arguments of the state-preparation use of the cross stage.
struct CrossArgs {
  dkg_output o;
  int d, rows;
  const double* x;  // [rows x d]
  double* q;        // fragment-packed Q
  double* mean;     // [pad16(rows)] (nullable)
};

hipError_t launch_kernel_matrix(const dkg_output& o, int d, const double* x1, int n1, const double* x2, int n2,
                                double diag_add, double* out, hipStream_t s);
hipError_t launch_pack_root(const double* r, int n, double* rf, hipStream_t s);
// State preparation (dkg_linalg.hip): blocked Cholesky with device status (L in A's lower triangle, the
// inverses of its diagonal blocks in X's), triangular inverse X = L^{-1}, alpha = Linv^T Linv (y - c),
// root_frag from Linv.
hipError_t launch_cholesky(double* A, double* X, int n, int* info, hipStream_t s);
// Several outputs' factorisations side by side: every launch of the blocked chains carries all of them
// (blockIdx.y = output).  A = the matrix (Cholesky: L on return) , X = the inverse (diagonal blocks written
// by the Cholesky, the rest by the inverse).
struct PrepBatch {
  double* A[DKG_MAX_OUTPUTS];
  double* X[DKG_MAX_OUTPUTS];
  int n[DKG_MAX_OUTPUTS];
  int* info[DKG_MAX_OUTPUTS];
};
hipError_t launch_cholesky_batch(const PrepBatch& b, int m, hipStream_t s);
hipError_t launch_tri_inverse_batch(const PrepBatch& b, int m, hipStream_t s);
hipError_t launch_tri_inverse(double* L, double* X, int n, const int* info, hipStream_t s);
hipError_t launch_alpha(const double* X, const double* y, double c, int n, double* alpha, const int* info,
                        hipStream_t s);
hipError_t launch_pack_linv(const double* X, int n, double* rf, hipStream_t s);
// One observation appended to an output's state (dkg_append.hip, dkg_append_observation).
struct AppendArgs {
  dkg_output o;            // the old output: n, kernel, hyperparameters, inv_lengthscale, disc_frag
  int d, N;
  const double* L;         // old L, row-major n x n
  const double* M;         // old L^{-1}, row-major n x n
  const double* xt;        // new train_x, (n + 1) x d, its last row the new point
  const double* y;         // new targets, n + 1
  double diag;             // noise + the old factorisation's jitter
  const double* disc;      // [N x d]
  double *Ln, *Mn;         // new L and L^{-1}, (n + 1) x (n + 1)
  double* alpha;           // [pad16(n + 1)]
  double* qn;              // new disc_frag, N_pad x pad16(n + 1)
  double* mean;            // new disc_mean [pad16(N)]
  double *lvec, *beta;     // workspace [1024] each: l and beta', zero padded
  double* lam;             // workspace: lambda
  int* info;               // workspace: 0, or n + 1 when lambda^2 <= 0
};
constexpr size_t APPEND_WS_LAM = 64, APPEND_WS_L = 256, APPEND_WS_BETA = 256 + 8192, APPEND_WS_BYTES = 256 + 16384;
// The copy, solve, pack and discretisation launches of one append (root_frag: the new R^T, from Mn).
hipError_t launch_append(const AppendArgs& a, double* root_frag, hipStream_t s);
// A block of K rows appended to many states at once (dkg_append.hip, dkg_append_rows): one job per (state, output),
// its descriptor resident in the workspace; every launch carries all jobs (one grid dimension over them).
constexpr int ROWS_MAX = DKG_APPEND_MAX_ROWS;  // K <= 32; the kernels carry K + 1 vectors (the rows, then r' / beta)
constexpr int ROWS_CHUNK = 128;                // rows of M per workgroup of the W = B M stage
constexpr int ROWS_CH_DOUBLES = ROWS_MAX * ROWS_MAX + 2 * ROWS_MAX;  // C^{-1} [32][32], beta2 [32], gamma [32]
struct RowsJob {
  dkg_output o;            // the old output: n, kernel, hyperparameters, inv_lengthscale, disc_frag
  const double *L, *M;     // old L and L^{-1}, row-major n x n
  const double* xt;        // new train_x, (n + K) x d, the old rows first
  const double* y;         // new targets, n + K
  const double* disc;      // [N x d]
  double diag;             // noise + the old factorisation's jitter
  double *Ln, *Mn;         // new L and L^{-1}, (n + K) x (n + K)
  double *alpha, *rf;      // [pad16(n + K)], fragment-packed M' [pad16(n + K)^2]
  double *qn, *mean;       // new disc_frag N_pad x pad16(n + K), new disc_mean [N_pad]
  // workspace, np = pad16(n): kx [K + 1][np] = s kappa(X2, X), then r'[0..n);  bx [K + 1][np] = B, then beta;
  // wp [ceil(n / ROWS_CHUNK)][K + 1][np] = the row chunks' partial sums of B M, then of M^T beta;
  // kd [K][N_pad] = s kappa(X2, D);  ch [ROWS_CH_DOUBLES]
  double *kx, *bx, *wp, *kd, *ch;
  int N, K;
};
// The launches of one dkg_append_rows: nmax, Kmax and Nmax are the largest n, K and N of the jobs (grid sizes).
hipError_t launch_append_rows(const RowsJob* jobs, int J, int d, int nmax, int Kmax, int Nmax, int* info,
                              hipStream_t s);
// Marginal log-likelihood and its gradient (dkg_mll.hip, dkg_mll_value_grad): after the factorisation, inverse
// and alpha of every output.  part: [mll_tiles(n)][MLL_NP] tile partials; out: [MLL_OUT] = value, then the
// gradient [c, l_1 .. l_d, s, noise].
constexpr int MLL_TB = 32;                    // tile width of the pair space
constexpr int MLL_NP = DKG_MAX_DIM + 2;       // partials per tile: tr W, sum W kappa, sum W h t_j^2 (j < d)
constexpr int MLL_OUT = DKG_MAX_DIM + 4;      // value + d + 3 gradient entries (stride of the result rows)
__host__ __device__ inline int mll_tiles(int n) {
  const int nt = (n + MLL_TB - 1) / MLL_TB;
  return nt * (nt + 1) / 2;
}
struct MllBatch {
  dkg_output o[DKG_MAX_OUTPUTS];             // n, kernel, hyperparameters, inv_lengthscale, train_x
  const double* y[DKG_MAX_OUTPUTS];          // targets [n]
  const double* L[DKG_MAX_OUTPUTS];          // chol(K), row-major n x n
  const double* M[DKG_MAX_OUTPUTS];          // L^{-1}, row-major n x n, zero upper triangle
  const double* alpha[DKG_MAX_OUTPUTS];      // K^{-1} (y - c) [pad16(n)]
  const int* info[DKG_MAX_OUTPUTS];          // the factorisation's status (non-zero: the output is skipped)
  double* part[DKG_MAX_OUTPUTS];
  double* out[DKG_MAX_OUTPUTS];
  int d;
};
hipError_t launch_mll(const MllBatch& b, int m, hipStream_t s);
// fp32 quad-packed copy (frag32_index) of a pair-packed fp64 (rows x n) matrix.
hipError_t launch_frag_to_f32(const double* frag, int rows, int n, float* out, hipStream_t s);
// The plan's per-scalarisation intercepts and their maxima (Plan::icpt / itop / itopk), from mu_all.
hipError_t launch_intercepts(const Plan& h, hipStream_t s);
// Row-major copy [rows][n_pad] of a fragment-packed (rows x n) matrix.
hipError_t launch_unpack_rows(const double* frag, int rows, int n, double* out, hipStream_t s);
hipError_t launch_cross_root(const CrossArgs& a, hipStream_t s);
// Value and gradient: kg[B] and dkg[B x d] (d KG(x_b) / d x_b), plan built with DKG_PLAN_GRAD.
// Candidates by value in the first kernel's arguments (dkg_plan_forward_grad_hostx); n = 0: unused.
struct XArg {
  double v[DKG_XARG_MAX];
  int n;
};
// hout (nullable): pinned host [kg (B) | dkg (B x d)] written by the envelope stage itself (split <= 2).
hipError_t launch_forward_grad(const Plan& h, const Plan* dev, const double* xnew, int B, double* kg, double* dkg,
                               hipStream_t s, const XArg* xa = nullptr, double* hout = nullptr);
// One stage of the forward (0 cross_root, 1 posterior_cov, 2 envelope) on stream s.  geom_B (0: B) is the
// batch size the covariance block shape is chosen for: a launch over K batches of geom_B candidates
// (dkg_plan_forward_batches) takes the blocks of one geom_B forward, so its results are those of K forwards.
hipError_t launch_stage(const Plan& h, const Plan* dev, const double* xnew, int B, double* kg, double* pairs,
                        hipStream_t s, int stage, int geom_B = 0);
hipError_t launch_forward(const Plan& host, const Plan* dev, const double* xnew, int B, double* kg, double* pairs,
                          hipStream_t s, hipEvent_t* ev, int geom_B = 0);
// The fused one-launch forward (dkg_fused.h) when the plan allows it (Plan::fused, no kg_pairs);
// otherwise the three stage kernels.  Same bits.
// Dynamic LDS bytes of the fused forward for a plan (dkg_fused.h fused_lds_bytes).
size_t fused_lds_bytes_host(const Plan& h);
// Sets dkg_last_error()'s thread-local message, printf-style (at most 511 bytes), and returns code; a hipError_t as
// a status (DKG_OK, or DKG_ERR_HIP and "what: the runtime's text"); the 256-byte rounding of the workspace carves.
// Every host translation unit reports through these; defined once, in dkg_abi.hip.
int failf(int code, const char* fmt, ...);
int hip_status(hipError_t e, const char* what);
size_t up256(size_t x);
// A workspace carve: take(bytes) is the offset of the next section and moves on by bytes rounded up to `align`
// (from an aligned offset that is up256(off + bytes), and take(0) does not move)
struct Carve {
  size_t off = 0;
  size_t take(size_t bytes, size_t align = 256) {
    const size_t at = off;
    off = (off + bytes + align - 1) & ~(align - 1);
    return at;
  }
  size_t total() const { return off; }
};
template <class T>
T* at(void* base, size_t off) {
  return reinterpret_cast<T*>(static_cast<char*>(base) + off);
}
// dkg_rff.hip.  The argument check of a dkg_rff_paths, and the values of its S paths: sample s's points [P][d] at
// x + s * x_stride (0: every sample evaluates the same points) into F + s * f_stride [P][m]; lb / ub not NULL: the
// model input is unit_cube(x, lb, ub).
int check_rff_paths(const dkg_rff_paths* p);
hipError_t launch_rff_eval(const dkg_rff_paths& p, const double* x, size_t x_stride, double* F, size_t f_stride,
                           const double* lb, const double* ub, int P, hipStream_t s);
hipError_t launch_forward_auto(const Plan& host, const Plan* dev, const double* xnew, int B, double* kg,
                               double* pairs, hipStream_t s);
// Envelope stage alone over P sets of L lines: KG, envelope sizes (nullable) and, when idx is given, the
// reference walk's indices [P][cap] and intersections [P][cap - 1] (lines_kg_kernel / lines_walk_kernel).
hipError_t launch_lines_kg(const double* a, const double* b, int P, int L, double* kg, int* nhull, long long* idx,
                           double* xs, int cap, hipStream_t s);
// The lines of every (candidate, scalarisation) pair after stages 0-1 (dkg_plan_lines).
hipError_t launch_lines_export(const Plan& h, const Plan* dev, int B, double* a_out, double* b_out, hipStream_t s);
// Reference formula of E[f(Z)] for P piecewise-linear f of m pieces (dkg_pwl_expectation).
hipError_t launch_pwl_expectation(const double* a, const double* b, const double* c, int P, int m, double* out,
                                  hipStream_t s);
// Per-workgroup phase stamps of the forward kernels: [3 kernels][KST_WG][8].
constexpr int KST_WG = 1024;
hipError_t launch_debug_wave(const double* in, double* out, hipStream_t s);
// The opt-in fp64 covariance block kernels (dkg_debug_cov_kernels): sets the mask, returns the previous one.
int set_cov_enabled(int mask);
// cross_tall_kernel's dispatch (dkg_debug_cross_tall): sets the mode (-1 default rule, 0 never, 1 every eligible
// shape), returns the previous one; the launches that took the kernel so far; and whether a stage-0 launch of B
// candidates of a plan (widest n_pad, d, fp32 or not) takes it under the current mode.
int set_cross_tall_mode(int mode);
long long cross_tall_launches();
bool cross_tall_eligible(int max_np, int d, int B, bool f32);
// Which fp32 kernels a launch of B candidates (block shapes chosen for geom_B; 0: B) of an F32 plan takes, by
// the launcher's own predicates (dkg_debug_f32_dispatch): out = {cross: 0 cross_root_plan_kernel<DM, float> /
// 1 cross_big32_kernel, covariance: 0 posterior_cov_kernel<DM, float> / 1 posterior_cov_big32_kernel<DM>, DM,
// the covariance launch's column blocks, row blocks, block order (-1: the narrow kernel has none)}.  The plan's
// workspace is taken to hold the K(x, X) fill wherever a launch of B uses it (max_B >= B).  Host only.
void f32_dispatch(int max_np, int d, int N, int m, int B, int geom_B, int out[6]);
hipError_t launch_debug_mfma(const double* a, const double* b, double* c, hipStream_t s);

// Launch geometry of the envelope stage for S scalarisation pairs: waves per workgroup and
// workgroups per candidate.
void envelope_geometry(int S, int* waves_per_wg, int* split);
// Dynamic LDS bytes of an envelope launch: the total of the kernels' own layout (dkg_device.h env_lds) for the
// plan's shape and the kernel's mode (envelope_body's GRAD / STREAM / GROWS; grows: global rows, with grad and
// stream only).  d and max_np count in the gradient's regions alone.
size_t envelope_lds_bytes(int m, int N, int waves, int S, int d, int max_np, bool grad, bool stream, bool grows);
// That layout's region offsets (doubles; -1: not in this mode) in layout order, then the total
// (dkg_debug_envelope_lds).
void envelope_lds_regions(int m, int N, int waves, int S, int d, int max_np, bool grad, bool stream, bool grows,
                          int out[DKG_ENV_LDS_REGIONS + 1]);
size_t cross_root_lds_bytes(int np, int d);

}  // namespace dkg
