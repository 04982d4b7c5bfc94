/*
 * dkg.h — C ABI of the MI355X-native Discrete Knowledge Gradient hot path.
 *
 * The reference (quasirandom/decoupled-kg, pure Python) computes the discrete
 * multi-objective KG in
 *   src/decoupledbo/modules/acquisition/discretekg.py
 *     DiscreteKnowledgeGradient.forward                       :131-159
 *     calculate_discrete_kg                                    :162-235
 *     calculate_discrete_kg_conditioning_on_single_output      :238-338
 *     calculate_epigraph_indices                               :341-412
 *     calculate_expected_value_of_piecewise_linear_function    :415-452
 * on top of BoTorch/GPyTorch exact GP posteriors (model.posterior at
 * :182-185 and :275-284; model family src/decoupledbo/modules/model/factory.py).
 *
 * This library replaces that arithmetic with hand-written HIP kernels for
 * gfx950.  Plain pointers and sizes only; every pointer marked "device" is a
 * device allocation owned by the caller; every entry point is stream ordered
 * on `stream` (a hipStream_t, NULL = legacy default stream) and never
 * synchronises unless its name says "timed".  Status codes instead of
 * exceptions; dkg_last_error() returns a thread-local message.
 *
 * Data layout in HBM (see DESIGN.md "Data layout"):
 *   n_pad(n) = n rounded up to a multiple of 16.
 *   A "fragment-packed" matrix P (rows x n, rows padded to 16, KB = n_pad/4
 *   k-blocks) is stored pair-packed:
 *     F[t][j][l][h] = P[16 t + (l & 15)][4 (2 j + h) + (l >> 4)],
 *   t < rows_pad/16, j < KB/2, l < 64, h < 2 — the per-lane operand order of
 *   v_mfma_f64_16x16x4_f64 for k-blocks 2j and 2j+1 side by side, so one
 *   coalesced 16-byte-per-lane (1 KiB) load feeds two MFMAs.  Padding entries
 *   are zero.
 */
#ifndef DKG_AMD_DKG_H
#define DKG_AMD_DKG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DKG_ABI_VERSION 9  /* 9: dkg_append_observation; 8: dkg_plan_forward_batches, dkg_plan_time_stage_batches */
/* Added under 9 since (new symbols only; nothing that existed changed): dkg_mll_*, dkg_posterior_mean, dkg_pareto_*,
 * dkg_jes_*, dkg_rff_workspace, dkg_rff_weights, dkg_rff_eval, dkg_debug_rff_gram, dkg_pareto_paths_workspace,
 * dkg_pareto_nsga2_paths, dkg_pareto_prune, dkg_hvkg_*, dkg_hypervolume, dkg_dominated_boxes*, dkg_hypervolume_front*,
 * dkg_append_rows*. */
#define DKG_MAX_OUTPUTS 8   /* outputs (objectives) per model list */
#define DKG_MAX_DIM 16      /* input dimension d */

enum dkg_status {
  DKG_OK = 0,
  DKG_ERR_ARG = 1,          /* bad argument / shape (reference raises BotorchTensorDimensionError) */
  DKG_ERR_UNSUPPORTED = 2,  /* outside supported sizes (reference: UnsupportedError) */
  DKG_ERR_WORKSPACE = 3,    /* workspace too small */
  DKG_ERR_HIP = 4,          /* HIP runtime error */
  DKG_ERR_NO_LINES = 5,     /* no lines (reference: ValueError, discretekg.py:466-470) */
  DKG_ERR_NOT_PD = 6        /* covariance not positive definite after the jitter retries
                               (linear_operator psd_safe_cholesky raises NotPSDError) */
};

/* Covariance families of model/factory.py:116 (ScaleKernel(base)). */
enum dkg_kernel { DKG_MATERN12 = 0, DKG_MATERN32 = 1, DKG_MATERN52 = 2, DKG_RBF = 3 };

/* Fitted state of one output GP (one SingleTaskGP of the ModelListGP,
 * factory.py:63-88) plus its caches over the discretisation.  The caches are
 * the quantities GPyTorch keeps for exact prediction with fast_pred_var:
 * R = L^{-T} with L = chol(K_XX + noise I), alpha = (K_XX + noise I)^{-1}(y - c). */
typedef struct dkg_output {
  int32_t n;                 /* training points */
  int32_t kernel;            /* enum dkg_kernel */
  double outputscale;        /* ScaleKernel outputscale s */
  double noise;              /* likelihood noise variance (model space) */
  double mean_constant;      /* ConstantMean c */
  double y_mean, y_std;      /* Standardize(m=1) untransform (0, 1 if absent) */
  const double* inv_lengthscale; /* device [d]: 1 / ARD lengthscale */
  const double* train_x;     /* device [n x d] row-major (normalised inputs) */
  const double* alpha;       /* device [n_pad(n)], zero padded */
  const double* root_frag;   /* device, fragment-packed R^T (P[c][r] = R[r][c]), n_pad^2 */
  const double* disc_frag;   /* device, fragment-packed Q_D = K(D,X) R: N_pad x n_pad (nullable for dkg_cross_root) */
  const double* disc_mean;   /* device [N]: c + K(D,X) alpha, model space (nullable for dkg_cross_root) */
} dkg_output;

int dkg_abi_version(void);
const char* dkg_last_error(void);

/* Number of doubles of a fragment-packed (rows x n) matrix: n_pad(rows)*n_pad(n). */
size_t dkg_frag_elems(int rows, int n);

/* out[i*n2+j] = s*k(x1_i, x2_j) (+ diag_add on i==j when n1==n2).
 * Replaces the covariance evaluation of ScaleKernel(Matern|RBF) (factory.py:110-135,
 * GPyTorch Kernel.forward) used to build K_XX + noise I for the Cholesky. */
int dkg_kernel_matrix(const dkg_output* o, int d, const double* x1, int n1, const double* x2, int n2,
                      double diag_add, double* out, void* stream);

/* Bytes of device scratch dkg_prepare_output needs for n training points. */
size_t dkg_prepare_workspace(int n);

/* Fitted-state caches of one output computed on the device by the library's
 * own kernels (no rocSOLVER / rocBLAS): the quantities GPyTorch's exact
 * prediction caches behind model.posterior (discretekg.py:182-185, 275-284;
 * gpytorch DefaultPredictionStrategy, linear_operator psd_safe_cholesky):
 *   K = s k(X, X) + noise I (+ jitter I)
 *   L = chol(K): blocked right-looking Cholesky; when it fails, retried with
 *       absolute jitter 1e-8 * 10^i, i < max_tries (linear_operator's policy)
 *   R = L^{-T} (root_inv_decomposition), packed into root_frag
 *   alpha = K^{-1} (y - c)  (n_pad doubles, zero padded)
 * o: n, kernel, outputscale, noise, mean_constant, inv_lengthscale, train_x
 *    (alpha / root_frag / disc_* are ignored).  train_y: device [n] targets
 * (model space).  L: device [n x n], receives L (row-major, zero upper
 * triangle).  work: device scratch of dkg_prepare_workspace(n) bytes; on
 * return it starts with L^{-1} (row-major n x n).  jitter_used (host,
 * nullable): the absolute jitter that made K positive definite (0 if none).
 * Synchronises `stream` once per Cholesky attempt (the retry policy reads the
 * factorisation status).  DKG_ERR_NOT_PD if every attempt failed. */
int dkg_prepare_output(const dkg_output* o, int d, const double* train_y, int max_tries, double* L, void* work,
                       size_t work_bytes, double* alpha, double* root_frag, double* jitter_used, void* stream);

/* dkg_prepare_output for m outputs at once (host arrays of m per-output pointers): every launch of
 * the first Cholesky attempt and of the inverse carries all outputs (one workgroup column per output),
 * one synchronisation checks all the factorisations, and only outputs that failed are retried with
 * jitter, one by one.  Same results as m calls of dkg_prepare_output.  jitter_used: host [m]. */
int dkg_prepare_outputs(const dkg_output* outs, int m, int d, const double* const* train_y, int max_tries,
                        double* const* L, void* const* work, const size_t* work_bytes, double* const* alpha,
                        double* const* root_frag, double* jitter_used, void* stream);

/* Pack dense row-major R (n x n, device) into o->root_frag layout (device). */
int dkg_pack_root(const double* r, int n, double* root_frag, void* stream);

/* Q = K(x, X) R (fragment-packed, rows x n) and mean = c + K(x, X) alpha (model
 * space, nullable).  This is the test-train half of GPyTorch's exact
 * prediction (DefaultPredictionStrategy mean_cache / covar_cache products)
 * behind model.posterior (discretekg.py:182-185, :275-284).  With x = the
 * discretisation D it builds disc_frag / disc_mean. */
int dkg_cross_root(const dkg_output* o, int d, const double* x, int rows, double* q_frag,
                   double* mean, void* stream);

/* Bytes of device scratch dkg_append_observation needs (n training points before the append, N
 * discretisation points); 0 for n < 1 or N < 0. */
size_t dkg_append_workspace(int n, int N);

/* One observation appended to an output's fitted state without refactorising: from the caches of
 * (X, y) those of ([X; x_new], y'), by the bordered Cholesky in fp64.  The reference rebuilds its model,
 * and every cache behind model.posterior (discretekg.py:182-185), at each BO iteration
 * (bo_loop.py:457-465); a decoupled step adds one row to one output and leaves the others alone.
 * With M = L^{-1}, k = s kappa(X, x_new), r' = y' - c:
 *   l = M k, lambda^2 = s kappa(x, x) + noise + jitter - l.l
 *   L' = [[L, 0], [l^T, lambda]],  M' = [[M, 0], [-(l^T M) / lambda, 1 / lambda]]
 *   alpha' = M'^T M' r',  Q_D' = [Q_D, (s kappa(D, x_new) - Q_D l) / lambda],  mu_D' = c + Q_D' M' r'
 *   o       : the old state: n, kernel, hyperparameters, inv_lengthscale, disc_frag (N_pad x n_pad(n);
 *             train_x, alpha, root_frag and disc_mean are not read)
 *   L, Linv : device [n x n] row-major, the old L and L^{-1} (dkg_prepare_output's L and the head of its work)
 *   disc    : device [N x d], the discretisation the old disc_frag was built over (nullable when N = 0,
 *             as are o->disc_frag, disc_frag_new and disc_mean_new)
 *   train_x : device [(n + 1) x d], its last row x_new;  train_y: device [n + 1], the new targets y'
 *             (the old ones with y_new appended, or wholly new values)
 *   jitter  : the absolute jitter the old factorisation used (dkg_prepare_output's jitter_used)
 *   L_new, Linv_new [(n + 1)^2], alpha_new [n_pad(n + 1)], root_frag_new [n_pad(n + 1)^2],
 *   disc_frag_new [N_pad x n_pad(n + 1)], disc_mean_new [N_pad]: device, written; padding exactly zero.
 *   work    : device scratch of dkg_append_workspace(n, N) bytes.
 * Out of place: nothing of the old state is written, so plans and captured graphs on it stay valid.
 * Stream ordered; synchronises `stream` once to read the status.  DKG_ERR_NOT_PD when lambda^2 <= 0 or is
 * not finite (the outputs are then not to be used: rebuild with dkg_prepare_output, which applies the
 * jitter policy), DKG_ERR_UNSUPPORTED when n_pad(n + 1) > 1024, DKG_ERR_ARG for NULL pointers or bad
 * sizes; the arguments are checked before any HIP call.  Deterministic: every sum runs in a fixed order. */
int dkg_append_observation(const dkg_output* o, int d, const double* L, const double* Linv, const double* disc, int N,
                           const double* train_x, const double* train_y, double jitter, double* L_new,
                           double* Linv_new, double* alpha_new, double* root_frag_new, double* disc_frag_new,
                           double* disc_mean_new, void* work, size_t work_bytes, void* stream);

/* A block of K observations appended to each of J fitted states in one batched update: exact-GP conditioning on
 * new rows (BoTorch's condition_on_observations) without refactorising, every launch carrying all jobs.  One
 * job, with M = L^{-1}, X2 the K new rows, r' = y' - c, j the old factorisation's jitter:
 *   B  = s kappa(X2, X) M^T  [K x n],   beta = M r'[0..n)
 *   S  = s kappa(X2, X2) + (noise + j) I - B B^T,  C = chol(S)   (a pivot <= 0 or not finite: not positive definite)
 *   W  = B M,   L' = [[L, 0], [B, C]],   M' = [[M, 0], [-C^{-1} W, C^{-1}]]
 *   beta2 = C^{-1} (r'[n..) - B beta),  gamma = C^{-T} beta2,  alpha' = M'^T M' r' = [M^T beta - W^T gamma ; gamma]
 *   Q_D' = [Q_D, (s kappa(D, X2) - Q_D B^T) C^{-T}],  mu_D' = c + Q_D beta + Q_D'[:, n..) beta2
 * alpha' is always formed from all n + K targets, as dkg_append_observation forms it: the old targets may change.
 *   o, L, Linv, disc, N, jitter : as dkg_append_observation reads them (o also passes dkg_cross_root's checks)
 *   K       : new rows, 1..DKG_APPEND_MAX_ROWS, with n_pad(n + K) <= 1024
 *   train_x : device [(n + K) x d], the old rows first;  train_y: device [n + K]
 *   L_new, Linv_new [(n + K)^2], alpha_new [n_pad(n + K)], root_frag_new [n_pad(n + K)^2],
 *   disc_frag_new [N_pad x n_pad(n + K)], disc_mean_new [N_pad]: device, written; padding exactly zero.
 * Out of place; fp64; no atomics; every sum in a fixed order that depends on the job's own n, K and N alone, so a
 * job's bits do not depend on the other jobs of the call or on its position among them.  The number of launches
 * does not depend on J. */
#define DKG_APPEND_MAX_ROWS 32
#define DKG_APPEND_MAX_JOBS 512   /* DKG_JES_MAX_SAMPLES x DKG_MAX_OUTPUTS */
typedef struct dkg_append_job {
  const dkg_output* o;               /* old state, as dkg_append_observation reads it */
  const double *L, *Linv;            /* old, device [n x n] */
  const double* disc; int32_t N;     /* NULL / 0: no discretisation */
  int32_t K;
  const double* train_x;             /* device [(n + K) x d], the old rows first */
  const double* train_y;             /* device [n + K] */
  double jitter;
  double *L_new, *Linv_new, *alpha_new, *root_frag_new, *disc_frag_new, *disc_mean_new;
} dkg_append_job;

/* Bytes of device scratch dkg_append_rows needs for these jobs; 0 for NULL jobs, J outside
 * 1..DKG_APPEND_MAX_JOBS, d outside 1..DKG_MAX_DIM, or a job with a NULL o, n < 1, K outside
 * 1..DKG_APPEND_MAX_ROWS, n_pad(n + K) > 1024 or N < 0. */
size_t dkg_append_rows_workspace(const dkg_append_job* jobs, int J, int d);

/* Runs the J jobs.  info: host [J], receives 0 or, for a job that is not positive definite, the failing column
 * + 1 (n + the failing pivot of S + 1); such a job's outputs are not to be used, the others' are complete.
 * Synchronises `stream` once, for all status words.  DKG_OK when every job succeeded, DKG_ERR_NOT_PD when any
 * failed; DKG_ERR_ARG for NULL pointers and bad sizes, DKG_ERR_UNSUPPORTED for K, J or n + K beyond the limits,
 * DKG_ERR_WORKSPACE for a short workspace: the arguments are checked before any HIP call. */
int dkg_append_rows(const dkg_append_job* jobs, int J, int d, int32_t* info, void* work, size_t work_bytes,
                    void* stream);

/* Bytes of device scratch dkg_mll_value_grad needs for m outputs of n[i] training points; 0 for a NULL n,
 * m outside 1..DKG_MAX_OUTPUTS or an n[i] outside 1..1024. */
size_t dkg_mll_workspace(const int* n, int m);

/* The marginal log-likelihood of m outputs and its gradient in the hyperparameters, on the device: the objective
 * of the MAP fit (the reference's fit_gpytorch_mll on ExactMarginalLogLikelihood, factory.py:24-151,
 * bo_loop.py:63-79, 589-619) without priors, parameter transforms or the division by n, which stay with the
 * caller.  Per output o (reads n, kernel, outputscale s, noise, mean_constant c, inv_lengthscale, train_x and
 * train_y[o], device [n], model space), with K = s kappa(X, X) + (noise + jitter) I, L = chol(K), M = L^{-1},
 * r = y - c, alpha = M^T M r, G = M^T M, W = alpha alpha^T - G and t_ik = (x_i - x_k) / l:
 *   value[o] = log N(y | c 1, K) = -1/2 r.alpha - sum_i log L_ii - (n / 2) log 2 pi
 *   grad[o]  = [d/dc, d/dl_1 .. d/dl_d, d/ds, d/dnoise]  (host [m][d + 3]; lengthscales l, not their inverses;
 *              constrained space)
 *     d/dc = sum_i alpha_i,  d/dnoise = 1/2 tr W,  d/ds = 1/2 sum_ik W_ik kappa_ik,
 *     d/dl_j = -1/2 sum_ik W_ik s h(|t_ik|^2) t_ik,j^2 / l_j,  h = kappa'(r) / r (0 for Matern-1/2 at
 *     r^2 <= 1e-30: the diagonal and duplicated training points, as the reference's distance clamp gives)
 * The factorisation is dkg_prepare_outputs' own (all outputs in every launch; absolute jitter 1e-8 * 10^i,
 * i < max_tries, for the outputs that fail; jitter_used: host [m], nullable); DKG_ERR_NOT_PD if every attempt
 * failed.  The contraction runs over 32 x 32 tiles of the pair space with v_mfma_f64_16x16x4_f64; K^{-1} is
 * never written to memory.  work: device scratch of dkg_mll_workspace() bytes, the only memory written besides
 * the host results.  Synchronises `stream` (the results go to host memory).  Deterministic: every sum runs in a
 * fixed order, no atomics.  DKG_ERR_UNSUPPORTED for n > 1024, m > DKG_MAX_OUTPUTS or d > DKG_MAX_DIM,
 * DKG_ERR_ARG for NULL pointers or bad sizes, DKG_ERR_WORKSPACE for a short workspace; the arguments are
 * checked before any HIP call. */
int dkg_mll_value_grad(const dkg_output* outs, int m, int d, const double* const* train_y, int max_tries,
                       void* work, size_t work_bytes, double* value, double* grad, double* jitter_used,
                       void* stream);

/* ---- Posterior-mean Pareto front: NSGA-II on the device (dkg_pareto.hip) -----------------------------
 * The reference samples the Pareto front of the surrogate's posterior mean with pygmo.nsga2(gen=100) at every
 * BO iteration (modules/pareto/sample.py:16-48; "Record metrics", bo_loop.py:294-332, 480-520) and of the test
 * problem once (main.py:174).  pygmo is not restated: the operators are the published ones (Deb & Agrawal 1995,
 * Deb et al. 2002) with pygmo's documented nsga2 defaults, every random number comes from the caller, and no
 * trajectory parity with pygmo is claimed.  All objectives are maximised.  Limits: m <= DKG_MAX_OUTPUTS,
 * d <= DKG_MAX_DIM, n <= 1024 per output, population P a multiple of 4 with 8 <= P <= 1024 (DKG_ERR_UNSUPPORTED /
 * DKG_ERR_ARG otherwise, checked before any device work).  Stream ordered; nothing synchronises. */

/* mean[p*m + i] = y_mean_i + y_std_i (c_i + K(x_p, X_i) alpha_i) for P points x (device [P][d], model inputs):
 * the posterior mean BoTorchModel.batch_fitness (sample.py:138-144) and GPTestProblem.evaluate_true
 * (gp_testproblem.py:76-97) take from model.posterior, without the O(P n^2) product Q = K(x, X) R that
 * dkg_cross_root forms next to it.  Reads n, kernel, the hyperparameters, inv_lengthscale, train_x and alpha
 * (dkg_prepare_outputs' caches); root_frag and disc_* are not read.  The kernel terms are the cross stage's; a
 * point's result is one fma chain per lane over the training points and a fixed-order wave reduction, so it has
 * the same bits whatever P is and whichever row holds the point.  P = 0 is a no-op. */
int dkg_posterior_mean(const dkg_output* outs, int m, int d, const double* x, int P, double* mean, void* stream);

/* Bytes of device scratch dkg_pareto_rank's wide path needs for Q points of m objectives (dominator counts and
 * fronts [Q] ints each, a few scalars); 0 outside 1 <= Q <= 16384, 1 <= m <= DKG_MAX_OUTPUTS. */
size_t dkg_pareto_rank_workspace(int Q, int m);

/* Non-dominated ranks, crowding distances and survivor order of Q points F (device [Q][m], m <= 8): Q <= 2048
 * without a workspace, Q <= 16384 with one.
 *   dominance: a dominates b iff a >= b in every objective and a > b in at least one (equal points do not
 *              dominate each other)
 *   rank     : fronts are peeled in order (Deb et al. 2002) until at least `keep` points carry a rank
 *              (1 <= keep <= Q; the last front peeled is ranked whole); the rest get rank -1 and crowding 0
 *   crowd    : within each ranked front, for j = 0 .. m-1 in order: members sorted by (f_j ascending, index
 *              ascending), the two ends add +inf, an interior member adds (f_j[next] - f_j[prev]) /
 *              (f_j^max - f_j^min), or 0 when the front's range in j is 0; one subtraction, one division and
 *              one addition per step, no fused multiply-add
 *   order    : device int [Q]: the ranked points by (rank ascending, crowding descending, index ascending),
 *              then -1; its first `keep` entries are the survivors
 * The results are integers and one subtraction, division and addition per crowding step, so both paths below
 * give the same bits.  Every loop of every kernel is bounded by Q; no workgroup waits on another.
 *   work == NULL: one workgroup (pareto_rank_kernel) ranks the Q <= 2048 points out of its LDS;
 *                 DKG_ERR_UNSUPPORTED above 2048.  work_bytes is not read.
 *   work != NULL: device scratch of at least dkg_pareto_rank_workspace(Q, m) bytes (DKG_ERR_WORKSPACE when
 *                 work_bytes is short; DKG_ERR_UNSUPPORTED for Q > 16384), overwritten by every call and carrying
 *                 nothing from one call to the next.  2048 < Q <= 16384 runs the wide path: five stream-ordered
 *                 launches (clear, dominator counts over point tiles x slices of the points, the front peel in one
 *                 workgroup, crowding and order with one wave per point).  Q <= 2048 runs the path a host rule of
 *                 (Q, m) names, measured per objective bucket (dkg_debug_pareto_wide overrides it).
 * Argument checks come before any device work. */
int dkg_pareto_rank(const double* F, int Q, int m, int keep, int* rank, double* crowd, int* order, void* work,
                    size_t work_bytes, void* stream);

/* NSGA-II's variation parameters; pygmo.nsga2's documented defaults are {0.95, 10, 0.01, 50}.  raw_inputs
 * (dkg_pareto_nsga2 only): 0 = the model takes inputs normalised to the unit cube with lb / ub (a surrogate,
 * sample.py:129-130), 1 = it takes the points as they are (a test problem, gp_testproblem.py:76-97). */
typedef struct dkg_nsga2_params {
  double cr;     /* crossover probability per pair of children */
  double eta_c;  /* distribution index of the simulated binary crossover */
  double m;      /* mutation probability per coordinate */
  double eta_m;  /* distribution index of the polynomial mutation */
  int32_t raw_inputs;
  int32_t reserved;
} dkg_nsga2_params;

/* Uniforms in [0, 1) one dkg_pareto_variation call reads for a population of P in d dimensions (0 for an odd or
 * non-positive P or d < 1).  Layout, H = P / 2 pairs of children (children 2k, 2k + 1 from winners 2k, 2k + 1):
 *   [0, 2P)                  u[2w], u[2w + 1]: the two members floor(u P) of winner w's tournament
 *   [2P, 2P + H)             pair k crosses over iff u < cr
 *   then [H][d][3]           per (pair, coordinate): the coordinate is crossed iff u0 < 0.5 (and the parents differ
 *                            by more than 1e-14), u1 the spread draw, the two children are swapped iff u2 < 0.5
 *   then [P][d][2]           per (child, coordinate): mutated iff u0 < m, u1 the perturbation draw */
size_t dkg_pareto_draws(int P, int d);

/* P children (device [P][d]) of a ranked population X (device [P][d]; rank, crowd: device [P], every member
 * ranked, as dkg_pareto_rank with keep = P leaves them).  Selection: binary tournament between two members drawn
 * with replacement; the lower rank wins, then the larger crowding, then the first drawn.  Crossover: bounded
 * simulated binary crossover on consecutive winners; mutation: bounded polynomial mutation; children are clipped
 * into [lb, ub] (device [d] each).  No random number generator runs on the device: `uniforms` (device,
 * dkg_pareto_draws(P, d) doubles in [0, 1)) is the only randomness.  With cr = 0 and m = 0 every child is a
 * bit-exact copy of its tournament winner. */
int dkg_pareto_variation(const double* X, const int* rank, const double* crowd, int P, int d, const double* lb,
                         const double* ub, const dkg_nsga2_params* prm, const double* uniforms, double* children,
                         void* stream);

/* Bytes of device scratch dkg_pareto_nsga2 needs (0 outside the limits above); it includes
 * dkg_pareto_rank_workspace(2P, m), so its ranks follow dkg_pareto_rank's rule with a workspace.  The posterior-mean
 * kernel normalises the points itself, so there is no section for normalised points: the value is smaller, by
 * P d doubles rounded up to 256 bytes, than the first libraries of this ABI version returned. */
size_t dkg_pareto_workspace(int P, int d, int m);

/* The whole evolution, no host synchronisation inside: what pop = algo.evolve(pop) does at sample.py:40-44.
 *   uniforms: device, P d + gens * dkg_pareto_draws(P, d) doubles in [0, 1)
 *   generation 0: X = lb + u (ub - lb) from the first P d uniforms, F = the posterior mean there, ranked with
 *                 keep = P (X keeps the sampled order)
 *   generation g >= 1, from the uniforms at P d + (g - 1) dkg_pareto_draws(P, d):
 *     dkg_pareto_variation -> P children; dkg_posterior_mean of the children (of (x - lb) / (ub - lb) unless
 *     prm->raw_inputs); dkg_pareto_rank of the 2P points [parents; children] with keep = P; the survivors, in
 *     `order` order, become X, F, rank, crowd ((mu + lambda) elitist survival)
 *   X [P][d], F [P][m], rank [P], crowd [P]: device, the final population and its ranking
 *   work: device scratch of dkg_pareto_workspace(P, d, m) bytes (DKG_ERR_WORKSPACE when short)
 * Bit for bit what the same sequence of the three stage entries gives. */
int dkg_pareto_nsga2(const dkg_output* outs, int m, int d, const double* lb, const double* ub, int P, int gens,
                     const dkg_nsga2_params* prm, const double* uniforms, double* X, double* F, int* rank,
                     double* crowd, void* work, size_t work_bytes, void* stream);

/* ---- Lower-bound joint entropy search (JES-LB / LB2, Tu et al. 2022) on the device (dkg_jes.hip) ------------
 * The reference's qLowerBoundMultiObjectiveJointEntropySearch (modules/acquisition/joint_entropy_search.py:291-526)
 * for q = 1 with estimation_type "LB" / "LB2" and its target_output_ix: per candidate x
 *   acq(x) = H_0(x) - (1 / P) sum_p H_p(x)
 * with H_0 the entropy of the model's noisy predictive at x (:402-425; all outputs, or the target alone) and H_p
 * the entropy bound of _compute_entropy_upper_bound (:596-732) on the moments of the model conditioned on Pareto
 * sample p (:365-376, 428-470) over that sample's boxes.  All objectives are maximised.  DESIGN.md 8d states the
 * formulas.  A "state" is one model: state 0 the model itself, state p + 1 the model conditioned on sample p;
 * each is m dkg_output structs of which n, kernel, outputscale, noise, mean_constant, y_mean, y_std,
 * inv_lengthscale, train_x, alpha and root_frag are read (dkg_prepare_outputs' caches; disc_* are not read).
 * Limits (DKG_ERR_UNSUPPORTED beyond them): m <= DKG_MAX_OUTPUTS, d <= DKG_MAX_DIM, n <= 1024 per state-output,
 * P <= DKG_JES_MAX_SAMPLES samples, J <= DKG_JES_MAX_BOXES boxes per sample, max_B <= DKG_JES_MAX_CANDIDATES. */
#define DKG_JES_MAX_SAMPLES 64
#define DKG_JES_MAX_BOXES 4096
#define DKG_JES_MAX_CANDIDATES 65536
/* Bytes of the host plan (caller memory, kept unchanged while the plan is in use). */
size_t dkg_jes_plan_bytes(void);
/* Bytes of device scratch a plan for up to max_B candidates needs: the state table, and per (state, output,
 * candidate) the model-space mean, |K(x, X) R|^2 and their d x-derivatives.  0 for sizes dkg_jes_init refuses. */
size_t dkg_jes_workspace(int m, int P, int d, int J, int max_B);
/* A plan: everything an evaluation needs besides the candidates.
 *   states       : host array of (P + 1) m structs, state s output i at s m + i; copied into host_plan and
 *                  uploaded once into the workspace on `stream` (the device buffers they point to must outlive
 *                  the plan)
 *   bounds       : device [P][2][J][m], the hypercell bounds (hypercell_bounds of :66-71; [.][0] lower, [.][1]
 *                  upper corners, untransformed output space).  Lower bounds may be -1e10 and a sample with
 *                  fewer boxes is padded with zero-width boxes [0, 0] (jes_sample_pareto.py:243-245).  Read at
 *                  every evaluation, not copied.
 *   target       : -1 all outputs observed, t in [0, m) the reference's target_output_ix
 *   only_diagonal: 0 "LB", non-zero "LB2" (:232-250)
 *   workspace    : device scratch of dkg_jes_workspace() bytes, owned by the plan while it is in use
 * DKG_ERR_ARG for NULL pointers, sizes < 1, a target outside [-1, m), n < 1 or an unknown kernel id;
 * DKG_ERR_UNSUPPORTED beyond the limits above; DKG_ERR_WORKSPACE for a short workspace.  The arguments are checked
 * before any HIP call; nothing synchronises. */
int dkg_jes_init(const dkg_output* states, int m, int P, int d, const double* bounds, int J, int target,
                 int only_diagonal, int max_B, void* workspace, size_t workspace_bytes, void* host_plan, void* stream);
/* acq[b] for B <= max_B candidates x (device [B][d], model inputs) and, when dacq_dx is not NULL,
 * dacq_dx[b*d + j] = d acq[b] / d x[b*d + j] (device [B][d]): what autograd gives optimize_acqf through
 * qLowerBoundMultiObjectiveJointEntropySearch.forward (:512-526, acquisition_optimisation_strategy.py:493-508).
 * Wherever one of the reference's clamps binds, that term's derivative is 0, as clamp_min / clamp_max give.
 *   moments_out (nullable): device [3][(P + 1) m][B], untransformed space, per (state, output, candidate):
 *     [0] the posterior mean, [1] v = max(var, eps), [2] tau = max(max(var + noise, eps) - v, eps)
 *     (eps = 2^-52, :403, 440-461); state 0: [1] holds var + noise (the argument of H_0) and [2] is 0.
 * Two launches whatever P and m are: the moments of every (state, output) over 16-candidate tiles
 * (v_mfma_f64_16x16x4_f64 against root_frag; K(x, X) R is never written to memory), then one workgroup per
 * candidate for the entropies and the chain rule to dx.  Stream ordered, nothing synchronises.  Deterministic:
 * every sum runs in a fixed order without atomics, so two calls give the same bits and a candidate's result has
 * the same bits whatever B is and whichever row holds it.  DKG_ERR_ARG for NULL pointers, an uninitialised plan
 * or B outside [1, max_B], checked before any HIP call. */
int dkg_jes_forward(const void* host_plan, const double* x, int B, double* acq, double* dacq_dx, double* moments_out,
                    void* stream);

/* ---- The Pareto samples of joint entropy search on the device (dkg_rff.hip) -----------------------------------
 * The reference's sample_discrete_pareto_optimal_points (modules/pareto/jes_sample_pareto.py:48-232): per sample a
 * posterior path of the model drawn with random Fourier features (BoTorch's get_gp_samples, :81-86), NSGA-II on the
 * path (:146-207) and the pruning of its front by repeated crowding distance (:210-232).  Here every sample runs in
 * the same launches.  fp64, stream ordered, every sum in a fixed order, no atomics on floating-point values, every
 * random number from the caller.  All objectives are maximised.  DESIGN.md 8e states what differs from BoTorch and
 * pymoo.  Limits (DKG_ERR_UNSUPPORTED beyond them): S <= DKG_JES_MAX_SAMPLES samples, R <= DKG_RFF_MAX_FEATURES
 * features, m <= DKG_MAX_OUTPUTS, d <= DKG_MAX_DIM, n <= 1024; the arguments are checked before any HIP call. */
#define DKG_RFF_MAX_FEATURES 1024
/* S samples of an m-output model: sample s, output i is the function of the model inputs x
 *   f(x) = offset[s][i] + sum_r coef[s][i][r] cos(omega[s][i][r] . x + bias[s][i][r]).
 * Every pointer is a device allocation of the caller's. */
typedef struct dkg_rff_paths {
  int32_t S, m, d, R;
  double* omega;  /* [S][m][R][d] */
  double* bias;   /* [S][m][R] */
  double* coef;   /* [S][m][R] */
  double* offset; /* [S][m] */
} dkg_rff_paths;

/* Bytes of device scratch dkg_rff_weights needs for R features and outputs of at most n_max training points: eight
 * problems' A, L^{-1} and Phi at a time.  0 outside 1 <= R <= DKG_RFF_MAX_FEATURES, 1 <= n_max <= 1024. */
size_t dkg_rff_workspace(int R, int n_max);

/* The weight-space posterior sample of every (sample, output): fills paths->omega, bias, coef, offset (paths->S,
 * m, d, R give the sizes; m and d must equal the arguments).  Per (sample s, output i), from the caller's draws
 * (device; standard normals wn [S][m][R][d] and z [S][m][R], g [S][m][R] draws of Gamma(shape nu, rate nu) for a
 * Matern-nu output (not read for DKG_RBF; nullable when every output is DKG_RBF), uniforms ub [S][m][R] in [0, 1)):
 *   omega_r = wn_r * inv_lengthscale * g_r^(-1/2)      (the factor g_r^(-1/2) = 1 / sqrt(g_r) for Matern only: the
 *                                                       multivariate-t spectral density with 2 nu degrees of freedom)
 *   b_r = 2 pi ub_r,  amp = sqrt(2 s / R),  Phi[k][r] = amp cos(omega_r . x_k + b_r)  over the output's n training
 *                                                       rows; the phase is one fma per coordinate in order from 0,
 *                                                       then + b_r
 *   A = Phi^T Phi + noise I  (sums over the rows in order),  L = chol(A)
 *   theta = L^{-T} (L^{-1} Phi^T (y - c) + sqrt(noise) z),  so theta ~ N(A^{-1} Phi^T (y - c), noise A^{-1})
 *           (the products are with the explicit L^{-1}; the mean term A^{-1} Phi^T (y - c) is refined once against
 *           L L^T, which brings it to the accuracy of a substitution solve)
 *   coef_r = y_std amp theta_r,  offset = y_mean + y_std c
 * outs: n, kernel, outputscale s, noise, mean_constant c, y_mean, y_std, inv_lengthscale and train_x are read;
 * train_y: host array of m device pointers, [n] targets in model space.  The constant mean is taken off the targets
 * and restored in the offset.  The factorisation is dkg_prepare_outputs' own (launch_cholesky_batch and
 * launch_tri_inverse_batch over at most eight matrices per call, one status check per batch; a problem that fails is
 * retried on its own with absolute jitter 1e-8 * 10^i, i < max_tries, added to the diagonal of A; theta keeps
 * sqrt(noise)); DKG_ERR_NOT_PD if every attempt failed.  jitter_used: host [S][m], nullable.  work: device scratch
 * of dkg_rff_workspace(R, max n) bytes (DKG_ERR_WORKSPACE when short).  Synchronises `stream` once per batch of
 * eight problems (the retry policy reads the status).  A is conditioned like noise^-1 s n: at noise <= 1e-8 s the
 * system is too ill-conditioned for any fp64 solve to pin theta; the sample is still a sample. */
int dkg_rff_weights(const dkg_output* outs, int m, int d, const double* const* train_y, const double* wn,
                    const double* g, const double* ub, const double* z, int max_tries, const dkg_rff_paths* paths,
                    void* work, size_t work_bytes, double* jitter_used, void* stream);

/* Which kernel forms Phi^T Phi: 0 tiles of v_mfma_f64_16x16x4_f64 (the default), 1 VALU fma tiles (A/B
 * measurements; the two round differently), -1 only reads.  Returns the previous mode, -2 on a bad one. */
int dkg_debug_rff_gram(int mode);

/* Dynamic LDS of the path evaluation's workgroup: one output's omega [R][d], bias [R] and coef [R].  At the limits
 * (R = 1024, d = 16) it is 144 KiB of the 160 KiB a workgroup can have, so nothing is staged in halves. */
#define DKG_RFF_EVAL_LDS_BYTES(R, d) ((size_t)(R) * ((d) + 2) * 8)

/* F[s][p][i] = f_{s,i}(x_{s,p}) for x device [S][P][d] (shared_x = 0) or one [P][d] evaluated by every sample
 * (shared_x != 0); F device [S][P][m].  One workgroup per (sample, output, 16 points) stages the output's (omega,
 * bias, coef) in LDS once; one wave per point; lane l owns the features l, l + 64, ...: the phase is one fma per
 * coordinate in order from 0, then + bias_r, and acc = fma(cos(phase), coef_r, acc) is one chain per lane; wave_sum's fixed-order
 * reduction; F = offset + sum.  A point's bits depend on the point and its path alone: not on P, on its row, or on
 * the samples evaluated beside it (a struct whose pointers start at sample s evaluates that sample alone).
 * P = 0 is a no-op. */
int dkg_rff_eval(const dkg_rff_paths* paths, const double* x, int P, int shared_x, double* F, void* stream);

/* Bytes of device scratch dkg_pareto_nsga2_paths needs (0 outside the limits). */
size_t dkg_pareto_paths_workspace(int S, int P, int d, int m);

/* dkg_pareto_nsga2 for S populations at once, population s evolving on sample s of `paths`.  It is the same
 * generation driver with the paths as its fitness (dkg_pareto.hip: dkg_pareto_nsga2 is its S = 1 case on the
 * posterior mean, with the wide rank's scratch): every launch carries a sample axis (init; then per generation the
 * variation, which also copies the parents; dkg_rff_eval of the children; the one-workgroup rank of the 2P points,
 * one workgroup per sample; the gather).  Four launches per generation whatever S is, no host synchronisation.
 *   uniforms: device [S][P d + gens * dkg_pareto_draws(P, d)], sample s's row laid out as dkg_pareto_nsga2's
 *   lb, ub  : device [d], shared by the samples; the path takes (x - lb) / (ub - lb) unless prm->raw_inputs
 *   X [S][P][d], F [S][P][m], rank [S][P], crowd [S][P]: device, the final populations and their rankings
 *   work    : device scratch of dkg_pareto_paths_workspace(S, P, d, m) bytes
 * Sample s of the result has exactly the bits the stage entries give for that sample alone (dkg_pareto_variation,
 * dkg_rff_eval on sample s, dkg_pareto_rank with keep = P, the survivors in `order` order), and so the bits of an
 * S = 1 call on sample s with its row of uniforms.  P as dkg_pareto_nsga2 (a multiple of 4, 8 <= P <= 1024). */
int dkg_pareto_nsga2_paths(const dkg_rff_paths* paths, const double* lb, const double* ub, int P, int gens,
                           const dkg_nsga2_params* prm, const double* uniforms, double* X, double* F, int* rank,
                           double* crowd, void* work, size_t work_bytes, void* stream);

/* The reference's prune_pareto_front (jes_sample_pareto.py:210-232) on the non-dominated members of S populations
 * F (device [S][Q][m]) ranked by `rank` (device [S][Q], as dkg_pareto_rank leaves it), one workgroup per sample:
 *   - the members are the points of rank 0 (pymoo's result is the non-dominated set, :207);
 *   - of members with bit-equal objective vectors only the lowest index stays (eliminate_duplicates, :202);
 *   - while more than k members are left: the crowding distance of each within the set that is left, by
 *     dkg_pareto_rank's arithmetic (per objective in order one subtraction, division and addition, no fused
 *     multiply-add; the ends +inf), and the member of smallest (crowding, index) is retired.  The reference breaks
 *     ties at random; here the lowest index goes.
 *   count [S]: the members left (<= k);  index [S][k]: their indices ascending, then -1.
 * 1 <= Q <= 2048, 1 <= k <= 2048, S <= DKG_JES_MAX_SAMPLES, m <= DKG_MAX_OUTPUTS.
 * Cost: every retirement is a round of the sample's one workgroup in which each member left rescans the Q points
 * per objective, so a sample takes (members - k) rounds of O(Q m) each, one after the other: 90 rounds at the
 * preset (100 members to 10), but about 2047 rounds of 4096 m reads per thread at Q = 2048, all of rank 0, k = 1
 * (tens of milliseconds).  Sized for populations, not for the 16384-point fronts of dkg_pareto_rank. */
int dkg_pareto_prune(const double* F, const int* rank, int S, int Q, int m, int k, int* count, int* index,
                     void* stream);

/* ---- Hypervolume knowledge gradient (HVKG, Daulton et al. 2023) on the device (dkg_hvkg.hip) -------------------
 * BoTorch's qHypervolumeKnowledgeGradient as the reference's HvkgOptimisationSpec drives it
 * (modules/acquisition_optimisation_strategy.py:276-444): q = 1, one-shot, the posterior mean as the inner value
 * function, X_evaluation_mask for the decoupled setting, and its value function (the hypervolume of the posterior
 * mean at q points, _compute_current_optimum :428-444).  All objectives are maximised; everything is fp64.
 * A one-shot point is X_full [1 + Nf Np][d]: row 0 the candidate x, row 1 + f Np + p point p of fantasy f
 * (BoTorch's layout).  Per output i, with mu_i, c_i the model-space posterior mean and covariance and
 * sigma~_i(x) = sqrt(c_i(x, x) + noise_i):
 *   Y_fp,i = y_mean_i + y_std_i (mu_i(x'_fp) + [i in E] z_f,i c_i(x'_fp, x) / sigma~_i(x))
 *   HV_f   = the volume of the union over p of the boxes [ref, Y_fp]; a point that is not strictly above ref in
 *            every objective adds nothing
 *   acq    = ((1 / Nf) sum_f HV_f - current_value) / cost
 * The fantasy mean is the exact posterior mean after observing mu_i(x) + sigma~_i(x) z_f,i at x with the
 * likelihood's noise (fantasize + PosteriorMeanModel, without refactorising).  Gradient conventions at kinks
 * (subgradients): a point that adds no volume (dominated, or not strictly above ref) gets exactly 0; of points
 * with equal coordinates the lowest index takes the derivative.  DESIGN.md 8f.
 * Outputs are dkg_prepare_outputs' structs (n, kernel, the hyperparameters, y_mean, y_std, inv_lengthscale,
 * train_x, alpha and root_frag are read; disc_* are not).  Limits (DKG_ERR_UNSUPPORTED beyond them): m = 2 or 3,
 * d <= DKG_MAX_DIM, n <= 1024, and the three below. */
#define DKG_HVKG_MAX_FANTASIES 64
#define DKG_HVKG_MAX_PARETO 32
#define DKG_HVKG_MAX_RESTARTS 4096
/* Bytes of the host plan (caller memory, kept unchanged while the plan is in use). */
size_t dkg_hvkg_plan_bytes(void);
/* Bytes of device scratch a plan for up to max_B restarts needs; 0 for sizes dkg_hvkg_init refuses. */
size_t dkg_hvkg_workspace(int m, int d, int num_fantasies, int num_pareto, int max_B);
/* A plan: everything an evaluation needs besides the one-shot points.
 *   outs         : host array of m structs, copied into host_plan and uploaded into the workspace on `stream`
 *   ref_point    : host [m], untransformed output space
 *   base_samples : host [num_fantasies][m], the z_f,i (not read, nullable, when mask is 0)
 *   mask         : bit i set = output i is evaluated at the candidate (BoTorch's X_evaluation_mask for q = 1).
 *                  0 selects the value function: no candidate row, num_fantasies must be 1 and the input of
 *                  dkg_hvkg_forward is X [B][num_pareto][d]
 *   current_value, cost: the scalars of acq above (0 and 1 when absent); cost > 0
 *   workspace    : device scratch of dkg_hvkg_workspace() bytes, owned by the plan while it is in use
 * DKG_ERR_ARG for NULL pointers, sizes < 1, a mask with bits at or above m, an empty mask with num_fantasies != 1,
 * a cost that is not positive, n < 1 or an unknown kernel id; DKG_ERR_UNSUPPORTED beyond the limits or for m not in
 * {2, 3}; DKG_ERR_WORKSPACE for a short workspace.  The arguments are checked before any HIP call; nothing
 * synchronises. */
int dkg_hvkg_init(const dkg_output* outs, int m, int d, const double* ref_point, int num_fantasies, int num_pareto,
                  const double* base_samples, unsigned mask, double current_value, double cost, int max_B,
                  void* workspace, size_t workspace_bytes, void* host_plan, void* stream);
/* acq[b] for B <= max_B one-shot points x_full (device [B][1 + Nf Np][d]; value-function mode [B][Np][d]) and, when
 * dacq_dx is not NULL, the gradient in every entry of x_full (device, the shape of x_full), by a hand-written
 * adjoint.  y_out (nullable): device [B][Nf][Np][m], the fantasised means Y.  Four launches (three in
 * value-function mode) whatever B, Nf, Np and m are: the candidate's K^-1 k(X, x) and sigma~ per (restart, output
 * in E); one wave per fantasy point for Y and dY/dx'; one wave per (restart, fantasy) for HV_f and dHV_f/dY; one
 * workgroup per restart for acq and the gradient, which costs one more product with K^-1 per (restart, output in
 * E), not per fantasy point.  Stream ordered, nothing synchronises, no atomics, every sum in a fixed order: two
 * calls give the same bits, and a restart's value and gradient have the same bits whatever B is and whichever row
 * holds it.  DKG_ERR_ARG for NULL pointers, an uninitialised plan or B outside [1, max_B], checked before any HIP
 * call. */
int dkg_hvkg_forward(const void* host_plan, const double* x_full, int B, double* acq, double* dacq_dx, double* y_out,
                     void* stream);
/* The hypervolume stage alone (the kernel dkg_hvkg_forward launches): hv[s] = the volume of the union of the boxes
 * [ref, Y[s][p]] over the num_pareto <= DKG_HVKG_MAX_PARETO points of set s, and, when dhv is not NULL,
 * dhv[s][p][i] = d hv[s] / d Y[s][p][i] with the conventions above.  Y, hv, dhv: device; ref_point: host [m].
 * m = 2: a sort and one sweep; m = 3: slabs on the last objective over 2-d sweeps; every term of the value is
 * positive.  DKG_ERR_UNSUPPORTED for m not in {2, 3} or num_pareto beyond the limit. */
int dkg_hypervolume(const double* Y, int S, int num_pareto, int m, const double* ref_point, double* hv, double* dhv,
                    void* stream);

/* ---- Dominated-space boxes and the hypervolume of large fronts, m <= 3 (dkg_boxes.hip) --------------------------
 * The region a point set dominates above a reference point, cut into disjoint boxes (what BoTorch's
 * DominatedPartitioning gives the reference's JES, jes_sample_pareto.py:235-347), and the sum of their volumes (the
 * hypervolume of the BO metrics, botorch_hypervolume.py).  All objectives are maximised; everything is fp64.
 * DESIGN.md 8g.  The specification:
 *   A point qualifies if it is strictly above ref in every objective; other points (NaN and padding rows included)
 *   contribute nothing.  Boxes are (lo, hi].  Every corner coordinate is a copy of an input value or of ref: no
 *   arithmetic makes a corner.  Boxes with an empty interior are not emitted.
 *   m = 1: the one box (ref, max].
 *   m = 2: the staircase (a_1, b_1) ... (a_k, b_k) of the non-dominated qualifying points (repeated points once), a
 *     ascending and b descending; box j is (a_{j-1}, a_j] x (ref_1, b_j] with a_0 = ref_0, emitted by ascending j.
 *   m = 3: take the qualifying points in level order: y_2 descending, then index ascending.  For point p in that
 *     order let s_1 ... s_t be the 2-d staircase in (y_0, y_1) of the points before it, y_0 ascending: the earlier
 *     points not weakly dominated in (y_0, y_1) by another earlier point; of equal pairs the first in level order
 *     stays.  The region only p adds, (ref_0, p_0] x (ref_1, p_1] less what the earlier points dominate, is cut
 *     into vertical strips: strip i is (s_{i-1,0}, min(s_{i,0}, p_0)] x (s_{i,1}, p_1] with s_{0,0} = ref_0, and
 *     the last strip is (s_{t,0}, p_0] x (ref_1, p_1].  Each strip with an interior gives the box
 *     strip x (ref_2, p_2].  Boxes are emitted in level order of p, and within p by ascending strip.
 *   Count bound: a point emits at most (staircase points it removes + 1) boxes, so K points give at most 2K - 1
 *     boxes at m = 3, at most K at m = 2 and 1 at m = 1.
 *   hv = the sum over the boxes of prod(hi - lo); every term is a product of non-negative differences, so nothing
 *     cancels.
 * Rounding of dkg_hypervolume_front: |hv - exact| <= (L + 4) 2^-52 exact with L = K + ceil(K / 1024) + 10, the
 * longest chain of additions a term passes through: a point's strips are summed in its lane in walk order, each by
 * one fma (at most K strips: K - 1 additions after the first, which adds to zero); the per-point volumes are summed
 * by 1024 lanes over every 1024th (ceil(K / 1024) - 1 additions after the first) and then by a binary tree (10).
 * That is K + ceil(K / 1024) + 8; the term itself rounds five times (two differences into the fma, the fma, the
 * last difference and its product), one of them the first link of the chain and four the "+ 4"; the other 2 of L
 * cover the second-order terms.  L <= K + 26 <= K + 64.
 * Samples with fewer points are padded by the caller with rows that do not qualify (ref itself will do).  Results
 * depend on a sample's qualifying points only: two calls give the same bits, a set's result does not depend on S or
 * on its row, and appended rows that do not qualify change no bit.  Stream ordered, nothing synchronises, no
 * atomics, no workgroup waits on another.  Limits (DKG_ERR_UNSUPPORTED beyond them): m <= 3, S <= 65535, K <=
 * DKG_BOXES_MAX_POINTS for the boxes and DKG_HV_FRONT_MAX_POINTS for the volume, J <= DKG_JES_MAX_BOXES. */
#define DKG_BOXES_MAX_POINTS 2048      /* 2K - 1 <= DKG_JES_MAX_BOXES */
#define DKG_HV_FRONT_MAX_POINTS 16384  /* dkg_pareto_rank's cap */
/* Bytes of device scratch for S sets of K points; 0 for sizes the call refuses. */
size_t dkg_dominated_boxes_workspace(int S, int K, int m);
/* bounds[s][0][j] / bounds[s][1][j]: the lower / upper corner of box j < count[s] of set s; rows count[s] ... J - 1
 * are [0, 0] boxes, as the reference pads.  Y: device [S][K][m]; ref_point: host [m] (JES passes -1e10 everywhere);
 * bounds: device [S][2][J][m]; count: device [S].  J must hold the count bound (1 / K / 2K - 1 at m = 1 / 2 / 3).
 * Two launches.  DKG_ERR_ARG for NULL pointers, sizes < 1 or J below the count bound; DKG_ERR_UNSUPPORTED beyond the
 * limits; DKG_ERR_WORKSPACE for a short workspace; all checked before any HIP call. */
int dkg_dominated_boxes(const double* Y, int S, int K, int m, const double* ref_point, int J, double* bounds,
                        int* count, void* work, size_t work_bytes, void* stream);
size_t dkg_hypervolume_front_workspace(int S, int K, int m);
/* hv[s] (device [S]) = the hypervolume of set s above ref_point.  Three launches.  Errors as above. */
int dkg_hypervolume_front(const double* Y, int S, int K, int m, const double* ref_point, double* hv, void* work,
                          size_t work_bytes, void* stream);

/* Bytes of scratch dkg_forward needs for (m outputs, N points, B candidates, S weights). */
size_t dkg_forward_workspace(const dkg_output* outs, int m, int N, int B, int S);

/* Discrete KG for B candidates: kg[b] = mean_j KG(xnew_b, w_j).
 * Replaces DiscreteKnowledgeGradient.forward (discretekg.py:131-159) with
 * target = -1 -> calculate_discrete_kg (:162-235, coupled evaluation),
 * target = t  -> calculate_discrete_kg_conditioning_on_single_output (:238-338).
 *   outs    : m output states (host array of structs holding device pointers)
 *   disc    : device [N x d] discretisation (x_discretisation)
 *   xnew    : device [B x d] candidates
 *   weights : device [S x m] linear scalarisation weights
 *   kg      : device [B] output
 *   kg_pairs: device [B x S] per-(candidate, scalarisation) KG, nullable
 *   workspace: device scratch of dkg_forward_workspace() bytes */
int dkg_forward(const dkg_output* outs, int m, int d, const double* disc, int N, const double* xnew,
                int B, const double* weights, int S, int target, double* kg, double* kg_pairs,
                void* workspace, size_t workspace_bytes, void* stream);

/* As dkg_forward, but records HIP events around each of the three kernels on
 * `stream`, synchronises, and returns their durations in ms:
 * stage_ms[0] = cross (K(x,X) R), [1] = posterior covariance GEMM, [2] = envelope + expectation. */
int dkg_forward_timed(const dkg_output* outs, int m, int d, const double* disc, int N, const double* xnew,
                      int B, const double* weights, int S, int target, double* kg, double* kg_pairs,
                      void* workspace, size_t workspace_bytes, void* stream, float* stage_ms);

/* ---- Plan API (the fast path) -------------------------------------------
 * A plan is everything a forward needs besides the candidates: the m output
 * states, the discretisation, the weights, the target and the workspace carve
 * for up to max_B candidates.  dkg_plan_init validates it, writes it to
 * `host_plan` (caller memory of dkg_plan_bytes() bytes, kept unchanged while
 * the plan is in use) and copies it to `dev_plan` (device memory of the same
 * size) on `stream`.  dkg_plan_forward then launches the three kernels with a
 * pointer to the device copy (no per-call host-to-device traffic).  The
 * disc/weights/workspace buffers must outlive the plan.  The weights are
 * frozen at dkg_plan_init: the staged envelope's intercept cache and each
 * scalarisation's top intercept (Plan::icpt / itop) are derived from them
 * there, so a caller that changes its weights builds a new plan (the Python
 * host passes the plan a copy of its weights and rebuilds on a change). */
/* Plan flags: DKG_PLAN_GRAD adds the gradient buffers (dkg_plan_forward_grad). */
#define DKG_PLAN_GRAD 1
/* DKG_PLAN_FORCE_WALK (test hook): the envelope stage takes its list-overflow
 * path (gift wrap over all lines) for every pair; same results, slower. */
#define DKG_PLAN_FORCE_WALK 2
/* DKG_PLAN_F32: the two contractions of the forward (Q_X = K(x,X) R and
 * Q_X . Q_D, BASELINE configs[4]'s "fp32 MFMA-bound stress") run in fp32 on
 * v_mfma_f32_16x16x4_f32 over fp32 copies of R and Q_D made at plan init; the
 * kernel evaluations, means, variances (fp64 sums of the fp32 Q_X squares),
 * the line build, envelope and expectation stay fp64.  Not a reference mode
 * (the reference is fp64 throughout, constants.py:8): results agree with the
 * fp64 plan to ~1e-3 relative when the noise is >= 1e-3 of the outputscale.
 * Forward only (not combinable with DKG_PLAN_GRAD). */
#define DKG_PLAN_F32 4
/* DKG_PLAN_FUSED: dkg_plan_forward launches the forward as ONE kernel whose cross,
 * covariance and envelope workgroups hand the stages on through arrival counters
 * (dkg_fused.h), instead of the three stage kernels; fp64 plans whose lines fit the
 * staged envelope (N + 1 <= 1088).  Same bits either way.  Not the default: on
 * MI355X an in-launch hand-off costs about what the kernel boundary it replaces
 * does, and the early-dispatched consumers slow the producers. */
#define DKG_PLAN_FUSED 8
/* DKG_PLAN_NO_CHAIN (test hook): the streaming envelope (N + 1 > 2112 lines, or line data beyond LDS)
 * filters without its sample chain: the extremes from the streamed lines, the quickhull refinement and
 * the walks of the list-overflow path for every pair; same results, slower. */
#define DKG_PLAN_NO_CHAIN 16
/* DKG_PLAN_GRAD_GLOBAL_ROWS (with DKG_PLAN_GRAD only; DKG_ERR_ARG without it): where the gradient plan would be
 * refused because every output's Q_X row and its d rows of J do not fit in the envelope stage's LDS
 * ("gradient: ... exceed the envelope stage's LDS"), build a streaming plan whose envelope reads those rows
 * from the workspace instead ("global rows").  Every plan that is built without the flag is built the same,
 * bit for bit, with it; the other refusals are unchanged. */
#define DKG_PLAN_GRAD_GLOBAL_ROWS 32
/* DKG_PLAN_FORCE_GLOBAL_ROWS (test hook, with DKG_PLAN_GRAD only): the streaming global-rows envelope on any
 * shape; the bits of the plan's staged-rows streaming envelope. */
#define DKG_PLAN_FORCE_GLOBAL_ROWS 128
size_t dkg_plan_bytes(void);
size_t dkg_plan_workspace(const dkg_output* outs, int m, int d, int N, int max_B, int S, int flags);
int dkg_plan_init(const dkg_output* outs, int m, int d, const double* disc, int N, const double* weights, int S,
                  int target, int max_B, int flags, void* workspace, size_t workspace_bytes, void* host_plan,
                  void* dev_plan, void* stream);
/* Where a gradient plan of these outputs, N discretisation points, S scalarisations and `flags` (with
 * DKG_PLAN_GRAD) takes the candidates' Q_X and J rows from: 0 staged in LDS, 1 global rows
 * (DKG_PLAN_GRAD_GLOBAL_ROWS where the staged rows do not fit, DKG_PLAN_FORCE_GLOBAL_ROWS always), or the
 * status dkg_plan_init would refuse the shape or the flags with, negated (-DKG_ERR_*; dkg_last_error set).  Host
 * arithmetic only: no device call, and the outputs' pointers are checked for NULL, never followed. */
int dkg_plan_grad_rows(const dkg_output* outs, int m, int d, int N, int S, int flags);
/* 1 if the plan's gradient envelope reads global rows, 0 if it stages them (or the plan has no gradient). */
int dkg_plan_grad_rows_of(const void* host_plan);
/* A plan of T targets: `targets` (host, [T]) holds 1 <= T <= m + 1 distinct entries in [-1, m), -1 = all
 * outputs observed; anything else is DKG_ERR_ARG.  The cross and covariance stages do not depend on the
 * target, so every call on the plan runs them once and the envelope once per (target, candidate): row
 * (tau, b) of a result has exactly the bits a single-target plan of targets[tau] writes for candidate b.
 *   dkg_plan_forward             kg[tau*B + b], kg_pairs[tau][b][S]
 *   dkg_plan_hull_sizes          out[tau][b][S]
 *   dkg_plan_forward_grad        kg[tau*B + b], dkg_dx[tau][b][d]
 *   dkg_plan_forward_grad_hostx  the same (B * d <= DKG_XARG_MAX: the candidates are shared); out_host holds
 *                                T * B * (d + 1) doubles [kg | dkg_dx]
 *   dkg_plan_forward_timed, dkg_plan_time_stage   kg holds T * B doubles
 *   dkg_plan_lines               the lines of targets[0]
 * DKG_PLAN_F32 plans are accepted (forward only, as with one target).  DKG_PLAN_FUSED with T > 1 and
 * dkg_plan_forward_batches / dkg_plan_time_stage_batches on a plan of T > 1 return DKG_ERR_UNSUPPORTED.
 * dkg_plan_init is the T = 1 case and dkg_plan_workspace_targets(T = 1) equals dkg_plan_workspace; the
 * workspace grows with T by the per-item result buffers only (0 for T outside 1..m + 1). */
size_t dkg_plan_workspace_targets(const dkg_output* outs, int m, int d, int N, int max_B, int S, int T, int flags);
int dkg_plan_init_targets(const dkg_output* outs, int m, int d, const double* disc, int N, const double* weights,
                          int S, const int* targets, int T, int max_B, int flags, void* workspace,
                          size_t workspace_bytes, void* host_plan, void* dev_plan, void* stream);
/* kg[b] (and kg_pairs[b x S], nullable) for B <= max_B candidates xnew (device, B x d);
 * same result as dkg_forward with the plan's arguments.  One fused launch for a plan built
 * with DKG_PLAN_FUSED (a call given kg_pairs runs the three stages). */
int dkg_plan_forward(const void* host_plan, const void* dev_plan, const double* xnew, int B, double* kg,
                     double* kg_pairs, void* stream);
/* nbatch forward batches of B candidates in one launch per stage: xnew is device [nbatch][B][d], kg
 * device [nbatch][B], nbatch * B <= max_B.  kg[k][b] is bit-for-bit what dkg_plan_forward of batch k
 * alone writes (every candidate's result depends on its own x only, and the covariance blocks are the
 * ones a B-candidate forward takes), so this is nbatch dkg_plan_forward calls with 3 launches instead
 * of 3 * nbatch: the throughput form of the reference's per-batch forward (discretekg.py:131-159) when
 * a caller has several batches ready (bench.py's steps).  Always the three stage kernels (a fused plan
 * included). */
int dkg_plan_forward_batches(const void* host_plan, const void* dev_plan, const double* xnew, int B, int nbatch,
                             double* kg, void* stream);
/* As dkg_plan_forward with per-kernel HIP-event timings (synchronises): stage_ms[3]. */
int dkg_plan_forward_timed(const void* host_plan, const void* dev_plan, const double* xnew, int B, double* kg,
                           double* kg_pairs, void* stream, float* stage_ms);
/* Value and gradient (plan built with DKG_PLAN_GRAD): kg[b] as dkg_plan_forward
 * and dkg_dx[b*d + j] = d kg[b] / d xnew[b*d + j] (device, B x d).  Replaces
 * the autograd backward of DiscreteKnowledgeGradient.forward (discretekg.py:
 * 131-159; exercised by test_discretekg.py:110-135 and by optimize_acqf,
 * acquisition_optimisation_strategy.py:217-224, 259-266).  With the upper
 * envelope fixed (envelope theorem), per scalarisation
 *   dKG/dx = sum_{envelope lines e} [ (phi(c_L) - phi(c_R)) db_e/dx
 *                                      + (Phi(c_R) - Phi(c_L)) [e = 0] da_0/dx ]
 *            - [line 0 attains max a] da_0/dx,
 * where only the candidate's own line 0 intercept and the slopes depend on x. */
int dkg_plan_forward_grad(const void* host_plan, const void* dev_plan, const double* xnew, int B, double* kg,
                          double* dkg_dx, void* stream);
/* Largest B * d of dkg_plan_forward_grad_hostx. */
#define DKG_XARG_MAX 64
/* dkg_plan_forward_grad for candidates given in HOST memory (x_host[b*d + j], B * d <= DKG_XARG_MAX):
 * the candidates travel inside the first kernel's arguments instead of a host-to-device copy
 * (one copy fewer on the optimize_acqf L-BFGS-B path, batch_limit = 1: bo_loop.py:127-129), and
 * that kernel leaves them in x_dev (device, B x d) for the later kernels.  x_host may be reused as
 * soon as this returns.  out_host (nullable): pinned host memory of B * (d + 1) doubles that
 * receives [kg | dkg_dx], written by the envelope kernel itself (no copy after it); with out_host the
 * call synchronises the stream and returns with the results in place (one host call per L-BFGS-B
 * evaluation).  Same results, bit for bit, as dkg_plan_forward_grad on x_dev. */
int dkg_plan_forward_grad_hostx(const void* host_plan, const void* dev_plan, const double* x_host, double* x_dev,
                                int B, double* kg, double* dkg_dx, double* out_host, void* stream);
/* Envelope sizes of the plan's last forward that was given kg_pairs (same B):
 * out[b*S + j] = the number of upper-envelope lines of pair (b, j), i.e. the
 * len(indices) of calculate_epigraph_indices (discretekg.py:341-412); 1 when the
 * pair short-circuits (all |b| < 1e-9, :363-367).  Device int[B x S]; stream
 * ordered.  Diagnostics (log the envelope-size histogram). */
int dkg_plan_hull_sizes(const void* host_plan, int* out, int B, void* stream);
/* Hand-off status of the plan's fused launches (DKG_PLAN_FUSED) (stream ordered, synchronises):
 * *err = the OR of the bits of every in-launch wait that gave up since the last
 * reset (1 covariance on cross, 2 envelope on covariance; 0 = every wait matched;
 * a wait that gives up lets its workgroup go on, so the launch ends and its
 * results are not to be used).  reset != 0: clear the bits and re-zero the arrival
 * counters.  Returns DKG_OK (or a HIP error). */
int dkg_plan_status(const void* host_plan, int* err, int reset, void* stream);
/* 1 if dkg_plan_forward runs the plan's forward as the fused single launch, 0 if as the three stage kernels. */
int dkg_plan_fused(const void* host_plan);
/* Benchmark helper: average HIP-event duration (ms) of `reps` back-to-back
 * launches of one stage (0 cross_root, 1 posterior_cov, 2 envelope, 3 the
 * whole forward as dkg_plan_forward launches it) on
 * `stream`, after one full forward that primes its inputs; a final full
 * forward leaves kg / kg_pairs valid.  Synchronises. */
int dkg_plan_time_stage(const void* host_plan, const void* dev_plan, const double* xnew, int B, double* kg,
                        double* kg_pairs, void* stream, int stage, int reps, float* avg_ms);
/* As dkg_plan_time_stage for the launches of dkg_plan_forward_batches (nbatch batches of B candidates,
 * xnew [nbatch][B][d], kg [nbatch][B]): the stage as that entry launches it (stage 3: its three kernels). */
int dkg_plan_time_stage_batches(const void* host_plan, const void* dev_plan, const double* xnew, int B, int nbatch,
                                double* kg, void* stream, int stage, int reps, float* avg_ms);

/* Envelope stage alone: for P independent sets of L lines a_k + b_k z
 * (device, row-major [P][L]) kg[p] = E[max_k (a_k + b_k Z)] - max_k a_k, Z ~ N(0,1),
 * and optionally the number of upper-envelope lines n_hull[p] (nullable).
 * Replaces calculate_epigraph_indices + calculate_expected_value_of_piecewise_
 * linear_function + the baseline subtraction (discretekg.py:225-233, 341-452);
 * L = 0 -> DKG_ERR_NO_LINES (the reference's ValueError, :466-470).  Any L. */
int dkg_lines_kg(const double* intercepts, const double* slopes, int P, int L, double* kg, int* n_hull,
                 void* stream);

/* The reference's epigraph, exactly: calculate_epigraph_indices
 * (discretekg.py:341-412) for P sets of L lines (device, [P][L]).
 *   indices      : device int64 [P][cap], the envelope's line indices left to right
 *   intersections: device [P][cap - 1], the breakpoints between them (nullable if cap == 1)
 *   count        : device int [P], the envelope size m (entries beyond cap are not written)
 * Same walk as the reference: lines ordered by slope ascending then intercept
 * descending, each step to the later line of a different slope whose
 * intersection -(a_i - a_j)/(b_i - b_j) is first, ties to the first in that
 * order; the intersections are the same IEEE values.  Every |b| < 1e-9 -> the
 * first line of maximal intercept, no intersections (:363-367).  Among exact
 * duplicate lines (equal slope and intercept) the lowest index is returned
 * (the reference's first sort is not stable for more than 16 lines on CPU
 * torch; any duplicate is an equal line).  L = 0 -> DKG_ERR_NO_LINES. */
int dkg_epigraph(const double* intercepts, const double* slopes, int P, int L, int cap, long long* indices,
                 double* intersections, int* count, void* stream);

/* calculate_expected_value_of_piecewise_linear_function (discretekg.py:415-452)
 * for P functions of m pieces: out[p] = sum_j a_j (Phi(c_j) - Phi(c_{j-1}))
 * - b_j (phi(c_j) - phi(c_{j-1})), c_0 = -inf, c_m = +inf, boundaries [P][m-1]
 * (device; nullable when m == 1).  m = 0 -> DKG_ERR_NO_LINES. */
int dkg_pwl_expectation(const double* intercepts, const double* slopes, const double* boundaries, int P, int m,
                        double* out, void* stream);

/* The lines the plan's envelope stage builds for candidates xnew (device,
 * B x d): intercepts / slopes device [B][S][N + 1], line 0 the candidate
 * itself (discretekg.py:182-223 full, :300-321 decoupled), bit-identical to
 * the envelope's.  Runs the cross and covariance stages (an F32 plan: its fp32 contractions). */
int dkg_plan_lines(const void* host_plan, const void* dev_plan, const double* xnew, int B, double* intercepts,
                   double* slopes, void* stream);

/* Debug: per-workgroup phase stamps of the three forward kernels, written when
 * the env var DKG_DEBUG_STAMPS=1 at plan creation: [3][1024][8] words (slot 0
 * s_memrealtime at start, 1..6 s_memtime at phase boundaries, 7 s_memrealtime
 * at end); n words are copied.  DKG_DEBUG_STAMPS=3: the same buffer as [12288][2]
 * words, written by the envelope launch alone, per workgroup id: s_memrealtime at
 * start, then s_memrealtime at end in bits 59:0 with the XCD the workgroup ran on
 * (HW_REG_XCC_ID) in bits 63:60. */
int dkg_debug_read_kstamps(unsigned long long* host, int n);

/* Debug/self-test of the register-only wave butterflies the kernels use
 * (DPP row ops + ds_bpermute for the 16/32 steps): in[64] -> out[512]; out[64 s + l] is the
 * partner value lane l receives at butterfly step s (0..5), out[384 + l] the
 * wave sum and out[448 + l] the wave max seen by lane l. */
int dkg_debug_wave_ops(const double* in, double* out, void* stream);

/* Debug/self-test: C[16x16] = A[16x4] B[4x16] (row-major, device) with one
 * v_mfma_f64_16x16x4_f64 using the operand/result lane maps the kernels assume. */
int dkg_debug_mfma_f64(const double* a, const double* b, double* c, void* stream);

/* The opt-in fp64 covariance block kernels for the launches that would take them (bits below; tests and A/B
 * measurements; initially from the environment variables DKG_COV_BLK / DKG_COV_REC2 / DKG_COV_REG).  Every one
 * gives the bits of the default kernels.  Returns the previous mask; a mask < 0 only reads it.
 * Process-wide: call it with no forward in flight. */
#define DKG_COV_ENABLE_BLK 1  /* 64 x 32 LDS-staged blocks, three workgroups per CU */
#define DKG_COV_ENABLE_REC2 2 /* m = 2, d <= 2: both outputs' whole records from one 8-wave workgroup per CU */
#define DKG_COV_ENABLE_REG 4  /* register-operand blocks, any m, one 8-wave workgroup per CU */
int dkg_debug_cov_kernels(int mask);

/* The cross stage's one-launch kernel with K(x, X) kept in LDS (cross_tall_kernel; fp64 plans, every output's
 * n_pad <= 256).  mode -1: the default dispatch (launches of at least 512 candidates, which would otherwise fill
 * K(x, X) with a kernel of its own), 0: never, 1: every eligible shape whatever the candidate count (tests and
 * A/B measurements; initially from the environment variable DKG_CROSS_TALL).  Same bits either way.  Returns the
 * previous mode; any other value of mode is an error (returns -2, dkg_last_error) and changes nothing.  The mode is
 * read when a launch is issued: graphs captured earlier keep the kernels they were captured with. */
int dkg_debug_cross_tall(int mode);
/* Launches issued (or captured) through the one-launch cross kernel since the library was loaded. */
long long dkg_debug_cross_tall_launches(void);
/* 1 when a forward launch over B candidates of a plan with widest padded n `max_n_pad` (a multiple of 16), input
 * dimension d and fp32 contractions or not (f32) takes the one-launch cross kernel under the current mode, else 0;
 * -2 on bad arguments.  Host only: no device is touched. */
int dkg_debug_cross_tall_eligible(int max_n_pad, int d, int B, int f32);

/* The fp32 Q_X = K(x, X) R of output `output` (Plan::q32) as the last dkg_plan_lines or forward of B candidates
 * on an initialised DKG_PLAN_F32 plan left it: copied to the host and unpacked from the quad-packed layout into
 * host_out [n_pad16(B)][n_pad(output)] row-major (host memory; the padding rows and columns included).  No kernel
 * is launched; `stream` (the plan's) is synchronised.  DKG_ERR_UNSUPPORTED for an fp64 plan, DKG_ERR_ARG for
 * NULL pointers, an output outside [0, m) or B outside [1, max_B]. */
int dkg_debug_plan_qx32(const void* host_plan, int output, int B, float* host_out, void* stream);

/* Which fp32 kernels the cross and covariance stages of a DKG_PLAN_F32 plan launch for a shape, by the launcher's
 * own predicates: widest padded n `max_n_pad` (a multiple of 16), input dimension d, N discretisation points, m
 * outputs, B candidates in the launch, and geom_B the batch size the block shapes are chosen for (0: B; see
 * dkg_plan_forward_batches).  The plan is taken to be sized for the launch (max_B >= B).
 * out = {cross stage: 0 cross_root_plan_kernel<DM, float>, 1 cross_big32_kernel;
 *        covariance stage: 0 posterior_cov_kernel<DM, float>, 1 posterior_cov_big32_kernel<DM>;
 *        DM, the dimension bucket (2, 4, 8 or 16);
 *        the covariance launch's column (line) blocks, row (candidate) blocks, and the 64 x 64 blocks' order
 *        (-1 for the narrow kernel's 32 x 32 blocks)}.
 * The environment variables DKG_CROSS_BIG / DKG_COV_BIG / DKG_COV_BIG32 / DKG_COV_ORDER count as in a launch.
 * Returns 0, or -2 on bad arguments (dkg_last_error).  Host only: no device is touched. */
int dkg_debug_f32_dispatch(int max_n_pad, int d, int N, int m, int B, int geom_B, int out[6]);

/* Which kernels rank Q <= 2048 points when dkg_pareto_rank has a workspace (and every rank inside
 * dkg_pareto_nsga2).  mode -1: the measured rule (the default), 0: never the wide path, 1: always the wide path
 * (tests and A/B measurements).  Same bits either way; Q > 2048 is always the wide path.  Returns the previous
 * mode; any other value of mode is an error (returns -2, dkg_last_error) and changes nothing.  Read when a call
 * issues its launches. */
int dkg_debug_pareto_wide(int mode);

/* Which envelope kernel an initialised plan launches (decided by the LDS arithmetic of dkg_plan_init):
 * out = {register slots per lane of the staged envelope (2, 8, 17 or 33; 0 when the plan streams its lines),
 * 1 if it streams them from global memory else 0, waves per workgroup, workgroups per candidate}.  Returns 0, or
 * -2 when host_plan or out is NULL (dkg_last_error).  Host only: no device is touched. */
int dkg_debug_plan_envelope(const void* host_plan, int out[4]);

/* The dynamic LDS of the envelope kernels for a shape (m outputs, N discretisation points, `waves` waves per
 * workgroup, S scalarisations, input dimension d, widest padded training size max_np) and a kernel mode (grad,
 * stream; grows: global rows, with grad and stream only): the offset in doubles of every region in layout order
 * (DESIGN.md 4.13 names them; -1: the mode has no such region), then the total in doubles.  The same arithmetic
 * the kernels carve their LDS by and dkg_plan_init sizes and refuses by.  Returns DKG_OK, or DKG_ERR_ARG for a
 * NULL pointer or a shape outside 1 <= m <= 8, 0 <= N <= 2^22, 1 <= waves <= 8, S >= 1 (S m <= 2^24),
 * 1 <= d <= 16, max_np a multiple of 16 in [16, 1024], or grows without grad and stream.  Host only. */
#define DKG_ENV_LDS_REGIONS 20
int dkg_debug_envelope_lds(int m, int N, int waves, int S, int d, int max_np, int grad, int stream, int grows,
                           int out[DKG_ENV_LDS_REGIONS + 1]);

/* Which (item, member) workgroup id L of an envelope launch over `nitems` items of `groups` workgroups each runs
 * (csrc/dkg_common.h xcd_deal; the launch has 8 * groups * ceil(nitems / 8) ids, ids L and L + 8 share an XCD):
 * the members of an item on consecutive ids of one XCD, the items of every aligned eight rotated over the launch
 * residues so that item b runs on residue (b + b / 8 + b / 64) mod 8.  Returns 1 and sets *item, *member for an id
 * that runs an item, 0 for a padding id (*item >= nitems then), -2 for a NULL pointer, nitems < 1, groups < 1, a
 * launch of 2^31 ids or more, or L outside the launch (dkg_last_error).  Host only: the arithmetic the kernels
 * run. */
int dkg_debug_envelope_deal(int L, int nitems, int groups, int* item, int* member);

/* ---- Launcher: captured forward graphs of several streams enqueued side by side from host threads.
 * A hipGraphLaunch costs ~1 us of host time per kernel node plus ~9 us; one thread launching every
 * stream's graphs in turn leaves the last stream idle for the others' launches.  The
 * launcher keeps `threads - 1` worker threads (the caller is thread 0); stream s's graphs
 * graphs[offs[s] .. offs[s+1]) (hipGraphExec_t) are launched in order on streams[s] (hipStream_t) by
 * thread s % threads.  dkg_launcher_graphs returns once every launch call has returned; concurrent
 * calls on one launcher are serialised (a launcher runs one launch set at a time).  Armed
 * workers spin (wake-up in ~1 us) for `seconds`; otherwise they sleep on a condition variable.
 * Host-side scheduling only (the reference has no counterpart: its forward is a Python loop,
 * discretekg.py:145-159); no kernel is launched that the caller did not capture. */
int dkg_launcher_create(int threads, void** launcher);
int dkg_launcher_arm(void* launcher, double seconds);
int dkg_launcher_graphs(void* launcher, int n_streams, void* const* streams, const int* offs,
                        void* const* graphs);
int dkg_launcher_destroy(void* launcher);

#ifdef __cplusplus
}
#endif
#endif /* DKG_AMD_DKG_H */
