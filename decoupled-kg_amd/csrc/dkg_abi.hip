// C ABI of the Discrete-KG library (include/dkg.h).  Host-side validation,
// workspace carving and kernel sequencing; no device work happens here.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

#include "dkg_kernels.h"

using namespace dkg;

namespace {

thread_local std::string g_err;
unsigned long long* g_kstamps_buf = nullptr;  // debug phase stamps (allocated on first use, kept)

}  // namespace

// dkg_kernels.h: the one error, status and rounding helper set of the host translation units
int dkg::failf(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

int dkg::hip_status(hipError_t e, const char* what) {
  return e == hipSuccess ? DKG_OK : failf(DKG_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

size_t dkg::up256(size_t x) { return (x + 255) & ~(size_t)255; }

namespace {

// The widest n_pad over the outputs (Plan::max_np).
int max_np_of(const dkg_output* outs, int m) {
  int np = 16;
  for (int i = 0; i < m; ++i) np = std::max(np, pad16(outs[i].n));
  return np;
}

// The forward workspace, walked once: each line is a section's Plan pointer, its bytes and (the `if` around it) its
// condition, in the order they lie.  Returns the total.  Given a workspace and its plan (zeroed, Plan::stream set) it
// also points the plan at each section it takes; a section that is not taken leaves its pointer null.  Without a
// plan it is the size query.
// T: the plan's targets (dkg_plan_init_targets).  The per-candidate result buffers hold one row per item
// (tau, b) at tau * Bp + b: `items` rows where a single-target plan has max(B, 1), T * Bp where it has Bp.
size_t carve_plan(const dkg_output* outs, int m, int N, int B, int S, int d, int flags, int T, void* ws = nullptr,
                  Plan* P = nullptr) {
  Plan unset;  // where the pointers go that no plan takes (never read)
  Plan& p = P ? *P : unset;
  Carve c;
  auto sec = [&](auto*& ptr, size_t bytes) {
    const size_t off = c.take(bytes);
    if (P) ptr = at<std::remove_reference_t<decltype(*ptr)>>(ws, off);
  };
  const size_t Bp = pad16(std::max(B, 1)), B1 = std::max(B, 1), N1 = std::max(N, 1), S1 = std::max(S, 1);
  const size_t items = (size_t)(T - 1) * Bp + B1;
  const bool grad = (flags & DKG_PLAN_GRAD) != 0, f32 = (flags & DKG_PLAN_F32) != 0;
  const bool fill = cross_kfill_launch(max_np_of(outs, m), B);  // the launch covers every output of the plan
  p.sync_bytes = sync_layout(m, std::max(B, 1)).bytes;
  sec(p.sync, p.sync_bytes);  // the fused forward's counter block, at offset 0 (zeroed by one memset)
  for (int i = 0; i < m; ++i) {
    const size_t np = pad16(outs[i].n);
    if (grad) sec(p.jq[i], (size_t)d * Bp * np * sizeof(double));
    if (grad) sec(p.gmu[i], (size_t)d * Bp * sizeof(double));
    if (grad) sec(p.qxrm[i], Bp * np * sizeof(double));
    if (grad) sec(p.qdrm[i], N1 * np * sizeof(double));
    sec(p.q[i], Bp * np * sizeof(double));
    if (fill) sec(p.kx[i], Bp * np * sizeof(double));
    if (f32) sec(p.q32[i], Bp * np * sizeof(float));
    if (f32) sec(p.root32[i], np * np * sizeof(float));
    if (f32) sec(p.disc32[i], (size_t)pad16(std::max(N, 1)) * np * sizeof(float));
    if (f32 && fill) sec(p.kx32[i], Bp * np * sizeof(float));
  }
  // contiguous blocks (the envelope stage addresses them from kernel-argument
  // base pointers): means and variances at the candidates [m][Bp]; the
  // covariance rows [B][N][rec] and mu_D [N][rec] as line records
  // (rec = cov_rec(m) doubles per line, outputs side by side)
  const size_t rec = (size_t)cov_rec(m);
  sec(p.mux_all, (size_t)m * Bp * sizeof(double));
  sec(p.var_all, (size_t)m * Bp * sizeof(double));
  sec(p.cov_all, rec * B1 * N1 * sizeof(double));
  sec(p.mu_all, rec * N1 * sizeof(double));
  for (int i = 0; i < m && P; ++i) {
    p.mux[i] = p.mux_all + (size_t)i * Bp;
    p.var[i] = p.var_all + (size_t)i * Bp;
  }
  int sw, split;
  envelope_geometry(std::max(S, 1), &sw, &split);
  // split > 1: every pair's KG (and, value+gradient, its dKG/dx) for the last workgroup's ordered sums
  const size_t ng = pair_groups(std::max(S, 1)), pcols = S1 + ng;  // pair values + group terms
  sec(p.wg_part, split > 1 ? items * pcols * sizeof(double) : 0);
  sec(p.wg_gpart, grad && split > 1 ? items * pcols * d * sizeof(double) : 0);
  sec(p.tickets, (size_t)T * Bp * (ng + 1) * sizeof(int));
  sec(p.dup, Bp * sizeof(int));
  sec(p.hull_pairs, items * S1 * sizeof(int));
  if (N + 1 <= 64 * 33) {
    // staged forward: intercepts_kernel's scratch (Plan::icpt) and its results (itop / itopk); each scalarisation's
    // top intercept serves the staged forward envelope (a gradient plan's forward included).  A streaming plan has
    // the bytes and no pointers.
    Plan& staged = P && !P->stream ? *P : unset;
    sec(staged.icpt, S1 * 64 * env_slots(N + 1) * sizeof(double));
    sec(staged.itop, S1 * sizeof(double));
    sec(staged.itopk, S1 * 2 * sizeof(int));
  }
  return c.total();
}

int check_outputs(const dkg_output* outs, int m, int d) {
  if (outs == nullptr) return failf(DKG_ERR_ARG, "outs is NULL");
  if (m < 1 || m > DKG_MAX_OUTPUTS)
    return failf(DKG_ERR_UNSUPPORTED, "m=%d outputs (supported 1..%d)", m, DKG_MAX_OUTPUTS);
  if (d < 1 || d > DKG_MAX_DIM) return failf(DKG_ERR_UNSUPPORTED, "d=%d (supported 1..%d)", d, DKG_MAX_DIM);
  for (int i = 0; i < m; ++i) {
    const dkg_output& o = outs[i];
    if (o.n < 1) return failf(DKG_ERR_ARG, "output %d: n=%d training points", i, o.n);
    if (pad16(o.n) > 1024) return failf(DKG_ERR_UNSUPPORTED, "output %d: n=%d > 1024 training points", i, o.n);
    if (cross_root_lds_bytes(pad16(o.n), d) > 160 * 1024)
      return failf(DKG_ERR_UNSUPPORTED, "output %d: n=%d, d=%d exceed the cross stage's LDS budget", i, o.n, d);
    if (o.kernel < DKG_MATERN12 || o.kernel > DKG_RBF)
      return failf(DKG_ERR_ARG, "output %d: kernel id %d", i, o.kernel);
    if (!o.inv_lengthscale || !o.train_x || !o.alpha || !o.root_frag)
      return failf(DKG_ERR_ARG, "output %d: missing device state pointer", i);
  }
  return DKG_OK;
}

// The targets of a plan (dkg_plan_init_targets): 1 <= T <= m + 1 distinct entries in [-1, m).
int check_targets(const int* targets, int T, int m) {
  if (!targets) return failf(DKG_ERR_ARG, "targets is NULL");
  if (T < 1 || T > m + 1 || T > DKG_MAX_OUTPUTS + 1)
    return failf(DKG_ERR_ARG, "T=%d targets (1..%d for %d outputs)", T, m + 1, m);
  for (int t = 0; t < T; ++t) {
    if (targets[t] < -1 || targets[t] >= m)
      return failf(DKG_ERR_ARG, "targets[%d]=%d out of range for %d outputs", t, targets[t], m);
    for (int u = 0; u < t; ++u)
      if (targets[u] == targets[t]) return failf(DKG_ERR_ARG, "targets[%d]=%d repeats targets[%d]", t, targets[t], u);
  }
  return DKG_OK;
}

// Where a gradient plan's envelope takes the candidate's q_i / J_i rows from: 0 staged in LDS, 1 global rows
// (envelope_rows_kernel, always streaming), or the refusal's status negated.  Without DKG_PLAN_GRAD_GLOBAL_ROWS /
// DKG_PLAN_FORCE_GLOBAL_ROWS this is the staged plan or its refusal; DKG_PLAN_GRAD_GLOBAL_ROWS changes the
// refusal alone.  Host arithmetic only (dkg_plan_grad_rows).
int grad_rows_rule(int m, int N, int sw, int S, int d, int max_np, int flags) {
  const bool fits = envelope_lds_bytes(m, N, sw, S, d, max_np, true, true, false) <= 160 * 1024;
  if (fits && !(flags & DKG_PLAN_FORCE_GLOBAL_ROWS)) return 0;
  if ((flags & (DKG_PLAN_GRAD_GLOBAL_ROWS | DKG_PLAN_FORCE_GLOBAL_ROWS)) &&
      envelope_lds_bytes(m, N, sw, S, d, max_np, true, true, true) <= 160 * 1024)
    return 1;
  return -failf(DKG_ERR_UNSUPPORTED, "gradient: m=%d outputs, n=%d, d=%d exceed the envelope stage's LDS", m, max_np,
                d);
}

// The flag checks of a plan, in build_plan's order.
int check_plan_flags(int flags) {
  if (flags & ~(DKG_PLAN_GRAD | DKG_PLAN_FORCE_WALK | DKG_PLAN_F32 | DKG_PLAN_FUSED | DKG_PLAN_NO_CHAIN |
                DKG_PLAN_GRAD_GLOBAL_ROWS | DKG_PLAN_FORCE_GLOBAL_ROWS))
    return failf(DKG_ERR_ARG, "unknown plan flags 0x%x", flags);
  if ((flags & (DKG_PLAN_GRAD_GLOBAL_ROWS | DKG_PLAN_FORCE_GLOBAL_ROWS)) && !(flags & DKG_PLAN_GRAD))
    return failf(DKG_ERR_ARG, "plan flags 0x%x: the global-rows flags need DKG_PLAN_GRAD", flags);
  if ((flags & DKG_PLAN_GRAD) && (flags & DKG_PLAN_F32))
    return failf(DKG_ERR_UNSUPPORTED, "the fp32 plan (DKG_PLAN_F32) is forward only; the gradient runs in fp64");
  return DKG_OK;
}

// What dkg_plan_init and dkg_plan_grad_rows check alike once their sizes are non-negative and S >= 1: the limit on
// N, and the envelope geometry (waves per workgroup, workgroups per candidate) with the weights' LDS.
int plan_geometry(int m, int N, int S, int d, int max_np, int* sw, int* split) {
  if (N > (1 << 22)) return failf(DKG_ERR_UNSUPPORTED, "N=%d discretisation points (supported <= %d)", N, 1 << 22);
  envelope_geometry(S, sw, split);
  if (envelope_lds_bytes(m, N, *sw, S, d, max_np, false, true, false) > 160 * 1024)
    return failf(DKG_ERR_UNSUPPORTED, "S=%d x m=%d weights exceed the envelope stage's LDS", S, m);
  return DKG_OK;
}

// targets == nullptr: the single-target plan of `target`.
int build_plan(const dkg_output* outs, int m, int d, const double* disc, int N, const double* weights, int S,
               int target, int max_B, void* workspace, size_t workspace_bytes, Plan* P, int flags = 0,
               const int* targets = nullptr, int T = 1) {
  int st = check_outputs(outs, m, d);
  if (st) return st;
  if (max_B < 0 || N < 0) return failf(DKG_ERR_ARG, "negative size B=%d N=%d", max_B, N);
  if (S < 1) return failf(DKG_ERR_ARG, "S=%d scalarisations", S);
  if (targets) {
    if ((st = check_targets(targets, T, m))) return st;
    target = targets[0];
    if (T > 1 && (flags & DKG_PLAN_FUSED))
      return failf(DKG_ERR_UNSUPPORTED, "DKG_PLAN_FUSED runs one target per plan; got T=%d targets", T);
  }
  if (target < -1 || target >= m)
    return failf(DKG_ERR_ARG, "target_output_ix=%d out of range for %d outputs", target, m);
  const int max_np = max_np_of(outs, m);
  int sw, split;
  if ((st = plan_geometry(m, N, S, d, max_np, &sw, &split))) return st;
  if (!weights || !workspace || (N > 0 && !disc)) return failf(DKG_ERR_ARG, "NULL data pointer");
  for (int i = 0; i < m; ++i)
    if (N > 0 && (!outs[i].disc_frag || !outs[i].disc_mean))
      return failf(DKG_ERR_ARG, "output %d: discretisation caches missing", i);
  if ((st = check_plan_flags(flags))) return st;
  const bool want_grad = (flags & DKG_PLAN_GRAD) != 0;
  const int grows = want_grad ? grad_rows_rule(m, N, sw, S, d, max_np, flags) : 0;
  if (grows < 0) return -grows;
  const size_t need = carve_plan(outs, m, N, max_B, S, d, flags, T);
  if (workspace_bytes < need)
    return failf(DKG_ERR_WORKSPACE, "workspace %zu bytes < required %zu", workspace_bytes, need);
  *P = Plan{};
  P->m = m;
  P->d = d;
  P->N = N;
  P->S = S;
  P->target = target;
  P->ntgt = T;
  for (int t = 0; t < T; ++t) {
    P->tlist[t] = targets ? targets[t] : target;
    P->tpack |= (unsigned long long)(P->tlist[t] + 1) << (4 * t);
  }
  P->max_B = max_B;
  P->max_np = max_np;
  P->sw = sw;
  P->split = split;
  P->disc = (N > 0) ? disc : static_cast<const double*>(workspace);  // always a readable address
  P->weights = weights;
  P->grad = want_grad ? 1 : 0;
  P->f32 = (flags & DKG_PLAN_F32) ? 1 : 0;
  // the envelope stages the line data in LDS when it fits and the lines fit the register slots; otherwise it
  // streams them from global memory (envelope_lds_bytes' last three arguments: grad, stream, grows)
  P->stream = N + 1 > 64 * 33 || envelope_lds_bytes(m, N, sw, S, d, max_np, false, false, false) > 160 * 1024 ||
              (want_grad && envelope_lds_bytes(m, N, sw, S, d, max_np, true, false, false) > 160 * 1024) ||
              (want_grad && (flags & DKG_PLAN_FORCE_GLOBAL_ROWS));
  P->grad_rows = grows;  // 1 only where stream is set: by the force flag, or because the staged rows do not fit
  P->bpad = pad16(std::max(max_B, 1));
  for (int i = 0; i < m; ++i) P->o[i] = outs[i];
  carve_plan(outs, m, N, max_B, S, d, flags, T, workspace, P);
  P->cov_stride = (int64_t)std::max(N, 1) * cov_rec(m);
  if (P->icpt) P->icpt_stride = 64 * env_slots(N + 1);
  static const char* denv = std::getenv("DKG_DEBUG_ENV_FLAGS");
  static const char* dcov = std::getenv("DKG_DEBUG_COV_FLAGS");
  P->debug_env = (denv ? std::atoi(denv) : 0) | ((flags & DKG_PLAN_FORCE_WALK) ? 1 : 0) |
                  ((flags & DKG_PLAN_NO_CHAIN) ? 8 : 0);
  P->debug_cov = dcov ? std::atoi(dcov) : 0;
  static const char* dst = std::getenv("DKG_DEBUG_STAMPS");
  P->debug_stamp = dst ? std::atoi(dst) : 0;
  // the fused one-launch forward (dkg_fused.h) only on explicit request (DKG_PLAN_FUSED): fp64, staged
  // lines, no test hooks; its bounded in-launch waits report give-ups through dkg_plan_status
  const bool split_stages = !(flags & DKG_PLAN_FUSED) || (flags & DKG_PLAN_FORCE_WALK);
  P->sync_err = reinterpret_cast<int*>(P->sync + sync_layout(m, std::max(max_B, 1)).err);
  P->fused = (!split_stages && !P->f32 && !P->stream && N >= 1 && N + 1 <= 64 * 17 && !P->debug_env && !P->debug_cov &&
              !DKG_ABLATIONS && fused_lds_bytes_host(*P) <= 160 * 1024)
                 ? 1
                 : 0;
  if (P->debug_stamp) {
    if (!g_kstamps_buf &&
        hip_status(hipMalloc(&g_kstamps_buf, sizeof(unsigned long long) * 3 * KST_WG * 8), "hipMalloc(stamps)"))
      return DKG_ERR_HIP;
    P->kstamps = g_kstamps_buf;
  }
  return DKG_OK;
}

// The candidate count of a plan's forward: DKG_OK to run, -1 where B == 0 leaves nothing to do (the entry returns
// DKG_OK), else the refusal.
int check_batch(const Plan& h, int B) {
  if (B < 0) return failf(DKG_ERR_ARG, "negative B=%d", B);
  if (B == 0) return -1;
  if (B > h.max_B) return failf(DKG_ERR_ARG, "B=%d candidates > plan capacity %d", B, h.max_B);
  return DKG_OK;
}

int run_forward(const Plan& h, const Plan* dev, const double* xnew, int B, double* kg, double* kg_pairs,
                hipStream_t stream, float* stage_ms) {
  if (int st = check_batch(h, B)) return std::max(st, 0);
  if (!xnew || !kg) return failf(DKG_ERR_ARG, "NULL data pointer");
  hipEvent_t ev[4];
  int st;
  if (stage_ms)
    for (int k = 0; k < 4; ++k)
      if ((st = hip_status(hipEventCreate(&ev[k]), "hipEventCreate"))) return st;
  if ((st = hip_status(stage_ms ? launch_forward(h, dev, xnew, B, kg, kg_pairs, stream, ev)
                                : launch_forward_auto(h, dev, xnew, B, kg, kg_pairs, stream),
                       "forward")))
    return st;
  if (stage_ms) {
    if ((st = hip_status(hipEventSynchronize(ev[3]), "hipEventSynchronize"))) return st;
    for (int k = 0; k < 3; ++k) (void)hipEventElapsedTime(&stage_ms[k], ev[k], ev[k + 1]);
    for (int k = 0; k < 4; ++k) (void)hipEventDestroy(ev[k]);
  }
  return DKG_OK;
}

size_t plan_slot_bytes() { return up256(sizeof(Plan)); }

// mu_D of every output into the plan's line records [N][cov_rec(m)] (stream
// ordered); the padding components (m < cov_rec(m)) of mu_D and of every
// covariance row are zeroed here once (the covariance stage writes components
// < m only), so they enter the line build as 0 with a zero weight.
int copy_disc_means(const Plan& P, hipStream_t s) {
  if (int st = hip_status(hipMemsetAsync(P.sync, 0, P.sync_bytes, s), "hipMemsetAsync(sync)")) return st;
  const int rec = cov_rec(P.m);
  if (rec > P.m && P.N > 0) {
    const size_t rows = (size_t)std::max(P.max_B, 1) * P.N;
    int st = hip_status(hipMemsetAsync(P.mu_all, 0, sizeof(double) * rec * P.N, s), "hipMemsetAsync(mu_D)");
    if (!st) st = hip_status(hipMemsetAsync(P.cov_all, 0, sizeof(double) * rec * rows, s), "hipMemsetAsync(cov)");
    if (st) return st;
  }
  for (int i = 0; i < P.m && P.f32; ++i) {
    // F32: fp32 copies of R^T and Q_D for the fp32 contractions
    int st = hip_status(launch_frag_to_f32(P.o[i].root_frag, P.o[i].n, P.o[i].n, P.root32[i], s), "frag_to_f32(R)");
    if (st) return st;
    if (P.N > 0 &&
        (st = hip_status(launch_frag_to_f32(P.o[i].disc_frag, P.N, P.o[i].n, P.disc32[i], s), "frag_to_f32(Q_D)")))
      return st;
  }
  for (int i = 0; i < P.m && P.N > 0; ++i) {
    int st = hip_status(hipMemcpy2DAsync(P.mu_all + i, sizeof(double) * rec, P.o[i].disc_mean, sizeof(double),
                                         sizeof(double), P.N, hipMemcpyDeviceToDevice, s), "hipMemcpy2DAsync(mu_D)");
    if (st) return st;
    // GRAD: row-major Q_D for the envelope's per-line row gathers
    if (P.grad && (st = hip_status(launch_unpack_rows(P.o[i].disc_frag, P.N, P.o[i].n, P.qdrm[i], s), "unpack_rows")))
      return st;
  }
  if (P.icpt) return hip_status(launch_intercepts(P, s), "intercepts");
  return DKG_OK;
}

// The tail of dkg_plan_init / dkg_plan_init_targets after build_plan (st: its status): the plan's constant device
// data, then its device copy.
int upload_plan(int st, const Plan* h, void* dev_plan, hipStream_t s) {
  if (st || (st = copy_disc_means(*h, s))) return st;
  return hip_status(hipMemcpyAsync(dev_plan, h, sizeof(Plan), hipMemcpyHostToDevice, s), "hipMemcpyAsync");
}

// One-shot path: plan built on the host per call, its device copy placed in
// the workspace tail (one small host-to-device copy per call).
int forward_oneshot(const dkg_output* outs, int m, int d, const double* disc, int N, const double* xnew, int B,
                    const double* weights, int S, int target, double* kg, double* kg_pairs, void* workspace,
                    size_t workspace_bytes, hipStream_t stream, float* stage_ms) {
  if (B == 0) return check_outputs(outs, m, d);
  const size_t slot = plan_slot_bytes() + 256;
  const size_t avail = workspace_bytes > slot ? workspace_bytes - slot : 0;
  thread_local Plan h;
  int st = build_plan(outs, m, d, disc, N, weights, S, target, B, workspace, avail, &h);
  if (st) return st;
  if ((st = copy_disc_means(h, stream))) return st;
  Plan* dev = reinterpret_cast<Plan*>((reinterpret_cast<uintptr_t>(workspace) + avail + 255) & ~(uintptr_t)255);
  if ((st = hip_status(hipMemcpyAsync(dev, &h, sizeof(Plan), hipMemcpyHostToDevice, stream), "hipMemcpyAsync")))
    return st;
  return run_forward(h, dev, xnew, B, kg, kg_pairs, stream, stage_ms);
}

}  // namespace

extern "C" {

int dkg_abi_version(void) { return DKG_ABI_VERSION; }

const char* dkg_last_error(void) { return g_err.c_str(); }

size_t dkg_frag_elems(int rows, int n) { return (size_t)pad16(std::max(rows, 0)) * pad16(std::max(n, 0)); }

size_t dkg_prepare_workspace(int n) {
  if (n < 1) return 0;
  return up256((size_t)n * n * sizeof(double)) + 256;
}

// Argument checks of one output's preparation (dkg_prepare_output / dkg_prepare_outputs).
static int check_prepare(const dkg_output* o, int d, const double* train_y, int max_tries, const double* L,
                         const void* work, size_t work_bytes, const double* alpha, const double* root_frag) {
  if (!o || !train_y || !L || !work || !alpha || !root_frag || !o->inv_lengthscale || !o->train_x)
    return failf(DKG_ERR_ARG, "NULL pointer");
  const int n = o->n;
  if (n < 1) return failf(DKG_ERR_ARG, "n=%d training points", n);
  if (pad16(n) > 1024) return failf(DKG_ERR_UNSUPPORTED, "n=%d > 1024 training points", n);
  if (d < 1 || d > DKG_MAX_DIM) return failf(DKG_ERR_UNSUPPORTED, "d=%d (supported 1..%d)", d, DKG_MAX_DIM);
  if (o->kernel < DKG_MATERN12 || o->kernel > DKG_RBF) return failf(DKG_ERR_ARG, "kernel id %d", o->kernel);
  if (max_tries < 0) return failf(DKG_ERR_ARG, "max_tries=%d", max_tries);
  if (work_bytes < dkg_prepare_workspace(n))
    return failf(DKG_ERR_WORKSPACE, "workspace %zu bytes < required %zu", work_bytes, dkg_prepare_workspace(n));
  return DKG_OK;
}

static int* prepare_info(void* work, int n) {
  return at<int>(work, up256((size_t)n * n * sizeof(double)));
}

// psd_safe_cholesky's attempts first .. max_tries of one output (attempt 0: no jitter; then absolute jitter
// 1e-8 * 10^(attempt - 1)), each checked on the host.  *jit: the jitter that worked.
static int cholesky_attempts(const dkg_output* o, int d, double* L, double* X, int* info, int first, int max_tries,
                             hipStream_t s, double* jit) {
  int st, h_info = 1;
  for (int attempt = first; attempt <= max_tries; ++attempt) {
    *jit = attempt == 0 ? 0.0 : 1e-8 * std::pow(10.0, attempt - 1);
    if ((st = hip_status(launch_kernel_matrix(*o, d, o->train_x, o->n, o->train_x, o->n, o->noise + *jit, L, s),
                         "kernel_matrix")))
      return st;
    if ((st = hip_status(hipMemsetAsync(info, 0, sizeof(int), s), "hipMemsetAsync")) ||
        (st = hip_status(launch_cholesky(L, X, o->n, info, s), "cholesky")) ||
        (st = hip_status(hipMemcpyAsync(&h_info, info, sizeof(int), hipMemcpyDeviceToHost, s), "hipMemcpyAsync")) ||
        (st = hip_status(hipStreamSynchronize(s), "hipStreamSynchronize")))
      return st;
    if (h_info == 0) return DKG_OK;
  }
  return failf(DKG_ERR_NOT_PD, "covariance not positive definite after %d jitter retries (pivot %d)", max_tries,
               h_info);
}

int dkg_prepare_output(const dkg_output* o, int d, const double* train_y, int max_tries, double* L, void* work,
                       size_t work_bytes, double* alpha, double* root_frag, double* jitter_used, void* stream) {
  int st = check_prepare(o, d, train_y, max_tries, L, work, work_bytes, alpha, root_frag);
  if (st) return st;
  hipStream_t s = (hipStream_t)stream;
  const int n = o->n;
  double* X = static_cast<double*>(work);
  int* info = prepare_info(work, n);
  double jit = 0.0;
  if ((st = cholesky_attempts(o, d, L, X, info, 0, max_tries, s, &jit))) return st;
  if (jitter_used) *jitter_used = jit;
  if ((st = hip_status(launch_tri_inverse(L, X, n, info, s), "tri_inverse")) ||
      (st = hip_status(launch_alpha(X, train_y, o->mean_constant, n, alpha, info, s), "alpha")) ||
      (st = hip_status(launch_pack_linv(X, n, root_frag, s), "pack_linv")))
    return st;
  return DKG_OK;
}

// The batched factorisation of dkg_prepare_outputs and dkg_mll_value_grad, from a batch whose kernel matrices are
// filled and whose flags are zeroed: every output's first attempt in one chain of launches and one status check, the
// outputs that failed retried with jitter one by one (as dkg_prepare_output from its second attempt), the inverses in
// one chain, then alpha (and, with root_frag, R^T's fragments) per output.  d_info: the flags where they lie side by
// side (one copy), NULL where each output has its own buffer (a copy each).
static int factor_batch(const dkg_output* outs, int m, int d, const double* const* train_y, int max_tries,
                        const PrepBatch& b, const int* d_info, double* const* alpha, double* const* root_frag,
                        double* jitter_used, hipStream_t s) {
  int st, h_info[DKG_MAX_OUTPUTS];
  if ((st = hip_status(launch_cholesky_batch(b, m, s), "cholesky_batch"))) return st;
  for (int i = 0; i < (d_info ? 1 : m); ++i)
    if ((st = hip_status(hipMemcpyAsync(&h_info[i], d_info ? d_info : b.info[i], (d_info ? m : 1) * sizeof(int),
                                        hipMemcpyDeviceToHost, s), "hipMemcpyAsync")))
      return st;
  if ((st = hip_status(hipStreamSynchronize(s), "hipStreamSynchronize"))) return st;
  double jit[DKG_MAX_OUTPUTS] = {};
  for (int i = 0; i < m; ++i)
    if (h_info[i] != 0 && (st = cholesky_attempts(&outs[i], d, b.A[i], b.X[i], b.info[i], 1, max_tries, s, &jit[i])))
      return st;
  if ((st = hip_status(launch_tri_inverse_batch(b, m, s), "tri_inverse_batch"))) return st;
  for (int i = 0; i < m; ++i) {
    if ((st = hip_status(launch_alpha(b.X[i], train_y[i], outs[i].mean_constant, b.n[i], alpha[i], b.info[i], s),
                         "alpha")) ||
        (root_frag && (st = hip_status(launch_pack_linv(b.X[i], b.n[i], root_frag[i], s), "pack_linv"))))
      return st;
    if (jitter_used) jitter_used[i] = jit[i];
  }
  return DKG_OK;
}

int dkg_prepare_outputs(const dkg_output* outs, int m, int d, const double* const* train_y, int max_tries,
                        double* const* L, void* const* work, const size_t* work_bytes, double* const* alpha,
                        double* const* root_frag, double* jitter_used, void* stream) {
  if (!outs || m < 1 || m > DKG_MAX_OUTPUTS) return failf(DKG_ERR_ARG, "m=%d outputs (1..%d)", m, DKG_MAX_OUTPUTS);
  if (!train_y || !L || !work || !work_bytes || !alpha || !root_frag) return failf(DKG_ERR_ARG, "NULL pointer");
  int st;
  for (int i = 0; i < m; ++i)
    if ((st = check_prepare(&outs[i], d, train_y[i], max_tries, L[i], work[i], work_bytes[i], alpha[i], root_frag[i])))
      return st;
  hipStream_t s = (hipStream_t)stream;
  PrepBatch b{};
  for (int i = 0; i < m; ++i) {
    b.A[i] = L[i];
    b.X[i] = static_cast<double*>(work[i]);
    b.n[i] = outs[i].n;
    b.info[i] = prepare_info(work[i], outs[i].n);
    if ((st = hip_status(launch_kernel_matrix(outs[i], d, outs[i].train_x, outs[i].n, outs[i].train_x, outs[i].n,
                                              outs[i].noise, L[i], s), "kernel_matrix")) ||
        (st = hip_status(hipMemsetAsync(b.info[i], 0, sizeof(int), s), "hipMemsetAsync")))
      return st;
  }
  return factor_batch(outs, m, d, train_y, max_tries, b, nullptr, alpha, root_frag, jitter_used, s);
}

// Workspace of dkg_mll_value_grad, walked once: a head shared by the outputs (their factorisation flags, then their
// result rows [DKG_MAX_OUTPUTS][MLL_OUT], each side by side: one copy each way), then per output the matrix, its
// inverse, alpha and the tile partials.  Returns the total; given the workspace it also fills the batches' pointers.
static size_t carve_mll(const int* n, int m, void* work = nullptr, PrepBatch* b = nullptr, MllBatch* mb = nullptr) {
  Carve c;
  const size_t info = c.take(DKG_MAX_OUTPUTS * sizeof(int)), out = c.take(DKG_MAX_OUTPUTS * MLL_OUT * sizeof(double));
  for (int i = 0; i < m; ++i) {
    const size_t A = c.take((size_t)n[i] * n[i] * sizeof(double)), X = c.take((size_t)n[i] * n[i] * sizeof(double));
    const size_t alpha = c.take((size_t)pad16(n[i]) * sizeof(double));
    const size_t part = c.take((size_t)mll_tiles(n[i]) * MLL_NP * sizeof(double));
    if (!work) continue;
    mb->L[i] = b->A[i] = at<double>(work, A);
    mb->M[i] = b->X[i] = at<double>(work, X);
    mb->info[i] = b->info[i] = at<int>(work, info) + i;
    b->n[i] = n[i];
    mb->alpha[i] = at<double>(work, alpha);
    mb->part[i] = at<double>(work, part);
    mb->out[i] = at<double>(work, out) + (size_t)i * MLL_OUT;
  }
  return c.total();
}

size_t dkg_mll_workspace(const int* n, int m) {
  if (!n || m < 1 || m > DKG_MAX_OUTPUTS) return 0;
  for (int i = 0; i < m; ++i)
    if (n[i] < 1 || n[i] > 1024) return 0;
  return carve_mll(n, m);
}

int dkg_mll_value_grad(const dkg_output* outs, int m, int d, const double* const* train_y, int max_tries, void* work,
                       size_t work_bytes, double* value, double* grad, double* jitter_used, void* stream) {
  if (!outs || !train_y || !work || !value || !grad) return failf(DKG_ERR_ARG, "NULL pointer");
  if (m < 1) return failf(DKG_ERR_ARG, "m=%d outputs", m);
  if (m > DKG_MAX_OUTPUTS) return failf(DKG_ERR_UNSUPPORTED, "m=%d outputs (supported 1..%d)", m, DKG_MAX_OUTPUTS);
  if (d < 1) return failf(DKG_ERR_ARG, "d=%d", d);
  if (d > DKG_MAX_DIM) return failf(DKG_ERR_UNSUPPORTED, "d=%d (supported 1..%d)", d, DKG_MAX_DIM);
  if (max_tries < 0) return failf(DKG_ERR_ARG, "max_tries=%d", max_tries);
  int ns[DKG_MAX_OUTPUTS];
  for (int i = 0; i < m; ++i) {
    const dkg_output& o = outs[i];
    if (!train_y[i] || !o.inv_lengthscale || !o.train_x) return failf(DKG_ERR_ARG, "NULL pointer");
    if (o.n < 1) return failf(DKG_ERR_ARG, "n=%d training points", o.n);
    if (o.n > 1024) return failf(DKG_ERR_UNSUPPORTED, "n=%d > 1024 training points", o.n);
    if (o.kernel < DKG_MATERN12 || o.kernel > DKG_RBF) return failf(DKG_ERR_ARG, "kernel id %d", o.kernel);
    ns[i] = o.n;
  }
  const size_t need = carve_mll(ns, m);
  if (work_bytes < need) return failf(DKG_ERR_WORKSPACE, "workspace %zu bytes < required %zu", work_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  PrepBatch b{};
  MllBatch mb{};
  mb.d = d;
  carve_mll(ns, m, work, &b, &mb);
  int st;
  double jit[DKG_MAX_OUTPUTS], *alpha[DKG_MAX_OUTPUTS];
  int* d_info = b.info[0];
  double* d_out = mb.out[0];
  if ((st = hip_status(hipMemsetAsync(d_info, 0, DKG_MAX_OUTPUTS * sizeof(int), s), "hipMemsetAsync"))) return st;
  for (int i = 0; i < m; ++i) {
    mb.o[i] = outs[i];
    mb.y[i] = train_y[i];
    alpha[i] = const_cast<double*>(mb.alpha[i]);
    if ((st = hip_status(launch_kernel_matrix(outs[i], d, outs[i].train_x, ns[i], outs[i].train_x, ns[i],
                                              outs[i].noise, b.A[i], s), "kernel_matrix")))
      return st;
  }
  if ((st = factor_batch(outs, m, d, train_y, max_tries, b, d_info, alpha, nullptr, jit, s))) return st;
  if ((st = hip_status(launch_mll(mb, m, s), "mll"))) return st;
  double h_out[DKG_MAX_OUTPUTS][MLL_OUT];
  if ((st = hip_status(hipMemcpyAsync(h_out, d_out, (size_t)m * MLL_OUT * sizeof(double), hipMemcpyDeviceToHost, s),
                       "hipMemcpyAsync")) ||
      (st = hip_status(hipStreamSynchronize(s), "hipStreamSynchronize")))
    return st;
  for (int i = 0; i < m; ++i) {
    value[i] = h_out[i][0];
    for (int j = 0; j < d + 3; ++j) grad[(size_t)i * (d + 3) + j] = h_out[i][1 + j];
    if (jitter_used) jitter_used[i] = jit[i];
  }
  return DKG_OK;
}

int dkg_kernel_matrix(const dkg_output* o, int d, const double* x1, int n1, const double* x2, int n2,
                      double diag_add, double* out, void* stream) {
  if (!o || !x1 || !x2 || !out || !o->inv_lengthscale) return failf(DKG_ERR_ARG, "NULL pointer");
  if (d < 1 || d > DKG_MAX_DIM) return failf(DKG_ERR_UNSUPPORTED, "d=%d", d);
  if (n1 < 0 || n2 < 0) return failf(DKG_ERR_ARG, "negative size");
  if (n1 == 0 || n2 == 0) return DKG_OK;
  return hip_status(launch_kernel_matrix(*o, d, x1, n1, x2, n2, diag_add, out, (hipStream_t)stream),
                    "kernel_matrix_kernel");
}

int dkg_pack_root(const double* r, int n, double* root_frag, void* stream) {
  if (!r || !root_frag || n < 1) return failf(DKG_ERR_ARG, "bad arguments");
  return hip_status(launch_pack_root(r, n, root_frag, (hipStream_t)stream), "pack_root_kernel");
}

int dkg_cross_root(const dkg_output* o, int d, const double* x, int rows, double* q_frag, double* mean,
                   void* stream) {
  int st = check_outputs(o, 1, d);
  if (st) return st;
  if (rows < 0 || !q_frag || (rows > 0 && !x)) return failf(DKG_ERR_ARG, "bad arguments");
  if (rows == 0) return DKG_OK;
  CrossArgs ca{};
  ca.o = *o;
  ca.d = d;
  ca.rows = rows;
  ca.x = x;
  ca.q = q_frag;
  ca.mean = mean;
  return hip_status(launch_cross_root(ca, (hipStream_t)stream), "cross_root_kernel");
}

size_t dkg_append_workspace(int n, int N) {
  if (n < 1 || N < 0) return 0;
  return APPEND_WS_BYTES;  // the info flag, lambda, l and beta' (1024 entries each)
}

int dkg_append_observation(const dkg_output* o, int d, const double* L, const double* Linv, const double* disc, int N,
                           const double* train_x, const double* train_y, double jitter, double* L_new,
                           double* Linv_new, double* alpha_new, double* root_frag_new, double* disc_frag_new,
                           double* disc_mean_new, void* work, size_t work_bytes, void* stream) {
  if (!o || !L || !Linv || !train_x || !train_y || !L_new || !Linv_new || !alpha_new || !root_frag_new || !work ||
      !o->inv_lengthscale)
    return failf(DKG_ERR_ARG, "NULL pointer");
  if (N < 0) return failf(DKG_ERR_ARG, "N=%d discretisation points", N);
  if (N > 0 && (!disc || !o->disc_frag || !disc_frag_new || !disc_mean_new)) return failf(DKG_ERR_ARG, "NULL pointer");
  const int n = o->n;
  if (n < 1) return failf(DKG_ERR_ARG, "n=%d training points", n);
  if (pad16(n + 1) > 1024) return failf(DKG_ERR_UNSUPPORTED, "n=%d > 1024 training points", n + 1);
  if (d < 1 || d > DKG_MAX_DIM) return failf(DKG_ERR_UNSUPPORTED, "d=%d (supported 1..%d)", d, DKG_MAX_DIM);
  if (N > (1 << 22)) return failf(DKG_ERR_UNSUPPORTED, "N=%d discretisation points (supported <= %d)", N, 1 << 22);
  if (o->kernel < DKG_MATERN12 || o->kernel > DKG_RBF) return failf(DKG_ERR_ARG, "kernel id %d", o->kernel);
  if (!(jitter >= 0.0)) return failf(DKG_ERR_ARG, "jitter=%g", jitter);
  if (work_bytes < dkg_append_workspace(n, N))
    return failf(DKG_ERR_WORKSPACE, "workspace %zu bytes < required %zu", work_bytes, dkg_append_workspace(n, N));
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(work);
  AppendArgs a{};
  a.o = *o;
  a.d = d;
  a.N = N;
  a.L = L;
  a.M = Linv;
  a.xt = train_x;
  a.y = train_y;
  a.diag = o->noise + jitter;  // as the old factorisation's kernel matrix took it
  a.disc = disc;
  a.Ln = L_new;
  a.Mn = Linv_new;
  a.alpha = alpha_new;
  a.qn = disc_frag_new;
  a.mean = disc_mean_new;
  a.info = reinterpret_cast<int*>(ws);
  a.lam = reinterpret_cast<double*>(ws + APPEND_WS_LAM);
  a.lvec = reinterpret_cast<double*>(ws + APPEND_WS_L);
  a.beta = reinterpret_cast<double*>(ws + APPEND_WS_BETA);
  int st, h_info = 1;
  if ((st = hip_status(hipMemsetAsync(a.info, 0, sizeof(int), s), "hipMemsetAsync")) ||
      (st = hip_status(launch_append(a, root_frag_new, s), "append")) ||
      (st = hip_status(hipMemcpyAsync(&h_info, a.info, sizeof(int), hipMemcpyDeviceToHost, s), "hipMemcpyAsync")) ||
      (st = hip_status(hipStreamSynchronize(s), "hipStreamSynchronize")))
    return st;
  if (h_info != 0)
    return failf(DKG_ERR_NOT_PD, "covariance not positive definite with the appended observation (pivot %d)", h_info);
  return DKG_OK;
}

// Workspace of dkg_append_rows, walked once: the status words side by side (one copy back), the job descriptors
// (one copy in), then each job's kx, bx, wp, kd and ch (RowsJob).  Returns the total; given `out` it fills the
// descriptors' workspace pointers (offsets from `work`).
static size_t carve_rows(const dkg_append_job* jobs, int J, void* work = nullptr, RowsJob* out = nullptr,
                         size_t* desc_off = nullptr) {
  Carve c;
  c.take((size_t)J * sizeof(int));
  const size_t desc = c.take((size_t)J * sizeof(RowsJob));
  if (desc_off) *desc_off = desc;
  for (int j = 0; j < J; ++j) {
    const size_t n = jobs[j].o->n, np = pad16((int)n), K1 = jobs[j].K + 1;
    const size_t kx = c.take(K1 * np * sizeof(double)), bx = c.take(K1 * np * sizeof(double));
    const size_t wp = c.take((n + ROWS_CHUNK - 1) / ROWS_CHUNK * K1 * np * sizeof(double));
    const size_t kd = c.take((size_t)jobs[j].K * pad16(jobs[j].N) * sizeof(double));
    const size_t ch = c.take(ROWS_CH_DOUBLES * sizeof(double));
    if (!out) continue;
    out[j].kx = at<double>(work, kx);
    out[j].bx = at<double>(work, bx);
    out[j].wp = at<double>(work, wp);
    out[j].kd = at<double>(work, kd);
    out[j].ch = at<double>(work, ch);
  }
  return c.total();
}

// The sizes of one job (shared by the workspace query, which answers 0, and the call, which reports).
static int check_rows_sizes(const dkg_append_job& b, int j) {
  if (!b.o) return failf(DKG_ERR_ARG, "job %d: o is NULL", j);
  if (b.o->n < 1) return failf(DKG_ERR_ARG, "job %d: n=%d training points", j, b.o->n);
  if (b.K < 1) return failf(DKG_ERR_ARG, "job %d: K=%d new rows", j, b.K);
  if (b.K > DKG_APPEND_MAX_ROWS)
    return failf(DKG_ERR_UNSUPPORTED, "job %d: K=%d new rows (supported 1..%d)", j, b.K, DKG_APPEND_MAX_ROWS);
  if (b.o->n > 1024 || pad16(b.o->n + b.K) > 1024)
    return failf(DKG_ERR_UNSUPPORTED, "job %d: n=%d > 1024 training points", j, b.o->n + b.K);
  if (b.N < 0) return failf(DKG_ERR_ARG, "job %d: N=%d discretisation points", j, b.N);
  if (b.N > (1 << 22))
    return failf(DKG_ERR_UNSUPPORTED, "job %d: N=%d discretisation points (supported <= %d)", j, b.N, 1 << 22);
  return DKG_OK;
}

static int check_rows_count(const dkg_append_job* jobs, int J, int d) {
  if (!jobs) return failf(DKG_ERR_ARG, "jobs is NULL");
  if (J < 1) return failf(DKG_ERR_ARG, "J=%d jobs", J);
  if (J > DKG_APPEND_MAX_JOBS) return failf(DKG_ERR_UNSUPPORTED, "J=%d jobs (supported 1..%d)", J, DKG_APPEND_MAX_JOBS);
  if (d < 1 || d > DKG_MAX_DIM) return failf(DKG_ERR_UNSUPPORTED, "d=%d (supported 1..%d)", d, DKG_MAX_DIM);
  return DKG_OK;
}

size_t dkg_append_rows_workspace(const dkg_append_job* jobs, int J, int d) {
  if (check_rows_count(jobs, J, d)) return 0;
  for (int j = 0; j < J; ++j)
    if (check_rows_sizes(jobs[j], j)) return 0;
  return carve_rows(jobs, J);
}

int dkg_append_rows(const dkg_append_job* jobs, int J, int d, int32_t* info, void* work, size_t work_bytes,
                    void* stream) {
  int st = check_rows_count(jobs, J, d);
  if (st) return st;
  if (!info) return failf(DKG_ERR_ARG, "info is NULL");
  int nmax = 0, Kmax = 0, Nmax = 0;
  for (int j = 0; j < J; ++j) {
    const dkg_append_job& b = jobs[j];
    if ((st = check_rows_sizes(b, j))) return st;
    if ((st = check_outputs(b.o, 1, d))) return failf(st, "job %d: %s", j, std::string(dkg_last_error()).c_str());
    if (!b.L || !b.Linv || !b.train_x || !b.train_y || !b.L_new || !b.Linv_new || !b.alpha_new || !b.root_frag_new)
      return failf(DKG_ERR_ARG, "job %d: NULL pointer", j);
    if (b.N > 0 && (!b.disc || !b.o->disc_frag || !b.disc_frag_new || !b.disc_mean_new))
      return failf(DKG_ERR_ARG, "job %d: N=%d with a NULL discretisation pointer", j, b.N);
    if (!(b.jitter >= 0.0)) return failf(DKG_ERR_ARG, "job %d: jitter=%g", j, b.jitter);
    nmax = std::max(nmax, (int)b.o->n);
    Kmax = std::max(Kmax, (int)b.K);
    Nmax = std::max(Nmax, (int)b.N);
  }
  if (!work) return failf(DKG_ERR_ARG, "work is NULL");
  const size_t need = carve_rows(jobs, J);
  if (work_bytes < need) return failf(DKG_ERR_WORKSPACE, "workspace %zu bytes < required %zu", work_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  std::vector<RowsJob> desc(J);
  size_t desc_off = 0;
  carve_rows(jobs, J, work, desc.data(), &desc_off);
  for (int j = 0; j < J; ++j) {
    const dkg_append_job& b = jobs[j];
    RowsJob& a = desc[j];
    a.o = *b.o;
    a.L = b.L;
    a.M = b.Linv;
    a.xt = b.train_x;
    a.y = b.train_y;
    a.disc = b.disc;
    a.diag = b.o->noise + b.jitter;  // as the old factorisation's kernel matrix took it
    a.Ln = b.L_new;
    a.Mn = b.Linv_new;
    a.alpha = b.alpha_new;
    a.rf = b.root_frag_new;
    a.qn = b.disc_frag_new;
    a.mean = b.disc_mean_new;
    a.N = b.N;
    a.K = b.K;
  }
  int* d_info = static_cast<int*>(work);
  RowsJob* d_jobs = at<RowsJob>(work, desc_off);
  for (int j = 0; j < J; ++j) info[j] = -1;
  if ((st = hip_status(hipMemcpyAsync(d_jobs, desc.data(), (size_t)J * sizeof(RowsJob), hipMemcpyHostToDevice, s),
                       "hipMemcpyAsync")) ||
      (st = hip_status(hipMemsetAsync(d_info, 0xff, (size_t)J * sizeof(int), s), "hipMemsetAsync")) ||
      (st = hip_status(launch_append_rows(d_jobs, J, d, nmax, Kmax, Nmax, d_info, s), "append_rows")) ||
      (st = hip_status(hipMemcpyAsync(info, d_info, (size_t)J * sizeof(int), hipMemcpyDeviceToHost, s),
                       "hipMemcpyAsync")) ||
      (st = hip_status(hipStreamSynchronize(s), "hipStreamSynchronize")))
    return st;
  int bad = 0, first = -1;
  for (int j = 0; j < J; ++j)
    if (info[j] != 0 && bad++ == 0) first = j;
  if (bad)
    return failf(DKG_ERR_NOT_PD, "covariance not positive definite with the appended rows: %d of %d jobs, the first "
                 "job %d (pivot %d)", bad, J, first, info[first]);
  return DKG_OK;
}

size_t dkg_forward_workspace(const dkg_output* outs, int m, int N, int B, int S) {
  if (!outs || m < 1 || m > DKG_MAX_OUTPUTS) return 0;
  return carve_plan(outs, m, N, B, S, 0, 0, 1) + plan_slot_bytes() + 256;
}

int dkg_forward(const dkg_output* outs, int m, int d, const double* disc, int N, const double* xnew, int B,
                const double* weights, int S, int target, double* kg, double* kg_pairs, void* workspace,
                size_t workspace_bytes, void* stream) {
  return forward_oneshot(outs, m, d, disc, N, xnew, B, weights, S, target, kg, kg_pairs, workspace, workspace_bytes,
                         (hipStream_t)stream, nullptr);
}

int dkg_forward_timed(const dkg_output* outs, int m, int d, const double* disc, int N, const double* xnew,
                      int B, const double* weights, int S, int target, double* kg, double* kg_pairs,
                      void* workspace, size_t workspace_bytes, void* stream, float* stage_ms) {
  if (!stage_ms) return failf(DKG_ERR_ARG, "stage_ms is NULL");
  return forward_oneshot(outs, m, d, disc, N, xnew, B, weights, S, target, kg, kg_pairs, workspace, workspace_bytes,
                         (hipStream_t)stream, stage_ms);
}

size_t dkg_plan_bytes(void) { return sizeof(Plan); }

static int time_stage(const void* host_plan, const void* dev_plan, const double* xnew, int B, double* kg,
                      double* kg_pairs, void* stream, int stage, int reps, float* avg_ms, int geom_B) {
  if (!host_plan || !dev_plan || !avg_ms) return failf(DKG_ERR_ARG, "NULL pointer");
  if (stage < 0 || stage > 3 || reps < 1) return failf(DKG_ERR_ARG, "stage=%d reps=%d", stage, reps);
  const Plan& h = *static_cast<const Plan*>(host_plan);
  if (B < 1 || B > h.max_B) return failf(DKG_ERR_ARG, "B=%d outside [1, %d]", B, h.max_B);
  if (!xnew || !kg) return failf(DKG_ERR_ARG, "NULL data pointer");
  const Plan* dev = static_cast<const Plan*>(dev_plan);
  hipStream_t s = (hipStream_t)stream;
  hipEvent_t ev[2];
  int st;
  for (int k = 0; k < 2; ++k)
    if ((st = hip_status(hipEventCreate(&ev[k]), "hipEventCreate"))) return st;
  // prime the inputs of the timed stage, then time reps back-to-back launches of it alone
  if ((st = hip_status(launch_forward(h, dev, xnew, B, kg, kg_pairs, s, nullptr, geom_B), "forward"))) return st;
  (void)hipEventRecord(ev[0], s);
  for (int r = 0; r < reps; ++r)
    if ((st = hip_status(stage == 3 ? (geom_B ? launch_forward(h, dev, xnew, B, kg, nullptr, s, nullptr, geom_B)
                                             : launch_forward_auto(h, dev, xnew, B, kg, nullptr, s))
                                   : launch_stage(h, dev, xnew, B, kg, kg_pairs, s, stage, geom_B),
                         "stage")))
      return st;
  (void)hipEventRecord(ev[1], s);
  if ((st = hip_status(hipEventSynchronize(ev[1]), "hipEventSynchronize"))) return st;
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
  *avg_ms = ms / reps;
  for (int k = 0; k < 2; ++k) (void)hipEventDestroy(ev[k]);
  // leave kg / kg_pairs valid again (repeated stages accumulate into kg)
  return hip_status(launch_forward(h, dev, xnew, B, kg, kg_pairs, s, nullptr, geom_B), "forward");
}

int dkg_plan_time_stage(const void* host_plan, const void* dev_plan, const double* xnew, int B, double* kg,
                        double* kg_pairs, void* stream, int stage, int reps, float* avg_ms) {
  return time_stage(host_plan, dev_plan, xnew, B, kg, kg_pairs, stream, stage, reps, avg_ms, 0);
}

int dkg_plan_time_stage_batches(const void* host_plan, const void* dev_plan, const double* xnew, int B, int nbatch,
                                double* kg, void* stream, int stage, int reps, float* avg_ms) {
  if (B < 1 || nbatch < 1) return failf(DKG_ERR_ARG, "B=%d nbatch=%d", B, nbatch);
  if (!host_plan) return failf(DKG_ERR_ARG, "NULL plan pointer");
  // (as dkg_plan_forward_batches: the product in 64 bits, so a wrapped int cannot pass the capacity check)
  if (static_cast<const Plan*>(host_plan)->ntgt > 1)
    return failf(DKG_ERR_UNSUPPORTED, "dkg_plan_time_stage_batches runs one target per plan; the plan has %d",
                 static_cast<const Plan*>(host_plan)->ntgt);
  if ((long long)B * nbatch > static_cast<const Plan*>(host_plan)->max_B)
    return failf(DKG_ERR_ARG, "%d batches of B=%d candidates > plan capacity %d", nbatch, B,
                 static_cast<const Plan*>(host_plan)->max_B);
  return time_stage(host_plan, dev_plan, xnew, B * nbatch, kg, nullptr, stream, stage, reps, avg_ms, B);
}

size_t dkg_plan_workspace(const dkg_output* outs, int m, int d, int N, int max_B, int S, int flags) {
  if (!outs || m < 1 || m > DKG_MAX_OUTPUTS) return 0;
  return carve_plan(outs, m, N, max_B, S, d, flags, 1);
}

int dkg_plan_grad_rows(const dkg_output* outs, int m, int d, int N, int S, int flags) {
  int st = check_outputs(outs, m, d);
  if (st) return -st;
  if (N < 0) return -failf(DKG_ERR_ARG, "negative size N=%d", N);
  if (S < 1) return -failf(DKG_ERR_ARG, "S=%d scalarisations", S);
  const int max_np = max_np_of(outs, m);
  int sw, split;
  if ((st = plan_geometry(m, N, S, d, max_np, &sw, &split)) || (st = check_plan_flags(flags))) return -st;
  if (!(flags & DKG_PLAN_GRAD)) return -failf(DKG_ERR_ARG, "dkg_plan_grad_rows: flags 0x%x lack DKG_PLAN_GRAD", flags);
  return grad_rows_rule(m, N, sw, S, d, max_np, flags);
}

int dkg_plan_init(const dkg_output* outs, int m, int d, const double* disc, int N, const double* weights, int S,
                  int target, int max_B, int flags, void* workspace, size_t workspace_bytes, void* host_plan,
                  void* dev_plan, void* stream) {
  if (!host_plan || !dev_plan) return failf(DKG_ERR_ARG, "NULL plan pointer");
  Plan* h = static_cast<Plan*>(host_plan);
  return upload_plan(build_plan(outs, m, d, disc, N, weights, S, target, max_B, workspace, workspace_bytes, h, flags),
                     h, dev_plan, (hipStream_t)stream);
}

size_t dkg_plan_workspace_targets(const dkg_output* outs, int m, int d, int N, int max_B, int S, int T, int flags) {
  if (!outs || m < 1 || m > DKG_MAX_OUTPUTS || T < 1 || T > m + 1) return 0;
  return carve_plan(outs, m, N, max_B, S, d, flags, T);
}

int dkg_plan_init_targets(const dkg_output* outs, int m, int d, const double* disc, int N, const double* weights,
                          int S, const int* targets, int T, int max_B, int flags, void* workspace,
                          size_t workspace_bytes, void* host_plan, void* dev_plan, void* stream) {
  if (!host_plan || !dev_plan) return failf(DKG_ERR_ARG, "NULL plan pointer");
  if (!targets) return failf(DKG_ERR_ARG, "targets is NULL");
  Plan* h = static_cast<Plan*>(host_plan);
  return upload_plan(build_plan(outs, m, d, disc, N, weights, S, -1, max_B, workspace, workspace_bytes, h, flags,
                                targets, T), h, dev_plan, (hipStream_t)stream);
}

int dkg_plan_forward(const void* host_plan, const void* dev_plan, const double* xnew, int B, double* kg,
                     double* kg_pairs, void* stream) {
  if (!host_plan || !dev_plan) return failf(DKG_ERR_ARG, "NULL plan pointer");
  return run_forward(*static_cast<const Plan*>(host_plan), static_cast<const Plan*>(dev_plan), xnew, B, kg, kg_pairs,
                     (hipStream_t)stream, nullptr);
}

int dkg_plan_forward_batches(const void* host_plan, const void* dev_plan, const double* xnew, int B, int nbatch,
                             double* kg, void* stream) {
  if (!host_plan || !dev_plan) return failf(DKG_ERR_ARG, "NULL plan pointer");
  const Plan& h = *static_cast<const Plan*>(host_plan);
  if (h.ntgt > 1)
    return failf(DKG_ERR_UNSUPPORTED, "dkg_plan_forward_batches runs one target per plan; the plan has %d", h.ntgt);
  if (B < 0 || nbatch < 0) return failf(DKG_ERR_ARG, "negative size B=%d nbatch=%d", B, nbatch);
  if ((long long)B * nbatch == 0) return DKG_OK;
  if ((long long)B * nbatch > h.max_B)
    return failf(DKG_ERR_ARG, "%d batches x B=%d candidates > plan capacity %d", nbatch, B, h.max_B);
  if (!xnew || !kg) return failf(DKG_ERR_ARG, "NULL data pointer");
  // the three stage kernels over all nbatch * B candidates, the covariance blocks chosen for one batch of B
  return hip_status(launch_forward(h, static_cast<const Plan*>(dev_plan), xnew, B * nbatch, kg, nullptr,
                                   (hipStream_t)stream, nullptr, B),
                    "forward_batches");
}

int dkg_plan_forward_timed(const void* host_plan, const void* dev_plan, const double* xnew, int B, double* kg,
                           double* kg_pairs, void* stream, float* stage_ms) {
  if (!host_plan || !dev_plan || !stage_ms) return failf(DKG_ERR_ARG, "NULL pointer");
  return run_forward(*static_cast<const Plan*>(host_plan), static_cast<const Plan*>(dev_plan), xnew, B, kg, kg_pairs,
                     (hipStream_t)stream, stage_ms);
}

int dkg_plan_forward_grad(const void* host_plan, const void* dev_plan, const double* xnew, int B, double* kg,
                          double* dkg_dx, void* stream) {
  if (!host_plan || !dev_plan) return failf(DKG_ERR_ARG, "NULL plan pointer");
  const Plan& h = *static_cast<const Plan*>(host_plan);
  if (!h.grad) return failf(DKG_ERR_ARG, "plan was not initialised with DKG_PLAN_GRAD");
  if (int st = check_batch(h, B)) return std::max(st, 0);
  if (!xnew || !kg || !dkg_dx) return failf(DKG_ERR_ARG, "NULL data pointer");
  return hip_status(launch_forward_grad(h, static_cast<const Plan*>(dev_plan), xnew, B, kg, dkg_dx,
                                        (hipStream_t)stream), "forward_grad");
}

int dkg_plan_forward_grad_hostx(const void* host_plan, const void* dev_plan, const double* x_host, double* x_dev,
                                int B, double* kg, double* dkg_dx, double* out_host, void* stream) {
  if (!host_plan || !dev_plan) return failf(DKG_ERR_ARG, "NULL plan pointer");
  const Plan& h = *static_cast<const Plan*>(host_plan);
  if (!h.grad) return failf(DKG_ERR_ARG, "plan was not initialised with DKG_PLAN_GRAD");
  if (int st = check_batch(h, B)) return std::max(st, 0);
  if ((long long)B * h.d > DKG_XARG_MAX)
    return failf(DKG_ERR_ARG, "B*d=%lld > DKG_XARG_MAX=%d (use dkg_plan_forward_grad)", (long long)B * h.d,
                 DKG_XARG_MAX);
  if (!x_host || !x_dev || !kg || !dkg_dx) return failf(DKG_ERR_ARG, "NULL data pointer");
  XArg xa;
  xa.n = B * h.d;
  for (int i = 0; i < xa.n; ++i) xa.v[i] = x_host[i];
  // (several targets: out_host holds [kg (T x B) | dkg_dx (T x B x d)])
  int st = hip_status(launch_forward_grad(h, static_cast<const Plan*>(dev_plan), x_dev, B, kg, dkg_dx,
                                          (hipStream_t)stream, &xa, out_host),
                      "forward_grad_hostx");
  if (st || !out_host) return st;
  return hip_status(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize");  // out_host is filled
}

int dkg_plan_status(const void* host_plan, int* err, int reset, void* stream) {
  if (!host_plan || !err) return failf(DKG_ERR_ARG, "NULL pointer");
  const Plan& h = *static_cast<const Plan*>(host_plan);
  hipStream_t s = (hipStream_t)stream;
  int st;
  if ((st = hip_status(hipMemcpyAsync(err, h.sync_err, sizeof(int), hipMemcpyDeviceToHost, s),
                       "hipMemcpyAsync(err)")) ||
      (st = hip_status(hipStreamSynchronize(s), "hipStreamSynchronize")))
    return st;
  if (reset) return hip_status(hipMemsetAsync(h.sync, 0, h.sync_bytes, s), "hipMemsetAsync(sync)");
  return DKG_OK;
}

int dkg_plan_fused(const void* host_plan) { return host_plan ? static_cast<const Plan*>(host_plan)->fused : 0; }

int dkg_plan_grad_rows_of(const void* host_plan) {
  return host_plan ? static_cast<const Plan*>(host_plan)->grad_rows : 0;
}

int dkg_plan_hull_sizes(const void* host_plan, int* out, int B, void* stream) {
  if (!host_plan || !out) return failf(DKG_ERR_ARG, "NULL pointer");
  const Plan& h = *static_cast<const Plan*>(host_plan);
  if (B < 0 || B > h.max_B) return failf(DKG_ERR_ARG, "B=%d outside [0, %d]", B, h.max_B);
  if (B == 0) return DKG_OK;
  if (h.ntgt > 1)  // [T][B][S] out of the workspace's items (tau * bpad + b)
    return hip_status(hipMemcpy2DAsync(out, sizeof(int) * (size_t)B * h.S, h.hull_pairs,
                                       sizeof(int) * (size_t)h.bpad * h.S, sizeof(int) * (size_t)B * h.S, h.ntgt,
                                       hipMemcpyDeviceToDevice, (hipStream_t)stream), "hipMemcpy2DAsync(hull sizes)");
  return hip_status(hipMemcpyAsync(out, h.hull_pairs, sizeof(int) * (size_t)B * h.S, hipMemcpyDeviceToDevice,
                                   (hipStream_t)stream), "hipMemcpyAsync(hull sizes)");
}

int dkg_lines_kg(const double* intercepts, const double* slopes, int P, int L, double* kg, int* n_hull,
                 void* stream) {
  if (P < 0 || L < 0) return failf(DKG_ERR_ARG, "negative size P=%d L=%d", P, L);
  if (P == 0) return DKG_OK;
  if (L == 0)
    return failf(DKG_ERR_NO_LINES, "Expected inputs to specify at least one line. Got intercepts.shape[-1]=0.");
  if (!intercepts || !slopes || !kg) return failf(DKG_ERR_ARG, "NULL pointer");
  return hip_status(launch_lines_kg(intercepts, slopes, P, L, kg, n_hull, nullptr, nullptr, 0, (hipStream_t)stream),
                    "lines_kg_kernel");
}

int dkg_epigraph(const double* intercepts, const double* slopes, int P, int L, int cap, long long* indices,
                 double* intersections, int* count, void* stream) {
  if (P < 0 || L < 0 || cap < 1) return failf(DKG_ERR_ARG, "bad size P=%d L=%d cap=%d", P, L, cap);
  if (P == 0) return DKG_OK;
  if (L == 0)
    return failf(DKG_ERR_NO_LINES, "Expected inputs to specify at least one line. Got intercepts.shape[-1]=0.");
  if (!intercepts || !slopes || !indices || !count || (cap > 1 && !intersections))
    return failf(DKG_ERR_ARG, "NULL pointer");
  return hip_status(launch_lines_kg(intercepts, slopes, P, L, nullptr, count, indices, intersections, cap,
                                    (hipStream_t)stream), "lines_kg_kernel(epigraph)");
}

int dkg_pwl_expectation(const double* intercepts, const double* slopes, const double* boundaries, int P, int m,
                        double* out, void* stream) {
  if (P < 0 || m < 0) return failf(DKG_ERR_ARG, "negative size P=%d m=%d", P, m);
  if (P == 0) return DKG_OK;
  if (m == 0)
    return failf(DKG_ERR_NO_LINES, "Expected inputs to specify at least one line. Got intercepts.shape[-1]=0.");
  if (!intercepts || !slopes || !out || (m > 1 && !boundaries)) return failf(DKG_ERR_ARG, "NULL pointer");
  return hip_status(launch_pwl_expectation(intercepts, slopes, boundaries, P, m, out, (hipStream_t)stream),
                    "pwl_expectation_kernel");
}

int dkg_plan_lines(const void* host_plan, const void* dev_plan, const double* xnew, int B, double* intercepts,
                   double* slopes, void* stream) {
  if (!host_plan || !dev_plan) return failf(DKG_ERR_ARG, "NULL plan pointer");
  const Plan& h = *static_cast<const Plan*>(host_plan);
  if (B < 0 || B > h.max_B) return failf(DKG_ERR_ARG, "B=%d outside [0, %d]", B, h.max_B);
  if (B == 0) return DKG_OK;
  if (!xnew || !intercepts || !slopes) return failf(DKG_ERR_ARG, "NULL data pointer");
  // several targets: the lines of tlist[0]; the cross stage clears ntgt rows of B accumulators in `intercepts`
  if ((long long)h.S * (h.N + 1) < h.ntgt)
    return failf(DKG_ERR_UNSUPPORTED, "dkg_plan_lines: S*(N+1)=%lld doubles per candidate < the plan's %d targets",
                 (long long)h.S * (h.N + 1), h.ntgt);
  // (an F32 plan exports the lines its fp32 contractions give: the error model's check, tools/f32_debug.py)
  const Plan* dev = static_cast<const Plan*>(dev_plan);
  hipStream_t s = (hipStream_t)stream;
  int st;
  for (int stage = 0; stage < 2; ++stage)  // K(x, X) R, means; covariance rows, variances (kg is only zeroed)
    if ((st = hip_status(launch_stage(h, dev, xnew, B, intercepts, nullptr, s, stage), "stage"))) return st;
  return hip_status(launch_lines_export(h, dev, B, intercepts, slopes, s), "lines_export_kernel");
}

int dkg_debug_read_kstamps(unsigned long long* host, int n) {
  if (!host || n < 0) return failf(DKG_ERR_ARG, "bad arguments");
  if (!g_kstamps_buf) return failf(DKG_ERR_ARG, "no plan was built with DKG_DEBUG_STAMPS=1");
  const size_t words = std::min<size_t>((size_t)n, (size_t)3 * KST_WG * 8);
  return hip_status(hipMemcpy(host, g_kstamps_buf, words * sizeof(unsigned long long), hipMemcpyDeviceToHost),
                    "hipMemcpy(stamps)");
}

int dkg_debug_cov_kernels(int mask) {
  if (mask < 0) {
    const int cur = set_cov_enabled(0);
    set_cov_enabled(cur);
    return cur;
  }
  return set_cov_enabled(mask);
}

int dkg_debug_cross_tall(int mode) {
  if (mode < -1 || mode > 1) {
    failf(DKG_ERR_ARG, "dkg_debug_cross_tall: mode=%d (-1 default, 0 never, 1 every eligible shape)", mode);
    return -2;
  }
  return set_cross_tall_mode(mode);
}

long long dkg_debug_cross_tall_launches(void) { return cross_tall_launches(); }

int dkg_debug_cross_tall_eligible(int max_n_pad, int d, int B, int f32) {
  if (max_n_pad < 16 || max_n_pad % 16 != 0 || d < 1 || d > DKG_MAX_DIM || B < 1) {
    failf(DKG_ERR_ARG, "dkg_debug_cross_tall_eligible: max_n_pad=%d d=%d B=%d", max_n_pad, d, B);
    return -2;
  }
  return cross_tall_eligible(max_n_pad, d, B, f32 != 0) ? 1 : 0;
}

int dkg_debug_plan_envelope(const void* host_plan, int out[4]) {
  if (!host_plan || !out) {
    failf(DKG_ERR_ARG, "dkg_debug_plan_envelope: NULL pointer");
    return -2;
  }
  const Plan& h = *static_cast<const Plan*>(host_plan);
  out[0] = h.stream ? 0 : env_slots(h.N + 1);
  out[1] = h.stream ? 1 : 0;
  out[2] = h.sw;
  out[3] = h.split;
  return 0;
}

int dkg_debug_plan_qx32(const void* host_plan, int output, int B, float* host_out, void* stream) {
  if (!host_plan || !host_out) return failf(DKG_ERR_ARG, "dkg_debug_plan_qx32: NULL pointer");
  const Plan& h = *static_cast<const Plan*>(host_plan);
  if (!h.f32) return failf(DKG_ERR_UNSUPPORTED, "dkg_debug_plan_qx32: the plan has no fp32 Q_X (DKG_PLAN_F32 only)");
  if (output < 0 || output >= h.m || B < 1 || B > h.max_B)
    return failf(DKG_ERR_ARG, "dkg_debug_plan_qx32: output=%d outside [0, %d) or B=%d outside [1, %d]", output, h.m, B,
                h.max_B);
  const int rows = pad16(B), np = pad16(h.o[output].n), KB = np / 4;
  std::vector<float> packed((size_t)rows * np);
  hipStream_t s = (hipStream_t)stream;
  int st;
  if ((st = hip_status(hipMemcpyAsync(packed.data(), h.q32[output], packed.size() * sizeof(float),
                                      hipMemcpyDeviceToHost, s), "hipMemcpyAsync(q32)")) ||
      (st = hip_status(hipStreamSynchronize(s), "hipStreamSynchronize")))
    return st;
  // element (16 t + (l & 15), 4 kb + (l >> 4)) sits at frag32_index(t, kb, l, KB)
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < np; ++c)
      host_out[(size_t)r * np + c] = packed[frag32_index(r >> 4, c >> 2, ((c & 3) << 4) | (r & 15), KB)];
  return DKG_OK;
}

int dkg_debug_f32_dispatch(int max_n_pad, int d, int N, int m, int B, int geom_B, int out[6]) {
  if (!out || max_n_pad < 16 || max_n_pad > 1024 || max_n_pad % 16 != 0 || d < 1 || d > DKG_MAX_DIM || N < 0 ||
      m < 1 || m > DKG_MAX_OUTPUTS || B < 1 || geom_B < 0) {
    failf(DKG_ERR_ARG, "dkg_debug_f32_dispatch: max_n_pad=%d d=%d N=%d m=%d B=%d geom_B=%d out=%s", max_n_pad, d, N, m,
          B, geom_B, out ? "set" : "NULL");
    return -2;
  }
  f32_dispatch(max_n_pad, d, N, m, B, geom_B, out);
  return 0;
}

int dkg_debug_envelope_lds(int m, int N, int waves, int S, int d, int max_np, int grad, int stream, int grows,
                           int out[DKG_ENV_LDS_REGIONS + 1]) {
  if (!out) return failf(DKG_ERR_ARG, "dkg_debug_envelope_lds: out is NULL");
  if (m < 1 || m > DKG_MAX_OUTPUTS || N < 0 || N > (1 << 22) || waves < 1 || waves > 8 || S < 1 ||
      (long long)S * m > (1 << 24) || d < 1 || d > DKG_MAX_DIM || max_np < 16 || max_np > 1024 || max_np % 16 != 0)
    return failf(DKG_ERR_ARG, "dkg_debug_envelope_lds: m=%d N=%d waves=%d S=%d d=%d max_np=%d", m, N, waves, S, d,
                 max_np);
  if (grows && !(grad && stream))
    return failf(DKG_ERR_ARG, "dkg_debug_envelope_lds: global rows are the streaming gradient envelope's alone");
  envelope_lds_regions(m, N, waves, S, d, max_np, grad != 0, stream != 0, grows != 0, out);
  return DKG_OK;
}

int dkg_debug_envelope_deal(int L, int nitems, int groups, int* item, int* member) {
  if (!item || !member || nitems < 1 || groups < 1 ||
      8ll * groups * (((long long)nitems + 7) / 8) > 0x7fffffffll || L < 0 || L >= xcd_group_size(nitems, groups)) {
    failf(DKG_ERR_ARG, "dkg_debug_envelope_deal: L=%d nitems=%d groups=%d item=%s member=%s", L, nitems, groups,
          item ? "set" : "NULL", member ? "set" : "NULL");
    return -2;
  }
  return xcd_deal(L, nitems, groups, *item, *member) ? 1 : 0;
}

int dkg_debug_wave_ops(const double* in, double* out, void* stream) {
  if (!in || !out) return failf(DKG_ERR_ARG, "NULL pointer");
  return hip_status(launch_debug_wave(in, out, (hipStream_t)stream), "debug_wave_kernel");
}

int dkg_debug_mfma_f64(const double* a, const double* b, double* c, void* stream) {
  if (!a || !b || !c) return failf(DKG_ERR_ARG, "NULL pointer");
  return hip_status(launch_debug_mfma(a, b, c, (hipStream_t)stream), "debug_mfma_kernel");
}

}  // extern "C"
