// The space dominated by a point set, cut into disjoint boxes, and its volume (gfx950, fp64, m <= 3 maximised
// objectives).  The specification is in include/dkg.h ("Dominated-space boxes"); DESIGN.md 8g.  JES takes the boxes
// (BoTorch's DominatedPartitioning in the reference, jes_sample_pareto.py:235-347), the BO metrics the volume
// (botorch_hypervolume.py).  One sweep serves m = 1, 2 and 3 through three internal axes:
//
//   x  the strip axis   y_0
//   y  the floor axis   y_1 at m = 3, else the constant 1 over the reference 0
//   z  the level axis   y_2 at m = 3, y_1 at m = 2, else the constant 1 over the reference 0
//
// Level order is z descending, then index ascending; at m < 3 x descending comes before the index, so that of two
// staircase candidates of equal height the outer one is first and the inner one finds itself covered.  Point p
// walks the qualifying points by x descending (ties: y, then z descending, then index: equal pairs in level order)
// and looks only at the points before it in level order.  `cur` is the right edge of the strip being cut (p_x at
// the start), `M` the floor (ref_y at the start).  A visited point above the floor is a staircase point: if it lies
// left of `cur` it closes the strip (e_x, cur] x (M, p_y]; then M = e_y.  The walk ends when the floor reaches p_y,
// or at the end of the list with the strip (ref_x, cur] x (M, p_y].  Every corner is a copy of an input or of ref.
//
//   boxes_order_kernel   grid (64 points, sample), 4 waves: wave w counts over the w-th quarter of the set the keys
//                        before each point's own (pareto_order_kernel's counting ranks), then scatters the point to
//                        its x rank, its level to slvl and its x rank to lrank[level].
//   boxes_hv_kernel      one lane per x rank: the walk, acc = fma(width, height, acc) per strip in walk order, then
//                        hvp[rank] = acc (p_z - ref_z).  The list entry of a step is the same for the whole wave.
//   boxes_sum_kernel     one workgroup per sample: hv = sum hvp, lane t over t, t + 1024, ... then a binary tree.
//   boxes_write_kernel   one workgroup per sample, two consecutive levels per thread: the walk counts, an LDS
//                        prefix sum places, the walk again writes (strips reversed: ascending x), the rest of the J
//                        rows are [0, 0] boxes.
//
// No atomics, no workgroup waits on another, every loop is bounded by K or J, every sum runs in a fixed order that
// depends on the sample's qualifying points only.
#include <cmath>

#include "dkg_acq.h"
#include "dkg_stages.h"

namespace dkg {

constexpr int BX_ORDER_WAVES = 4;   // slices of the counting loop
constexpr int BX_THREADS = 1024;    // boxes_sum_kernel, boxes_write_kernel
constexpr int BX_CHUNK = 8;         // list entries a walk loads at a time
constexpr int BX_PER_THREAD = DKG_BOXES_MAX_POINTS / BX_THREADS;  // levels per thread of boxes_write_kernel
static_assert(BX_PER_THREAD * BX_THREADS == DKG_BOXES_MAX_POINTS, "levels per thread");
static_assert(2 * DKG_BOXES_MAX_POINTS - 1 <= DKG_JES_MAX_BOXES, "count bound of the largest set");

struct BoxWs {
  size_t sx, sy, sz, hvp, slvl, lrank, nq, total;  // byte offsets; per sample K entries each, nq one
};

BoxWs box_ws(int S, int K) {
  BoxWs w;
  const size_t n = (size_t)S * K;
  Carve c;  // the sections follow each other as they are; the end is rounded to 256
  w.sx = c.take(n * sizeof(double), 1);
  w.sy = c.take(n * sizeof(double), 1);
  w.sz = c.take(n * sizeof(double), 1);
  w.hvp = c.take(n * sizeof(double), 1);
  w.slvl = c.take(n * sizeof(int), 1);
  w.lrank = c.take(n * sizeof(int), 1);
  w.nq = c.take((size_t)S * sizeof(int));
  w.total = c.total();
  return w;
}

struct BoxArgs {
  const double* Y;  // [S][K][m]
  int K, m;
  double rx, ry, rz;  // the reference point on the internal axes
  double* sx;         // [S][K] by x rank
  double* sy;
  double* sz;
  double* hvp;        // [S][K] by x rank: the volume only this point dominates among those up to its level
  int* slvl;          // [S][K] by x rank: the level
  int* lrank;         // [S][K] by level: the x rank
  int* nq;            // [S] qualifying points
  double* hv;         // [S]
  double* bounds;     // [S][2][J][m]
  int* count;         // [S]
  int J;
};

struct BoxPt {
  double x, y, z;
};

__device__ inline BoxPt box_load(const double* __restrict__ Y, int m, int row) {
  const double* p = Y + (size_t)row * m;
  BoxPt r;
  r.x = p[0];
  r.y = m == 3 ? p[1] : 1.0;
  r.z = m == 3 ? p[2] : (m == 2 ? p[1] : 1.0);
  return r;
}

__device__ inline bool box_qualifies(const BoxPt& p, const BoxArgs& a) {
  return p.x > a.rx && p.y > a.ry && p.z > a.rz;  // false for NaN
}

__global__ __launch_bounds__(BX_ORDER_WAVES * WAVE) void boxes_order_kernel(BoxArgs a) {
  __shared__ int c_lvl[BX_ORDER_WAVES][WAVE], c_rank[BX_ORDER_WAVES][WAVE], c_q[BX_ORDER_WAVES];
  const int s = blockIdx.y, lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  const int K = a.K, m = a.m;
  const int i = blockIdx.x * WAVE + lane;
  const double* __restrict__ Y = a.Y + (size_t)s * K * m;
  const BoxPt p = box_load(Y, m, i < K ? i : 0);
  const bool xtie = m < 3;
  const int per = (K + BX_ORDER_WAVES - 1) / BX_ORDER_WAVES;
  const int j0 = w * per, j1 = min(K, j0 + per);
  int lvl = 0, rank = 0, q = 0;
#pragma unroll 4
  for (int j = j0; j < j1; ++j) {
    const BoxPt e = box_load(Y, m, j);
    if (!box_qualifies(e, a)) continue;
    ++q;
    const bool first = j < i;
    const bool before_lvl = e.z > p.z || (e.z == p.z && (xtie ? (e.x > p.x || (e.x == p.x && first)) : first));
    const bool before_x =
        e.x > p.x || (e.x == p.x && (e.y > p.y || (e.y == p.y && (e.z > p.z || (e.z == p.z && first)))));
    lvl += before_lvl;
    rank += before_x;
  }
  c_lvl[w][lane] = lvl;
  c_rank[w][lane] = rank;
  if (lane == 0) c_q[w] = q;
  __syncthreads();
  if (w != 0) return;
  lvl = rank = q = 0;
  for (int k = 0; k < BX_ORDER_WAVES; ++k) {
    lvl += c_lvl[k][lane];
    rank += c_rank[k][lane];
    q += c_q[k];
  }
  if (blockIdx.x == 0 && lane == 0) a.nq[s] = q;
  if (i < K && box_qualifies(p, a)) {  // lvl and rank are below q <= K, each taken by one point
    const size_t o = (size_t)s * K;
    a.sx[o + rank] = p.x;
    a.sy[o + rank] = p.y;
    a.sz[o + rank] = p.z;
    a.slvl[o + rank] = lvl;
    a.lrank[o + lvl] = rank;
  }
}

// The walk of point (px, py) of level plvl over the Q list entries; strip(lo, hi, floor) per strip with an
// interior, by descending x.  Called by whole waves: `live` masks the lanes without a point.
template <class F>
__device__ inline void box_walk(const double* __restrict__ sx, const double* __restrict__ sy,
                                const int* __restrict__ slvl, int Q, bool live, double px, double py, int plvl,
                                double rx, double ry, F&& strip) {
  double cur = px, M = ry;
  auto visit = [&](double ex, double ey, int el) {
    if (live && el < plvl && ey > M) {
      if (ex < cur) {
        strip(ex, cur, M);
        cur = ex;
      }
      M = ey;
      live = M < py;
    }
  };
  int j = 0;
  for (; j + BX_CHUNK <= Q; j += BX_CHUNK) {  // the entries of a chunk are loaded together, ahead of their use
    if (__all(!live)) return;
    double ex[BX_CHUNK], ey[BX_CHUNK];
    int el[BX_CHUNK];
#pragma unroll
    for (int u = 0; u < BX_CHUNK; ++u) {
      ex[u] = sx[j + u];
      ey[u] = sy[j + u];
      el[u] = slvl[j + u];
    }
#pragma unroll
    for (int u = 0; u < BX_CHUNK; ++u) visit(ex[u], ey[u], el[u]);
  }
  for (; j < Q; ++j) visit(sx[j], sy[j], slvl[j]);
  if (live) strip(rx, cur, M);
}

__global__ __launch_bounds__(WAVE) void boxes_hv_kernel(BoxArgs a) {
  const int s = blockIdx.y, K = a.K;
  const int r = blockIdx.x * WAVE + threadIdx.x;
  const size_t o = (size_t)s * K;
  const int Q = a.nq[s];
  const bool live = r < Q;
  const int rr = live ? r : 0;
  const double px = a.sx[o + rr], py = a.sy[o + rr], pz = a.sz[o + rr];
  const int plvl = a.slvl[o + rr];
  double acc = 0.0;
  box_walk(a.sx + o, a.sy + o, a.slvl + o, Q, live, px, py, plvl, a.rx, a.ry,
           [&](double lo, double hi, double fl) { acc = fma(hi - lo, py - fl, acc); });
  if (r < K) a.hvp[o + r] = live ? acc * (pz - a.rz) : 0.0;
}

__global__ __launch_bounds__(BX_THREADS) void boxes_sum_kernel(BoxArgs a) {
  __shared__ double red[BX_THREADS];
  const int s = blockIdx.x, t = threadIdx.x;
  const double* __restrict__ v = a.hvp + (size_t)s * a.K;
  double acc = 0.0;
  for (int i = t; i < a.K; i += BX_THREADS) acc += v[i];
  red[t] = acc;
  __syncthreads();
  for (int off = BX_THREADS / 2; off > 0; off >>= 1) {
    if (t < off) red[t] += red[t + off];
    __syncthreads();
  }
  if (t == 0) a.hv[s] = red[0];
}

__global__ __launch_bounds__(BX_THREADS) void boxes_write_kernel(BoxArgs a) {
  __shared__ int scan[BX_THREADS];
  const int s = blockIdx.x, t = threadIdx.x, K = a.K, m = a.m, J = a.J;
  const size_t o = (size_t)s * K;
  const int Q = a.nq[s];
  const double* __restrict__ sx = a.sx + o;
  const double* __restrict__ sy = a.sy + o;
  const int* __restrict__ slvl = a.slvl + o;
  double px[BX_PER_THREAD], py[BX_PER_THREAD], pz[BX_PER_THREAD];
  int cnt[BX_PER_THREAD], mine = 0;
#pragma unroll
  for (int u = 0; u < BX_PER_THREAD; ++u) {
    const int l = t * BX_PER_THREAD + u;
    const bool live = l < Q;
    const int r = live ? a.lrank[o + l] : 0;
    px[u] = sx[r];
    py[u] = sy[r];
    pz[u] = a.sz[o + r];
    int c = 0;
    box_walk(sx, sy, slvl, Q, live, px[u], py[u], l, a.rx, a.ry, [&](double, double, double) { ++c; });
    cnt[u] = c;
    mine += c;
  }
  scan[t] = mine;
  __syncthreads();
  for (int off = 1; off < BX_THREADS; off <<= 1) {
    const int v = t >= off ? scan[t - off] : 0;
    __syncthreads();
    scan[t] += v;
    __syncthreads();
  }
  const int total = scan[BX_THREADS - 1];
  int base = scan[t] - mine;
  double* lo_rows = a.bounds + (size_t)s * 2 * J * m;
  double* hi_rows = lo_rows + (size_t)J * m;
#pragma unroll
  for (int u = 0; u < BX_PER_THREAD; ++u) {
    const int l = t * BX_PER_THREAD + u;
    int row = base + cnt[u] - 1;  // the walk cuts by descending x; the rows ascend
    const double hy = py[u], hz = pz[u];
    box_walk(sx, sy, slvl, Q, l < Q, px[u], hy, l, a.rx, a.ry, [&](double lo, double hi, double fl) {
      if (row >= 0 && row < J) {
        double* L = lo_rows + (size_t)row * m;
        double* H = hi_rows + (size_t)row * m;
        L[0] = lo;
        H[0] = hi;
        if (m == 3) {
          L[1] = fl;
          H[1] = hy;
        }
        if (m >= 2) {
          L[m - 1] = a.rz;
          H[m - 1] = hz;
        }
      }
      --row;
    });
    base += cnt[u];
  }
  for (int row = total + t; row < J; row += BX_THREADS)
    for (int c = 0; c < m; ++c) lo_rows[(size_t)row * m + c] = hi_rows[(size_t)row * m + c] = 0.0;
  if (t == 0) a.count[s] = min(total, J);
}

}  // namespace dkg

using namespace dkg;

namespace {

int box_check(const char* what, const void* Y, const void* ref, const void* out, const void* out2, const void* work,
              int S, int K, int m, int k_max) {
  if (!Y || !ref || !out || !out2 || !work) return failf(DKG_ERR_ARG, "%s: NULL pointer", what);
  if (S < 1 || K < 1 || m < 1) return failf(DKG_ERR_ARG, "%s: S=%d sets of K=%d points, m=%d objectives", what, S, K, m);
  if (m > 3) return failf(DKG_ERR_UNSUPPORTED, "%s: m=%d objectives (supported 1..3)", what, m);
  if (K > k_max) return failf(DKG_ERR_UNSUPPORTED, "%s: K=%d points (supported <= %d)", what, K, k_max);
  if (S > 65535) return failf(DKG_ERR_UNSUPPORTED, "%s: S=%d sets (supported <= 65535)", what, S);
  return DKG_OK;
}

bool box_sizes_ok(int S, int K, int m, int k_max) {
  return S >= 1 && S <= 65535 && K >= 1 && K <= k_max && m >= 1 && m <= 3;
}

BoxArgs box_args(const double* Y, int S, int K, int m, const double* ref, void* work) {
  const BoxWs w = box_ws(S, K);
  BoxArgs a{};
  a.Y = Y;
  a.K = K;
  a.m = m;
  a.rx = ref[0];
  a.ry = m == 3 ? ref[1] : 0.0;
  a.rz = m == 3 ? ref[2] : (m == 2 ? ref[1] : 0.0);
  a.sx = at<double>(work, w.sx);
  a.sy = at<double>(work, w.sy);
  a.sz = at<double>(work, w.sz);
  a.hvp = at<double>(work, w.hvp);
  a.slvl = at<int>(work, w.slvl);
  a.lrank = at<int>(work, w.lrank);
  a.nq = at<int>(work, w.nq);
  return a;
}

int box_order(const BoxArgs& a, int S, hipStream_t s) {
  hipLaunchKernelGGL(boxes_order_kernel, dim3((a.K + WAVE - 1) / WAVE, S), dim3(BX_ORDER_WAVES * WAVE), 0, s, a);
  return hip_status(hipGetLastError(), "boxes_order_kernel");
}

int box_count_bound(int K, int m) { return m == 1 ? 1 : (m == 2 ? K : 2 * K - 1); }

}  // namespace

extern "C" {

size_t dkg_dominated_boxes_workspace(int S, int K, int m) {
  return box_sizes_ok(S, K, m, DKG_BOXES_MAX_POINTS) ? box_ws(S, K).total : 0;
}

int dkg_dominated_boxes(const double* Y, int S, int K, int m, const double* ref_point, int J, double* bounds,
                        int* count, void* work, size_t work_bytes, void* stream) {
  int st = box_check("dkg_dominated_boxes", Y, ref_point, bounds, count, work, S, K, m, DKG_BOXES_MAX_POINTS);
  if (st) return st;
  if (J > DKG_JES_MAX_BOXES)
    return failf(DKG_ERR_UNSUPPORTED, "dkg_dominated_boxes: J=%d boxes (supported <= %d)", J, DKG_JES_MAX_BOXES);
  if (J < box_count_bound(K, m))
    return failf(DKG_ERR_ARG, "dkg_dominated_boxes: J=%d rows < %d, the most boxes K=%d points of m=%d objectives give",
                 J, box_count_bound(K, m), K, m);
  const BoxWs w = box_ws(S, K);
  if (work_bytes < w.total)
    return failf(DKG_ERR_WORKSPACE, "dkg_dominated_boxes: workspace %zu bytes < required %zu", work_bytes, w.total);
  BoxArgs a = box_args(Y, S, K, m, ref_point, work);
  a.bounds = bounds;
  a.count = count;
  a.J = J;
  hipStream_t s = (hipStream_t)stream;
  st = box_order(a, S, s);
  if (st) return st;
  hipLaunchKernelGGL(boxes_write_kernel, dim3(S), dim3(BX_THREADS), 0, s, a);
  return hip_status(hipGetLastError(), "boxes_write_kernel");
}

size_t dkg_hypervolume_front_workspace(int S, int K, int m) {
  return box_sizes_ok(S, K, m, DKG_HV_FRONT_MAX_POINTS) ? box_ws(S, K).total : 0;
}

int dkg_hypervolume_front(const double* Y, int S, int K, int m, const double* ref_point, double* hv, void* work,
                          size_t work_bytes, void* stream) {
  int st = box_check("dkg_hypervolume_front", Y, ref_point, hv, hv, work, S, K, m, DKG_HV_FRONT_MAX_POINTS);
  if (st) return st;
  const BoxWs w = box_ws(S, K);
  if (work_bytes < w.total)
    return failf(DKG_ERR_WORKSPACE, "dkg_hypervolume_front: workspace %zu bytes < required %zu", work_bytes, w.total);
  BoxArgs a = box_args(Y, S, K, m, ref_point, work);
  a.hv = hv;
  hipStream_t s = (hipStream_t)stream;
  st = box_order(a, S, s);
  if (st) return st;
  hipLaunchKernelGGL(boxes_hv_kernel, dim3((K + WAVE - 1) / WAVE, S), dim3(WAVE), 0, s, a);
  st = hip_status(hipGetLastError(), "boxes_hv_kernel");
  if (st) return st;
  hipLaunchKernelGGL(boxes_sum_kernel, dim3(S), dim3(BX_THREADS), 0, s, a);
  return hip_status(hipGetLastError(), "boxes_sum_kernel");
}

}  // extern "C"
