// ba.hip — bundle adjustment on the GPU: Optimizer::LocalBundleAdjustment (orb_slam2/src/mapping/optimizer.cpp:445-774) and
// Optimizer::BundleAdjustment (:51-229), monocular edges.  The arithmetic, the order of every sum and the stale-error rule are
// include/spfe_ba_math.h; the host statement the tests hold this kernel to is tests/ba_ref/ba_ref.c.
//
// The structure is dust.hip's, pose.hip's and sim3opt.hip's: ONE workgroup of 256 threads per problem and the whole Levenberg
// schedule inside one launch, __syncthreads() the only synchronisation (no grid barrier, no spin, no cooperative launch).
//   * Who owns what.  The robust chi2: edge e belongs to thread e % 256 (the contract's slot).  Hll / bl / Dinv / xl of point p:
//     thread p % 256, which walks the point's edges in order (the list is sorted by point, so they are one range).  Hpp / bp of an
//     unknown keyframe: the whole workgroup over that keyframe's edge list, position r on thread r % 256, the 27 sums through the
//     reduce-scatter butterfly and the four wavefronts in order.  The reduced system: the threads are cut in groups of G = 256 /
//     n_act, group a walks keyframe a's list and each of its threads owns fixed entries (r, c) of the 6 x 6 blocks of block row a
//     and of bs_a — an entry is only ever touched by its owner, in list order, so no atomics and no barrier inside the walk.
//     The Cholesky factorisation is right-looking (a column's division, then the trailing update: two barriers a column), the
//     two substitutions column-oriented (one barrier a step); per entry that is the contract's order.
//   * The keyframes' edge lists are built once in the prologue: a stable counting sort, 256 edges at a time.
//   * LDS: poses and their backups, Hpp | bp, bs, z, x, the diagonal of L, the partial sums, the per-keyframe tables — and the
//     reduced system itself while 6 n_free squared doubles fit behind them; it lies in scratch (L2-resident) otherwise, as do
//     the per-point and per-edge arrays.  The arithmetic does not depend on where the system lies.
#include <climits>
#include <type_traits>

#include "../../include/spfe_ba_math.h"
#include "../../include/spfe.h"
#include "spfe_kernels.h"
#include "wave_ops.h"

namespace spfe {

namespace {
constexpr int BA_THREADS = 256;
constexpr int KF = SPFE_BA_MAX_KEYFRAMES, FREE = SPFE_BA_MAX_FREE, NMAX = 6 * FREE;
constexpr int NPOSE = SPFE_BA_NPOSE;
static_assert(BA_THREADS == SPFE_DUST_SLOTS, "the contract's slot is the thread");
static_assert(KF == BA_MAX_KEYFRAMES, "BaArgs::base");
// doubles: pose[KF][7] | bak[KF][7] | Hpp[FREE][27] | bs | z | x | diag [NMAX] each | part[2][4][32] | misc[8]
constexpr size_t BA_LDS_DOUBLES = 2 * KF * 7 + FREE * NPOSE + 4 * NMAX + 256 + 8;
// ints: act | cnt | tot | cur | K | fix [KF] each | off[KF + 4] | kfa[FREE] | blk[512] | misc[16]
constexpr size_t BA_LDS_INTS = 6 * KF + KF + 4 + FREE + 512 + 16;
constexpr size_t BA_LDS_FIXED = (BA_LDS_DOUBLES * 8 + BA_LDS_INTS * 4 + 15) / 16 * 16;
constexpr size_t BA_LDS_MAX = 160 * 1024;
constexpr int ba_cap() {
  int c = 0;
  while (c < FREE && BA_LDS_FIXED + (size_t)36 * (c + 1) * (c + 1) * 8 <= BA_LDS_MAX) ++c;
  return c;
}
constexpr int BA_LDS_CAP = ba_cap();

struct Scratch {
  double *cur, *bak, *Hll, *bl, *Dinv, *W, *chi2, *Hs;
  float *obs;
  int *first, *last, *list, *pact, *eact;
  unsigned char *level;
};
__host__ __device__ inline size_t scratch_carve(unsigned char *b, int n, int E, Scratch *s) {
  const size_t np = (size_t)(n > 0 ? n : 1), ne = (size_t)(E > 0 ? E : 1);
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o = pad16(o + bytes); return at; };
  const size_t o_cur = take(np * 24), o_bak = take(np * 24), o_hll = take(np * 48), o_bl = take(np * 24), o_di = take(np * 48),
               o_w = take(ne * 144), o_chi = take(ne * 8), o_hs = take((size_t)NMAX * NMAX * 8), o_obs = take(ne * 16),
               o_first = take(np * 4), o_last = take(np * 4), o_list = take(ne * 4), o_pact = take(np * 4), o_eact = take(ne * 4), o_lv = take(ne);
  if (s) {
    s->cur = reinterpret_cast<double *>(b + o_cur); s->bak = reinterpret_cast<double *>(b + o_bak);
    s->Hll = reinterpret_cast<double *>(b + o_hll); s->bl = reinterpret_cast<double *>(b + o_bl);
    s->Dinv = reinterpret_cast<double *>(b + o_di); s->W = reinterpret_cast<double *>(b + o_w);
    s->chi2 = reinterpret_cast<double *>(b + o_chi); s->Hs = reinterpret_cast<double *>(b + o_hs);
    s->obs = reinterpret_cast<float *>(b + o_obs);
    s->first = reinterpret_cast<int *>(b + o_first); s->last = reinterpret_cast<int *>(b + o_last);
    s->list = reinterpret_cast<int *>(b + o_list); s->pact = reinterpret_cast<int *>(b + o_pact);
    s->eact = reinterpret_cast<int *>(b + o_eact);
    s->level = b + o_lv;
  }
  return o;
}

__device__ __forceinline__ void get_pose(const double *d, spfe_se3 &T) {
#pragma unroll
  for (int j = 0; j < 4; ++j) T.q[j] = d[j];
#pragma unroll
  for (int j = 0; j < 3; ++j) T.t[j] = d[4 + j];
}
__device__ __forceinline__ void put_pose(double *d, const spfe_se3 &T) {
#pragma unroll
  for (int j = 0; j < 4; ++j) d[j] = T.q[j];
#pragma unroll
  for (int j = 0; j < 3; ++j) d[4 + j] = T.t[j];
}
constexpr unsigned char LV_SKIPPED = 255;
}  // namespace

__global__ __launch_bounds__(BA_THREADS) void ba_kernel(BaArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double *s_pose = reinterpret_cast<double *>(smem_b);
  double *s_bak = s_pose + KF * 7;
  double *s_Hpp = s_bak + KF * 7;
  double *s_bs = s_Hpp + FREE * NPOSE;
  double *s_z = s_bs + NMAX;
  double *s_x = s_z + NMAX;
  double *s_diag = s_x + NMAX;
  double *s_part = s_diag + NMAX;   // [2][4][32]
  int *s_act = reinterpret_cast<int *>(s_part + 256 + 8);   // unknown number a of keyframe k in this round, or -1
  int *s_cnt = s_act + KF;                           // active edges of keyframe k in this round
  int *s_tot = s_cnt + KF;                           // served edges of keyframe k
  int *s_cur = s_tot + KF;
  int *s_K = s_cur + KF;
  int *s_fix = s_K + KF;
  int *s_off = s_fix + KF;                           // [KF + 1] list offsets
  int *s_kfa = s_off + KF + 4;                       // keyframe of unknown a
  int *s_blk = s_kfa + FREE;                         // [512]
  int *s_int = s_blk + 512;                          // [16]
  enum { I_STATUS = 0, I_UNSORTED, I_SERVED, I_NACTE, I_NACT, I_STOP, I_SPARE, I_COUNT, I_BASE, I_W0, I_W1, I_W2, I_W3, I_NFREE };

  const int n_kf = a.n_kf, n = a.n, E = a.E;
  Scratch sc;
  scratch_carve(a.scratch, n, E, &sc);
  unsigned char *out = a.out;
  int *hdr = reinterpret_cast<int *>(out);
  double *dout = reinterpret_cast<double *>(out + SPFE_BA_OFF_CHI2);
  float *Tcw_o = reinterpret_cast<float *>(out + SPFE_BA_OFF_TCW);
  float *xyz_o = reinterpret_cast<float *>(out + SPFE_BA_OFF_XYZ(n_kf));
  unsigned char *verdict = out + SPFE_BA_OFF_VERDICT(n_kf, n);
  int *erase = reinterpret_cast<int *>(out + SPFE_BA_OFF_ERASE(n_kf, n, E));
  const bool records = a.off_hdr >= 0;
  const bool local = a.schedule == SPFE_BA_LOCAL;
  const double fx = a.fx, fy = a.fy, cx = a.cx, cy = a.cy;
  const double w_full = (double)a.inv_sigma2_full;

  // ---- prologue: poses, flags, the records' K and status
  if (tid < 16) s_int[tid] = 0;
  __syncthreads();
  if (tid < KF) {
    s_tot[tid] = 0; s_cur[tid] = 0; s_cnt[tid] = 0; s_act[tid] = -1; s_K[tid] = 0; s_fix[tid] = 1;
    if (tid < n_kf) {
      spfe_se3 T;
      float Tf[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) Tf[k] = a.Tcw[16 * tid + k];
      spfe_se3_from_f32(Tf, &T);
      put_pose(s_pose + 7 * tid, T);
      s_fix[tid] = a.fixed[tid] != 0;
      if (records) {
        const int *h = reinterpret_cast<const int *>(a.base[tid] + a.off_hdr);
        s_K[tid] = min(max(h[0], 0), a.kmax);
        if (h[2]) atomicOr(&s_int[I_STATUS], h[2]);
      } else {
        s_K[tid] = INT_MAX;
      }
      if (!s_fix[tid]) atomicAdd(&s_int[I_NFREE], 1);
    }
  }
  if (tid == 0 && a.stop && *reinterpret_cast<const volatile int *>(a.stop) != 0) s_int[I_STOP] = 1;
  for (int p = tid; p < n; p += BA_THREADS) {
    sc.first[p] = INT_MAX;
    sc.last[p] = -1;
    sc.pact[p] = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) sc.cur[3 * p + c] = (double)a.xyz[3 * p + c];
  }
  block_fence_sync();
  const int n_free = s_int[I_NFREE];
  int status = s_int[I_STATUS];
  if (local && (status & SPFE_STATUS_COV_OVERFLOW)) status |= SPFE_BA_STATUS_COV_OVERFLOW;
  if (s_int[I_STOP]) status |= SPFE_BA_STATUS_STOPPED_EARLY;
  if (n_free > FREE) status |= SPFE_BA_STATUS_TOO_MANY_FREE;

  // ---- the served edges, their ranges per point, sortedness: thread t walks edges [t C, (t + 1) C) in order
  {
    const int C = (E + BA_THREADS - 1) / BA_THREADS;
    const int e0 = min(tid * C, E), e1 = min(e0 + C, E);
    int prev = -1, firstp = INT_MAX, served_n = 0, unsorted = 0;
    for (int e = e0; e < e1; ++e) {
      const int p = a.edges[3 * e], k = a.edges[3 * e + 1], kp = a.edges[3 * e + 2];
      const bool served = p >= 0 && p < n && k >= 0 && k < n_kf && kp >= 0 && kp < s_K[k];
      sc.level[e] = served ? 0 : LV_SKIPPED;
      sc.chi2[e] = 0.0;
      if (!served) continue;
      float ox, oy, w0 = 0.0f, w1 = 0.0f;
      if (records) {
        const float *xy = reinterpret_cast<const float *>(a.base[k] + a.off_xy);
        ox = xy[2 * kp]; oy = xy[2 * kp + 1];
        if (local) {
          const float *ci = reinterpret_cast<const float *>(a.base[k] + a.off_cinv);
          w0 = ci[2 * kp]; w1 = ci[2 * kp + 1];
        }
      } else {
        ox = a.obs_xy[2 * e]; oy = a.obs_xy[2 * e + 1];
        if (local) { w0 = a.inv_sigma2[2 * e]; w1 = a.inv_sigma2[2 * e + 1]; }
      }
      sc.obs[4 * e] = ox; sc.obs[4 * e + 1] = oy; sc.obs[4 * e + 2] = w0; sc.obs[4 * e + 3] = w1;
      if (p < prev) unsorted = 1;
      prev = p;
      if (firstp == INT_MAX) firstp = p;
      atomicMin(&sc.first[p], e);
      atomicMax(&sc.last[p], e);
      atomicAdd(&s_tot[k], 1);
      served_n++;
    }
    s_blk[2 * tid] = firstp;
    s_blk[2 * tid + 1] = prev;
    if (unsorted) atomicOr(&s_int[I_UNSORTED], 1);
    if (served_n) atomicAdd(&s_int[I_SERVED], served_n);
    block_fence_sync();
    if (tid == 0) {
      int last = -1, bad = 0;
      for (int t = 0; t < BA_THREADS; ++t) {
        if (s_blk[2 * t] == INT_MAX) continue;
        if (s_blk[2 * t] < last) bad = 1;
        last = s_blk[2 * t + 1];
      }
      if (bad) s_int[I_UNSORTED] = 1;
      int o = 0;
      for (int k = 0; k < KF; ++k) { s_off[k] = o; o += s_tot[k]; }
      s_off[KF] = o;
    }
    block_fence_sync();
  }
  if (s_int[I_UNSORTED]) status |= SPFE_BA_STATUS_UNSORTED;
  const int n_served = s_int[I_SERVED];

  if (status & (SPFE_BA_STATUS_COV_OVERFLOW | SPFE_BA_STATUS_STOPPED_EARLY | SPFE_BA_STATUS_TOO_MANY_FREE | SPFE_BA_STATUS_UNSORTED)) {
    for (int i = tid; i < 16 * n_kf; i += BA_THREADS) Tcw_o[i] = a.Tcw[i];
    for (int i = tid; i < 3 * n; i += BA_THREADS) xyz_o[i] = a.xyz[i];
    for (int e = tid; e < E; e += BA_THREADS) verdict[e] = SPFE_BA_SKIPPED;
    if (tid == 0) {
      hdr[0] = n_kf; hdr[1] = n_free; hdr[2] = n; hdr[3] = E;
      for (int k = 4; k < 11; ++k) hdr[k] = 0;
      hdr[11] = status;
      dout[0] = 0.0; dout[1] = 0.0; dout[2] = 0.0;
    }
    return;
  }

  // ---- the keyframes' edge lists: stable counting sort, 256 edges at a time
  for (int c0 = 0; c0 < E; c0 += BA_THREADS) {
    const int e = c0 + tid;
    const int k = (e < E && sc.level[e] != LV_SKIPPED) ? a.edges[3 * e + 1] : -1;
    s_blk[tid] = k;
    __syncthreads();
    if (k >= 0) {
      int rank = 0;
      for (int j = 0; j < tid; ++j) rank += s_blk[j] == k;
      sc.list[s_off[k] + s_cur[k] + rank] = e;
    }
    __syncthreads();
    if (k >= 0) atomicAdd(&s_cur[k], 1);
    __syncthreads();
  }
  block_fence_sync();

  auto edge_obs = [&](int e, double &ox, double &oy, double &w0, double &w1) {
    const float4 o = *reinterpret_cast<const float4 *>(sc.obs + 4 * e);
    ox = (double)o.x; oy = (double)o.y;
    if (local) { w0 = (double)o.z; w1 = (double)o.w; }
    else { w0 = w_full; w1 = w_full; }
  };
  auto point_of = [&](int p, double (&X)[3]) { X[0] = sc.cur[3 * p]; X[1] = sc.cur[3 * p + 1]; X[2] = sc.cur[3 * p + 2]; };

  int set = 0;
  // the tree over this thread's slot sum; every thread gets the total
  auto tree_total = [&](double v) -> double {
    v = wave_tree(v);
    double *part = s_part + set * 128;
    if (lane == 0) part[wave * 32] = v;
    __syncthreads();
    const double t = sum4_ordered(part, 32);
    set ^= 1;
    return t;
  };
  // computeActiveErrors + activeRobustChi2 at the estimate
  auto errors_and_chi = [&](int robust, double delta) -> double {
    double v = 0.0;
    for (int e = tid; e < E; e += BA_THREADS) {
      if (sc.level[e] != 0) continue;
      const int p = a.edges[3 * e], k = a.edges[3 * e + 1];
      spfe_se3 T;
      get_pose(s_pose + 7 * k, T);
      double X[3], ox, oy, w0, w1;
      point_of(p, X);
      edge_obs(e, ox, oy, w0, w1);
      const double chi = spfe_ba_edge_chi2(&T, X, fx, fy, cx, cy, ox, oy, w0, w1);
      sc.chi2[e] = chi;
      v += spfe_ba_rho0(chi, robust, delta);
    }
    return tree_total(v);
  };
  // linearize + the quadratic forms; returns the largest |diagonal| of Hpp and Hll
  auto build = [&](int robust, double delta, int n_act) -> double {
    double md = 0.0;
    for (int p = tid; p < n; p += BA_THREADS) {
      const int l = sc.last[p];
      int active = 0;
      double h[SPFE_BA_NPOINT];
#pragma unroll
      for (int j = 0; j < SPFE_BA_NPOINT; ++j) h[j] = 0.0;
      double X[3];
      point_of(p, X);
      for (int e = sc.first[p]; e <= l; ++e) {
        if (sc.level[e] != 0) continue;
        active = 1;
        const int k = a.edges[3 * e + 1];
        spfe_se3 T;
        get_pose(s_pose + 7 * k, T);
        double ox, oy, w0, w1, B0[3], B1[3], t[SPFE_BA_NPOINT];
        edge_obs(e, ox, oy, w0, w1);
        spfe_ba_edge g;
        spfe_ba_edge_eval(&T, X, fx, fy, cx, cy, ox, oy, w0, w1, robust, delta, &g);
        spfe_ba_point_jacobian(T.q, g.p, fx, fy, B0, B1);
        spfe_ba_point_terms(&g, B0, B1, t);
#pragma unroll
        for (int j = 0; j < SPFE_BA_NPOINT; ++j) h[j] += t[j];
        if (s_act[k] >= 0) {
          double A0[6], A1[6], W[18];
          spfe_pose_jacobian(g.p, fx, fy, A0, A1);
          spfe_ba_w(&g, A0, A1, B0, B1, W);
#pragma unroll
          for (int j = 0; j < 18; ++j) sc.W[(size_t)18 * e + j] = W[j];
        }
      }
      sc.pact[p] = active;
      if (active) {
#pragma unroll
        for (int j = 0; j < 6; ++j) sc.Hll[6 * p + j] = h[j];
#pragma unroll
        for (int j = 0; j < 3; ++j) sc.bl[3 * p + j] = h[6 + j];
        md = fmax(md, fmax(fabs(h[0]), fmax(fabs(h[2]), fabs(h[5]))));
      }
    }
    for (int ai = 0; ai < n_act; ++ai) {
      const int k = s_kfa[ai];
      const int lo = s_off[k], len = s_off[k + 1] - lo;
      spfe_se3 T;
      get_pose(s_pose + 7 * k, T);
      double v[32];
#pragma unroll
      for (int j = 0; j < 32; ++j) v[j] = 0.0;
      for (int r = tid; r < len; r += BA_THREADS) {
        const int e = sc.list[lo + r];
        if (sc.level[e] != 0) continue;
        const int p = a.edges[3 * e];
        double X[3], ox, oy, w0, w1, A0[6], A1[6], q[NPOSE];
        point_of(p, X);
        edge_obs(e, ox, oy, w0, w1);
        spfe_ba_edge g;
        spfe_ba_edge_eval(&T, X, fx, fy, cx, cy, ox, oy, w0, w1, robust, delta, &g);
        spfe_pose_jacobian(g.p, fx, fy, A0, A1);
        spfe_ba_pose_terms(&g, A0, A1, q);
#pragma unroll
        for (int j = 0; j < NPOSE; ++j) v[j] += q[j];
      }
      wave_tree_scatter32(v, lane);
      double *part = s_part + set * 128;
      if (!(lane & 1)) part[wave * 32 + (lane >> 1)] = v[0];
      __syncthreads();
      if (tid < NPOSE) s_Hpp[ai * NPOSE + tid] = sum4_ordered(part + tid, 32);
      set ^= 1;
    }
    block_fence_sync();
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) md = fmax(md, xchg(md, m));
    double *part = s_part + set * 128;
    if (lane == 0) part[wave * 32] = md;
    __syncthreads();
    md = fmax(fmax(part[0], part[32]), fmax(part[64], part[96]));
    set ^= 1;
    for (int ai = 0; ai < n_act; ++ai) {
      const double *H = s_Hpp + ai * NPOSE;
      md = fmax(md, fmax(fmax(fabs(H[0]), fabs(H[2])), fmax(fmax(fabs(H[5]), fabs(H[9])), fmax(fabs(H[14]), fabs(H[20])))));
    }
    return md;
  };

  // one trial's linear solve at lambda: Dinv, the reduced system, Cholesky, the substitutions; x in s_x; returns solved or not
  auto solve = [&](double lambda, int n_act, auto in_lds_tag) -> bool {
    // the system's home, named so that the LDS instantiation addresses LDS directly
    double *Hs;
    if constexpr (decltype(in_lds_tag)::value) Hs = reinterpret_cast<double *>(smem_b + BA_LDS_FIXED);
    else Hs = sc.Hs;
    const int nd = 6 * n_act;
    for (int p = tid; p < n; p += BA_THREADS) {
      if (!sc.pact[p]) continue;
      double h[6], Di[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) h[j] = sc.Hll[6 * p + j];
      spfe_ba_inv3(h, lambda, Di);
#pragma unroll
      for (int j = 0; j < 6; ++j) sc.Dinv[6 * p + j] = Di[j];
    }
    if (nd == 0) {
      block_fence_sync();
      return true;
    }
    for (int i = tid; i < nd * nd; i += BA_THREADS) Hs[i] = 0.0;
    block_fence_sync();
    for (int i = tid; i < n_act * 36; i += BA_THREADS) {
      const int ai = i / 36, r = (i % 36) / 6, c = i % 6;
      const int hi = r > c ? r : c, lo = r > c ? c : r;
      Hs[(size_t)(6 * ai + r) * nd + 6 * ai + c] = s_Hpp[ai * NPOSE + hi * (hi + 1) / 2 + lo] + (r == c ? lambda : 0.0);
    }
    for (int i = tid; i < nd; i += BA_THREADS) s_bs[i] = s_Hpp[(i / 6) * NPOSE + 21 + i % 6];
    block_fence_sync();
    {
      int G = BA_THREADS / n_act;
      G = G > 42 ? 42 : G;
      const int ai = tid / G, g = tid % G;
      if (ai < n_act) {
        const int k = s_kfa[ai];
        const int lo = s_off[k], hi = s_off[k + 1];
        for (int r = lo; r < hi; ++r) {
          const int e = sc.list[r];
          if (sc.eact[e] != ai) continue;   // not active in this round
          const int p = a.edges[3 * e];
          double Di[6], blp[3];
#pragma unroll
          for (int j = 0; j < 6; ++j) Di[j] = sc.Dinv[6 * p + j];
#pragma unroll
          for (int j = 0; j < 3; ++j) blp[j] = sc.bl[3 * p + j];
          const int f = sc.first[p], l = sc.last[p];
          // the point's edges eight at a time: their unknowns first (independent loads), then per owned entry the rows of W
          for (int e2 = f; e2 <= l; e2 += 8) {
            int a2s[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const int a2 = e2 + j <= l ? sc.eact[e2 + j] : -2;
              a2s[j] = a2 <= ai ? a2 : -2;
            }
            for (int idx = g; idx < 42; idx += G) {
              const int rr = idx < 36 ? idx / 6 : idx - 36;
              const double *Wr = sc.W + (size_t)18 * e + 3 * rr;
              const double Wrow[3] = {Wr[0], Wr[1], Wr[2]};
              double Y[3];
              spfe_ba_y_row(Wrow, Di, Y);
              if (idx >= 36) {
                if (e2 == f) s_bs[6 * ai + rr] -= spfe_ba_dot3(Y, blp);
              } else {
                const int c = idx % 6;
                double w2[8][3];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                  if (a2s[j] < 0) continue;
                  const double *W2 = sc.W + (size_t)18 * (e2 + j) + 3 * c;
                  w2[j][0] = W2[0]; w2[j][1] = W2[1]; w2[j][2] = W2[2];
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                  if (a2s[j] < 0) continue;
                  Hs[(size_t)(6 * ai + rr) * nd + 6 * a2s[j] + c] -= spfe_ba_dot3(Y, w2[j]);
                }
              }
            }
          }
        }
      }
    }
    block_fence_sync();
    // Cholesky, right-looking; the diagonal of L in s_diag
    bool ok = true;
    for (int kc = 0; kc < nd; ++kc) {
      const double d = Hs[(size_t)kc * nd + kc];
      if (!spfe_ba_pivot_ok(d)) { ok = false; break; }   // the same value in every thread
      const double ldiag = sqrt(d);
      if (tid == 0) s_diag[kc] = ldiag;
      for (int i = kc + 1 + tid; i < nd; i += BA_THREADS) Hs[(size_t)i * nd + kc] = Hs[(size_t)i * nd + kc] / ldiag;
      block_fence_sync();
      for (int i = kc + 1 + wave; i < nd; i += 4) {
        const double lik = Hs[(size_t)i * nd + kc];
        for (int j = kc + 1 + lane; j <= i; j += 64) Hs[(size_t)i * nd + j] -= lik * Hs[(size_t)j * nd + kc];
      }
      block_fence_sync();
    }
    if (!ok) {
      block_fence_sync();
      return false;
    }
    for (int kc = 0; kc < nd; ++kc) {
      const double zk = s_bs[kc] / s_diag[kc];
      if (tid == 0) s_z[kc] = zk;
      for (int i = kc + 1 + tid; i < nd; i += BA_THREADS) s_bs[i] -= Hs[(size_t)i * nd + kc] * zk;
      block_fence_sync();
    }
    for (int kc = nd - 1; kc >= 0; --kc) {
      const double xk = s_z[kc] / s_diag[kc];
      if (tid == 0) s_x[kc] = xk;
      for (int i = tid; i < kc; i += BA_THREADS) s_z[i] -= Hs[(size_t)kc * nd + i] * xk;
      block_fence_sync();
    }
    return true;
  };

  int stopped_late = 0;
  double chi_entry = 0.0, chi_exit = 0.0, lambda_out = 0.0;
  bool chi_entry_set = false;
  // initializeOptimization(level 0) + optimize(iterations): the iterations run, the trials into *trials
  auto optimize = [&](int robust, double delta, int iterations, int *trials) -> int {
    *trials = 0;
    // the round's active edges per keyframe, its unknowns
    if (tid < KF) s_cnt[tid] = 0;
    if (tid == 0) s_int[I_NACTE] = 0;
    __syncthreads();
    {
      int mine = 0;
      for (int e = tid; e < E; e += BA_THREADS)
        if (sc.level[e] == 0) { atomicAdd(&s_cnt[a.edges[3 * e + 1]], 1); mine++; }
      if (mine) atomicAdd(&s_int[I_NACTE], mine);
    }
    __syncthreads();
    if (tid == 0) {
      int na = 0;
      for (int k = 0; k < KF; ++k) {
        const bool unknown = k < n_kf && !s_fix[k] && s_cnt[k] > 0;
        s_act[k] = unknown ? na : -1;
        if (unknown) s_kfa[na++] = k;
      }
      s_int[I_NACT] = na;
    }
    __syncthreads();
    const int n_act = s_int[I_NACT];
    // per edge: its keyframe's unknown number, -1 for an active edge of a keyframe that is none, -2 when not active
    for (int e = tid; e < E; e += BA_THREADS) sc.eact[e] = sc.level[e] == 0 ? s_act[a.edges[3 * e + 1]] : -2;
    block_fence_sync();
    if (s_int[I_NACTE] == 0) return 0;
    const int nd = 6 * n_act;
    const bool in_lds = n_free <= BA_LDS_CAP;
    spfe_lm lm;
    lm.lambda = 0.0; lm.ni = 2.0;
    int it_done = 0, n_trials = 0;
    bool fresh = false, go = iterations > 0;
    double currentChi = 0.0;
    for (int it = 0; it < iterations && go; ++it) {
      if (a.stop) {   // terminate(): the flag, read once before the iteration
        __syncthreads();
        if (tid == 0) s_int[I_STOP] = *reinterpret_cast<const volatile int *>(a.stop) != 0;
        __syncthreads();
        if (s_int[I_STOP]) { stopped_late = 1; break; }
      }
      if (!fresh) currentChi = errors_and_chi(robust, delta);
      if (!chi_entry_set) { chi_entry = currentChi; chi_entry_set = true; }
      const double md = build(robust, delta, n_act);
      if (it == 0) {
        lm.lambda = SPFE_LM_TAU * md;
        lm.ni = 2;
      }
      double rho = 0;
      int qmax = 0;
      do {
        const bool ok = in_lds ? solve(lm.lambda, n_act, std::true_type{}) : solve(lm.lambda, n_act, std::false_type{});
        // the update: points by their owners (with the landmark part of the scale), poses by one thread each
        double vl = 0.0, vp = 0.0;
        if (ok) {
          for (int p = tid; p < n; p += BA_THREADS) {
            if (!sc.pact[p]) continue;
            double t[3], Di[6], bl3[3], xl[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) { bl3[j] = sc.bl[3 * p + j]; t[j] = bl3[j]; }
#pragma unroll
            for (int j = 0; j < 6; ++j) Di[j] = sc.Dinv[6 * p + j];
            const int l = sc.last[p];
            for (int e = sc.first[p]; e <= l; ++e) {
              const int a2 = sc.eact[e];
              if (a2 < 0) continue;
              double W[18], x6[6];
#pragma unroll
              for (int j = 0; j < 18; ++j) W[j] = sc.W[(size_t)18 * e + j];
#pragma unroll
              for (int j = 0; j < 6; ++j) x6[j] = s_x[6 * a2 + j];
#pragma unroll
              for (int c = 0; c < 3; ++c) t[c] -= spfe_ba_wtx(W, x6, c);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              double row[3];
              spfe_ba_sym_row(Di, c, row);
              xl[c] = spfe_ba_dot3(row, t);
            }
            vl += (spfe_ba_scale_term(xl[0], lm.lambda, bl3[0]) + spfe_ba_scale_term(xl[1], lm.lambda, bl3[1])) +
                  spfe_ba_scale_term(xl[2], lm.lambda, bl3[2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const double old = sc.cur[3 * p + c];
              sc.bak[3 * p + c] = old;
              sc.cur[3 * p + c] = old + xl[c];
            }
          }
          for (int j = tid; j < nd; j += BA_THREADS)
            vp += spfe_ba_scale_term(s_x[j], lm.lambda, s_Hpp[(j / 6) * NPOSE + 21 + j % 6]);
          if (tid < n_act) {
            const int k = s_kfa[tid];
            spfe_se3 T;
            get_pose(s_pose + 7 * k, T);
            put_pose(s_bak + 7 * k, T);
            double x6[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) x6[j] = s_x[6 * tid + j];
            spfe_se3_oplus(&T, x6);
            put_pose(s_pose + 7 * k, T);
          }
        }
        block_fence_sync();
        double sum = 0.0;
        if (ok) {
          const double Sp = tree_total(vp);
          const double Sl = tree_total(vl);
          sum = Sp + Sl;
        }
        const double chiT = errors_and_chi(robust, delta);
        const double tempChi = ok ? chiT : SPFE_BA_DBL_MAX;
        fresh = spfe_ba_lm_judge(&lm, currentChi, tempChi, sum, &rho) != 0;
        if (fresh) {
          currentChi = tempChi;
        } else if (ok) {   // pop: the estimates come back, the edges keep the candidate's errors
          for (int p = tid; p < n; p += BA_THREADS) {
            if (!sc.pact[p]) continue;
#pragma unroll
            for (int c = 0; c < 3; ++c) sc.cur[3 * p + c] = sc.bak[3 * p + c];
          }
          if (tid < n_act) {
            const int k = s_kfa[tid];
#pragma unroll
            for (int j = 0; j < 7; ++j) s_pose[7 * k + j] = s_bak[7 * k + j];
          }
        }
        block_fence_sync();
        qmax++;
        n_trials++;
      } while (rho < 0 && qmax < SPFE_LM_MAX_TRIALS);
      it_done++;
      if (qmax == SPFE_LM_MAX_TRIALS || rho == 0) go = false;
    }
    block_fence_sync();
    chi_exit = currentChi;
    lambda_out = lm.lambda;
    *trials = n_trials;
    return it_done;
  };

  // chi2 > 5.991 || !isDepthPositive on the errors the edge holds and the estimate as it stands
  auto edge_bad = [&](int e) -> bool {
    const int p = a.edges[3 * e], k = a.edges[3 * e + 1];
    spfe_se3 T;
    get_pose(s_pose + 7 * k, T);
    double X[3];
    point_of(p, X);
    return sc.chi2[e] > SPFE_BA_CHI2 || !(spfe_ba_depth(&T, X) > 0.0);
  };

  int iters[2] = {0, 0}, trials[2] = {0, 0}, n_level1 = 0, n_erase = 0;
  if (local) {
    iters[0] = optimize(1, SPFE_POSE_DELTA, a.it0, &trials[0]);
    if (!stopped_late && a.stop) {   // bDoMore
      __syncthreads();
      if (tid == 0) s_int[I_STOP] = *reinterpret_cast<const volatile int *>(a.stop) != 0;
      __syncthreads();
      stopped_late = s_int[I_STOP];
    }
    if (!stopped_late) {
      if (tid == 0) s_int[I_COUNT] = 0;
      __syncthreads();
      int mine = 0;
      for (int e = tid; e < E; e += BA_THREADS) {
        if (sc.level[e] != 0) continue;
        if (edge_bad(e)) { sc.level[e] = 1; mine++; }
      }
      if (mine) atomicAdd(&s_int[I_COUNT], mine);
      block_fence_sync();
      n_level1 = s_int[I_COUNT];
      iters[1] = optimize(0, 0.0, a.it1, &trials[1]);
    }
  } else {
    iters[0] = optimize(a.robust != 0, SPFE_BA_DELTA_FULL, a.it0, &trials[0]);
  }
  block_fence_sync();

  // the final test, the verdicts and the erase list in edge order
  if (tid == 0) s_int[I_BASE] = 0;
  __syncthreads();
  for (int c0 = 0; c0 < E; c0 += BA_THREADS) {
    const int e = c0 + tid;
    bool er = false;
    if (e < E) {
      const unsigned char lv = sc.level[e];
      unsigned char v = SPFE_BA_SKIPPED;
      if (lv != LV_SKIPPED) {
        er = local && edge_bad(e);
        v = er ? SPFE_BA_ERASE : (lv == 1 ? SPFE_BA_LEVEL1_KEPT : SPFE_BA_INLIER);
      }
      verdict[e] = v;
    }
    const unsigned long long m = __ballot(er);
    const int below = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_int[I_W0 + wave] = __popcll(m);
    __syncthreads();
    int off = s_int[I_BASE];
    for (int w = 0; w < wave; ++w) off += s_int[I_W0 + w];
    if (er) erase[off + below] = e;
    const int total = s_int[I_W0] + s_int[I_W1] + s_int[I_W2] + s_int[I_W3];
    __syncthreads();
    if (tid == 0) s_int[I_BASE] += total;
  }
  __syncthreads();
  n_erase = s_int[I_BASE];

  if (tid < n_kf) {
    float Tf[16];
    if (s_fix[tid]) {
#pragma unroll
      for (int k = 0; k < 16; ++k) Tf[k] = a.Tcw[16 * tid + k];
    } else {
      spfe_se3 T;
      get_pose(s_pose + 7 * tid, T);
      spfe_se3_to_f32(&T, Tf);
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) Tcw_o[16 * tid + k] = Tf[k];
  }
  for (int i = tid; i < 3 * n; i += BA_THREADS) xyz_o[i] = (float)sc.cur[i];
  if (tid == 0) {
    hdr[0] = n_kf; hdr[1] = n_free; hdr[2] = n; hdr[3] = E; hdr[4] = n_served;
    hdr[5] = iters[0]; hdr[6] = iters[1]; hdr[7] = trials[0]; hdr[8] = trials[1];
    hdr[9] = n_level1; hdr[10] = n_erase;
    hdr[11] = status | (stopped_late ? SPFE_BA_STATUS_STOPPED : 0);
    dout[0] = chi_entry; dout[1] = chi_exit; dout[2] = lambda_out;
  }
}

size_t ba_scratch_bytes(int n, int E) { return scratch_carve(nullptr, n, E, nullptr); }

int ba_lds_free_capacity() { return BA_LDS_CAP; }

hipError_t launch_ba(const BaArgs &a, hipStream_t s) {
  if (a.n_kf < 1 || a.n_kf > KF || a.n < 0 || a.n > SPFE_BA_MAX_POINTS || a.E < 0 || a.E > SPFE_BA_MAX_EDGES)
    return hipErrorInvalidValue;
  static LdsLimitOnce lds_once;   // (spfe_kernels.h)
  if (hipError_t e = raise_lds_limit(lds_once, reinterpret_cast<const void *>(ba_kernel), (int)BA_LDS_MAX); e != hipSuccess) return e;
  // the reduced system of up to BA_LDS_CAP free keyframes in LDS; a problem with more keeps it in scratch and asks for none
  const size_t lds = BA_LDS_FIXED + (size_t)36 * BA_LDS_CAP * BA_LDS_CAP * 8;
  hipLaunchKernelGGL(ba_kernel, dim3(1), dim3(BA_THREADS), lds, s, a);
  return hipGetLastError();
}

}  // namespace spfe
