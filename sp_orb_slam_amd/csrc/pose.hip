// pose.hip — covariance-weighted pose refinement on the GPU: the pose-only optimisations that consume the covariance
// stage's cov2_inv (Optimizer::PoseOptimizationDustPost, orb_slam2/src/mapping/optimizer_dust.cpp:35-167, and
// Optimizer::PoseOptimization, mapping/optimizer.cpp:231-443).  The arithmetic is include/spfe_pose_math.h; the host
// statement the tests hold this kernel to is tests/pose_ref/pose_ref.c.
//
// The structure is dust.hip's (read its header comment): ONE workgroup of 256 threads per solve, the latency of one trial
// step is what is optimised.
//   * Edge j (ascending keypoint index) belongs to thread j % 256 — the contract's slot.  Two kinds of phase, each ending
//     in ONE barrier: a trial's computeActiveErrors (the robust chi2 through the tree; every edge also stores the float
//     chi2 g2o would hold for it, which the classification of PoseOptimization reads for its inliers — possibly the error
//     of a rejected last trial) and an iteration's buildSystem (error + Jacobian per edge, the 27 entries of H's lower
//     triangle and b through the reduce-scatter butterfly, then the four wavefronts in order).  The Jacobians are formed
//     once per iteration, and the errors at the start of an iteration are skipped after an accepted trial (same pose,
//     same bits).
//   * The 6x6 L D L^T solve + exponential map run on the four wavefronts for the next four candidate lambdas at once.
//   * Edges.  The prologue compacts the keypoints that have a map point into the edge list (ballot + popcount per 256
//     keypoints, in order).  Per edge the LDS holds its keypoint index, its level and its float chi2 (9 B: 10,001 edges =
//     90 KB); when the edge data (observation, information, world point: 28 B) fits beside that it is staged in LDS too
//     (the tracker's sizes: ~1,000 edges = 28 KB), otherwise every evaluation re-reads it from the record and the point
//     array (L2-resident).
//   * Records with SPFE_STATUS_COV_OVERFLOW carry invalid cov2_inv: refused (pose echoed, counts 0, status bit).
#include "../../include/spfe_pose_math.h"
#include "../../include/spfe.h"
#include "spfe_kernels.h"
#include "wave_ops.h"

namespace spfe {

namespace {
constexpr int POSE_THREADS = 256;
constexpr int NSUM = SPFE_POSE_NSUM;
constexpr size_t POSE_LDS_FIXED = (2 * 4 * 32 + 4 * 16) * sizeof(double) + 64;  // partial sums | candidates | counters
constexpr size_t POSE_LDS_MAX = 160 * 1024;
static_assert(POSE_THREADS == SPFE_DUST_SLOTS, "the contract's slot is the thread");

// LDS layout for kmax keypoints: fixed | chi2f[kmax] | kp[kmax] | level[kmax] | edge data (7 floats SoA) [cap]
__host__ __device__ inline size_t pose_data_off(int kmax) { return pad16(POSE_LDS_FIXED + (size_t)kmax * 9); }
// edges whose data fits in an allocation of lds_bytes (the kernel's in-LDS test and pose_lds_edge_capacity share this)
__host__ __device__ inline int pose_edge_cap(size_t lds_bytes, int kmax) { return (int)((lds_bytes - pose_data_off(kmax)) / 28); }
}  // namespace

__global__ __launch_bounds__(POSE_THREADS) void pose_refine_kernel(PoseArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_p[];
  {
    const size_t f = blockIdx.x;
    a.kp_xy = reinterpret_cast<const float *>(reinterpret_cast<const char *>(a.kp_xy) + f * a.rec_stride);
    a.cinv = reinterpret_cast<const float *>(reinterpret_cast<const char *>(a.cinv) + f * a.rec_stride);
    if (a.hdr) a.hdr = reinterpret_cast<const int *>(reinterpret_cast<const char *>(a.hdr) + f * a.rec_stride);
    if (a.mp_of_kp) a.mp_of_kp = reinterpret_cast<const int *>(reinterpret_cast<const char *>(a.mp_of_kp) + f * a.map_stride);
    a.pts = reinterpret_cast<const float *>(reinterpret_cast<const char *>(a.pts) + f * a.pts_stride);
    a.Tcw_in = reinterpret_cast<const float *>(reinterpret_cast<const char *>(a.Tcw_in) + f * a.pose_stride);
    a.out = a.out + f * a.out_stride;
  }
  double *s_part = reinterpret_cast<double *>(smem_p);
  double *s_cand = s_part + 2 * 4 * 32;
  int *s_int = reinterpret_cast<int *>(s_cand + 4 * 16);   // [0..3] wavefront counts, [5] bad count
  float *s_chi2 = reinterpret_cast<float *>(smem_p + POSE_LDS_FIXED);
  int *s_kp = reinterpret_cast<int *>(s_chi2 + a.kmax);
  unsigned char *s_lvl = reinterpret_cast<unsigned char *>(s_kp + a.kmax);
  float *s_dat = reinterpret_cast<float *>(smem_p + pose_data_off(a.kmax));
  const int cap = pose_edge_cap(a.lds_bytes, a.kmax);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kmax = a.kmax;

  float *Tout = reinterpret_cast<float *>(a.out);
  int *cnt = reinterpret_cast<int *>(a.out + 64);   // n_initial, n_good, iterations[4], status, verdict, n_matches
  unsigned char *outlier = a.out + SPFE_POSE_OFF_OUTLIER;
  const int K = a.hdr ? min(max(a.hdr[0], 0), kmax) : a.k_imm;
  const int status = a.hdr ? a.hdr[2] : 0;
  const bool chain = a.gate_inliers != nullptr;

  for (int i = tid; i < kmax; i += POSE_THREADS) outlier[i] = 0;   // mvbOutlier of keypoints without an edge
  // the pose written when nothing is optimised (or, in the chained form, when a gate fails)
  auto finish_echo = [&](const float *Tsrc, int n_initial, int st, int verdict, int n_matches) {
    if (tid < 16) Tout[tid] = Tsrc[tid];
    if (tid == 0) {
      cnt[0] = n_initial; cnt[1] = 0; cnt[2] = cnt[3] = cnt[4] = cnt[5] = 0;
      cnt[6] = st; cnt[7] = verdict; cnt[8] = n_matches;
    }
  };
  if (status & SPFE_STATUS_COV_OVERFLOW) {
    finish_echo(chain ? a.Tcw_echo : a.Tcw_in, 0, SPFE_POSE_STATUS_COV_OVERFLOW, chain ? SPFE_TRACK_FAIL_COV : 0, 0);
    return;
  }
  if (chain && a.gate_inliers[0] < a.th_ninlier) {   // tracker_dust.cpp:97-102
    finish_echo(a.Tcw_echo, 0, 0, SPFE_TRACK_FAIL_INLIERS, 0);
    return;
  }

  // ---- the edge list: keypoints with a map point, ascending
  int n = 0;   // the edges of the chunks below this one (the same in every thread)
  for (int c = 0; c < K; c += POSE_THREADS) {
    const int kp = c + tid;
    bool has = kp < K;
    if (has && a.mp_of_kp) {
      const int mp = a.mp_of_kp[kp];
      has = mp >= 0 && (a.n_pts < 0 || mp < a.n_pts);
    }
    int total;
    const int rank = wg_ordered_rank<POSE_THREADS>(has, lane, wave, s_int, &total);
    if (has) s_kp[n + rank] = kp;
    n += total;
    __syncthreads();   // s_int is rewritten by the next chunk; behind the last one s_kp is whole
  }
  const bool in_lds = n <= cap;
  for (int j = tid; j < n; j += POSE_THREADS) {
    s_lvl[j] = 0;
    s_chi2[j] = 0.0f;
    if (in_lds) {
      const int kp = s_kp[j], mp = a.mp_of_kp ? a.mp_of_kp[kp] : kp;
      s_dat[j] = a.kp_xy[2 * kp];
      s_dat[cap + j] = a.kp_xy[2 * kp + 1];
      s_dat[2 * cap + j] = a.cinv[2 * kp];
      s_dat[3 * cap + j] = a.cinv[2 * kp + 1];
      s_dat[4 * cap + j] = a.pts[3 * mp];
      s_dat[5 * cap + j] = a.pts[3 * mp + 1];
      s_dat[6 * cap + j] = a.pts[3 * mp + 2];
    }
  }
  if (chain && n < a.th_nmatch) {   // tracker_dust.cpp:174-179
    finish_echo(a.Tcw_echo, 0, 0, SPFE_TRACK_FAIL_MATCHES, n);
    return;
  }
  if (n < 3) {   // nInitialCorrespondences < 3: return 0, the pose untouched
    const bool ok = chain && 0.0f / (float)n > a.th_ratio;   // tracker_dust.cpp:218 on nopt_inlier = 0
    finish_echo(chain && !ok ? a.Tcw_echo : a.Tcw_in, n, 0, chain ? (ok ? SPFE_TRACK_OK : SPFE_TRACK_FAIL_RATIO) : 0, n);
    return;
  }
  __syncthreads();

  const double fx = a.fx, fy = a.fy, cx = a.cx, cy = a.cy;
  // edge j: observation, information, world point
  auto load = [&](int j, double &ox, double &oy, double &w0, double &w1, double (&Xw)[3]) {
    if (in_lds) {
      ox = s_dat[j]; oy = s_dat[cap + j]; w0 = s_dat[2 * cap + j]; w1 = s_dat[3 * cap + j];
      Xw[0] = s_dat[4 * cap + j]; Xw[1] = s_dat[5 * cap + j]; Xw[2] = s_dat[6 * cap + j];
    } else {
      const int kp = s_kp[j], mp = a.mp_of_kp ? a.mp_of_kp[kp] : kp;
      ox = a.kp_xy[2 * kp]; oy = a.kp_xy[2 * kp + 1]; w0 = a.cinv[2 * kp]; w1 = a.cinv[2 * kp + 1];
      Xw[0] = a.pts[3 * mp]; Xw[1] = a.pts[3 * mp + 1]; Xw[2] = a.pts[3 * mp + 2];
    }
  };

  int robust = 1;
  int set = 0;
  // computeActiveErrors at Te + activeRobustChi2; every active edge keeps its float chi2
  auto errors_and_chi = [&](const spfe_se3 &Te) -> double {
    double v = 0.0;
    for (int j = tid; j < n; j += POSE_THREADS) {
      if (s_lvl[j]) continue;
      double ox, oy, w0, w1, Xw[3], p[3], e[2];
      load(j, ox, oy, w0, w1, Xw);
      spfe_pose_error(&Te, Xw, fx, fy, cx, cy, ox, oy, p, e);
      const double c = spfe_pose_chi2(e, w0, w1);
      s_chi2[j] = (float)c;
      v += spfe_pose_rho0(c, robust);
    }
    v = wave_tree(v);
    double *part = s_part + set * 128;
    if (lane == 0) part[wave * 32] = v;
    __syncthreads();
    const double chi = sum4_ordered(part, 32);
    set ^= 1;
    return chi;
  };
  // buildSystem at Te
  auto build = [&](const spfe_se3 &Te, double (&H)[36], double (&b)[6]) {
    double v[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) v[j] = 0.0;
    for (int j = tid; j < n; j += POSE_THREADS) {
      if (s_lvl[j]) continue;
      double ox, oy, w0, w1, Xw[3], p[3], e[2], A0[6], A1[6], q[NSUM];
      load(j, ox, oy, w0, w1, Xw);
      spfe_pose_error(&Te, Xw, fx, fy, cx, cy, ox, oy, p, e);
      spfe_pose_jacobian(p, fx, fy, A0, A1);
      spfe_pose_terms(e, A0, A1, w0, w1, robust, q);
#pragma unroll
      for (int k = 1; k < NSUM; ++k) v[k] += q[k];
    }
    wave_tree_scatter32(v, lane);
    double *part = s_part + set * 128;
    if (!(lane & 1)) part[wave * 32 + (lane >> 1)] = v[0];
    __syncthreads();
    const double mine = sum4_ordered(part + (lane & 31), 32);
    double tot[NSUM], chi_unused;
    tot[0] = 0.0;
#pragma unroll
    for (int k = 1; k < NSUM; ++k) tot[k] = bcast(mine, k);
    spfe_dust_unpack(tot, &chi_unused, H, b);
    set ^= 1;
  };
  // initializeOptimization(0); optimize(iterations) from T: the iterations run, 0 when no edge is at level 0 (g2o: -1)
  auto optimize = [&](spfe_se3 &T, int n_active) -> int {
    if (n_active == 0) return 0;
    spfe_lm lm;
    lm.lambda = 0.0; lm.ni = 2.0;
    int it_done = 0;
    bool fresh = false, go = a.iterations > 0;
    double currentChi = 0.0;
    for (int it = 0; it < a.iterations && go; ++it) {
      if (!fresh) currentChi = errors_and_chi(T);
      double H[36], b[6];
      build(T, H, b);
      if (it == 0) {
        double maxDiagonal = 0;
        for (int j = 0; j < 6; ++j) maxDiagonal = fabs(H[j * 6 + j]) > maxDiagonal ? fabs(H[j * 6 + j]) : maxDiagonal;
        lm.lambda = SPFE_LM_TAU * maxDiagonal;
        lm.ni = 2;
      }
      double rho = 0;
      int qmax = 0;
      do {
        if ((qmax & 3) == 0) {   // wavefront w: the step of the w-th trial from now, were all before it rejected
          double lam = lm.lambda, ni = lm.ni;
#pragma unroll
          for (int r = 0; r < 3; ++r)
            if (r < wave) { lam *= ni; ni *= 2; }
          double xc[6];
          spfe_se3 Tc = T;
          const int okc = spfe_solve6(H, lam, b, xc);
          if (okc) spfe_se3_oplus(&Tc, xc);
          if (lane == 0) {
            double *c = s_cand + wave * 16;
#pragma unroll
            for (int j = 0; j < 6; ++j) c[j] = xc[j];
#pragma unroll
            for (int j = 0; j < 4; ++j) c[6 + j] = Tc.q[j];
#pragma unroll
            for (int j = 0; j < 3; ++j) c[10 + j] = Tc.t[j];
            c[13] = okc ? 1.0 : 0.0;
          }
          __syncthreads();
        }
        double x[6];
        spfe_se3 Tt;
        const double *c = s_cand + (qmax & 3) * 16;
#pragma unroll
        for (int j = 0; j < 6; ++j) x[j] = c[j];
#pragma unroll
        for (int j = 0; j < 4; ++j) Tt.q[j] = c[6 + j];
#pragma unroll
        for (int j = 0; j < 3; ++j) Tt.t[j] = c[10 + j];
        const bool ok2 = c[13] != 0.0;
        const double chiT = errors_and_chi(Tt);
        const double tempChi = ok2 ? chiT : 1.7976931348623157e308;
        fresh = spfe_lm_judge(&lm, currentChi, tempChi, x, b, &rho) != 0;
        if (fresh) { currentChi = tempChi; T = Tt; }
        qmax++;
        // the candidates of the next group are written after this barrier-separated read (errors_and_chi's barrier
        // follows every thread's read of s_cand)
      } while (rho < 0 && qmax < SPFE_LM_MAX_TRIALS);
      it_done++;
      if (qmax == SPFE_LM_MAX_TRIALS || rho == 0) go = false;
    }
    __syncthreads();   // the next phase may rewrite s_cand / s_lvl
    return it_done;
  };
  // the classification after an optimize(): edges flagged `fresh` are evaluated at T first; returns nBad
  auto classify = [&](const spfe_se3 &T, bool post) -> int {
    int bad = 0;
    for (int j = tid; j < n; j += POSE_THREADS) {
      if (post || s_lvl[j]) {   // DustPost: computeError() on every edge; PoseOptimization: on the outliers only
        double ox, oy, w0, w1, Xw[3], p[3], e[2];
        load(j, ox, oy, w0, w1, Xw);
        spfe_pose_error(&T, Xw, fx, fy, cx, cy, ox, oy, p, e);
        s_chi2[j] = spfe_pose_chi2f(e, w0, w1);
      }
      const float chi2 = s_chi2[j];
      const int o = post ? ((double)chi2 > SPFE_POSE_CHI2_POST) : (chi2 > SPFE_POSE_CHI2_MONO);
      s_lvl[j] = (unsigned char)o;
      bad += o;
    }
    if (tid == 0) s_int[5] = 0;
    __syncthreads();
    if (bad) atomicAdd(&s_int[5], bad);
    __syncthreads();
    const int nb = s_int[5];
    __syncthreads();
    return nb;
  };

  spfe_se3 T;
  float Tin[16];
  for (int k = 0; k < 16; ++k) Tin[k] = a.Tcw_in[k];
  int iters[4] = {0, 0, 0, 0};
  int nBad = 0;
  if (a.schedule == SPFE_POSE_DUST_POST) {
    spfe_se3_from_f32(Tin, &T);
    iters[0] = optimize(T, n);
    nBad = classify(T, true);
    robust = 0;
    iters[1] = optimize(T, n - nBad);
  } else {
#pragma unroll 1
    for (int it = 0; it < 4; ++it) {
      spfe_se3_from_f32(Tin, &T);
      iters[it] = optimize(T, n - nBad);   // the edges at level 0: all in round 0, the inliers of the last round after
      nBad = classify(T, false);
      if (it == 2) robust = 0;
      if (n < 10) break;
    }
  }
  for (int j = tid; j < n; j += POSE_THREADS) outlier[s_kp[j]] = s_lvl[j];
  if (tid == 0) {
    const int n_good = n - nBad;
    int verdict = 0;
    bool echo = false;
    if (chain) {   // tracker_dust.cpp:218
      const bool ok = (float)n_good * 1.0f / (float)n > a.th_ratio;
      verdict = ok ? SPFE_TRACK_OK : SPFE_TRACK_FAIL_RATIO;
      echo = !ok;
    }
    float To[16];
    spfe_se3_to_f32(&T, To);
    for (int k = 0; k < 16; ++k) Tout[k] = echo ? a.Tcw_echo[k] : To[k];
    cnt[0] = n; cnt[1] = n_good;
    for (int k = 0; k < 4; ++k) cnt[2 + k] = iters[k];
    cnt[6] = 0; cnt[7] = verdict; cnt[8] = n;
  }
}

__global__ void pose_scatter_kernel(const int *kp_idx, int n, int *mp_of_kp, int kmax) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const int k = kp_idx[i];
    if (k >= 0 && k < kmax) mp_of_kp[k] = i;
  }
}

size_t pose_lds_bytes(int kmax) {
  const size_t want = pose_data_off(kmax) + (size_t)kmax * 28;
  return want < POSE_LDS_MAX ? want : POSE_LDS_MAX;
}

int pose_lds_edge_capacity(int kmax) {
  if (kmax < 1 || pose_data_off(kmax) > POSE_LDS_MAX) return -1;
  return pose_edge_cap(pose_lds_bytes(kmax), kmax);
}

hipError_t launch_pose_refine(const PoseArgs &a0, hipStream_t s) {
  PoseArgs a = a0;
  if (a.kmax < 1 || pose_data_off(a.kmax) > POSE_LDS_MAX) return hipErrorInvalidValue;
  a.lds_bytes = pose_lds_bytes(a.kmax);
  static LdsLimitOnce lds_once;   // (spfe_kernels.h)
  if (hipError_t e = raise_lds_limit(lds_once, reinterpret_cast<const void *>(pose_refine_kernel), (int)POSE_LDS_MAX); e != hipSuccess) return e;
  hipLaunchKernelGGL(pose_refine_kernel, dim3(a.nframes > 0 ? a.nframes : 1), dim3(POSE_THREADS), a.lds_bytes, s, a);
  return hipGetLastError();
}

hipError_t launch_pose_scatter(const int *kp_idx, int n, int *mp_of_kp, int kmax, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(pose_scatter_kernel, dim3((n + 255) / 256), dim3(256), 0, s, kp_idx, n, mp_of_kp, kmax);
  return hipGetLastError();
}

}  // namespace spfe
