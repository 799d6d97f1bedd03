// sim3opt.hip — the Sim3 optimisation of a loop hypothesis on the GPU (Optimizer::OptimizeSim3, orb_slam2/src/mapping/
// optimizer.cpp:1062-1252, as LoopClosingVLAD::ComputeSim3 calls it behind the guided match).  The arithmetic is
// include/spfe_sim3opt_math.h; the host statement the tests hold this kernel to is tests/sim3opt_ref/sim3opt_ref.c.
//
// The structure is dust.hip's and pose.hip's (read their header comments): ONE workgroup of 256 threads per solve, job q =
// blockIdx.x, and the latency of one trial step is what is optimised; the solves of a batched call run side by side.
//   * Term i (2 c for e12, 2 c + 1 for e21 of served correspondence c) belongs to thread i % 256 — the contract's slot — so an
//     even thread evaluates e12 edges only and an odd one e21 edges only.  Phases, each ending in ONE barrier: a trial's
//     computeActiveErrors (the robust chi2 through the tree; every edge also stores whether the chi2 g2o would hold for it
//     exceeds th2, which the classification reads — possibly of a rejected last trial), the 14 perturbed estimates of
//     linearizeOplus
//     (threads 0 .. 13, one each, with their inverses: they do not depend on the edge), and an iteration's buildSystem (per
//     edge the error and the 14 perturbed errors; the 35 entries of H's lower triangle and b go through the reduce-scatter
//     butterfly — 32 of them — and a plain butterfly — the last 3 — then the four wavefronts in order).
//   * The 7x7 L D L^T solve + exponential map + inverse run on the four wavefronts for the next four candidate lambdas at once.
//   * The prologue compacts the served correspondences in order (ballot + popcount per 256 keypoints) and forms P1c, P2c and
//     the observations once.  Per correspondence the LDS holds the alive flag and, per edge, whether the chi2 it holds exceeds
//     th2 (3 B: 32,767 keypoints = 98 KB; the classification needs no more of the stored errors); its keypoint is in the job's
//     scratch array.  When the edge data (10 floats) of all correspondences fits beside that it is staged in LDS too, otherwise
//     every evaluation reads it from the scratch array (L2-resident).  Both hold the same floats: the result does not depend
//     on which.
#include "../../include/spfe_sim3opt_math.h"
#include "../../include/spfe_sim3_math.h"
#include "../../include/spfe.h"
#include "spfe_kernels.h"
#include "wave_ops.h"

namespace spfe {

namespace {
constexpr int S3O_THREADS = 256;
constexpr int NSUM = SPFE_S3O_NSUM;
constexpr int CAND_D = 24;    // a candidate: x[7] | fwd q, t, s | inv q, t, s | ok
constexpr int SIM_D = 16;     // an estimate: fwd q, t, s | inv q, t, s
// partial sums (2 sets x 4 wavefronts x 36) | candidates | the estimate and its 14 perturbations | counters
constexpr size_t S3O_LDS_FIXED = (2 * 4 * NSUM + 4 * CAND_D + 15 * SIM_D) * sizeof(double) + 64;
constexpr size_t S3O_LDS_MAX = 160 * 1024;
constexpr int S3O_EDGE_FLOATS = 10;   // P1c[3] | P2c[3] | obs1[2] | obs2[2]
constexpr int S3O_MAX_KEYPOINTS = 32767;   // the host-array forms' limit; a handle's kmax is 10,001 at the most
static_assert(S3O_THREADS == SPFE_DUST_SLOTS, "the contract's slot is the thread");

// LDS layout for kmax keypoints: fixed | alive[kmax] | bad[2 kmax] | edge data (10 floats SoA) [cap]
__host__ __device__ inline size_t s3o_data_off(int kmax) { return pad16(S3O_LDS_FIXED + (size_t)kmax * 3); }
__host__ __device__ inline int s3o_edge_cap(size_t lds_bytes, int kmax) {
  return (int)((lds_bytes - s3o_data_off(kmax)) / (S3O_EDGE_FLOATS * 4));
}
static_assert(S3O_LDS_FIXED + (size_t)S3O_MAX_KEYPOINTS * 3 + 16 <= S3O_LDS_MAX, "S3O_MAX_KEYPOINTS");

__device__ __forceinline__ void put_sim(double *d, const spfe_s3o_sim &S) {
#pragma unroll
  for (int j = 0; j < 4; ++j) d[j] = S.q[j];
#pragma unroll
  for (int j = 0; j < 3; ++j) d[4 + j] = S.t[j];
  d[7] = S.s;
}
__device__ __forceinline__ void get_sim(const double *d, spfe_s3o_sim &S) {
#pragma unroll
  for (int j = 0; j < 4; ++j) S.q[j] = d[j];
#pragma unroll
  for (int j = 0; j < 3; ++j) S.t[j] = d[4 + j];
  S.s = d[7];
}
}  // namespace

__global__ __launch_bounds__(S3O_THREADS) void sim3opt_kernel(Sim3OptArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_s[];
  const int q = blockIdx.x, kmax = a.kmax;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double *s_part = reinterpret_cast<double *>(smem_s);
  double *s_cand = s_part + 2 * 4 * NSUM;
  double *s_sims = s_cand + 4 * CAND_D;
  int *s_int = reinterpret_cast<int *>(s_sims + 15 * SIM_D);   // [0..3] wavefront counts, [5] bad count
  unsigned char *s_alive = smem_s + S3O_LDS_FIXED;
  unsigned char *s_bad = s_alive + kmax;   // [2 c + kind]: the chi2 the edge holds exceeds th2
  float *s_dat = reinterpret_cast<float *>(smem_s + s3o_data_off(kmax));
  const int cap = s3o_edge_cap(a.lds_bytes, kmax);

  unsigned char *out = a.out + (size_t)q * SPFE_SIM3OPT_OUT_BYTES(kmax);
  int *cnt = reinterpret_cast<int *>(out);
  double *S12o = reinterpret_cast<double *>(out + SPFE_SIM3OPT_OFF_S12);
  float *T12o = reinterpret_cast<float *>(out + SPFE_SIM3OPT_OFF_T12);
  float *Scwo = reinterpret_cast<float *>(out + SPFE_SIM3OPT_OFF_SCW);
  int *m12o = reinterpret_cast<int *>(out + SPFE_SIM3OPT_OFF_MATCHES12);
  int *matched = reinterpret_cast<int *>(out + SPFE_SIM3OPT_OFF_MATCHED(kmax));
  unsigned char *verdict = out + SPFE_SIM3OPT_OFF_VERDICT(kmax);

  const int cj = a.cand[q];
  const unsigned char *rec2 = a.base2[q];
  const float *xy1 = reinterpret_cast<const float *>(a.base1 + a.off_xy);
  const float *xy2 = reinterpret_cast<const float *>(rec2 + a.off_xy);
  const int *hdr1 = a.off_hdr >= 0 ? reinterpret_cast<const int *>(a.base1 + a.off_hdr) : nullptr;
  const int *hdr2 = a.off_hdr >= 0 ? reinterpret_cast<const int *>(rec2 + a.off_hdr) : nullptr;
  const int K1 = hdr1 ? min(max(hdr1[0], 0), kmax) : a.k_imm1;
  const int K2 = hdr2 ? min(max(hdr2[0], 0), kmax) : a.k_imm2;
  const int status = (hdr1 ? hdr1[2] : 0) | (hdr2 ? hdr2[2] : 0);
  const int *mp1 = a.mp1;
  const int *mp2 = a.mp2 + (size_t)cj * kmax;
  const float *Tcw2p = a.Tcw2 + 16 * cj;
  const float *T12p = a.T12;
  const int *m12in = a.matches12;
  if (a.verify) {
    const unsigned char *vb = a.verify + (size_t)cj * SPFE_SIM3_OUT_BYTES(kmax, a.n_hyp);
    T12p = reinterpret_cast<const float *>(vb + SPFE_SIM3_OFF_T12(kmax, a.n_hyp)) + 13 * a.hyp[q];
    const unsigned char *gb = a.guided + (size_t)q * SPFE_GUIDED_OUT_BYTES(kmax);
    m12in = reinterpret_cast<const int *>(gb + SPFE_GUIDED_OFF_MATCHES12(kmax));
    const int gstatus = reinterpret_cast<const int *>(gb)[SPFE_GUIDED_OFF_STATUS / 4];
    if (gstatus & SPFE_GUIDED_STATUS_NOT_EVALUATED) {   // T12 of the verify block was never written
      for (int i = tid; i < kmax; i += S3O_THREADS) { m12o[i] = -1; matched[i] = -1; }
      if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) cnt[k] = 0;
        cnt[8] = status | SPFE_SIM3OPT_STATUS_NOT_EVALUATED;
      }
      return;
    }
  }
  float *g_dat = a.scratch + (size_t)q * (S3O_EDGE_FLOATS + 1) * kmax;
  int *g_k1 = reinterpret_cast<int *>(g_dat + (size_t)S3O_EDGE_FLOATS * kmax);   // the keypoint of correspondence c

  // ---- the served correspondences, ascending k1
  float Tc1[16], Tc2[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) { Tc1[k] = a.Tcw1[k]; Tc2[k] = Tcw2p[k]; }
  int n = 0;   // the correspondences of the chunks below this one (the same in every thread)
  for (int c0 = 0; c0 < kmax; c0 += S3O_THREADS) {
    const int k1 = c0 + tid;
    int k2 = -1, p1 = -1, p2 = -1;
    bool served = false;
    if (k1 < kmax) {
      k2 = k1 < K1 ? m12in[k1] : -1;
      unsigned char v = SPFE_SIM3OPT_NONE;
      if (k2 >= 0) {
        if (k2 < K2) {
          p1 = mp1[k1];
          p2 = mp2[k2];
          served = p1 >= 0 && p1 < a.n && p2 >= 0 && p2 < a.n && (a.flags[p1] & SPFE_PROJ_SEARCHABLE) &&
                   (a.flags[p2] & SPFE_PROJ_SEARCHABLE);
        }
        v = SPFE_SIM3OPT_SKIPPED;   // the served ones are rewritten by the classification
      }
      verdict[k1] = v;
      m12o[k1] = k2;
    }
    int total;
    const int rank = wg_ordered_rank<S3O_THREADS>(served, lane, wave, s_int, &total);
    if (served) {
      const int c = n + rank;
      g_k1[c] = k1;
      const float X1[3] = {a.xyz[3 * p1], a.xyz[3 * p1 + 1], a.xyz[3 * p1 + 2]};
      const float X2[3] = {a.xyz[3 * p2], a.xyz[3 * p2 + 1], a.xyz[3 * p2 + 2]};
      float P1[3], P2[3];
      spfe_sim3_to_cam(Tc1, X1, P1);
      spfe_sim3_to_cam(Tc2, X2, P2);
      const float d[S3O_EDGE_FLOATS] = {P1[0], P1[1], P1[2], P2[0], P2[1], P2[2], xy1[2 * k1], xy1[2 * k1 + 1],
                                        xy2[2 * k2], xy2[2 * k2 + 1]};
#pragma unroll
      for (int k = 0; k < S3O_EDGE_FLOATS; ++k) g_dat[(size_t)k * kmax + c] = d[k];
    }
    n += total;
    __syncthreads();   // s_int is rewritten by the next chunk
  }
  const bool in_lds = n <= cap;
  __threadfence_block();
  for (int c = tid; c < n; c += S3O_THREADS) {
    s_alive[c] = 1;
    s_bad[2 * c] = 0;
    s_bad[2 * c + 1] = 0;
    if (in_lds) {
#pragma unroll
      for (int k = 0; k < S3O_EDGE_FLOATS; ++k) s_dat[k * cap + c] = g_dat[(size_t)k * kmax + c];
    }
  }
  __syncthreads();

  // term i = 2 c + kind: the point that is mapped, the observation
  const int kind = tid & 1;
  const double fx = kind ? a.fx2 : a.fx1, fy = kind ? a.fy2 : a.fy1, cx = kind ? a.cx2 : a.cx1, cy = kind ? a.cy2 : a.cy1;
  auto load = [&](int c, double (&P)[3], double &ox, double &oy) {
    const int pk = kind ? 0 : 3, ok = kind ? 8 : 6;
    if (in_lds) {
      P[0] = s_dat[pk * cap + c]; P[1] = s_dat[(pk + 1) * cap + c]; P[2] = s_dat[(pk + 2) * cap + c];
      ox = s_dat[ok * cap + c]; oy = s_dat[(ok + 1) * cap + c];
    } else {
      P[0] = g_dat[(size_t)pk * kmax + c]; P[1] = g_dat[(size_t)(pk + 1) * kmax + c]; P[2] = g_dat[(size_t)(pk + 2) * kmax + c];
      ox = g_dat[(size_t)ok * kmax + c]; oy = g_dat[(size_t)(ok + 1) * kmax + c];
    }
  };

  int set = 0;
  // computeActiveErrors at the estimate whose forward / inverse forms are at `sim` (LDS) + activeRobustChi2
  auto errors_and_chi = [&](const double *sim) -> double {
    spfe_s3o_sim M;
    get_sim(sim + 8 * kind, M);
    double v = 0.0;
    for (int i = tid; i < 2 * n; i += S3O_THREADS) {
      const int c = i >> 1;
      if (!s_alive[c]) continue;
      double P[3], ox, oy, e[2];
      load(c, P, ox, oy);
      spfe_s3o_error(&M, P, fx, fy, cx, cy, ox, oy, e);
      const double chi = spfe_s3o_chi2(e);
      s_bad[i] = chi > a.th2;   // a double against the float th2
      v += spfe_s3o_rho0(chi);
    }
    v = wave_tree(v);
    double *part = s_part + set * (4 * NSUM);
    if (lane == 0) part[wave * NSUM] = v;
    __syncthreads();
    const double chi = sum4_ordered(part, NSUM);
    set ^= 1;
    return chi;
  };
  // linearizeOplus' estimates: s_sims[1 + p], p = 2 d + (minus); s_sims[0] is the estimate itself
  auto perturb = [&](const spfe_s3o_sim &S) {
    if (tid < 15) {
      spfe_s3o_sim F = S, I;
      if (tid == 0) spfe_s3o_inv(&S, &I);
      else spfe_s3o_perturb(&S, tid - 1, a.fix_scale, &F, &I);
      put_sim(s_sims + tid * SIM_D, F);
      put_sim(s_sims + tid * SIM_D + 8, I);
    }
    __syncthreads();
  };
  // buildSystem at s_sims
  auto build = [&](double (&H)[49], double (&b)[7]) {
    double v[32], w[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 32; ++j) v[j] = 0.0;
    for (int i = tid; i < 2 * n; i += S3O_THREADS) {
      const int c = i >> 1;
      if (!s_alive[c]) continue;
      double P[3], ox, oy, e[2], J0[7], J1[7], t[NSUM];
      load(c, P, ox, oy);
      spfe_s3o_sim M;
      get_sim(s_sims + 8 * kind, M);
      spfe_s3o_error(&M, P, fx, fy, cx, cy, ox, oy, e);
#pragma unroll
      for (int d = 0; d < 7; ++d) {
        double ep[2], em[2];
        get_sim(s_sims + (1 + 2 * d) * SIM_D + 8 * kind, M);
        spfe_s3o_error(&M, P, fx, fy, cx, cy, ox, oy, ep);
        get_sim(s_sims + (2 + 2 * d) * SIM_D + 8 * kind, M);
        spfe_s3o_error(&M, P, fx, fy, cx, cy, ox, oy, em);
        spfe_s3o_jcol(ep, em, &J0[d], &J1[d]);
      }
      spfe_s3o_terms(e, J0, J1, t);
#pragma unroll
      for (int k = 0; k < 32; ++k) v[k] += t[1 + k];
#pragma unroll
      for (int k = 0; k < 3; ++k) w[k] += t[33 + k];
    }
    wave_tree_scatter32(v, lane);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
      for (int k = 0; k < 3; ++k) w[k] = w[k] + xchg(w[k], m);
    }
    double *part = s_part + set * (4 * NSUM);
    if (!(lane & 1)) part[wave * NSUM + 1 + (lane >> 1)] = v[0];
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) part[wave * NSUM + 33 + k] = w[k];
    }
    __syncthreads();
    const int k_mine = lane < NSUM ? lane : 0;
    const double mine = sum4_ordered(part + k_mine, NSUM);
    double tot[NSUM];
    tot[0] = 0.0;
#pragma unroll
    for (int k = 1; k < NSUM; ++k) tot[k] = bcast(mine, k);
    spfe_s3o_unpack(tot, H, b);
    set ^= 1;
  };
  // initializeOptimization(); optimize(iterations) from S: the iterations run (0 when no edge is active), the trials into *trials
  auto optimize = [&](spfe_s3o_sim &S, int n_active, int iterations, int *trials) -> int {
    *trials = 0;
    if (n_active == 0) return 0;
    spfe_lm lm;
    lm.lambda = 0.0; lm.ni = 2.0;
    int it_done = 0, n_trials = 0;
    bool fresh = false, go = iterations > 0;
    double currentChi = 0.0;
    for (int it = 0; it < iterations && go; ++it) {
      perturb(S);
      if (!fresh) currentChi = errors_and_chi(s_sims);
      double H[49], b[7];
      build(H, b);
      if (it == 0) {
        double maxDiagonal = 0;
        for (int j = 0; j < 7; ++j) maxDiagonal = fabs(H[j * 7 + j]) > maxDiagonal ? fabs(H[j * 7 + j]) : maxDiagonal;
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
          double xc[7];
          spfe_s3o_sim Sc = S, Ic;
          const int okc = spfe_solve7(H, lam, b, xc);
          if (okc) spfe_s3o_oplus(&Sc, xc, a.fix_scale);
          spfe_s3o_inv(&Sc, &Ic);
          if (lane == 0) {
            double *c = s_cand + wave * CAND_D;
#pragma unroll
            for (int j = 0; j < 7; ++j) c[j] = xc[j];
            put_sim(c + 7, Sc);
            put_sim(c + 15, Ic);
            c[23] = okc ? 1.0 : 0.0;
          }
          __syncthreads();
        }
        double x[7];
        spfe_s3o_sim St;
        const double *c = s_cand + (qmax & 3) * CAND_D;
#pragma unroll
        for (int j = 0; j < 7; ++j) x[j] = c[j];
        get_sim(c + 7, St);
        const bool ok2 = c[23] != 0.0;
        const double chiT = errors_and_chi(c + 7);
        const double tempChi = ok2 ? chiT : 1.7976931348623157e308;
        fresh = spfe_s3o_lm_judge(&lm, currentChi, tempChi, x, b, &rho) != 0;
        if (fresh) { currentChi = tempChi; S = St; }
        qmax++;
        n_trials++;
        // the candidates of the next group are written after this barrier-separated read (errors_and_chi's barrier follows
        // every thread's read of s_cand)
      } while (rho < 0 && qmax < SPFE_LM_MAX_TRIALS);
      it_done++;
      if (qmax == SPFE_LM_MAX_TRIALS || rho == 0) go = false;
    }
    __syncthreads();   // the next phase may rewrite s_cand / s_sims / s_alive
    *trials = n_trials;
    return it_done;
  };
  // the test on the errors the edges hold; bad ones leave (matches12 = -1) with `code`, the others get `keep`; returns nBad
  auto classify = [&](unsigned char code, unsigned char keep) -> int {
    int bad = 0;
    for (int c = tid; c < n; c += S3O_THREADS) {
      if (!s_alive[c]) continue;
      const int k1 = g_k1[c];
      const int o = s_bad[2 * c] || s_bad[2 * c + 1];
      if (o) {
        s_alive[c] = 0;
        m12o[k1] = -1;
      }
      verdict[k1] = o ? code : keep;
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

  float Tin[13];
#pragma unroll
  for (int k = 0; k < 13; ++k) Tin[k] = T12p[k];
  spfe_s3o_sim S;
  spfe_s3o_from_f32(Tin, &S);
  int iters[2] = {0, 0}, trials[2] = {0, 0};
  iters[0] = optimize(S, n, a.iterations, &trials[0]);
  const int nBad = classify(SPFE_SIM3OPT_REMOVED, SPFE_SIM3OPT_KEPT);
  const bool stop = n - nBad < a.min_kept;
  int nIn = 0;
  if (!stop) {
    iters[1] = optimize(S, n - nBad, nBad > 0 ? 2 * a.iterations : a.iterations, &trials[1]);
    nIn = (n - nBad) - classify(SPFE_SIM3OPT_OUTLIER, SPFE_SIM3OPT_INLIER);
  }
  // matched: this thread's own entries of matches12_out (the strided ownership of the prologue and of nothing else: the
  // classification wrote through g_k1, so the block's writes are ordered first)
  __threadfence_block();
  __syncthreads();
  for (int k1 = tid; k1 < kmax; k1 += S3O_THREADS) {
    const int k2 = m12o[k1];
    matched[k1] = (k2 >= 0 && k2 < K2) ? mp2[k2] : -1;
  }
  if (tid == 0) {
    double S12[13];
    float T12f[13], Scw[16];
    if (stop) spfe_s3o_store_echo(Tin, S12, T12f);
    else spfe_s3o_store(&S, S12, T12f);
    spfe_s3o_scw(S12, Tc2, Scw);
    for (int k = 0; k < 13; ++k) { S12o[k] = S12[k]; T12o[k] = T12f[k]; }
    for (int k = 0; k < 16; ++k) Scwo[k] = Scw[k];
    cnt[0] = n; cnt[1] = nBad; cnt[2] = nIn; cnt[3] = (!stop && nIn >= a.min_inliers) ? 1 : 0;
    cnt[4] = iters[0]; cnt[5] = iters[1]; cnt[6] = trials[0]; cnt[7] = trials[1];
    cnt[8] = status;
  }
}

size_t sim3opt_lds_bytes(int kmax) {
  const size_t want = s3o_data_off(kmax) + (size_t)kmax * S3O_EDGE_FLOATS * 4;
  return want < S3O_LDS_MAX ? want : S3O_LDS_MAX;
}

size_t sim3opt_scratch_bytes(int kmax) { return (size_t)kmax * (S3O_EDGE_FLOATS + 1) * 4; }   // edge data | k1

int sim3opt_lds_edge_capacity(int kmax) {
  if (kmax < 1 || kmax > S3O_MAX_KEYPOINTS) return -1;
  return s3o_edge_cap(sim3opt_lds_bytes(kmax), kmax);
}

hipError_t launch_sim3opt(const Sim3OptArgs &a0, hipStream_t s) {
  Sim3OptArgs a = a0;
  if (a.kmax < 1 || a.kmax > S3O_MAX_KEYPOINTS || a.n_jobs < 1 || a.n_jobs > GUIDED_MAX_JOBS) return hipErrorInvalidValue;
  a.lds_bytes = sim3opt_lds_bytes(a.kmax);
  static LdsLimitOnce lds_once;   // (spfe_kernels.h)
  if (hipError_t e = raise_lds_limit(lds_once, reinterpret_cast<const void *>(sim3opt_kernel), (int)S3O_LDS_MAX); e != hipSuccess) return e;
  hipLaunchKernelGGL(sim3opt_kernel, dim3(a.n_jobs), dim3(S3O_THREADS), a.lds_bytes, s, a);
  return hipGetLastError();
}

}  // namespace spfe
