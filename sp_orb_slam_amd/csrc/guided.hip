// guided.hip — the guided match of SPMatcher::SearchBySim3Override (sp_matcher_loop.cpp:7-220, with
// KeyFrame::GetFeaturesInArea / IsInImage, keyframe.cpp:1018-1060) as LoopClosingVLAD::ComputeSim3 calls it for a returning
// hypothesis (loop_closer_vlad.cpp:418-432), between the current keyframe's record and the candidates' records resident in
// HBM.  The arithmetic is include/spfe_guided_math.h (on spfe_proj_math.h and spfe_sim3_math.h); the host statement the tests
// hold these kernels to is tests/guided_ref/guided_ref.c: every output is equal bit for bit.
//
//   guided_prepare_kernel  one workgroup per job: the seed, the transform and keyframe 2's already-mask into the job's
//                          scratch.  Single form: both are arrays.  Batched form: T12 of hypothesis h and the seed
//                          seed12[k1[i]] = match12[k1[i]] for the set inlier bits of h are read from the candidate's verify
//                          block (sim3.hip) on the device.
//   guided_search_kernel   grid (ceil(kmax / 4), 2 directions, n_jobs), one wavefront per keypoint: the gates are
//                          wave-uniform, then wave_search.h's window walk.  Nothing is kept per candidate: no keypoint is
//                          ever blocked, so the running best is the answer.
//   guided_agree_kernel    one workgroup per job walks the keypoints 1024 at a time: matches12 and the three counts — ballot
//                          + popcount inside a wavefront, the 16 wavefront totals through LDS, carried from chunk to chunk.
// Nothing here writes an input array, and nothing synchronises with the host.
//
// The loop-point projection of SPMatcher::SearchByProjectionLoop (sp_matcher_loop.cpp:222-332), spfe_guided_math.h (b):
//   loopproj_candidates_kernel  one wavefront per map point: SKIP_BAD, ALREADY_FOUND (wave_holds_id on `matched` on entry),
//                          spfe_fuse_project on the camera of Scw, then wave_search.h's window walk: ALL keypoints of the
//                          window in window order with their distances into scratch (taken or not: whether one is taken is
//                          the claim stage's business)
//   loopproj_claim_kernel  the ordered claim as a fixed point, a sibling of proj_resolve_kernel with its own rule: EVERY
//                          holder blocks, an accepted point always blocks, a refused point takes nothing.  One workgroup;
//                          claim[kmax] and blocked[kmax] in LDS; at most n rounds.  A matched point writes its id into
//                          `matched` (a keypoint is taken once at the most: it is blocked from then on).  Then the ordered
//                          compaction of the matched points (wg_ordered_rank).
#include "../../include/spfe.h"
#include "../../include/spfe_guided_math.h"
#include "spfe_kernels.h"
#include "wave_search.h"

static_assert(SPFE_PROJ_POINT_SEARCHABLE == SPFE_PROJ_SEARCHABLE, "flags");
static_assert(SPFE_GUIDED_R_NO_POINT == SPFE_GUIDED_NO_POINT && SPFE_GUIDED_R_ALREADY == SPFE_GUIDED_ALREADY &&
              SPFE_GUIDED_R_SKIP_BAD == SPFE_GUIDED_SKIP_BAD && SPFE_GUIDED_R_BEHIND == SPFE_GUIDED_BEHIND &&
              SPFE_GUIDED_R_OUTSIDE == SPFE_GUIDED_OUTSIDE && SPFE_GUIDED_R_RANGE == SPFE_GUIDED_RANGE &&
              SPFE_GUIDED_R_NO_CANDIDATE == SPFE_GUIDED_NO_CANDIDATE && SPFE_GUIDED_R_TOO_FAR == SPFE_GUIDED_TOO_FAR &&
              SPFE_GUIDED_R_MATCHED == SPFE_GUIDED_MATCHED, "reason codes");

namespace spfe {

static_assert(SPFE_LOOPPROJ_R_SKIP_BAD == SPFE_LOOPPROJ_SKIP_BAD && SPFE_LOOPPROJ_R_ALREADY_FOUND == SPFE_LOOPPROJ_ALREADY_FOUND &&
              SPFE_LOOPPROJ_R_BEHIND == SPFE_LOOPPROJ_BEHIND && SPFE_LOOPPROJ_R_OUTSIDE == SPFE_LOOPPROJ_OUTSIDE &&
              SPFE_LOOPPROJ_R_RANGE == SPFE_LOOPPROJ_RANGE && SPFE_LOOPPROJ_R_ANGLE == SPFE_LOOPPROJ_ANGLE &&
              SPFE_LOOPPROJ_R_NO_CANDIDATE == SPFE_LOOPPROJ_NO_CANDIDATE && SPFE_LOOPPROJ_R_TOO_FAR == SPFE_LOOPPROJ_TOO_FAR &&
              SPFE_LOOPPROJ_R_MATCHED == SPFE_LOOPPROJ_MATCHED, "reason codes");
static_assert(SPFE_LOOPPROJ_R_BEHIND == SPFE_FUSE_R_BEHIND && SPFE_LOOPPROJ_R_OUTSIDE == SPFE_FUSE_R_OUTSIDE &&
              SPFE_LOOPPROJ_R_RANGE == SPFE_FUSE_R_RANGE && SPFE_LOOPPROJ_R_ANGLE == SPFE_FUSE_R_ANGLE, "spfe_fuse_project's codes");
static_assert(GUIDED_MAX_JOBS == SPFE_GUIDED_MAX_JOBS, "jobs");

// one job's scratch: seed [kmax] int32 | T12 and the skip flag, 64 bytes | already2 [kmax] uint8
__host__ __device__ size_t guided_scratch_bytes(int kmax) { return ((size_t)kmax * 5 + 64 + 15) / 16 * 16; }

namespace {
constexpr int GD_WG = 1024;

// job q's view of the arguments
struct GuidedJob {
  const uint8_t *rec1, *rec2;
  const int *mp2;
  const float *Tcw2;
  int *seed;        // [kmax] scratch: seed12 of the job
  float *T;         // [16] scratch: T12 (13 floats), then the skip flag as an int
  uint8_t *al2;     // [kmax] scratch: already2
  uint8_t *out;
  int K1, K2, status;
};
__device__ __forceinline__ int guided_K(const GuidedArgs &a, const uint8_t *rec, int k_imm, int *status) {
  if (a.off_hdr < 0) return min(max(k_imm, 0), a.kmax);
  const int *hdr = reinterpret_cast<const int *>(rec + a.off_hdr);
  *status |= hdr[2];
  return min(max(hdr[0], 0), a.kmax);
}
__device__ __forceinline__ GuidedJob guided_job(const GuidedArgs &a, int q) {
  GuidedJob j;
  j.rec1 = a.base1;
  j.rec2 = a.base2[q];
  j.mp2 = a.mp2 + (size_t)a.cand[q] * a.kmax;
  j.Tcw2 = a.Tcw2 + 16 * (size_t)a.cand[q];
  uint8_t *scr = a.scratch + (size_t)q * guided_scratch_bytes(a.kmax);
  j.seed = reinterpret_cast<int *>(scr);
  j.T = reinterpret_cast<float *>(scr + (size_t)a.kmax * 4);
  j.al2 = scr + (size_t)a.kmax * 4 + 64;
  j.out = a.out + (size_t)q * SPFE_GUIDED_OUT_BYTES(a.kmax);
  j.status = 0;
  j.K1 = guided_K(a, j.rec1, a.k_imm1, &j.status);
  j.K2 = guided_K(a, j.rec2, a.k_imm2, &j.status);
  return j;
}
__device__ __forceinline__ int guided_skip(const GuidedJob &j) { return reinterpret_cast<const int *>(j.T)[13]; }
}  // namespace

__global__ __launch_bounds__(256) void guided_prepare_kernel(GuidedArgs a) {
  const int q = blockIdx.x, tid = threadIdx.x;
  const GuidedJob j = guided_job(a, q);
  for (int k = tid; k < a.kmax; k += 256) {
    j.seed[k] = -1;
    j.al2[k] = 0;
  }
  __syncthreads();
  int skip = 0;
  if (a.verify) {   // vpMapPointMatches[k1] of the solver's inliers   loop_closer_vlad.cpp:418-423
    const uint8_t *blk = a.verify + (size_t)a.cand[q] * SPFE_SIM3_OUT_BYTES(a.kmax, a.n_hyp);
    const int *fld = reinterpret_cast<const int *>(blk);
    skip = fld[SPFE_SIM3_OFF_BEST_H / 4] < 0;   // not evaluated: T12 and the inlier words were never written
    if (!skip) {
      const int N = min(max(fld[SPFE_SIM3_OFF_N / 4], 0), a.kmax);
      const int *k1_list = reinterpret_cast<const int *>(blk + SPFE_SIM3_OFF_K1);
      const unsigned long long *bits = reinterpret_cast<const unsigned long long *>(blk + SPFE_SIM3_OFF_INLIERS(a.kmax, a.n_hyp)) +
                                       (size_t)a.hyp[q] * SPFE_SIM3_WORDS(a.kmax);
      const int *match12 = a.match12 + (size_t)a.cand[q] * a.kmax;
      for (int i = tid; i < N; i += 256) {
        const int k1 = k1_list[i];
        if (k1 >= 0 && k1 < j.K1 && ((bits[i >> 6] >> (i & 63)) & 1ull)) j.seed[k1] = match12[k1];   // the k1 of a list are distinct
      }
      if (tid < 13) j.T[tid] = reinterpret_cast<const float *>(blk + SPFE_SIM3_OFF_T12(a.kmax, a.n_hyp))[(size_t)a.hyp[q] * 13 + tid];
    }
  } else {
    for (int k = tid; k < j.K1; k += 256) j.seed[k] = a.seed12[k];
    if (tid < 13) j.T[tid] = a.T12[tid];
  }
  if (tid == 13) reinterpret_cast<int *>(j.T)[13] = skip;
  __syncthreads();
  for (int k = tid; k < j.K1; k += 256) {   // GetIndexInKeyFrame(pKF2) of the seeded point is its keypoint of keyframe 2
    const int s = j.seed[k];
    if (s >= 0 && s < j.K2) j.al2[s] = 1;
  }
}

__global__ __launch_bounds__(256) void guided_search_kernel(GuidedArgs a) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int dir = blockIdx.y;   // 0: keyframe 1's points into keyframe 2; 1: the mirror image
  const GuidedJob j = guided_job(a, blockIdx.z);
  if (guided_skip(j)) return;
  const int Ks = dir ? j.K2 : j.K1, Kt = dir ? j.K1 : j.K2;
  if (i >= Ks) return;   // wave-uniform
  const uint8_t *tgt = dir ? j.rec1 : j.rec2;
  const float *kp_xy = reinterpret_cast<const float *>(tgt + a.off_xy);
  const int16_t *occ = reinterpret_cast<const int16_t *>(tgt + a.off_occ);
  const float *kp_desc = reinterpret_cast<const float *>(tgt + a.off_desc);

  int reason = 0, best_k = -1;
  float best = spfe_guided_best_init();
  const int id = (dir ? j.mp2 : a.mp1)[i];
  if (id < 0 || id >= a.n) reason = SPFE_GUIDED_NO_POINT;
  else if (dir ? j.al2[i] != 0 : j.seed[i] >= 0) reason = SPFE_GUIDED_ALREADY;
  else if (!(a.flags[id] & SPFE_PROJ_SEARCHABLE)) reason = SPFE_GUIDED_SKIP_BAD;
  float u = 0.0f, v = 0.0f;
  if (!reason) {
    float Tcw[16], T13[13], T12[12], T21[12];
    const float *src = dir ? j.Tcw2 : a.Tcw1;
#pragma unroll
    for (int k = 0; k < 16; ++k) Tcw[k] = src[k];
#pragma unroll
    for (int k = 0; k < 13; ++k) T13[k] = j.T[k];
    spfe_sim3_T T;
    spfe_guided_T_from_f32(T13, &T);
    spfe_sim3_forms(&T, T12, T21);
    spfe_guided_view vw;
    vw.fx = dir ? a.fx1 : a.fx2; vw.fy = dir ? a.fy1 : a.fy2; vw.cx = dir ? a.cx1 : a.cx2; vw.cy = dir ? a.cy1 : a.cy2;
    vw.W = a.W; vw.H = a.H; vw.min_factor = a.min_factor; vw.max_factor = a.max_factor;
    const float P[3] = {a.xyz[3 * id], a.xyz[3 * id + 1], a.xyz[3 * id + 2]};
    reason = spfe_guided_project(Tcw, dir ? T12 : T21, &vw, P, a.dist_range[2 * id], a.dist_range[2 * id + 1], &u, &v);
  }
  if (!reason) {   // wave-uniform: the window
    const float4 m4 = *reinterpret_cast<const float4 *>(a.desc + (size_t)id * 256 + lane * 4);
    const float mf[4] = {m4.x, m4.y, m4.z, m4.w};
    wave_window_search(occ, a.wc, a.hc, kp_xy, Kt, u, v, a.th, lane, no_gate(), [&](int kk, float, float) {
      const float d = wave_desc_dist(mf, kp_desc, kk, lane, a.kp_desc_bf16);
      if (d < best) { best = d; best_k = kk; }
    });
    reason = best_k < 0 ? SPFE_GUIDED_NO_CANDIDATE : (best > a.th_dist ? SPFE_GUIDED_TOO_FAR : SPFE_GUIDED_MATCHED);
  }
  if (lane == 0) {
    const bool hit = reason == SPFE_GUIDED_MATCHED;
    const size_t om = dir ? SPFE_GUIDED_OFF_MATCH2(a.kmax) : SPFE_GUIDED_OFF_MATCH1;
    const size_t od = dir ? SPFE_GUIDED_OFF_DIST2(a.kmax) : SPFE_GUIDED_OFF_DIST1(a.kmax);
    const size_t orr = dir ? SPFE_GUIDED_OFF_REASON2(a.kmax) : SPFE_GUIDED_OFF_REASON1(a.kmax);
    reinterpret_cast<int *>(j.out + om)[i] = hit ? best_k : -1;
    reinterpret_cast<float *>(j.out + od)[i] = hit ? best : 0.0f;
    (j.out + orr)[i] = (uint8_t)reason;
  }
}

__global__ __launch_bounds__(GD_WG) void guided_agree_kernel(GuidedArgs a) {
  __shared__ int wave_total[3][GD_WG / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const GuidedJob j = guided_job(a, blockIdx.x);
  const bool skip = guided_skip(j) != 0;
  const int *match1 = reinterpret_cast<const int *>(j.out + SPFE_GUIDED_OFF_MATCH1);
  const int *match2 = reinterpret_cast<const int *>(j.out + SPFE_GUIDED_OFF_MATCH2(a.kmax));
  int *matches12 = reinterpret_cast<int *>(j.out + SPFE_GUIDED_OFF_MATCHES12(a.kmax));
  int n_found = 0, n_total = 0, n_seed = 0;   // of the chunks below this one (the same in every lane)
  for (int base = 0; base < a.kmax; base += GD_WG) {
    const int i1 = base + tid;
    int m = -1, found = 0, seeded = 0;
    if (i1 < j.K1 && !skip) {
      const int seed = j.seed[i1], k2 = match1[i1];
      const int back = (k2 >= 0 && k2 < j.K2) ? match2[k2] : -1;
      m = spfe_guided_agree(i1, (k2 >= 0 && k2 < j.K2) ? k2 : -1, back, seed, &found);
      seeded = seed >= 0;
    }
    if (i1 < a.kmax) matches12[i1] = m;
    const unsigned long long vf = __ballot(found != 0), vt = __ballot(m >= 0), vs = __ballot(seeded != 0);
    if (lane == 0) {
      wave_total[0][wave] = __popcll(vf);
      wave_total[1][wave] = __popcll(vt);
      wave_total[2][wave] = __popcll(vs);
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < GD_WG / 64; ++w) {
      n_found += wave_total[0][w];
      n_total += wave_total[1][w];
      n_seed += wave_total[2][w];
    }
    __syncthreads();   // wave_total is rewritten by the next chunk
  }
  if (tid == 0) {
    int *hdr = reinterpret_cast<int *>(j.out);
    hdr[SPFE_GUIDED_OFF_N_FOUND / 4] = n_found;
    hdr[SPFE_GUIDED_OFF_N_TOTAL / 4] = n_total;
    hdr[SPFE_GUIDED_OFF_N_SEED / 4] = n_seed;
    hdr[SPFE_GUIDED_OFF_STATUS / 4] = j.status | (skip ? SPFE_GUIDED_STATUS_NOT_EVALUATED : 0);
  }
}

hipError_t launch_guided_match(const GuidedArgs &a, hipStream_t s) {
  if (a.n_jobs < 1 || a.n_jobs > GUIDED_MAX_JOBS || a.kmax < 1 || a.n < 0 || a.n > SPFE_PROJ_MAX_POINTS || !a.scratch)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(guided_prepare_kernel, dim3(a.n_jobs), dim3(256), 0, s, a);
  hipLaunchKernelGGL(guided_search_kernel, dim3((a.kmax + 3) / 4, 2, a.n_jobs), dim3(256), 0, s, a);
  hipLaunchKernelGGL(guided_agree_kernel, dim3(a.n_jobs), dim3(GD_WG), 0, s, a);
  return hipGetLastError();
}

// ---- the loop-point projection -------------------------------------------------------------------------------------------
namespace {
constexpr int LP_CAND = SPFE_PROJ_MAX_CAND;
constexpr int LP_PER = SPFE_PROJ_MAX_POINTS / GD_WG;   // map points per thread of the claim workgroup
static_assert(LP_PER * GD_WG == SPFE_PROJ_MAX_POINTS, "points per thread");
__device__ __forceinline__ int loopproj_K(const LoopProjArgs &a) { return a.hdr ? min(max(a.hdr[0], 0), a.kmax) : min(max(a.k_imm, 0), a.kmax); }
}  // namespace

__global__ __launch_bounds__(256) void loopproj_candidates_kernel(LoopProjArgs a) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.n) return;   // wave-uniform
  const int K = loopproj_K(a);
  int reason = 0, cnt = 0;
  if (!(a.flags[i] & SPFE_PROJ_SEARCHABLE)) reason = SPFE_LOOPPROJ_SKIP_BAD;
  // spAlreadyFound, built from the entry state: this launch ends before the claim writes
  if (!reason && wave_holds_id(a.matched, K, a.point_id[i], lane)) reason = SPFE_LOOPPROJ_ALREADY_FOUND;
  float u = 0.0f, v = 0.0f;
  if (!reason) {
    float S[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) S[k] = a.Scw[k];
    spfe_proj_cam cam;
    spfe_loop_cam_from_scw(S, &cam);
    const spfe_fuse_view vw = fuse_view_of(a);
    const float P[3] = {a.xyz[3 * i], a.xyz[3 * i + 1], a.xyz[3 * i + 2]};
    const float N[3] = {a.normal[3 * i], a.normal[3 * i + 1], a.normal[3 * i + 2]};
    reason = spfe_fuse_project(&cam, &vw, P, N, a.dist_range[2 * i], a.dist_range[2 * i + 1], &u, &v);
  }
  if (!reason) {   // wave-uniform: the window
    const float4 m4 = *reinterpret_cast<const float4 *>(a.desc + (size_t)i * 256 + lane * 4);
    const float mf[4] = {m4.x, m4.y, m4.z, m4.w};
    int *ck = a.cand_k + (size_t)i * LP_CAND;
    float *cd = a.cand_d + (size_t)i * LP_CAND;
    wave_window_search(a.occ, a.wc, a.hc, a.kp_xy, K, u, v, a.th, lane, no_gate(), [&](int kk, float, float) {
      const float d = wave_desc_dist(mf, a.kp_desc, kk, lane, a.kp_desc_bf16);
      if (lane == 0 && cnt < LP_CAND) {   // one keypoint per cell: at most LP_CAND
        ck[cnt] = kk;
        cd[cnt] = d;
      }
      cnt++;
    });
    if (cnt == 0) reason = SPFE_LOOPPROJ_NO_CANDIDATE;
  }
  if (lane == 0) {
    a.cand_n[i] = reason ? 0 : min(cnt, LP_CAND);
    (a.out + SPFE_LOOPPROJ_OFF_REASON(a.cap))[i] = (uint8_t)reason;   // 0: the claim stage decides
  }
}

__global__ __launch_bounds__(GD_WG) void loopproj_claim_kernel(LoopProjArgs a) {
  extern __shared__ __attribute__((aligned(16))) int sm_lp[];
  __shared__ int pending, wave_total[GD_WG / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = a.n;
  const int K = loopproj_K(a);
  int *claim = sm_lp;                                              // [kmax] the earliest unfinished point that could take it
  uint8_t *blocked = reinterpret_cast<uint8_t *>(claim + a.kmax);   // [kmax] the keypoint holds a point, whichever
  int *kp_of_mp = reinterpret_cast<int *>(a.out + SPFE_LOOPPROJ_OFF_KP_OF_MP);
  float *best_dist = reinterpret_cast<float *>(a.out + SPFE_LOOPPROJ_OFF_BEST_DIST(a.cap));
  int *matched_idx = reinterpret_cast<int *>(a.out + SPFE_LOOPPROJ_OFF_MATCHED_IDX(a.cap));
  uint8_t *reason = a.out + SPFE_LOOPPROJ_OFF_REASON(a.cap);
  for (int k = tid; k < K; k += GD_WG) blocked[k] = a.matched[k] != -1;
  int cn[LP_PER];
  bool done[LP_PER];
#pragma unroll
  for (int q = 0; q < LP_PER; ++q) {
    const int i = tid + q * GD_WG;
    cn[q] = i < n ? a.cand_n[i] : 0;
    done[q] = cn[q] == 0;
    if (i < n && done[q]) {   // refused before the window, or an empty window
      kp_of_mp[i] = -1;
      best_dist[i] = 0.0f;
    }
  }
  __syncthreads();
  const float best0 = spfe_loopproj_best_init();
  for (int round = 0; round <= n; ++round) {   // at most n rounds are needed: the lowest unfinished point is always final
    for (int k = tid; k < K; k += GD_WG) claim[k] = 0x7fffffff;
    if (tid == 0) pending = 0;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < LP_PER; ++q) {
      if (done[q]) continue;
      const int i = tid + q * GD_WG;
      const int *ck = a.cand_k + (size_t)i * LP_CAND;
      for (int c = 0; c < cn[q]; ++c) {
        const int k = ck[c];
        if (!blocked[k]) atomicMin(&claim[k], i);
      }
    }
    __syncthreads();
    bool fin[LP_PER];
    int pick[LP_PER];
    float bd[LP_PER];
#pragma unroll
    for (int q = 0; q < LP_PER; ++q) {
      fin[q] = false;
      pick[q] = -1;
      bd[q] = best0;
      if (done[q]) continue;
      const int i = tid + q * GD_WG;
      const int *ck = a.cand_k + (size_t)i * LP_CAND;
      const float *cd = a.cand_d + (size_t)i * LP_CAND;
      bool first = true;
      float best = best0;
      int bk = -1;
      for (int c = 0; c < cn[q]; ++c) {
        const int k = ck[c];
        if (blocked[k]) continue;
        if (claim[k] != i) { first = false; break; }
        const float d = cd[c];
        if (d < best) { best = d; bk = k; }
      }
      fin[q] = first;
      if (first && bk >= 0 && !(best > a.th_dist)) { pick[q] = bk; bd[q] = best; }
    }
    __syncthreads();   // every decision read `blocked` before anybody writes it
    bool mine = false;
#pragma unroll
    for (int q = 0; q < LP_PER; ++q) {
      if (done[q]) continue;
      if (fin[q]) {
        const int i = tid + q * GD_WG;
        const bool hit = pick[q] >= 0;
        kp_of_mp[i] = pick[q];
        best_dist[i] = hit ? bd[q] : 0.0f;
        reason[i] = hit ? SPFE_LOOPPROJ_MATCHED : SPFE_LOOPPROJ_TOO_FAR;
        if (hit) {   // two points final in one round share no unblocked candidate: one writer per keypoint
          blocked[pick[q]] = 1;
          a.matched[pick[q]] = a.point_id[i];
        }
        done[q] = true;
      } else {
        mine = true;
      }
    }
    if (mine) pending = 1;
    __syncthreads();
    if (!pending) break;
    __syncthreads();
  }
  __syncthreads();   // this block's own writes of `reason` are read below
  int total_done = 0;
  for (int base = 0; base < n; base += GD_WG) {
    const int i = base + tid;
    const bool hit = i < n && reason[i] == SPFE_LOOPPROJ_MATCHED;
    int total;
    const int rank = wg_ordered_rank<GD_WG>(hit, lane, wave, wave_total, &total);
    if (hit) matched_idx[total_done + rank] = i;
    total_done += total;
    __syncthreads();   // wave_total is rewritten by the next chunk
  }
  if (tid == 0) {
    int *hdr = reinterpret_cast<int *>(a.out);
    hdr[SPFE_LOOPPROJ_OFF_N_MATCHED / 4] = total_done;
    hdr[SPFE_LOOPPROJ_OFF_N / 4] = n;
    hdr[SPFE_LOOPPROJ_OFF_STATUS / 4] = a.hdr ? a.hdr[2] : 0;
  }
}

size_t loop_proj_lds_bytes(int kmax) { return (size_t)kmax * 5 + 16; }   // the dynamic part
// loopproj_claim_kernel's static LDS: pending and wave_total[16] (68 bytes), padded to the 16-byte alignment of the dynamic array
// behind them (the kernel descriptor's group-segment size).  kmax <= 32748 fits the 160 KB a workgroup can have.
constexpr size_t LP_LDS_STATIC = 80;
static_assert(LP_LDS_STATIC + 5 * (size_t)SPFE_LOOPPROJ_MAX_KEYPOINTS + 16 <= 160 * 1024 &&
              LP_LDS_STATIC + 5 * (size_t)(SPFE_LOOPPROJ_MAX_KEYPOINTS + 1) + 16 > 160 * 1024, "SPFE_LOOPPROJ_MAX_KEYPOINTS");
size_t loop_proj_lds_total(int kmax) { return LP_LDS_STATIC + loop_proj_lds_bytes(kmax); }

hipError_t launch_loop_proj(const LoopProjArgs &a, hipStream_t s) {
  if (a.cap < 1 || a.cap > SPFE_PROJ_MAX_POINTS || a.n < 0 || a.n > a.cap || a.kmax < 1) return hipErrorInvalidValue;
  const size_t lds = loop_proj_lds_bytes(a.kmax);
  if (loop_proj_lds_total(a.kmax) > 160 * 1024) return hipErrorInvalidValue;
  if (lds > 48 * 1024) {   // beyond the default dynamic-LDS limit: raise it
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(loopproj_claim_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  if (a.n > 0) hipLaunchKernelGGL(loopproj_candidates_kernel, dim3((a.n + 3) / 4), dim3(256), 0, s, a);
  hipLaunchKernelGGL(loopproj_claim_kernel, dim3(1), dim3(GD_WG), lds, s, a);
  return hipGetLastError();
}

}  // namespace spfe
