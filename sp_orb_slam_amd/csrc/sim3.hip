// sim3.hip — verification of loop candidates against the current keyframe: the pair list and the RANSAC hypotheses of
// Sim3Solver (sim3_solver.cpp) as LoopClosingVLAD::ComputeSim3 drives it (loop_closer_vlad.cpp:345-449), behind the masked
// cross-check match of SPMatcher::SearchByBruteForce (sp_matcher_loop.cpp:334-376; match.hip).  The arithmetic is
// include/spfe_sim3_math.h, shared with the host reference tests/sim3_ref/sim3_ref.c: the outputs are equal bit for bit.
//
//   loop_match_invert_kernel  the match's per-query train index turned into match12[k1] = k2 (the cross-check leaves a train
//                             row to one query at the most) and nmatches
//   sim3_pairs_kernel         ONE workgroup per candidate walks k1 upward 256 at a time: the pair test, then an ordered
//                             compaction (wave_ops.h's wg_ordered_rank) so that pair i is the i-th in ascending k1; X1c,
//                             X2c, P1im1, P2im2 to scratch, k1 and N to the block
//   sim3_hypotheses_kernel    one WAVEFRONT per (hypothesis, candidate): the draws and Horn's closed form are wave-uniform
//                             (every lane evaluates them on the same operands), then the lanes stride over the N pairs; per
//                             64 pairs a ballot is one word of the inlier bit set and its popcount adds to the count
//   sim3_select_kernel        one workgroup per candidate, one lane per hypothesis: inclusive prefix maximum of the counts,
//                             the returns compacted in order, the best
// Nothing here synchronises with the host; a candidate with fewer than max(3, min_inliers) pairs is settled by the pairs
// kernel and the two launches behind it return at once.
#include "../../include/spfe.h"
#include "../../include/spfe_sim3_math.h"
#include "spfe_kernels.h"
#include "wave_ops.h"

namespace spfe {

namespace {
constexpr int S3_WG = 256;                         // pairs kernel
constexpr int S3_HYP_WAVES = 4;                    // hypotheses per workgroup
constexpr int S3_SEL = SPFE_SIM3_MAX_HYPOTHESES;   // select kernel: one lane per hypothesis

__device__ __forceinline__ int *s3_field(uint8_t *out, size_t off) { return reinterpret_cast<int *>(out + off); }
__device__ __forceinline__ uint8_t *s3_block(const Sim3Args &a, int cand) {
  return a.out + (size_t)cand * SPFE_SIM3_OUT_BYTES(a.kcap, a.n_hyp);
}
__device__ __forceinline__ int s3_floor(const Sim3Args &a) { return max(3, a.min_inliers); }
}  // namespace

__global__ __launch_bounds__(256) void loop_match_invert_kernel(const int32_t *__restrict__ train_idx,
                                                                const int *__restrict__ hdr2, int kmax,
                                                                int *__restrict__ match12, int *__restrict__ n_matches) {
  __shared__ int total;
  const int tid = threadIdx.x;
  if (tid == 0) total = 0;
  for (int k = tid; k < kmax; k += 256) match12[k] = -1;
  __syncthreads();
  const int K2 = min(max(hdr2[0], 0), kmax);
  int mine = 0;
  for (int q = tid; q < K2; q += 256) {
    const int t = train_idx[q];
    if (t >= 0 && t < kmax) {
      match12[t] = q;
      ++mine;
    }
  }
  if (mine) atomicAdd(&total, mine);
  __syncthreads();
  if (tid == 0) *n_matches = total;
}

__global__ __launch_bounds__(S3_WG) void sim3_pairs_kernel(Sim3Args a) {
  __shared__ int wave_total[S3_WG / 64];
  const int cand = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint8_t *out = s3_block(a, cand);
  const int K1 = a.hdr1 ? min(max(a.hdr1[0], 0), a.kcap) : min(max(a.k_imm, 0), a.kcap);
  const int *match12 = a.match12 + (size_t)cand * a.kcap, *mp2 = a.mp2 + (size_t)cand * a.kcap;
  float *scr = a.scratch + (size_t)cand * a.kcap * 10;
  int *k1_list = s3_field(out, SPFE_SIM3_OFF_K1);
  float T1[16], T2[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) { T1[i] = a.Tcw1[i]; T2[i] = a.Tcw2[16 * cand + i]; }
  int done = 0;   // pairs of the chunks below this one (the same in every lane)
  for (int base = 0; base < K1; base += S3_WG) {
    const int k1 = base + tid;
    int p1 = -1, p2 = -1;
    bool pair = false;
    if (k1 < K1) {
      const int k2 = match12[k1];
      if (k2 >= 0 && k2 < a.kcap) {
        p1 = a.mp1[k1];
        p2 = mp2[k2];
        pair = p1 >= 0 && p1 < a.n && p2 >= 0 && p2 < a.n;
        if (pair) pair = (a.flags[p1] & SPFE_PROJ_SEARCHABLE) && (a.flags[p2] & SPFE_PROJ_SEARCHABLE);
      }
    }
    int total;
    const int rank = wg_ordered_rank<S3_WG>(pair, lane, wave, wave_total, &total);
    if (pair) {
      const int i = done + rank;   // i < K1 <= kcap: one pair per k1 at the most
      const float X1[3] = {a.xyz[3 * p1], a.xyz[3 * p1 + 1], a.xyz[3 * p1 + 2]};
      const float X2[3] = {a.xyz[3 * p2], a.xyz[3 * p2 + 1], a.xyz[3 * p2 + 2]};
      float c1[3], c2[3], u1[2], u2[2];
      spfe_sim3_to_cam(T1, X1, c1);
      spfe_sim3_to_cam(T2, X2, c2);
      spfe_sim3_image(a.fx1, a.fy1, a.cx1, a.cy1, c1, u1);
      spfe_sim3_image(a.fx2, a.fy2, a.cx2, a.cy2, c2, u2);
      float *p = scr + (size_t)i * 10;
      p[0] = c1[0]; p[1] = c1[1]; p[2] = c1[2];
      p[3] = c2[0]; p[4] = c2[1]; p[5] = c2[2];
      p[6] = u1[0]; p[7] = u1[1];
      p[8] = u2[0]; p[9] = u2[1];
      k1_list[i] = k1;
    }
    done += total;
    __syncthreads();   // wave_total is rewritten by the next chunk
  }
  const bool idle = done < s3_floor(a);
  if (tid == 0) {
    *s3_field(out, SPFE_SIM3_OFF_N) = done;
    *s3_field(out, SPFE_SIM3_OFF_N_HYP) = a.n_hyp;
    if (idle) {
      *s3_field(out, SPFE_SIM3_OFF_N_RETURNS) = 0;
      *s3_field(out, SPFE_SIM3_OFF_BEST_H) = -1;
      *s3_field(out, SPFE_SIM3_OFF_BEST_COUNT) = 0;
    }
  }
  if (idle) {
    int *count = s3_field(out, SPFE_SIM3_OFF_COUNT(a.kcap));
    for (int h = tid; h < a.n_hyp; h += S3_WG) count[h] = 0;
  }
}

__global__ __launch_bounds__(64 * S3_HYP_WAVES) void sim3_hypotheses_kernel(Sim3Args a) {
  const int cand = blockIdx.y, lane = threadIdx.x & 63;
  const int h = blockIdx.x * S3_HYP_WAVES + (threadIdx.x >> 6);
  uint8_t *out = s3_block(a, cand);
  const int N = min(*s3_field(out, SPFE_SIM3_OFF_N), a.kcap);
  if (h >= a.n_hyp || N < s3_floor(a)) return;   // wave-uniform
  const float *scr = a.scratch + (size_t)cand * a.kcap * 10;
  const uint32_t *rw = a.rnd + ((size_t)cand * a.n_hyp + h) * 3;
  const uint32_t w[3] = {rw[0], rw[1], rw[2]};
  int idx[3];
  spfe_sim3_draws(w, N, 1, idx);
  float P1[9], P2[9];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float *p = scr + (size_t)idx[i] * 10;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      P1[3 * r + i] = p[r];
      P2[3 * r + i] = p[3 + r];
    }
  }
  spfe_sim3_T T;
  spfe_sim3_horn(P1, P2, a.fix_scale, SPFE_SIM3_JACOBI_SWEEPS, &T);
  float T12[12], T21[12];
  spfe_sim3_forms(&T, T12, T21);
  const int words = (int)SPFE_SIM3_WORDS(a.kcap);
  unsigned long long *bits =
      reinterpret_cast<unsigned long long *>(out + SPFE_SIM3_OFF_INLIERS(a.kcap, a.n_hyp)) + (size_t)h * words;
  int count = 0;
  for (int b = 0; b < words; ++b) {
    const int i = b * 64 + lane;
    bool in = false;
    if (i < N) {
      const float *p = scr + (size_t)i * 10;
      const float e1 = spfe_sim3_err(T12, p + 3, a.fx1, a.fy1, a.cx1, a.cy1, p + 6);   // X2c through T12 into image 1
      const float e2 = spfe_sim3_err(T21, p, a.fx2, a.fy2, a.cx2, a.cy2, p + 8);       // X1c through T21 into image 2
      in = e1 < a.max_err1 && e2 < a.max_err2;
    }
    const unsigned long long votes = __ballot(in);
    count += __popcll(votes);
    if (lane == 0) bits[b] = votes;
  }
  if (lane == 0) {
    s3_field(out, SPFE_SIM3_OFF_COUNT(a.kcap))[h] = count;
    float *t = reinterpret_cast<float *>(out + SPFE_SIM3_OFF_T12(a.kcap, a.n_hyp)) + (size_t)h * 13;
    t[0] = T.s;
#pragma unroll
    for (int i = 0; i < 9; ++i) t[1 + i] = T.R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[10 + i] = T.t[i];
  }
}

__global__ __launch_bounds__(S3_SEL) void sim3_select_kernel(Sim3Args a) {
  __shared__ int scan[2][S3_SEL];
  __shared__ int wave_total[S3_SEL / 64];
  __shared__ int best;
  const int cand = blockIdx.x, h = threadIdx.x, lane = h & 63, wave = h >> 6;
  uint8_t *out = s3_block(a, cand);
  if (*s3_field(out, SPFE_SIM3_OFF_N) < s3_floor(a)) return;   // settled by the pairs kernel
  const int c = h < a.n_hyp ? s3_field(out, SPFE_SIM3_OFF_COUNT(a.kcap))[h] : 0;
  if (h == 0) best = -1;
  scan[0][h] = c;
  __syncthreads();
  int cur = 0;
  for (int d = 1; d < S3_SEL; d <<= 1) {   // inclusive prefix maximum in hypothesis order
    const int v = scan[cur][h];
    scan[cur ^ 1][h] = h >= d ? max(v, scan[cur][h - d]) : v;
    cur ^= 1;
    __syncthreads();
  }
  const int pmax = scan[cur][h], top = scan[cur][S3_SEL - 1];   // (entries at and beyond n_hyp hold 0: counts are >= 0)
  const bool ret = h < a.n_hyp && spfe_sim3_returns(c, pmax, a.min_inliers);
  if (h < a.n_hyp && c == top) atomicMax(&best, h);
  int total;
  const int rank = wg_ordered_rank<S3_SEL>(ret, lane, wave, wave_total, &total);
  if (ret) s3_field(out, SPFE_SIM3_OFF_RETURN_IDX(a.kcap, a.n_hyp))[rank] = h;   // rank < n_hyp
  if (h == 0) {
    *s3_field(out, SPFE_SIM3_OFF_N_RETURNS) = total;
    *s3_field(out, SPFE_SIM3_OFF_BEST_H) = best;
    *s3_field(out, SPFE_SIM3_OFF_BEST_COUNT) = top;
  }
}

hipError_t launch_loop_match_invert(const int32_t *train_idx, const int *hdr2, int kmax, int *match12, int *n_matches,
                                    hipStream_t s) {
  hipLaunchKernelGGL(loop_match_invert_kernel, dim3(1), dim3(256), 0, s, train_idx, hdr2, kmax, match12, n_matches);
  return hipGetLastError();
}

hipError_t launch_sim3(const Sim3Args &a, hipStream_t s) {
  if (a.n_cand < 1 || a.n_hyp < 1 || a.n_hyp > SPFE_SIM3_MAX_HYPOTHESES || a.kcap < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sim3_pairs_kernel, dim3(a.n_cand), dim3(S3_WG), 0, s, a);
  hipLaunchKernelGGL(sim3_hypotheses_kernel, dim3((a.n_hyp + S3_HYP_WAVES - 1) / S3_HYP_WAVES, a.n_cand),
                     dim3(64 * S3_HYP_WAVES), 0, s, a);
  hipLaunchKernelGGL(sim3_select_kernel, dim3(a.n_cand), dim3(S3_SEL), 0, s, a);
  return hipGetLastError();
}

}  // namespace spfe
