// tri.hip — new map points between the current keyframe (1) and one neighbour (2), on their records resident in HBM:
// LocalMapping::CreateNewMapPointsOverride (local_mapper.cpp:558-814) with SPMatcher::SearchForTriByFlann
// (sp_matcher.cpp:183-262) and CheckDistEpipolarLine (:441-469).  The arithmetic is include/spfe_tri_math.h, shared with the
// host reference tests/tri_ref/tri_ref.c: the outputs are equal bit for bit.
//
//   tri_begin_kernel        in FRONT of the 2-NN search (match.hip, launch_match_knn2_free): the refusal (a record with
//                           SPFE_STATUS_COV_OVERFLOW has no valid cov2_inv), the baseline test (:603-611), the block's int32
//                           fields, match12 = -1, verdict = 0, and the id counter
//   tri_gate_kernel         one lane per query k2: ratio, epipole and epipolar-line gates on its two nearest free train rows,
//                           then atomicMax(match12[k1], k2) — the reference's loop runs k2 upward and the last writer stays —
//                           and the count of every acceptance
//   tri_triangulate_kernel  ONE workgroup walks k1 upward 1024 at a time, one lane per k1 that holds a match: the verdict, then
//                           an ordered compaction (wave_ops.h's wg_ordered_rank) so that new point t is the t-th success
//                           in ascending k1 whatever the scheduling
// Nothing here synchronises with the host; the decisions of one launch are read by the next from the output block.
#include "../../include/spfe.h"
#include "../../include/spfe_tri_math.h"
#include "spfe_kernels.h"
#include "wave_ops.h"

namespace spfe {

namespace {
constexpr unsigned long long T_NONE = ~0ull;
constexpr int T_WG = 1024;

__device__ __forceinline__ int tri_count(const int *hdr, int kmax) { return min(max(hdr[0], 0), kmax); }
__device__ __forceinline__ int *tri_field(uint8_t *out, int off) { return reinterpret_cast<int *>(out + off); }

__device__ __forceinline__ void tri_cams(const TriArgs &a, spfe_tri_cam *c1, spfe_tri_cam *c2) {
  float T1[16], T2[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) { T1[i] = a.Tcw1[i]; T2[i] = a.Tcw2[i]; }
  spfe_tri_cam_from_f32(T1, a.fx1, a.fy1, a.cx1, a.cy1, c1);
  spfe_tri_cam_from_f32(T2, a.fx2, a.fy2, a.cx2, a.cy2, c2);
}
// the launches behind tri_begin_kernel do nothing for a refused or skipped neighbour
__device__ __forceinline__ bool tri_idle(const TriArgs &a) {
  return *tri_field(a.out, SPFE_TRI_OFF_STATUS) != 0 || *tri_field(a.out, SPFE_TRI_OFF_SKIPPED) != 0;
}
}  // namespace

__global__ __launch_bounds__(256) void tri_begin_kernel(TriArgs a) {
  const int tid = threadIdx.x;
  if (tid == 0 && a.set_base) *a.next_id = a.point_base;
  if ((a.hdr1[2] | a.hdr2[2]) & SPFE_STATUS_COV_OVERFLOW) {
    if (tid == 0) *tri_field(a.out, SPFE_TRI_OFF_STATUS) = SPFE_TRI_STATUS_COV_OVERFLOW;
    return;
  }
  int skip = 0;
  if (a.median_depth) {
    spfe_tri_cam c1, c2;
    tri_cams(a, &c1, &c2);
    skip = spfe_tri_baseline_skip(&c1, &c2, *a.median_depth, a.min_baseline_depth_ratio);
  }
  if (tid == 0) {
    for (int off = SPFE_TRI_OFF_N_MATCHES; off <= SPFE_TRI_OFF_N_REJ_DEGENERATE; off += 4) *tri_field(a.out, off) = 0;
    *tri_field(a.out, SPFE_TRI_OFF_SKIPPED) = skip;
    *tri_field(a.out, SPFE_TRI_OFF_STATUS) = 0;
    *tri_field(a.out, SPFE_TRI_OFF_POINT_BASE) = *a.next_id;   // (this thread wrote it above when set_base)
  }
  if (skip) return;
  int *match12 = tri_field(a.out, SPFE_TRI_OFF_MATCH12), *verdict = tri_field(a.out, SPFE_TRI_OFF_VERDICT(a.kmax));
  for (int k = tid; k < a.kmax; k += 256) {
    match12[k] = -1;
    verdict[k] = SPFE_TRI_NONE;
  }
}

__global__ __launch_bounds__(256) void tri_gate_kernel(TriArgs a) {
  if (tri_idle(a)) return;
  const int k2 = blockIdx.x * 256 + threadIdx.x;
  const int K1 = tri_count(a.hdr1, a.kmax), K2 = tri_count(a.hdr2, a.kmax);
  if (k2 >= K2 || a.mp2[k2] >= 0) return;
  const unsigned long long b1 = a.best1[k2], b2 = a.best2[k2];
  if (b1 == T_NONE || b2 == T_NONE) return;   // fewer than two free train rows: no match
  const int k1 = (int)(unsigned)b1;
  if (k1 >= K1) return;
  spfe_tri_cam c1, c2;
  spfe_tri_pair pr;
  tri_cams(a, &c1, &c2);
  spfe_tri_pair_from_cams(&c1, &c2, &pr);
  const float d0 = __uint_as_float((unsigned)(b1 >> 32)), d1 = __uint_as_float((unsigned)(b2 >> 32));
  if (!spfe_tri_gate(&pr, d0, d1, a.xy1[2 * k1], a.xy1[2 * k1 + 1], a.xy2[2 * k2], a.xy2[2 * k2 + 1], a.cinv2[2 * k2],
                     a.cinv2[2 * k2 + 1], a.ratio, a.epipole_r2, a.chi2_line))
    return;
  atomicMax(tri_field(a.out, SPFE_TRI_OFF_MATCH12) + k1, k2);
  atomicAdd(tri_field(a.out, SPFE_TRI_OFF_N_MATCHES), 1);
}

__global__ __launch_bounds__(T_WG) void tri_triangulate_kernel(TriArgs a) {
  if (tri_idle(a)) return;
  __shared__ int wave_total[T_WG / 64];
  __shared__ int rejects[4];   // parallax, depth, reprojection, degenerate
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K1 = tri_count(a.hdr1, a.kmax), K2 = tri_count(a.hdr2, a.kmax);
  const int id0 = *a.next_id;
  if (tid < 4) rejects[tid] = 0;
  spfe_tri_cam c1, c2;
  tri_cams(a, &c1, &c2);
  const int *match12 = tri_field(a.out, SPFE_TRI_OFF_MATCH12);
  int *verdict = tri_field(a.out, SPFE_TRI_OFF_VERDICT(a.kmax));
  float *new_xyz = reinterpret_cast<float *>(a.out + SPFE_TRI_OFF_NEW_XYZ(a.kmax));
  int *new_k1 = tri_field(a.out, 0) + SPFE_TRI_OFF_NEW_K1(a.kmax) / 4, *new_k2 = tri_field(a.out, 0) + SPFE_TRI_OFF_NEW_K2(a.kmax) / 4;
  int done = 0;   // new points of the chunks below this one (the same in every lane)
  __syncthreads();
  for (int base = 0; base < K1; base += T_WG) {
    const int k1 = base + tid;
    int k2 = -1, v = SPFE_TRI_NONE;
    float X[3] = {0.0f, 0.0f, 0.0f};
    if (k1 < K1) {
      k2 = match12[k1];
      if (k2 >= 0 && k2 < K2)
        v = spfe_tri_triangulate(&c1, &c2, a.xy1[2 * k1], a.xy1[2 * k1 + 1], a.cinv1[2 * k1], a.cinv1[2 * k1 + 1], a.xy2[2 * k2],
                                 a.xy2[2 * k2 + 1], a.cinv2[2 * k2], a.cinv2[2 * k2 + 1], a.cos_parallax_max, a.chi2_reproj,
                                 SPFE_TRI_JACOBI_SWEEPS, X);
      verdict[k1] = v;
    }
    if (v == SPFE_TRI_PARALLAX) atomicAdd(&rejects[0], 1);
    else if (v == SPFE_TRI_DEPTH) atomicAdd(&rejects[1], 1);
    else if (v == SPFE_TRI_REPROJ) atomicAdd(&rejects[2], 1);
    else if (v == SPFE_TRI_DEGENERATE) atomicAdd(&rejects[3], 1);
    const bool fresh = v == SPFE_TRI_NEW;
    int total;
    const int rank = wg_ordered_rank<T_WG>(fresh, lane, wave, wave_total, &total);
    if (fresh) {
      const int t = done + rank;   // t < K1 <= kmax: one success per k1 at the most
      new_xyz[3 * t] = X[0];
      new_xyz[3 * t + 1] = X[1];
      new_xyz[3 * t + 2] = X[2];
      new_k1[t] = k1;
      new_k2[t] = k2;
      a.mp1[k1] = id0 + t;
      a.mp2[k2] = id0 + t;
    }
    done += total;
    __syncthreads();   // wave_total is rewritten by the next chunk
  }
  if (tid == 0) {
    *tri_field(a.out, SPFE_TRI_OFF_N_NEW) = done;
    *tri_field(a.out, SPFE_TRI_OFF_N_REJ_PARALLAX) = rejects[0];
    *tri_field(a.out, SPFE_TRI_OFF_N_REJ_DEPTH) = rejects[1];
    *tri_field(a.out, SPFE_TRI_OFF_N_REJ_REPROJ) = rejects[2];
    *tri_field(a.out, SPFE_TRI_OFF_N_REJ_DEGENERATE) = rejects[3];
    *a.next_id = id0 + done;
  }
}

hipError_t launch_tri_begin(const TriArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(tri_begin_kernel, dim3(1), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_tri_gate_triangulate(const TriArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(tri_gate_kernel, dim3((a.kmax + 255) / 256), dim3(256), 0, s, a);
  hipLaunchKernelGGL(tri_triangulate_kernel, dim3(1), dim3(T_WG), 0, s, a);
  return hipGetLastError();
}

}  // namespace spfe
