// wave_search.h — what the searches on a record share on the device (proj.hip, fuse.hip, loopfuse.hip, guided.hip; match.hip
// and mappoint.hip take the descriptor load and distance): everything here is inlined into its kernel, and the arithmetic stays
// in include/spfe_proj_math.h.  The ordered compaction of the searches (wg_ordered_rank) is wave_ops.h's, included here.
//
// The window search of ONE wavefront for ONE projected point (u, v) with radius r in a record's occupancy grid:
// Frame::GetFeaturesInArea (frame.cpp:390-430) / KeyFrame::GetFeaturesInArea (keyframe.cpp:1018-1060).  Every lane holds the
// same u, v, r (same inputs, same operations: same bits in all 64 lanes, which is what a broadcast of lane 0's would give).
// The window's cells are numbered in the reference's order, ix outer, iy inner (frame.cpp:405-406, keyframe.cpp:1040-1041);
// lane c tests cell c, 64 cells per pass, and a ballot turns the survivors into the candidate list in that order.  Per
// candidate each lane loads 16 bytes of both descriptors and the wave does the double butterfly.
#pragma once
#include "../../include/spfe.h"
#include "../../include/spfe_fuse_math.h"
#include "spfe_kernels.h"
#include "wave_ops.h"

namespace spfe {

// four consecutive descriptor elements from element index e: f32 rows, or bf16 rows widened (exact)
__device__ __forceinline__ float4 desc4(const float *rows, size_t e, int bf16) {
  if (!bf16) return *reinterpret_cast<const float4 *>(rows + e);
  const uint2 p = *reinterpret_cast<const uint2 *>(reinterpret_cast<const unsigned short *>(rows) + e);
  return make_float4(__uint_as_float(p.x << 16), __uint_as_float(p.x & 0xffff0000u), __uint_as_float(p.y << 16),
                     __uint_as_float(p.y & 0xffff0000u));
}

// the distance between the descriptor whose elements 4 lane .. 4 lane + 3 this lane holds in mf and row kk of kp_desc
// (wave-uniform kk).  The same bits in every lane: both operands of every level's sum are swapped.
__device__ __forceinline__ float wave_desc_dist(const float mf[4], const float *kp_desc, int kk, int lane, int bf16) {
  const float4 k4 = desc4(kp_desc, (size_t)kk * 256 + lane * 4, bf16);
  const float kf[4] = {k4.x, k4.y, k4.z, k4.w};
  double s = spfe_proj_lane_sum(mf, kf);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s = s + __shfl_xor(s, off, 64);
  return spfe_proj_dist(s);
}

// The walk.  gate(kx, ky) is a further per-lane test of a cell's keypoint; visit(kk, kx, ky) runs wave-uniformly once per
// candidate, in candidate order, with the keypoint's index and position.
template <class Gate, class Visit>
__device__ __forceinline__ void wave_window_search(const int16_t *occ, int wc, int hc, const float *kp_xy, int K, float u, float v,
                                                   float r, int lane, Gate gate, Visit visit) {
  int x0, x1, y0, y1;
  spfe_proj_window(u, r, wc, &x0, &x1);
  spfe_proj_window(v, r, hc, &y0, &y1);
  // (the host refused radii beyond SPFE_PROJ_MAX_RADIUS: the clamps cannot bind)
  const int nx = min(max(x1 - x0 + 1, 0), SPFE_PROJ_MAX_CELLS_AXIS), ny = min(max(y1 - y0 + 1, 0), SPFE_PROJ_MAX_CELLS_AXIS);
  const int total = nx * ny;
  for (int base = 0; base < total; base += 64) {
    const int c = base + lane;
    int k = -1;
    float kx = 0.0f, ky = 0.0f;
    bool cand = false;
    if (c < total) {
      const int ix = x0 + c / ny, iy = y0 + c % ny;
      k = occ[iy * wc + ix];
      if (k >= 0 && k < K) {
        kx = kp_xy[2 * k];
        ky = kp_xy[2 * k + 1];
        cand = spfe_proj_in_window(kx, ky, u, v, r) && gate(kx, ky);
      }
    }
    unsigned long long mask = __ballot(cand);
    while (mask) {
      const int src = __builtin_ctzll(mask);
      mask &= mask - 1;
      visit(__shfl(k, src, 64), __shfl(kx, src, 64), __shfl(ky, src, 64));
    }
  }
}
struct no_gate {
  __device__ __forceinline__ bool operator()(float, float) const { return true; }
};

// does ids[0 .. K) hold id?  Lane l compares entries l, l + 64, ..., a ballot decides.
__device__ __forceinline__ bool wave_holds_id(const int *ids, int K, int id, int lane) {
  bool hit = false;
  for (int k = lane; k < K; k += 64) hit |= ids[k] == id;
  return __ballot(hit) != 0;
}

// the view of spfe_fuse_project from a FuseArgs / LoopProjArgs
template <class Args>
__device__ __forceinline__ spfe_fuse_view fuse_view_of(const Args &a) {
  spfe_fuse_view vw;
  vw.fx = a.fx; vw.fy = a.fy; vw.cx = a.cx; vw.cy = a.cy; vw.W = a.W; vw.H = a.H;
  vw.min_factor = a.min_factor; vw.max_factor = a.max_factor; vw.view_cos = a.view_cos;
  return vw;
}

// target j's view of a FuseArgs
struct FuseTarget {
  const float *kp_xy;
  const int16_t *occ;
  const float *kp_desc;
  const int *mp;
  const float *Tcw;
  uint8_t *out;
  int K, status;
};
__device__ __forceinline__ FuseTarget fuse_target(const FuseArgs &a, int j) {
  const uint8_t *b = a.base[j];
  FuseTarget t;
  t.kp_xy = reinterpret_cast<const float *>(b + a.off_xy);
  t.occ = reinterpret_cast<const int16_t *>(b + a.off_occ);
  t.kp_desc = reinterpret_cast<const float *>(b + a.off_desc);
  t.mp = a.kf_mp_of_kp + (size_t)j * a.kmax;
  t.Tcw = a.Tcw + 16 * (size_t)j;
  t.out = a.out + (size_t)j * SPFE_FUSE_OUT_BYTES(a.cap);
  t.K = a.k_imm;
  t.status = 0;
  if (a.off_hdr >= 0) {
    const int *hdr = reinterpret_cast<const int *>(b + a.off_hdr);
    t.K = min(max(hdr[0], 0), a.kmax);
    t.status = hdr[2];
  }
  return t;
}

}  // namespace spfe
