// fuse.hip — the search of SPMatcher::Fuse(KeyFrame *, const vector<MapPoint *> &, th) (sp_matcher.cpp:965-1104, with
// KeyFrame::GetFeaturesInArea / IsInImage, keyframe.cpp:1018-1060) as LocalMapping::SearchInNeighbors calls it
// (local_mapper.cpp:854-860, :888): one shared list of map points projected into n_targets keyframes whose records are
// resident in HBM.  The arithmetic is include/spfe_fuse_math.h (on spfe_proj_math.h); the host statement the tests hold these
// kernels to is tests/fuse_ref/fuse_ref.c: every output is equal bit for bit.
//
//   fuse_search_kernel   target j = blockIdx.y, one wavefront per map point, four points per workgroup (as
//                        proj_candidates_kernel maps them).  IsInKeyFrame is a scan of the target's kf_mp_of_kp for the
//                        point's id: lane l compares entries l, l + 64, ..., a ballot decides.  Every lane evaluates the
//                        projection and the gates (same inputs, same operations: same bits in all 64 lanes); lane c tests
//                        cell c of the window in the reference's order (ix outer, iy inner), a ballot turns the survivors
//                        into the candidate list in that order, and per candidate each lane loads 16 bytes of both
//                        descriptors and the wave does the butterfly.  Nothing is kept per candidate: Fuse blocks no
//                        keypoint, so the running best is the answer.
//   fuse_compact_kernel  one workgroup per target walks the points 1024 at a time: fused_idx is the ordered compaction of
//                        the proposed points — ballot + popcount inside a wavefront, the 16 wavefront totals through LDS, as
//                        tri_triangulate_kernel does — and the block's three int32 fields.
// Nothing here writes kf_mp_of_kp, and nothing synchronises with the host.
#include "../../include/spfe.h"
#include "../../include/spfe_fuse_math.h"
#include "spfe_kernels.h"
#include "fuse_target.h"

static_assert(SPFE_PROJ_POINT_SEARCHABLE == SPFE_PROJ_SEARCHABLE, "flags");
static_assert(SPFE_FUSE_R_SKIP_BAD == SPFE_FUSE_SKIP_BAD && SPFE_FUSE_R_SKIP_IN_KF == SPFE_FUSE_SKIP_IN_KF &&
              SPFE_FUSE_R_BEHIND == SPFE_FUSE_BEHIND && SPFE_FUSE_R_OUTSIDE == SPFE_FUSE_OUTSIDE &&
              SPFE_FUSE_R_RANGE == SPFE_FUSE_RANGE && SPFE_FUSE_R_ANGLE == SPFE_FUSE_ANGLE &&
              SPFE_FUSE_R_NO_CANDIDATE == SPFE_FUSE_NO_CANDIDATE && SPFE_FUSE_R_TOO_FAR == SPFE_FUSE_TOO_FAR &&
              SPFE_FUSE_R_PROPOSED == SPFE_FUSE_PROPOSED, "reason codes");

namespace spfe {

static_assert(FUSE_MAX_TARGETS == SPFE_FUSE_MAX_TARGETS, "targets");

namespace {
constexpr int FU_AXIS = SPFE_PROJ_MAX_CELLS_AXIS;
constexpr int FU_WG = 1024;

}  // namespace

__global__ __launch_bounds__(256) void fuse_search_kernel(FuseArgs a) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.n) return;   // wave-uniform
  const FuseTarget t = fuse_target(a, blockIdx.y);
  const int K = t.K;

  int reason = 0, best_k = -1;
  float best = spfe_fuse_best_init();
  if (!(a.flags[i] & SPFE_PROJ_SEARCHABLE)) reason = SPFE_FUSE_SKIP_BAD;
  if (!reason) {   // MapPoint::IsInKeyFrame: K compares
    const int id = a.point_id[i];
    bool hit = false;
    for (int k = lane; k < K; k += 64) hit |= t.mp[k] == id;
    if (__ballot(hit)) reason = SPFE_FUSE_SKIP_IN_KF;
  }
  float u = 0.0f, v = 0.0f;
  if (!reason) {
    float Tcw[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) Tcw[k] = t.Tcw[k];
    spfe_proj_cam cam;
    spfe_proj_cam_from_f32(Tcw, &cam);
    spfe_fuse_view vw;
    vw.fx = a.fx; vw.fy = a.fy; vw.cx = a.cx; vw.cy = a.cy; vw.W = a.W; vw.H = a.H;
    vw.min_factor = a.min_factor; vw.max_factor = a.max_factor; vw.view_cos = a.view_cos;
    const float P[3] = {a.xyz[3 * i], a.xyz[3 * i + 1], a.xyz[3 * i + 2]};
    const float N[3] = {a.normal[3 * i], a.normal[3 * i + 1], a.normal[3 * i + 2]};
    reason = spfe_fuse_project(&cam, &vw, P, N, a.dist_range[2 * i], a.dist_range[2 * i + 1], &u, &v);
  }
  if (!reason) {   // wave-uniform: the window
    const float r = a.th;
    int x0, x1, y0, y1;
    spfe_proj_window(u, r, a.wc, &x0, &x1);
    spfe_proj_window(v, r, a.hc, &y0, &y1);
    // (the host refused radii beyond SPFE_PROJ_MAX_RADIUS: the clamps cannot bind)
    const int nx = min(max(x1 - x0 + 1, 0), FU_AXIS), ny = min(max(y1 - y0 + 1, 0), FU_AXIS);
    const int total = nx * ny;
    const float4 m4 = *reinterpret_cast<const float4 *>(a.desc + (size_t)i * 256 + lane * 4);
    const float mf[4] = {m4.x, m4.y, m4.z, m4.w};
    for (int base = 0; base < total; base += 64) {
      const int c = base + lane;
      int k = -1;
      bool cand = false;
      if (c < total) {
        const int ix = x0 + c / ny, iy = y0 + c % ny;   // ix outer, iy inner (keyframe.cpp:1040-1041)
        k = t.occ[iy * a.wc + ix];
        if (k >= 0 && k < K) {
          const float kx = t.kp_xy[2 * k], ky = t.kp_xy[2 * k + 1];
          cand = spfe_proj_in_window(kx, ky, u, v, r) && spfe_fuse_chi2_pass(kx, ky, u, v, a.chi2);
        }
      }
      unsigned long long mask = __ballot(cand);
      while (mask) {
        const int src = __builtin_ctzll(mask);
        mask &= mask - 1;
        const int kk = __shfl(k, src, 64);
        const float4 k4 = fuse_desc4(t.kp_desc, (size_t)kk * 256 + lane * 4, a.kp_desc_bf16);
        const float kf[4] = {k4.x, k4.y, k4.z, k4.w};
        double s = spfe_proj_lane_sum(mf, kf);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s = s + __shfl_xor(s, off, 64);
        const float d = spfe_proj_dist(s);   // the same bits in every lane: both operands of every level's sum are swapped
        if (d < best) { best = d; best_k = kk; }
      }
    }
    reason = best_k < 0 ? SPFE_FUSE_NO_CANDIDATE : (best > a.th_dist ? SPFE_FUSE_TOO_FAR : SPFE_FUSE_PROPOSED);
  }
  if (lane == 0) {
    const bool prop = reason == SPFE_FUSE_PROPOSED;
    reinterpret_cast<int *>(t.out + SPFE_FUSE_OFF_KP_OF_MP)[i] = prop ? best_k : -1;
    reinterpret_cast<float *>(t.out + SPFE_FUSE_OFF_BEST_DIST(a.cap))[i] = prop ? best : 0.0f;
    reinterpret_cast<int *>(t.out + SPFE_FUSE_OFF_HOLDER(a.cap))[i] = prop ? t.mp[best_k] : -1;
    (t.out + SPFE_FUSE_OFF_REASON(a.cap))[i] = (uint8_t)reason;
  }
}

__global__ __launch_bounds__(FU_WG) void fuse_compact_kernel(FuseArgs a) {
  __shared__ int wave_total[FU_WG / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const FuseTarget t = fuse_target(a, blockIdx.x);
  const uint8_t *reason = t.out + SPFE_FUSE_OFF_REASON(a.cap);
  int *fused_idx = reinterpret_cast<int *>(t.out + SPFE_FUSE_OFF_FUSED_IDX(a.cap));
  int done = 0;   // proposals of the chunks below this one (the same in every lane)
  for (int base = 0; base < a.n; base += FU_WG) {
    const int i = base + tid;
    const bool prop = i < a.n && reason[i] == SPFE_FUSE_PROPOSED;
    const unsigned long long votes = __ballot(prop);
    const int rank = __popcll(votes & ((1ull << lane) - 1ull));
    if (lane == 0) wave_total[wave] = __popcll(votes);
    __syncthreads();
    int below = 0, total = 0;
#pragma unroll
    for (int w = 0; w < FU_WG / 64; ++w) {
      const int c = wave_total[w];
      below += w < wave ? c : 0;
      total += c;
    }
    if (prop) fused_idx[done + below + rank] = i;   // < n <= cap: one entry per point at the most
    done += total;
    __syncthreads();   // wave_total is rewritten by the next chunk
  }
  if (tid == 0) {
    int *hdr = reinterpret_cast<int *>(t.out);
    hdr[SPFE_FUSE_OFF_N_FUSED / 4] = done;
    hdr[SPFE_FUSE_OFF_N / 4] = a.n;
    hdr[SPFE_FUSE_OFF_STATUS / 4] = t.status;
  }
}

hipError_t launch_fuse_search(const FuseArgs &a, hipStream_t s) {
  if (a.n_targets < 1 || a.n_targets > FUSE_MAX_TARGETS || a.cap < 1 || a.cap > SPFE_PROJ_MAX_POINTS || a.n < 0 || a.n > a.cap ||
      a.kmax < 1)
    return hipErrorInvalidValue;
  if (a.n > 0) hipLaunchKernelGGL(fuse_search_kernel, dim3((a.n + 3) / 4, a.n_targets), dim3(256), 0, s, a);
  return launch_fuse_compact(a, s);
}

hipError_t launch_fuse_compact(const FuseArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(fuse_compact_kernel, dim3(a.n_targets), dim3(FU_WG), 0, s, a);
  return hipGetLastError();
}

}  // namespace spfe
