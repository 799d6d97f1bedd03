// fuse.hip — the search of SPMatcher::Fuse(KeyFrame *, const vector<MapPoint *> &, th) (sp_matcher.cpp:965-1104, with
// KeyFrame::GetFeaturesInArea / IsInImage, keyframe.cpp:1018-1060) as LocalMapping::SearchInNeighbors calls it
// (local_mapper.cpp:854-860, :888): one shared list of map points projected into n_targets keyframes whose records are
// resident in HBM.  The arithmetic is include/spfe_fuse_math.h (on spfe_proj_math.h); the host statement the tests hold these
// kernels to is tests/fuse_ref/fuse_ref.c: every output is equal bit for bit.
//
//   fuse_search_kernel   target j = blockIdx.y, one wavefront per map point, four points per workgroup.  IsInKeyFrame is
//                        wave_holds_id on the target's kf_mp_of_kp; the projection and the gates are wave-uniform; then
//                        wave_search.h's window walk with the chi-square gate.  Nothing is kept per candidate: Fuse blocks
//                        no keypoint, so the running best is the answer.
//   fuse_compact_kernel  one workgroup per target walks the points 1024 at a time: fused_idx is the ordered compaction of
//                        the proposed points (wg_ordered_rank) and the block's three int32 fields.
// Nothing here writes kf_mp_of_kp, and nothing synchronises with the host.
#include "../../include/spfe.h"
#include "../../include/spfe_fuse_math.h"
#include "spfe_kernels.h"
#include "wave_search.h"

static_assert(SPFE_PROJ_POINT_SEARCHABLE == SPFE_PROJ_SEARCHABLE, "flags");
static_assert(SPFE_FUSE_R_SKIP_BAD == SPFE_FUSE_SKIP_BAD && SPFE_FUSE_R_SKIP_IN_KF == SPFE_FUSE_SKIP_IN_KF &&
              SPFE_FUSE_R_BEHIND == SPFE_FUSE_BEHIND && SPFE_FUSE_R_OUTSIDE == SPFE_FUSE_OUTSIDE &&
              SPFE_FUSE_R_RANGE == SPFE_FUSE_RANGE && SPFE_FUSE_R_ANGLE == SPFE_FUSE_ANGLE &&
              SPFE_FUSE_R_NO_CANDIDATE == SPFE_FUSE_NO_CANDIDATE && SPFE_FUSE_R_TOO_FAR == SPFE_FUSE_TOO_FAR &&
              SPFE_FUSE_R_PROPOSED == SPFE_FUSE_PROPOSED, "reason codes");

namespace spfe {

static_assert(FUSE_MAX_TARGETS == SPFE_FUSE_MAX_TARGETS, "targets");

namespace {
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
  if (!reason && wave_holds_id(t.mp, K, a.point_id[i], lane)) reason = SPFE_FUSE_SKIP_IN_KF;   // MapPoint::IsInKeyFrame
  float u = 0.0f, v = 0.0f;
  if (!reason) {
    float Tcw[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) Tcw[k] = t.Tcw[k];
    spfe_proj_cam cam;
    spfe_proj_cam_from_f32(Tcw, &cam);
    const spfe_fuse_view vw = fuse_view_of(a);
    const float P[3] = {a.xyz[3 * i], a.xyz[3 * i + 1], a.xyz[3 * i + 2]};
    const float N[3] = {a.normal[3 * i], a.normal[3 * i + 1], a.normal[3 * i + 2]};
    reason = spfe_fuse_project(&cam, &vw, P, N, a.dist_range[2 * i], a.dist_range[2 * i + 1], &u, &v);
  }
  if (!reason) {   // wave-uniform: the window
    const float4 m4 = *reinterpret_cast<const float4 *>(a.desc + (size_t)i * 256 + lane * 4);
    const float mf[4] = {m4.x, m4.y, m4.z, m4.w};
    wave_window_search(
        t.occ, a.wc, a.hc, t.kp_xy, K, u, v, a.th, lane,
        [&](float kx, float ky) { return spfe_fuse_chi2_pass(kx, ky, u, v, a.chi2) != 0; },
        [&](int kk, float, float) {
          const float d = wave_desc_dist(mf, t.kp_desc, kk, lane, a.kp_desc_bf16);
          if (d < best) { best = d; best_k = kk; }
        });
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
    int total;
    const int rank = wg_ordered_rank<FU_WG>(prop, lane, wave, wave_total, &total);
    if (prop) fused_idx[done + rank] = i;   // < n <= cap: one entry per point at the most
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
