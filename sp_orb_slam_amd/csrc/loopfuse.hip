// loopfuse.hip — the device side of the loop closer's fusion step (LoopClosingVLAD::CorrectLoop / SearchAndFuse,
// loop_closer_vlad.cpp:536-571, :608-618, :701-726): the search of SPMatcher::Fuse(KeyFrame *, cv::Mat Scw, const
// vector<MapPoint *> &, th, vpReplacePoint) (sp_matcher.cpp:1106-1219) of ONE shared list of loop map points in n_targets
// keyframes whose records are resident in HBM, and the corrected Sim3 / SE3 poses those searches run under.  The arithmetic
// is include/spfe_loopfuse_math.h; the host statement the tests hold these kernels to is tests/loopfuse_ref/loopfuse_ref.c:
// every output is equal bit for bit.
//
//   loopfuse_search_kernel   a workgroup (four wavefronts) serves ONE target (blockIdx.y) and a STRIP of LF_STRIP
//                            consecutive points (blockIdx.x).  It copies the target's kf_mp_of_kp[0 .. K) into dynamic LDS once
//                            and forms the camera of the target's Scw once; then wavefront w walks points w, w + 4, ... of
//                            the strip.  Per point: the id scan reads the staged holders 16 bytes per lane, a ballot decides;
//                            projection and gates run on wave-uniform values; then wave_search.h's window walk with
//                            no further gate, the running best as in fuse.hip.  Against fuse_search_kernel, where every
//                            (point, target) wavefront reads the target's whole holder array from L2 and rebuilds the
//                            camera, the holders cross the L2 once per LF_STRIP points.
//   fuse_compact_kernel      fuse.hip's, through launch_fuse_compact: the block has the fuse block's layout and codes.
//   loopfuse_poses_kernel    one thread per connected keyframe: spfe_loopfuse_pose.
// Nothing here writes kf_mp_of_kp, and nothing synchronises with the host.
#include "../../include/spfe.h"
#include "../../include/spfe_loopfuse_math.h"
#include "spfe_kernels.h"
#include "wave_search.h"

static_assert(SPFE_LOOPFUSE_R_SKIP_BAD == SPFE_LOOPFUSE_SKIP_BAD && SPFE_LOOPFUSE_R_SKIP_IN_KF == SPFE_LOOPFUSE_SKIP_IN_KF &&
              SPFE_LOOPFUSE_R_BEHIND == SPFE_LOOPFUSE_BEHIND && SPFE_LOOPFUSE_R_OUTSIDE == SPFE_LOOPFUSE_OUTSIDE &&
              SPFE_LOOPFUSE_R_RANGE == SPFE_LOOPFUSE_RANGE && SPFE_LOOPFUSE_R_ANGLE == SPFE_LOOPFUSE_ANGLE &&
              SPFE_LOOPFUSE_R_NO_CANDIDATE == SPFE_LOOPFUSE_NO_CANDIDATE && SPFE_LOOPFUSE_R_TOO_FAR == SPFE_LOOPFUSE_TOO_FAR &&
              SPFE_LOOPFUSE_R_PROPOSED == SPFE_LOOPFUSE_PROPOSED, "reason codes");
static_assert(SPFE_LOOPFUSE_OUT_BYTES(1000) == SPFE_FUSE_OUT_BYTES(1000) && SPFE_LOOPFUSE_OFF_REASON(7) == SPFE_FUSE_OFF_REASON(7),
              "the block is the fuse block");

namespace spfe {

namespace {
constexpr int LF_WAVES = 4;
constexpr int LF_STRIP = SPFE_LOOPFUSE_STRIP;
static_assert(LF_STRIP % LF_WAVES == 0, "strip");
}  // namespace

size_t loopfuse_lds_bytes(int kmax) { return ((size_t)(kmax > 0 ? kmax : 1) * 4 + 15) / 16 * 16; }

__global__ __launch_bounds__(LF_WAVES * 64) void loopfuse_search_kernel(FuseArgs a) {
  extern __shared__ __attribute__((aligned(16))) int lf_mp[];   // kf_mp_of_kp[0 .. K) of this target
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const FuseTarget t = fuse_target(a, blockIdx.y);
  const int K = t.K;   // <= kmax, what the launch sized the LDS for
  for (int k = threadIdx.x; k < K; k += LF_WAVES * 64) lf_mp[k] = t.mp[k];

  // the camera of this target's Scw and the view: once per workgroup, the same bits in every lane
  float Scw[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) Scw[k] = t.Tcw[k];
  spfe_proj_cam cam;
  spfe_loop_cam_from_scw(Scw, &cam);
  const spfe_fuse_view vw = fuse_view_of(a);
  __syncthreads();

  const int K4 = K >> 2;
  const int4 *mp4 = reinterpret_cast<const int4 *>(lf_mp);
  const int i_end = min((int)(blockIdx.x + 1) * LF_STRIP, a.n);
  for (int i = blockIdx.x * LF_STRIP + wave; i < i_end; i += LF_WAVES) {   // wave-uniform
    int reason = 0, best_k = -1, any = 0;
    float best = spfe_loopfuse_best_init();
    if (!(a.flags[i] & SPFE_PROJ_SEARCHABLE)) reason = SPFE_LOOPFUSE_SKIP_BAD;
    if (!reason) {   // spAlreadyFound.count(pMP): K compares out of LDS
      const int id = a.point_id[i];
      bool hit = false;
      for (int q = lane; q < K4; q += 64) {
        const int4 m = mp4[q];
        hit |= (m.x == id) | (m.y == id) | (m.z == id) | (m.w == id);
      }
      if (lane < (K & 3)) hit |= lf_mp[4 * K4 + lane] == id;
      if (__ballot(hit)) reason = SPFE_LOOPFUSE_SKIP_IN_KF;
    }
    float u = 0.0f, v = 0.0f;
    if (!reason) {
      const float P[3] = {a.xyz[3 * i], a.xyz[3 * i + 1], a.xyz[3 * i + 2]};
      const float N[3] = {a.normal[3 * i], a.normal[3 * i + 1], a.normal[3 * i + 2]};
      reason = spfe_fuse_project(&cam, &vw, P, N, a.dist_range[2 * i], a.dist_range[2 * i + 1], &u, &v);
    }
    if (!reason) {   // wave-uniform: the window
      const float4 m4 = *reinterpret_cast<const float4 *>(a.desc + (size_t)i * 256 + lane * 4);
      const float mf[4] = {m4.x, m4.y, m4.z, m4.w};
      wave_window_search(t.occ, a.wc, a.hc, t.kp_xy, K, u, v, a.th, lane, no_gate(), [&](int kk, float, float) {
        any = 1;   // (no chi-square gate: a keypoint of the window is a candidate)
        const float d = wave_desc_dist(mf, t.kp_desc, kk, lane, a.kp_desc_bf16);
        if (d < best) { best = d; best_k = kk; }
      });
      reason = spfe_loopfuse_verdict(any, best_k, best, a.th_dist);
    }
    if (lane == 0) {
      const bool prop = reason == SPFE_LOOPFUSE_PROPOSED;   // then 0 <= best_k < K
      reinterpret_cast<int *>(t.out + SPFE_FUSE_OFF_KP_OF_MP)[i] = prop ? best_k : -1;
      reinterpret_cast<float *>(t.out + SPFE_FUSE_OFF_BEST_DIST(a.cap))[i] = prop ? best : 0.0f;
      reinterpret_cast<int *>(t.out + SPFE_FUSE_OFF_HOLDER(a.cap))[i] = prop ? lf_mp[best_k] : -1;
      (t.out + SPFE_FUSE_OFF_REASON(a.cap))[i] = (uint8_t)reason;
    }
  }
}

__global__ __launch_bounds__(64) void loopfuse_poses_kernel(const double *S12, const float *Tcw2, const float *Twc, const float *Tiw,
                                                             int n_targets, int cur_index, float *Siw, float *Tiw_corrected) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= n_targets) return;
  double s12[13];
  float tcw2[16], twc[16], tiw[16], siw[16], tc[16];
#pragma unroll
  for (int k = 0; k < 13; ++k) s12[k] = S12[k];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    tcw2[k] = Tcw2[k];
    twc[k] = Twc[k];
    tiw[k] = Tiw[16 * (size_t)j + k];
  }
  spfe_loopfuse_pose(s12, tcw2, twc, tiw, j == cur_index, siw, tc);
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    Siw[16 * (size_t)j + k] = siw[k];
    Tiw_corrected[16 * (size_t)j + k] = tc[k];
  }
}

hipError_t launch_loopfuse_search(const FuseArgs &a, hipStream_t s) {
  if (a.n_targets < 1 || a.n_targets > FUSE_MAX_TARGETS || a.cap < 1 || a.cap > SPFE_PROJ_MAX_POINTS || a.n < 0 || a.n > a.cap ||
      a.kmax < 1 || a.kmax > 32767)
    return hipErrorInvalidValue;
  const size_t lds = loopfuse_lds_bytes(a.kmax);
  if (lds > 48 * 1024) {   // beyond the default dynamic-LDS limit (the host-array form alone gets here): raise it
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(loopfuse_search_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  if (a.n > 0)
    hipLaunchKernelGGL(loopfuse_search_kernel, dim3((a.n + LF_STRIP - 1) / LF_STRIP, a.n_targets), dim3(LF_WAVES * 64), lds, s, a);
  return launch_fuse_compact(a, s);
}

hipError_t launch_loopfuse_poses(const double *S12, const float *Tcw2, const float *Twc, const float *Tiw, int n_targets,
                                 int cur_index, float *Siw, float *Tiw_corrected, hipStream_t s) {
  if (n_targets < 1 || n_targets > FUSE_MAX_TARGETS || cur_index < -1 || cur_index >= n_targets) return hipErrorInvalidValue;
  hipLaunchKernelGGL(loopfuse_poses_kernel, dim3((n_targets + 63) / 64), dim3(64), 0, s, S12, Tcw2, Twc, Tiw, n_targets, cur_index,
                     Siw, Tiw_corrected);
  return hipGetLastError();
}

}  // namespace spfe
