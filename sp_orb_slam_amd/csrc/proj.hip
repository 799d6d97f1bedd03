// proj.hip — window search by projection on the GPU: SPMatcher::SearchByProjection against a local map
// (orb_slam2/src/cv/sp_matcher.cpp:344-432, behind Frame::isInFrustum, src/type/frame.cpp:330-380, as
// Tracking::SearchLocalPoints calls them, src/tracking/tracker.cpp:768-832) and against the last frame
// (sp_matcher.cpp:1439-1543), on what a record holds: kp_xy, occ_grid, descriptors.  The arithmetic is
// include/spfe_proj_math.h; the host statement the tests hold these kernels to is tests/proj_ref/proj_ref.c.
//
// The structure is the patch association's (match.hip): the distances are independent, the claims are ordered.
//   proj_prepare_kernel     LOCAL_MAP: what SearchLocalPoints does to mvpMapPoints first — keypoints that hold a point
//                           that is not searchable are emptied, the points the others hold are marked (they are not
//                           searched: mnLastFrameSeen).  One workgroup per frame.
//   proj_candidates_kernel  one wavefront per map point: the projection, then wave_search.h's window walk; every keypoint of
//                           the window goes into the candidate list, in window order.
//   proj_resolve_kernel     the ordered greedy claim as a fixed point, one workgroup per frame.  State: the holder of
//                           every keypoint (mp_of_kp) and whether it is blocked (holds an OBSERVED point), in LDS.  Each
//                           round every unfinished point posts its index on its unblocked candidates (atomic min); a
//                           point that finds ITSELF on all of them is final: no earlier unfinished point shares a
//                           keypoint it could still take, so nothing an earlier point does later can change what it
//                           sees, and nothing it does can change what an earlier point sees.  It takes its nearest
//                           unblocked candidate (first on ties), applies the acceptance rule, writes itself into the
//                           holder array and blocks the keypoint if it is OBSERVED.  Two points that finish in the same
//                           round share no unblocked candidate, and of two points that share one the earlier always
//                           finishes in an earlier round: writes to one keypoint happen in index order, so the plain
//                           store is "the last writer wins".  The lowest unfinished index is always final, so n points
//                           need at most n rounds (the chain in which every point contests its predecessor's keypoint
//                           takes exactly that), and the result does not depend on the number of rounds.
//   local_map_verdict_kernel  mnMatchesInliers and TrackLocalMap's verdict into the pose block (tracker.cpp:576-612).
//   track_discard_kernel    "Discard outliers" of TrackWithMotionModel / trackReferenceKeyFrameANN behind PoseOptimization
//                           (tracker.cpp:519-535, :395-410), the counts and the verdict into the pose block.
// The gated form (ProjArgs::gate_count) is TrackWithMotionModel's retry with the doubled window (tracker.cpp:503-508) decided
// on the device: the same launches again, which return at once unless the first search found too little.
#include <float.h>

#include "../../include/spfe.h"
#include "../../include/spfe_proj_math.h"
#include "spfe_kernels.h"
#include "wave_search.h"

static_assert(SPFE_PROJ_MODE_LOCAL_MAP == SPFE_PROJ_LOCAL_MAP && SPFE_PROJ_MODE_LAST_FRAME == SPFE_PROJ_LAST_FRAME, "modes");
static_assert(SPFE_PROJ_POINT_SEARCHABLE == SPFE_PROJ_SEARCHABLE && SPFE_PROJ_POINT_OBSERVED == SPFE_PROJ_OBSERVED, "flags");

namespace spfe {

namespace {
constexpr int PJ_CAND = SPFE_PROJ_MAX_CAND;
constexpr int PJ_RES_THREADS = 1024;
constexpr int PJ_PER = SPFE_PROJ_MAX_POINTS / PJ_RES_THREADS;   // map points per thread of the resolve workgroup
constexpr size_t PJ_LDS_MAX = 160 * 1024;
// proj_resolve_kernel's static LDS: pending, s_matches, s_view (12 bytes), padded to the 16-byte alignment of the dynamic
// array behind them (the kernel descriptor's group-segment size)
constexpr size_t PJ_LDS_STATIC = 16;
static_assert(PJ_LDS_STATIC + 9 * (size_t)SPFE_PROJ_MAX_KEYPOINTS + 16 <= PJ_LDS_MAX &&
              PJ_LDS_STATIC + 9 * (size_t)(SPFE_PROJ_MAX_KEYPOINTS + 1) + 16 > PJ_LDS_MAX, "SPFE_PROJ_MAX_KEYPOINTS");
static_assert(PJ_PER * PJ_RES_THREADS == SPFE_PROJ_MAX_POINTS, "points per thread");

template <class T>
__device__ __forceinline__ T *at(T *p, size_t bytes) {
  return reinterpret_cast<T *>(reinterpret_cast<uintptr_t>(p) + bytes);
}
// frame f's view of the arguments
__device__ __forceinline__ void select_frame(ProjArgs &a, size_t f) {
  a.kp_xy = at(a.kp_xy, f * a.rec_stride);
  a.occ = at(a.occ, f * a.rec_stride);
  a.kp_desc = at(a.kp_desc, f * a.rec_stride);
  if (a.hdr) a.hdr = at(a.hdr, f * a.rec_stride);
  a.xyz = at(a.xyz, f * a.xyz_stride);
  a.normal = at(a.normal, f * a.xyz_stride);
  a.desc = at(a.desc, f * a.desc_stride);
  a.flags = at(a.flags, f * a.flags_stride);
  a.mp_of_kp = at(a.mp_of_kp, f * a.map_stride);
  a.Tcw = at(a.Tcw, f * a.pose_stride);
  a.out = a.out + f * a.out_stride;
  a.cand_k += f * (size_t)a.cap * PJ_CAND;
  a.cand_d += f * (size_t)a.cap * PJ_CAND;
  a.cand_duv += f * (size_t)a.cap * PJ_CAND;
  a.cand_n += f * (size_t)a.cap;
  if (a.held) a.held += f * (size_t)a.cap;
  if (a.n_dev) a.n = min(max(a.n_dev[f], 0), a.cap);
}
__device__ __forceinline__ int frame_K(const ProjArgs &a) { return a.hdr ? min(max(a.hdr[0], 0), a.kmax) : a.k_imm; }
__device__ __forceinline__ bool frame_refused(const ProjArgs &a) {
  return a.refuse_overflow && a.hdr && (a.hdr[2] & SPFE_STATUS_COV_OVERFLOW);
}
// gated form: does this run search?  (uniform over the launch: one frame, one count)
__device__ __forceinline__ bool gate_open(const ProjArgs &a) { return !frame_refused(a) && a.gate_count[0] < a.gate_min; }
}  // namespace

__global__ __launch_bounds__(256) void proj_prepare_kernel(ProjArgs a) {
  select_frame(a, blockIdx.x);
  if (frame_refused(a)) return;
  const int n = a.n, K = frame_K(a);
  for (int i = threadIdx.x; i < n; i += 256) a.held[i] = 0;
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += 256) {
    const int m = a.mp_of_kp[k];
    if (m < 0 || m >= n) continue;
    if (a.flags[m] & SPFE_PROJ_SEARCHABLE) a.held[m] = 1;   // pMP->mnLastFrameSeen = mCurrentFrame.mnId
    else a.mp_of_kp[k] = -1;                                 // *vit = NULL for bad points
  }
}

__global__ __launch_bounds__(256) void proj_candidates_kernel(ProjArgs a) {
  select_frame(a, blockIdx.y);
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.n) return;
  if (a.gate_count && !gate_open(a)) return;
  const int K = frame_K(a);
  const unsigned fl = a.flags[i];
  bool ok = (fl & SPFE_PROJ_SEARCHABLE) && !frame_refused(a);
  if (a.mode == SPFE_PROJ_LOCAL_MAP && a.held[i]) ok = false;

  float Tcw[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) Tcw[k] = a.Tcw[k];
  spfe_proj_cam cam;
  spfe_proj_cam_from_f32(Tcw, &cam);
  const float P[3] = {a.xyz[3 * i], a.xyz[3 * i + 1], a.xyz[3 * i + 2]};
  float N[3] = {0.0f, 0.0f, 0.0f};
  if (a.mode == SPFE_PROJ_LOCAL_MAP) { N[0] = a.normal[3 * i]; N[1] = a.normal[3 * i + 1]; N[2] = a.normal[3 * i + 2]; }
  float u = 0.0f, v = 0.0f, vc = 0.0f;
  const bool in_view =
      ok && spfe_proj_project(&cam, P, N, a.fx, a.fy, a.cx, a.cy, a.W, a.H, a.mode, a.view_cos_limit, &u, &v, &vc);

  int cnt = 0;
  if (in_view) {   // wave-uniform
    const float r = spfe_proj_radius(a.mode, vc, a.th);
    const float4 m4 = *reinterpret_cast<const float4 *>(a.desc + (size_t)i * 256 + lane * 4);
    const float mf[4] = {m4.x, m4.y, m4.z, m4.w};
    int *ck = a.cand_k + (size_t)i * PJ_CAND;
    float *cd = a.cand_d + (size_t)i * PJ_CAND, *cq = a.cand_duv + (size_t)i * PJ_CAND;
    wave_window_search(a.occ, a.wc, a.hc, a.kp_xy, K, u, v, r, lane, no_gate(), [&](int kk, float kx, float ky) {
      const float d = wave_desc_dist(mf, a.kp_desc, kk, lane, a.kp_desc_bf16);
      if (lane == 0 && cnt < PJ_CAND) {
        ck[cnt] = kk;
        cd[cnt] = d;
        cq[cnt] = spfe_proj_duv(kx, ky, u, v);
      }
      cnt++;
    });
  }
  if (lane == 0) {
    a.cand_n[i] = min(cnt, PJ_CAND);
    a.out[SPFE_PROJ_OFF_VIEW + i] = in_view ? 1 : 0;
    float *uv = reinterpret_cast<float *>(a.out + SPFE_PROJ_OFF_UV);
    uv[2 * i] = in_view ? u : 0.0f;
    uv[2 * i + 1] = in_view ? v : 0.0f;
    reinterpret_cast<float *>(a.out + SPFE_PROJ_OFF_COS)[i] = in_view ? vc : 0.0f;
  }
}

__global__ __launch_bounds__(PJ_RES_THREADS) void proj_resolve_kernel(ProjArgs a) {
  extern __shared__ __attribute__((aligned(16))) int sm_pj[];
  select_frame(a, blockIdx.x);
  const int tid = threadIdx.x, n = a.n, kmax = a.kmax;
  int *holder = sm_pj;                                            // [kmax] mp_of_kp
  int *claim = holder + kmax;                                     // [kmax] earliest unfinished point that could take it
  uint8_t *blocked = reinterpret_cast<uint8_t *>(claim + kmax);   // [kmax] holds an OBSERVED point
  __shared__ int pending, s_matches, s_view;
  int *hdr_out = reinterpret_cast<int *>(a.out);
  int32_t *kp_of_mp = reinterpret_cast<int32_t *>(a.out + SPFE_PROJ_OFF_KP);
  const uint8_t *in_view = a.out + SPFE_PROJ_OFF_VIEW;
  const bool refused = frame_refused(a);
  const int K = refused ? 0 : frame_K(a);
  const bool gated = a.gate_count != nullptr;
  if (gated) {   // (the count may be this block's own n_matches: tid 0 writes that behind the barriers below)
    const bool open = gate_open(a);
    if (tid == 0 && a.gate_flag) *a.gate_flag = open ? 1 : 0;
    if (!open) return;
  }

  if (tid == 0) { s_matches = 0; s_view = 0; }
  for (int k = tid; k < K; k += PJ_RES_THREADS) {
    const int m = gated ? -1 : a.mp_of_kp[k];
    holder[k] = m;
    blocked[k] = (m >= 0 && m < n && (a.flags[m] & SPFE_PROJ_OBSERVED)) ? 1 : 0;
  }
  int cn[PJ_PER];
  bool done[PJ_PER], obs[PJ_PER];
  int views = 0;
#pragma unroll
  for (int q = 0; q < PJ_PER; ++q) {
    const int i = tid + q * PJ_RES_THREADS;
    cn[q] = 0;
    obs[q] = false;
    if (i < n) {
      cn[q] = refused ? 0 : a.cand_n[i];
      obs[q] = (a.flags[i] & SPFE_PROJ_OBSERVED) != 0;
      views += in_view[i];
      if (cn[q] == 0) kp_of_mp[i] = -1;
    }
    done[q] = cn[q] == 0;
  }
  __syncthreads();
  if (views) atomicAdd(&s_view, views);

  const float best0 = spfe_proj_best_init(a.mode);
  int matches = 0;
  for (int round = 0; round <= n; ++round) {   // at most n rounds are needed: the lowest unfinished point is always final
    for (int k = tid; k < K; k += PJ_RES_THREADS) claim[k] = 0x7fffffff;
    if (tid == 0) pending = 0;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PJ_PER; ++q) {
      if (done[q]) continue;
      const int i = tid + q * PJ_RES_THREADS;
      const int *ck = a.cand_k + (size_t)i * PJ_CAND;
      for (int c = 0; c < cn[q]; ++c) {
        const int k = ck[c];
        if (!blocked[k]) atomicMin(&claim[k], i);
      }
    }
    __syncthreads();
    bool fin[PJ_PER], acc[PJ_PER];
    int pick[PJ_PER];
#pragma unroll
    for (int q = 0; q < PJ_PER; ++q) {
      fin[q] = acc[q] = false;
      pick[q] = -1;
      if (done[q]) continue;
      const int i = tid + q * PJ_RES_THREADS;
      const int *ck = a.cand_k + (size_t)i * PJ_CAND;
      const float *cd = a.cand_d + (size_t)i * PJ_CAND;
      bool first = true;
      float best = best0;
      int bc = -1;
      for (int c = 0; c < cn[q]; ++c) {
        const int k = ck[c];
        if (blocked[k]) continue;
        if (claim[k] != i) { first = false; break; }
        const float d = cd[c];
        if (d < best) { best = d; bc = c; }
      }
      fin[q] = first;
      if (first && bc >= 0) {
        pick[q] = ck[bc];
        acc[q] = spfe_proj_accept(a.mode, best, a.cand_duv[(size_t)i * PJ_CAND + bc], a.th_dist, a.adaptive, a.c2) != 0;
      }
    }
    __syncthreads();   // every decision read `blocked` before anybody writes it
    bool mine = false;
#pragma unroll
    for (int q = 0; q < PJ_PER; ++q) {
      if (done[q]) continue;
      if (fin[q]) {
        const int i = tid + q * PJ_RES_THREADS;
        kp_of_mp[i] = acc[q] ? pick[q] : -1;
        if (acc[q]) {
          holder[pick[q]] = i;
          if (obs[q]) blocked[pick[q]] = 1;
          matches++;
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
  if (matches) atomicAdd(&s_matches, matches);
  __syncthreads();
  for (int k = tid; k < K; k += PJ_RES_THREADS) a.mp_of_kp[k] = holder[k];
  if (tid == 0) {
    hdr_out[0] = s_matches;
    hdr_out[1] = s_view;
    hdr_out[2] = n;
  }
}

__global__ __launch_bounds__(256) void local_map_verdict_kernel(const int *hdr, int kmax, const int *mp_of_kp,
                                                                const uint8_t *flags, int n, const uint8_t *proj_out,
                                                                int th_ninlier, uint8_t *pose_out) {
  __shared__ int s_cnt;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  const int K = min(max(hdr[0], 0), kmax);
  const uint8_t *outlier = pose_out + SPFE_POSE_OFF_OUTLIER;
  int c = 0;
  for (int k = threadIdx.x; k < K; k += 256) {
    const int m = mp_of_kp[k];
    if (m >= 0 && m < n && !outlier[k] && (flags[m] & SPFE_PROJ_OBSERVED)) c++;
  }
  if (c) atomicAdd(&s_cnt, c);
  __syncthreads();
  if (threadIdx.x == 0) {
    int *cnt = reinterpret_cast<int *>(pose_out + 64);
    const bool refused = (cnt[6] & SPFE_POSE_STATUS_COV_OVERFLOW) != 0;
    const int n_inliers = refused ? 0 : s_cnt;
    cnt[7] = refused ? SPFE_TRACK_FAIL_COV : (n_inliers >= th_ninlier ? SPFE_TRACK_OK : SPFE_TRACK_FAIL_LOCAL_INLIERS);
    cnt[8] = reinterpret_cast<const int *>(proj_out)[0];
    cnt[9] = n_inliers;
  }
}

__global__ __launch_bounds__(256) void track_discard_kernel(const int *hdr, int kmax, int *mp_of_kp, const uint8_t *flags, int n,
                                                            const int *n_matches_src, int th_nmatch_opt, int fail_verdict,
                                                            uint8_t *pose_out) {
  __shared__ int s_held, s_out, s_in;
  if (threadIdx.x == 0) s_held = s_out = s_in = 0;
  __syncthreads();
  const int K = min(max(hdr[0], 0), kmax);
  uint8_t *outlier = pose_out + SPFE_POSE_OFF_OUTLIER;
  int held = 0, nout = 0, nin = 0;
  for (int k = threadIdx.x; k < K; k += 256) {
    const int m = mp_of_kp[k];
    if (m < 0 || m >= n) continue;
    held++;
    if (outlier[k]) {   // mvpMapPoints[i] = NULL; mvbOutlier[i] = false
      mp_of_kp[k] = -1;
      outlier[k] = 0;
      nout++;
    } else if (flags[m] & SPFE_PROJ_OBSERVED) {
      nin++;
    }
  }
  if (held) atomicAdd(&s_held, held);
  if (nout) atomicAdd(&s_out, nout);
  if (nin) atomicAdd(&s_in, nin);
  __syncthreads();
  if (threadIdx.x == 0) {
    int *cnt = reinterpret_cast<int *>(pose_out + 64);
    const bool refused = (cnt[6] & SPFE_POSE_STATUS_COV_OVERFLOW) != 0;
    cnt[7] = refused ? SPFE_TRACK_FAIL_COV : (s_in >= th_nmatch_opt ? SPFE_TRACK_OK : fail_verdict);
    cnt[8] = n_matches_src ? n_matches_src[0] : s_held;
    cnt[9] = s_in;
    cnt[(SPFE_POSE_OFF_N_OUTLIERS - 64) / 4] = s_out;
  }
}

size_t proj_resolve_lds_bytes(int kmax) { return (size_t)kmax * 9 + 16; }   // the dynamic part
// ... and what the workgroup allocates in all: kmax <= 18200 fits the 160 KB a workgroup can have
size_t proj_resolve_lds_total(int kmax) { return PJ_LDS_STATIC + proj_resolve_lds_bytes(kmax); }

hipError_t launch_proj_search(const ProjArgs &a0, hipStream_t s) {
  ProjArgs a = a0;
  if (a.nframes < 1) a.nframes = 1;
  if (a.cap < 1 || a.cap > SPFE_PROJ_MAX_POINTS || a.n < 0 || a.n > a.cap || a.kmax < 1) return hipErrorInvalidValue;
  const size_t lds = proj_resolve_lds_bytes(a.kmax);
  if (proj_resolve_lds_total(a.kmax) > PJ_LDS_MAX) return hipErrorInvalidValue;
  if (lds > 48 * 1024) {   // beyond the default dynamic-LDS limit: raise it
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(proj_resolve_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  if (a.mode == SPFE_PROJ_LOCAL_MAP) hipLaunchKernelGGL(proj_prepare_kernel, dim3(a.nframes), dim3(256), 0, s, a);
  hipLaunchKernelGGL(proj_candidates_kernel, dim3((a.cap + 3) / 4, a.nframes), dim3(256), 0, s, a);
  hipLaunchKernelGGL(proj_resolve_kernel, dim3(a.nframes), dim3(PJ_RES_THREADS), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_local_map_verdict(const int *hdr, int kmax, const int *mp_of_kp, const uint8_t *flags, int n,
                                    const uint8_t *proj_out, int th_ninlier, uint8_t *pose_out, hipStream_t s) {
  hipLaunchKernelGGL(local_map_verdict_kernel, dim3(1), dim3(256), 0, s, hdr, kmax, mp_of_kp, flags, n, proj_out,
                     th_ninlier, pose_out);
  return hipGetLastError();
}

hipError_t launch_track_discard(const int *hdr, int kmax, int *mp_of_kp, const uint8_t *flags, int n, const int *n_matches_src,
                                int th_nmatch_opt, int fail_verdict, uint8_t *pose_out, hipStream_t s) {
  hipLaunchKernelGGL(track_discard_kernel, dim3(1), dim3(256), 0, s, hdr, kmax, mp_of_kp, flags, n, n_matches_src,
                     th_nmatch_opt, fail_verdict, pose_out);
  return hipGetLastError();
}

}  // namespace spfe
