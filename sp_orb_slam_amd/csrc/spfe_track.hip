// spfe_track.hip — C ABI of the tracker's stages on records resident in HBM, and their host-array forms, on the handle's
// buffers and streams:
//   direct "dust" alignment               optimizer_dust.cpp:170-294, and its chain with the patch-wise association
//                                         (tracker_dust.cpp:92-172)
//   covariance-weighted pose refinement   optimizer_dust.cpp:35-167, optimizer.cpp:231-443, and the whole of
//                                         trackFrameDustKFLocal behind the extraction (tracker_dust.cpp:22-228)
//   window search by projection           sp_matcher.cpp:344-432, :1439-1543, and TrackLocalMap (tracker.cpp:561-615, :768-832)
//   the tracker's fallback steps          TrackWithMotionModel (tracker.cpp:480-559) and trackReferenceKeyFrameANN
//                                         (tracker.cpp:372-417, sp_matcher.cpp:1642-1674)
//   new map points of a keyframe          CreateNewMapPointsOverride (local_mapper.cpp:558-814) with SearchForTriByFlann
//                                         (sp_matcher.cpp:183-262)
//   the search of the mapper's fuse step  SPMatcher::Fuse (sp_matcher.cpp:965-1104) as SearchInNeighbors calls it
//                                         (local_mapper.cpp:816-904)
//   verification of loop candidates       LoopClosingVLAD::ComputeSim3 (loop_closer_vlad.cpp:345-449): SearchByBruteForce
//                                         (sp_matcher_loop.cpp:334-376) and the hypotheses of Sim3Solver (sim3_solver.cpp)
//   the guided match of a hypothesis      SPMatcher::SearchBySim3Override (sp_matcher_loop.cpp:7-220) as ComputeSim3 calls it
//                                         (loop_closer_vlad.cpp:418-432)
//   the loop's points into the keyframe   SPMatcher::SearchByProjectionLoop (sp_matcher_loop.cpp:222-332)
//   the Sim3 optimisation of a hypothesis Optimizer::OptimizeSim3 (optimizer.cpp:1062-1252) behind the guided match
//   the loop's fusion step                SPMatcher::Fuse with a Sim3 (sp_matcher.cpp:1106-1219) as SearchAndFuse calls it, and
//                                         the corrected poses of CorrectLoop (loop_closer_vlad.cpp:536-571, :608-618, :701-726)
#include <climits>
#include <cmath>

#include "spfe_host.h"
#include "../../include/spfe_proj_math.h"
#include "../../include/spfe_loopfuse_math.h"
using namespace spfe_host;

namespace {
// ---- dust alignment ------------------------------------------------------------------------------
int dust_check(spfe_handle h, int n, const spfe_dust_params *prm) {
  if (n < 0 || n > SPFE_DUST_MAX_POINTS) return fail(SPFE_EINVAL, "n_points %d not in [0, %d]", n, SPFE_DUST_MAX_POINTS);
  if (prm->max_iterations < 0 || prm->max_iterations > 1000) return fail(SPFE_EINVAL, "max_iterations %d", prm->max_iterations);
  if (!(prm->huber_delta > 0)) return fail(SPFE_EINVAL, "huber_delta must be positive");
  if (spfe::dust_lds_bytes(h->hc, h->wc) > 160 * 1024) return fail(SPFE_EINVAL, "dust map %dx%d too large for LDS", h->wc, h->hc);
  return SPFE_OK;
}
int dust_launch(spfe_handle h, const float *d_dust, const void *d_pts, int n, const void *d_T, const spfe_dust_params *prm,
                void *d_out, hipStream_t s, int nframes = 1, size_t dust_stride = 0, const void *d_n = nullptr) {
  uint8_t *out = reinterpret_cast<uint8_t *>(d_out);
  spfe::DustArgs a{};
  a.nframes = nframes; a.dust_stride = dust_stride; a.pts_stride = (size_t)SPFE_DUST_MAX_POINTS * 12; a.pose_stride = 64;
  a.out_stride = SPFE_DUST_OUT_BYTES; a.n_dev = reinterpret_cast<const int *>(d_n);
  a.dust = d_dust; a.hc = h->hc; a.wc = h->wc; a.pts = reinterpret_cast<const float *>(d_pts); a.n = n;
  a.Tcw_in = reinterpret_cast<const float *>(d_T);
  a.fx = prm->fx; a.fy = prm->fy; a.cx = prm->cx; a.cy = prm->cy;
  a.max_iterations = prm->max_iterations; a.delta = prm->huber_delta; a.inlier_chi2 = prm->inlier_chi2;
  a.Tcw_out = reinterpret_cast<float *>(out);
  a.counts = reinterpret_cast<int *>(out + 64);
  a.uv = reinterpret_cast<float *>(out + SPFE_DUST_OFF_UV);
  a.inlier = out + SPFE_DUST_OFF_INLIER;
  HIP_TRY(spfe::launch_dust_align(a, s));
  return SPFE_OK;
}

// ---- pose refinement -----------------------------------------------------------------------------
constexpr int kPoseMaxEdges = 10001;
size_t pose_out_bytes(int kmax) { return align_up((size_t)SPFE_POSE_OFF_OUTLIER + (size_t)kmax, 256); }
int pose_check(const spfe_pose_params *prm) {
  if (prm->schedule != SPFE_POSE_DUST_POST && prm->schedule != SPFE_POSE_OPTIMIZATION)
    return fail(SPFE_EINVAL, "pose schedule %d", prm->schedule);
  if (prm->iterations < 0 || prm->iterations > 1000) return fail(SPFE_EINVAL, "iterations %d", prm->iterations);
  return SPFE_OK;
}
// n_pts: the rows of d_pts, so that holders outside [0, n_pts) are no edges (the chains that take n); -1: not known
spfe::PoseArgs pose_args(spfe_handle h, const RecordView &rec, const void *d_mp_of_kp, const void *d_pts, const void *d_T,
                         const spfe_pose_params *prm, void *d_out, int n_pts = -1) {
  spfe::PoseArgs a{};
  a.kp_xy = rec.xy();
  a.cinv = rec.cinv();
  a.hdr = rec.hdr();
  a.mp_of_kp = reinterpret_cast<const int *>(d_mp_of_kp);
  a.pts = reinterpret_cast<const float *>(d_pts);
  a.n_pts = n_pts;
  a.Tcw_in = reinterpret_cast<const float *>(d_T);
  a.fx = prm->fx; a.fy = prm->fy; a.cx = prm->cx; a.cy = prm->cy;
  a.schedule = prm->schedule; a.iterations = prm->iterations;
  a.out = reinterpret_cast<unsigned char *>(d_out);
  a.kmax = h->kmax;
  a.nframes = 1;
  return a;
}

// ---- window search by projection -----------------------------------------------------------------
int proj_check(spfe_handle h, int n, int kmax, const spfe_proj_params *prm) {
  if (n < 0 || n > SPFE_PROJ_MAX_POINTS) return fail(SPFE_EINVAL, "n_points %d not in [0, %d]", n, SPFE_PROJ_MAX_POINTS);
  if (prm->mode != SPFE_PROJ_LOCAL_MAP && prm->mode != SPFE_PROJ_LAST_FRAME) return fail(SPFE_EINVAL, "projection mode %d", prm->mode);
  if (!(prm->th > 0.0f)) return fail(SPFE_EINVAL, "th must be positive");
  const float rmax = spfe_proj_max_radius(prm->mode, prm->th);
  if (!(rmax <= (float)SPFE_PROJ_MAX_RADIUS))
    return fail(SPFE_EINVAL, "th %g gives a window radius of %g px, beyond SPFE_PROJ_MAX_RADIUS = %d", prm->th, rmax, SPFE_PROJ_MAX_RADIUS);
  if (spfe::proj_resolve_lds_total(kmax) > 160 * 1024)
    return fail(SPFE_EINVAL, "%d keypoints are too many for the claim stage's LDS (at most %d)", kmax, SPFE_PROJ_MAX_KEYPOINTS);
  return SPFE_OK;
}
// candidate lists for `points` map points (all frames of the call)
int proj_scratch(spfe_handle h, size_t points) {
  int rc;
  if ((rc = reserve(h, h->pj_ck, points * SPFE_PROJ_MAX_CAND * 4)) || (rc = reserve(h, h->pj_cd, points * SPFE_PROJ_MAX_CAND * 4)) ||
      (rc = reserve(h, h->pj_cq, points * SPFE_PROJ_MAX_CAND * 4)) || (rc = reserve(h, h->pj_cn, points * 4)))
    return rc;
  return reserve(h, h->pj_held, points);
}
void proj_fill(spfe_handle h, spfe::ProjArgs &a, const spfe_proj_params *prm) {
  a.hc = h->hc; a.wc = h->wc;
  a.W = (float)h->W; a.H = (float)h->H;
  a.fx = prm->fx; a.fy = prm->fy; a.cx = prm->cx; a.cy = prm->cy;
  a.mode = prm->mode; a.th = prm->th; a.th_dist = prm->th_dist; a.view_cos_limit = prm->view_cos_limit;
  a.adaptive = prm->adaptive; a.c2 = prm->c2_thresh;
  a.cand_k = h->pj_ck.as<int>(); a.cand_d = h->pj_cd.as<float>(); a.cand_duv = h->pj_cq.as<float>();
  a.cand_n = h->pj_cn.as<int>(); a.held = h->pj_held.p;
}
spfe::ProjArgs proj_record_args(spfe_handle h, const RecordView &rec, const void *d_xyz, const void *d_normal, const void *d_desc,
                                const void *d_flags, void *d_mp_of_kp, const void *d_Tcw, const spfe_proj_params *prm,
                                void *d_out) {
  spfe::ProjArgs a{};
  proj_fill(h, a, prm);
  a.kp_xy = rec.xy();
  a.occ = rec.occ();
  a.kp_desc = rec.desc();
  a.kp_desc_bf16 = rec.desc_bf16();
  a.hdr = rec.hdr();
  a.kmax = h->kmax;
  a.xyz = reinterpret_cast<const float *>(d_xyz);
  a.normal = reinterpret_cast<const float *>(d_normal);
  a.desc = reinterpret_cast<const float *>(d_desc);
  a.flags = reinterpret_cast<const uint8_t *>(d_flags);
  a.mp_of_kp = reinterpret_cast<int *>(d_mp_of_kp);
  a.Tcw = reinterpret_cast<const float *>(d_Tcw);
  a.out = reinterpret_cast<uint8_t *>(d_out);
  a.nframes = 1;
  return a;
}
// ---- new map points between keyframes ----------------------------------------------------------
int tri_check(spfe_handle h, const spfe_tri_params *prm, int point_base) {
  if (point_base < 0) return fail(SPFE_EINVAL, "point_base %d", point_base);
  if (!(prm->fx1 > 0 && prm->fy1 > 0 && prm->fx2 > 0 && prm->fy2 > 0)) return fail(SPFE_EINVAL, "focal lengths must be positive");
  return SPFE_OK;
}
int tri_scratch(spfe_handle h) {
  int rc = match_scratch(h, 1, h->kmax);
  if (rc) return rc;
  if (!h->tri_next && (rc = dev_alloc(h, &h->tri_next, 1))) return rc;
  return SPFE_OK;
}
// one neighbour: begin, the 2-NN search between the free rows, gate + triangulation
int tri_neighbour(spfe_handle h, const void *d_record1, const void *d_record2, void *d_mp1, void *d_mp2, const void *d_Tcw1,
                  const void *d_Tcw2, const float *d_median, const spfe_tri_params *prm, int point_base, bool set_base,
                  void *d_out, hipStream_t s) {
  const RecordView r1(h, d_record1), r2(h, d_record2);
  spfe::TriArgs a{};
  a.hdr1 = r1.hdr(); a.hdr2 = r2.hdr();
  a.xy1 = r1.xy(); a.xy2 = r2.xy(); a.cinv1 = r1.cinv(); a.cinv2 = r2.cinv();
  a.kmax = h->kmax;
  a.mp1 = reinterpret_cast<int *>(d_mp1); a.mp2 = reinterpret_cast<int *>(d_mp2);
  a.Tcw1 = reinterpret_cast<const float *>(d_Tcw1); a.Tcw2 = reinterpret_cast<const float *>(d_Tcw2);
  a.median_depth = d_median;
  a.fx1 = prm->fx1; a.fy1 = prm->fy1; a.cx1 = prm->cx1; a.cy1 = prm->cy1;
  a.fx2 = prm->fx2; a.fy2 = prm->fy2; a.cx2 = prm->cx2; a.cy2 = prm->cy2;
  a.ratio = prm->ratio; a.epipole_r2 = prm->epipole_r2;
  a.chi2_line = prm->chi2_line; a.chi2_reproj = prm->chi2_reproj; a.cos_parallax_max = prm->cos_parallax_max;
  a.min_baseline_depth_ratio = prm->min_baseline_depth_ratio;
  a.point_base = point_base; a.set_base = set_base ? 1 : 0;
  a.next_id = h->tri_next;
  a.best1 = h->m_best_q.as<unsigned long long>(); a.best2 = h->m_best_t.as<unsigned long long>();
  a.out = reinterpret_cast<uint8_t *>(d_out);
  HIP_TRY(spfe::launch_tri_begin(a, s));
  // pKF1->flann->knnMatch(pKF2->mDescReamin, matches, 2): queries = the neighbour's free rows, train = the keyframe's
  spfe::MatchSide q = record_side(h, d_record2), t = record_side(h, d_record1);
  q.mask = a.mp2; q.mask_free = 1;
  t.mask = a.mp1; t.mask_free = 1;
  HIP_TRY(spfe::launch_match_knn2_free(q, t, h->m_best_q.as<unsigned long long>(), h->m_best_t.as<unsigned long long>(), s));
  HIP_TRY(spfe::launch_tri_gate_triangulate(a, s));
  return SPFE_OK;
}

// ---- the search of SPMatcher::Fuse --------------------------------------------------------------
int fuse_check(int n, int n_cap, const spfe_fuse_params *prm) {
  if (n_cap < 1 || n_cap > SPFE_PROJ_MAX_POINTS) return fail(SPFE_EINVAL, "n_cap %d not in [1, %d]", n_cap, SPFE_PROJ_MAX_POINTS);
  if (n < 0 || n > n_cap) return fail(SPFE_EINVAL, "n_points %d not in [0, n_cap = %d]", n, n_cap);
  if (!(prm->th > 0.0f && prm->th <= (float)SPFE_PROJ_MAX_RADIUS))
    return fail(SPFE_EINVAL, "th %g is not a window radius in (0, SPFE_PROJ_MAX_RADIUS = %d]", prm->th, SPFE_PROJ_MAX_RADIUS);
  return SPFE_OK;
}
void fuse_fill(spfe_handle h, spfe::FuseArgs &a, const spfe_fuse_params *prm) {
  a.hc = h->hc; a.wc = h->wc;
  a.W = (float)h->W; a.H = (float)h->H;
  a.fx = prm->fx; a.fy = prm->fy; a.cx = prm->cx; a.cy = prm->cy;
  a.th = prm->th; a.th_dist = prm->th_dist; a.chi2 = prm->chi2; a.view_cos = prm->view_cos;
  a.min_factor = prm->min_factor; a.max_factor = prm->max_factor;
}
using FuseLaunch = hipError_t (*)(const spfe::FuseArgs &, hipStream_t);
// the targets of `a` (set by the caller: records, or the host form's staged arrays) against one point list
int fuse_launch(spfe_handle h, spfe::FuseArgs &a, const void *d_kf_mp_of_kp, const void *d_Tcw, const void *d_point_id,
                const void *d_xyz, const void *d_normal, const void *d_dist_range, const void *d_desc, const void *d_flags, int n,
                int n_cap, const spfe_fuse_params *prm, void *d_out, hipStream_t s, FuseLaunch launch) {
  fuse_fill(h, a, prm);
  a.kf_mp_of_kp = reinterpret_cast<const int *>(d_kf_mp_of_kp);
  a.Tcw = reinterpret_cast<const float *>(d_Tcw);
  a.point_id = reinterpret_cast<const int *>(d_point_id);
  a.xyz = reinterpret_cast<const float *>(d_xyz);
  a.normal = reinterpret_cast<const float *>(d_normal);
  a.dist_range = reinterpret_cast<const float *>(d_dist_range);
  a.desc = reinterpret_cast<const float *>(d_desc);
  a.flags = reinterpret_cast<const uint8_t *>(d_flags);
  a.n = n; a.cap = n_cap;
  a.out = reinterpret_cast<uint8_t *>(d_out);
  HIP_TRY(launch(a, s));
  return SPFE_OK;
}
// n_targets records of the handle's layout against one point list
int fuse_records(spfe_handle h, const void *const *d_records, int n_targets, const void *d_kf_mp_of_kp, const void *d_Tcw,
                 const void *d_point_id, const void *d_xyz, const void *d_normal, const void *d_dist_range, const void *d_desc,
                 const void *d_flags, int n, int n_cap, const spfe_fuse_params *prm, void *d_out, hipStream_t s,
                 FuseLaunch launch = spfe::launch_fuse_search) {
  spfe::FuseArgs a{};
  for (int j = 0; j < n_targets; ++j) a.base[j] = reinterpret_cast<const uint8_t *>(d_records[j]);
  a.n_targets = n_targets;
  a.off_xy = (long)h->rl.off_xy; a.off_occ = (long)h->rl.off_occ; a.off_desc = (long)h->rl.off_desc; a.off_hdr = (long)h->rl.off_hdr;
  a.kp_desc_bf16 = h->rl.desc_bf16;
  a.kmax = h->kmax;
  return fuse_launch(h, a, d_kf_mp_of_kp, d_Tcw, d_point_id, d_xyz, d_normal, d_dist_range, d_desc, d_flags, n, n_cap, prm, d_out, s,
                     launch);
}
// the loop's fuse search on the same arguments: no chi-square gate (FuseArgs::chi2 is not read), d_Tcw holds the similarities
spfe_fuse_params loop_fuse_params(const spfe_loop_fuse_params *p) {
  spfe_fuse_params f{};
  f.fx = p->fx; f.fy = p->fy; f.cx = p->cx; f.cy = p->cy;
  f.th = p->th; f.th_dist = p->th_dist; f.chi2 = 0.0; f.view_cos = p->view_cos;
  f.min_factor = p->min_factor; f.max_factor = p->max_factor;
  return f;
}
bool fuse_null_points(int n, const void *id, const void *xyz, const void *normal, const void *range, const void *desc,
                      const void *flags) {
  return n > 0 && (!id || !xyz || !normal || !range || !desc || !flags);
}

// ---- the guided match of a Sim3 hypothesis ---------------------------------------------------------
int guided_check(int n, const spfe_guided_params *prm) {
  if (n < 0 || n > SPFE_PROJ_MAX_POINTS) return fail(SPFE_EINVAL, "n_points %d not in [0, %d]", n, SPFE_PROJ_MAX_POINTS);
  if (!(prm->th > 0.0f && prm->th <= (float)SPFE_PROJ_MAX_RADIUS))
    return fail(SPFE_EINVAL, "th %g is not a window radius in (0, SPFE_PROJ_MAX_RADIUS = %d]", prm->th, SPFE_PROJ_MAX_RADIUS);
  return SPFE_OK;
}
void guided_fill(spfe_handle h, spfe::GuidedArgs &a, const spfe_guided_params *prm) {
  a.hc = h->hc; a.wc = h->wc;
  a.W = (float)h->W; a.H = (float)h->H;
  a.fx1 = prm->fx1; a.fy1 = prm->fy1; a.cx1 = prm->cx1; a.cy1 = prm->cy1;
  a.fx2 = prm->fx2; a.fy2 = prm->fy2; a.cx2 = prm->cx2; a.cy2 = prm->cy2;
  a.th = prm->th; a.th_dist = prm->th_dist; a.min_factor = prm->min_factor; a.max_factor = prm->max_factor;
}
// the map, the poses and the output block, common to all three forms
void guided_map(spfe::GuidedArgs &a, const void *d_kf1_mp_of_kp, const void *d_kf2_mp_of_kp, const void *d_xyz, const void *d_flags,
                const void *d_dist_range, const void *d_desc, int n, const void *d_Tcw1, const void *d_Tcw2, void *d_out) {
  a.mp1 = reinterpret_cast<const int *>(d_kf1_mp_of_kp); a.mp2 = reinterpret_cast<const int *>(d_kf2_mp_of_kp);
  a.xyz = reinterpret_cast<const float *>(d_xyz); a.flags = reinterpret_cast<const uint8_t *>(d_flags);
  a.dist_range = reinterpret_cast<const float *>(d_dist_range); a.desc = reinterpret_cast<const float *>(d_desc); a.n = n;
  a.Tcw1 = reinterpret_cast<const float *>(d_Tcw1); a.Tcw2 = reinterpret_cast<const float *>(d_Tcw2);
  a.out = reinterpret_cast<uint8_t *>(d_out);
}
// ... and the records of the handle's layout, common to the two device forms
void guided_records(spfe_handle h, spfe::GuidedArgs &a, const void *d_record1, const void *d_kf1_mp_of_kp,
                    const void *d_kf2_mp_of_kp, const void *d_xyz, const void *d_flags, const void *d_dist_range, const void *d_desc,
                    int n, const void *d_Tcw1, const void *d_Tcw2, void *d_out) {
  a.base1 = reinterpret_cast<const uint8_t *>(d_record1);
  a.off_xy = (long)h->rl.off_xy; a.off_occ = (long)h->rl.off_occ; a.off_desc = (long)h->rl.off_desc; a.off_hdr = (long)h->rl.off_hdr;
  a.kp_desc_bf16 = h->rl.desc_bf16;
  a.kmax = h->kmax;
  guided_map(a, d_kf1_mp_of_kp, d_kf2_mp_of_kp, d_xyz, d_flags, d_dist_range, d_desc, n, d_Tcw1, d_Tcw2, d_out);
}
bool guided_null_map(int n, const void *xyz, const void *flags, const void *range, const void *desc) {
  return n > 0 && (!xyz || !flags || !range || !desc);
}

// ---- the Sim3 optimisation of a hypothesis -----------------------------------------------------------
int sim3opt_check(int n, int kmax, const spfe_sim3opt_params *prm) {
  if (n < 0 || n > SPFE_PROJ_MAX_POINTS) return fail(SPFE_EINVAL, "n_points %d not in [0, %d]", n, SPFE_PROJ_MAX_POINTS);
  if (prm->iterations < 1 || prm->iterations > 1000) return fail(SPFE_EINVAL, "iterations %d not in [1, 1000]", prm->iterations);
  if (spfe::sim3opt_lds_edge_capacity(kmax) < 0) return fail(SPFE_EINVAL, "%d keypoints are too many for the solve's LDS", kmax);
  return SPFE_OK;
}
void sim3opt_fill(spfe::Sim3OptArgs &a, const spfe_sim3opt_params *prm) {
  a.fx1 = prm->fx1; a.fy1 = prm->fy1; a.cx1 = prm->cx1; a.cy1 = prm->cy1;
  a.fx2 = prm->fx2; a.fy2 = prm->fy2; a.cx2 = prm->cx2; a.cy2 = prm->cy2;
  a.th2 = prm->th2; a.fix_scale = prm->fix_scale; a.iterations = prm->iterations; a.min_kept = prm->min_kept;
  a.min_inliers = prm->min_inliers;
}
// the map, the poses and the output block, common to all three forms
void sim3opt_map(spfe::Sim3OptArgs &a, const void *d_kf1_mp_of_kp, const void *d_kf2_mp_of_kp, const void *d_xyz, const void *d_flags,
                 int n, const void *d_Tcw1, const void *d_Tcw2, void *d_out) {
  a.mp1 = reinterpret_cast<const int *>(d_kf1_mp_of_kp); a.mp2 = reinterpret_cast<const int *>(d_kf2_mp_of_kp);
  a.xyz = reinterpret_cast<const float *>(d_xyz); a.flags = reinterpret_cast<const uint8_t *>(d_flags); a.n = n;
  a.Tcw1 = reinterpret_cast<const float *>(d_Tcw1); a.Tcw2 = reinterpret_cast<const float *>(d_Tcw2);
  a.out = reinterpret_cast<uint8_t *>(d_out);
}
// ... and the records of the handle's layout, common to the two device forms
void sim3opt_records(spfe_handle h, spfe::Sim3OptArgs &a, const void *d_record1, const void *d_kf1_mp_of_kp,
                     const void *d_kf2_mp_of_kp, const void *d_xyz, const void *d_flags, int n, const void *d_Tcw1,
                     const void *d_Tcw2, void *d_out) {
  a.base1 = reinterpret_cast<const uint8_t *>(d_record1);
  a.off_xy = (long)h->rl.off_xy; a.off_hdr = (long)h->rl.off_hdr;
  a.kmax = h->kmax;
  sim3opt_map(a, d_kf1_mp_of_kp, d_kf2_mp_of_kp, d_xyz, d_flags, n, d_Tcw1, d_Tcw2, d_out);
}

// ---- the loop's map points projected into the current keyframe ---------------------------------------
int loop_proj_check(int n, int n_cap, int kmax, const spfe_loop_proj_params *prm) {
  if (n_cap < 1 || n_cap > SPFE_PROJ_MAX_POINTS) return fail(SPFE_EINVAL, "n_cap %d not in [1, %d]", n_cap, SPFE_PROJ_MAX_POINTS);
  if (n < 0 || n > n_cap) return fail(SPFE_EINVAL, "n_points %d not in [0, n_cap = %d]", n, n_cap);
  if (!(prm->th > 0.0f && prm->th <= (float)SPFE_PROJ_MAX_RADIUS))
    return fail(SPFE_EINVAL, "th %g is not a window radius in (0, SPFE_PROJ_MAX_RADIUS = %d]", prm->th, SPFE_PROJ_MAX_RADIUS);
  if (spfe::loop_proj_lds_total(kmax) > 160 * 1024)
    return fail(SPFE_EINVAL, "%d keypoints are too many for the claim stage's LDS (at most %d)", kmax, SPFE_LOOPPROJ_MAX_KEYPOINTS);
  return SPFE_OK;
}
void loop_proj_fill(spfe_handle h, spfe::LoopProjArgs &a, const spfe_loop_proj_params *prm) {
  a.hc = h->hc; a.wc = h->wc;
  a.W = (float)h->W; a.H = (float)h->H;
  a.fx = prm->fx; a.fy = prm->fy; a.cx = prm->cx; a.cy = prm->cy;
  a.th = prm->th; a.th_dist = prm->th_dist; a.view_cos = prm->view_cos;
  a.min_factor = prm->min_factor; a.max_factor = prm->max_factor;
  a.cand_k = h->pj_ck.as<int>(); a.cand_d = h->pj_cd.as<float>(); a.cand_n = h->pj_cn.as<int>();
}

// ---- verification of loop candidates -------------------------------------------------------------
int sim3_check(int n, int n_hyp, const spfe_sim3_params *prm) {
  if (n < 0 || n > SPFE_PROJ_MAX_POINTS) return fail(SPFE_EINVAL, "n_points %d not in [0, %d]", n, SPFE_PROJ_MAX_POINTS);
  if (n_hyp < 1 || n_hyp > SPFE_SIM3_MAX_HYPOTHESES)
    return fail(SPFE_EINVAL, "n_hyp %d not in [1, %d]", n_hyp, SPFE_SIM3_MAX_HYPOTHESES);
  if (prm->min_inliers < 0) return fail(SPFE_EINVAL, "min_inliers %d", prm->min_inliers);
  return SPFE_OK;
}
void sim3_fill(spfe::Sim3Args &a, const spfe_sim3_params *prm) {
  a.fx1 = prm->fx1; a.fy1 = prm->fy1; a.cx1 = prm->cx1; a.cy1 = prm->cy1;
  a.fx2 = prm->fx2; a.fy2 = prm->fy2; a.cx2 = prm->cx2; a.cy2 = prm->cy2;
  a.max_err1 = prm->max_err1; a.max_err2 = prm->max_err2;
  a.min_inliers = prm->min_inliers; a.fix_scale = prm->fix_scale ? 1 : 0;
}
int sim3_scratch(spfe_handle h, int n_cand, int kcap) { return reserve(h, h->s3_scratch, (size_t)n_cand * kcap * 40); }
int loop_match_scratch(spfe_handle h) {
  int rc = match_scratch(h, 1, h->kmax);
  return rc ? rc : reserve(h, h->m_out, (size_t)h->kmax * 8);
}
// SearchByBruteForce(mpCurrentKF, pKF, vvpMapPointMatches[i]): train = the current keyframe's held rows, queries = the
// candidate's (sp_matcher_loop.cpp:348-368), then vpMatches12[train] = the query's point (:370-373) as its keypoint
int loop_match(spfe_handle h, const void *d_record1, const void *d_record2, const void *d_mp1, const void *d_mp2, void *d_match12,
               void *d_n_matches, hipStream_t s) {
  spfe::MatchSide q = record_side(h, d_record2), t = record_side(h, d_record1);
  q.mask = reinterpret_cast<const int *>(d_mp2); q.mask_n = INT_MAX;
  t.mask = reinterpret_cast<const int *>(d_mp1); t.mask_n = INT_MAX;
  HIP_TRY(spfe::launch_match(q, t, 1, true, h->m_best_t.as<unsigned long long>(), h->m_best_q.as<unsigned long long>(),
                             h->m_out.p, 0, s));
  HIP_TRY(spfe::launch_loop_match_invert(h->m_out.as<int32_t>(), RecordView(h, d_record2).hdr(), h->kmax,
                                         reinterpret_cast<int *>(d_match12), reinterpret_cast<int *>(d_n_matches), s));
  return SPFE_OK;
}

bool proj_null_points(int n, int mode, const void *xyz, const void *normal, const void *desc, const void *flags) {
  return n > 0 && (!xyz || !desc || !flags || (mode == SPFE_PROJ_LOCAL_MAP && !normal));
}
}  // namespace

extern "C" {

// ---- direct "dust" alignment (optimizer_dust.cpp:170-294) -----------------
int spfe_align_dust_record_device(spfe_handle h, const void *d_record, const void *d_points_xyz, int n,
                                  const void *d_Tcw, const spfe_dust_params *prm, void *d_out, void *stream) {
  if (!h || !d_record || !d_Tcw || !prm || !d_out || (n > 0 && !d_points_xyz)) return fail(SPFE_EINVAL, "null argument");
  int rc = dust_check(h, n, prm);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  return dust_launch(h, RecordView(h, d_record).dense_dust(), d_points_xyz, n, d_Tcw, prm, d_out, stream_of(h, stream));
}

int spfe_align_dust_batch_device(spfe_handle h, const void *d_records, int n_frames, const void *d_points_xyz,
                                 const void *d_n_points, const void *d_Tcw, const spfe_dust_params *prm, void *d_out,
                                 void *stream) {
  if (!h || !d_records || !d_Tcw || !prm || !d_out || !d_points_xyz || !d_n_points) return fail(SPFE_EINVAL, "null argument");
  if (n_frames < 1 || n_frames > 65535) return fail(SPFE_EINVAL, "n_frames %d", n_frames);
  int rc = dust_check(h, 0, prm);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  return dust_launch(h, RecordView(h, d_records).dense_dust(), d_points_xyz, 0, d_Tcw, prm, d_out, stream_of(h, stream), n_frames,
                     h->rl.bytes, d_n_points);
}

int spfe_align_dust(spfe_handle h, const float *dense_dust, const float *points_xyz, int n, const float *Tcw,
                    const spfe_dust_params *prm, float *Tcw_out, uint8_t *inlier, float *proj_uv, int *n_inlier,
                    int *iterations) {
  if (!h || !dense_dust || !Tcw || !prm || !Tcw_out || (n > 0 && !points_xyz)) return fail(SPFE_EINVAL, "null argument");
  int rc = dust_check(h, n, prm);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  HostStage st(h);
  const int b_map = st.in(dense_dust, (size_t)h->C * 4, (size_t)h->C * 4, 4),
            b_pts = st.in(points_xyz, (size_t)n * 12, (size_t)SPFE_DUST_MAX_POINTS * 12, 4), b_T = st.in(Tcw, 64, 64, 4),
            b_out = st.out(SPFE_DUST_OUT_BYTES, nullptr, 4);
  if ((rc = st.commit())) return rc;
  rc = dust_launch(h, st.dev<float>(b_map), st.dev<void>(b_pts), n, st.dev<void>(b_T), prm, st.dev<void>(b_out), h->stream);
  if (rc) return rc;
  st.fetch(b_out, SPFE_DUST_OUT_BYTES);
  if ((rc = st.sync())) return rc;
  const uint8_t *o = st.host<uint8_t>(b_out);
  memcpy(Tcw_out, o, 64);
  const int *cnt = reinterpret_cast<const int *>(o + 64);
  if (n_inlier) *n_inlier = cnt[0];
  if (iterations) *iterations = cnt[1];
  if (proj_uv && n > 0) memcpy(proj_uv, o + SPFE_DUST_OFF_UV, (size_t)n * 8);
  if (inlier && n > 0) memcpy(inlier, o + SPFE_DUST_OFF_INLIER, (size_t)n);
  return SPFE_OK;
}

int spfe_track_dust_record_device(spfe_handle h, const void *d_record, const void *d_points_xyz, const void *d_mp_desc, int n,
                                  const void *d_Tcw, const spfe_dust_params *prm, int min_inliers, float max_dist,
                                  void *d_dust_out, void *d_kp_idx, void *stream) {
  if (!h || !d_record || !d_Tcw || !prm || !d_dust_out || !d_kp_idx || (n > 0 && (!d_points_xyz || !d_mp_desc)))
    return fail(SPFE_EINVAL, "null argument");
  int rc = dust_check(h, n, prm);
  if (rc || (rc = patch_check(h->kmax))) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = patch_scratch(h))) return rc;
  hipStream_t s = stream_of(h, stream);
  const RecordView rec(h, d_record);
  const uint8_t *dout = reinterpret_cast<const uint8_t *>(d_dust_out);
  // PoseOptimizationDust(&mCurrentFrame, mps_for_track, is_visible)   tracker_dust.cpp:92-94
  rc = dust_launch(h, rec.dense_dust(), d_points_xyz, n, d_Tcw, prm, d_dust_out, s);
  if (rc || n == 0) return rc;
  // the patch-wise association of the in_view points at their dust_proj_u / v   :113-172, on the same stream: the
  // projections, the flags and n_inlier are read where the alignment left them
  spfe::PatchArgs a = patch_args(h, rec, d_mp_desc, dout + SPFE_DUST_OFF_UV, n);
  a.in_view = dout + SPFE_DUST_OFF_INLIER;
  a.gate_ptr = reinterpret_cast<const int *>(dout + 64);
  a.gate_min = min_inliers;
  HIP_TRY(spfe::launch_match_patches(a, h->kmax, max_dist, h->p_cidx, h->p_cdist, reinterpret_cast<int32_t *>(d_kp_idx), s));
  return SPFE_OK;
}

// ---- covariance-weighted pose refinement (optimizer_dust.cpp:35-167, optimizer.cpp:231-443) -------------------------
size_t spfe_pose_out_bytes(spfe_handle h) { return h ? pose_out_bytes(h->kmax) : 0; }

int spfe_pose_lds_edge_capacity(spfe_handle h) { return h ? spfe::pose_lds_edge_capacity(h->kmax) : -1; }

int spfe_refine_pose(spfe_handle h, const float *obs_xy, const float *inv_sigma2, const float *points_xyz, int n,
                     const float *Tcw, const spfe_pose_params *prm, float *Tcw_out, uint8_t *outlier, int *iterations,
                     int *n_good) {
  if (!h || !Tcw || !prm || !Tcw_out || (n > 0 && (!obs_xy || !inv_sigma2 || !points_xyz))) return fail(SPFE_EINVAL, "null argument");
  if (n < 0 || n > kPoseMaxEdges) return fail(SPFE_EINVAL, "n %d not in [0, %d]", n, kPoseMaxEdges);
  int rc = pose_check(prm);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t ne = (size_t)std::max(n, 1), out_b = pose_out_bytes((int)ne);
  HostStage st(h);
  const int b_obs = st.in(obs_xy, (size_t)n * 8, ne * 8, 4), b_inf = st.in(inv_sigma2, (size_t)n * 8, ne * 8, 4),
            b_pts = st.in(points_xyz, (size_t)n * 12, ne * 12, 4), b_T = st.in(Tcw, 64, 64, 4), b_out = st.out(out_b);
  if ((rc = st.commit())) return rc;
  spfe::PoseArgs a{};
  a.kp_xy = st.dev<float>(b_obs);
  a.cinv = st.dev<float>(b_inf);
  a.pts = st.dev<float>(b_pts);
  a.Tcw_in = st.dev<float>(b_T);
  a.k_imm = n;
  a.n_pts = -1;
  a.fx = prm->fx; a.fy = prm->fy; a.cx = prm->cx; a.cy = prm->cy;
  a.schedule = prm->schedule; a.iterations = prm->iterations;
  a.out = st.dev<uint8_t>(b_out);
  a.kmax = (int)ne;
  a.nframes = 1;
  HIP_TRY(spfe::launch_pose_refine(a, h->stream));
  st.fetch(b_out, out_b);
  if ((rc = st.sync())) return rc;
  const uint8_t *o = st.host<uint8_t>(b_out);
  memcpy(Tcw_out, o, 64);
  const int *cnt = reinterpret_cast<const int *>(o + 64);
  if (n_good) *n_good = cnt[1];
  if (iterations) memcpy(iterations, cnt + 2, 16);
  if (outlier && n > 0) memcpy(outlier, o + SPFE_POSE_OFF_OUTLIER, (size_t)n);
  return SPFE_OK;
}

int spfe_refine_pose_record_device(spfe_handle h, const void *d_record, const void *d_mp_of_kp, const void *d_points_xyz,
                                   const void *d_Tcw, const spfe_pose_params *prm, void *d_out, void *stream) {
  if (!h || !d_record || !d_mp_of_kp || !d_points_xyz || !d_Tcw || !prm || !d_out) return fail(SPFE_EINVAL, "null argument");
  int rc = pose_check(prm);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  const spfe::PoseArgs a = pose_args(h, RecordView(h, d_record), d_mp_of_kp, d_points_xyz, d_Tcw, prm, d_out);
  HIP_TRY(spfe::launch_pose_refine(a, stream_of(h, stream)));
  return SPFE_OK;
}

int spfe_refine_pose_batch_device(spfe_handle h, const void *d_records, int n_frames, const void *d_mp_of_kp,
                                  const void *d_points_xyz, size_t points_stride, const void *d_Tcw,
                                  const spfe_pose_params *prm, void *d_out, void *stream) {
  if (!h || !d_records || !d_mp_of_kp || !d_points_xyz || !d_Tcw || !prm || !d_out) return fail(SPFE_EINVAL, "null argument");
  if (n_frames < 1 || n_frames > 65535) return fail(SPFE_EINVAL, "n_frames %d", n_frames);
  int rc = pose_check(prm);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  spfe::PoseArgs a = pose_args(h, RecordView(h, d_records), d_mp_of_kp, d_points_xyz, d_Tcw, prm, d_out);
  a.nframes = n_frames;
  a.rec_stride = h->rl.bytes;
  a.map_stride = (size_t)h->kmax * 4;
  a.pts_stride = points_stride * 4;
  a.pose_stride = 64;
  a.out_stride = pose_out_bytes(h->kmax);
  HIP_TRY(spfe::launch_pose_refine(a, stream_of(h, stream)));
  return SPFE_OK;
}

int spfe_track_dust_refine_record_device(spfe_handle h, const void *d_record, const void *d_points_xyz, const void *d_mp_desc,
                                         int n, const void *d_Tcw, const spfe_dust_params *dust_prm,
                                         const spfe_pose_params *pose_prm, int th_ninlier, int th_nmatch, float th_ratio,
                                         float max_dist, void *d_dust_out, void *d_kp_idx, void *d_pose_out, void *stream) {
  if (!h || !d_record || !d_Tcw || !dust_prm || !pose_prm || !d_dust_out || !d_kp_idx || !d_pose_out ||
      (n > 0 && (!d_points_xyz || !d_mp_desc)))
    return fail(SPFE_EINVAL, "null argument");
  if (pose_prm->schedule != SPFE_POSE_DUST_POST) return fail(SPFE_EINVAL, "the chained form runs SPFE_POSE_DUST_POST");
  int rc = pose_check(pose_prm);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  if (!h->pose_map && (rc = dev_alloc(h, &h->pose_map, (size_t)h->kmax))) return rc;
  hipStream_t s = stream_of(h, stream);
  // alignment, th_ninlier gate, association   tracker_dust.cpp:92-172
  rc = spfe_track_dust_record_device(h, d_record, d_points_xyz, d_mp_desc, n, d_Tcw, dust_prm, th_ninlier, max_dist,
                                     d_dust_out, d_kp_idx, s);
  if (rc) return rc;
  // mCurrentFrame.mvpMapPoints[best_idx] = mp: the associations in keypoint order
  HIP_TRY(spfe::launch_fill_u32(h->pose_map, 0xffffffffu, (size_t)h->kmax, s));
  if (n > 0) HIP_TRY(spfe::launch_pose_scatter(reinterpret_cast<const int *>(d_kp_idx), n, h->pose_map, h->kmax, s));
  // th_nmatch gate, PoseOptimizationDustPost from the aligned pose, the ratio test   :174-227
  spfe::PoseArgs a = pose_args(h, RecordView(h, d_record), h->pose_map, n > 0 ? d_points_xyz : d_Tcw, d_dust_out, pose_prm,
                               d_pose_out);
  a.Tcw_echo = reinterpret_cast<const float *>(d_Tcw);
  a.gate_inliers = reinterpret_cast<const int *>(reinterpret_cast<const uint8_t *>(d_dust_out) + 64);
  a.th_ninlier = th_ninlier; a.th_nmatch = th_nmatch; a.th_ratio = th_ratio;
  HIP_TRY(spfe::launch_pose_refine(a, s));
  return SPFE_OK;
}

// ---- window search by projection and TrackLocalMap (sp_matcher.cpp:344-432, :1439-1543; tracker.cpp:561-615, :768-832) ----
size_t spfe_proj_out_bytes(spfe_handle h) { return h ? (size_t)SPFE_PROJ_OUT_BYTES : 0; }

int spfe_search_projection_record_device(spfe_handle h, const void *d_record, const void *d_xyz, const void *d_normal,
                                         const void *d_desc, const void *d_flags, int n, void *d_mp_of_kp, const void *d_Tcw,
                                         const spfe_proj_params *prm, void *d_out, void *stream) {
  if (!h || !d_record || !d_mp_of_kp || !d_Tcw || !prm || !d_out) return fail(SPFE_EINVAL, "null argument");
  int rc = proj_check(h, n, h->kmax, prm);
  if (rc) return rc;
  if (proj_null_points(n, prm->mode, d_xyz, d_normal, d_desc, d_flags)) return fail(SPFE_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = proj_scratch(h, (size_t)std::max(n, 1)))) return rc;
  spfe::ProjArgs a = proj_record_args(h, RecordView(h, d_record), d_xyz, d_normal, d_desc, d_flags, d_mp_of_kp, d_Tcw, prm, d_out);
  a.n = n;
  a.cap = std::max(n, 1);
  HIP_TRY(spfe::launch_proj_search(a, stream_of(h, stream)));
  return SPFE_OK;
}

int spfe_search_projection_batch_device(spfe_handle h, const void *d_records, int n_frames, const void *d_xyz,
                                        const void *d_normal, const void *d_desc, const void *d_flags, const void *d_n_points,
                                        size_t points_stride, void *d_mp_of_kp, const void *d_Tcw, const spfe_proj_params *prm,
                                        void *d_out, void *stream) {
  if (!h || !d_records || !d_mp_of_kp || !d_Tcw || !prm || !d_out || !d_n_points) return fail(SPFE_EINVAL, "null argument");
  if (n_frames < 1 || n_frames > 65535) return fail(SPFE_EINVAL, "n_frames %d", n_frames);
  if (points_stride < 1 || points_stride > SPFE_PROJ_MAX_POINTS)
    return fail(SPFE_EINVAL, "points_stride %zu not in [1, %d]", points_stride, SPFE_PROJ_MAX_POINTS);
  int rc = proj_check(h, (int)points_stride, h->kmax, prm);
  if (rc) return rc;
  if (proj_null_points(1, prm->mode, d_xyz, d_normal, d_desc, d_flags)) return fail(SPFE_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = proj_scratch(h, (size_t)n_frames * points_stride))) return rc;
  spfe::ProjArgs a = proj_record_args(h, RecordView(h, d_records), d_xyz, d_normal, d_desc, d_flags, d_mp_of_kp, d_Tcw, prm, d_out);
  a.n = 0;
  a.n_dev = reinterpret_cast<const int *>(d_n_points);
  a.cap = (int)points_stride;
  a.nframes = n_frames;
  a.rec_stride = h->rl.bytes;
  a.xyz_stride = points_stride * 12;
  a.desc_stride = points_stride * 1024;
  a.flags_stride = points_stride;
  a.map_stride = (size_t)h->kmax * 4;
  a.pose_stride = 64;
  a.out_stride = SPFE_PROJ_OUT_BYTES;
  HIP_TRY(spfe::launch_proj_search(a, stream_of(h, stream)));
  return SPFE_OK;
}

int spfe_search_projection(spfe_handle h, const float *kp_xy, const int16_t *occ_grid, const float *kp_desc, int K,
                           const float *xyz, const float *normal, const float *desc, const uint8_t *flags, int n,
                           int32_t *mp_of_kp, const float *Tcw, const spfe_proj_params *prm, int32_t *kp_of_mp,
                           uint8_t *in_view, float *proj_uv, float *view_cos, int *n_matches, int *n_to_match) {
  if (!h || !occ_grid || !Tcw || !prm) return fail(SPFE_EINVAL, "null argument");
  if (K < 0 || K > 32767) return fail(SPFE_EINVAL, "n_keypoints %d out of range", K);
  if (K > 0 && (!kp_xy || !kp_desc || !mp_of_kp)) return fail(SPFE_EINVAL, "null argument");
  const int kcap = std::max(K, 1);
  int rc = proj_check(h, n, kcap, prm);
  if (rc) return rc;
  if (proj_null_points(n, prm->mode, xyz, normal, desc, flags)) return fail(SPFE_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(h->cfg.device));
  const int ncap = std::max(n, 1);
  if ((rc = proj_scratch(h, (size_t)ncap))) return rc;
  const size_t cells = (size_t)h->hc * h->wc;
  const size_t kc = (size_t)kcap, nc = (size_t)ncap;
  HostStage st(h);
  const int b_xy = st.in(kp_xy, (size_t)K * 8, kc * 8, 16), b_occ = st.in(occ_grid, cells * 2, cells * 2, 16),
            b_kd = st.in(kp_desc, (size_t)K * 1024, kc * 1024, 16), b_p = st.in(xyz, (size_t)n * 12, nc * 12, 4),
            b_n = st.in(normal, (size_t)n * 12, nc * 12, 4), b_d = st.in(desc, (size_t)n * 1024, nc * 1024, 16),
            b_f = st.in(flags, (size_t)n, nc, 1), b_map = st.in(mp_of_kp, (size_t)K * 4, kc * 4, 16), b_T = st.in(Tcw, 64, 64, 4),
            b_out = st.out(SPFE_PROJ_OUT_BYTES);
  if ((rc = st.commit())) return rc;
  spfe::ProjArgs a{};
  proj_fill(h, a, prm);
  a.kp_xy = st.dev<float>(b_xy);
  a.occ = st.dev<int16_t>(b_occ);
  a.kp_desc = st.dev<float>(b_kd);
  a.k_imm = K;
  a.kmax = kcap;
  a.xyz = st.dev<float>(b_p);
  a.normal = st.dev<float>(b_n);
  a.desc = st.dev<float>(b_d);
  a.flags = st.dev<uint8_t>(b_f);
  a.n = n;
  a.cap = ncap;
  a.mp_of_kp = st.dev<int>(b_map);
  a.Tcw = st.dev<float>(b_T);
  a.out = st.dev<uint8_t>(b_out);
  a.nframes = 1;
  HIP_TRY(spfe::launch_proj_search(a, h->stream));
  st.fetch(b_out, SPFE_PROJ_OUT_BYTES);
  if ((rc = st.fetch_to(mp_of_kp, a.mp_of_kp, (size_t)K * 4)) || (rc = st.sync())) return rc;
  const uint8_t *o = st.host<uint8_t>(b_out);
  const int *cnt = reinterpret_cast<const int *>(o);
  if (n_matches) *n_matches = cnt[0];
  if (n_to_match) *n_to_match = cnt[1];
  if (n > 0) {
    if (kp_of_mp) memcpy(kp_of_mp, o + SPFE_PROJ_OFF_KP, (size_t)n * 4);
    if (proj_uv) memcpy(proj_uv, o + SPFE_PROJ_OFF_UV, (size_t)n * 8);
    if (view_cos) memcpy(view_cos, o + SPFE_PROJ_OFF_COS, (size_t)n * 4);
    if (in_view) memcpy(in_view, o + SPFE_PROJ_OFF_VIEW, (size_t)n);
  }
  return SPFE_OK;
}

int spfe_track_local_map_record_device(spfe_handle h, const void *d_record, const void *d_xyz, const void *d_normal,
                                       const void *d_desc, const void *d_flags, int n, void *d_mp_of_kp, const void *d_Tcw,
                                       const spfe_proj_params *proj_prm, const spfe_pose_params *pose_prm, int th_ninlier,
                                       void *d_proj_out, void *d_pose_out, void *stream) {
  if (!h || !d_record || !d_mp_of_kp || !d_Tcw || !proj_prm || !pose_prm || !d_proj_out || !d_pose_out)
    return fail(SPFE_EINVAL, "null argument");
  if (proj_prm->mode != SPFE_PROJ_LOCAL_MAP) return fail(SPFE_EINVAL, "the chained form searches in SPFE_PROJ_LOCAL_MAP mode");
  if (pose_prm->schedule != SPFE_POSE_OPTIMIZATION) return fail(SPFE_EINVAL, "the chained form runs SPFE_POSE_OPTIMIZATION");
  int rc = pose_check(pose_prm);
  if (rc) return rc;
  if ((rc = proj_check(h, n, h->kmax, proj_prm))) return rc;
  if (proj_null_points(n, proj_prm->mode, d_xyz, d_normal, d_desc, d_flags)) return fail(SPFE_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = proj_scratch(h, (size_t)std::max(n, 1)))) return rc;
  hipStream_t s = stream_of(h, stream);
  const RecordView rec(h, d_record);
  // SearchLocalPoints   tracker.cpp:569, :768-832
  spfe::ProjArgs a = proj_record_args(h, rec, d_xyz, d_normal, d_desc, d_flags, d_mp_of_kp, d_Tcw, proj_prm, d_proj_out);
  a.n = n;
  a.cap = std::max(n, 1);
  a.refuse_overflow = 1;
  HIP_TRY(spfe::launch_proj_search(a, s));
  // Optimizer::PoseOptimization(&mCurrentFrame) over the updated associations   :572
  const spfe::PoseArgs p = pose_args(h, rec, d_mp_of_kp, n > 0 ? d_xyz : d_Tcw, d_Tcw, pose_prm, d_pose_out, n);
  HIP_TRY(spfe::launch_pose_refine(p, s));
  // mnMatchesInliers and the verdict   :576-612
  HIP_TRY(spfe::launch_local_map_verdict(rec.hdr(), h->kmax, reinterpret_cast<const int *>(d_mp_of_kp),
                                         reinterpret_cast<const uint8_t *>(d_flags), n,
                                         reinterpret_cast<const uint8_t *>(d_proj_out), th_ninlier,
                                         reinterpret_cast<uint8_t *>(d_pose_out), s));
  return SPFE_OK;
}

// ---- the fallback steps of Tracking::track() (tracker.cpp:182-233) -------------------------------------------------------
int spfe_track_motion_model_record_device(spfe_handle h, const void *d_record, const void *d_xyz, const void *d_desc,
                                          const void *d_flags, int n, void *d_mp_of_kp, const void *d_Tcw,
                                          const spfe_proj_params *proj_prm, const spfe_pose_params *pose_prm, int th_nmatch_proj,
                                          int th_nmatch_opt, void *d_proj_out, void *d_pose_out, void *stream) {
  if (!h || !d_record || !d_mp_of_kp || !d_Tcw || !proj_prm || !pose_prm || !d_proj_out || !d_pose_out)
    return fail(SPFE_EINVAL, "null argument");
  if (proj_prm->mode != SPFE_PROJ_LAST_FRAME) return fail(SPFE_EINVAL, "the motion-model chain searches in SPFE_PROJ_LAST_FRAME mode");
  if (pose_prm->schedule != SPFE_POSE_OPTIMIZATION) return fail(SPFE_EINVAL, "the chained form runs SPFE_POSE_OPTIMIZATION");
  int rc = pose_check(pose_prm);
  if (rc) return rc;
  spfe_proj_params wide = *proj_prm;   // the retry's window (tracker.cpp:506): it must fit as well
  wide.th = 2 * proj_prm->th;
  if ((rc = proj_check(h, n, h->kmax, proj_prm)) || (rc = proj_check(h, n, h->kmax, &wide))) return rc;
  if (proj_null_points(n, proj_prm->mode, d_xyz, nullptr, d_desc, d_flags)) return fail(SPFE_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = proj_scratch(h, (size_t)std::max(n, 1)))) return rc;
  hipStream_t s = stream_of(h, stream);
  const RecordView rec(h, d_record);
  uint8_t *pose_out = reinterpret_cast<uint8_t *>(d_pose_out);
  // fill(mvpMapPoints, NULL); SearchByProjection(mCurrentFrame, mLastFrame, th, mono)   tracker.cpp:489, :499
  HIP_TRY(spfe::launch_fill_u32(d_mp_of_kp, 0xffffffffu, (size_t)h->kmax, s));
  spfe::ProjArgs a = proj_record_args(h, rec, d_xyz, nullptr, d_desc, d_flags, d_mp_of_kp, d_Tcw, proj_prm, d_proj_out);
  a.n = n;
  a.cap = std::max(n, 1);
  a.refuse_overflow = 1;
  HIP_TRY(spfe::launch_proj_search(a, s));
  // if (nmatches < th_nmatch_proj): fill(NULL) and the search with 2 * th   :503-508, on the first search's own count
  a.th = wide.th;
  a.gate_count = reinterpret_cast<const int *>(d_proj_out);
  a.gate_min = th_nmatch_proj;
  a.gate_flag = reinterpret_cast<int *>(pose_out + SPFE_POSE_OFF_WIDENED);
  HIP_TRY(spfe::launch_proj_search(a, s));
  // Optimizer::PoseOptimization(&mCurrentFrame)   :517
  const spfe::PoseArgs p = pose_args(h, rec, d_mp_of_kp, n > 0 ? d_xyz : d_Tcw, d_Tcw, pose_prm, d_pose_out, n);
  HIP_TRY(spfe::launch_pose_refine(p, s));
  // Discard outliers, nmatchesMap >= th_nmatch_opt   :520-535, :558
  HIP_TRY(spfe::launch_track_discard(rec.hdr(), h->kmax, reinterpret_cast<int *>(d_mp_of_kp),
                                     reinterpret_cast<const uint8_t *>(d_flags), n, reinterpret_cast<const int *>(d_proj_out),
                                     th_nmatch_opt, SPFE_TRACK_FAIL_MOTION_INLIERS, pose_out, s));
  return SPFE_OK;
}

int spfe_track_reference_kf_record_device(spfe_handle h, const void *d_record, const void *d_kf_record, const void *d_kf_mp_of_kp,
                                          const void *d_xyz, const void *d_flags, int n, void *d_mp_of_kp, const void *d_Tcw,
                                          const spfe_pose_params *pose_prm, int th_nmatch_opt, void *d_pose_out, void *stream) {
  if (!h || !d_record || !d_kf_record || !d_kf_mp_of_kp || !d_mp_of_kp || !d_Tcw || !pose_prm || !d_pose_out ||
      (n > 0 && (!d_xyz || !d_flags)))
    return fail(SPFE_EINVAL, "null argument");
  if (n < 0 || n > SPFE_PROJ_MAX_POINTS) return fail(SPFE_EINVAL, "n_points %d not in [0, %d]", n, SPFE_PROJ_MAX_POINTS);
  if (pose_prm->schedule != SPFE_POSE_OPTIMIZATION) return fail(SPFE_EINVAL, "the chained form runs SPFE_POSE_OPTIMIZATION");
  int rc = pose_check(pose_prm);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = match_scratch(h, 1, h->kmax)) || (rc = reserve(h, h->m_out, (size_t)h->kmax * 8))) return rc;
  hipStream_t s = stream_of(h, stream);
  const RecordView rec(h, d_record);
  // SearchByBruteForce(mpReferenceKF, mCurrentFrame, mps): the train set is the keyframe's keypoints that hold a point
  // (sp_matcher.cpp:1654-1660), BFMatcher(NORM_L2, crossCheck)->match(all of the frame's rows)   :1662-1669
  const spfe::MatchSide q = record_side(h, d_record);
  spfe::MatchSide t = record_side(h, d_kf_record);
  t.mask = reinterpret_cast<const int *>(d_kf_mp_of_kp);
  t.mask_n = n;
  HIP_TRY(spfe::launch_match(q, t, 1, true, h->m_best_t.as<unsigned long long>(), h->m_best_q.as<unsigned long long>(),
                             h->m_out.p, 0, s));
  // vpMatches12[m.queryIdx] = vpMapPoints1[indices_train[m.trainIdx]]   :1671-1673
  HIP_TRY(spfe::launch_match_scatter_points(h->m_out.as<int32_t>(), t.mask, rec.hdr(), h->kmax, n,
                                            reinterpret_cast<int *>(d_mp_of_kp), s));
  // SetPose(mLastFrame.mTcw); Optimizer::PoseOptimization(&mCurrentFrame)   tracker.cpp:391-393
  const spfe::PoseArgs p = pose_args(h, rec, d_mp_of_kp, n > 0 ? d_xyz : d_Tcw, d_Tcw, pose_prm, d_pose_out, n);
  HIP_TRY(spfe::launch_pose_refine(p, s));
  // Discard outliers, nmatchesMap >= th_nmatch_opt   :395-416
  HIP_TRY(spfe::launch_track_discard(rec.hdr(), h->kmax, reinterpret_cast<int *>(d_mp_of_kp),
                                     reinterpret_cast<const uint8_t *>(d_flags), n, nullptr, th_nmatch_opt,
                                     SPFE_TRACK_FAIL_REFKF_INLIERS, reinterpret_cast<uint8_t *>(d_pose_out), s));
  return SPFE_OK;
}

// ---- the mapper: CreateNewMapPointsOverride (local_mapper.cpp:558-814) ---------------------------------------------------
size_t spfe_tri_out_bytes(spfe_handle h) { return h ? SPFE_TRI_OUT_BYTES(h->kmax) : 0; }

int spfe_create_map_points_pair_record_device(spfe_handle h, const void *d_record1, const void *d_record2, void *d_mp1_of_kp,
                                              void *d_mp2_of_kp, const void *d_Tcw1, const void *d_Tcw2,
                                              const spfe_tri_params *prm, int point_base, void *d_out, void *stream) {
  if (!h || !d_record1 || !d_record2 || !d_mp1_of_kp || !d_mp2_of_kp || !d_Tcw1 || !d_Tcw2 || !prm || !d_out)
    return fail(SPFE_EINVAL, "null argument");
  int rc = tri_check(h, prm, point_base);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = tri_scratch(h))) return rc;
  return tri_neighbour(h, d_record1, d_record2, d_mp1_of_kp, d_mp2_of_kp, d_Tcw1, d_Tcw2, nullptr, prm, point_base, true, d_out,
                       stream_of(h, stream));
}

int spfe_create_map_points_record_device(spfe_handle h, const void *d_record1, const void *const *d_records2, int n_neigh,
                                         void *d_mp1_of_kp, void *d_mp2_of_kp, const void *d_Tcw1, const void *d_Tcw2,
                                         const void *d_median_depth, const spfe_tri_params *prm, int point_base, void *d_out,
                                         void *stream) {
  if (!h || !d_record1 || !d_records2 || !d_mp1_of_kp || !d_mp2_of_kp || !d_Tcw1 || !d_Tcw2 || !d_median_depth || !prm || !d_out)
    return fail(SPFE_EINVAL, "null argument");
  if (n_neigh < 1 || n_neigh > SPFE_TRI_MAX_NEIGHBOURS)
    return fail(SPFE_EINVAL, "n_neigh %d not in [1, %d]", n_neigh, SPFE_TRI_MAX_NEIGHBOURS);
  for (int j = 0; j < n_neigh; ++j)
    if (!d_records2[j]) return fail(SPFE_EINVAL, "null argument");
  int rc = tri_check(h, prm, point_base);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = tri_scratch(h))) return rc;
  hipStream_t s = stream_of(h, stream);
  const size_t out_b = SPFE_TRI_OUT_BYTES(h->kmax);
  // for (i < vpNeighKFs.size()): the baseline test, the search, the triangulation, buildIndexes() of both   :592-800
  for (int j = 0; j < n_neigh; ++j) {
    rc = tri_neighbour(h, d_record1, d_records2[j], d_mp1_of_kp, reinterpret_cast<int *>(d_mp2_of_kp) + (size_t)j * h->kmax,
                       d_Tcw1, reinterpret_cast<const float *>(d_Tcw2) + 16 * j,
                       reinterpret_cast<const float *>(d_median_depth) + j, prm, point_base, j == 0,
                       reinterpret_cast<uint8_t *>(d_out) + (size_t)j * out_b, s);
    if (rc) return rc;
  }
  return SPFE_OK;
}

// ---- the mapper: the search of SPMatcher::Fuse in SearchInNeighbors (sp_matcher.cpp:965-1104, local_mapper.cpp:816-904) ----
int spfe_fuse_record_device(spfe_handle h, const void *d_record, const void *d_kf_mp_of_kp, const void *d_Tcw,
                            const void *d_point_id, const void *d_xyz, const void *d_normal, const void *d_dist_range,
                            const void *d_desc, const void *d_flags, int n, int n_cap, const spfe_fuse_params *prm, void *d_out,
                            void *stream) {
  if (!h || !d_record || !d_kf_mp_of_kp || !d_Tcw || !prm || !d_out) return fail(SPFE_EINVAL, "null argument");
  int rc = fuse_check(n, n_cap, prm);
  if (rc) return rc;
  if (fuse_null_points(n, d_point_id, d_xyz, d_normal, d_dist_range, d_desc, d_flags)) return fail(SPFE_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(h->cfg.device));
  return fuse_records(h, &d_record, 1, d_kf_mp_of_kp, d_Tcw, d_point_id, d_xyz, d_normal, d_dist_range, d_desc, d_flags, n, n_cap,
                      prm, d_out, stream_of(h, stream));
}

int spfe_fuse_targets_record_device(spfe_handle h, const void *const *d_records, int n_targets, const void *d_kf_mp_of_kp,
                                    const void *d_Tcw, const void *d_point_id, const void *d_xyz, const void *d_normal,
                                    const void *d_dist_range, const void *d_desc, const void *d_flags, int n, int n_cap,
                                    const spfe_fuse_params *prm, void *d_out, void *stream) {
  if (!h || !d_records || !d_kf_mp_of_kp || !d_Tcw || !prm || !d_out) return fail(SPFE_EINVAL, "null argument");
  if (n_targets < 1 || n_targets > SPFE_FUSE_MAX_TARGETS)
    return fail(SPFE_EINVAL, "n_targets %d not in [1, %d]", n_targets, SPFE_FUSE_MAX_TARGETS);
  for (int j = 0; j < n_targets; ++j)
    if (!d_records[j]) return fail(SPFE_EINVAL, "null argument");
  int rc = fuse_check(n, n_cap, prm);
  if (rc) return rc;
  if (fuse_null_points(n, d_point_id, d_xyz, d_normal, d_dist_range, d_desc, d_flags)) return fail(SPFE_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(h->cfg.device));
  // for (vit : vpTargetKFs) matcher.Fuse(pKFi, vpMapPointMatches): the targets are blockIdx.y of the same two launches   :854-860
  return fuse_records(h, d_records, n_targets, d_kf_mp_of_kp, d_Tcw, d_point_id, d_xyz, d_normal, d_dist_range, d_desc, d_flags, n,
                      n_cap, prm, d_out, stream_of(h, stream));
}

// the host-array form of both fuse searches: one target staged into the handle's buffer, `launch` on it, the block copied back
static int fuse_search_host(spfe_handle h, const float *kp_xy, const int16_t *occ_grid, const float *kp_desc, int K,
                            const int32_t *kf_mp_of_kp, const float *Tcw, const int32_t *point_id, const float *xyz,
                            const float *normal, const float *dist_range, const float *desc, const uint8_t *flags, int n,
                            const spfe_fuse_params *prm, int32_t *kp_of_mp, float *best_dist, int32_t *holder, uint8_t *reason,
                            int32_t *fused_idx, int *n_fused, FuseLaunch launch) {
  if (!h || !occ_grid || !Tcw || !prm) return fail(SPFE_EINVAL, "null argument");
  if (K < 0 || K > 32767) return fail(SPFE_EINVAL, "n_keypoints %d out of range", K);
  if (K > 0 && (!kp_xy || !kp_desc || !kf_mp_of_kp)) return fail(SPFE_EINVAL, "null argument");
  const int ncap = std::max(n, 1), kcap = std::max(K, 1);
  int rc = fuse_check(n, n < 0 ? 1 : ncap, prm);
  if (rc) return rc;
  if (fuse_null_points(n, point_id, xyz, normal, dist_range, desc, flags)) return fail(SPFE_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t cells = (size_t)h->hc * h->wc, out_b = SPFE_FUSE_OUT_BYTES(ncap);
  const size_t kc = (size_t)kcap, nc = (size_t)ncap;
  HostStage st(h);
  const int b_xy = st.in(kp_xy, (size_t)K * 8, kc * 8, 16), b_occ = st.in(occ_grid, cells * 2, cells * 2, 16),
            b_kd = st.in(kp_desc, (size_t)K * 1024, kc * 1024, 16), b_map = st.in(kf_mp_of_kp, (size_t)K * 4, kc * 4, 16),
            b_T = st.in(Tcw, 64, 64, 4), b_id = st.in(point_id, (size_t)n * 4, nc * 4, 4), b_p = st.in(xyz, (size_t)n * 12, nc * 12, 4),
            b_n = st.in(normal, (size_t)n * 12, nc * 12, 4), b_r = st.in(dist_range, (size_t)n * 8, nc * 8, 4),
            b_d = st.in(desc, (size_t)n * 1024, nc * 1024, 16), b_f = st.in(flags, (size_t)n, nc, 1), b_out = st.out(out_b);
  if ((rc = st.commit())) return rc;
  spfe::FuseArgs a{};   // the staging buffer as the one "record"
  a.base[0] = st.base();
  a.n_targets = 1;
  a.off_xy = (long)st.off(b_xy); a.off_occ = (long)st.off(b_occ); a.off_desc = (long)st.off(b_kd); a.off_hdr = -1;
  a.k_imm = K;
  a.kmax = kcap;
  rc = fuse_launch(h, a, st.dev<void>(b_map), st.dev<void>(b_T), st.dev<void>(b_id), st.dev<void>(b_p), st.dev<void>(b_n),
                   st.dev<void>(b_r), st.dev<void>(b_d), st.dev<void>(b_f), n, ncap, prm, st.dev<void>(b_out), h->stream, launch);
  if (rc) return rc;
  st.fetch(b_out, out_b);
  if ((rc = st.sync())) return rc;
  const uint8_t *o = st.host<uint8_t>(b_out);
  const int nf = *reinterpret_cast<const int *>(o + SPFE_FUSE_OFF_N_FUSED);
  if (n_fused) *n_fused = nf;
  if (n > 0) {
    if (kp_of_mp) memcpy(kp_of_mp, o + SPFE_FUSE_OFF_KP_OF_MP, (size_t)n * 4);
    if (best_dist) memcpy(best_dist, o + SPFE_FUSE_OFF_BEST_DIST(ncap), (size_t)n * 4);
    if (holder) memcpy(holder, o + SPFE_FUSE_OFF_HOLDER(ncap), (size_t)n * 4);
    if (reason) memcpy(reason, o + SPFE_FUSE_OFF_REASON(ncap), (size_t)n);
    if (fused_idx && nf > 0) memcpy(fused_idx, o + SPFE_FUSE_OFF_FUSED_IDX(ncap), (size_t)std::min(nf, n) * 4);
  }
  return SPFE_OK;
}

int spfe_fuse_search(spfe_handle h, const float *kp_xy, const int16_t *occ_grid, const float *kp_desc, int K,
                     const int32_t *kf_mp_of_kp, const float *Tcw, const int32_t *point_id, const float *xyz, const float *normal,
                     const float *dist_range, const float *desc, const uint8_t *flags, int n, const spfe_fuse_params *prm,
                     int32_t *kp_of_mp, float *best_dist, int32_t *holder, uint8_t *reason, int32_t *fused_idx, int *n_fused) {
  return fuse_search_host(h, kp_xy, occ_grid, kp_desc, K, kf_mp_of_kp, Tcw, point_id, xyz, normal, dist_range, desc, flags, n, prm,
                          kp_of_mp, best_dist, holder, reason, fused_idx, n_fused, spfe::launch_fuse_search);
}

// ---- the loop closer: SearchAndFuse and the corrected poses of CorrectLoop (loop_closer_vlad.cpp:536-571, :608-618, :701-726) ----
int spfe_loop_fuse_record_device(spfe_handle h, const void *d_record, const void *d_kf_mp_of_kp, const void *d_Scw,
                                 const void *d_point_id, const void *d_xyz, const void *d_normal, const void *d_dist_range,
                                 const void *d_desc, const void *d_flags, int n, int n_cap, const spfe_loop_fuse_params *prm,
                                 void *d_out, void *stream) {
  if (!h || !d_record || !d_kf_mp_of_kp || !d_Scw || !prm || !d_out) return fail(SPFE_EINVAL, "null argument");
  const spfe_fuse_params f = loop_fuse_params(prm);
  int rc = fuse_check(n, n_cap, &f);
  if (rc) return rc;
  if (fuse_null_points(n, d_point_id, d_xyz, d_normal, d_dist_range, d_desc, d_flags)) return fail(SPFE_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(h->cfg.device));
  return fuse_records(h, &d_record, 1, d_kf_mp_of_kp, d_Scw, d_point_id, d_xyz, d_normal, d_dist_range, d_desc, d_flags, n, n_cap,
                      &f, d_out, stream_of(h, stream), spfe::launch_loopfuse_search);
}

int spfe_loop_fuse_targets_record_device(spfe_handle h, const void *const *d_records, int n_targets, const void *d_kf_mp_of_kp,
                                         const void *d_Scw, const void *d_point_id, const void *d_xyz, const void *d_normal,
                                         const void *d_dist_range, const void *d_desc, const void *d_flags, int n, int n_cap,
                                         const spfe_loop_fuse_params *prm, void *d_out, void *stream) {
  if (!h || !d_records || !d_kf_mp_of_kp || !d_Scw || !prm || !d_out) return fail(SPFE_EINVAL, "null argument");
  if (n_targets < 1 || n_targets > SPFE_FUSE_MAX_TARGETS)
    return fail(SPFE_EINVAL, "n_targets %d not in [1, %d]", n_targets, SPFE_FUSE_MAX_TARGETS);
  for (int j = 0; j < n_targets; ++j)
    if (!d_records[j]) return fail(SPFE_EINVAL, "null argument");
  const spfe_fuse_params f = loop_fuse_params(prm);
  int rc = fuse_check(n, n_cap, &f);
  if (rc) return rc;
  if (fuse_null_points(n, d_point_id, d_xyz, d_normal, d_dist_range, d_desc, d_flags)) return fail(SPFE_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(h->cfg.device));
  // for (mit : CorrectedPosesMap) matcher.Fuse(pKF, cvScw, mvpLoopMapPoints, 4, ...): the targets are blockIdx.y   :704-714
  return fuse_records(h, d_records, n_targets, d_kf_mp_of_kp, d_Scw, d_point_id, d_xyz, d_normal, d_dist_range, d_desc, d_flags, n,
                      n_cap, &f, d_out, stream_of(h, stream), spfe::launch_loopfuse_search);
}

int spfe_loop_fuse_search(spfe_handle h, const float *kp_xy, const int16_t *occ_grid, const float *kp_desc, int K,
                          const int32_t *kf_mp_of_kp, const float *Scw, const int32_t *point_id, const float *xyz,
                          const float *normal, const float *dist_range, const float *desc, const uint8_t *flags, int n,
                          const spfe_loop_fuse_params *prm, int32_t *kp_of_mp, float *best_dist, int32_t *holder, uint8_t *reason,
                          int32_t *fused_idx, int *n_fused) {
  if (!prm) return fail(SPFE_EINVAL, "null argument");
  const spfe_fuse_params f = loop_fuse_params(prm);
  return fuse_search_host(h, kp_xy, occ_grid, kp_desc, K, kf_mp_of_kp, Scw, point_id, xyz, normal, dist_range, desc, flags, n, &f,
                          kp_of_mp, best_dist, holder, reason, fused_idx, n_fused, spfe::launch_loopfuse_search);
}

static int loop_poses_check(int n_targets, int cur_index) {
  if (n_targets < 1 || n_targets > SPFE_FUSE_MAX_TARGETS)
    return fail(SPFE_EINVAL, "n_targets %d not in [1, %d]", n_targets, SPFE_FUSE_MAX_TARGETS);
  if (cur_index < -1 || cur_index >= n_targets) return fail(SPFE_EINVAL, "cur_index %d not in [-1, n_targets = %d)", cur_index, n_targets);
  return SPFE_OK;
}

int spfe_loop_corrected_poses_device(spfe_handle h, const void *d_opt_block, const void *d_Tcw2, const void *d_Twc, const void *d_Tiw,
                                     int n_targets, int cur_index, void *d_Siw, void *d_Tiw_corrected, void *stream) {
  if (!h || !d_opt_block || !d_Tcw2 || !d_Twc || !d_Tiw || !d_Siw || !d_Tiw_corrected) return fail(SPFE_EINVAL, "null argument");
  int rc = loop_poses_check(n_targets, cur_index);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  const double *S12 = reinterpret_cast<const double *>(reinterpret_cast<const uint8_t *>(d_opt_block) + SPFE_SIM3OPT_OFF_S12);
  HIP_TRY(spfe::launch_loopfuse_poses(S12, reinterpret_cast<const float *>(d_Tcw2), reinterpret_cast<const float *>(d_Twc),
                                      reinterpret_cast<const float *>(d_Tiw), n_targets, cur_index, reinterpret_cast<float *>(d_Siw),
                                      reinterpret_cast<float *>(d_Tiw_corrected), stream_of(h, stream)));
  return SPFE_OK;
}

int spfe_loop_corrected_poses(const double *S12, const float *Tcw2, const float *Twc, const float *Tiw, int n_targets, int cur_index,
                              float *Siw, float *Tiw_corrected) {
  if (!S12 || !Tcw2 || !Twc || !Tiw || !Siw || !Tiw_corrected) return fail(SPFE_EINVAL, "null argument");
  int rc = loop_poses_check(n_targets, cur_index);
  if (rc) return rc;
  for (int j = 0; j < n_targets; ++j)
    spfe_loopfuse_pose(S12, Tcw2, Twc, Tiw + 16 * (size_t)j, j == cur_index, Siw + 16 * (size_t)j, Tiw_corrected + 16 * (size_t)j);
  return SPFE_OK;
}

// ---- the loop closer: the front half of ComputeSim3 (loop_closer_vlad.cpp:345-449) ---------------------------------------
int spfe_loop_match_record_device(spfe_handle h, const void *d_record1, const void *d_record2, const void *d_kf1_mp_of_kp,
                                  const void *d_kf2_mp_of_kp, void *d_match12, void *d_n_matches, void *stream) {
  if (!h || !d_record1 || !d_record2 || !d_kf1_mp_of_kp || !d_kf2_mp_of_kp || !d_match12 || !d_n_matches)
    return fail(SPFE_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(h->cfg.device));
  int rc = loop_match_scratch(h);
  if (rc) return rc;
  return loop_match(h, d_record1, d_record2, d_kf1_mp_of_kp, d_kf2_mp_of_kp, d_match12, d_n_matches, stream_of(h, stream));
}

int spfe_sim3_ransac_device(spfe_handle h, int K1, const void *d_match12, const void *d_kf1_mp_of_kp, const void *d_kf2_mp_of_kp,
                            const void *d_xyz, const void *d_flags, int n, const void *d_Tcw1, const void *d_Tcw2,
                            const void *d_rand_u32, int n_hyp, const spfe_sim3_params *prm, void *d_out, void *stream) {
  if (!h || !d_match12 || !d_kf1_mp_of_kp || !d_kf2_mp_of_kp || !d_Tcw1 || !d_Tcw2 || !d_rand_u32 || !prm || !d_out ||
      (n > 0 && (!d_xyz || !d_flags)))
    return fail(SPFE_EINVAL, "null argument");
  if (K1 < 0 || K1 > h->kmax) return fail(SPFE_EINVAL, "K1 %d not in [0, kmax = %d]", K1, h->kmax);
  int rc = sim3_check(n, n_hyp, prm);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = sim3_scratch(h, 1, h->kmax))) return rc;
  spfe::Sim3Args a{};
  sim3_fill(a, prm);
  a.n_cand = 1; a.k_imm = K1; a.kcap = h->kmax;
  a.match12 = reinterpret_cast<const int *>(d_match12);
  a.mp1 = reinterpret_cast<const int *>(d_kf1_mp_of_kp); a.mp2 = reinterpret_cast<const int *>(d_kf2_mp_of_kp);
  a.xyz = reinterpret_cast<const float *>(d_xyz); a.flags = reinterpret_cast<const uint8_t *>(d_flags); a.n = n;
  a.Tcw1 = reinterpret_cast<const float *>(d_Tcw1); a.Tcw2 = reinterpret_cast<const float *>(d_Tcw2);
  a.rnd = reinterpret_cast<const uint32_t *>(d_rand_u32); a.n_hyp = n_hyp;
  a.scratch = h->s3_scratch.as<float>();
  a.out = reinterpret_cast<uint8_t *>(d_out);
  HIP_TRY(spfe::launch_sim3(a, stream_of(h, stream)));
  return SPFE_OK;
}

int spfe_sim3_ransac(spfe_handle h, int K1, const int32_t *match12, const int32_t *kf1_mp_of_kp, int K2,
                     const int32_t *kf2_mp_of_kp, const float *xyz, const uint8_t *flags, int n, const float *Tcw1,
                     const float *Tcw2, const uint32_t *rand_u32, int n_hyp, const spfe_sim3_params *prm, void *out) {
  if (!h || !Tcw1 || !Tcw2 || !rand_u32 || !prm || !out || (n > 0 && (!xyz || !flags))) return fail(SPFE_EINVAL, "null argument");
  if (K1 < 0 || K1 > 32767 || K2 < 0 || K2 > 32767) return fail(SPFE_EINVAL, "keypoint counts %d, %d out of range", K1, K2);
  if ((K1 > 0 && (!match12 || !kf1_mp_of_kp)) || (K2 > 0 && !kf2_mp_of_kp)) return fail(SPFE_EINVAL, "null argument");
  int rc = sim3_check(n, n_hyp, prm);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  const int kcap = std::max(std::max(K1, K2), 1), ncap = std::max(n, 1);
  const size_t out_b = SPFE_SIM3_OUT_BYTES(kcap, n_hyp);
  const size_t kc = (size_t)kcap, nc = (size_t)ncap;
  HostStage st(h);   // the three index arrays: -1 beyond K1 / K2
  const int b_m = st.in(match12, (size_t)K1 * 4, kc * 4, 4, true), b_1 = st.in(kf1_mp_of_kp, (size_t)K1 * 4, kc * 4, 4, true),
            b_2 = st.in(kf2_mp_of_kp, (size_t)K2 * 4, kc * 4, 4, true), b_p = st.in(xyz, (size_t)n * 12, nc * 12, 4),
            b_f = st.in(flags, (size_t)n, nc, 1), b_T1 = st.in(Tcw1, 64, 64, 4), b_T2 = st.in(Tcw2, 64, 64, 4),
            b_r = st.in(rand_u32, (size_t)n_hyp * 12, (size_t)n_hyp * 12, 4), b_out = st.out(out_b, out);
  if ((rc = sim3_scratch(h, 1, kcap)) || (rc = st.commit())) return rc;
  spfe::Sim3Args a{};
  sim3_fill(a, prm);
  a.n_cand = 1; a.k_imm = K1; a.kcap = kcap;
  a.match12 = st.dev<int>(b_m);
  a.mp1 = st.dev<int>(b_1); a.mp2 = st.dev<int>(b_2);
  a.xyz = st.dev<float>(b_p); a.flags = st.dev<uint8_t>(b_f); a.n = n;
  a.Tcw1 = st.dev<float>(b_T1); a.Tcw2 = st.dev<float>(b_T2);
  a.rnd = st.dev<uint32_t>(b_r); a.n_hyp = n_hyp;
  a.scratch = h->s3_scratch.as<float>();
  a.out = st.dev<uint8_t>(b_out);
  HIP_TRY(spfe::launch_sim3(a, h->stream));
  if ((rc = st.fetch_to(out, a.out, out_b))) return rc;
  return st.sync();
}

int spfe_loop_verify_records_device(spfe_handle h, const void *d_record1, const void *const *d_records2, int n_cand,
                                    const void *d_kf1_mp_of_kp, const void *d_kf2_mp_of_kp, const void *d_xyz, const void *d_flags,
                                    int n, const void *d_Tcw1, const void *d_Tcw2, const void *d_rand_u32, int n_hyp,
                                    const spfe_sim3_params *prm, void *d_match12, void *d_n_matches, void *d_out, void *stream) {
  if (!h || !d_record1 || !d_records2 || !d_kf1_mp_of_kp || !d_kf2_mp_of_kp || !d_Tcw1 || !d_Tcw2 || !d_rand_u32 || !prm ||
      !d_match12 || !d_n_matches || !d_out || (n > 0 && (!d_xyz || !d_flags)))
    return fail(SPFE_EINVAL, "null argument");
  if (n_cand < 1 || n_cand > SPFE_SIM3_MAX_CANDIDATES)
    return fail(SPFE_EINVAL, "n_cand %d not in [1, %d]", n_cand, SPFE_SIM3_MAX_CANDIDATES);
  for (int j = 0; j < n_cand; ++j)
    if (!d_records2[j]) return fail(SPFE_EINVAL, "null argument");
  int rc = sim3_check(n, n_hyp, prm);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = loop_match_scratch(h)) || (rc = sim3_scratch(h, n_cand, h->kmax))) return rc;
  hipStream_t s = stream_of(h, stream);
  // for (i < nInitialCandidates) SearchByBruteForce(mpCurrentKF, pKF, vvpMapPointMatches[i])   :367-391
  for (int j = 0; j < n_cand; ++j) {
    rc = loop_match(h, d_record1, d_records2[j], d_kf1_mp_of_kp, reinterpret_cast<const int *>(d_kf2_mp_of_kp) + (size_t)j * h->kmax,
                    reinterpret_cast<int *>(d_match12) + (size_t)j * h->kmax, reinterpret_cast<int *>(d_n_matches) + j, s);
    if (rc) return rc;
  }
  // new Sim3Solver(...) and every hypothesis iterate() can reach, the candidates side by side   :384-386, :395-449
  spfe::Sim3Args a{};
  sim3_fill(a, prm);
  a.n_cand = n_cand; a.hdr1 = RecordView(h, d_record1).hdr(); a.kcap = h->kmax;
  a.match12 = reinterpret_cast<const int *>(d_match12);
  a.mp1 = reinterpret_cast<const int *>(d_kf1_mp_of_kp); a.mp2 = reinterpret_cast<const int *>(d_kf2_mp_of_kp);
  a.xyz = reinterpret_cast<const float *>(d_xyz); a.flags = reinterpret_cast<const uint8_t *>(d_flags); a.n = n;
  a.Tcw1 = reinterpret_cast<const float *>(d_Tcw1); a.Tcw2 = reinterpret_cast<const float *>(d_Tcw2);
  a.rnd = reinterpret_cast<const uint32_t *>(d_rand_u32); a.n_hyp = n_hyp;
  a.scratch = h->s3_scratch.as<float>();
  a.out = reinterpret_cast<uint8_t *>(d_out);
  HIP_TRY(spfe::launch_sim3(a, s));
  return SPFE_OK;
}

// ---- the loop closer: SearchBySim3Override of a returning hypothesis (sp_matcher_loop.cpp:7-220, loop_closer_vlad.cpp:418-432) ----
int spfe_search_by_sim3_record_device(spfe_handle h, const void *d_record1, const void *d_record2, const void *d_kf1_mp_of_kp,
                                      const void *d_kf2_mp_of_kp, const void *d_xyz, const void *d_flags, const void *d_dist_range,
                                      const void *d_desc, int n, const void *d_Tcw1, const void *d_Tcw2, const void *d_T12,
                                      const void *d_seed12, const spfe_guided_params *prm, void *d_out, void *stream) {
  if (!h || !d_record1 || !d_record2 || !d_kf1_mp_of_kp || !d_kf2_mp_of_kp || !d_Tcw1 || !d_Tcw2 || !d_T12 || !d_seed12 || !prm ||
      !d_out || guided_null_map(n, d_xyz, d_flags, d_dist_range, d_desc))
    return fail(SPFE_EINVAL, "null argument");
  int rc = guided_check(n, prm);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = reserve(h, h->gd_scratch, spfe::guided_scratch_bytes(h->kmax)))) return rc;
  spfe::GuidedArgs a{};
  guided_fill(h, a, prm);
  guided_records(h, a, d_record1, d_kf1_mp_of_kp, d_kf2_mp_of_kp, d_xyz, d_flags, d_dist_range, d_desc, n, d_Tcw1, d_Tcw2, d_out);
  a.base2[0] = reinterpret_cast<const uint8_t *>(d_record2);
  a.n_jobs = 1;
  a.T12 = reinterpret_cast<const float *>(d_T12); a.seed12 = reinterpret_cast<const int *>(d_seed12);
  a.scratch = h->gd_scratch.p;
  HIP_TRY(spfe::launch_guided_match(a, stream_of(h, stream)));
  return SPFE_OK;
}

int spfe_loop_guided_match_records_device(spfe_handle h, const void *d_record1, const void *const *d_records2, int n_cand,
                                          const int32_t *jobs, int n_jobs, const void *d_kf1_mp_of_kp, const void *d_kf2_mp_of_kp,
                                          const void *d_xyz, const void *d_flags, const void *d_dist_range, const void *d_desc, int n,
                                          const void *d_Tcw1, const void *d_Tcw2, const void *d_match12, const void *d_verify_out,
                                          int n_hyp, const spfe_guided_params *prm, void *d_out, void *stream) {
  if (!h || !d_record1 || !d_records2 || !jobs || !d_kf1_mp_of_kp || !d_kf2_mp_of_kp || !d_Tcw1 || !d_Tcw2 || !d_match12 ||
      !d_verify_out || !prm || !d_out || guided_null_map(n, d_xyz, d_flags, d_dist_range, d_desc))
    return fail(SPFE_EINVAL, "null argument");
  if (n_cand < 1 || n_cand > SPFE_SIM3_MAX_CANDIDATES)
    return fail(SPFE_EINVAL, "n_cand %d not in [1, %d]", n_cand, SPFE_SIM3_MAX_CANDIDATES);
  if (n_jobs < 1 || n_jobs > SPFE_GUIDED_MAX_JOBS) return fail(SPFE_EINVAL, "n_jobs %d not in [1, %d]", n_jobs, SPFE_GUIDED_MAX_JOBS);
  if (n_hyp < 1 || n_hyp > SPFE_SIM3_MAX_HYPOTHESES)
    return fail(SPFE_EINVAL, "n_hyp %d not in [1, %d]", n_hyp, SPFE_SIM3_MAX_HYPOTHESES);
  for (int j = 0; j < n_cand; ++j)
    if (!d_records2[j]) return fail(SPFE_EINVAL, "null argument");
  for (int q = 0; q < n_jobs; ++q)
    if (jobs[2 * q] < 0 || jobs[2 * q] >= n_cand || jobs[2 * q + 1] < 0 || jobs[2 * q + 1] >= n_hyp)
      return fail(SPFE_EINVAL, "job %d names candidate %d of %d, hypothesis %d of %d", q, jobs[2 * q], n_cand, jobs[2 * q + 1], n_hyp);
  int rc = guided_check(n, prm);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = reserve(h, h->gd_scratch, (size_t)n_jobs * spfe::guided_scratch_bytes(h->kmax)))) return rc;
  spfe::GuidedArgs a{};
  guided_fill(h, a, prm);
  guided_records(h, a, d_record1, d_kf1_mp_of_kp, d_kf2_mp_of_kp, d_xyz, d_flags, d_dist_range, d_desc, n, d_Tcw1, d_Tcw2, d_out);
  for (int q = 0; q < n_jobs; ++q) {
    a.cand[q] = jobs[2 * q];
    a.hyp[q] = jobs[2 * q + 1];
    a.base2[q] = reinterpret_cast<const uint8_t *>(d_records2[jobs[2 * q]]);
  }
  a.n_jobs = n_jobs;
  a.verify = reinterpret_cast<const uint8_t *>(d_verify_out); a.match12 = reinterpret_cast<const int *>(d_match12); a.n_hyp = n_hyp;
  a.scratch = h->gd_scratch.p;
  // for every returning hypothesis: SearchBySim3Override(mpCurrentKF, pKF, vpMapPointMatches, s, R, t, 7.5)   :418-432
  HIP_TRY(spfe::launch_guided_match(a, stream_of(h, stream)));
  return SPFE_OK;
}

int spfe_search_by_sim3(spfe_handle h, const float *kp_xy1, const int16_t *occ_grid1, const float *kp_desc1, int K1,
                        const int32_t *kf1_mp_of_kp, const float *kp_xy2, const int16_t *occ_grid2, const float *kp_desc2, int K2,
                        const int32_t *kf2_mp_of_kp, const float *xyz, const uint8_t *flags, const float *dist_range,
                        const float *desc, int n, const float *Tcw1, const float *Tcw2, const float *T12, const int32_t *seed12,
                        const spfe_guided_params *prm, void *out) {
  if (!h || !occ_grid1 || !occ_grid2 || !Tcw1 || !Tcw2 || !T12 || !prm || !out) return fail(SPFE_EINVAL, "null argument");
  if (K1 < 0 || K1 > 32767 || K2 < 0 || K2 > 32767) return fail(SPFE_EINVAL, "keypoint counts %d, %d out of range", K1, K2);
  if ((K1 > 0 && (!kp_xy1 || !kp_desc1 || !kf1_mp_of_kp || !seed12)) || (K2 > 0 && (!kp_xy2 || !kp_desc2 || !kf2_mp_of_kp)))
    return fail(SPFE_EINVAL, "null argument");
  if (guided_null_map(n, xyz, flags, dist_range, desc)) return fail(SPFE_EINVAL, "null argument");
  int rc = guided_check(n, prm);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  const int kcap = std::max(std::max(K1, K2), 1), ncap = std::max(n, 1);
  const size_t cells = (size_t)h->hc * h->wc, out_b = SPFE_GUIDED_OUT_BYTES(kcap);
  const size_t kc = (size_t)kcap, nc = (size_t)ncap;
  HostStage st(h);
  // the two keyframes, each a unit of 256 bytes with the same offsets (the "records" of this call); then the three index
  // arrays, -1 beyond K1 / K2
  const int b_xy1 = st.in(kp_xy1, (size_t)K1 * 8, kc * 8, 256), b_occ1 = st.in(occ_grid1, cells * 2, cells * 2, 16),
            b_kd1 = st.in(kp_desc1, (size_t)K1 * 1024, kc * 1024, 16);
  st.pad(256);
  const int b_xy2 = st.in(kp_xy2, (size_t)K2 * 8, kc * 8, 256);
  st.in(occ_grid2, cells * 2, cells * 2, 16);
  st.in(kp_desc2, (size_t)K2 * 1024, kc * 1024, 16);
  st.pad(256);
  const int b_m1 = st.in(kf1_mp_of_kp, (size_t)K1 * 4, kc * 4, 4, true), b_m2 = st.in(kf2_mp_of_kp, (size_t)K2 * 4, kc * 4, 4, true),
            b_seed = st.in(seed12, (size_t)K1 * 4, kc * 4, 4, true), b_p = st.in(xyz, (size_t)n * 12, nc * 12, 4),
            b_r = st.in(dist_range, (size_t)n * 8, nc * 8, 4), b_d = st.in(desc, (size_t)n * 1024, nc * 1024, 16),
            b_f = st.in(flags, (size_t)n, nc, 1), b_T1 = st.in(Tcw1, 64, 64, 4), b_T2 = st.in(Tcw2, 64, 64, 4),
            b_T12 = st.in(T12, 52, 64, 4), b_out = st.out(out_b, out);
  if ((rc = reserve(h, h->gd_scratch, spfe::guided_scratch_bytes(kcap))) || (rc = st.commit())) return rc;
  spfe::GuidedArgs a{};
  guided_fill(h, a, prm);
  a.base1 = st.dev<uint8_t>(b_xy1);
  a.base2[0] = st.dev<uint8_t>(b_xy2);
  a.n_jobs = 1;
  a.off_xy = 0; a.off_occ = (long)(st.off(b_occ1) - st.off(b_xy1)); a.off_desc = (long)(st.off(b_kd1) - st.off(b_xy1)); a.off_hdr = -1;
  a.k_imm1 = K1; a.k_imm2 = K2;
  a.kmax = kcap;
  guided_map(a, st.dev<void>(b_m1), st.dev<void>(b_m2), st.dev<void>(b_p), st.dev<void>(b_f), st.dev<void>(b_r), st.dev<void>(b_d), n,
             st.dev<void>(b_T1), st.dev<void>(b_T2), st.dev<void>(b_out));
  a.T12 = st.dev<float>(b_T12); a.seed12 = st.dev<int>(b_seed);
  a.scratch = h->gd_scratch.p;
  HIP_TRY(spfe::launch_guided_match(a, h->stream));
  if ((rc = st.fetch_to(out, a.out, out_b))) return rc;
  return st.sync();
}

// ---- the loop closer: SearchByProjectionLoop behind the accepted candidate (sp_matcher_loop.cpp:222-332) ----
int spfe_search_loop_points_record_device(spfe_handle h, const void *d_record, const void *d_Scw, void *d_matched,
                                          const void *d_point_id, const void *d_xyz, const void *d_normal, const void *d_dist_range,
                                          const void *d_desc, const void *d_flags, int n, int n_cap, const spfe_loop_proj_params *prm,
                                          void *d_out, void *stream) {
  if (!h || !d_record || !d_Scw || !d_matched || !prm || !d_out) return fail(SPFE_EINVAL, "null argument");
  int rc = loop_proj_check(n, n_cap, h->kmax, prm);
  if (rc) return rc;
  if (fuse_null_points(n, d_point_id, d_xyz, d_normal, d_dist_range, d_desc, d_flags)) return fail(SPFE_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = proj_scratch(h, (size_t)n_cap))) return rc;
  const RecordView rec(h, d_record);
  spfe::LoopProjArgs a{};
  loop_proj_fill(h, a, prm);
  a.kp_xy = rec.xy(); a.occ = rec.occ(); a.kp_desc = rec.desc(); a.kp_desc_bf16 = rec.desc_bf16(); a.hdr = rec.hdr();
  a.kmax = h->kmax;
  a.Scw = reinterpret_cast<const float *>(d_Scw);
  a.matched = reinterpret_cast<int *>(d_matched);
  a.point_id = reinterpret_cast<const int *>(d_point_id);
  a.xyz = reinterpret_cast<const float *>(d_xyz); a.normal = reinterpret_cast<const float *>(d_normal);
  a.dist_range = reinterpret_cast<const float *>(d_dist_range); a.desc = reinterpret_cast<const float *>(d_desc);
  a.flags = reinterpret_cast<const uint8_t *>(d_flags);
  a.n = n; a.cap = n_cap;
  a.out = reinterpret_cast<uint8_t *>(d_out);
  HIP_TRY(spfe::launch_loop_proj(a, stream_of(h, stream)));
  return SPFE_OK;
}

int spfe_search_loop_points(spfe_handle h, const float *kp_xy, const int16_t *occ_grid, const float *kp_desc, int K, const float *Scw,
                            int32_t *matched, const int32_t *point_id, const float *xyz, const float *normal,
                            const float *dist_range, const float *desc, const uint8_t *flags, int n,
                            const spfe_loop_proj_params *prm, int32_t *kp_of_mp, float *best_dist, uint8_t *reason,
                            int32_t *matched_idx, int *n_matched) {
  if (!h || !occ_grid || !Scw || !prm) return fail(SPFE_EINVAL, "null argument");
  if (K < 0 || K > 32767) return fail(SPFE_EINVAL, "n_keypoints %d out of range", K);
  if (K > 0 && (!kp_xy || !kp_desc || !matched)) return fail(SPFE_EINVAL, "null argument");
  const int ncap = std::max(n, 1), kcap = std::max(K, 1);
  int rc = loop_proj_check(n, n < 0 ? 1 : ncap, kcap, prm);
  if (rc) return rc;
  if (fuse_null_points(n, point_id, xyz, normal, dist_range, desc, flags)) return fail(SPFE_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t cells = (size_t)h->hc * h->wc, out_b = SPFE_LOOPPROJ_OUT_BYTES(ncap);
  const size_t kc = (size_t)kcap, nc = (size_t)ncap;
  HostStage st(h);
  const int b_xy = st.in(kp_xy, (size_t)K * 8, kc * 8, 16), b_occ = st.in(occ_grid, cells * 2, cells * 2, 16),
            b_kd = st.in(kp_desc, (size_t)K * 1024, kc * 1024, 16), b_map = st.in(matched, (size_t)K * 4, kc * 4, 16, true),
            b_T = st.in(Scw, 64, 64, 4), b_id = st.in(point_id, (size_t)n * 4, nc * 4, 4), b_p = st.in(xyz, (size_t)n * 12, nc * 12, 4),
            b_n = st.in(normal, (size_t)n * 12, nc * 12, 4), b_r = st.in(dist_range, (size_t)n * 8, nc * 8, 4),
            b_d = st.in(desc, (size_t)n * 1024, nc * 1024, 16), b_f = st.in(flags, (size_t)n, nc, 1), b_out = st.out(out_b);
  if ((rc = proj_scratch(h, nc)) || (rc = st.commit())) return rc;
  spfe::LoopProjArgs a{};
  loop_proj_fill(h, a, prm);
  a.kp_xy = st.dev<float>(b_xy); a.occ = st.dev<int16_t>(b_occ);
  a.kp_desc = st.dev<float>(b_kd); a.kp_desc_bf16 = 0; a.hdr = nullptr; a.k_imm = K;
  a.kmax = kcap;
  a.Scw = st.dev<float>(b_T);
  a.matched = st.dev<int>(b_map);
  a.point_id = st.dev<int>(b_id);
  a.xyz = st.dev<float>(b_p); a.normal = st.dev<float>(b_n);
  a.dist_range = st.dev<float>(b_r); a.desc = st.dev<float>(b_d);
  a.flags = st.dev<uint8_t>(b_f);
  a.n = n; a.cap = ncap;
  a.out = st.dev<uint8_t>(b_out);
  HIP_TRY(spfe::launch_loop_proj(a, h->stream));
  st.fetch(b_out, out_b);
  st.fetch(b_map, (size_t)K * 4);
  if ((rc = st.sync())) return rc;
  if (K > 0) memcpy(matched, st.host<int32_t>(b_map), (size_t)K * 4);
  const uint8_t *o = st.host<uint8_t>(b_out);
  const int nm = *reinterpret_cast<const int *>(o + SPFE_LOOPPROJ_OFF_N_MATCHED);
  if (n_matched) *n_matched = nm;
  if (n > 0) {
    if (kp_of_mp) memcpy(kp_of_mp, o + SPFE_LOOPPROJ_OFF_KP_OF_MP, (size_t)n * 4);
    if (best_dist) memcpy(best_dist, o + SPFE_LOOPPROJ_OFF_BEST_DIST(ncap), (size_t)n * 4);
    if (reason) memcpy(reason, o + SPFE_LOOPPROJ_OFF_REASON(ncap), (size_t)n);
    if (matched_idx && nm > 0) memcpy(matched_idx, o + SPFE_LOOPPROJ_OFF_MATCHED_IDX(ncap), (size_t)std::min(nm, n) * 4);
  }
  return SPFE_OK;
}

// ---- the loop closer: OptimizeSim3 behind the guided match (optimizer.cpp:1062-1252, loop_closer_vlad.cpp:434-445) ----
int spfe_sim3opt_lds_edge_capacity(spfe_handle h, int kmax) {
  if (!h) return fail(SPFE_EINVAL, "null argument");
  return spfe::sim3opt_lds_edge_capacity(kmax > 0 ? kmax : h->kmax);
}

int spfe_optimize_sim3_record_device(spfe_handle h, const void *d_record1, const void *d_record2, const void *d_kf1_mp_of_kp,
                                     const void *d_kf2_mp_of_kp, const void *d_xyz, const void *d_flags, int n, const void *d_Tcw1,
                                     const void *d_Tcw2, const void *d_T12, const void *d_matches12,
                                     const spfe_sim3opt_params *prm, void *d_out, void *stream) {
  if (!h || !d_record1 || !d_record2 || !d_kf1_mp_of_kp || !d_kf2_mp_of_kp || !d_Tcw1 || !d_Tcw2 || !d_T12 || !d_matches12 ||
      !prm || !d_out || (n > 0 && (!d_xyz || !d_flags)))
    return fail(SPFE_EINVAL, "null argument");
  int rc = sim3opt_check(n, h->kmax, prm);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = reserve(h, h->so_scratch, spfe::sim3opt_scratch_bytes(h->kmax)))) return rc;
  spfe::Sim3OptArgs a{};
  sim3opt_fill(a, prm);
  sim3opt_records(h, a, d_record1, d_kf1_mp_of_kp, d_kf2_mp_of_kp, d_xyz, d_flags, n, d_Tcw1, d_Tcw2, d_out);
  a.base2[0] = reinterpret_cast<const uint8_t *>(d_record2);
  a.n_jobs = 1;
  a.T12 = reinterpret_cast<const float *>(d_T12); a.matches12 = reinterpret_cast<const int *>(d_matches12);
  a.scratch = h->so_scratch.as<float>();
  HIP_TRY(spfe::launch_sim3opt(a, stream_of(h, stream)));
  return SPFE_OK;
}

int spfe_loop_optimize_sim3_records_device(spfe_handle h, const void *d_record1, const void *const *d_records2, int n_cand,
                                           const int32_t *jobs, int n_jobs, const void *d_kf1_mp_of_kp, const void *d_kf2_mp_of_kp,
                                           const void *d_xyz, const void *d_flags, int n, const void *d_Tcw1, const void *d_Tcw2,
                                           const void *d_verify_out, int n_hyp, const void *d_guided_out,
                                           const spfe_sim3opt_params *prm, void *d_out, void *stream) {
  if (!h || !d_record1 || !d_records2 || !jobs || !d_kf1_mp_of_kp || !d_kf2_mp_of_kp || !d_Tcw1 || !d_Tcw2 || !d_verify_out ||
      !d_guided_out || !prm || !d_out || (n > 0 && (!d_xyz || !d_flags)))
    return fail(SPFE_EINVAL, "null argument");
  if (n_cand < 1 || n_cand > SPFE_SIM3_MAX_CANDIDATES)
    return fail(SPFE_EINVAL, "n_cand %d not in [1, %d]", n_cand, SPFE_SIM3_MAX_CANDIDATES);
  if (n_jobs < 1 || n_jobs > SPFE_GUIDED_MAX_JOBS) return fail(SPFE_EINVAL, "n_jobs %d not in [1, %d]", n_jobs, SPFE_GUIDED_MAX_JOBS);
  if (n_hyp < 1 || n_hyp > SPFE_SIM3_MAX_HYPOTHESES)
    return fail(SPFE_EINVAL, "n_hyp %d not in [1, %d]", n_hyp, SPFE_SIM3_MAX_HYPOTHESES);
  for (int j = 0; j < n_cand; ++j)
    if (!d_records2[j]) return fail(SPFE_EINVAL, "null argument");
  for (int q = 0; q < n_jobs; ++q)
    if (jobs[2 * q] < 0 || jobs[2 * q] >= n_cand || jobs[2 * q + 1] < 0 || jobs[2 * q + 1] >= n_hyp)
      return fail(SPFE_EINVAL, "job %d names candidate %d of %d, hypothesis %d of %d", q, jobs[2 * q], n_cand, jobs[2 * q + 1], n_hyp);
  int rc = sim3opt_check(n, h->kmax, prm);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = reserve(h, h->so_scratch, (size_t)n_jobs * spfe::sim3opt_scratch_bytes(h->kmax)))) return rc;
  spfe::Sim3OptArgs a{};
  sim3opt_fill(a, prm);
  sim3opt_records(h, a, d_record1, d_kf1_mp_of_kp, d_kf2_mp_of_kp, d_xyz, d_flags, n, d_Tcw1, d_Tcw2, d_out);
  for (int q = 0; q < n_jobs; ++q) {
    a.cand[q] = jobs[2 * q];
    a.hyp[q] = jobs[2 * q + 1];
    a.base2[q] = reinterpret_cast<const uint8_t *>(d_records2[jobs[2 * q]]);
  }
  a.n_jobs = n_jobs;
  a.verify = reinterpret_cast<const uint8_t *>(d_verify_out); a.guided = reinterpret_cast<const uint8_t *>(d_guided_out);
  a.n_hyp = n_hyp;
  a.scratch = h->so_scratch.as<float>();
  // for every returning hypothesis: Optimizer::OptimizeSim3(mpCurrentKF, pKF, vpMapPointMatches, gScm, 10, mbFixScale)   :434-445
  HIP_TRY(spfe::launch_sim3opt(a, stream_of(h, stream)));
  return SPFE_OK;
}

int spfe_optimize_sim3(spfe_handle h, const float *kp_xy1, int K1, const int32_t *kf1_mp_of_kp, const float *kp_xy2, int K2,
                       const int32_t *kf2_mp_of_kp, const float *xyz, const uint8_t *flags, int n, const float *Tcw1,
                       const float *Tcw2, const float *T12, const int32_t *matches12, const spfe_sim3opt_params *prm, void *out) {
  if (!h || !Tcw1 || !Tcw2 || !T12 || !prm || !out) return fail(SPFE_EINVAL, "null argument");
  if (K1 < 0 || K1 > 32767 || K2 < 0 || K2 > 32767) return fail(SPFE_EINVAL, "keypoint counts %d, %d out of range", K1, K2);
  if ((K1 > 0 && (!kp_xy1 || !kf1_mp_of_kp || !matches12)) || (K2 > 0 && (!kp_xy2 || !kf2_mp_of_kp)) || (n > 0 && (!xyz || !flags)))
    return fail(SPFE_EINVAL, "null argument");
  const int kcap = std::max(std::max(K1, K2), 1), ncap = std::max(n, 1);
  int rc = sim3opt_check(n, kcap, prm);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t out_b = SPFE_SIM3OPT_OUT_BYTES(kcap);
  const size_t kc = (size_t)kcap, nc = (size_t)ncap;
  HostStage st(h);   // the three index arrays: -1 beyond K1 / K2
  const int b_xy1 = st.in(kp_xy1, (size_t)K1 * 8, kc * 8, 16), b_xy2 = st.in(kp_xy2, (size_t)K2 * 8, kc * 8, 16),
            b_m1 = st.in(kf1_mp_of_kp, (size_t)K1 * 4, kc * 4, 4, true), b_m2 = st.in(kf2_mp_of_kp, (size_t)K2 * 4, kc * 4, 4, true),
            b_m12 = st.in(matches12, (size_t)K1 * 4, kc * 4, 4, true), b_p = st.in(xyz, (size_t)n * 12, nc * 12, 4),
            b_f = st.in(flags, (size_t)n, nc, 1), b_T1 = st.in(Tcw1, 64, 64, 4), b_T2 = st.in(Tcw2, 64, 64, 4),
            b_T12 = st.in(T12, 52, 64, 4), b_out = st.out(out_b, out);
  if ((rc = reserve(h, h->so_scratch, spfe::sim3opt_scratch_bytes(kcap))) || (rc = st.commit())) return rc;
  spfe::Sim3OptArgs a{};
  sim3opt_fill(a, prm);
  a.base1 = st.dev<uint8_t>(b_xy1);
  a.base2[0] = st.dev<uint8_t>(b_xy2);
  a.n_jobs = 1;
  a.off_xy = 0; a.off_hdr = -1;
  a.k_imm1 = K1; a.k_imm2 = K2;
  a.kmax = kcap;
  sim3opt_map(a, st.dev<void>(b_m1), st.dev<void>(b_m2), st.dev<void>(b_p), st.dev<void>(b_f), n, st.dev<void>(b_T1),
              st.dev<void>(b_T2), st.dev<void>(b_out));
  a.T12 = st.dev<float>(b_T12); a.matches12 = st.dev<int>(b_m12);
  a.scratch = h->so_scratch.as<float>();
  HIP_TRY(spfe::launch_sim3opt(a, h->stream));
  if ((rc = st.fetch_to(out, a.out, out_b))) return rc;
  return st.sync();
}

int spfe_sim3_iteration_limit(int N, double probability, int min_inliers, int max_iterations) {
  int n_iterations = 1;
  if (N > min_inliers) {
    const float epsilon = (float)min_inliers / N;
    const double x = ceil(log(1 - probability) / log(1 - pow(epsilon, 3)));
    n_iterations = x < (double)max_iterations ? (int)x : max_iterations;
  }
  return std::max(1, std::min(n_iterations, max_iterations));
}

}  // extern "C"
