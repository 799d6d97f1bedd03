/*
 * spfe_fuse_math.h — the arithmetic of the mapper's fuse search, shared by the GPU kernels (sp_orb_slam_amd/csrc/fuse.hip)
 * and the host C reference of the test suite (tests/fuse_ref/fuse_ref.c) so that both evaluate the same sequence of IEEE
 * operations (compile with -ffp-contract=off).  The camera, the window, the lane sum and the distance are those of
 * spfe_proj_math.h, unchanged.
 *
 * What it restates, in this project's own words:
 *   SPMatcher::Fuse(KeyFrame *, const vector<MapPoint *> &, th)   orb_slam2/src/cv/sp_matcher.cpp:965-1104
 *   KeyFrame::GetFeaturesInArea, KeyFrame::IsInImage              orb_slam2/src/type/keyframe.cpp:1018-1060
 *   as LocalMapping::SearchInNeighbors calls them                 orb_slam2/src/mapping/local_mapper.cpp:816-904
 *
 * One target keyframe: K keypoints with their occupancy grid and descriptor rows, a pose Tcw (row-major 4x4, f32) and
 * kf_mp_of_kp[k], the id of the map point keypoint k holds or -1.  Point i of the list: an id >= 0, a world position P, the
 * (not normalised) mean viewing direction n, the distance range (dmin, dmax) = (mfMinDistance, mfMaxDistance), a
 * descriptor and the SEARCHABLE flag (!isBad()).  The steps, in this order; the first that fails is the point's reason code:
 *
 *   1 SKIP_BAD       the point is not SEARCHABLE
 *   2 SKIP_IN_KF     some k < K has kf_mp_of_kp[k] == id   (MapPoint::IsInKeyFrame)
 *   3 BEHIND         Pc = (R_r0 Px + R_r1 Py + R_r2 Pz) + t_r  (f32, left to right, as spfe_proj_project);  Pc.z < 0
 *   4 OUTSIDE        invz = 1.0f / Pc.z;  x = Pc.x * invz, y = Pc.y * invz;  u = fx * x + cx, v = fy * y + cy  — Fuse's
 *                    operation order, NOT the frame's (fx * Pc.x) * invz + cx;  refused unless 0 <= u < W and 0 <= v < H
 *                    (the upper bound is strict, unlike Frame::isInFrustum's), written so that a NaN is refused
 *   5 RANGE          PO = P - Ow (f32; Ow = spfe_proj_cam's), dist3D = (float)sqrt(((double)POx POx + (double)POy POy) +
 *                    (double)POz POz)  — cv::norm of a CV_32F matrix accumulates in double —;
 *                    dist3D < min_factor * dmin or dist3D > max_factor * dmax  (f32 products: 0.8f, 1.2f)
 *   6 ANGLE          dot = ((double)POx nx + (double)POy ny) + (double)POz nz  — Mat::dot of CV_32F accumulates in double —;
 *                    dot < view_cos * (double)dist3D  (view_cos = 0.5, compared in double)
 *   7 NO_CANDIDATE   the window of radius th about (u, v): spfe_proj_window / spfe_proj_in_window, ix outer, iy inner;
 *                    a keypoint of the window is a candidate unless (double)(e2 * 1.0f) > chi2, e2 = ex ex + ey ey in f32,
 *                    ex = u - kx, ey = v - ky (the level's inverse sigma^2 is 1).  No candidate — an empty window, or every
 *                    keypoint of it refused by the gate — is this code; the reference leaves bestDist at 256 there.
 *                    The predicted level is always 0 and the level test always passes: the extractor has one level.
 *                    Monocular only: mvuRight is -1 throughout, the stereo branch is not provided.
 *   8 TOO_FAR        best = 256.0f; over the candidates in window order: dist < best takes over (strict: the first wins a
 *                    tie; a NaN distance never does); dist = spfe_proj_dist of spfe_proj_lane_sum and its butterfly;
 *                    best > th_dist (TH_LOW = 0.3f)
 *   9 PROPOSED       what the reference counts in nFused.  kp = the best keypoint, holder = kf_mp_of_kp[kp] ON ENTRY.
 *
 * Nothing is written into kf_mp_of_kp and no keypoint is ever blocked, so every point's result is a function of the
 * call's inputs alone; the host applies Replace / AddObservation in index order over the proposals (sp_matcher.cpp:1086-1099).
 *
 * Where the reference leaves a case undefined, this header defines it:
 *   Pc.z == 0     invz = +-inf.  Pc.z = -0.0f passes `Pc.z < 0` and gives -inf.  u is then +-inf or (Pc.x == 0) NaN: neither
 *                 satisfies 0 <= u < W, so the point is OUTSIDE.  (The reference's IsInImage refuses the same values.)
 *   dist3D == 0   the point sits on the camera centre.  Then Pc = R (P - Ow) is 0 up to rounding and the case above or
 *                 OUTSIDE usually decides first; where it does not, RANGE is evaluated as written (0 < 0.8 dmin refuses
 *                 for any dmin > 0) and ANGLE as written (dot = 0 < 0 is false: it passes).  No division by dist3D is made.
 *   PredictScale  ceil(log(dmax / dist3D) / mfLogScaleFactor) divides by log(1) = 0 in the reference: +-inf or NaN cast to
 *                 int, then clamped to [0, nLevels - 1] = [0, 0] — or, for the NaN's INT_MIN, to 0 as well.  Here the level
 *                 is 0 by definition and the expression is not evaluated.
 */
#ifndef SPFE_FUSE_MATH_H
#define SPFE_FUSE_MATH_H

#include "spfe_proj_math.h"

#define SPFE_FUSE_R_SKIP_BAD 1
#define SPFE_FUSE_R_SKIP_IN_KF 2
#define SPFE_FUSE_R_BEHIND 3
#define SPFE_FUSE_R_OUTSIDE 4
#define SPFE_FUSE_R_RANGE 5
#define SPFE_FUSE_R_ANGLE 6
#define SPFE_FUSE_R_NO_CANDIDATE 7
#define SPFE_FUSE_R_TOO_FAR 8
#define SPFE_FUSE_R_PROPOSED 9

typedef struct {
  float fx, fy, cx, cy, W, H;
  float min_factor, max_factor;
  double view_cos;
} spfe_fuse_view;

/* steps 3 - 6: 0 when the point goes on to the window search (*u, *v set), else its reason code */
SPFE_PM int spfe_fuse_project(const spfe_proj_cam *c, const spfe_fuse_view *p, const float P[3], const float nrm[3], float dmin,
                              float dmax, float *u, float *v) {
  float Pc[3];
  for (int r = 0; r < 3; ++r) Pc[r] = ((c->R[3 * r] * P[0] + c->R[3 * r + 1] * P[1]) + c->R[3 * r + 2] * P[2]) + c->t[r];
  if (Pc[2] < 0.0f) return SPFE_FUSE_R_BEHIND;
  const float invz = 1.0f / Pc[2];
  const float x = Pc[0] * invz, y = Pc[1] * invz;
  const float uu = p->fx * x + p->cx, vv = p->fy * y + p->cy;
  if (!(uu >= 0.0f && uu < p->W)) return SPFE_FUSE_R_OUTSIDE;
  if (!(vv >= 0.0f && vv < p->H)) return SPFE_FUSE_R_OUTSIDE;
  const float ox = P[0] - c->Ow[0], oy = P[1] - c->Ow[1], oz = P[2] - c->Ow[2];
  const float dist = (float)__builtin_sqrt(((double)ox * (double)ox + (double)oy * (double)oy) + (double)oz * (double)oz);
  if (dist < p->min_factor * dmin || dist > p->max_factor * dmax) return SPFE_FUSE_R_RANGE;
  const double dot = ((double)ox * (double)nrm[0] + (double)oy * (double)nrm[1]) + (double)oz * (double)nrm[2];
  if (dot < p->view_cos * (double)dist) return SPFE_FUSE_R_ANGLE;
  *u = uu;
  *v = vv;
  return 0;
}

/* step 7's gate on a keypoint of the window: 1 when it stays a candidate */
SPFE_PM int spfe_fuse_chi2_pass(float kx, float ky, float u, float v, double chi2) {
  const float ex = u - kx, ey = v - ky;
  const float e2 = ex * ex + ey * ey;
  return !((double)(e2 * 1.0f) > chi2);
}

SPFE_PM float spfe_fuse_best_init(void) { return 256.0f; }

#endif /* SPFE_FUSE_MATH_H */
