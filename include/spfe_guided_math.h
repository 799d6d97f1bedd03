/*
 * spfe_guided_math.h — the arithmetic of the loop closer's guided match between the current keyframe and a loop candidate
 * under a Sim3 hypothesis, shared by the GPU kernels (sp_orb_slam_amd/csrc/guided.hip) and the host C reference of the test
 * suite (tests/guided_ref/guided_ref.c) so that both evaluate the same sequence of IEEE operations (compile with
 * -ffp-contract=off).  The camera, the window, the lane sum and the distance are those of spfe_proj_math.h, the transform
 * (s, R, t) and its two 3x4 forms those of spfe_sim3_math.h §4 (spfe_sim3_T, spfe_sim3_forms), all unchanged: a transform
 * that comes out of the verify block is applied here with the very bits the RANSAC used.
 *
 * What it restates, in this project's own words:
 *   SPMatcher::SearchBySim3Override       orb_slam2/src/cv/sp_matcher_loop.cpp:7-220
 *   KeyFrame::GetFeaturesInArea, IsInImage orb_slam2/src/type/keyframe.cpp:1018-1060
 *   as LoopClosingVLAD::ComputeSim3 calls it   orb_slam2/src/loopclosing/loop_closer_vlad.cpp:418-432
 *
 * Keyframe 1 is the current keyframe, keyframe 2 the candidate: K1 / K2 keypoints with their occupancy grids and descriptor
 * rows, the poses Tcw1 / Tcw2 (row-major 4x4, f32) and kf1_mp_of_kp / kf2_mp_of_kp, the id of the map point a keypoint holds
 * — an index into the map arrays xyz [n][3], flags [n], dist_range [n][2] = (mfMinDistance, mfMaxDistance), desc [n][256] —
 * or -1.  T12 = (s, R, t) takes camera-2 coordinates to camera-1 coordinates.  seed12[k1] = k2 or -1 is what the caller
 * already holds for keypoint k1 (vpMapPointMatches: the RANSAC's inliers, loop_closer_vlad.cpp:418-423).
 *
 * The masks.  already1[k1] = seed12[k1] >= 0.  already2[k2] = some k1 < K1 has seed12[k1] == k2 (and k2 < K2).  The reference
 * marks keyframe 2's side through MapPoint::GetIndexInKeyFrame(pKF2) of the seeded point; here the seeded point is named BY
 * its keypoint of keyframe 2 — it was taken from keyframe 2's own holder array — so GetIndexInKeyFrame(pKF2) of it IS that
 * keypoint, by definition.
 *
 * Direction 1 -> 2, per keypoint i1 < K1 (direction 2 -> 1 is the mirror image: Xc2 = Tcw2 P, Xc1 = [sR | t] Xc2, the window
 * in keyframe 1, already2 for already1).  The first step that refuses is the keypoint's reason code:
 *
 *   1 NO_POINT       id = kf1_mp_of_kp[i1] is < 0 or >= n
 *   2 ALREADY        already1[i1]
 *   3 SKIP_BAD       flags[id] lacks SEARCHABLE (isBad())
 *   4 BEHIND         Xc1 = Tcw1 P (spfe_sim3_to_cam), Xc2 = T21 Xc1 with T21 the 3x4 form of spfe_sim3_forms, applied like a
 *                    pose: Xc2_r = ((A_r0 X_0 + A_r1 X_1) + A_r2 X_2) + A_r3, f32, left to right;  Xc2.z < 0
 *   5 OUTSIDE        invz = 1.0f / Xc2.z;  x = Xc2.x * invz, y = Xc2.y * invz;  u = fx * x + cx, v = fy * y + cy  (Fuse's order);
 *                    refused unless 0 <= u < W and 0 <= v < H, written so that a NaN is refused
 *   6 RANGE          dist3D = (float)sqrt(((double)X X + (double)Y Y) + (double)Z Z) of Xc2 — the CAMERA-frame vector after
 *                    the similarity, not P - Ow: with s != 1 the two differ by the scale —; cv::norm accumulates in double;
 *                    dist3D < min_factor * dmin or dist3D > max_factor * dmax  (f32 products)
 *   7 NO_CANDIDATE   the window of radius th about (u, v) (spfe_proj_window / spfe_proj_in_window, ix outer, iy inner) holds
 *                    no keypoint.  There is NO chi-square gate, no viewing-angle test and no level test (one pyramid level:
 *                    the predicted level is 0 and every keypoint's octave is 0).  Keypoints that are already matched or hold
 *                    no point stay candidates.
 *   8 TOO_FAR        best = FLT_MAX; over the window's keypoints in order: dist < best takes over (strict: the first wins a
 *                    tie; a NaN distance never does); dist = spfe_proj_dist of spfe_proj_lane_sum and its butterfly;
 *                    best > th_dist
 *   9 MATCHED        vnMatch1[i1] = the best keypoint
 *
 * Agreement.  matches12[i1] = k2 exactly when vnMatch1[i1] = k2 and vnMatch2[k2] = i1; otherwise matches12[i1] = seed12[i1].
 * n_found counts the agreements, n_total the non-negative entries of matches12 (what Optimizer::OptimizeSim3 receives),
 * n_seed the non-negative entries of seed12 below K1.  An agreement never overwrites a seed: a seeded i1 is ALREADY and has
 * no vnMatch1, a seeded k2 has no vnMatch2.
 *
 * th_dist.  The reference writes `bestDist <= 0.7` (a double literal) in direction 1 -> 2 and `bestDist <= TH_HIGH` (the
 * float 0.7f) in the other.  0.7f = 0.699999988079071044921875 is the largest f32 not above the double 0.7 (its successor,
 * 0.7f + 2^-24 = 0.700000047683715..., is above it), so for an f32 bestDist `(double)bestDist <= 0.7` and `bestDist <= 0.7f`
 * hold for exactly the same values: no f32 value separates the two, and both directions compare against th_dist = 0.7f.
 *
 * DEPARTURE.  The reference projects with pKF1's intrinsics in BOTH directions (:11-14).  Here each direction uses its
 * target's intrinsics: (fx2, fy2, cx2, cy2) into keyframe 2, (fx1, fy1, cx1, cy1) into keyframe 1.  For the one camera of a
 * monocular sequence the two are identical.
 *
 * Where the reference leaves a case undefined, this header defines it as spfe_fuse_math.h does: Xc.z == 0 gives invz = +-inf
 * and u, v = +-inf or NaN, which is OUTSIDE; -0.0f passes the depth test and is OUTSIDE likewise.  A NaN transform (a
 * degenerate hypothesis) makes every projection NaN: BEHIND is false, OUTSIDE refuses.
 *
 * ---- (b) Loop-point projection --------------------------------------------------------------------------------------------
 * What it restates:  SPMatcher::SearchByProjectionLoop   orb_slam2/src/cv/sp_matcher_loop.cpp:222-332, as ComputeSim3 calls it
 * behind the accepted candidate (loop_closer_vlad.cpp:470-473).  One keyframe record, the similarity Scw (row-major 4x4, f32:
 * [s R | s t]), a LIST of map points as the fuse search takes it (point_id >= 0, xyz, normal, dist_range, desc, flags) and
 * matched[k], in/out: the id keypoint k holds or -1 (mvpCurrentMatchedPoints).
 *
 * The camera of Scw (spfe_loop_cam_from_scw), each operation defined once:
 *   scw = sqrt(((double)S00 S00 + (double)S01 S01) + (double)S02 S02)   (row 0's dot product accumulated in double)
 *   inv = 1.0 / scw (double);  Rcw_rc = (float)((double)S_rc * inv);  tcw_r = (float)((double)S_r3 * inv)
 *   Ow = -(R_0c t0 + R_1c t1 + R_2c t2) in f32, as spfe_proj_cam_from_f32 forms it.
 *
 * Per point i, in list order; the first step that refuses is its reason code:
 *   1 SKIP_BAD        the point is not SEARCHABLE
 *   2 ALREADY_FOUND   its id occurs in matched[0 .. K) ON ENTRY (spAlreadyFound is built once, before the loop)
 *   3 BEHIND  4 OUTSIDE  5 RANGE  6 ANGLE   exactly spfe_fuse_project on that camera (spfe_fuse_math.h steps 3 - 6)
 *   7 NO_CANDIDATE    the window of radius th (10) about (u, v) holds no keypoint at all (taken or not)
 *   8 TOO_FAR         best = 256.0f; over the window's keypoints in order WHOSE matched ENTRY IS -1 AT THAT MOMENT: dist < best
 *                     takes over (strict; a NaN never wins);  best > th_dist (0.7f) — which also covers "every keypoint of
 *                     the window is taken"
 *   9 MATCHED         matched[best] = id: that keypoint is blocked for every later point
 * The result is that of this sequential loop.  The kernels reach it as the fixed point of proj_resolve_kernel's ordered claim
 * (proj.hip): each round every unfinished point posts its index on its unblocked candidates, and a point that finds itself on
 * all of them is final.  That gives the sequential result because (1) every holder blocks — a keypoint whose entry is not -1
 * is never a candidate again, whoever holds it —, (2) an accepted point always blocks its keypoint, so a later point can
 * never undo an earlier point's choice, and (3) a refused point takes nothing, so it changes what no other point sees.  The
 * lowest unfinished index is always final: n points need at most n rounds.  A keypoint that only a LATER-indexed point wants
 * is free for the earlier one.
 * Lists beyond the capacity go in chunks with `matched` carried from call to call.  That is exact: the ids of a list are
 * unique, so rebuilding "already found" between chunks adds only ids that earlier chunks wrote — ids that do not occur again.
 * (A list that repeats an id is served as written: the second occurrence is ALREADY_FOUND only if the id was there on entry
 * of ITS call.)
 */
#ifndef SPFE_GUIDED_MATH_H
#define SPFE_GUIDED_MATH_H

#include "spfe_fuse_math.h"
#include "spfe_sim3_math.h"

#define SPFE_GUIDED_R_NO_POINT 1
#define SPFE_GUIDED_R_ALREADY 2
#define SPFE_GUIDED_R_SKIP_BAD 3
#define SPFE_GUIDED_R_BEHIND 4
#define SPFE_GUIDED_R_OUTSIDE 5
#define SPFE_GUIDED_R_RANGE 6
#define SPFE_GUIDED_R_NO_CANDIDATE 7
#define SPFE_GUIDED_R_TOO_FAR 8
#define SPFE_GUIDED_R_MATCHED 9

typedef struct {
  float fx, fy, cx, cy, W, H; /* the TARGET keyframe's intrinsics and frame */
  float min_factor, max_factor;
} spfe_guided_view;

/* T12 as stored by the verify block (s, R[9], t[3]) */
SPFE_PM void spfe_guided_T_from_f32(const float T[13], spfe_sim3_T *out) {
  out->s = T[0];
  for (int i = 0; i < 9; ++i) out->R[i] = T[1 + i];
  for (int i = 0; i < 3; ++i) out->t[i] = T[10 + i];
}

/* steps 4 - 6 of one direction: Tcw the SOURCE keyframe's pose, A the 3x4 form that takes its camera frame to the target's
 * (T21 for 1 -> 2, T12 for 2 -> 1).  0 when the point goes on to the window search (*u, *v set), else its reason code */
SPFE_PM int spfe_guided_project(const float Tcw[16], const float A[12], const spfe_guided_view *p, const float P[3], float dmin,
                                float dmax, float *u, float *v) {
  float Xs[3], Xt[3];
  spfe_sim3_to_cam(Tcw, P, Xs);
  for (int r = 0; r < 3; ++r) Xt[r] = ((A[4 * r] * Xs[0] + A[4 * r + 1] * Xs[1]) + A[4 * r + 2] * Xs[2]) + A[4 * r + 3];
  if (Xt[2] < 0.0f) return SPFE_GUIDED_R_BEHIND;
  const float invz = 1.0f / Xt[2];
  const float x = Xt[0] * invz, y = Xt[1] * invz;
  const float uu = p->fx * x + p->cx, vv = p->fy * y + p->cy;
  if (!(uu >= 0.0f && uu < p->W)) return SPFE_GUIDED_R_OUTSIDE;
  if (!(vv >= 0.0f && vv < p->H)) return SPFE_GUIDED_R_OUTSIDE;
  const float dist =
      (float)__builtin_sqrt(((double)Xt[0] * (double)Xt[0] + (double)Xt[1] * (double)Xt[1]) + (double)Xt[2] * (double)Xt[2]);
  if (dist < p->min_factor * dmin || dist > p->max_factor * dmax) return SPFE_GUIDED_R_RANGE;
  *u = uu;
  *v = vv;
  return 0;
}

SPFE_PM float spfe_guided_best_init(void) { return 3.402823466e+38f; }

/* the agreement of i1: the entry of matches12 (found is set to 1 on an agreement).  k2 = vnMatch1[i1] (-1: none),
 * back = vnMatch2[k2] (read only when 0 <= k2 < K2), seed = seed12[i1] */
SPFE_PM int spfe_guided_agree(int i1, int k2, int back, int seed, int *found) {
  *found = k2 >= 0 && back == i1;
  return *found ? k2 : seed;
}

/* ---- (b) loop-point projection ---- */
#define SPFE_LOOPPROJ_R_SKIP_BAD 1
#define SPFE_LOOPPROJ_R_ALREADY_FOUND 2
#define SPFE_LOOPPROJ_R_BEHIND 3
#define SPFE_LOOPPROJ_R_OUTSIDE 4
#define SPFE_LOOPPROJ_R_RANGE 5
#define SPFE_LOOPPROJ_R_ANGLE 6
#define SPFE_LOOPPROJ_R_NO_CANDIDATE 7
#define SPFE_LOOPPROJ_R_TOO_FAR 8
#define SPFE_LOOPPROJ_R_MATCHED 9

SPFE_PM void spfe_loop_cam_from_scw(const float Scw[16], spfe_proj_cam *c) {
  const double s2 = ((double)Scw[0] * (double)Scw[0] + (double)Scw[1] * (double)Scw[1]) + (double)Scw[2] * (double)Scw[2];
  const double inv = 1.0 / __builtin_sqrt(s2);
  float T[16];
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 4; ++k) T[4 * r + k] = (float)((double)Scw[4 * r + k] * inv);
  T[12] = T[13] = T[14] = 0.0f;
  T[15] = 1.0f;
  spfe_proj_cam_from_f32(T, c);
}

SPFE_PM float spfe_loopproj_best_init(void) { return 256.0f; }

#endif /* SPFE_GUIDED_MATH_H */
