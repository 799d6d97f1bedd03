/*
 * spfe_mappoint_math.h — the arithmetic of a map point's refresh (its distinctive descriptor, its mean viewing direction and
 * its distance range), shared by the GPU kernels (sp_orb_slam_amd/csrc/mappoint.hip) and the host C reference of the test suite
 * (tests/mp_ref/mp_ref.c) so that both evaluate the same sequence of IEEE operations (compile with -ffp-contract=off).  The
 * camera centre of a pose, the lane sum and the distance are those of spfe_proj_math.h, unchanged.
 *
 * What it restates, in this project's own words:
 *   MapPoint::ComputeDistinctiveDescriptors()   orb_slam2/src/type/mappoint.cpp:237-302
 *   MapPoint::UpdateNormalAndDepth()            orb_slam2/src/type/mappoint.cpp:322-364
 *   as the mapper, the optimiser, the loop closer and the initialiser call them behind every step that changes a point's
 *   observations or position (local_mapper.cpp:264-265, :524-528, :779-783, :892-900; optimizer.cpp:222, :772, :1058;
 *   loop_closer_vlad.cpp:605, :635; mono_tracker.cpp:149-152).
 *
 * A point p has observations o = 0 .. N_all - 1, each (keyframe slot, keypoint), in the order the CALLER gives: the order in
 * which the reference iterates mObservations, a std::map<KeyFrame *, size_t> — pointer order, which only the host knows.
 *
 * ---- (a) The distinctive descriptor -----------------------------------------------------------------------------------------
 * The GOOD observations are those whose keyframe is not bad (:259); in the given order they are the rows vDescriptors[0 .. N).
 *   D[i][j]   = spfe_proj_dist of the butterfly of spfe_proj_lane_sum of rows i and j: the distance of every search here
 *               (spfe_proj_math.h:37-39); bf16 rows are widened exactly first.  D[i][i] = 0 whatever the row holds (:273).
 *               (a - b)^2 == (b - a)^2 exactly and the sums are the same sums, so D is symmetric bit for bit: an implementation
 *               may compute a pair once or twice.
 *   median_i  = the element of rank k = (size_t)(0.5 * (N - 1)) — the floor — in the ascending order of row i, the self-distance
 *               0 included (:286-289).  The k-th smallest of a multiset is a value, not a position: selection by counting
 *               (spfe_mp_is_rank) gives what the sort gives.  Where a row holds a NaN std::sort is undefined in the reference;
 *               HERE a NaN ranks above every number, +inf included, and all NaNs rank equal.
 *   BestMedian = FLT_MAX, BestIdx = 0; for i ascending median_i < BestMedian takes over (:283-295).  Strict: the first wins a tie;
 *               a NaN or +inf median never wins, and where none wins row 0 stays.
 *   The point's descriptor becomes row BestIdx, as f32 (:300).
 *   The small cases follow from the rule:
 *     N = 1   k = 0   row 0
 *     N = 2   k = 0   both medians are the self-distance 0: row 0
 *     N = 3   k = 1   each row's median is the smaller of its two distances to the others
 *     N = 4   k = 1   each row's median is the smallest of its three distances to the others (rank 1, behind the 0)
 *
 * ---- (b) Normal and depth -------------------------------------------------------------------------------------------------
 * Over ALL observations: the reference does not skip bad keyframes here (:342-350).  P is the point's f32 position.
 *   Ow_i   = the keyframe's camera centre as spfe_proj_cam_from_f32 forms it from the f32 pose, unchanged
 *   d      = P - Ow_i, element-wise in f32
 *   nd     = sqrt(((double)dx^2 + (double)dy^2) + (double)dz^2)           cv::norm of a CV_32F vector
 *   w      = (float)(1.0 / nd)
 *   normal += d * w, element-wise in f32, in observation order, from +0
 *   normal_out = normal * (float)(1.0 / (double)n), n = N_all
 *   dist   = (float)nd against the REFERENCE keyframe's centre (ref_slot: mpRefKF)
 *   max    = dist * level_scale,  min = max / top_scale   (mvScaleFactors[level], mvScaleFactors[nLevels - 1]: both 1 with this
 *            extractor's single pyramid level; the formula is kept)
 * This DEFINES `Mat / double` and cv::norm here: OpenCV evaluates Mat / s of a CV_32F matrix as a scale by 1 / s narrowed to f32;
 * its kernel is not pinned.  nd == 0 gives inf / NaN by IEEE, as in the reference.
 *
 * ---- (c) Codes ------------------------------------------------------------------------------------------------------------
 * One per listed point; the first that applies:
 *   1 SKIP_BAD     the point's flags lack SPFE_PROJ_POINT_SEARCHABLE (mbBad, :244, :329)                  nothing written
 *   2 NO_OBS       N_all == 0 (:249, :337)                                                               nothing written
 *   3 INVALID      an index that cannot be followed (see spfe.h)                                         nothing written
 *   4 NO_GOOD_KF   N == 0 (:263)                                        descriptor kept, normal / depth written
 *   5 TOO_MANY     N > SPFE_MP_MAX_OBS: the host refreshes this one     descriptor kept, normal / depth written
 *   6 REFRESHED    descriptor and normal / depth
 * mode is a bit set; a part that is not asked for is not written, and codes 4 and 5 belong to the descriptor: without
 * SPFE_MP_DESC a point that passes 1 - 3 is REFRESHED.
 */
#ifndef SPFE_MAPPOINT_MATH_H
#define SPFE_MAPPOINT_MATH_H

#include "spfe_proj_math.h"

#define SPFE_MP_MAX_OBS 256
#define SPFE_MP_DESC 1
#define SPFE_MP_NORMAL_DEPTH 2
#define SPFE_MP_R_SKIP_BAD 1
#define SPFE_MP_R_NO_OBS 2
#define SPFE_MP_R_INVALID 3
#define SPFE_MP_R_NO_GOOD_KF 4
#define SPFE_MP_R_TOO_MANY 5
#define SPFE_MP_R_REFRESHED 6

/* ---- (a) ---- */
SPFE_PM int spfe_mp_median_rank(int N) { return (int)(0.5 * (double)(N - 1)); }
SPFE_PM float spfe_mp_best_init(void) { return 3.402823466e+38f; }
/* the order of a row: numbers ascending, every NaN above them */
SPFE_PM int spfe_mp_before(float a, float b) { return a == a && (b != b || a < b); }
SPFE_PM int spfe_mp_same(float a, float b) { return a == b || (a != a && b != b); }
/* v, an element of a row with n_before elements before it and n_same equal to it (itself included), is the element of rank k */
SPFE_PM int spfe_mp_is_rank(int n_before, int n_same, int k) { return n_before <= k && k < n_before + n_same; }
SPFE_PM int spfe_mp_takes_over(float median, float best) { return median < best; }

/* the code behind steps 1 - 3, from the number of good rows */
SPFE_PM int spfe_mp_code(int mode, int n_good) {
  if (!(mode & SPFE_MP_DESC)) return SPFE_MP_R_REFRESHED;
  if (n_good == 0) return SPFE_MP_R_NO_GOOD_KF;
  if (n_good > SPFE_MP_MAX_OBS) return SPFE_MP_R_TOO_MANY;
  return SPFE_MP_R_REFRESHED;
}

/* ---- (b) ---- */
/* d = P - Ow and its norm */
SPFE_PM double spfe_mp_offset(const float P[3], const float Ow[3], float d[3]) {
  d[0] = P[0] - Ow[0];
  d[1] = P[1] - Ow[1];
  d[2] = P[2] - Ow[2];
  return __builtin_sqrt(((double)d[0] * (double)d[0] + (double)d[1] * (double)d[1]) + (double)d[2] * (double)d[2]);
}
/* one observation's share of the normal: c = d * w */
SPFE_PM void spfe_mp_share(const float P[3], const float Ow[3], float c[3]) {
  float d[3];
  const double nd = spfe_mp_offset(P, Ow, d);
  const float w = (float)(1.0 / nd);
  c[0] = d[0] * w;
  c[1] = d[1] * w;
  c[2] = d[2] * w;
}
SPFE_PM void spfe_mp_normal_out(const float sum[3], int n, float out[3]) {
  const float s = (float)(1.0 / (double)n);
  out[0] = sum[0] * s;
  out[1] = sum[1] * s;
  out[2] = sum[2] * s;
}
/* range[0] = mfMinDistance, range[1] = mfMaxDistance */
SPFE_PM void spfe_mp_range(const float P[3], const float Ow_ref[3], float level_scale, float top_scale, float range[2]) {
  float d[3];
  const float dist = (float)spfe_mp_offset(P, Ow_ref, d);
  range[1] = dist * level_scale;
  range[0] = range[1] / top_scale;
}

#endif /* SPFE_MAPPOINT_MATH_H */
