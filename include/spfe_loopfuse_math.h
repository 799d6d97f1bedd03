/*
 * spfe_loopfuse_math.h — the arithmetic of the loop closer's fusion step, shared by the GPU kernels
 * (sp_orb_slam_amd/csrc/loopfuse.hip) and the host C reference of the test suite (tests/loopfuse_ref/loopfuse_ref.c) so that
 * both evaluate the same sequence of IEEE operations (compile with -ffp-contract=off).  The camera of a pose, the window, the
 * lane sum and the distance are those of spfe_proj_math.h, the gates behind the projection those of spfe_fuse_math.h
 * (spfe_fuse_project), the camera of a similarity that of spfe_guided_math.h (spfe_loop_cam_from_scw), the double Sim3 and its
 * narrowing those of spfe_sim3opt_math.h — all unchanged.
 *
 * What it restates, in this project's own words:
 *   SPMatcher::Fuse(KeyFrame *, cv::Mat Scw, const vector<MapPoint *> &, th, vpReplacePoint)   orb_slam2/src/cv/sp_matcher.cpp:1106-1219
 *   KeyFrame::GetFeaturesInArea, KeyFrame::IsInImage                                           orb_slam2/src/type/keyframe.cpp:1018-1060
 *   as LoopClosingVLAD::SearchAndFuse calls it                          orb_slam2/src/loopclosing/loop_closer_vlad.cpp:701-726
 *   the corrected poses of LoopClosingVLAD::CorrectLoop                 loop_closer_vlad.cpp:536-571, :608-618
 *
 * ---- (a) The search -------------------------------------------------------------------------------------------------------
 * One target keyframe: K keypoints with their occupancy grid and descriptor rows, kf_mp_of_kp[k] (the id of the map point
 * keypoint k holds, or -1) and the similarity Scw (row-major 4x4, f32, [s R | t]: what Converter::toCvMat(g2o::Sim3) gives).
 * The point LIST of the fuse search: point_id >= 0, xyz, normal (not normalised), dist_range = (mfMinDistance,
 * mfMaxDistance), desc, flags (SEARCHABLE = !isBad()).  Per point; the first step that refuses is its reason code:
 *
 *   1 SKIP_BAD       the point is not SEARCHABLE
 *   2 SKIP_IN_KF     its id occurs in kf_mp_of_kp[0 .. K) ON ENTRY.  The reference's spAlreadyFound = pKF->GetMapPoints() is
 *                    built once, before the loop (:1123); GetMapPoints leaves out bad points, which step 1 has refused already.
 *   3 BEHIND  4 OUTSIDE  5 RANGE  6 ANGLE     exactly spfe_fuse_project (spfe_fuse_math.h steps 3 - 6) on the camera
 *                    spfe_loop_cam_from_scw(Scw): the norm of row 0 of the 3x3 block is accumulated in double, and R AND t are
 *                    both divided by it (:1117-1119) — the search ignores the scale of the similarity.
 *                    invz.  The reference writes `const float invz = 1.0 / p3Dc.at<float>(2)` (:1148): the double quotient
 *                    1.0 / (double)z narrowed to f32.  That IS the f32 division 1.0f / z: the double quotient of two f32
 *                    values carries 53 bits, more than 2 * 24 + 2, and rounding a quotient of two p-bit values first to 2p + 2
 *                    bits or more and then to p bits gives the correctly rounded p-bit quotient (double rounding is innocuous
 *                    for division at that width).  So spfe_fuse_project's 1.0f / Pc.z has the reference's bits.
 *   7 NO_CANDIDATE   the window of radius th (4) about (u, v) (spfe_proj_window / spfe_proj_in_window, ix outer, iy inner)
 *                    holds no keypoint.  There is NO chi-square gate: every keypoint of the window is a candidate.  The
 *                    predicted level is 0 and the level test always passes (one pyramid level); monocular only.
 *   8 TOO_FAR        best = FLT_MAX; over the candidates in window order: dist < best takes over (strict: the first wins a
 *                    tie; a NaN distance never does; neither does +inf); dist = spfe_proj_dist of spfe_proj_lane_sum and its
 *                    butterfly.  Refused when best > th_dist (TH_HIGH = 0.7f) — and when no candidate ever took over, whatever
 *                    th_dist is: a window whose distances are all NaN is THIS code, not 7 (the reference leaves bestIdx at
 *                    -1 there and bestDist at FLT_MAX, which TH_HIGH refuses).
 *   9 PROPOSED       what the reference counts in nFused.  kp = the best keypoint, its distance, holder = kf_mp_of_kp[kp] ON
 *                    ENTRY.
 *
 * Nothing is written into kf_mp_of_kp and no keypoint is ever blocked, so every point's result is a function of the call's
 * inputs alone and the targets are independent.  What Fuse and SearchAndFuse do with a find (AddObservation / AddMapPoint on
 * the live keyframe inside Fuse, pRep->Replace(loopMP) behind it) needs the observation graph and stays with the host, which
 * walks fused_idx in order (tests/loopfuse_ref/loopfuse_walk.py is the recipe).
 * A NaN Scw makes every projection NaN: BEHIND is false, OUTSIDE refuses.  Pc.z == 0, dist3D == 0 and PredictScale are
 * defined as spfe_fuse_math.h defines them.
 *
 * ---- (b) The corrected poses ----------------------------------------------------------------------------------------------
 * Inputs: S12 (double[13] = s, R row-major, t: as the optimise block stores it), Tcw2 (the matched keyframe's f32 pose), Twc
 * (the current keyframe's f32 GetPoseInverse()), Tiw (a connected keyframe's f32 pose), and whether that keyframe IS the
 * current one.  Only + - * / sqrt occur, so that the GPU and the host give the same bits.
 *   1  Scw, a double similarity: the product spfe_s3o_scw forms before it narrows, Sim3(S12) * Sim3(quat(Rcw2), tcw2, 1)
 *      (spfe_s3o_scw_sim) — mg2oScw (:438-441).
 *   2  Tic = Tiw * Twc (:555), entry by entry: Tic_rc = (float)(((p0 + p1) + p2) + p3), p_k = (double)Tiw_rk * (double)Twc_kc,
 *      k ascending, all four k (the last row of Twc takes part as it stands).  This DEFINES the CV_32F matrix product here
 *      (OpenCV's gemm accumulates CV_32F products in double and narrows once; its blocking is not pinned).
 *   3  Sic = Sim3(spfe_quat_from_rot((double)Ric), (double)tic, 1)                                             (:556-559)
 *   4  P = Sic * Scw with spfe_s3o_mul                                                                         (:560)
 *      For the entry that is the current keyframe P = Scw itself, no product                                   (:540)
 *   5  Siw           f32[16] = [P.s * R(P.q) | P.t; 0 0 0 1]: the cvScw SearchAndFuse hands to Fuse (:710) — spfe_s3o_sim_to_f32
 *      Tiw_corrected f32[16] = [R(P.q) | P.t * (1.0 / P.s); 0 0 0 1]: correctedTiw (:610-616)
 *      both narrowed entry by entry with every NaN replaced by the quiet NaN, as spfe_s3o_scw narrows.
 */
#ifndef SPFE_LOOPFUSE_MATH_H
#define SPFE_LOOPFUSE_MATH_H

#include "spfe_proj_math.h"
#include "spfe_fuse_math.h"
#include "spfe_guided_math.h"
#include "spfe_sim3opt_math.h"

/* the reason codes ARE the fuse search's */
#define SPFE_LOOPFUSE_R_SKIP_BAD SPFE_FUSE_R_SKIP_BAD
#define SPFE_LOOPFUSE_R_SKIP_IN_KF SPFE_FUSE_R_SKIP_IN_KF
#define SPFE_LOOPFUSE_R_BEHIND SPFE_FUSE_R_BEHIND
#define SPFE_LOOPFUSE_R_OUTSIDE SPFE_FUSE_R_OUTSIDE
#define SPFE_LOOPFUSE_R_RANGE SPFE_FUSE_R_RANGE
#define SPFE_LOOPFUSE_R_ANGLE SPFE_FUSE_R_ANGLE
#define SPFE_LOOPFUSE_R_NO_CANDIDATE SPFE_FUSE_R_NO_CANDIDATE
#define SPFE_LOOPFUSE_R_TOO_FAR SPFE_FUSE_R_TOO_FAR
#define SPFE_LOOPFUSE_R_PROPOSED SPFE_FUSE_R_PROPOSED

/* ---- (a) ---- */
SPFE_PM float spfe_loopfuse_best_init(void) { return 3.402823466e+38f; }

/* steps 7 - 9 behind the window: any = the window held a keypoint, best_k = the keypoint that took over last (-1: none did) */
SPFE_PM int spfe_loopfuse_verdict(int any, int best_k, float best, float th_dist) {
  if (!any) return SPFE_LOOPFUSE_R_NO_CANDIDATE;
  if (best_k < 0 || best > th_dist) return SPFE_LOOPFUSE_R_TOO_FAR;
  return SPFE_LOOPFUSE_R_PROPOSED;
}

/* ---- (b) ---- */
/* step 2: rows 0 - 2 of the CV_32F product Tiw * Twc, row-major 3x4 */
SPFE_DM void spfe_loopfuse_tic(const float Tiw[16], const float Twc[16], float Tic[12]) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) {
      double s = (double)Tiw[4 * r] * (double)Twc[c];
      s = s + (double)Tiw[4 * r + 1] * (double)Twc[4 + c];
      s = s + (double)Tiw[4 * r + 2] * (double)Twc[8 + c];
      s = s + (double)Tiw[4 * r + 3] * (double)Twc[12 + c];
      Tic[4 * r + c] = (float)s;
    }
}

/* step 5, the second output: [R(P.q) | P.t / P.s] */
SPFE_DM void spfe_loopfuse_se3_to_f32(const spfe_s3o_sim *P, float T[16]) {
  double R[9];
  spfe_quat_to_rot(P->q, R);
  const double inv = 1.0 / P->s;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T[r * 4 + c] = spfe_s3o_canonf((float)R[r * 3 + c]);
    T[r * 4 + 3] = spfe_s3o_canonf((float)(P->t[r] * inv));
  }
  T[12] = T[13] = T[14] = 0.0f;
  T[15] = 1.0f;
}

/* steps 1 - 5 for one connected keyframe */
SPFE_DM void spfe_loopfuse_pose(const double S12[13], const float Tcw2[16], const float Twc[16], const float Tiw[16],
                                int is_current, float Siw[16], float Tiw_corrected[16]) {
  spfe_s3o_sim Scw, P;
  spfe_s3o_scw_sim(S12, Tcw2, &Scw);
  if (is_current) {
    P = Scw;
  } else {
    spfe_s3o_sim Sic;
    float Tic[12];
    double Ric[9];
    spfe_loopfuse_tic(Tiw, Twc, Tic);
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) Ric[3 * r + c] = (double)Tic[4 * r + c];
      Sic.t[r] = (double)Tic[4 * r + 3];
    }
    spfe_quat_from_rot(Ric, Sic.q);
    Sic.s = 1.0;
    spfe_s3o_mul(&Sic, &Scw, &P);
  }
  spfe_s3o_sim_to_f32(&P, Siw);
  spfe_loopfuse_se3_to_f32(&P, Tiw_corrected);
}

#endif /* SPFE_LOOPFUSE_MATH_H */
