/*
 * spfe_proj_math.h — the arithmetic of the window search by projection, shared by the GPU kernels
 * (sp_orb_slam_amd/csrc/proj.hip) and the host C reference of the test suite (tests/proj_ref/proj_ref.c) so that both
 * evaluate the same sequence of IEEE operations (compile with -ffp-contract=off).
 *
 * What it restates, in this project's own words:
 *   Frame::isInFrustum                               orb_slam2/src/type/frame.cpp:330-380
 *   Frame::GetFeaturesInArea                         orb_slam2/src/type/frame.cpp:382-420
 *   SPMatcher::SearchByProjection(F, points, th, d)  orb_slam2/src/cv/sp_matcher.cpp:344-432   SPFE_PROJ_LOCAL_MAP
 *   SPMatcher::SearchByProjection(Cur, Last, th, 1)  orb_slam2/src/cv/sp_matcher.cpp:1439-1543 SPFE_PROJ_LAST_FRAME
 *   Tracking::SearchLocalPoints                      orb_slam2/src/tracking/tracker.cpp:768-832
 *
 * Projection of map point P with unit normal n under Tcw = [Rcw | tcw] (row-major 4x4), all in f32, every sum left to right:
 *   Pc   = (R_r0 Px + R_r1 Py + R_r2 Pz) + t_r                       LOCAL_MAP rejects Pc.z < 0
 *   invz = 1.0f / Pc.z                                               LAST_FRAME: (float)(1.0 / (double)Pc.z), rejects invz < 0
 *   u    = (fx * Pc.x) * invz + cx,  v = (fy * Pc.y) * invz + cy     rejected unless 0 <= u <= W and 0 <= v <= H
 *                                                                    (mnMinX .. mnMaxY of an undistorted frame; written so
 *                                                                    that a NaN projection — Pc.z == 0 — is rejected, where
 *                                                                    the reference goes on to index with it)
 *   LOCAL_MAP only:
 *   Ow   = -(R_0c t0 + R_1c t1 + R_2c t2)                            the camera centre, -Rcw^T tcw
 *   PO   = P - Ow,  dist = sqrtf(POx POx + POy POy + POz POz),  viewCos = (POx nx + POy ny + POz nz) / dist
 *                                                                    rejected when viewCos < view_cos_limit (a NaN passes, as
 *                                                                    in the reference: dist == 0)
 *   The distance-range test is commented out in the reference and is not made.  The predicted scale level is always 0: the
 *   extractor has one pyramid level, every scale factor is 1 and tracking::scale_check selects nothing.
 *
 * Radius:  LOCAL_MAP  r = ((double)viewCos > 0.998 ? 2.5f : 4.0f), times th when th != 1;   LAST_FRAME  r = th.
 *
 * Window of radius r about (u, v) on the 8-pixel occupancy grid (wc x hc cells, one keypoint per cell):
 *   ix from max(0, (int)floorf((u - r) / 8)) to min(wc - 1, (int)ceilf((u + r) / 8)), iy likewise with v and hc;
 *   ix is the OUTER loop, iy the inner one — the candidates keep this order, and ties go to the first;
 *   cell (ix, iy) contributes k = occ_grid[iy][ix] when k != -1, k < K, |kp.x - u| < r and |kp.y - v| < r.
 *   2 r / 8 cells and one more at either end: at most SPFE_PROJ_MAX_CELLS_AXIS per axis at the largest radius (one further
 *   cell is allowed for the rounding of the two f32 quotients).
 *
 * Distance: (float) cv::norm(a, b, NORM_L2) — squared differences of the f32 elements accumulated in double, in the order of
 * the patch association (match.hip): lane l of 64 adds dimensions 4l .. 4l+3 in order, then the butterfly
 * s_l += s_(l ^ m), m = 32, 16, 8, 4, 2, 1; dist = (float)sqrt(s).  bf16 descriptor rows are widened exactly first.
 *
 * Choice and acceptance, per map point in index order:
 *   best = 256.0f (LOCAL_MAP) or FLT_MAX (LAST_FRAME); over the window's keypoints in order, skipping the blocked ones:
 *   dist < best takes over (strict: the first wins a tie; a NaN distance never does).
 *   A keypoint is blocked while it holds a map point whose OBSERVED flag is set.
 *   Where every candidate is blocked the reference indexes with bestIdx = -1; here that case is "no match".
 *   LOCAL_MAP  accept when best <= th_dist, else when best < thr, thr = adaptive ? (1.2f * c2) / (c2 + duv) : 0.7f,
 *              duv = du du + dv dv the squared pixel offset of that keypoint from (u, v).
 *   LAST_FRAME accept when best <= 0.7f.
 *   A point whose best candidate is refused takes nothing (no second best).  An accepted point writes itself into
 *   mp_of_kp[best]; that overwrites an unobserved holder, so the last writer wins.
 */
#ifndef SPFE_PROJ_MATH_H
#define SPFE_PROJ_MATH_H

#if defined(__HIPCC__)
#define SPFE_PM __host__ __device__ static inline
#else
#define SPFE_PM static inline
#endif

#define SPFE_PROJ_MODE_LOCAL_MAP 0
#define SPFE_PROJ_MODE_LAST_FRAME 1
#define SPFE_PROJ_CELL 8.0f
#define SPFE_PROJ_POINT_SEARCHABLE 1u /* !isBad() */
#define SPFE_PROJ_POINT_OBSERVED 2u   /* Observations() > 0 */

typedef struct {
  float R[9], t[3]; /* Rcw row-major, tcw */
  float Ow[3];      /* camera centre */
} spfe_proj_cam;

SPFE_PM void spfe_proj_cam_from_f32(const float Tcw[16], spfe_proj_cam *c) {
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) c->R[3 * r + k] = Tcw[4 * r + k];
    c->t[r] = Tcw[4 * r + 3];
  }
  for (int k = 0; k < 3; ++k) c->Ow[k] = -((c->R[k] * c->t[0] + c->R[3 + k] * c->t[1]) + c->R[6 + k] * c->t[2]);
}

/* 1 when the point is in view; *u, *v, *view_cos are then set (view_cos = 0 in LAST_FRAME mode) */
SPFE_PM int spfe_proj_project(const spfe_proj_cam *c, const float P[3], const float nrm[3], float fx, float fy, float cx,
                              float cy, float W, float H, int mode, float view_cos_limit, float *u, float *v,
                              float *view_cos) {
  float Pc[3];
  for (int r = 0; r < 3; ++r) Pc[r] = ((c->R[3 * r] * P[0] + c->R[3 * r + 1] * P[1]) + c->R[3 * r + 2] * P[2]) + c->t[r];
  float invz;
  if (mode == SPFE_PROJ_MODE_LOCAL_MAP) {
    if (Pc[2] < 0.0f) return 0;
    invz = 1.0f / Pc[2];
  } else {
    invz = (float)(1.0 / (double)Pc[2]);
    if (invz < 0) return 0;
  }
  const float uu = (fx * Pc[0]) * invz + cx, vv = (fy * Pc[1]) * invz + cy;
  if (!(uu >= 0.0f && uu <= W)) return 0;
  if (!(vv >= 0.0f && vv <= H)) return 0;
  float vc = 0.0f;
  if (mode == SPFE_PROJ_MODE_LOCAL_MAP) {
    const float x = P[0] - c->Ow[0], y = P[1] - c->Ow[1], z = P[2] - c->Ow[2];
    const float dist = __builtin_sqrtf((x * x + y * y) + z * z);
    vc = ((x * nrm[0] + y * nrm[1]) + z * nrm[2]) / dist;
    if (vc < view_cos_limit) return 0;
  }
  *u = uu;
  *v = vv;
  *view_cos = vc;
  return 1;
}

SPFE_PM float spfe_proj_radius(int mode, float view_cos, float th) {
  if (mode != SPFE_PROJ_MODE_LOCAL_MAP) return th;
  float r = (double)view_cos > 0.998 ? 2.5f : 4.0f;
  if (th != 1.0f) r *= th;
  return r;
}

/* the largest radius a call with these parameters can use (the capacity check of the entry points) */
SPFE_PM float spfe_proj_max_radius(int mode, float th) {
  if (mode != SPFE_PROJ_MODE_LOCAL_MAP) return th;
  return th != 1.0f ? 4.0f * th : 4.0f;
}

/* cells lo .. hi (inclusive; empty when lo > hi) of one axis with `cells` cells */
SPFE_PM void spfe_proj_window(float x, float r, int cells, int *lo, int *hi) {
  const int a = (int)__builtin_floorf((x - r) / SPFE_PROJ_CELL), b = (int)__builtin_ceilf((x + r) / SPFE_PROJ_CELL);
  *lo = a > 0 ? a : 0;
  *hi = b < cells - 1 ? b : cells - 1;
}

SPFE_PM int spfe_proj_in_window(float kx, float ky, float u, float v, float r) {
  return __builtin_fabsf(kx - u) < r && __builtin_fabsf(ky - v) < r;
}

SPFE_PM float spfe_proj_duv(float kx, float ky, float u, float v) {
  const float du = kx - u, dv = ky - v;
  return du * du + dv * dv;
}

/* one lane's share of the squared distance: four consecutive dimensions, in order */
SPFE_PM double spfe_proj_lane_sum(const float a[4], const float b[4]) {
  const float d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2], d3 = a[3] - b[3];
  double s = (double)d0 * (double)d0;
  s = s + (double)d1 * (double)d1;
  s = s + (double)d2 * (double)d2;
  s = s + (double)d3 * (double)d3;
  return s;
}
SPFE_PM float spfe_proj_dist(double s) { return (float)__builtin_sqrt(s); }

SPFE_PM float spfe_proj_best_init(int mode) { return mode == SPFE_PROJ_MODE_LOCAL_MAP ? 256.0f : 3.402823466e+38f; }

SPFE_PM int spfe_proj_accept(int mode, float best, float duv, float th_dist, int adaptive, float c2) {
  if (mode != SPFE_PROJ_MODE_LOCAL_MAP) return best <= 0.7f;
  if (best <= th_dist) return 1;
  const float thr = adaptive ? (1.2f * c2) / (c2 + duv) : 0.7f;
  return best < thr;
}

#endif /* SPFE_PROJ_MATH_H */
