/* tri_ref.c — host reference of the creation of new map points between the current keyframe (1) and one neighbour (2), built
 * from include/spfe_tri_math.h: the sequence of operations the GPU kernels (sp_orb_slam_amd/csrc/tri.hip) evaluate, in plain C
 * loops.  `mutate` selects deliberately wrong variants that the fixtures of tests/golden/tri_*.npz must reject. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/spfe_tri_math.h"

#define EXPORT __attribute__((visibility("default")))

enum {
  MUT_NONE = 0,
  MUT_LOWEST_K2_WINS = 1,    /* the first accepted query keeps the train row */
  MUT_EPIPOLE_NAN_REJECTS = 2,
  MUT_LINE_TEST_FLOAT = 3,   /* dsqr < 3.84f * factor in float */
  MUT_RATIO_SQUARED = 4,     /* the ratio test on squared distances */
  MUT_COUNT_AFTER_OVERWRITE = 5, /* n_matches = the train rows that hold a match */
  MUT_DEPTH_LT = 6           /* z < 0 instead of z <= 0 */
};

/* parameter block, in the order of spfe_tri_params behind the intrinsics */
typedef struct {
  float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
  float ratio, epipole_r2;
  double chi2_line, chi2_reproj, cos_parallax_max, min_baseline_depth_ratio;
} tri_params;

static float dist256(const float *a, const float *b) {
  float s = 0.0f;
  for (int k = 0; k < 256; ++k) {
    const float d = a[k] - b[k];
    s = fmaf(d, d, s);
  }
  return sqrtf(s);
}

static int triangulate_depth_lt(const spfe_tri_cam *c1, const spfe_tri_cam *c2, float x1, float y1, float s1x, float s1y, float x2,
                                float y2, float s2x, float s2y, const tri_params *p, int sweeps, float X[3]) {
  float xn1[3], xn2[3], ray1[3], ray2[3];
  spfe_tri_xn(c1, x1, y1, xn1);
  spfe_tri_xn(c2, x2, y2, xn2);
  for (int k = 0; k < 3; ++k) {
    ray1[k] = (c1->R[k] * xn1[0] + c1->R[3 + k] * xn1[1]) + c1->R[6 + k] * xn1[2];
    ray2[k] = (c2->R[k] * xn2[0] + c2->R[3 + k] * xn2[1]) + c2->R[6 + k] * xn2[2];
  }
  const float cosr = (float)(spfe_tri_dot3(ray1, ray2) / (spfe_tri_norm3(ray1) * spfe_tri_norm3(ray2)));
  if (!(cosr > 0 && (double)cosr < p->cos_parallax_max)) return SPFE_TRI_PARALLAX;
  float A[16], x[4];
  spfe_tri_rows(c1, xn1, A);
  spfe_tri_rows(c2, xn2, A + 8);
  spfe_tri_null4(A, sweeps, x);
  if (x[3] == 0) return SPFE_TRI_DEGENERATE;
  for (int k = 0; k < 3; ++k) X[k] = x[k] / x[3];
  const float z1 = (float)(spfe_tri_dot3(&c1->R[6], X) + (double)c1->t[2]);
  if (z1 < 0) return SPFE_TRI_DEPTH;
  const float z2 = (float)(spfe_tri_dot3(&c2->R[6], X) + (double)c2->t[2]);
  if (z2 < 0) return SPFE_TRI_DEPTH;
  if (spfe_tri_reproj_reject(c1, X, z1, x1, y1, s1x, s1y, p->chi2_reproj)) return SPFE_TRI_REPROJ;
  if (spfe_tri_reproj_reject(c2, X, z2, x2, y2, s2x, s2y, p->chi2_reproj)) return SPFE_TRI_REPROJ;
  const float n1[3] = {X[0] - c1->Ow[0], X[1] - c1->Ow[1], X[2] - c1->Ow[2]};
  const float n2[3] = {X[0] - c2->Ow[0], X[1] - c2->Ow[1], X[2] - c2->Ow[2]};
  if ((float)spfe_tri_norm3(n1) == 0 || (float)spfe_tri_norm3(n2) == 0) return SPFE_TRI_DEGENERATE;
  return SPFE_TRI_NEW;
}

/* 1 when the baseline test skips the neighbour */
EXPORT int tri_ref_skip(const float *Tcw1, const float *Tcw2, const tri_params *p, float median_depth) {
  spfe_tri_cam c1, c2;
  spfe_tri_cam_from_f32(Tcw1, p->fx1, p->fy1, p->cx1, p->cy1, &c1);
  spfe_tri_cam_from_f32(Tcw2, p->fx2, p->fy2, p->cx2, p->cy2, &c2);
  return spfe_tri_baseline_skip(&c1, &c2, median_depth, p->min_baseline_depth_ratio);
}

/* One neighbour.  kp / cinv: [K][2], desc: [K][256] f32, mp: [K] in/out.  match12, verdict: [K1] (all written);
 * counts[6]: n_matches, n_new, n_rej_parallax, n_rej_depth, n_rej_reproj, n_rej_degenerate; new_xyz [K1][3], new_k1 / new_k2
 * [K1]: the first n_new entries written; null_vec [K1][4]: the null vector of every triangulated pair with `sweeps` sweeps
 * (may be null).  Returns n_new. */
EXPORT int tri_ref_pair(const float *kp1, const float *cinv1, const float *desc1, int K1, const float *kp2, const float *cinv2,
                        const float *desc2, int K2, int32_t *mp1, int32_t *mp2, const float *Tcw1, const float *Tcw2,
                        const tri_params *p, int point_base, int sweeps, int32_t *match12, int32_t *verdict, int32_t *counts,
                        float *new_xyz, int32_t *new_k1, int32_t *new_k2, float *null_vec, int mutate) {
  spfe_tri_cam c1, c2;
  spfe_tri_pair pr;
  spfe_tri_cam_from_f32(Tcw1, p->fx1, p->fy1, p->cx1, p->cy1, &c1);
  spfe_tri_cam_from_f32(Tcw2, p->fx2, p->fy2, p->cx2, p->cy2, &c2);
  spfe_tri_pair_from_cams(&c1, &c2, &pr);
  for (int k = 0; k < K1; ++k) { match12[k] = -1; verdict[k] = SPFE_TRI_NONE; }
  memset(counts, 0, 6 * sizeof(int32_t));
  for (int k2 = 0; k2 < K2; ++k2) {
    if (mp2[k2] >= 0) continue;
    int i0 = -1, i1 = -1;
    float d0 = 0, d1 = 0;
    for (int k1 = 0; k1 < K1; ++k1) {
      if (mp1[k1] >= 0) continue;
      const float d = dist256(desc2 + (size_t)k2 * 256, desc1 + (size_t)k1 * 256);
      if (!(d < 3.402823466e+38f)) continue;
      if (i0 < 0 || d < d0) { i1 = i0; d1 = d0; i0 = k1; d0 = d; }
      else if (i1 < 0 || d < d1) { i1 = k1; d1 = d; }
    }
    if (i1 < 0) continue;
    const float x1 = kp1[2 * i0], y1 = kp1[2 * i0 + 1], x2 = kp2[2 * k2], y2 = kp2[2 * k2 + 1];
    int ok;
    if (mutate == MUT_NONE || mutate == MUT_LOWEST_K2_WINS || mutate == MUT_COUNT_AFTER_OVERWRITE || mutate == MUT_DEPTH_LT) {
      ok = spfe_tri_gate(&pr, d0, d1, x1, y1, x2, y2, cinv2[2 * k2], cinv2[2 * k2 + 1], p->ratio, p->epipole_r2, p->chi2_line);
    } else {
      ok = mutate == MUT_RATIO_SQUARED ? (d0 * d0 < p->ratio * (d1 * d1)) : spfe_tri_ratio_ok(d0, d1, p->ratio);
      if (ok) {
        const float dx = pr.ex - x2, dy = pr.ey - y2;
        if (mutate == MUT_EPIPOLE_NAN_REJECTS ? !(dx * dx + dy * dy >= p->epipole_r2) : spfe_tri_epipole_reject(&pr, x2, y2, p->epipole_r2))
          ok = 0;
      }
      if (ok) {
        if (mutate == MUT_LINE_TEST_FLOAT) {
          const float *F = pr.F;
          const float a = (x1 * F[0] + y1 * F[3]) + F[6], b = (x1 * F[1] + y1 * F[4]) + F[7], c = (x1 * F[2] + y1 * F[5]) + F[8];
          const float s = cinv2[2 * k2 + 1] < cinv2[2 * k2] ? cinv2[2 * k2 + 1] : cinv2[2 * k2];
          const float factor = 1.0f / s, num = (a * x2 + b * y2) + c, den = a * a + b * b;
          ok = den != 0 && (num * num) / den < (float)p->chi2_line * factor;
        } else {
          ok = spfe_tri_line_ok(&pr, x1, y1, x2, y2, cinv2[2 * k2], cinv2[2 * k2 + 1], p->chi2_line);
        }
      }
    }
    if (!ok) continue;
    if (!(mutate == MUT_LOWEST_K2_WINS && match12[i0] >= 0)) match12[i0] = k2;
    counts[0]++;
  }
  if (mutate == MUT_COUNT_AFTER_OVERWRITE) {
    counts[0] = 0;
    for (int k = 0; k < K1; ++k) counts[0] += match12[k] >= 0;
  }
  int n_new = 0;
  for (int k1 = 0; k1 < K1; ++k1) {
    const int k2 = match12[k1];
    if (k2 < 0) continue;
    float X[3] = {0, 0, 0};
    int v;
    if (mutate == MUT_DEPTH_LT)
      v = triangulate_depth_lt(&c1, &c2, kp1[2 * k1], kp1[2 * k1 + 1], cinv1[2 * k1], cinv1[2 * k1 + 1], kp2[2 * k2], kp2[2 * k2 + 1],
                               cinv2[2 * k2], cinv2[2 * k2 + 1], p, sweeps, X);
    else
      v = spfe_tri_triangulate(&c1, &c2, kp1[2 * k1], kp1[2 * k1 + 1], cinv1[2 * k1], cinv1[2 * k1 + 1], kp2[2 * k2], kp2[2 * k2 + 1],
                               cinv2[2 * k2], cinv2[2 * k2 + 1], p->cos_parallax_max, p->chi2_reproj, sweeps, X);
    verdict[k1] = v;
    if (null_vec) {
      float xn1[3], xn2[3], A[16];
      spfe_tri_xn(&c1, kp1[2 * k1], kp1[2 * k1 + 1], xn1);
      spfe_tri_xn(&c2, kp2[2 * k2], kp2[2 * k2 + 1], xn2);
      spfe_tri_rows(&c1, xn1, A);
      spfe_tri_rows(&c2, xn2, A + 8);
      spfe_tri_null4(A, sweeps, null_vec + 4 * k1);
    }
    if (v == SPFE_TRI_PARALLAX) counts[2]++;
    else if (v == SPFE_TRI_DEPTH) counts[3]++;
    else if (v == SPFE_TRI_REPROJ) counts[4]++;
    else if (v == SPFE_TRI_DEGENERATE) counts[5]++;
    else {
      memcpy(new_xyz + 3 * n_new, X, 12);
      new_k1[n_new] = k1;
      new_k2[n_new] = k2;
      mp1[k1] = mp2[k2] = point_base + n_new;
      n_new++;
    }
  }
  counts[1] = n_new;
  return n_new;
}

EXPORT int tri_ref_default_sweeps(void) { return SPFE_TRI_JACOBI_SWEEPS; }
