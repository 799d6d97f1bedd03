/* loopfuse_ref.c — host reference of the loop closer's fusion step: the search of SPMatcher::Fuse(KeyFrame *, cv::Mat Scw, const
 * vector<MapPoint *> &, th, vpReplacePoint) as the sequential loop over the points, and the corrected poses of CorrectLoop, on
 * the arithmetic of include/spfe_loopfuse_math.h (the header the GPU kernels share).  Compile with -ffp-contract=off.
 * `mutate` switches ONE rule of the search to a wrong one, so that the tests can show that the fixtures tell the difference:
 *   1 image bound `<=` for `<`   2 the mapper's chi-square gate (5.99) kept   3 `<=` for `<` in the choice of the best (the
 *   last wins a tie)   4 the distance-range test dropped   5 the camera taken from Scw as it stands (the scale not divided
 *   out)   6 R divided by the scale but t not   7 TH_LOW (0.3f) for TH_HIGH   8 "already in the keyframe" ignored   9 `holder`
 *   read after the proposals of the points before it were written into kf_mp_of_kp   10 window loops swapped (iy outer)
 *   11 a window in which no candidate took over (all distances NaN) reported as NO_CANDIDATE */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spfe_loopfuse_math.h"

#define EXPORT __attribute__((visibility("default")))

typedef struct {
  float fx, fy, cx, cy, th, th_dist;
  double view_cos;
  float min_factor, max_factor;
} loopfuse_ref_params;

static float distance(const float *a, const float *b) {
  double s[64], t[64];
  for (int l = 0; l < 64; ++l) s[l] = spfe_proj_lane_sum(a + 4 * l, b + 4 * l);
  for (int off = 32; off >= 1; off >>= 1) {
    for (int l = 0; l < 64; ++l) t[l] = s[l] + s[l ^ off];
    memcpy(s, t, sizeof s);
  }
  return spfe_proj_dist(s[0]);
}

/* the camera with the division by the scale mutated */
static void cam_mutated(const float Scw[16], spfe_proj_cam *c, int mutate) {
  const double s2 = ((double)Scw[0] * (double)Scw[0] + (double)Scw[1] * (double)Scw[1]) + (double)Scw[2] * (double)Scw[2];
  const double inv = 1.0 / __builtin_sqrt(s2);
  float T[16];
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 4; ++k) T[4 * r + k] = (mutate == 5 || (mutate == 6 && k == 3)) ? Scw[4 * r + k] : (float)((double)Scw[4 * r + k] * inv);
  T[12] = T[13] = T[14] = 0.0f;
  T[15] = 1.0f;
  spfe_proj_cam_from_f32(T, c);
}

/* steps 3 - 6 with one rule mutated */
static int project_mutated(const spfe_proj_cam *c, const spfe_fuse_view *p, const float P[3], const float nrm[3], float dmin,
                           float dmax, float *u, float *v, int mutate) {
  float Pc[3];
  for (int r = 0; r < 3; ++r) Pc[r] = ((c->R[3 * r] * P[0] + c->R[3 * r + 1] * P[1]) + c->R[3 * r + 2] * P[2]) + c->t[r];
  if (Pc[2] < 0.0f) return SPFE_LOOPFUSE_R_BEHIND;
  const float invz = 1.0f / Pc[2];
  const float x = Pc[0] * invz, y = Pc[1] * invz;
  const float uu = p->fx * x + p->cx, vv = p->fy * y + p->cy;
  if (!(uu >= 0.0f && uu <= p->W)) return SPFE_LOOPFUSE_R_OUTSIDE;
  if (!(vv >= 0.0f && vv <= p->H)) return SPFE_LOOPFUSE_R_OUTSIDE;
  if (mutate != 1) {
    if (!(uu < p->W)) return SPFE_LOOPFUSE_R_OUTSIDE;
    if (!(vv < p->H)) return SPFE_LOOPFUSE_R_OUTSIDE;
  }
  const float ox = P[0] - c->Ow[0], oy = P[1] - c->Ow[1], oz = P[2] - c->Ow[2];
  const float dist = (float)__builtin_sqrt(((double)ox * (double)ox + (double)oy * (double)oy) + (double)oz * (double)oz);
  const double dot = ((double)ox * (double)nrm[0] + (double)oy * (double)nrm[1]) + (double)oz * (double)nrm[2];
  if (mutate != 4 && (dist < p->min_factor * dmin || dist > p->max_factor * dmax)) return SPFE_LOOPFUSE_R_RANGE;
  if (dot < p->view_cos * (double)dist) return SPFE_LOOPFUSE_R_ANGLE;
  *u = uu;
  *v = vv;
  return 0;
}

EXPORT int loopfuse_ref_search(const float *kp_xy, const int16_t *occ, const float *kp_desc, int K, int hc, int wc, float W,
                               float H, const int32_t *kf_mp_of_kp, const float *Scw, const int32_t *point_id, const float *xyz,
                               const float *normal, const float *dist_range, const float *desc, const uint8_t *flags, int n,
                               const loopfuse_ref_params *prm, int32_t *kp_of_mp, float *best_dist, int32_t *holder,
                               uint8_t *reason, int32_t *fused_idx, int mutate) {
  spfe_proj_cam cam;
  if (mutate == 5 || mutate == 6) cam_mutated(Scw, &cam, mutate);
  else spfe_loop_cam_from_scw(Scw, &cam);
  spfe_fuse_view vw = {prm->fx, prm->fy, prm->cx, prm->cy, W, H, prm->min_factor, prm->max_factor, prm->view_cos};
  const float th_dist = mutate == 7 ? 0.3f : prm->th_dist;
  int32_t *live = (int32_t *)malloc(sizeof(int32_t) * (size_t)(K > 0 ? K : 1));   /* mutate 9 only */
  if (K > 0) memcpy(live, kf_mp_of_kp, sizeof(int32_t) * (size_t)K);
  int nfused = 0;
  for (int i = 0; i < n; ++i) {
    kp_of_mp[i] = -1;
    holder[i] = -1;
    best_dist[i] = 0.0f;
    reason[i] = 0;
    if (!(flags[i] & SPFE_PROJ_POINT_SEARCHABLE)) { reason[i] = SPFE_LOOPFUSE_R_SKIP_BAD; continue; }
    int in_kf = 0;
    for (int k = 0; k < K; ++k) in_kf |= kf_mp_of_kp[k] == point_id[i];
    if (in_kf && mutate != 8) { reason[i] = SPFE_LOOPFUSE_R_SKIP_IN_KF; continue; }
    float u, v;
    const int why = (mutate == 1 || mutate == 4)
                        ? project_mutated(&cam, &vw, xyz + 3 * i, normal + 3 * i, dist_range[2 * i], dist_range[2 * i + 1], &u, &v, mutate)
                        : spfe_fuse_project(&cam, &vw, xyz + 3 * i, normal + 3 * i, dist_range[2 * i], dist_range[2 * i + 1], &u, &v);
    if (why) { reason[i] = (uint8_t)why; continue; }
    const float r = prm->th;
    int x0, x1, y0, y1;
    spfe_proj_window(u, r, wc, &x0, &x1);
    spfe_proj_window(v, r, hc, &y0, &y1);
    float best = spfe_loopfuse_best_init();
    int bi = -1, any = 0;
    const int nx = x1 - x0 + 1, ny = y1 - y0 + 1;
    for (int c = 0; nx > 0 && ny > 0 && c < nx * ny; ++c) {
      const int ix = mutate == 10 ? x0 + c % nx : x0 + c / ny, iy = mutate == 10 ? y0 + c / nx : y0 + c % ny;
      const int k = occ[iy * wc + ix];
      if (k < 0 || k >= K) continue;
      const float kx = kp_xy[2 * k], ky = kp_xy[2 * k + 1];
      if (!spfe_proj_in_window(kx, ky, u, v, r)) continue;
      if (mutate == 2 && !spfe_fuse_chi2_pass(kx, ky, u, v, 5.99)) continue;
      any = 1;
      const float d = distance(desc + 256 * (size_t)i, kp_desc + 256 * (size_t)k);
      if (mutate == 3 ? d <= best : d < best) { best = d; bi = k; }
    }
    int verdict = spfe_loopfuse_verdict(any, bi, best, th_dist);
    if (mutate == 11 && bi < 0) verdict = SPFE_LOOPFUSE_R_NO_CANDIDATE;
    reason[i] = (uint8_t)verdict;
    if (verdict != SPFE_LOOPFUSE_R_PROPOSED) continue;
    kp_of_mp[i] = bi;
    best_dist[i] = best;
    holder[i] = mutate == 9 ? live[bi] : kf_mp_of_kp[bi];
    live[bi] = point_id[i];
    fused_idx[nfused++] = i;
  }
  free(live);
  return nfused;
}

EXPORT void loopfuse_ref_poses(const double *S12, const float *Tcw2, const float *Twc, const float *Tiw, int n_targets,
                               int cur_index, float *Siw, float *Tiw_corrected) {
  for (int j = 0; j < n_targets; ++j)
    spfe_loopfuse_pose(S12, Tcw2, Twc, Tiw + 16 * (size_t)j, j == cur_index, Siw + 16 * (size_t)j, Tiw_corrected + 16 * (size_t)j);
}
