/* guided_ref.c — host reference of SPMatcher::SearchBySim3Override: the two sequential loops over the keypoints and the
 * agreement, on the arithmetic of include/spfe_guided_math.h (the header the GPU kernels share).  Compile with
 * -ffp-contract=off.  `mutate` switches ONE rule to a wrong one, so that the tests can show that the fixtures tell the
 * difference:
 *   1 RANGE on the world-frame distance |P - Ow| of the target keyframe   2 Fuse's viewing-angle test added (needs `normal`)
 *   3 Fuse's chi-square gate added   4 already-matched keypoints removed from the windows   5 `<=` for `<` in the choice of the
 *   best (the last wins a tie)   6 agreement replaced by one-way (vnMatch1 alone decides)   7 the seed overwritten
 *   (matches12 starts empty)   8 window loops swapped (iy outer)
 * loopproj_ref_search is the literal sequential loop of SPMatcher::SearchByProjectionLoop on part (b) of the header; its
 * mutations:   1 "already found" rebuilt per point from the live array   2 a later point blocks an earlier one (the list is
 *   walked backwards)   3 `<=` on ties   4 the best is taken over ALL keypoints of the window and refused when it is taken
 *   5 the angle test dropped */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spfe_guided_math.h"

#define EXPORT __attribute__((visibility("default")))

typedef struct {
  float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2, th, th_dist, min_factor, max_factor;
} guided_ref_params;

typedef struct {
  const float *kp_xy;
  const int16_t *occ;
  const float *kp_desc;
  int K;
  const int32_t *mp;
  const float *Tcw;
} guided_ref_kf;

static float distance(const float *a, const float *b) {
  double s[64], t[64];
  for (int l = 0; l < 64; ++l) s[l] = spfe_proj_lane_sum(a + 4 * l, b + 4 * l);
  for (int off = 32; off >= 1; off >>= 1) {
    for (int l = 0; l < 64; ++l) t[l] = s[l] + s[l ^ off];
    memcpy(s, t, sizeof s);
  }
  return spfe_proj_dist(s[0]);
}

/* one direction: the points of `src` into `tgt` through the 3x4 form A */
static void direction(const guided_ref_kf *src, const guided_ref_kf *tgt, const float A[12], const spfe_guided_view *vw, int hc, int wc,
                      const float *xyz, const uint8_t *flags, const float *dist_range, const float *desc, const float *normal, int n,
                      const uint8_t *already_src, const uint8_t *already_tgt, float th, float th_dist, int32_t *match, float *dist,
                      uint8_t *reason, int mutate) {
  spfe_proj_cam cam_t;
  spfe_proj_cam_from_f32(tgt->Tcw, &cam_t);
  for (int i = 0; i < src->K; ++i) {
    match[i] = -1;
    dist[i] = 0.0f;
    const int id = src->mp[i];
    if (id < 0 || id >= n) { reason[i] = SPFE_GUIDED_R_NO_POINT; continue; }
    if (already_src[i]) { reason[i] = SPFE_GUIDED_R_ALREADY; continue; }
    if (!(flags[id] & SPFE_PROJ_POINT_SEARCHABLE)) { reason[i] = SPFE_GUIDED_R_SKIP_BAD; continue; }
    const float *P = xyz + 3 * id;
    float u, v;
    int why;
    if (mutate == 1) {
      spfe_guided_view open = *vw;
      open.min_factor = 0.0f;
      open.max_factor = 3.0e38f;
      why = spfe_guided_project(src->Tcw, A, &open, P, 0.0f, 1.0f, &u, &v);
      if (!why) {
        const float ox = P[0] - cam_t.Ow[0], oy = P[1] - cam_t.Ow[1], oz = P[2] - cam_t.Ow[2];
        const float d = (float)__builtin_sqrt(((double)ox * (double)ox + (double)oy * (double)oy) + (double)oz * (double)oz);
        if (d < vw->min_factor * dist_range[2 * id] || d > vw->max_factor * dist_range[2 * id + 1]) why = SPFE_GUIDED_R_RANGE;
      }
    } else {
      why = spfe_guided_project(src->Tcw, A, vw, P, dist_range[2 * id], dist_range[2 * id + 1], &u, &v);
    }
    if (!why && mutate == 2) {
      const float ox = P[0] - cam_t.Ow[0], oy = P[1] - cam_t.Ow[1], oz = P[2] - cam_t.Ow[2];
      const float d = (float)__builtin_sqrt(((double)ox * (double)ox + (double)oy * (double)oy) + (double)oz * (double)oz);
      const double dot = ((double)ox * (double)normal[3 * id] + (double)oy * (double)normal[3 * id + 1]) + (double)oz * (double)normal[3 * id + 2];
      if (dot < 0.5 * (double)d) why = SPFE_GUIDED_R_RANGE;
    }
    if (why) { reason[i] = (uint8_t)why; continue; }
    int x0, x1, y0, y1;
    spfe_proj_window(u, th, wc, &x0, &x1);
    spfe_proj_window(v, th, hc, &y0, &y1);
    float best = spfe_guided_best_init();
    int bi = -1;
    const int nx = x1 - x0 + 1, ny = y1 - y0 + 1;
    for (int c = 0; nx > 0 && ny > 0 && c < nx * ny; ++c) {
      const int ix = mutate == 8 ? x0 + c % nx : x0 + c / ny, iy = mutate == 8 ? y0 + c / nx : y0 + c % ny;
      const int k = tgt->occ[iy * wc + ix];
      if (k < 0 || k >= tgt->K) continue;
      const float kx = tgt->kp_xy[2 * k], ky = tgt->kp_xy[2 * k + 1];
      if (!spfe_proj_in_window(kx, ky, u, v, th)) continue;
      if (mutate == 3) {
        const float ex = u - kx, ey = v - ky;
        if ((double)(ex * ex + ey * ey) > 5.99) continue;
      }
      if (mutate == 4 && already_tgt[k]) continue;
      const float d = distance(desc + 256 * (size_t)id, tgt->kp_desc + 256 * (size_t)k);
      if (mutate == 5 ? d <= best : d < best) { best = d; bi = k; }
    }
    if (bi < 0) { reason[i] = SPFE_GUIDED_R_NO_CANDIDATE; continue; }
    if (best > th_dist) { reason[i] = SPFE_GUIDED_R_TOO_FAR; continue; }
    reason[i] = SPFE_GUIDED_R_MATCHED;
    match[i] = bi;
    dist[i] = best;
  }
}

/* counts: n_found, n_total, n_seed.  matches12 has kcap >= K1 entries, all written. */
EXPORT void guided_ref_search(const float *kp_xy1, const int16_t *occ1, const float *kp_desc1, int K1, const int32_t *mp1,
                              const float *kp_xy2, const int16_t *occ2, const float *kp_desc2, int K2, const int32_t *mp2, int hc,
                              int wc, float W, float H, const float *xyz, const uint8_t *flags, const float *dist_range,
                              const float *desc, const float *normal, int n, const float *Tcw1, const float *Tcw2,
                              const float *T13, const int32_t *seed12, const guided_ref_params *prm, int32_t *match1, float *dist1,
                              uint8_t *reason1, int32_t *match2, float *dist2, uint8_t *reason2, int32_t *matches12, int kcap,
                              int32_t *counts, int mutate) {
  const guided_ref_kf kf1 = {kp_xy1, occ1, kp_desc1, K1, mp1, Tcw1}, kf2 = {kp_xy2, occ2, kp_desc2, K2, mp2, Tcw2};
  spfe_sim3_T T;
  float T12[12], T21[12];
  spfe_guided_T_from_f32(T13, &T);
  spfe_sim3_forms(&T, T12, T21);
  uint8_t *al1 = (uint8_t *)calloc((size_t)(K1 > 0 ? K1 : 1), 1), *al2 = (uint8_t *)calloc((size_t)(K2 > 0 ? K2 : 1), 1);
  for (int k1 = 0; k1 < K1; ++k1) {
    const int s = seed12[k1];
    if (s >= 0) {
      al1[k1] = 1;
      if (s < K2) al2[s] = 1;
    }
  }
  const spfe_guided_view into2 = {prm->fx2, prm->fy2, prm->cx2, prm->cy2, W, H, prm->min_factor, prm->max_factor};
  const spfe_guided_view into1 = {prm->fx1, prm->fy1, prm->cx1, prm->cy1, W, H, prm->min_factor, prm->max_factor};
  direction(&kf1, &kf2, T21, &into2, hc, wc, xyz, flags, dist_range, desc, normal, n, al1, al2, prm->th, prm->th_dist, match1, dist1,
            reason1, mutate);
  direction(&kf2, &kf1, T12, &into1, hc, wc, xyz, flags, dist_range, desc, normal, n, al2, al1, prm->th, prm->th_dist, match2, dist2,
            reason2, mutate);
  int n_found = 0, n_total = 0, n_seed = 0;
  for (int i1 = 0; i1 < kcap; ++i1) {
    int m = -1;
    if (i1 < K1) {
      const int k2 = match1[i1], seed = mutate == 7 ? -1 : seed12[i1];
      int found;
      if (mutate == 6) {
        found = k2 >= 0;
        m = found ? k2 : seed;
      } else {
        m = spfe_guided_agree(i1, k2, (k2 >= 0 && k2 < K2) ? match2[k2] : -1, seed, &found);
      }
      n_found += found;
      n_seed += seed12[i1] >= 0;
    }
    matches12[i1] = m;
    n_total += m >= 0;
  }
  counts[0] = n_found;
  counts[1] = n_total;
  counts[2] = n_seed;
  free(al1);
  free(al2);
}

typedef struct {
  float fx, fy, cx, cy, th, th_dist;
  double view_cos;
  float min_factor, max_factor;
} loopproj_ref_params;

/* matched [K] is in/out.  -> n_matched */
EXPORT int loopproj_ref_search(const float *kp_xy, const int16_t *occ, const float *kp_desc, int K, int hc, int wc, float W, float H,
                               const float *Scw, int32_t *matched, const int32_t *point_id, const float *xyz, const float *normal,
                               const float *dist_range, const float *desc, const uint8_t *flags, int n,
                               const loopproj_ref_params *prm, int32_t *kp_of_mp, float *best_dist, uint8_t *reason,
                               int32_t *matched_idx, int mutate) {
  spfe_proj_cam cam;
  spfe_loop_cam_from_scw(Scw, &cam);
  spfe_fuse_view vw = {prm->fx, prm->fy, prm->cx, prm->cy, W, H, prm->min_factor, prm->max_factor, mutate == 5 ? -1.0e30 : prm->view_cos};
  int32_t *entry = (int32_t *)malloc(sizeof(int32_t) * (size_t)(K > 0 ? K : 1));   /* spAlreadyFound: the entry state */
  if (K > 0) memcpy(entry, matched, sizeof(int32_t) * (size_t)K);
  for (int step = 0; step < n; ++step) {
    const int i = mutate == 2 ? n - 1 - step : step;
    kp_of_mp[i] = -1;
    best_dist[i] = 0.0f;
    reason[i] = 0;
    if (!(flags[i] & SPFE_PROJ_POINT_SEARCHABLE)) { reason[i] = SPFE_LOOPPROJ_R_SKIP_BAD; continue; }
    int found = 0;
    for (int k = 0; k < K; ++k) found |= (mutate == 1 ? matched[k] : entry[k]) == point_id[i];
    if (found) { reason[i] = SPFE_LOOPPROJ_R_ALREADY_FOUND; continue; }
    float u, v;
    const int why = spfe_fuse_project(&cam, &vw, xyz + 3 * i, normal + 3 * i, dist_range[2 * i], dist_range[2 * i + 1], &u, &v);
    if (why) { reason[i] = (uint8_t)why; continue; }
    const float r = prm->th;
    int x0, x1, y0, y1;
    spfe_proj_window(u, r, wc, &x0, &x1);
    spfe_proj_window(v, r, hc, &y0, &y1);
    float best = spfe_loopproj_best_init();
    int bi = -1, any = 0;
    const int nx = x1 - x0 + 1, ny = y1 - y0 + 1;
    for (int c = 0; nx > 0 && ny > 0 && c < nx * ny; ++c) {
      const int ix = x0 + c / ny, iy = y0 + c % ny;
      const int k = occ[iy * wc + ix];
      if (k < 0 || k >= K) continue;
      if (!spfe_proj_in_window(kp_xy[2 * k], kp_xy[2 * k + 1], u, v, r)) continue;
      any = 1;
      if (mutate != 4 && matched[k] != -1) continue;
      const float d = distance(desc + 256 * (size_t)i, kp_desc + 256 * (size_t)k);
      if (mutate == 3 ? d <= best : d < best) { best = d; bi = k; }
    }
    if (!any) { reason[i] = SPFE_LOOPPROJ_R_NO_CANDIDATE; continue; }
    if (best > prm->th_dist || bi < 0 || (mutate == 4 && matched[bi] != -1)) { reason[i] = SPFE_LOOPPROJ_R_TOO_FAR; continue; }
    reason[i] = SPFE_LOOPPROJ_R_MATCHED;
    kp_of_mp[i] = bi;
    best_dist[i] = best;
    matched[bi] = point_id[i];
  }
  int nm = 0;
  for (int i = 0; i < n; ++i)
    if (reason[i] == SPFE_LOOPPROJ_R_MATCHED) matched_idx[nm++] = i;
  free(entry);
  return nm;
}
