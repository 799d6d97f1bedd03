/* proj_ref.c — host reference of the window search by projection: the sequential loop of SPMatcher::SearchByProjection behind
 * Tracking::SearchLocalPoints / Frame::isInFrustum, on the arithmetic of include/spfe_proj_math.h (the header the GPU kernels
 * share).  Compile with -ffp-contract=off.  `mutate` switches ONE rule to a wrong one, so that the tests can show that the
 * fixtures tell the difference:
 *   1 window loops swapped (iy outer)   2 `<=` for `<` in the radius test   3 fallback to the second best when the best is
 *   refused   4 unobserved holders block   5 the already-held rule dropped   6 float accumulation of the distance */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spfe_proj_math.h"

#define EXPORT __attribute__((visibility("default")))

static float distance(const float *a, const float *b, int mutate) {
  if (mutate == 6) {
    float s = 0.0f;
    for (int k = 0; k < 256; ++k) { const float d = a[k] - b[k]; s = s + d * d; }
    return __builtin_sqrtf(s);
  }
  double s[64], t[64];
  for (int l = 0; l < 64; ++l) s[l] = spfe_proj_lane_sum(a + 4 * l, b + 4 * l);
  for (int off = 32; off >= 1; off >>= 1) {
    for (int l = 0; l < 64; ++l) t[l] = s[l] + s[l ^ off];
    memcpy(s, t, sizeof s);
  }
  return spfe_proj_dist(s[0]);
}

EXPORT int proj_ref_search(const float *kp_xy, const int16_t *occ, const float *kp_desc, int K, int hc, int wc, float W, float H,
                           const float *xyz, const float *normal, const float *desc, const uint8_t *flags, int n,
                           int32_t *mp_of_kp, const float *Tcw, float fx, float fy, float cx, float cy, int mode, float th,
                           float th_dist, float view_cos_limit, int adaptive, float c2, int32_t *kp_of_mp, uint8_t *in_view,
                           float *proj_uv, float *view_cos, float *best_dist, int *n_to_match, int mutate) {
  spfe_proj_cam cam;
  spfe_proj_cam_from_f32(Tcw, &cam);
  uint8_t *held = (uint8_t *)calloc((size_t)(n > 0 ? n : 1), 1);
  if (mode == SPFE_PROJ_MODE_LOCAL_MAP)
    for (int k = 0; k < K; ++k) {
      const int m = mp_of_kp[k];
      if (m < 0 || m >= n) continue;
      if (flags[m] & SPFE_PROJ_POINT_SEARCHABLE) held[m] = mutate == 5 ? 0 : 1;
      else mp_of_kp[k] = -1;
    }
  int nmatches = 0, ntm = 0;
  const float zero3[3] = {0.0f, 0.0f, 0.0f};
  for (int i = 0; i < n; ++i) {
    kp_of_mp[i] = -1;
    in_view[i] = 0;
    proj_uv[2 * i] = proj_uv[2 * i + 1] = view_cos[i] = best_dist[i] = 0.0f;
    if (!(flags[i] & SPFE_PROJ_POINT_SEARCHABLE) || held[i]) continue;
    float u, v, vc;
    if (!spfe_proj_project(&cam, xyz + 3 * i, normal ? normal + 3 * i : zero3, fx, fy, cx, cy, W, H, mode, view_cos_limit, &u,
                           &v, &vc))
      continue;
    in_view[i] = 1;
    proj_uv[2 * i] = u;
    proj_uv[2 * i + 1] = v;
    view_cos[i] = vc;
    ntm++;
    const float r = spfe_proj_radius(mode, vc, th);
    int x0, x1, y0, y1;
    spfe_proj_window(u, r, wc, &x0, &x1);
    spfe_proj_window(v, r, hc, &y0, &y1);
    float best = spfe_proj_best_init(mode), best2 = best, bduv = 0.0f, bduv2 = 0.0f;
    int bi = -1, bi2 = -1;
    const int nx = x1 - x0 + 1, ny = y1 - y0 + 1;
    for (int c = 0; nx > 0 && ny > 0 && c < nx * ny; ++c) {
      const int ix = mutate == 1 ? x0 + c % nx : x0 + c / ny, iy = mutate == 1 ? y0 + c / nx : y0 + c % ny;
      const int k = occ[iy * wc + ix];
      if (k < 0 || k >= K) continue;
      const float kx = kp_xy[2 * k], ky = kp_xy[2 * k + 1];
      if (mutate == 2) {
        if (!(__builtin_fabsf(kx - u) <= r && __builtin_fabsf(ky - v) <= r)) continue;
      } else if (!spfe_proj_in_window(kx, ky, u, v, r)) {
        continue;
      }
      const int m = mp_of_kp[k];
      if (m >= 0 && m < n && (mutate == 4 || (flags[m] & SPFE_PROJ_POINT_OBSERVED))) continue;   /* blocked */
      const float d = distance(desc + 256 * (size_t)i, kp_desc + 256 * (size_t)k, mutate);
      if (d < best) {
        best2 = best; bi2 = bi; bduv2 = bduv;
        best = d; bi = k; bduv = spfe_proj_duv(kx, ky, u, v);
      } else if (d < best2) {
        best2 = d; bi2 = k; bduv2 = spfe_proj_duv(kx, ky, u, v);
      }
    }
    if (bi < 0) continue;   /* nothing in the window, or everything blocked: no match */
    best_dist[i] = best;
    int take = -1;
    if (spfe_proj_accept(mode, best, bduv, th_dist, adaptive, c2)) take = bi;
    else if (mutate == 3 && bi2 >= 0 && spfe_proj_accept(mode, best2, bduv2, th_dist, adaptive, c2)) take = bi2;
    if (take >= 0) {
      mp_of_kp[take] = i;
      kp_of_mp[i] = take;
      nmatches++;
    }
  }
  free(held);
  *n_to_match = ntm;
  return nmatches;
}
