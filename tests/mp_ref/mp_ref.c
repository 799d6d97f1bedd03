/* mp_ref.c — host reference of the map-point refresh: MapPoint::ComputeDistinctiveDescriptors and
 * MapPoint::UpdateNormalAndDepth for a list of points, as the plain sequential statement — the full row of distances, a sort, the
 * element of the median's rank; nested loops over the observations — on the arithmetic of include/spfe_mappoint_math.h (the
 * header the GPU kernels share).  Compile with -ffp-contract=off.
 * `mutate` switches ONE rule to a wrong one, so that the tests can show that the fixtures tell the difference:
 *   1 the median's rank rounded up   2 `<=` for `<` in the choice of the best row (the last wins a tie)   3 bad keyframes not
 *   skipped in the descriptor   4 bad keyframes skipped in the normal   5 the self-distance left out of the row   6 the normal
 *   not divided by n   7 min and max swapped   8 the best row started at -1 (where no row takes over nothing is written)
 *   9 NaN ranked below every number */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spfe.h"
#include "../../include/spfe_mappoint_math.h"

#define EXPORT __attribute__((visibility("default")))

static float distance(const float *a, const float *b) {
  double s[64], t[64];
  for (int l = 0; l < 64; ++l) s[l] = spfe_proj_lane_sum(a + 4 * l, b + 4 * l);
  for (int off = 32; off >= 1; off >>= 1) {
    for (int l = 0; l < 64; ++l) t[l] = s[l] + s[l ^ off];
    memcpy(s, t, sizeof s);
  }
  return spfe_proj_dist(s[0]);
}

static int nan_low;
static int by_rank(const void *pa, const void *pb) {
  const float a = *(const float *)pa, b = *(const float *)pb;
  if (nan_low) {
    if (a != a || b != b) return (a != a) ? ((b != b) ? 0 : -1) : 1;
    return a < b ? -1 : (b < a ? 1 : 0);
  }
  return spfe_mp_before(a, b) ? -1 : (spfe_mp_before(b, a) ? 1 : 0);
}

EXPORT void mp_ref_ow(const float *Tcw, float *Ow) {
  spfe_proj_cam c;
  spfe_proj_cam_from_f32(Tcw, &c);
  memcpy(Ow, c.Ow, sizeof c.Ow);
}

/* The keyframes: kf_flags [n_kf] (bit 0: bad), kf_K [n_kf] (the record's keypoint count; -1: the record pointer is null),
 * kf_status [n_kf], Tcw [n_kf][16], kf_desc [n_kf][row_cap][256] (f32, bf16 rows widened).  The rest as
 * spfe_refresh_map_points_device; `block` is the output block, the table arrays are written in place. */
EXPORT void mp_ref_refresh(int n_kf, const uint8_t *kf_flags, const int32_t *kf_K, const int32_t *kf_status, const float *Tcw,
                           const float *kf_desc, int row_cap, const int32_t *point_idx, const int32_t *obs_start, const int32_t *obs,
                           const int32_t *ref_slot, int m, int E, const float *xyz, const uint8_t *flags, float *normal,
                           float *dist_range, float *desc, int n_table, int mode, float level_scale, float top_scale, uint8_t *block,
                           int mutate) {
  int32_t *best_obs = (int32_t *)(block + SPFE_MP_OFF_BEST_OBS), *n_good = (int32_t *)(block + SPFE_MP_OFF_N_GOOD(m));
  float *best_median = (float *)(block + SPFE_MP_OFF_BEST_MEDIAN(m));
  uint8_t *code = block + SPFE_MP_OFF_CODE(m);
  int n_desc = 0, n_nd = 0, status = 0;
  for (int k = 0; k < n_kf; ++k)
    if (kf_K[k] >= 0) status |= kf_status[k];
  float *D = (float *)malloc(sizeof(float) * (SPFE_MP_MAX_OBS + 1) * (SPFE_MP_MAX_OBS + 1));
  float *rowv = (float *)malloc(sizeof(float) * (SPFE_MP_MAX_OBS + 1));
  for (int i = 0; i < m; ++i) {
    best_obs[i] = -1;
    n_good[i] = 0;
    best_median[i] = 0.0f;
    const int row = point_idx ? point_idx[i] : i;
    if (row < 0 || row >= n_table) { code[i] = SPFE_MP_R_INVALID; continue; }
    if (!(flags[row] & SPFE_PROJ_POINT_SEARCHABLE)) { code[i] = SPFE_MP_R_SKIP_BAD; continue; }
    const int s = obs_start[i], e = obs_start[i + 1];
    if (s < 0 || e > E || e < s) { code[i] = SPFE_MP_R_INVALID; continue; }
    if (e == s) { code[i] = SPFE_MP_R_NO_OBS; continue; }
    int bad = ref_slot[i] < 0 || ref_slot[i] >= n_kf, N = 0;
    for (int o = s; o < e; ++o) {
      const int slot = obs[2 * o], kp = obs[2 * o + 1];
      if (slot < 0 || slot >= n_kf) { bad = 1; continue; }
      const int good = !(kf_flags[slot] & 1);
      if (kf_K[slot] < 0) bad |= good;
      else bad |= kp < 0 || kp >= kf_K[slot];
      N += good;
    }
    if (bad) { code[i] = SPFE_MP_R_INVALID; continue; }
    n_good[i] = N;
    code[i] = (uint8_t)spfe_mp_code(mode, N);
    const float *P = xyz + 3 * (size_t)row;
    if (mode & SPFE_MP_NORMAL_DEPTH) { /* ---- (b) ---- */
      float sum[3] = {0.0f, 0.0f, 0.0f}, Ow[3], c[3];
      int n = 0;
      for (int o = s; o < e; ++o) {
        if (mutate == 4 && (kf_flags[obs[2 * o]] & 1)) continue;
        mp_ref_ow(Tcw + 16 * (size_t)obs[2 * o], Ow);
        spfe_mp_share(P, Ow, c);
        for (int k = 0; k < 3; ++k) sum[k] = sum[k] + c[k];
        ++n;
      }
      if (mutate == 6) memcpy(normal + 3 * (size_t)row, sum, sizeof sum);
      else spfe_mp_normal_out(sum, n, normal + 3 * (size_t)row);
      float range[2];
      mp_ref_ow(Tcw + 16 * (size_t)ref_slot[i], Ow);
      spfe_mp_range(P, Ow, level_scale, top_scale, range);
      dist_range[2 * (size_t)row] = range[mutate == 7 ? 1 : 0];
      dist_range[2 * (size_t)row + 1] = range[mutate == 7 ? 0 : 1];
      ++n_nd;
    }
    if (!(mode & SPFE_MP_DESC)) continue;
    /* ---- (a) ---- */
    const float *rows[SPFE_MP_MAX_OBS + 1];
    int rows_obs[SPFE_MP_MAX_OBS + 1], Nr = 0;
    for (int o = s; o < e; ++o) {
      const int slot = obs[2 * o];
      if ((kf_flags[slot] & 1) && !(mutate == 3 && kf_K[slot] >= 0)) continue;
      if (Nr <= SPFE_MP_MAX_OBS) {
        rows[Nr] = kf_desc + ((size_t)slot * row_cap + obs[2 * o + 1]) * 256;
        rows_obs[Nr] = o - s;
      }
      ++Nr;
    }
    if (mutate == 3) {
      if (Nr == 0 || Nr > SPFE_MP_MAX_OBS) continue;
    } else if (code[i] != SPFE_MP_R_REFRESHED) {
      continue;
    }
    const int Nn = Nr;
    for (int a = 0; a < Nn; ++a) {
      D[a * Nn + a] = 0.0f;
      for (int b = a + 1; b < Nn; ++b) D[a * Nn + b] = D[b * Nn + a] = distance(rows[a], rows[b]);
    }
    float best = spfe_mp_best_init();
    int besti = mutate == 8 ? -1 : 0;
    nan_low = mutate == 9;
    for (int a = 0; a < Nn; ++a) {
      int len = 0;
      for (int b = 0; b < Nn; ++b)
        if (!(mutate == 5 && b == a)) rowv[len++] = D[a * Nn + b];
      qsort(rowv, (size_t)len, sizeof(float), by_rank);
      int k = spfe_mp_median_rank(Nn);
      if (mutate == 1) k = Nn / 2; /* the ceiling of (N - 1) / 2 */
      const float median = len ? rowv[k < len ? k : len - 1] : 0.0f;
      if (mutate == 2 ? median <= best : spfe_mp_takes_over(median, best)) {
        best = median;
        besti = a;
      }
    }
    if (besti < 0) { best_median[i] = best; continue; }
    memcpy(desc + 256 * (size_t)row, rows[besti], 1024);
    best_obs[i] = rows_obs[besti];
    best_median[i] = best;
    ++n_desc;
  }
  free(D);
  free(rowv);
  int32_t *h = (int32_t *)block;
  h[0] = m;
  h[1] = n_desc;
  h[2] = n_nd;
  h[3] = status;
}
