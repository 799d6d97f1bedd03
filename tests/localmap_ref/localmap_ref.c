/* localmap_ref.c — the host reference of the tracker's local map: a sequential restatement of
 *   Tracking::UpdateLocalKeyFrames   orb_slam2/src/tracking/tracker.cpp:868-984
 *   Tracking::UpdateLocalPoints      orb_slam2/src/tracking/tracker.cpp:843-866
 * on the arrays of include/spfe.h ("the tracker's local map"), with the contract of include/spfe_localmap_math.h.  It writes the
 * whole block of spfe_update_local_map_resident, every byte; the GPU tests compare byte for byte.
 * `mutate` switches ONE line to a plausible misreading, so that tests/test_localmap_reference.py can show that its cases tell
 * them apart:
 *   1 the parent's break leaves only the inner scope (the walk goes on)      5 a point held twice counts once
 *   2 the parent is tested for bad                                           6 bad keyframes get no votes
 *   3 >= for > at the 80 rule                                                7 held points are not listed first
 *   4 >= for > in the greatest vote                                          8 the walk iterates the grown list
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spfe.h"
#include "../../include/spfe_localmap_math.h"

#define EXPORT __attribute__((visibility("default")))

static int holds(const uint8_t *mp_flags, int n_table, const int32_t *mp_of_kp, const uint8_t *outlier, int k) {
  const int p = mp_of_kp[k];
  if (!spfe_lm_in_table(p, n_table) || !(mp_flags[p] & SPFE_PROJ_SEARCHABLE)) return 0;
  return !(outlier && outlier[k]);
}

/* steps (1) and (2): the table bytes (n_table) and votes / total (n_slots) */
static void vote(const int32_t *rows, int kp_stride, const uint8_t *kf_flags, int n_slots, const uint8_t *mp_flags, int n_table,
                 const int32_t *mp_of_kp, const uint8_t *outlier, int n_kp, uint8_t *table, int32_t *votes, int32_t *total,
                 int mutate) {
  int *count = (int *)calloc((size_t)(n_table > 0 ? n_table : 1), sizeof(int));
  for (int k = 0; k < n_kp; ++k)
    if (holds(mp_flags, n_table, mp_of_kp, outlier, k)) {
      const int p = mp_of_kp[k];
      if (mutate == 5 && count[p]) continue;
      count[p]++;
    }
  for (int p = 0; p < n_table; ++p) table[p] = (uint8_t)spfe_lm_table_byte(mp_flags[p], count[p]);
  for (int s = 0; s < n_slots; ++s) {
    int v = 0, t = 0;
    for (int k = 0; k < kp_stride; ++k) {
      const int p = rows[(size_t)s * kp_stride + k];
      if (!spfe_lm_in_table(p, n_table)) continue;
      v += spfe_lm_weight(table[p]);
      t += spfe_lm_searchable(table[p]);
    }
    if (mutate == 6 && kf_flags && (kf_flags[s] & 1)) v = 0;
    votes[s] = v;
    total[s] = t;
  }
  free(count);
}

EXPORT void localmap_ref_count(const int32_t *rows, int kp_stride, int n_slots, const uint8_t *mp_flags, int n_table,
                               const int32_t *mp_of_kp, const uint8_t *outlier, int n_kp, int32_t *votes, int32_t *total) {
  uint8_t *table = (uint8_t *)malloc((size_t)(n_table > 0 ? n_table : 1));
  vote(rows, kp_stride, NULL, n_slots, mp_flags, n_table, mp_of_kp, outlier, n_kp, table, votes, total, 0);
  free(table);
}

EXPORT void localmap_ref_update(const int32_t *rows, int kp_stride, const uint8_t *kf_flags, const int32_t *best_cov, int n_best,
                                const int32_t *parent, int n_slots, const uint8_t *mp_flags, int n_table, const int32_t *mp_of_kp,
                                int n_kp, int max_keyframes, int point_cap, uint8_t *out, int mutate) {
  const int n = n_slots;
  memset(out, 0, SPFE_LOCALMAP_OUT_BYTES(n, point_cap, n_kp));
  int32_t *hdr = (int32_t *)out;
  int32_t *local_kf = (int32_t *)(out + SPFE_LOCALMAP_OFF_LOCAL_KF);
  int32_t *votes = (int32_t *)(out + SPFE_LOCALMAP_OFF_VOTES(n));
  int32_t *total = (int32_t *)(out + SPFE_LOCALMAP_OFF_TOTAL(n));
  int32_t *point_idx = (int32_t *)(out + SPFE_LOCALMAP_OFF_POINT_IDX(n));
  int32_t *list = (int32_t *)(out + SPFE_LOCALMAP_OFF_MP_OF_KP_LIST(n, point_cap));
  uint8_t *table = (uint8_t *)malloc((size_t)(n_table > 0 ? n_table : 1));
  uint8_t *marked = (uint8_t *)calloc((size_t)n, 1);
  int *pos = (int *)malloc(sizeof(int) * (size_t)(n_table > 0 ? n_table : 1)); /* list position of a point, -1 = not listed */
  int32_t *all = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n_table > 0 ? n_table : 1));
  for (int p = 0; p < n_table; ++p) pos[p] = -1;

  vote(rows, kp_stride, kf_flags, n, mp_flags, n_table, mp_of_kp, NULL, n_kp, table, votes, total, mutate);

  /* (3) the voted set in slot order, the reference keyframe */
  int n_voted = 0, max = 0, ref_slot = -1, status = 0;
  for (int s = 0; s < n; ++s) {
    if (votes[s] <= 0) continue; /* not in keyframeCounter */
    if (kf_flags[s] & 1) continue;
    if (mutate == 4 ? votes[s] >= max : votes[s] > max) {
      max = votes[s];
      ref_slot = s;
    }
    local_kf[n_voted++] = s;
    marked[s] = 1;
  }
  int n_local = n_voted;
  if (n_voted == 0) status |= SPFE_LOCALMAP_NO_VOTES;

  /* (4) the walk */
  for (int i = 0; i < (mutate == 8 ? n_local : n_voted); ++i) {
    if (mutate == 3 ? n_local >= max_keyframes : spfe_lm_full(n_local, max_keyframes)) break;
    const int v = local_kf[i];
    for (int j = 0; j < n_best; ++j) {
      const int s = best_cov[(size_t)v * n_best + j];
      if (s < 0 || s >= n) {
        if (s != -1) status |= SPFE_LOCALMAP_BAD_SLOT;
        continue;
      }
      if ((kf_flags[s] & 1) || marked[s]) continue;
      local_kf[n_local++] = s;
      marked[s] = 1;
      break;
    }
    for (int c = 0; c < n; ++c)
      if (parent[c] == v && !(kf_flags[c] & 1) && !marked[c]) {
        local_kf[n_local++] = c;
        marked[c] = 1;
        break;
      }
    const int p = parent[v];
    if (p < -1 || p >= n) {
      status |= SPFE_LOCALMAP_BAD_SLOT;
    } else if (p >= 0 && !marked[p] && !(mutate == 2 && (kf_flags[p] & 1))) {
      local_kf[n_local++] = p;
      marked[p] = 1;
      if (mutate != 1) break;
    }
  }
  for (int j = n_local; j < n; ++j) local_kf[j] = -1;

  /* (5) the list: the held points first, then the rows of L */
  int n_all = 0, n_held = 0;
  if (mutate != 7)
    for (int k = 0; k < n_kp; ++k)
      if (holds(mp_flags, n_table, mp_of_kp, NULL, k) && pos[mp_of_kp[k]] < 0) {
        pos[mp_of_kp[k]] = n_all;
        all[n_all++] = mp_of_kp[k];
      }
  n_held = n_all;
  for (int i = 0; i < n_local; ++i)
    for (int k = 0; k < kp_stride; ++k) {
      const int p = rows[(size_t)local_kf[i] * kp_stride + k];
      if (!spfe_lm_in_table(p, n_table) || !spfe_lm_searchable(table[p]) || pos[p] >= 0) continue;
      pos[p] = n_all;
      all[n_all++] = p;
    }
  if (mutate == 7) { /* the held points behind the rows' */
    for (int k = 0; k < n_kp; ++k)
      if (holds(mp_flags, n_table, mp_of_kp, NULL, k) && pos[mp_of_kp[k]] < 0) {
        pos[mp_of_kp[k]] = n_all;
        all[n_all++] = mp_of_kp[k];
      }
    for (int k = 0; k < n_kp; ++k) n_held += holds(mp_flags, n_table, mp_of_kp, NULL, k) != 0;
  }
  const int n_points = n_all < point_cap ? n_all : point_cap;
  for (int j = 0; j < point_cap; ++j) point_idx[j] = j < n_points ? all[j] : -1;
  for (int k = 0; k < n_kp; ++k) list[k] = holds(mp_flags, n_table, mp_of_kp, NULL, k) ? pos[mp_of_kp[k]] : -1;
  if (n_all > point_cap) status |= SPFE_LOCALMAP_TRUNCATED;

  hdr[SPFE_LOCALMAP_OFF_N_VOTED / 4] = n_voted;
  hdr[SPFE_LOCALMAP_OFF_N_LOCAL_KF / 4] = n_local;
  hdr[SPFE_LOCALMAP_OFF_REF_SLOT / 4] = ref_slot;
  hdr[SPFE_LOCALMAP_OFF_N_HELD / 4] = n_held;
  hdr[SPFE_LOCALMAP_OFF_N_POINTS / 4] = n_points;
  hdr[SPFE_LOCALMAP_OFF_N_POINTS_TOTAL / 4] = n_all;
  hdr[SPFE_LOCALMAP_OFF_STATUS / 4] = status;
  free(table);
  free(marked);
  free(pos);
  free(all);
}

/* the header's macros as the Python wrapper must have them: out[0..6] = OFF_LOCAL_KF, OFF_VOTES, OFF_TOTAL, OFF_POINT_IDX,
 * OFF_MP_OF_KP_LIST, OUT_BYTES, and the status bits and limits behind them */
EXPORT void localmap_ref_layout(int n_slots, int point_cap, int n_kp, int64_t *out) {
  out[0] = SPFE_LOCALMAP_OFF_LOCAL_KF;
  out[1] = (int64_t)SPFE_LOCALMAP_OFF_VOTES(n_slots);
  out[2] = (int64_t)SPFE_LOCALMAP_OFF_TOTAL(n_slots);
  out[3] = (int64_t)SPFE_LOCALMAP_OFF_POINT_IDX(n_slots);
  out[4] = (int64_t)SPFE_LOCALMAP_OFF_MP_OF_KP_LIST(n_slots, point_cap);
  out[5] = (int64_t)SPFE_LOCALMAP_OUT_BYTES(n_slots, point_cap, n_kp);
  out[6] = SPFE_LOCALMAP_NO_VOTES;
  out[7] = SPFE_LOCALMAP_TRUNCATED;
  out[8] = SPFE_LOCALMAP_BAD_SLOT;
  out[9] = SPFE_LOCALMAP_MAX_KEYFRAMES;
  out[10] = SPFE_LOCALMAP_MAX_STRIDE;
  out[11] = SPFE_LOCALMAP_MAX_BEST;
  out[12] = SPFE_LOCALMAP_MAX_WEIGHT;
  out[13] = SPFE_LOCALMAP_OFF_N_VOTED;
  out[14] = SPFE_LOCALMAP_OFF_N_LOCAL_KF;
  out[15] = SPFE_LOCALMAP_OFF_REF_SLOT;
  out[16] = SPFE_LOCALMAP_OFF_N_HELD;
  out[17] = SPFE_LOCALMAP_OFF_N_POINTS;
  out[18] = SPFE_LOCALMAP_OFF_N_POINTS_TOTAL;
  out[19] = SPFE_LOCALMAP_OFF_STATUS;
}
