/* lba_ref.c — the host reference of the two forms around the local bundle adjustment on resident state: a sequential restatement of
 *   Optimizer::LocalBundleAdjustment, the gathering      orb_slam2/src/mapping/optimizer.cpp:447-499, :568-658
 *   Optimizer::LocalBundleAdjustment, the map edits      orb_slam2/src/mapping/optimizer.cpp:660-662, :739-773
 * on the arrays of include/spfe.h ("local bundle adjustment on resident state"), with the contract of include/spfe_lba_math.h.  The
 * gather walks as the reference does — the ord row, the local rows, the points and their observations in order — and writes the whole
 * block, every byte; the application edits rows, flags, counts, reference slots, positions and poses in place and writes its block.
 * The GPU tests compare all of it byte for byte.
 * `mutate` switches ONE line to a plausible misreading, so that tests/test_lba_reference.py can show that its cases tell them apart:
 *   1 bad keyframes of the ord row not skipped                7 the reference keyframe not moved
 *   2 first occurrence of a point by slot, not by list order  8 positions of points that went bad not written
 *   3 observations in keypoint-major order                    9 repeated entries of the ord row not skipped
 *   4 the fixed list ordered by slot alone                   10 a solver that STOPPED mid-way refused as well
 *   5 a cut that keeps a later entry that fits               11 the remaining observations of a bad point left in the rows
 *   6 < 2 for <= 2 at the observation count
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spfe.h"
#include "../../include/spfe_lba_math.h"

#define EXPORT __attribute__((visibility("default")))

static int cmp_int(const void *a, const void *b) { return (*(const int *)a > *(const int *)b) - (*(const int *)a < *(const int *)b); }

EXPORT void lba_ref_gather(const int32_t *ord_row, int conn_cap, const int32_t *rows, int kp_stride, const uint8_t *kf_flags, int n_slots,
                           const uint8_t *mp_flags, const float *xyz, int n_table, const float *Tcw, int cur_slot, int origin_slot, int kf_cap,
                           int free_cap, int point_cap, int edge_cap, uint8_t *out, int mutate) {
  const size_t bytes = SPFE_LBA_GATHER_BYTES(kf_cap, point_cap, edge_cap);
  memset(out, 0, bytes);
  int32_t *hdr = (int32_t *)out, *kf_slot = (int32_t *)(out + SPFE_LBA_OFF_KF_SLOT);
  uint8_t *fixed = out + SPFE_LBA_OFF_FIXED(kf_cap);
  float *o_Tcw = (float *)(out + SPFE_LBA_OFF_TCW(kf_cap)), *o_xyz = (float *)(out + SPFE_LBA_OFF_XYZ(kf_cap, point_cap));
  int32_t *point_idx = (int32_t *)(out + SPFE_LBA_OFF_POINT_IDX(kf_cap)), *obs_start = (int32_t *)(out + SPFE_LBA_OFF_OBS_START(kf_cap, point_cap));
  int32_t *obs = (int32_t *)(out + SPFE_LBA_OFF_OBS(kf_cap, point_cap)), *edges = (int32_t *)(out + SPFE_LBA_OFF_EDGES(kf_cap, point_cap, edge_cap));
  int *ba_of = malloc(sizeof(int) * (size_t)n_slots), *place = malloc(sizeof(int) * (size_t)n_table);
  int status = 0;
  for (int s = 0; s < n_slots; ++s) ba_of[s] = -1;
  for (int p = 0; p < n_table; ++p) place[p] = -1;   /* -2: counted, not listed */
  /* (G1) */
  int n_local = 1, n_free = cur_slot == origin_slot ? 0 : 1;
  kf_slot[0] = cur_slot;
  fixed[0] = cur_slot == origin_slot;
  ba_of[cur_slot] = 0;
  int ended = 0;
  for (int j = 0; j < conn_cap && ord_row[j] != -1; ++j) {
    const int s = ord_row[j];
    if (!spfe_lb_in_range(s, n_slots) || s == cur_slot) continue;
    if (ba_of[s] >= 0 && mutate != 9) continue;
    if ((kf_flags[s] & 1u) && mutate != 1) continue;
    if (ended == 1) {   /* a repeated entry behind the cut is skipped all the same; another one is dropped */
      continue;
    }
    const int is_fixed = s == origin_slot;
    if (!spfe_lb_local_fits(n_local, n_free, is_fixed, kf_cap, free_cap)) {
      status |= SPFE_LBA_LOCAL_CUT;
      if (mutate != 5) ended = 1;
      continue;
    }
    kf_slot[n_local] = s;
    fixed[n_local] = (uint8_t)is_fixed;
    ba_of[s] = n_local++;
    n_free += !is_fixed;
  }
  /* (G2) */
  int n = 0, n_all = 0;
  int order[SPFE_BA_MAX_KEYFRAMES];
  for (int b = 0; b < n_local; ++b) order[b] = kf_slot[b];
  if (mutate == 2) qsort(order, (size_t)n_local, sizeof(int), cmp_int);
  for (int b = 0; b < n_local; ++b) {
    const int s = order[b];
    if (kf_flags[s] & 1u) continue;
    for (int k = 0; k < kp_stride; ++k) {
      const int p = rows[(size_t)s * kp_stride + k];
      if (!spfe_lb_in_range(p, n_table) || !spfe_lb_good(mp_flags[p]) || place[p] != -1) continue;
      ++n_all;
      if (n < point_cap) {
        point_idx[n] = p;
        memcpy(o_xyz + 3 * (size_t)n, xyz + 3 * (size_t)p, 12);
        place[p] = n++;
      } else {
        place[p] = -2;
      }
    }
  }
  if (n_all > point_cap) status |= SPFE_LBA_POINT_CUT;
  for (int i = n; i < point_cap; ++i) point_idx[i] = -1;
  /* (G3): one walk over all rows in (slot, keypoint) order files every observation under its point */
  int64_t *first = calloc((size_t)n + 1, sizeof(int64_t));
  for (int s = 0; s < n_slots; ++s) {
    if (kf_flags[s] & 1u) continue;
    for (int k = 0; k < kp_stride; ++k) {
      const int p = rows[(size_t)s * kp_stride + k];
      if (spfe_lb_in_range(p, n_table) && place[p] >= 0) ++first[place[p] + 1];
    }
  }
  for (int i = 0; i < n; ++i) first[i + 1] += first[i];
  const int64_t needed = first[n];
  int32_t *all_obs = malloc(sizeof(int32_t) * 2 * (size_t)(needed ? needed : 1));
  int64_t *at = malloc(sizeof(int64_t) * ((size_t)n + 1));
  memcpy(at, first, sizeof(int64_t) * ((size_t)n + 1));
  if (mutate == 3) {
    for (int k = 0; k < kp_stride; ++k)
      for (int s = 0; s < n_slots; ++s) {
        const int p = (kf_flags[s] & 1u) ? -1 : rows[(size_t)s * kp_stride + k];
        if (spfe_lb_in_range(p, n_table) && place[p] >= 0) {
          all_obs[2 * at[place[p]]] = s;
          all_obs[2 * at[place[p]]++ + 1] = k;
        }
      }
  } else {
    for (int s = 0; s < n_slots; ++s) {
      if (kf_flags[s] & 1u) continue;
      for (int k = 0; k < kp_stride; ++k) {
        const int p = rows[(size_t)s * kp_stride + k];
        if (spfe_lb_in_range(p, n_table) && place[p] >= 0) {
          all_obs[2 * at[place[p]]] = s;
          all_obs[2 * at[place[p]]++ + 1] = k;
        }
      }
    }
  }
  /* (G4) */
  int n_fixed = 0, n_cand = 0;
  const int room = kf_cap - n_local;
  int *cand = malloc(sizeof(int) * (size_t)n_slots);
  uint8_t *seen = calloc((size_t)n_slots, 1);
  for (int64_t t = 0; t < needed; ++t) {
    const int s = all_obs[2 * t];
    if (ba_of[s] >= 0 || seen[s]) continue;
    seen[s] = 1;
    cand[n_cand++] = s;
  }
  if (mutate == 4) qsort(cand, (size_t)n_cand, sizeof(int), cmp_int);
  for (int c = 0; c < n_cand; ++c) {
    if (n_fixed == room) {
      status |= SPFE_LBA_FIXED_CUT;
      break;
    }
    kf_slot[n_local + n_fixed] = cand[c];
    fixed[n_local + n_fixed] = 1;
    ba_of[cand[c]] = n_local + n_fixed++;
  }
  const int n_kf = n_local + n_fixed;
  for (int b = n_kf; b < kf_cap; ++b) kf_slot[b] = -1;
  /* (G6) */
  for (int b = 0; b < n_kf; ++b) memcpy(o_Tcw + 16 * (size_t)b, Tcw + 16 * (size_t)kf_slot[b], 64);
  /* (G5) */
  int n_obs = 0, n_edges = 0;
  if (needed > edge_cap) {
    status |= SPFE_LBA_EDGE_OVERFLOW;
    for (int i = 0; i <= point_cap; ++i) obs_start[i] = -1;
  } else {
    for (int i = 0; i < n; ++i) {
      obs_start[i] = n_obs;
      for (int64_t t = first[i]; t < first[i + 1]; ++t) {
        const int s = all_obs[2 * t], k = all_obs[2 * t + 1];
        obs[2 * n_obs] = s;
        obs[2 * n_obs++ + 1] = k;
        if (ba_of[s] >= 0) {
          edges[3 * n_edges] = i;
          edges[3 * n_edges + 1] = ba_of[s];
          edges[3 * n_edges++ + 2] = k;
        }
      }
    }
    obs_start[n] = n_obs;
    for (int i = n + 1; i <= point_cap; ++i) obs_start[i] = -1;
  }
  for (int t = 2 * n_obs; t < 2 * edge_cap; ++t) obs[t] = -1;
  for (int t = 3 * n_edges; t < 3 * edge_cap; ++t) edges[t] = -1;
  hdr[SPFE_LBA_OFF_STATUS / 4] = status;
  hdr[SPFE_LBA_OFF_N_LOCAL / 4] = n_local;
  hdr[SPFE_LBA_OFF_N_FREE / 4] = n_free;
  hdr[SPFE_LBA_OFF_N_FIXED / 4] = n_fixed;
  hdr[SPFE_LBA_OFF_N_KF / 4] = n_kf;
  hdr[SPFE_LBA_OFF_N_POINTS / 4] = n;
  hdr[SPFE_LBA_OFF_N_POINTS_ALL / 4] = n_all;
  hdr[SPFE_LBA_OFF_N_OBS / 4] = n_obs;
  hdr[SPFE_LBA_OFF_N_EDGES / 4] = n_edges;
  hdr[SPFE_LBA_OFF_N_OBS_NEEDED / 4] = (int32_t)needed;
  free(ba_of); free(place); free(first); free(all_obs); free(at); free(cand); free(seen);
}

static int valid_obs(int slot, int kp, const uint8_t *kf_flags, int n_slots, int kp_stride) {
  return spfe_lb_in_range(slot, n_slots) && !(kf_flags[slot] & 1u) && spfe_lb_in_range(kp, kp_stride);
}

EXPORT void lba_ref_apply(const uint8_t *gather, const uint8_t *ba, int32_t *rows, int kp_stride, const uint8_t *kf_flags, int n_slots,
                          uint8_t *mp_flags, int32_t *nobs, int32_t *ref_slot, float *xyz, int n_table, float *Tcw, int kf_cap, int point_cap,
                          int edge_cap, int bad_cap, uint8_t *out, int mutate) {
  memset(out, 0, SPFE_LBA_APPLY_BYTES(point_cap, edge_cap, bad_cap));
  int32_t *hdr = (int32_t *)out, *bad_point = (int32_t *)(out + SPFE_LBA_APPLY_OFF_BAD_POINT);
  int32_t *o_start = (int32_t *)(out + SPFE_LBA_APPLY_OFF_OBS_START(bad_cap)), *o_obs = (int32_t *)(out + SPFE_LBA_APPLY_OFF_OBS(point_cap, bad_cap));
  int32_t *o_ref = (int32_t *)(out + SPFE_LBA_APPLY_OFF_REF_SLOT(point_cap, edge_cap, bad_cap));
  const int32_t *g = (const int32_t *)gather, *s = (const int32_t *)ba;
  /* (A0) */
  int n_local = g[SPFE_LBA_OFF_N_LOCAL / 4], n_kf = g[SPFE_LBA_OFF_N_KF / 4], n = g[SPFE_LBA_OFF_N_POINTS / 4];
  int n_obs = g[SPFE_LBA_OFF_N_OBS / 4], n_edges = g[SPFE_LBA_OFF_N_EDGES / 4], n_erase = s[SPFE_BA_OFF_N_ERASE / 4];
  int refuse_bits = SPFE_BA_STATUS_UNSORTED | SPFE_BA_STATUS_COV_OVERFLOW | SPFE_BA_STATUS_TOO_MANY_FREE | SPFE_BA_STATUS_STOPPED_EARLY;
  if (mutate == 10) refuse_bits |= SPFE_BA_STATUS_STOPPED;
  const int ok = !(s[SPFE_BA_OFF_STATUS / 4] & refuse_bits) && !(g[SPFE_LBA_OFF_STATUS / 4] & SPFE_LBA_EDGE_OVERFLOW) &&
                 s[SPFE_BA_OFF_N_KF / 4] == n_kf && s[SPFE_BA_OFF_N_POINTS / 4] == n && s[SPFE_BA_OFF_N_EDGES / 4] == n_edges && n_local >= 1 &&
                 n_local <= n_kf && n_kf <= kf_cap && n >= 0 && n <= point_cap && n_edges >= 0 && n_edges <= n_obs && n_obs <= edge_cap &&
                 n_erase >= 0 && n_erase <= n_edges;
  if (!ok) n_local = n_kf = n = n_obs = n_edges = n_erase = 0;
  const int32_t *kf_slot = (const int32_t *)(gather + SPFE_LBA_OFF_KF_SLOT), *point_idx = (const int32_t *)(gather + SPFE_LBA_OFF_POINT_IDX(kf_cap));
  const int32_t *obs_start = (const int32_t *)(gather + SPFE_LBA_OFF_OBS_START(kf_cap, point_cap));
  const int32_t *obs = (const int32_t *)(gather + SPFE_LBA_OFF_OBS(kf_cap, point_cap));
  const int32_t *edges = (const int32_t *)(gather + SPFE_LBA_OFF_EDGES(kf_cap, point_cap, edge_cap));
  const float *Tcw_out = (const float *)(ba + SPFE_BA_OFF_TCW), *xyz_out = (const float *)(ba + SPFE_BA_OFF_XYZ(n_kf));
  const int32_t *erase_idx = (const int32_t *)(ba + SPFE_BA_OFF_ERASE(n_kf, n, n_edges));
  uint8_t *mark = calloc((size_t)edge_cap, 1);
  int wild = 0, n_erased = 0, n_bad = 0, n_moved = 0, n_after = 0;
#define RANGE(i, lo, len)                                                                  \
  do {                                                                                     \
    const int lo_ = obs_start[i], hi_ = obs_start[(i) + 1];                                \
    const int fine_ = lo_ >= 0 && lo_ <= hi_ && hi_ <= n_obs;                              \
    lo = fine_ ? lo_ : 0;                                                                  \
    len = fine_ ? hi_ - lo_ : 0;                                                           \
    if (!fine_) range_bad = 1;                                                             \
  } while (0)
  /* (A1) */
  for (int j = 0; j < n_erase; ++j) {
    const int e = erase_idx[j];
    int followed = 0, range_bad = 0;
    if (spfe_lb_in_range(e, n_edges)) {
      const int i = edges[3 * (size_t)e], b = edges[3 * (size_t)e + 1], kp = edges[3 * (size_t)e + 2];
      if (spfe_lb_in_range(i, n) && spfe_lb_in_range(b, n_kf) && spfe_lb_in_range(point_idx[i], n_table) &&
          valid_obs(kf_slot[b], kp, kf_flags, n_slots, kp_stride)) {
        int lo, len;
        RANGE(i, lo, len);
        for (int t = lo; t < lo + len && !followed; ++t)
          if (obs[2 * (size_t)t] == kf_slot[b] && obs[2 * (size_t)t + 1] == kp) {
            mark[t] = 1;
            rows[(size_t)kf_slot[b] * kp_stride + kp] = -1;
            followed = 1;
          }
      }
    }
    (void)range_bad;
    if (!followed) wild = 1;
  }
  /* (A2), (A3), (A5), (A6) point by point */
  for (int i = 0; i < n; ++i) {
    const int p = point_idx[i];
    o_start[i] = n_after;
    if (!spfe_lb_in_range(p, n_table)) {
      wild = 1;
      o_ref[i] = -1;
      continue;
    }
    int lo, len, range_bad = 0, k = 0, remaining = 0, least = -1, ref_hit = 0, went_bad = 0;
    RANGE(i, lo, len);
    if (range_bad) wild = 1;
    for (int t = lo; t < lo + len; ++t) {
      const int slot = obs[2 * (size_t)t], kp = obs[2 * (size_t)t + 1];
      if (!valid_obs(slot, kp, kf_flags, n_slots, kp_stride)) {
        wild = 1;
        continue;
      }
      if (mark[t]) {
        ++k;
        ref_hit |= slot == ref_slot[p];
      } else {
        if (!remaining) least = slot;
        ++remaining;
      }
    }
    n_erased += k;
    if (spfe_lb_good(mp_flags[p])) {
      nobs[p] -= k;
      if (mutate == 6 ? (k > 0 && nobs[p] < 2) : spfe_lb_goes_bad(k, nobs[p])) {
        went_bad = 1;
        mp_flags[p] = (uint8_t)(mp_flags[p] & ~1u);
        if (n_bad < bad_cap) bad_point[n_bad] = p;
        ++n_bad;
        for (int t = lo; t < lo + len && mutate != 11; ++t) {
          const int slot = obs[2 * (size_t)t], kp = obs[2 * (size_t)t + 1];
          if (valid_obs(slot, kp, kf_flags, n_slots, kp_stride) && !mark[t]) rows[(size_t)slot * kp_stride + kp] = -1;
        }
      } else {
        if (ref_hit && remaining > 0 && mutate != 7) {
          ref_slot[p] = least;
          ++n_moved;
        }
        for (int t = lo; t < lo + len; ++t) {
          const int slot = obs[2 * (size_t)t], kp = obs[2 * (size_t)t + 1];
          if (!valid_obs(slot, kp, kf_flags, n_slots, kp_stride) || mark[t]) continue;
          o_obs[2 * (size_t)n_after] = slot;
          o_obs[2 * (size_t)n_after++ + 1] = kp;
        }
      }
    }
    o_ref[i] = ref_slot[p];
    if (!(went_bad && mutate == 8)) memcpy(xyz + 3 * (size_t)p, xyz_out + 3 * (size_t)i, 12);   /* (A5) */
  }
#undef RANGE
  o_start[n] = n_after;
  for (int i = n + 1; i <= point_cap; ++i) o_start[i] = -1;
  for (int i = n; i < point_cap; ++i) o_ref[i] = -1;
  for (int t = 2 * n_after; t < 2 * edge_cap; ++t) o_obs[t] = -1;
  const int stored = n_bad < bad_cap ? n_bad : bad_cap;
  for (int j = stored; j < bad_cap; ++j) bad_point[j] = -1;
  /* (A4) */
  for (int b = 0; b < n_local; ++b)
    if (spfe_lb_in_range(kf_slot[b], n_slots)) memcpy(Tcw + 16 * (size_t)kf_slot[b], Tcw_out + 16 * (size_t)b, 64);
  hdr[SPFE_LBA_APPLY_OFF_STATUS / 4] = (ok ? 0 : SPFE_LBA_NOT_APPLIED) | (n_bad > bad_cap ? SPFE_LBA_BAD_CUT : 0) | (wild ? SPFE_LBA_WILD : 0);
  hdr[SPFE_LBA_APPLY_OFF_N_ERASED / 4] = n_erased;
  hdr[SPFE_LBA_APPLY_OFF_N_BAD / 4] = n_bad;
  hdr[SPFE_LBA_APPLY_OFF_N_BAD_STORED / 4] = stored;
  hdr[SPFE_LBA_APPLY_OFF_N_REF_MOVED / 4] = n_moved;
  hdr[SPFE_LBA_APPLY_OFF_N_OBS_AFTER / 4] = n_after;
  free(mark);
}

/* the layout as the header's macros give it, for the Python side */
EXPORT void lba_ref_layout(int k, int p, int e, int b, int64_t *v) {
  v[0] = (int64_t)SPFE_LBA_OFF_FIXED(k);
  v[1] = (int64_t)SPFE_LBA_OFF_TCW(k);
  v[2] = (int64_t)SPFE_LBA_OFF_POINT_IDX(k);
  v[3] = (int64_t)SPFE_LBA_OFF_XYZ(k, p);
  v[4] = (int64_t)SPFE_LBA_OFF_OBS_START(k, p);
  v[5] = (int64_t)SPFE_LBA_OFF_OBS(k, p);
  v[6] = (int64_t)SPFE_LBA_OFF_EDGES(k, p, e);
  v[7] = (int64_t)SPFE_LBA_GATHER_BYTES(k, p, e);
  v[8] = (int64_t)SPFE_LBA_APPLY_OFF_OBS_START(b);
  v[9] = (int64_t)SPFE_LBA_APPLY_OFF_OBS(p, b);
  v[10] = (int64_t)SPFE_LBA_APPLY_OFF_REF_SLOT(p, e, b);
  v[11] = (int64_t)SPFE_LBA_APPLY_BYTES(p, e, b);
  v[12] = SPFE_LBA_LOCAL_CUT | SPFE_LBA_POINT_CUT << 4 | SPFE_LBA_FIXED_CUT << 8 | SPFE_LBA_EDGE_OVERFLOW << 12;
  v[13] = SPFE_LBA_NOT_APPLIED | SPFE_LBA_BAD_CUT << 4 | SPFE_LBA_WILD << 8;
  v[14] = sizeof(spfe_lba_gather_params);
  v[15] = sizeof(spfe_lba_apply_params);
  v[16] = (int64_t)SPFE_BA_OFF_XYZ(k);
  v[17] = (int64_t)SPFE_BA_OFF_ERASE(k, p, e);
  v[18] = (int64_t)SPFE_BA_OUT_BYTES(k, p, e);
}
