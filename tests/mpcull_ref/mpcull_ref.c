/* mpcull_ref.c — the host reference of map-point culling and of its resident state: a sequential restatement of
 *   LocalMapping::MapPointCulling                  orb_slam2/src/mapping/local_mapper.cpp:281-310
 *   LocalMapping::CreateNewMapPoints (the tail)    orb_slam2/src/mapping/local_mapper.cpp:770-787
 *   MapPoint::MapPoint / IncreaseVisible / Found   orb_slam2/src/type/mappoint.cpp:37-53, :191-203
 *   Tracking::TrackLocalMap / SearchLocalPoints    orb_slam2/src/tracking/tracker.cpp:576-588, :772-807
 * on the arrays of include/spfe.h ("map-point culling"), with the contract of include/spfe_mpcull_math.h.  It edits the state, the
 * rows and the table in place and writes the whole block of each form, every byte; the GPU tests compare all of it byte for byte.
 * The cull is ONE walk over the list that reads the flags as the walk left them: the statement the kernels' first-entry scratch has
 * to equal.
 * `mutate` switches ONE line to a plausible misreading, so that tests/test_mpcull_reference.py can show that its cases tell them
 * apart:
 *   1 <= for < at the ratio                                   7 a duplicate entry decided on the flags at entry
 *   2 the integer test 4 * found < visible for the division   8 the compaction not stable (a kept entry swapped in from the end)
 *   3 > for >= at the age of 2                                9 nobs cleared on a cull
 *   4 > for >= at the age of 3                               10 first_kf taken as a slot (the admission stores cur_slot)
 *   5 < for <= at th_obs                                     11 the statistics count a point held twice once
 *   6 the rows of bad slots edited too
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spfe.h"
#include "../../include/spfe_mpcull_math.h"

#define EXPORT __attribute__((visibility("default")))

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

EXPORT void mpcull_ref_reset(const spfe_mp_life *l, int first_row, int n_rows, int reset_list) {
  uint8_t *flags = (uint8_t *)l->d_mp_flags;
  int32_t *nobs = (int32_t *)l->d_mp_nobs, *found = (int32_t *)l->d_mp_found, *visible = (int32_t *)l->d_mp_visible;
  int32_t *first_kf = (int32_t *)l->d_mp_first_kf, *recent = (int32_t *)l->d_recent;
  for (int p = first_row; p < first_row + n_rows; ++p) {
    flags[p] = 0;
    nobs[p] = 0;
    found[p] = 0;
    visible[p] = 0;
    first_kf[p] = -1;
  }
  if (reset_list) {
    for (int e = 0; e < l->recent_cap; ++e) recent[e] = -1;
    *(int32_t *)l->d_recent_n = 0;
  }
}

/* (A) */
EXPORT void mpcull_ref_admit(const spfe_mp_life *l, const uint8_t *tri, size_t tri_stride, int kmax, int n_neigh, const int32_t *neigh_slot,
                             int cur_slot, int cur_kf_id, int32_t *rows, int kp_stride, int n_slots, float *xyz, uint8_t *out, int mutate) {
  uint8_t *flags = (uint8_t *)l->d_mp_flags;
  int32_t *nobs = (int32_t *)l->d_mp_nobs, *found = (int32_t *)l->d_mp_found, *visible = (int32_t *)l->d_mp_visible;
  int32_t *first_kf = (int32_t *)l->d_mp_first_kf, *recent = (int32_t *)l->d_recent, *recent_n = (int32_t *)l->d_recent_n;
  int32_t *hdr = (int32_t *)out, *admitted = (int32_t *)(out + SPFE_ADMIT_OFF_ADMITTED);
  int cnt[SPFE_TRI_MAX_NEIGHBOURS], base[SPFE_TRI_MAX_NEIGHBOURS], slot[SPFE_TRI_MAX_NEIGHBOURS], used[SPFE_TRI_MAX_NEIGHBOURS];
  memset(out, 0, SPFE_ADMIT_OUT_BYTES);
  const int n_before = clampi(*recent_n, 0, l->recent_cap);
  /* (A1) */
  for (int j = 0; j < n_neigh; ++j) {
    const uint8_t *blk = tri + (size_t)j * tri_stride;
    used[j] = *(const int32_t *)(blk + SPFE_TRI_OFF_STATUS) == 0;
    cnt[j] = used[j] ? *(const int32_t *)(blk + SPFE_TRI_OFF_N_NEW) : 0;
    base[j] = used[j] ? *(const int32_t *)(blk + SPFE_TRI_OFF_POINT_BASE) : 0;
    slot[j] = used[j] ? neigh_slot[j] : -1;
  }
  /* (A2) */
  int status = 0;
  int64_t total = 0;
  for (int j = 0; j < n_neigh; ++j) {
    if (!used[j]) continue;
    if (spfe_mc_block_bad(cnt[j], base[j], slot[j], cur_slot, kmax, n_slots, l->n_table)) status |= SPFE_ADMIT_BAD_RANGE;
    for (int i = 0; i < j; ++i)
      if (used[i] && slot[i] == slot[j]) status |= SPFE_ADMIT_BAD_RANGE;
    if (cnt[j] >= 0 && cnt[j] <= kmax) total += cnt[j];
  }
  const int64_t needed = (int64_t)n_before + total;
  if (needed > l->recent_cap) status |= SPFE_ADMIT_RECENT_OVERFLOW;
  if (!(status & SPFE_ADMIT_BAD_RANGE)) {
    for (int j = 0; j < n_neigh; ++j) {
      const uint8_t *blk = tri + (size_t)j * tri_stride;
      const int32_t *k1 = (const int32_t *)(blk + SPFE_TRI_OFF_NEW_K1(kmax)), *k2 = (const int32_t *)(blk + SPFE_TRI_OFF_NEW_K2(kmax));
      for (int t = 0; t < cnt[j]; ++t)
        if (!spfe_mc_kp_in_range(k1[t], kp_stride) || !spfe_mc_kp_in_range(k2[t], kp_stride)) status |= SPFE_ADMIT_BAD_RANGE;
    }
  }
  hdr[SPFE_ADMIT_OFF_N_RECENT_BEFORE / 4] = n_before;
  hdr[SPFE_ADMIT_OFF_N_NEEDED / 4] = (int32_t)(needed < INT32_MAX ? needed : INT32_MAX);
  if (status) {
    hdr[SPFE_ADMIT_OFF_STATUS / 4] = status;
    hdr[SPFE_ADMIT_OFF_N_RECENT_AFTER / 4] = n_before;
    return;
  }
  /* (A3) */
  int at = n_before, displaced = 0;
  for (int j = 0; j < n_neigh; ++j) {
    const uint8_t *blk = tri + (size_t)j * tri_stride;
    const int32_t *k1 = (const int32_t *)(blk + SPFE_TRI_OFF_NEW_K1(kmax)), *k2 = (const int32_t *)(blk + SPFE_TRI_OFF_NEW_K2(kmax));
    const float *x = (const float *)(blk + SPFE_TRI_OFF_NEW_XYZ(kmax));
    for (int t = 0; t < cnt[j]; ++t) {
      const int p = base[j] + t;
      int32_t *e1 = rows + (size_t)cur_slot * kp_stride + k1[t], *e2 = rows + (size_t)slot[j] * kp_stride + k2[t];
      displaced += (*e1 != -1) + (*e2 != -1);
      *e1 = p;
      *e2 = p;
      for (int c = 0; c < 3; ++c) xyz[3 * (size_t)p + c] = x[3 * (size_t)t + c];
      nobs[p] = 2;
      found[p] = 1;
      visible[p] = 1;
      first_kf[p] = mutate == 10 ? cur_slot : cur_kf_id;
      flags[p] = (uint8_t)(SPFE_PROJ_SEARCHABLE | SPFE_PROJ_OBSERVED);
      recent[at++] = p;
    }
    admitted[j] = cnt[j];
  }
  if (at > n_before) *recent_n = at;
  hdr[SPFE_ADMIT_OFF_STATUS / 4] = displaced ? SPFE_ADMIT_DISPLACED : 0;
  hdr[SPFE_ADMIT_OFF_N_ADMITTED / 4] = at - n_before;
  hdr[SPFE_ADMIT_OFF_N_RECENT_AFTER / 4] = at;
  hdr[SPFE_ADMIT_OFF_N_DISPLACED / 4] = displaced;
}

/* (B) */
EXPORT void mpcull_ref_stat(const spfe_mp_life *l, const int32_t *entry, const int32_t *after, int n_kp, const int32_t *point_idx,
                            int point_cap, const uint8_t *in_view, const uint8_t *outlier, uint8_t *out, int mutate) {
  const uint8_t *flags = (const uint8_t *)l->d_mp_flags;
  int32_t *found = (int32_t *)l->d_mp_found, *visible = (int32_t *)l->d_mp_visible, *hdr = (int32_t *)out;
  uint8_t *seen = mutate == 11 ? (uint8_t *)calloc((size_t)l->n_table, 1) : NULL;
  int held = 0, view = 0, fnd = 0;
  memset(out, 0, SPFE_MPSTAT_OUT_BYTES);
  for (int k = 0; k < n_kp; ++k) {   /* (B1) tracker.cpp:772-807, the held points */
    const int r = entry[k];
    if (!spfe_mc_in_range(r, l->n_table) || !spfe_mc_good(flags[r])) continue;
    if (seen && seen[r]) continue;
    if (seen) seen[r] = 1;
    visible[r]++;
    ++held;
  }
  for (int i = 0; i < point_cap; ++i) {   /* (B2) the projected points in view */
    if (in_view[i] == 0) continue;
    const int r = point_idx[i];
    if (!spfe_mc_in_range(r, l->n_table)) continue;
    visible[r]++;
    ++view;
  }
  if (seen) memset(seen, 0, (size_t)l->n_table);
  for (int k = 0; k < n_kp; ++k) {   /* (B3) tracker.cpp:576-588 */
    const int r = after[k];
    if (!spfe_mc_in_range(r, l->n_table) || outlier[k] != 0) continue;
    if (seen && seen[r]) continue;
    if (seen) seen[r] = 1;
    found[r]++;
    ++fnd;
  }
  free(seen);
  hdr[SPFE_MPSTAT_OFF_N_VISIBLE_HELD / 4] = held;
  hdr[SPFE_MPSTAT_OFF_N_VISIBLE_VIEW / 4] = view;
  hdr[SPFE_MPSTAT_OFF_N_FOUND / 4] = fnd;
}

static int rule(int found, int visible, int first_kf, int nobs, int cur_kf_id, int th_obs, float found_ratio, int mutate) {
  if (mutate < 1 || mutate > 5) return spfe_mc_rule(found, visible, first_kf, nobs, cur_kf_id, th_obs, found_ratio);
  const int64_t age = spfe_mc_age(cur_kf_id, first_kf);
  const float ratio = spfe_mc_ratio(found, visible);
  const int low = mutate == 1 ? ratio <= found_ratio : mutate == 2 ? 4 * (int64_t)found < (int64_t)visible : ratio < found_ratio;
  if (low) return SPFE_MPCULL_CODE_CULLED_RATIO;
  if ((mutate == 3 ? age > 2 : age >= 2) && (mutate == 5 ? nobs < th_obs : nobs <= th_obs)) return SPFE_MPCULL_CODE_CULLED_OBS;
  if (mutate == 4 ? age > 3 : age >= 3) return SPFE_MPCULL_CODE_RETIRED;
  return SPFE_MPCULL_CODE_KEPT;
}

/* (C) */
EXPORT void mpcull_ref_cull(const spfe_mp_life *l, int32_t *rows, int kp_stride, const uint8_t *kf_flags, int n_slots, int cur_kf_id,
                            int th_obs, float found_ratio, int bad_cap, uint8_t *out, int mutate) {
  uint8_t *flags = (uint8_t *)l->d_mp_flags;
  int32_t *nobs = (int32_t *)l->d_mp_nobs;
  const int32_t *found = (const int32_t *)l->d_mp_found, *visible = (const int32_t *)l->d_mp_visible, *first_kf = (const int32_t *)l->d_mp_first_kf;
  int32_t *recent = (int32_t *)l->d_recent, *recent_n = (int32_t *)l->d_recent_n;
  const int cap = l->recent_cap, nt = l->n_table;
  memset(out, 0, SPFE_MPCULL_OUT_BYTES(cap, bad_cap));
  int32_t *hdr = (int32_t *)out, *e_point = (int32_t *)(out + SPFE_MPCULL_OFF_ENTRY_POINT);
  int32_t *e_code = (int32_t *)(out + SPFE_MPCULL_OFF_ENTRY_CODE(cap)), *bad_point = (int32_t *)(out + SPFE_MPCULL_OFF_BAD_POINT(cap));
  for (int e = 0; e < cap; ++e) e_point[e] = e_code[e] = -1;
  for (int j = 0; j < bad_cap; ++j) bad_point[j] = -1;
  const int n = clampi(*recent_n, 0, cap);
  uint8_t *mark = (uint8_t *)calloc((size_t)nt, 1), *at_entry = (uint8_t *)malloc((size_t)nt);
  memcpy(at_entry, flags, (size_t)nt);
  int counts[6] = {0, 0, 0, 0, 0, 0}, kept = 0, n_bad = 0;
  for (int e = 0; e < n; ++e) {   /* the walk: an erase from the list is "not copied forward" */
    const int p = recent[e];
    int code;
    if (!spfe_mc_in_range(p, nt)) {
      code = SPFE_MPCULL_CODE_WILD;
    } else if (!spfe_mc_good(mutate == 7 ? at_entry[p] : flags[p])) {
      code = SPFE_MPCULL_CODE_ERASED_BAD;
    } else {
      code = rule(found[p], visible[p], first_kf[p], nobs[p], cur_kf_id, th_obs, found_ratio, mutate);
      if (spfe_mc_culls(code)) {   /* MapPoint::SetBadFlag; the rows are edited below (C9) */
        if (!mark[p]) {
          if (n_bad < bad_cap) bad_point[n_bad] = p;
          ++n_bad;
        }
        flags[p] = (uint8_t)(flags[p] & ~SPFE_PROJ_SEARCHABLE);
        mark[p] = 1;
        if (mutate == 9) nobs[p] = 0;
      }
    }
    e_point[e] = p;
    e_code[e] = code;
    counts[code]++;
    if (code == SPFE_MPCULL_CODE_KEPT) recent[kept++] = p;
  }
  if (mutate == 8 && kept >= 2) {
    const int32_t t = recent[0];
    recent[0] = recent[kept - 1];
    recent[kept - 1] = t;
  }
  for (int e = kept; e < n; ++e) recent[e] = -1;
  *recent_n = kept;
  if (n_bad)
    for (int s = 0; s < n_slots; ++s) {   /* (C9) */
      if ((kf_flags[s] & 1u) && mutate != 6) continue;
      for (int k = 0; k < kp_stride; ++k) {
        const int p = rows[(size_t)s * kp_stride + k];
        if (spfe_mc_in_range(p, nt) && mark[p]) rows[(size_t)s * kp_stride + k] = -1;
      }
    }
  free(mark);
  free(at_entry);
  hdr[SPFE_MPCULL_OFF_STATUS / 4] = (n_bad > bad_cap ? SPFE_MPCULL_BAD_CUT : 0) | (counts[SPFE_MPCULL_CODE_WILD] ? SPFE_MPCULL_WILD_ENTRY : 0);
  hdr[SPFE_MPCULL_OFF_N_LISTED / 4] = n;
  hdr[SPFE_MPCULL_OFF_N_KEPT / 4] = kept;
  hdr[SPFE_MPCULL_OFF_N_CULLED_RATIO / 4] = counts[SPFE_MPCULL_CODE_CULLED_RATIO];
  hdr[SPFE_MPCULL_OFF_N_CULLED_OBS / 4] = counts[SPFE_MPCULL_CODE_CULLED_OBS];
  hdr[SPFE_MPCULL_OFF_N_RETIRED / 4] = counts[SPFE_MPCULL_CODE_RETIRED];
  hdr[SPFE_MPCULL_OFF_N_ERASED_BAD / 4] = counts[SPFE_MPCULL_CODE_ERASED_BAD];
  hdr[SPFE_MPCULL_OFF_N_WILD / 4] = counts[SPFE_MPCULL_CODE_WILD];
  hdr[SPFE_MPCULL_OFF_N_BAD / 4] = n_bad;
  hdr[SPFE_MPCULL_OFF_N_BAD_STORED / 4] = n_bad < bad_cap ? n_bad : bad_cap;
}

/* the layout as this translation unit sees the macros */
EXPORT void mpcull_ref_layout(int recent_cap, int bad_cap, int kmax, int64_t *v) {
  int i = 0;
  v[i++] = SPFE_MPCULL_OFF_ENTRY_POINT;
  v[i++] = (int64_t)SPFE_MPCULL_OFF_ENTRY_CODE(recent_cap);
  v[i++] = (int64_t)SPFE_MPCULL_OFF_BAD_POINT(recent_cap);
  v[i++] = (int64_t)SPFE_MPCULL_OUT_BYTES(recent_cap, bad_cap);
  v[i++] = SPFE_MPCULL_BAD_CUT;
  v[i++] = SPFE_MPCULL_WILD_ENTRY;
  v[i++] = SPFE_ADMIT_RECENT_OVERFLOW;
  v[i++] = SPFE_ADMIT_BAD_RANGE;
  v[i++] = SPFE_ADMIT_DISPLACED;
  v[i++] = SPFE_ADMIT_OFF_ADMITTED;
  v[i++] = SPFE_ADMIT_OUT_BYTES;
  v[i++] = SPFE_MPSTAT_OUT_BYTES;
  v[i++] = SPFE_MP_MAX_POINTS;
  v[i++] = SPFE_TRI_MAX_NEIGHBOURS;
  v[i++] = (int64_t)SPFE_TRI_OUT_BYTES(kmax);
  v[i++] = (int64_t)SPFE_TRI_OFF_NEW_XYZ(kmax);
  v[i++] = (int64_t)SPFE_TRI_OFF_NEW_K1(kmax);
  v[i++] = (int64_t)SPFE_TRI_OFF_NEW_K2(kmax);
  v[i++] = SPFE_PROJ_OFF_VIEW;
  v[i++] = SPFE_POSE_OFF_OUTLIER;
  v[i++] = (int64_t)sizeof(spfe_mp_life);
  v[i++] = (int64_t)sizeof(spfe_mpcull_params);
  v[i++] = SPFE_MPCULL_OFF_N_BAD_STORED;
  v[i++] = SPFE_ADMIT_OFF_N_NEEDED;
}
