/* cull_ref.c — the host reference of keyframe culling: a sequential restatement of
 *   LocalMapping::KeyFrameCullingOverride           orb_slam2/src/mapping/local_mapper.cpp:979-1032
 *   KeyFrame::SetBadFlag / EraseConnection          orb_slam2/src/type/keyframe.cpp:911-997, :1004-1016
 *   MapPoint::EraseObservation / SetBadFlag         orb_slam2/src/type/mappoint.cpp:122-173
 * on the arrays of include/spfe.h ("keyframe culling"), with the contract of include/spfe_cull_math.h.  It edits the rows, the
 * flags, the observation counts, the graph state and the two tables in place and writes the whole block of
 * spfe_cull_keyframes_resident, every byte; the GPU tests compare all of it byte for byte.
 * `mutate` switches ONE line to a plausible misreading, so that tests/test_cull_reference.py can show that its cases tell them
 * apart:
 *   1 >= for > in the choice (the last of equal ratios)      6 the point goes bad at nobs <= 1
 *   2 <= for < in the drop                                    7 a link removed from conn[s] although conn[c] does not hold s
 *   3 the step's maximum reset for each child                 8 > for >= th_obs
 *   4 bad children left out of the left-over                  9 the rows of bad slots edited too
 *   5 ord rebuilt from ord instead of conn                   10 the steps skip a child by its flag after the call (a keyframe
 *                                                               culled LATER in the call is still alive when its parent is)
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spfe.h"
#include "../../include/spfe_covis_math.h"
#include "../../include/spfe_cull_math.h"

#define EXPORT __attribute__((visibility("default")))

static int key_desc(const void *pa, const void *pb) {
  const int64_t a = *(const int64_t *)pa, b = *(const int64_t *)pb;
  return a > b ? -1 : (a < b ? 1 : 0);
}

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

EXPORT void cull_ref_count(const int32_t *rows, int kp_stride, const uint8_t *kf_flags, int n_slots, int32_t *nobs, int n_table) {
  for (int p = 0; p < n_table; ++p) nobs[p] = 0;
  for (int s = 0; s < n_slots; ++s) {
    if (kf_flags[s] & 1u) continue;
    for (int k = 0; k < kp_stride; ++k) {
      const int p = rows[(size_t)s * kp_stride + k];
      if (p >= 0 && p < n_table) nobs[p]++;
    }
  }
}

static void table_rows(int32_t *best_a, int n_best_a, int32_t *best_b, int n_best_b, int slot, const int32_t *os, int n) {
  if (best_a)
    for (int j = 0; j < n_best_a; ++j) best_a[(size_t)slot * n_best_a + j] = j < n ? os[j] : -1;
  if (best_b)
    for (int j = 0; j < n_best_b; ++j) best_b[(size_t)slot * n_best_b + j] = j < n ? os[j] : -1;
}

EXPORT void cull_ref_run(int32_t *rows, int kp_stride, uint8_t *kf_flags, uint8_t *mp_flags, int32_t *nobs, int n_table, int n_slots,
                         int conn_cap, int32_t *conn_slot, int32_t *conn_w, int32_t *conn_n, int32_t *ord_slot, int32_t *ord_w,
                         int32_t *ord_n, int32_t *parent, uint8_t *first_conn, int cur, int th_obs, float cov_ratio, int origin_slot,
                         int bad_cap, int32_t *best_a, int n_best_a, int32_t *best_b, int n_best_b, uint8_t *out, int mutate) {
  const int n = n_slots, cap = conn_cap;
  (void)first_conn;
  memset(out, 0, SPFE_CULL_OUT_BYTES(n, cap, bad_cap));
  int32_t *hdr = (int32_t *)out;
  int32_t *e_slot = (int32_t *)(out + SPFE_CULL_OFF_ENTRY_SLOT), *e_code = (int32_t *)(out + SPFE_CULL_OFF_ENTRY_CODE(cap));
  int32_t *e_pass = (int32_t *)(out + SPFE_CULL_OFF_ENTRY_PASS(cap)), *e_mps = (int32_t *)(out + SPFE_CULL_OFF_ENTRY_MPS(cap));
  int32_t *e_red = (int32_t *)(out + SPFE_CULL_OFF_ENTRY_RED(cap)), *culled = (int32_t *)(out + SPFE_CULL_OFF_CULLED_SLOT(cap));
  int32_t *touched = (int32_t *)(out + SPFE_CULL_OFF_TOUCHED_SLOT(cap)), *ev_c = (int32_t *)(out + SPFE_CULL_OFF_EVENT_CHILD(n, cap));
  int32_t *ev_p = (int32_t *)(out + SPFE_CULL_OFF_EVENT_PARENT(n, cap)), *bad_point = (int32_t *)(out + SPFE_CULL_OFF_BAD_POINT(n, cap));
  for (int j = 0; j < cap; ++j) e_slot[j] = e_code[j] = e_pass[j] = culled[j] = -1;
  for (int s = 0; s < n; ++s) touched[s] = ev_c[s] = ev_p[s] = -1;
  for (int j = 0; j < bad_cap; ++j) bad_point[j] = -1;
  int status = 0, n_passes = 0, n_culled = 0, n_deferred = 0, n_bad = 0;

  /* (1) the list, read once */
  const int n_listed = clampi(ord_n[cur], 0, cap);
  int *live = (int *)malloc(sizeof(int) * (size_t)(cap + 1));
  int n_live = 0;
  for (int j = 0; j < n_listed; ++j) {
    const int s = ord_slot[(size_t)cur * cap + j];
    e_slot[j] = s;
    e_pass[j] = 0;
    if (!spfe_ck_entry_in_range(s, n)) {
      e_code[j] = SPFE_CULL_CODE_WILD;
      status |= SPFE_CULL_WILD_ENTRY;
      continue;
    }
    e_code[j] = spfe_ck_entry_code(s, origin_slot, kf_flags[s]);
    if (e_code[j] < 0) live[n_live++] = j;
  }
  uint8_t *newly_bad = (uint8_t *)calloc((size_t)(n_table > 0 ? n_table : 1), 1);
  int *cnt = (int *)calloc((size_t)(n_table > 0 ? n_table : 1), sizeof(int));

  /* (2)-(5) the passes */
  while (n_live > 0) {
    ++n_passes;
    float ratio_max = 0.0f;
    int choice = -1, kept = 0;
    for (int i = 0; i < n_live; ++i) {
      const int j = live[i], s = e_slot[j];
      int n_mps = 0, n_red = 0;
      for (int k = 0; k < kp_stride; ++k) {
        const int p = rows[(size_t)s * kp_stride + k];
        if (spfe_ck_good(p, n_table, mp_flags)) {
          ++n_mps;
          n_red += mutate == 8 ? nobs[p] > th_obs : nobs[p] >= th_obs;
        }
      }
      e_mps[j] = n_mps;
      e_red[j] = n_red;
      e_pass[j] = n_passes;
      const float ratio = spfe_ck_ratio(n_red, n_mps);
      if (mutate == 2 ? ratio <= cov_ratio : spfe_ck_drops(ratio, cov_ratio)) {
        e_code[j] = SPFE_CULL_CODE_DROPPED;
        continue;
      }
      if (mutate == 1 ? (ratio >= ratio_max && ratio > 0.0f) : ratio > ratio_max) {
        ratio_max = ratio;
        choice = j;
      }
      live[kept++] = j;
    }
    n_live = kept;
    if (choice < 0) {
      if (n_live > 0) {   /* (3) */
        status |= SPFE_CULL_STALLED;
        for (int i = 0; i < n_live; ++i) e_code[live[i]] = SPFE_CULL_CODE_STALLED;
      }
      break;
    }
    kept = 0;
    for (int i = 0; i < n_live; ++i)
      if (live[i] != choice) live[kept++] = live[i];
    n_live = kept;
    const int m = e_slot[choice];
    if (kf_flags[m] & SPFE_KF_NOT_ERASE) {   /* (4) */
      kf_flags[m] |= SPFE_KF_TO_BE_ERASED;
      e_code[choice] = SPFE_CULL_CODE_DEFERRED;
      ++n_deferred;
      continue;
    }
    e_code[choice] = SPFE_CULL_CODE_CULLED;
    culled[n_culled++] = m;
    /* (5) */
    int32_t *row = rows + (size_t)m * kp_stride;
    for (int k = 0; k < kp_stride; ++k)
      if (spfe_ck_good(row[k], n_table, mp_flags)) cnt[row[k]]++;
    for (int k = 0; k < kp_stride; ++k) {
      const int p = row[k];
      if (!spfe_ck_good(p, n_table, mp_flags) || cnt[p] == 0) continue;   /* cnt 0: not the first entry of p */
      nobs[p] -= cnt[p];
      cnt[p] = 0;
      if (mutate == 6 ? nobs[p] <= 1 : spfe_ck_goes_bad(nobs[p])) {
        mp_flags[p] &= (uint8_t)~SPFE_PROJ_SEARCHABLE;
        newly_bad[p] = 1;
        if (n_bad < bad_cap) bad_point[n_bad] = p;
        ++n_bad;
      }
    }
    kf_flags[m] |= 1u;
  }
  if (n_bad > bad_cap) status |= SPFE_CULL_BAD_CUT;

  /* (6) the graph, in cull order */
  int64_t *key = (int64_t *)malloc(sizeof(int64_t) * (size_t)(cap + 1));
  uint8_t *is_touched = (uint8_t *)calloc((size_t)n, 1), *cand = (uint8_t *)calloc((size_t)n, 1);
  int *child = (int *)malloc(sizeof(int) * (size_t)n);
  int n_reparented = 0;
  int *cull_idx = (int *)malloc(sizeof(int) * (size_t)n);   /* the place of a slot in cull order, -1: not culled in this call */
  for (int s = 0; s < n; ++s) cull_idx[s] = -1;
  for (int ci = 0; ci < n_culled; ++ci) cull_idx[culled[ci]] = ci;
  for (int ci = 0; ci < n_culled; ++ci) {
    const int c = culled[ci];
    int32_t *ccs = conn_slot + (size_t)c * cap, *ccw = conn_w + (size_t)c * cap;
    int32_t *cos = ord_slot + (size_t)c * cap, *cow = ord_w + (size_t)c * cap;
    const int cn_c = clampi(conn_n[c], 0, cap);
    /* (a) */
    for (int q = 0; q < (mutate == 7 ? n : cn_c); ++q) {
      const int s = mutate == 7 ? q : ccs[q];
      if (!spfe_ck_entry_in_range(s, n) || s == c) continue;
      int32_t *cs = conn_slot + (size_t)s * cap, *cw = conn_w + (size_t)s * cap;
      int32_t *os = ord_slot + (size_t)s * cap, *ow = ord_w + (size_t)s * cap;
      const int cn = clampi(conn_n[s], 0, cap);
      int found = -1;
      for (int i = 0; i < cn && found < 0; ++i)
        if (cs[i] == c) found = i;
      if (found < 0) continue;
      for (int i = found; i + 1 < cn; ++i) {
        cs[i] = cs[i + 1];
        cw[i] = cw[i + 1];
      }
      cs[cn - 1] = -1;
      cw[cn - 1] = 0;
      conn_n[s] = cn - 1;
      int m = 0;
      if (mutate == 5) {
        const int on = clampi(ord_n[s], 0, cap);
        for (int i = 0; i < on; ++i)
          if (os[i] != c) key[m++] = spfe_cv_key(ow[i], os[i]);
      } else {
        for (int i = 0; i < cn - 1; ++i) key[m++] = spfe_cv_key(cw[i], cs[i]);
      }
      qsort(key, (size_t)m, sizeof(int64_t), key_desc);
      for (int i = 0; i < cap; ++i) {
        os[i] = i < m ? spfe_cv_key_slot(key[i]) : -1;
        ow[i] = i < m ? spfe_cv_key_w(key[i]) : 0;
      }
      ord_n[s] = m;
      table_rows(best_a, n_best_a, best_b, n_best_b, s, os, m);
      is_touched[s] = 1;
    }
    /* (b) */
    for (int i = 0; i < cap; ++i) {
      ccs[i] = cos[i] = -1;
      ccw[i] = cow[i] = 0;
    }
    conn_n[c] = ord_n[c] = 0;
    table_rows(best_a, n_best_a, best_b, n_best_b, c, cos, 0);
    /* (c) */
    int n_child = 0;
    for (int s = 0; s < n; ++s)
      if (s != c && parent[s] == c) child[n_child++] = s;
    const int p0 = spfe_ck_entry_in_range(parent[c], n) ? parent[c] : -1;
    if (p0 < 0) status |= SPFE_CULL_NO_PARENT;   /* with or without children: mpParent is dereferenced either way */
    if (n_child == 0) continue;
    memset(cand, 0, (size_t)n);
    if (p0 >= 0) cand[p0] = 1;
    for (;;) {
      int64_t best = SPFE_CULL_STEP_NONE;
      for (int a = 0; a < n_child; ++a) {
        const int s = child[a];
        if (s < 0) continue;
        /* isBad() as it stood when c was culled: bad before the call, or culled earlier in it */
        if (mutate == 10 ? (kf_flags[s] & 1u) : spfe_ck_child_is_bad(kf_flags[s], cull_idx[s], ci)) continue;
        int64_t child_best = SPFE_CULL_STEP_NONE;
        const int on = clampi(ord_n[s], 0, cap), cn = clampi(conn_n[s], 0, cap);
        for (int i = 0; i < on; ++i) {
          const int e = ord_slot[(size_t)s * cap + i];
          if (!spfe_ck_entry_in_range(e, n) || !cand[e]) continue;
          int w = 0;
          for (int t = 0; t < cn; ++t)
            if (conn_slot[(size_t)s * cap + t] == e) {
              w = conn_w[(size_t)s * cap + t];
              break;
            }
          const int64_t k = spfe_ck_step_key(w, a, i, cap);
          if (k > child_best) child_best = k;
        }
        /* mutate 3: the maximum starts again at each child, so the LAST child with any offer wins */
        if (mutate == 3 ? child_best != SPFE_CULL_STEP_NONE : child_best > best) best = child_best;
      }
      if (best == SPFE_CULL_STEP_NONE) break;
      const uint32_t walk = spfe_ck_step_walk(best);
      const int a = (int)(walk / (uint32_t)cap), i = (int)(walk % (uint32_t)cap), s = child[a];
      const int np = ord_slot[(size_t)s * cap + i];
      parent[s] = np;
      cand[s] = 1;
      child[a] = -1;
      if (n_reparented < n) {
        ev_c[n_reparented] = s;
        ev_p[n_reparented] = np;
      }
      ++n_reparented;
    }
    for (int a = 0; a < n_child; ++a) {
      const int s = child[a];
      if (s < 0 || (mutate == 4 && (kf_flags[s] & 1u))) continue;
      parent[s] = p0;
      if (n_reparented < n) {
        ev_c[n_reparented] = s;
        ev_p[n_reparented] = p0;
      }
      ++n_reparented;
    }
  }
  if (n_reparented > n) status |= SPFE_CULL_EVENT_CUT;
  int n_touched = 0;
  for (int s = 0; s < n; ++s)
    if (is_touched[s]) touched[n_touched++] = s;

  /* (8) the rows */
  if (n_bad > 0)
    for (int s = 0; s < n; ++s) {
      if ((kf_flags[s] & 1u) && mutate != 9) continue;
      for (int k = 0; k < kp_stride; ++k) {
        const int p = rows[(size_t)s * kp_stride + k];
        if (p >= 0 && p < n_table && newly_bad[p]) rows[(size_t)s * kp_stride + k] = -1;
      }
    }

  hdr[SPFE_CULL_OFF_STATUS / 4] = status;
  hdr[SPFE_CULL_OFF_N_LISTED / 4] = n_listed;
  hdr[SPFE_CULL_OFF_N_PASSES / 4] = n_passes;
  hdr[SPFE_CULL_OFF_N_CULLED / 4] = n_culled;
  hdr[SPFE_CULL_OFF_N_DEFERRED / 4] = n_deferred;
  hdr[SPFE_CULL_OFF_N_TOUCHED / 4] = n_touched;
  hdr[SPFE_CULL_OFF_N_REPARENTED / 4] = n_reparented;
  hdr[SPFE_CULL_OFF_N_EVENTS / 4] = n_reparented < n ? n_reparented : n;
  hdr[SPFE_CULL_OFF_N_BAD / 4] = n_bad;
  hdr[SPFE_CULL_OFF_N_BAD_STORED / 4] = n_bad < bad_cap ? n_bad : bad_cap;
  free(live);
  free(newly_bad);
  free(cnt);
  free(key);
  free(is_touched);
  free(cand);
  free(child);
  free(cull_idx);
}

/* the macros as this file sees them: offsets for (n_slots, conn_cap, bad_cap), status bits, flag bits and codes */
EXPORT void cull_ref_layout(int n_slots, int conn_cap, int bad_cap, int64_t *v) {
  v[0] = SPFE_CULL_OFF_ENTRY_SLOT;
  v[1] = (int64_t)SPFE_CULL_OFF_ENTRY_CODE(conn_cap);
  v[2] = (int64_t)SPFE_CULL_OFF_ENTRY_PASS(conn_cap);
  v[3] = (int64_t)SPFE_CULL_OFF_ENTRY_MPS(conn_cap);
  v[4] = (int64_t)SPFE_CULL_OFF_ENTRY_RED(conn_cap);
  v[5] = (int64_t)SPFE_CULL_OFF_CULLED_SLOT(conn_cap);
  v[6] = (int64_t)SPFE_CULL_OFF_TOUCHED_SLOT(conn_cap);
  v[7] = (int64_t)SPFE_CULL_OFF_EVENT_CHILD(n_slots, conn_cap);
  v[8] = (int64_t)SPFE_CULL_OFF_EVENT_PARENT(n_slots, conn_cap);
  v[9] = (int64_t)SPFE_CULL_OFF_BAD_POINT(n_slots, conn_cap);
  v[10] = (int64_t)SPFE_CULL_OUT_BYTES(n_slots, conn_cap, bad_cap);
  v[11] = SPFE_CULL_STALLED;
  v[12] = SPFE_CULL_WILD_ENTRY;
  v[13] = SPFE_CULL_BAD_CUT;
  v[14] = SPFE_CULL_EVENT_CUT;
  v[15] = SPFE_CULL_NO_PARENT;
  v[16] = SPFE_KF_NOT_ERASE;
  v[17] = SPFE_KF_TO_BE_ERASED;
  v[18] = SPFE_MP_MAX_POINTS;
}
