/* covis_ref.c — the host reference of the covisibility graph: a sequential restatement of
 *   KeyFrame::UpdateConnections                     orb_slam2/src/type/keyframe.cpp:757-849
 *   KeyFrame::AddConnection / UpdateBestCovisibles  orb_slam2/src/type/keyframe.cpp:577-612
 * on the arrays of include/spfe.h ("the covisibility graph"), with the contract of include/spfe_covis_math.h.  It updates the
 * state and the two tables in place and writes the whole block of spfe_update_connections_resident, every byte; the GPU tests
 * compare all of it byte for byte.
 * `mutate` switches ONE line to a plausible misreading, so that tests/test_covis_reference.py can show that its cases tell them
 * apart:
 *   1 a re-sort on an equal weight                      6 a neighbour's ord from the entries at or above th only
 *   2 equal weights ordered by ascending slot           7 a re-parent on the second call
 *   3 the last instead of the first maximum             8 a parent given to origin_slot
 *   4 > for >= th                                       9 bad slots counted
 *   5 ord[cur] built from the whole map                10 cur_slot counted
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spfe.h"
#include "../../include/spfe_covis_math.h"
#include "../../include/spfe_localmap_math.h"

#define EXPORT __attribute__((visibility("default")))

typedef struct {
  int32_t *conn_slot, *conn_w, *conn_n, *ord_slot, *ord_w, *ord_n, *parent;
  uint8_t *first_conn;
} state_t;

static int g_mutate;

static int key_desc(const void *pa, const void *pb) {
  int64_t a = *(const int64_t *)pa, b = *(const int64_t *)pb;
  if (g_mutate == 2 && spfe_cv_key_w(a) == spfe_cv_key_w(b)) { const int64_t t = a; a = b; b = t; }
  return a > b ? -1 : (a < b ? 1 : 0);
}

/* ord row and table rows of `slot` from n keys (sorted here) */
static void write_ord(const state_t *st, int cap, int slot, int64_t *key, int n, int whole_row, int32_t *best_a, int n_best_a,
                      int32_t *best_b, int n_best_b) {
  qsort(key, (size_t)n, sizeof(int64_t), key_desc);
  int32_t *os = st->ord_slot + (size_t)slot * cap, *ow = st->ord_w + (size_t)slot * cap;
  for (int i = 0; i < (whole_row ? cap : n); ++i) {
    os[i] = i < n ? spfe_cv_key_slot(key[i]) : -1;
    ow[i] = i < n ? spfe_cv_key_w(key[i]) : 0;
  }
  st->ord_n[slot] = n;
  if (best_a)
    for (int j = 0; j < n_best_a; ++j) best_a[(size_t)slot * n_best_a + j] = j < n ? spfe_cv_key_slot(key[j]) : -1;
  if (best_b)
    for (int j = 0; j < n_best_b; ++j) best_b[(size_t)slot * n_best_b + j] = j < n ? spfe_cv_key_slot(key[j]) : -1;
}

EXPORT void covis_ref_reset(int n_slots, int conn_cap, int32_t *conn_slot, int32_t *conn_w, int32_t *conn_n, int32_t *ord_slot,
                            int32_t *ord_w, int32_t *ord_n, int32_t *parent, uint8_t *first_conn, int first_slot, int n) {
  (void)n_slots;
  for (int s = first_slot; s < first_slot + n; ++s) {
    for (int i = 0; i < conn_cap; ++i) {
      conn_slot[(size_t)s * conn_cap + i] = -1;
      conn_w[(size_t)s * conn_cap + i] = 0;
      ord_slot[(size_t)s * conn_cap + i] = -1;
      ord_w[(size_t)s * conn_cap + i] = 0;
    }
    conn_n[s] = 0;
    ord_n[s] = 0;
    parent[s] = -1;
    first_conn[s] = 1;
  }
}

EXPORT void covis_ref_update(const int32_t *rows, int kp_stride, const uint8_t *kf_flags, const uint8_t *mp_flags, int n_table,
                             int n_slots, int conn_cap, int32_t *conn_slot, int32_t *conn_w, int32_t *conn_n, int32_t *ord_slot,
                             int32_t *ord_w, int32_t *ord_n, int32_t *parent, uint8_t *first_conn, int cur, int th, int origin_slot,
                             int32_t *best_a, int n_best_a, int32_t *best_b, int n_best_b, uint8_t *out, int mutate) {
  const int n = n_slots, cap = conn_cap;
  const state_t st = {conn_slot, conn_w, conn_n, ord_slot, ord_w, ord_n, parent, first_conn};
  g_mutate = mutate;
  memset(out, 0, SPFE_COVIS_OUT_BYTES(n, cap));
  int32_t *hdr = (int32_t *)out;
  int32_t *counter = (int32_t *)(out + SPFE_COVIS_OFF_COUNTER);
  int32_t *linked_slot = (int32_t *)(out + SPFE_COVIS_OFF_LINKED_SLOT(n));
  int32_t *linked_code = (int32_t *)(out + SPFE_COVIS_OFF_LINKED_CODE(n, cap));
  for (int j = 0; j < cap; ++j) linked_slot[j] = linked_code[j] = -1;
  hdr[SPFE_COVIS_OFF_PARENT_SET / 4] = -1;

  /* (1) the weight of a point = the entries of the current row that hold it, capped; the counter = the weights a row sums */
  int *count = (int *)calloc((size_t)(n_table > 0 ? n_table : 1), sizeof(int));
  const int32_t *row = rows + (size_t)cur * kp_stride;
  for (int k = 0; k < kp_stride; ++k)
    if (spfe_lm_in_table(row[k], n_table) && (mp_flags[row[k]] & SPFE_PROJ_SEARCHABLE)) count[row[k]]++;
  for (int s = 0; s < n; ++s) {
    int v = 0;
    for (int k = 0; k < kp_stride; ++k) {
      const int p = rows[(size_t)s * kp_stride + k];
      if (spfe_lm_in_table(p, n_table)) v += spfe_lm_weight(spfe_lm_table_byte(mp_flags[p], count[p]));
    }
    counter[s] = spfe_cv_counter(v, s, mutate == 10 ? -1 : cur, mutate == 9 ? 0u : kf_flags[s]);
  }
  free(count);

  /* (2), (3) */
  int nc = 0, na = 0, max_count = 0, max_slot = -1;
  for (int s = 0; s < n; ++s) {
    const int c = counter[s];
    nc += c > 0;
    na += mutate == 4 ? c > th : c >= th;
    if (mutate == 3 ? (c > 0 && c >= max_count) : spfe_cv_max_beats(c, s, max_count, max_slot)) {
      max_count = c;
      max_slot = s;
    }
  }
  hdr[SPFE_COVIS_OFF_N_COUNTER / 4] = nc;
  hdr[SPFE_COVIS_OFF_MAX_SLOT / 4] = max_slot;
  hdr[SPFE_COVIS_OFF_MAX_COUNT / 4] = max_count;
  if (nc == 0 || nc > cap) {
    hdr[SPFE_COVIS_OFF_STATUS / 4] = nc == 0 ? SPFE_COVIS_NO_SHARED : SPFE_COVIS_CUR_OVERFLOW;
    return;
  }
  const int th_p = mutate == 4 ? th + 1 : th;
  int64_t *key = (int64_t *)malloc(sizeof(int64_t) * (size_t)(cap + 1));
  int64_t *pkey = (int64_t *)malloc(sizeof(int64_t) * (size_t)(cap + 1));
  int n_linked = 0, n_changed = 0, n_overflow = 0, status = 0;

  /* (4) the neighbours, in slot order */
  for (int s = 0; s < n; ++s) {
    const int c = counter[s];
    if (c <= 0 || !spfe_cv_linked(c, s, th_p, na, max_slot)) continue;
    linked_slot[n_linked] = s;
    pkey[n_linked] = spfe_cv_key(c, s);
    int32_t *cs = conn_slot + (size_t)s * cap, *cw = conn_w + (size_t)s * cap;
    const int cn = conn_n[s];
    int found = -1, pos = 0;
    for (int i = 0; i < cn; ++i) {
      if (cs[i] == cur) found = i;
      pos += cs[i] < cur;
    }
    const int code = spfe_cv_add_code(found >= 0, found >= 0 ? cw[found] : 0, c, cn, cap);
    linked_code[n_linked++] = code;
    if (code == SPFE_COVIS_CODE_REPLACED) {
      cw[found] = c;
    } else if (code == SPFE_COVIS_CODE_INSERTED) {
      for (int i = cn; i > pos; --i) {
        cs[i] = cs[i - 1];
        cw[i] = cw[i - 1];
      }
      cs[pos] = cur;
      cw[pos] = c;
      conn_n[s] = cn + 1;
    } else if (code == SPFE_COVIS_CODE_FULL) {
      n_overflow++;
      status |= SPFE_COVIS_NEIGH_OVERFLOW;
    }
    if (code == SPFE_COVIS_CODE_REPLACED || code == SPFE_COVIS_CODE_INSERTED || (mutate == 1 && code == SPFE_COVIS_CODE_SAME)) {
      int m = 0;
      for (int i = 0; i < conn_n[s]; ++i)
        if (mutate != 6 || cw[i] >= th) key[m++] = spfe_cv_key(cw[i], cs[i]);
      write_ord(&st, cap, s, key, m, 0, best_a, n_best_a, best_b, n_best_b);
      n_changed += code != SPFE_COVIS_CODE_SAME;
    }
  }

  /* (5) the current keyframe: both rows whole */
  int32_t *cs = conn_slot + (size_t)cur * cap, *cw = conn_w + (size_t)cur * cap;
  int m = 0;
  for (int s = 0; s < n; ++s)
    if (counter[s] > 0) {
      cs[m] = s;
      cw[m] = counter[s];
      if (mutate == 5) pkey[m] = spfe_cv_key(counter[s], s);
      ++m;
    }
  for (int i = m; i < cap; ++i) {
    cs[i] = -1;
    cw[i] = 0;
  }
  conn_n[cur] = nc;
  write_ord(&st, cap, cur, pkey, mutate == 5 ? m : n_linked, 1, best_a, n_best_a, best_b, n_best_b);

  /* (6) */
  if ((first_conn[cur] || mutate == 7) && (cur != origin_slot || mutate == 8)) {
    parent[cur] = ord_slot[(size_t)cur * cap];
    first_conn[cur] = 0;
    hdr[SPFE_COVIS_OFF_PARENT_SET / 4] = parent[cur];
  }
  hdr[SPFE_COVIS_OFF_STATUS / 4] = status;
  hdr[SPFE_COVIS_OFF_N_LINKED / 4] = n_linked;
  hdr[SPFE_COVIS_OFF_N_CHANGED / 4] = n_changed;
  hdr[SPFE_COVIS_OFF_N_OVERFLOW / 4] = n_overflow;
  free(key);
  free(pkey);
}

/* the macros as this file sees them: offsets for (n_slots, conn_cap), status bits and limits */
EXPORT void covis_ref_layout(int n_slots, int conn_cap, int64_t *v) {
  v[0] = SPFE_COVIS_OFF_COUNTER;
  v[1] = (int64_t)SPFE_COVIS_OFF_LINKED_SLOT(n_slots);
  v[2] = (int64_t)SPFE_COVIS_OFF_LINKED_CODE(n_slots, conn_cap);
  v[3] = (int64_t)SPFE_COVIS_OUT_BYTES(n_slots, conn_cap);
  v[4] = SPFE_COVIS_NO_SHARED;
  v[5] = SPFE_COVIS_CUR_OVERFLOW;
  v[6] = SPFE_COVIS_NEIGH_OVERFLOW;
  v[7] = SPFE_COVIS_MAX_CONN;
  v[8] = SPFE_LOCALMAP_MAX_BEST;
}
