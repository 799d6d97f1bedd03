/* cull_ref_main.c — a stand-alone driver of cull_ref.c for the host sanitizers (tests/test_cull_reference.py builds both with
 * -fsanitize=address,undefined and runs the program): random worlds of every awkward shape — one slot, one-entry rows, a table of
 * no points, full neighbour maps, wild list entries, wild parents, bad_cap 0 — through cull_ref_count and cull_ref_run, every
 * mutation included, each array allocated at exactly its documented size so that a step past an end is a report. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spfe.h"

void cull_ref_count(const int32_t *rows, int kp_stride, const uint8_t *kf_flags, int n_slots, int32_t *nobs, int n_table);
void cull_ref_run(int32_t *rows, int kp_stride, uint8_t *kf_flags, uint8_t *mp_flags, int32_t *nobs, int n_table, int n_slots,
                  int conn_cap, int32_t *conn_slot, int32_t *conn_w, int32_t *conn_n, int32_t *ord_slot, int32_t *ord_w, int32_t *ord_n,
                  int32_t *parent, uint8_t *first_conn, int cur, int th_obs, float cov_ratio, int origin_slot, int bad_cap,
                  int32_t *best_a, int n_best_a, int32_t *best_b, int n_best_b, uint8_t *out, int mutate);

static uint32_t g_seed = 12345u;
static int rnd(int n) {
  g_seed = g_seed * 1664525u + 1013904223u;
  return (int)((g_seed >> 8) % (uint32_t)(n > 0 ? n : 1));
}

static void one(int n, int stride, int n_table, int cap, int bad_cap, int mutate) {
  int32_t *rows = malloc(sizeof(int32_t) * (size_t)n * stride), *nobs = malloc(sizeof(int32_t) * (size_t)(n_table ? n_table : 1));
  uint8_t *kf = malloc((size_t)n), *mp = malloc((size_t)(n_table ? n_table : 1)), *fc = malloc((size_t)n);
  int32_t *row_arr[4], *cnt[2], *parent = malloc(sizeof(int32_t) * (size_t)n);
  for (int i = 0; i < 4; ++i) row_arr[i] = malloc(sizeof(int32_t) * (size_t)n * cap);
  for (int i = 0; i < 2; ++i) cnt[i] = malloc(sizeof(int32_t) * (size_t)n);
  const int nba = 1 + rnd(32), nbb = 1 + rnd(32);
  int32_t *ta = malloc(sizeof(int32_t) * (size_t)n * nba), *tb = rnd(2) ? malloc(sizeof(int32_t) * (size_t)n * nbb) : NULL;
  uint8_t *out = malloc(SPFE_CULL_OUT_BYTES(n, cap, bad_cap));
  for (int i = 0; i < n * stride; ++i) rows[i] = rnd(8) ? rnd(n_table + 2) - 1 : -1;
  for (int s = 0; s < n; ++s) {
    kf[s] = (uint8_t)(rnd(10) == 0 ? 1 : (rnd(10) == 0 ? 2 : 0));
    fc[s] = 0;
    parent[s] = rnd(12) == 0 ? -1 : rnd(n + 1) - (rnd(20) == 0);
    const int cn = rnd(cap + 1) < n ? rnd(cap + 1) : 0;   /* ascending distinct slots */
    int at = 0;
    for (int t = 0; t < n && at < cn; ++t)
      if (rnd(2)) {
        row_arr[0][(size_t)s * cap + at] = t;
        row_arr[1][(size_t)s * cap + at] = 1 + rnd(30);
        ++at;
      }
    cnt[0][s] = at;
    const int on = rnd(at + 1);
    for (int i = 0; i < cap; ++i) {
      if (i >= at) row_arr[0][(size_t)s * cap + i] = -1, row_arr[1][(size_t)s * cap + i] = 0;
      row_arr[2][(size_t)s * cap + i] = i < on ? (rnd(15) == 0 ? n + 3 : row_arr[0][(size_t)s * cap + (at - 1 - i)]) : -1;
      row_arr[3][(size_t)s * cap + i] = i < on ? row_arr[1][(size_t)s * cap + (at - 1 - i)] : 0;
    }
    cnt[1][s] = on;
  }
  for (int p = 0; p < n_table; ++p) mp[p] = (uint8_t)(rnd(8) ? 1 : 0);
  cull_ref_count(rows, stride, kf, n, nobs, n_table);
  cull_ref_run(rows, stride, kf, mp, nobs, n_table, n, cap, row_arr[0], row_arr[1], cnt[0], row_arr[2], row_arr[3], cnt[1], parent, fc,
               rnd(n), 1 + rnd(4), (float)rnd(11) / 10.0f, rnd(n + 1) - 1, bad_cap, ta, nba, tb, nbb, out, mutate);
  free(rows); free(nobs); free(kf); free(mp); free(fc); free(parent); free(ta); free(tb); free(out);
  for (int i = 0; i < 4; ++i) free(row_arr[i]);
  for (int i = 0; i < 2; ++i) free(cnt[i]);
}

int main(void) {
  static const int shapes[][5] = {{1, 1, 0, 1, 0}, {2, 1, 1, 1, 1}, {7, 3, 5, 2, 0}, {33, 17, 60, 8, 3}, {64, 40, 300, 64, 500}, {9, 5, 40, 16, 2}};
  int runs = 0;
  for (int rep = 0; rep < 60; ++rep)
    for (unsigned i = 0; i < sizeof(shapes) / sizeof(shapes[0]); ++i)
      for (int m = 0; m <= 10; ++m, ++runs) one(shapes[i][0], shapes[i][1], shapes[i][2], shapes[i][3], shapes[i][4], m);
  printf("cull_ref_main: %d runs\n", runs);
  return 0;
}
