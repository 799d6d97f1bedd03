/* mpcull_ref_main.c — a stand-alone driver of mpcull_ref.c for the host sanitizers (tests/test_mpcull_reference.py builds both with
 * -fsanitize=address,undefined and runs the program): random worlds of every awkward shape — one slot, one-entry rows, a table of
 * one point, a list of one entry, wild list entries, counts beyond the capacity, extreme keyframe ids, bad_cap 0, refused blocks
 * full of garbage, counts and ids out of range — through the reset, the admission, the statistics and the cull, every mutation
 * included, each array allocated at exactly its documented size so that a step past an end is a report. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spfe.h"

void mpcull_ref_reset(const spfe_mp_life *l, int first_row, int n_rows, int reset_list);
void mpcull_ref_admit(const spfe_mp_life *l, const uint8_t *tri, size_t tri_stride, int kmax, int n_neigh, const int32_t *neigh_slot,
                      int cur_slot, int cur_kf_id, int32_t *rows, int kp_stride, int n_slots, float *xyz, uint8_t *out, int mutate);
void mpcull_ref_stat(const spfe_mp_life *l, const int32_t *entry, const int32_t *after, int n_kp, const int32_t *point_idx, int point_cap,
                     const uint8_t *in_view, const uint8_t *outlier, uint8_t *out, int mutate);
void mpcull_ref_cull(const spfe_mp_life *l, int32_t *rows, int kp_stride, const uint8_t *kf_flags, int n_slots, int cur_kf_id, int th_obs,
                     float found_ratio, int bad_cap, uint8_t *out, int mutate);

static uint32_t g_seed = 24680u;
static int rnd(int n) {
  g_seed = g_seed * 1664525u + 1013904223u;
  return (int)((g_seed >> 8) % (uint32_t)(n > 0 ? n : 1));
}

static void one(int n, int stride, int n_table, int cap, int bad_cap, int kmax, int mutate) {
  spfe_mp_life l;
  int32_t *i32[5];
  l.n_table = n_table;
  l.recent_cap = cap;
  l.d_mp_flags = malloc((size_t)n_table);
  for (int i = 0; i < 4; ++i) i32[i] = malloc(sizeof(int32_t) * (size_t)n_table);
  l.d_mp_nobs = i32[0]; l.d_mp_found = i32[1]; l.d_mp_visible = i32[2]; l.d_mp_first_kf = i32[3];
  l.d_recent = malloc(sizeof(int32_t) * (size_t)cap);
  l.d_recent_n = malloc(sizeof(int32_t));
  int32_t *rows = malloc(sizeof(int32_t) * (size_t)n * stride);
  uint8_t *kf = malloc((size_t)n);
  float *xyz = malloc(sizeof(float) * 3 * (size_t)n_table);
  mpcull_ref_reset(&l, 0, n_table, 1);
  for (int i = 0; i < n * stride; ++i) rows[i] = rnd(3) ? rnd(n_table + 2) - 1 : -1;
  for (int s = 0; s < n; ++s) kf[s] = (uint8_t)(rnd(6) == 0);
  for (int p = 0; p < n_table; ++p) {
    ((uint8_t *)l.d_mp_flags)[p] = (uint8_t)(rnd(6) ? 3 : 2);
    i32[0][p] = rnd(5);
    i32[1][p] = rnd(4) ? rnd(9) : INT32_MAX - rnd(2);
    i32[2][p] = rnd(4) ? rnd(12) : INT32_MAX - rnd(2);
    i32[3][p] = rnd(8) ? 40 + rnd(12) : (rnd(2) ? INT32_MIN : INT32_MAX);
    xyz[3 * p] = xyz[3 * p + 1] = xyz[3 * p + 2] = 0.0f;
  }
  /* (A): blocks of exactly n_neigh * SPFE_TRI_OUT_BYTES(kmax) bytes of garbage, then headers and the entries below n_new */
  const int n_neigh = 1 + rnd(SPFE_TRI_MAX_NEIGHBOURS);
  const size_t tb = SPFE_TRI_OUT_BYTES(kmax);
  uint8_t *tri = malloc(tb * (size_t)n_neigh);
  int32_t *ns = malloc(sizeof(int32_t) * (size_t)n_neigh);
  memset(tri, 0xA5, tb * (size_t)n_neigh);
  int at = rnd(n_table + 1);
  const int cur_slot = rnd(n);
  for (int j = 0; j < n_neigh; ++j) {
    uint8_t *blk = tri + tb * (size_t)j;
    int32_t *h = (int32_t *)blk;
    ns[j] = rnd(20) ? (n > 1 ? (cur_slot + 1 + j) % n : 0) : rnd(n + 2) - 1;
    if (rnd(5) == 0) {
      h[SPFE_TRI_OFF_STATUS / 4] = 1;
      continue;
    }
    const int c = rnd(30) == 0 ? (rnd(2) ? -1 : kmax + 1) : rnd(kmax < 4 ? kmax + 1 : 4);
    memset(blk, 0, 36);
    h[SPFE_TRI_OFF_N_NEW / 4] = c;
    h[SPFE_TRI_OFF_POINT_BASE / 4] = rnd(25) ? at : (rnd(2) ? -3 : n_table);
    for (int t = 0; t < c && t < kmax; ++t) {
      ((int32_t *)(blk + SPFE_TRI_OFF_NEW_K1(kmax)))[t] = rnd(40) ? rnd(stride) : stride;
      ((int32_t *)(blk + SPFE_TRI_OFF_NEW_K2(kmax)))[t] = rnd(40) ? rnd(stride) : -1;
      for (int q = 0; q < 3; ++q) ((float *)(blk + SPFE_TRI_OFF_NEW_XYZ(kmax)))[3 * t + q] = (float)rnd(100);
    }
    at += c > 0 ? c : 0;
  }
  uint8_t *a_out = malloc(SPFE_ADMIT_OUT_BYTES);
  *(int32_t *)l.d_recent_n = rnd(cap + 1);
  mpcull_ref_admit(&l, tri, tb, kmax, n_neigh, ns, cur_slot, 50, rows, stride, n, xyz, a_out, mutate);
  /* (B) */
  const int n_kp = rnd(40), point_cap = 1 + rnd(50);
  int32_t *entry = malloc(sizeof(int32_t) * (size_t)(n_kp ? n_kp : 1)), *after = malloc(sizeof(int32_t) * (size_t)(n_kp ? n_kp : 1));
  int32_t *pidx = malloc(sizeof(int32_t) * (size_t)point_cap);
  uint8_t *view = malloc((size_t)point_cap), *outl = malloc((size_t)(n_kp ? n_kp : 1)), *s_out = malloc(SPFE_MPSTAT_OUT_BYTES);
  for (int k = 0; k < n_kp; ++k) entry[k] = rnd(n_table + 3) - 2, after[k] = rnd(n_table + 3) - 2, outl[k] = (uint8_t)(rnd(4) == 0);
  for (int i = 0; i < point_cap; ++i) pidx[i] = rnd(n_table + 3) - 2, view[i] = (uint8_t)rnd(2);
  for (int p = 0; p < n_table; ++p) {   /* counters beyond INT32_MAX are not served */
    if (i32[1][p] > INT32_MAX - 200) i32[1][p] = INT32_MAX - 200;
    if (i32[2][p] > INT32_MAX - 200) i32[2][p] = INT32_MAX - 200;
  }
  mpcull_ref_stat(&l, entry, after, n_kp, pidx, point_cap, view, outl, s_out, mutate);
  /* (C) */
  int32_t *recent = (int32_t *)l.d_recent;
  for (int e = 0; e < cap; ++e) recent[e] = rnd(10) ? rnd(n_table) : rnd(n_table + 4) - 2;
  *(int32_t *)l.d_recent_n = rnd(12) ? rnd(cap + 1) : (rnd(2) ? cap + 7 : -2);
  uint8_t *c_out = malloc(SPFE_MPCULL_OUT_BYTES(cap, bad_cap));
  mpcull_ref_cull(&l, rows, stride, kf, n, rnd(10) ? 50 + rnd(4) : INT32_MAX, rnd(4), (float)rnd(5) / 8.0f, bad_cap, c_out, mutate);
  free(l.d_mp_flags); free(l.d_recent); free(l.d_recent_n); free(rows); free(kf); free(xyz); free(tri); free(ns); free(a_out);
  free(entry); free(after); free(pidx); free(view); free(outl); free(s_out); free(c_out);
  for (int i = 0; i < 4; ++i) free(i32[i]);
}

int main(void) {
  /* n_slots, stride, n_table, recent_cap, bad_cap, kmax */
  static const int shapes[][6] = {{1, 1, 1, 1, 0, 1}, {2, 1, 2, 1, 1, 2}, {7, 3, 5, 2, 0, 3}, {33, 17, 60, 8, 3, 10}, {64, 40, 300, 64, 500, 100},
                                  {9, 5, 40, 300, 2, 7}};
  int runs = 0;
  for (int rep = 0; rep < 60; ++rep)
    for (unsigned i = 0; i < sizeof(shapes) / sizeof(shapes[0]); ++i)
      for (int m = 0; m <= 11; ++m, ++runs) one(shapes[i][0], shapes[i][1], shapes[i][2], shapes[i][3], shapes[i][4], shapes[i][5], m);
  printf("mpcull_ref_main: %d runs\n", runs);
  return 0;
}
