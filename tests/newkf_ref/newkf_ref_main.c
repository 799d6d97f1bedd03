/* newkf_ref_main.c — a stand-alone driver of newkf_ref.c for the host sanitizers (tests/test_newkf_reference.py builds both with
 * -fsanitize=address,undefined and runs the program): random worlds of every awkward shape — one slot, one-entry rows, a table of
 * one point, frames of 0 keypoints and of as many as the row holds, wild and repeated entries, lists without an index array that run
 * past the table, capacities of 0 and one short, counts beyond the list's capacity, both record formats and neither — through the
 * insertion and the listing, every mutation included, each array allocated at exactly its documented size so that a step past an
 * end is a report. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spfe.h"

void newkf_ref_insert(const spfe_mp_life *l, const int32_t *frame, int n_kp, int cur_slot, int32_t *rows, int kp_stride, const uint8_t *kf_flags,
                      int n_slots, const uint8_t *rec_desc, int desc_bf16, float *desc_track, uint8_t *out, int mutate);
void newkf_ref_list(const int32_t *point_idx, int first_row, int m, const int32_t *rows, int kp_stride, const uint8_t *kf_flags, int n_slots,
                    const int32_t *mp_ref_slot, int n_table, int obs_cap, uint8_t *out, int mutate);

static uint32_t g_seed = 13579u;
static int rnd(int n) {
  g_seed = g_seed * 1664525u + 1013904223u;
  return (int)((g_seed >> 8) % (uint32_t)(n > 0 ? n : 1));
}
static int32_t entry(int n_table) { return rnd(3) ? rnd(n_table + 2) - 1 : (rnd(4) ? -1 : (rnd(2) ? INT32_MIN : INT32_MAX)); }

static void one(int n, int stride, int n_table, int cap, int m, int mutate) {
  spfe_mp_life l;
  memset(&l, 0, sizeof l);
  l.n_table = n_table;
  l.recent_cap = cap;
  uint8_t *flags = malloc((size_t)n_table), *kf = malloc((size_t)n);
  int32_t *nobs = malloc(sizeof(int32_t) * (size_t)n_table), *recent = malloc(sizeof(int32_t) * (size_t)cap), *recent_n = malloc(sizeof(int32_t));
  int32_t *rows = malloc(sizeof(int32_t) * (size_t)n * stride), *ref_slot = malloc(sizeof(int32_t) * (size_t)n_table);
  l.d_mp_flags = flags; l.d_mp_nobs = nobs; l.d_recent = recent; l.d_recent_n = recent_n;
  for (int i = 0; i < n * stride; ++i) rows[i] = entry(n_table);
  for (int s = 0; s < n; ++s) kf[s] = (uint8_t)(rnd(6) == 0);
  for (int p = 0; p < n_table; ++p) flags[p] = (uint8_t)(rnd(6) ? 0x81 : 2), nobs[p] = rnd(9), ref_slot[p] = rnd(n);
  for (int e = 0; e < cap; ++e) recent[e] = rnd(n_table);
  *recent_n = rnd(12) ? rnd(cap + 1) : (rnd(2) ? cap + 7 : -2);
  /* (O) on the rows as they are: with an index array and without */
  for (int with = 0; with < 2; ++with) {
    int32_t *pidx = with && m ? malloc(sizeof(int32_t) * (size_t)m) : NULL;
    for (int i = 0; pidx && i < m; ++i) pidx[i] = entry(n_table);
    const int obs_cap = rnd(3) ? rnd(2 * n * stride + 1) : 0;
    uint8_t *out = malloc(SPFE_LISTOBS_OUT_BYTES(m, obs_cap));
    newkf_ref_list(pidx, rnd(4) ? rnd(n_table + 1) : INT32_MAX - rnd(3), m, rows, stride, kf, n, ref_slot, n_table, obs_cap, out, mutate);
    free(out);
    free(pidx);
  }
  /* (I): the row empty three times in four, the slot good five times in six */
  const int cur = rnd(n), n_kp = rnd(3) ? rnd(stride + 1) : stride, fmt = rnd(3);   /* fmt 0: no record, 1: f32, 2: bf16 */
  if (rnd(4))
    for (int k = 0; k < stride; ++k) rows[(size_t)cur * stride + k] = rnd(5) ? -1 : -2 - rnd(9);
  int32_t *frame = n_kp ? malloc(sizeof(int32_t) * (size_t)n_kp) : NULL;
  for (int i = 0; i < n_kp; ++i) frame[i] = entry(n_table);
  const size_t row_b = fmt == 2 ? 512 : 1024;
  uint8_t *rec = fmt && n_kp ? malloc(row_b * (size_t)n_kp) : NULL;
  if (rec) memset(rec, 0x3C, row_b * (size_t)n_kp);
  float *track = rnd(4) ? malloc(sizeof(float) * 256 * (size_t)n_table) : NULL;
  if (track) memset(track, 0, sizeof(float) * 256 * (size_t)n_table);
  uint8_t *out = malloc(SPFE_NEWKF_OUT_BYTES(n_kp, stride));
  newkf_ref_insert(&l, frame, n_kp, cur, rows, stride, kf, n, rec, fmt == 2, track, out, mutate);
  free(out); free(track); free(rec); free(frame);
  free(flags); free(kf); free(nobs); free(recent); free(recent_n); free(rows); free(ref_slot);
}

int main(void) {
  /* n_slots, stride, n_table, recent_cap, m */
  static const int shapes[][5] = {{1, 1, 1, 1, 0}, {2, 1, 2, 1, 1}, {7, 3, 5, 2, 9}, {33, 17, 60, 8, 70}, {64, 40, 300, 64, 65}, {9, 5, 40, 300, 1025}};
  int runs = 0;
  for (int rep = 0; rep < 60; ++rep)
    for (unsigned i = 0; i < sizeof(shapes) / sizeof(shapes[0]); ++i)
      for (int m = 0; m <= 12; ++m, ++runs) one(shapes[i][0], shapes[i][1], shapes[i][2], shapes[i][3], shapes[i][4], m);
  printf("newkf_ref_main: %d runs\n", runs);
  return 0;
}
