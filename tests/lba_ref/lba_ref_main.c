/* lba_ref_main.c — a stand-alone driver of lba_ref.c for the host sanitizers (tests/test_lba_reference.py builds both with
 * -fsanitize=address,undefined and runs the program): random maps of every awkward shape — one slot, one-entry rows, a table of one
 * point, capacities of one, ord rows full of wild, repeated and bad entries, rows with wild entries — through the gather, then the
 * application of a solver's block with random erase lists (wild indices included) and, every few runs, of blocks whose counts, edges
 * and observations were overwritten with garbage; every mutation included, each array allocated at exactly its documented size so
 * that a step past an end is a report. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spfe.h"

void lba_ref_gather(const int32_t *ord_row, int conn_cap, const int32_t *rows, int kp_stride, const uint8_t *kf_flags, int n_slots,
                    const uint8_t *mp_flags, const float *xyz, int n_table, const float *Tcw, int cur_slot, int origin_slot, int kf_cap,
                    int free_cap, int point_cap, int edge_cap, uint8_t *out, int mutate);
void lba_ref_apply(const uint8_t *gather, const uint8_t *ba, int32_t *rows, int kp_stride, const uint8_t *kf_flags, int n_slots,
                   uint8_t *mp_flags, int32_t *nobs, int32_t *ref_slot, float *xyz, int n_table, float *Tcw, int kf_cap, int point_cap,
                   int edge_cap, int bad_cap, uint8_t *out, int mutate);

static uint32_t g_seed = 13579u;
static int rnd(int n) {
  g_seed = g_seed * 1664525u + 1013904223u;
  return (int)((g_seed >> 8) % (uint32_t)(n > 0 ? n : 1));
}

static void one(int n, int stride, int n_table, int conn_cap, int kf_cap, int free_cap, int point_cap, int edge_cap, int bad_cap, int mutate) {
  int32_t *rows = malloc(sizeof(int32_t) * (size_t)n * stride), *ord = malloc(sizeof(int32_t) * (size_t)conn_cap);
  int32_t *nobs = malloc(sizeof(int32_t) * (size_t)n_table), *ref = malloc(sizeof(int32_t) * (size_t)n_table);
  uint8_t *kf = malloc((size_t)n), *mf = malloc((size_t)n_table);
  float *xyz = malloc(12 * (size_t)n_table), *Tcw = malloc(64 * (size_t)n);
  for (int i = 0; i < n * stride; ++i) rows[i] = rnd(3) ? rnd(n_table + 2) - 1 : -1;
  for (int s = 0; s < n; ++s) kf[s] = (uint8_t)(rnd(7) == 0);
  for (int p = 0; p < n_table; ++p) mf[p] = (uint8_t)(rnd(7) ? 3 : 2), nobs[p] = rnd(6), ref[p] = rnd(n + 1) - 1;
  for (int i = 0; i < 3 * n_table; ++i) xyz[i] = (float)rnd(100);
  for (int i = 0; i < 16 * n; ++i) Tcw[i] = (float)rnd(100);
  for (int j = 0; j < conn_cap; ++j) ord[j] = rnd(12) ? rnd(n + 2) - (rnd(9) == 0) : (rnd(3) ? -1 : 1 << 30);
  const int cur = rnd(n), origin = rnd(3) ? rnd(n + 1) - 1 : cur;
  const size_t gb = SPFE_LBA_GATHER_BYTES(kf_cap, point_cap, edge_cap);
  uint8_t *g = malloc(gb);
  lba_ref_gather(ord, conn_cap, rows, stride, kf, n, mf, xyz, n_table, Tcw, cur, origin, kf_cap, free_cap, point_cap, edge_cap, g, mutate);
  int32_t *gh = (int32_t *)g;
  const int n_kf = gh[SPFE_LBA_OFF_N_KF / 4], np = gh[SPFE_LBA_OFF_N_POINTS / 4], E = gh[SPFE_LBA_OFF_N_EDGES / 4];
  /* the solver's block at exactly SPFE_BA_OUT_BYTES of the gather's counts */
  const size_t bb = SPFE_BA_OUT_BYTES(n_kf, np, E);
  uint8_t *ba = malloc(bb);
  memset(ba, 0xA5, bb);
  int32_t *bh = (int32_t *)ba;
  memset(ba, 0, 48);
  bh[SPFE_BA_OFF_N_KF / 4] = n_kf;
  bh[SPFE_BA_OFF_N_POINTS / 4] = np;
  bh[SPFE_BA_OFF_N_EDGES / 4] = E;
  bh[SPFE_BA_OFF_STATUS / 4] = rnd(6) ? (rnd(4) ? 0 : SPFE_BA_STATUS_STOPPED) : (0x100 << rnd(5));
  const int n_erase = rnd(E + 1);
  bh[SPFE_BA_OFF_N_ERASE / 4] = rnd(15) ? n_erase : (rnd(2) ? -1 : E + 1);
  for (int j = 0; j < n_erase; ++j) ((int32_t *)(ba + SPFE_BA_OFF_ERASE(n_kf, np, E)))[j] = rnd(20) ? rnd(E) : rnd(E + 3) - 1;
  for (int i = 0; i < 16 * n_kf; ++i) ((float *)(ba + SPFE_BA_OFF_TCW))[i] = (float)rnd(50);
  for (int i = 0; i < 3 * np; ++i) ((float *)(ba + SPFE_BA_OFF_XYZ(n_kf)))[i] = (float)rnd(50);
  if (rnd(4) == 0) {   /* garbage in what the application follows; the counts stay, so the solver's block keeps its size */
    int32_t *w = (int32_t *)(g + SPFE_LBA_OFF_KF_SLOT);
    const size_t words = (gb - SPFE_LBA_OFF_KF_SLOT) / 4;
    for (int t = 0; t < 12; ++t) w[rnd((int)words)] = rnd(2) ? rnd(1 << 20) - 5 : -rnd(1 << 20);
  }
  if (rnd(9) == 0) gh[1 + rnd(8)] = rnd(2) ? 1 << 28 : -3;   /* a wild count: refused, and then nothing behind the solver's header is read */
  uint8_t *a = malloc(SPFE_LBA_APPLY_BYTES(point_cap, edge_cap, bad_cap));
  const int wild_count = gh[SPFE_LBA_OFF_N_KF / 4] != n_kf || gh[SPFE_LBA_OFF_N_POINTS / 4] != np || gh[SPFE_LBA_OFF_N_EDGES / 4] != E;
  if (wild_count) {   /* the solver's block of such a call may be as short as its header */
    uint8_t *hdr_only = malloc(128);
    memcpy(hdr_only, ba, 128);
    free(ba);
    ba = hdr_only;
  }
  lba_ref_apply(g, ba, rows, stride, kf, n, mf, nobs, ref, xyz, n_table, Tcw, kf_cap, point_cap, edge_cap, bad_cap, a, mutate);
  free(rows); free(ord); free(nobs); free(ref); free(kf); free(mf); free(xyz); free(Tcw); free(g); free(ba); free(a);
}

int main(void) {
  /* n_slots, stride, n_table, conn_cap, kf_cap, free_cap, point_cap, edge_cap, bad_cap */
  static const int shapes[][9] = {{1, 1, 1, 1, 1, 1, 1, 1, 0}, {2, 1, 2, 1, 1, 1, 1, 2, 1},   {7, 3, 5, 4, 3, 2, 4, 9, 0},
                                  {33, 17, 60, 40, 12, 5, 30, 200, 3}, {64, 40, 300, 16, 128, 64, 400, 3000, 500}, {9, 5, 40, 300, 4, 4, 3, 6, 2}};
  int runs = 0;
  for (int rep = 0; rep < 40; ++rep)
    for (unsigned i = 0; i < sizeof(shapes) / sizeof(shapes[0]); ++i)
      for (int m = 0; m <= 11; ++m, ++runs)
        one(shapes[i][0], shapes[i][1], shapes[i][2], shapes[i][3], shapes[i][4], shapes[i][5], shapes[i][6], shapes[i][7], shapes[i][8], m);
  printf("lba_ref_main: %d runs\n", runs);
  return 0;
}
