/* sim3_ref.c — host reference of the verification of one loop candidate (pair list, hypotheses, the rule of the returns), built
 * from include/spfe_sim3_math.h: the sequence of operations the GPU kernels (sp_orb_slam_amd/csrc/sim3.hip) evaluate, in plain
 * C loops, written into the block of include/spfe.h (SPFE_SIM3_OFF_*).  -DSIM3_MUTATION=k compiles a deliberately wrong
 * variant that the fixtures of tests/golden/sim3_*.npz must reject. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spfe.h"
#include "../../include/spfe_sim3_math.h"

#define EXPORT __attribute__((visibility("default")))

#ifndef SIM3_MUTATION
#define SIM3_MUTATION 0
#endif
#define MUT_BEST_GT 1      /* > for >= in the update of the best */
#define MUT_MIN_GE 2       /* >= for > against min_inliers */
#define MUT_TH_921 3       /* thresholds 9.21 instead of the truncated 9 */
#define MUT_ONE_DIRECTION 4 /* only the error in image 1 */
#define MUT_NO_REMOVAL 5   /* every draw from 0 .. N-1 */
#define MUT_SCALE_ONE 6    /* scale forced to 1 */

EXPORT int sim3_ref_mutation(void) { return SIM3_MUTATION; }
EXPORT int sim3_ref_default_sweeps(void) { return SPFE_SIM3_JACOBI_SWEEPS; }
EXPORT size_t sim3_ref_out_bytes(int kcap, int n_hyp) { return SPFE_SIM3_OUT_BYTES(kcap, n_hyp); }
EXPORT void sim3_ref_offsets(int kcap, int n_hyp, size_t *o) {
  o[0] = SPFE_SIM3_OFF_N; o[1] = SPFE_SIM3_OFF_N_RETURNS; o[2] = SPFE_SIM3_OFF_BEST_H; o[3] = SPFE_SIM3_OFF_BEST_COUNT;
  o[4] = SPFE_SIM3_OFF_N_HYP; o[5] = SPFE_SIM3_OFF_K1; o[6] = SPFE_SIM3_OFF_COUNT(kcap);
  o[7] = SPFE_SIM3_OFF_RETURN_IDX(kcap, n_hyp); o[8] = SPFE_SIM3_OFF_T12(kcap, n_hyp); o[9] = SPFE_SIM3_OFF_INLIERS(kcap, n_hyp);
  o[10] = SPFE_SIM3_OUT_BYTES(kcap, n_hyp); o[11] = SPFE_SIM3_WORDS(kcap);
  o[12] = SPFE_SIM3_MAX_CANDIDATES; o[13] = SPFE_SIM3_MAX_HYPOTHESES;
}

/* One candidate.  The index arrays have kcap entries, K1 <= kcap keypoints of keyframe 1 are walked.  err (or NULL):
 * [n_hyp][kcap][2] receives err1, err2 of every pair.  Returns N. */
EXPORT int sim3_ref_run(int kcap, int K1, const int32_t *match12, const int32_t *mp1, const int32_t *mp2, const float *xyz,
                        const uint8_t *flags, int n, const float *Tcw1, const float *Tcw2, const uint32_t *rnd, int n_hyp,
                        const spfe_sim3_params *prm, int sweeps, uint8_t *out, float *err) {
  int32_t *fld = (int32_t *)out;
  int32_t *k1_list = (int32_t *)(out + SPFE_SIM3_OFF_K1), *count = (int32_t *)(out + SPFE_SIM3_OFF_COUNT(kcap));
  int32_t *ret = (int32_t *)(out + SPFE_SIM3_OFF_RETURN_IDX(kcap, n_hyp));
  float *T12s = (float *)(out + SPFE_SIM3_OFF_T12(kcap, n_hyp));
  uint64_t *bits = (uint64_t *)(out + SPFE_SIM3_OFF_INLIERS(kcap, n_hyp));
  const int words = (int)SPFE_SIM3_WORDS(kcap);
  float *scr = (float *)malloc((size_t)(kcap > 0 ? kcap : 1) * 10 * sizeof(float));
  int N = 0;
  for (int k1 = 0; k1 < K1; ++k1) {
    const int k2 = match12[k1];
    if (k2 < 0 || k2 >= kcap) continue;
    const int p1 = mp1[k1], p2 = mp2[k2];
    if (p1 < 0 || p1 >= n || p2 < 0 || p2 >= n) continue;
    if (!(flags[p1] & SPFE_PROJ_SEARCHABLE) || !(flags[p2] & SPFE_PROJ_SEARCHABLE)) continue;
    float *p = scr + (size_t)N * 10;
    spfe_sim3_to_cam(Tcw1, xyz + 3 * p1, p);
    spfe_sim3_to_cam(Tcw2, xyz + 3 * p2, p + 3);
    spfe_sim3_image(prm->fx1, prm->fy1, prm->cx1, prm->cy1, p, p + 6);
    spfe_sim3_image(prm->fx2, prm->fy2, prm->cx2, prm->cy2, p + 3, p + 8);
    k1_list[N++] = k1;
  }
  fld[0] = N;
  fld[4] = n_hyp;
  const int floor_n = prm->min_inliers > 3 ? prm->min_inliers : 3;
  if (N < floor_n) {
    fld[1] = 0; fld[2] = -1; fld[3] = 0;
    for (int h = 0; h < n_hyp; ++h) count[h] = 0;
    free(scr);
    return N;
  }
  float th1 = prm->max_err1, th2 = prm->max_err2;
  if (SIM3_MUTATION == MUT_TH_921) th1 = th2 = 9.21f;
  int best = 0, best_h = -1, n_ret = 0;   /* mnBestInliers = 0 */
  for (int h = 0; h < n_hyp; ++h) {
    int idx[3];
    spfe_sim3_draws(rnd + 3 * h, N, SIM3_MUTATION != MUT_NO_REMOVAL, idx);
    float P1[9], P2[9];
    for (int i = 0; i < 3; ++i)
      for (int r = 0; r < 3; ++r) {
        P1[3 * r + i] = scr[(size_t)idx[i] * 10 + r];
        P2[3 * r + i] = scr[(size_t)idx[i] * 10 + 3 + r];
      }
    spfe_sim3_T T;
    spfe_sim3_horn(P1, P2, prm->fix_scale || SIM3_MUTATION == MUT_SCALE_ONE, sweeps, &T);
    float A12[12], A21[12];
    spfe_sim3_forms(&T, A12, A21);
    uint64_t *row = bits + (size_t)h * words;
    for (int b = 0; b < words; ++b) row[b] = 0;
    int c = 0;
    for (int i = 0; i < N; ++i) {
      const float *p = scr + (size_t)i * 10;
      const float e1 = spfe_sim3_err(A12, p + 3, prm->fx1, prm->fy1, prm->cx1, prm->cy1, p + 6);
      const float e2 = spfe_sim3_err(A21, p, prm->fx2, prm->fy2, prm->cx2, prm->cy2, p + 8);
      if (err) { err[((size_t)h * kcap + i) * 2] = e1; err[((size_t)h * kcap + i) * 2 + 1] = e2; }
      const int in = SIM3_MUTATION == MUT_ONE_DIRECTION ? e1 < th1 : (e1 < th1 && e2 < th2);
      if (in) { row[i >> 6] |= 1ull << (i & 63); ++c; }
    }
    count[h] = c;
    T12s[13 * h] = T.s;
    memcpy(T12s + 13 * h + 1, T.R, 36);
    memcpy(T12s + 13 * h + 10, T.t, 12);
    /* iterate() :184-199 */
    if (SIM3_MUTATION == MUT_BEST_GT ? c > best : c >= best) {
      best = c;
      best_h = h;
      if (SIM3_MUTATION == MUT_MIN_GE ? c >= prm->min_inliers : c > prm->min_inliers) ret[n_ret++] = h;
    }
  }
  fld[1] = n_ret; fld[2] = best_h; fld[3] = best;
  free(scr);
  return N;
}
