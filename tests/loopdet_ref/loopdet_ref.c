/* loopdet_ref.c — host reference of the loop detection: LoopClosingVLAD::detectLoopCandidates and the minimum score of
 * detectLoopVLAD for one query keyframe, as the plain sequential statement — one loop over the slots per step, lists filled in
 * order — on the arithmetic of include/spfe_loopdet_math.h (the header the GPU kernels share).  It writes the whole output block
 * of include/spfe.h.  Compile with -ffp-contract=off.
 * `mutate` switches ONE rule to a wrong one, so that the tests can show that the fixtures tell the difference:
 *   1 `>=` for `>` in the retrieval   2 connected keyframes not excluded   3 bad keyframes excluded in the retrieval   4 the best
 *   keyframe taken over on `>=`   5 acc without the entry's own score   6 best_acc_score started at 0   7 the last occurrence of a
 *   best keyframe kept   8 nine neighbours   9 the floor ignored */
#include <limits.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spfe.h"
#include "../../include/spfe_loopdet_math.h"

#define EXPORT __attribute__((visibility("default")))

EXPORT float loopdet_ref_dot(const float *a, const float *b, int dim) { return spfe_ld_dot(a, b, dim); }

EXPORT void loopdet_ref_detect(const float *gdesc, int dim, const uint8_t *kf_flags, const uint8_t *in_db, const int32_t *best_cov,
                               int n, int cur_slot, const int32_t *connected, int n_conn, const int32_t *covisible, int n_cov,
                               float min_score_init, float min_score_floor, float retain_ratio, uint8_t *out, int mutate) {
  int32_t *hdr = (int32_t *)out;
  float *hf = (float *)(out + SPFE_LOOPDET_OFF_COV_MIN_SCORE);
  float *score = (float *)(out + SPFE_LOOPDET_OFF_SCORE);
  int32_t *pass_slot = (int32_t *)(out + SPFE_LOOPDET_OFF_PASS_SLOT(n));
  float *acc_score = (float *)(out + SPFE_LOOPDET_OFF_ACC_SCORE(n));
  int32_t *best_slot = (int32_t *)(out + SPFE_LOOPDET_OFF_BEST_SLOT(n));
  int32_t *cand_slot = (int32_t *)(out + SPFE_LOOPDET_OFF_CAND_SLOT(n));
  float *cand_acc = (float *)(out + SPFE_LOOPDET_OFF_CAND_ACC(n));
  int32_t *first_pos = (int32_t *)(out + SPFE_LOOPDET_OFF_FIRST_POS(n));
  uint8_t *role = out + SPFE_LOOPDET_OFF_ROLE(n);
  const float *query = gdesc + (size_t)cur_slot * dim;
  int status = 0, n_scored = 0, n_pass = 0, n_cand = 0;

  /* roles */
  for (int s = 0; s < n; ++s) {
    role[s] = (in_db[s] && s != cur_slot) ? SPFE_LOOPDET_ROLE_DB : 0;
    if (mutate == 3 && (kf_flags[s] & 1)) role[s] = 0;
  }
  for (int i = 0; i < n_conn; ++i) {
    const int s = connected[i];
    if (s < 0 || s >= n) {
      status |= SPFE_LOOPDET_BAD_LIST_INDEX;
      continue;
    }
    if (mutate != 2) role[s] &= (uint8_t)~SPFE_LOOPDET_ROLE_DB;
  }
  for (int i = 0; i < n_cov; ++i) {
    const int s = covisible[i];
    if (s < 0 || s >= n) {
      status |= SPFE_LOOPDET_BAD_LIST_INDEX;
      continue;
    }
    if (!(kf_flags[s] & 1)) role[s] |= SPFE_LOOPDET_ROLE_COV;
  }

  /* scores */
  for (int s = 0; s < n; ++s) {
    if (role[s]) {
      score[s] = spfe_ld_dot(query, gdesc + (size_t)s * dim, dim);
      ++n_scored;
    } else {
      const uint32_t none = SPFE_LOOPDET_NO_SCORE_BITS;
      memcpy(&score[s], &none, 4);
    }
  }

  /* the minimum score */
  float cov_min = spfe_ld_inf();
  for (int s = 0; s < n; ++s)
    if ((role[s] & SPFE_LOOPDET_ROLE_COV) && spfe_ld_lowers(score[s], cov_min)) cov_min = score[s];
  float min_score = spfe_ld_min_score(min_score_init, cov_min, min_score_floor);
  if (mutate == 9) min_score = spfe_ld_lowers(cov_min, min_score_init) ? cov_min : min_score_init;

  /* the retrieval */
  uint8_t *kept = (uint8_t *)calloc((size_t)n, 1);
  for (int s = 0; s < n; ++s) {
    if (!(role[s] & SPFE_LOOPDET_ROLE_DB)) continue;
    if (mutate == 1 ? score[s] >= min_score : spfe_ld_passes(score[s], min_score)) {
      kept[s] = 1;
      pass_slot[n_pass++] = s;
    }
  }

  /* accumulation over the best covisibles */
  float best_acc = mutate == 6 ? 0.0f : min_score;
  const int neigh = mutate == 8 ? SPFE_LOOPDET_NEIGH - 1 : SPFE_LOOPDET_NEIGH;
  for (int p = 0; p < n_pass; ++p) {
    const int s = pass_slot[p];
    float best = score[s], acc = mutate == 5 ? 0.0f : score[s];
    int bs = s;
    for (int k = 0; k < neigh; ++k) {
      const int nb = best_cov[(size_t)s * SPFE_LOOPDET_NEIGH + k];
      if (nb < 0 || nb >= n) {
        if (nb != -1) status |= SPFE_LOOPDET_BAD_NEIGHBOUR;
        continue;
      }
      if (!kept[nb]) continue;
      acc = acc + score[nb];
      if (mutate == 4 ? score[nb] >= best : spfe_ld_raises(score[nb], best)) {
        best = score[nb];
        bs = nb;
      }
    }
    acc_score[p] = acc;
    best_slot[p] = bs;
    if (spfe_ld_raises(acc, best_acc)) best_acc = acc;
  }

  /* the candidates */
  const float retain = spfe_ld_retain(retain_ratio, best_acc);
  for (int s = 0; s < n; ++s) first_pos[s] = INT_MAX;
  for (int p = 0; p < n_pass; ++p)
    if (spfe_ld_passes(acc_score[p], retain) && p < first_pos[best_slot[p]]) first_pos[best_slot[p]] = p;
  for (int p = 0; p < n_pass; ++p) {
    if (!spfe_ld_passes(acc_score[p], retain)) continue;
    int emit = first_pos[best_slot[p]] == p;
    if (mutate == 7) {
      emit = 1;
      for (int q = p + 1; q < n_pass; ++q)
        if (spfe_ld_passes(acc_score[q], retain) && best_slot[q] == best_slot[p]) emit = 0;
    }
    if (emit) {
      cand_slot[n_cand] = best_slot[p];
      cand_acc[n_cand] = acc_score[p];
      ++n_cand;
    }
  }
  free(kept);

  hdr[0] = status;
  hdr[1] = n_scored;
  hdr[2] = n_pass;
  hdr[3] = n_cand;
  hf[0] = cov_min;
  hf[1] = min_score;
  hf[2] = best_acc;
  hf[3] = retain;
}
