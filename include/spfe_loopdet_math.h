/*
 * spfe_loopdet_math.h — the arithmetic of the loop detection (the NetVLAD retrieval and the scoring of its candidates), shared by
 * the GPU kernels (sp_orb_slam_amd/csrc/loopdet.hip) and the host C reference of the test suite (tests/loopdet_ref/loopdet_ref.c)
 * so that both evaluate the same sequence of IEEE operations (compile with -ffp-contract=off).
 *
 * What it restates, in this project's own words:
 *   LoopClosingVLAD::detectLoopCandidates(minScore)   orb_slam2/src/loopclosing/loop_closer_vlad.cpp:42-118
 *   the minimum score of detectLoopVLAD               orb_slam2/src/loopclosing/loop_closer_vlad.cpp:150-165
 *
 * ---- (a) The score ------------------------------------------------------------------------------------------------------
 * The reference's score is cv::Mat::dot of two CV_32F rows: a double accumulation whose order depends on the OpenCV build.  HERE
 * the sum is defined.  For rows a, b of `dim` f32 (dim a multiple of 4, at most SPFE_LOOPDET_MAX_DIM):
 *   p[e]   = (double)a[e] * (double)b[e]                              exact: 24 x 24 bits fit 53
 *   s[t]   = 0.0 + p[e0] + p[e1] + ...   over the e with (e >> 2) & 255 == t, ascending       t = 0 .. 255
 *            (element e belongs to slot t: four consecutive elements a slot and pass of 1024, so that a thread's share of a row
 *            is 16-byte loads; a slot without an element stays 0.0)
 *   tree     for m = 128, 64, ..., 1:  s[l] = s[l] + s[l + m]  for l < m
 *   score  = (float)s[0]                                              rounded once
 *
 * ---- (b) The decisions, all on f32 as the reference writes them ------------------------------------------------------------
 *   cov_min     the least score over the covisible keyframes that are not bad: from +inf, `score < cov_min` takes over, in slot
 *               order (the value does not depend on the order; of -0 and +0 the one at the lower slot stays).  A NaN never
 *               lowers it.  +inf where there is none.
 *   min_score   m = min_score_init; cov_min < m lowers it; then std::max(m, min_score_floor): m < floor ? floor : m
 *   passes      score > min_score                                     a NaN never passes
 *   acc, best   acc = best = the entry's score; a neighbour that passed in this query adds its score (acc = acc + s, in the row's
 *               order) and becomes the best keyframe on s > best
 *   best_acc    from min_score, raised on acc > best_acc               a NaN never wins
 *   retain      retain_ratio * best_acc; an entry is retained on acc > retain; of the retained entries with the same best keyframe
 *               the first is the candidate
 */
#ifndef SPFE_LOOPDET_MATH_H
#define SPFE_LOOPDET_MATH_H

#if defined(__HIPCC__)
#define SPFE_LD __host__ __device__ static inline
#else
#define SPFE_LD static inline
#endif

#define SPFE_LOOPDET_TREE_SLOTS 256
#define SPFE_LOOPDET_MAX_DIM 4096
#define SPFE_LOOPDET_PASS_ELEMS (4 * SPFE_LOOPDET_TREE_SLOTS) /* the elements of one pass over the 256 slots */
/* role[s] of a keyframe slot in one query */
#define SPFE_LOOPDET_ROLE_DB 1  /* a member of the database that is not connected to the current keyframe (and not itself) */
#define SPFE_LOOPDET_ROLE_COV 2 /* a covisible keyframe that is not bad */

SPFE_LD double spfe_ld_prod(float a, float b) { return (double)a * (double)b; }
/* the four elements of slot t in the pass that starts at element `base` (base = 1024 p + 4 t), added to s in ascending order */
SPFE_LD double spfe_ld_add4(double s, const float a[4], const float b[4]) {
  s = s + spfe_ld_prod(a[0], b[0]);
  s = s + spfe_ld_prod(a[1], b[1]);
  s = s + spfe_ld_prod(a[2], b[2]);
  s = s + spfe_ld_prod(a[3], b[3]);
  return s;
}
/* s[t] of two whole rows */
SPFE_LD double spfe_ld_slot_sum(const float *a, const float *b, int dim, int t) {
  double s = 0.0;
  for (int base = 4 * t; base < dim; base += SPFE_LOOPDET_PASS_ELEMS) s = spfe_ld_add4(s, a + base, b + base);
  return s;
}
/* the whole sum, as the plain sequential statement */
SPFE_LD float spfe_ld_dot(const float *a, const float *b, int dim) {
  double s[SPFE_LOOPDET_TREE_SLOTS];
  for (int t = 0; t < SPFE_LOOPDET_TREE_SLOTS; ++t) s[t] = spfe_ld_slot_sum(a, b, dim, t);
  for (int m = SPFE_LOOPDET_TREE_SLOTS / 2; m >= 1; m >>= 1)
    for (int l = 0; l < m; ++l) s[l] = s[l] + s[l + m];
  return (float)s[0];
}

SPFE_LD float spfe_ld_inf(void) { return __builtin_inff(); }
SPFE_LD int spfe_ld_lowers(float score, float m) { return score < m; }
SPFE_LD int spfe_ld_passes(float score, float min_score) { return score > min_score; }
SPFE_LD float spfe_ld_min_score(float init, float cov_min, float floor_) {
  float m = init;
  if (spfe_ld_lowers(cov_min, m)) m = cov_min;
  return m < floor_ ? floor_ : m;
}
SPFE_LD int spfe_ld_raises(float v, float best) { return v > best; }
SPFE_LD float spfe_ld_retain(float ratio, float best_acc) { return ratio * best_acc; }

#endif /* SPFE_LOOPDET_MATH_H */
