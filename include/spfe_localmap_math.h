/*
 * spfe_localmap_math.h — the contract of the local map on the device (keyframe votes, expansion, ordered point list), shared by
 * the GPU kernels (sp_orb_slam_amd/csrc/localmap.hip) and the host C reference of the test suite
 * (tests/localmap_ref/localmap_ref.c).  Integers only: every output is equal byte for byte whatever the order of evaluation.
 *
 * What it restates, in this project's own words:
 *   Tracking::UpdateLocalKeyFrames   orb_slam2/src/tracking/tracker.cpp:868-984
 *   Tracking::UpdateLocalPoints      orb_slam2/src/tracking/tracker.cpp:843-866
 *   KeyFrame::getTrackedInCommon     orb_slam2/src/map/keyframe.cpp:697-724   (the same count, with total_obs)
 *
 * ---- (1) Frame clean-up and weights (:889-903) ---------------------------------------------------------------------------
 *   A keypoint HOLDS point p when p = mp_of_kp[k] lies in [0, n_table) and mp_flags[p] has SPFE_PROJ_SEARCHABLE (and, in the
 *   count form, the keypoint is not an outlier).  Every other keypoint holds nothing from here on.
 *   count[p] = the number of keypoints that hold p (a point held twice counts twice, as keyframeCounter[..]++ runs twice);
 *   w[p] = min(count[p], SPFE_LOCALMAP_MAX_WEIGHT): the weight table is one byte a point, whose top bit says SEARCHABLE.  The
 *   reference has no such limit; more than 127 keypoints of ONE frame on one point is no state a tracker reaches.
 * ---- (2) Votes -------------------------------------------------------------------------------------------------------------
 *   votes[s] = sum over k < kp_stride of w[row s][k],  total[s] = the entries of row s that name a SEARCHABLE point; an entry
 *   outside [0, n_table) names nothing.  Bad keyframes are counted like the others.
 * ---- (3) Voted set V (:915-930) ----------------------------------------------------------------------------------------------
 *   V = the slots with votes > 0 and bit 0 of kf_flags clear, ASCENDING (the reference walks a std::map keyed by heap address:
 *   slot order is this project's statement of it).  ref_slot = the first of V with the strictly greatest vote, -1 for none.
 *   V empty: status SPFE_LOCALMAP_NO_VOTES, no local keyframes.
 * ---- (4) Expansion (:932-978), sequential ---------------------------------------------------------------------------------
 *   L = V, all of V marked.  For i = 0 .. |V| - 1 (V as it stood):
 *     |L| > max_keyframes: stop.
 *     the first j < n_best with s = best_cov[V[i]][j] in [0, n_slots), not bad, not marked: push, mark; at most one.  Entries in
 *       front of it outside [-1, n_slots) set SPFE_LOCALMAP_BAD_SLOT and are skipped.
 *     the lowest slot c with parent[c] == V[i], not bad, not marked: push, mark; at most one.
 *     p = parent[V[i]]: outside [-1, n_slots) sets SPFE_LOCALMAP_BAD_SLOT; in [0, n_slots) and not marked: push, mark and END THE
 *       WHOLE LOOP (the break at :975 leaves the outer for).  The parent is not tested for bad.
 * ---- (5) Point list ------------------------------------------------------------------------------------------------------------
 *   The held points in keypoint order, first occurrence of each (n_held of them), then for the keyframes of L in order and k
 *   ascending every SEARCHABLE point not yet listed.  A point's place is decided by its KEY, the least of
 *     k                                  for a keypoint k that holds it
 *     n_kp + i * kp_stride + k           for entry k of the row of L[i]
 *   and the list is the points in ascending key order; n_points_total counts them all, n_points = min(that, point_cap).
 */
#ifndef SPFE_LOCALMAP_MATH_H
#define SPFE_LOCALMAP_MATH_H

#if defined(__HIPCC__)
#define SPFE_LM __host__ __device__ static inline
#else
#define SPFE_LM static inline
#endif

#define SPFE_LOCALMAP_MAX_WEIGHT 127
#define SPFE_LOCALMAP_SEARCHABLE_BIT 0x80u
#define SPFE_LOCALMAP_NO_KEY 0x7fffffff

/* the byte of a point in the weight table: bit 7 = SEARCHABLE, bits 0-6 = w */
SPFE_LM unsigned spfe_lm_table_byte(unsigned mp_flag, int count) {
  if (!(mp_flag & 1u)) return 0u;
  return SPFE_LOCALMAP_SEARCHABLE_BIT | (unsigned)(count > SPFE_LOCALMAP_MAX_WEIGHT ? SPFE_LOCALMAP_MAX_WEIGHT : count);
}
SPFE_LM int spfe_lm_weight(unsigned table_byte) { return (int)(table_byte & 0x7fu); }
SPFE_LM int spfe_lm_searchable(unsigned table_byte) { return (int)(table_byte >> 7); }

/* a row entry or a holder names a table row */
SPFE_LM int spfe_lm_in_table(int p, int n_table) { return p >= 0 && p < n_table; }

/* (vote, slot) a takes the reference keyframe from b: the strictly greater vote, the lower slot among equals; slot -1 = none */
SPFE_LM int spfe_lm_ref_beats(int av, int as, int bv, int bs) {
  if (as < 0) return 0;
  if (bs < 0) return 1;
  return av > bv || (av == bv && as < bs);
}

/* the 80 rule: the walk stops when the list has grown BEYOND max_keyframes */
SPFE_LM int spfe_lm_full(int n_local, int max_keyframes) { return n_local > max_keyframes; }

#endif
