/*
 * spfe_covis_math.h — the contract of the covisibility graph on the device (KeyFrame::UpdateConnections on resident rows),
 * shared by the GPU kernels (sp_orb_slam_amd/csrc/covis.hip) and the host C reference of the test suite
 * (tests/covis_ref/covis_ref.c).  Integers only: every output is equal byte for byte whatever the order of evaluation.
 *
 * What it restates, in this project's own words:
 *   KeyFrame::UpdateConnections                     orb_slam2/src/type/keyframe.cpp:757-849
 *   KeyFrame::AddConnection / UpdateBestCovisibles  orb_slam2/src/type/keyframe.cpp:577-612
 *   the accessors the consumers read through        orb_slam2/src/type/keyframe.cpp:614-662
 *
 * The state, a row a keyframe slot: conn (mConnectedKeyFrameWeights: keys ascending by slot, conn_n of them, -1 / 0 behind),
 * ord (mvpOrderedConnectedKeyFrames / mvOrderedWeights, ord_n of them, -1 / 0 behind), parent (mpParent, -1 for none) and
 * first_conn (mbFirstConnection).  The preset of a slot: counts 0, rows -1 / 0, parent -1, first_conn 1.
 *
 * ---- (1) Counter (:760-793) ------------------------------------------------------------------------------------------------
 *   counter[s] = votes[s] of spfe_localmap_math.h (1)-(2), the "frame" being row cur_slot of kf_mp_of_kp itself (n_kp =
 *   kp_stride, no outlier mask): a point held by two entries of the current row counts twice, as KFcounter[..]++ runs per
 *   entry.  counter[cur_slot] = 0 (:789), and counter[s] = 0 where bit 0 of kf_flags[s] is set (a bad keyframe's observations
 *   are erased in the reference); cur_slot itself is not tested for bad.
 *   Two deviations, both inherited from the vote: a point's weight is capped at SPFE_LOCALMAP_MAX_WEIGHT (127 entries of ONE
 *   row on one point is no state a map reaches), and a NEIGHBOUR row that holds one point twice counts it twice where the
 *   reference's observation map (one index a keyframe) counts it once.
 * ---- (2) Empty and overflow (:796) ---------------------------------------------------------------------------------------------
 *   n_counter = the slots with counter > 0.  n_counter == 0: status SPFE_COVIS_NO_SHARED; n_counter > conn_cap: status
 *   SPFE_COVIS_CUR_OVERFLOW.  In both NO state changes anywhere; the block holds status, n_counter, counter, max_slot and
 *   max_count, n_linked = n_changed = n_overflow = 0, parent_set = -1, and -1 in every linked_slot / linked_code.
 * ---- (3) Linked set (:803-825) -----------------------------------------------------------------------------------------------
 *   max_slot = the lowest slot with the strictly greatest counter (the reference walks a std::map keyed by heap address: slot
 *   order is this project's statement of it).  P = the slots with counter >= th, ascending; none: P = {max_slot}.
 * ---- (4) Neighbours (:577-612) -----------------------------------------------------------------------------------------------
 *   For every s in P, AddConnection(cur, counter[s]) on slot s, as a code:
 *     0  cur_slot is in conn[s] with this weight: NOTHING, not even a re-sort (the early return at :585)
 *     1  it is there with another weight: the weight is replaced
 *     2  it is absent: inserted, keeping ascending slot order
 *     3  it is absent and conn_n[s] == conn_cap: s is left unchanged, status SPFE_COVIS_NEIGH_OVERFLOW
 *   On 1 and 2, ord[s] = ALL entries of conn[s] by weight descending, slot DESCENDING among equal weights (sort of (weight,
 *   pointer) pairs, then push_front): the (weight, slot) key below, descending.  Links of slots outside P are not touched.
 * ---- (5) Current keyframe (:827-841) ----------------------------------------------------------------------------------------
 *   conn[cur] = every (s, counter[s]) with counter > 0, ascending: the whole row is written (-1 / 0 behind n_counter).
 *   ord[cur] = P alone in the order of (4), the whole row written likewise.
 * ---- (6) Parent (:843-847) ---------------------------------------------------------------------------------------------------
 *   first_conn[cur] set and cur_slot != origin_slot: parent[cur] = ord_slot[cur][0], first_conn[cur] = 0, parent_set = that
 *   slot.  Otherwise both stay and parent_set = -1.
 * ---- (7) Tables (:628-635) ---------------------------------------------------------------------------------------------------
 *   For cur_slot and every neighbour with code 1 or 2, the slot's row in each best_cov table given = the first n_best entries
 *   of its ord_slot, -1 padded.  No other row is written.
 */
#ifndef SPFE_COVIS_MATH_H
#define SPFE_COVIS_MATH_H

#include <stdint.h>

#if defined(__HIPCC__)
#define SPFE_CV __host__ __device__ static inline
#else
#define SPFE_CV static inline
#endif

#define SPFE_COVIS_CODE_SAME 0
#define SPFE_COVIS_CODE_REPLACED 1
#define SPFE_COVIS_CODE_INSERTED 2
#define SPFE_COVIS_CODE_FULL 3

/* (1): the vote of slot s as the counter of the keyframe at cur */
SPFE_CV int spfe_cv_counter(int vote, int s, int cur, unsigned kf_flag) { return (s == cur || (kf_flag & 1u)) ? 0 : vote; }

/* (3): (count, slot) a takes the maximum from b: the strictly greater count, the lower slot among equals; slot -1 = none.
 * Only counts above 0 are ever offered. */
SPFE_CV int spfe_cv_max_beats(int ac, int as, int bc, int bs) {
  if (as < 0 || ac <= 0) return 0;
  if (bs < 0) return 1;
  return ac > bc || (ac == bc && as < bs);
}

/* (3): s belongs to P; n_above = the number of slots with counter >= th */
SPFE_CV int spfe_cv_linked(int c, int s, int th, int n_above, int max_slot) { return n_above > 0 ? c >= th : s == max_slot; }

/* (4): the order of ord is these keys DESCENDING; keys of one row are unique because its slots are */
SPFE_CV int64_t spfe_cv_key(int w, int slot) { return (int64_t)(((uint64_t)(uint32_t)w << 32) | (uint32_t)slot); }
SPFE_CV int spfe_cv_key_w(int64_t k) { return (int)(uint32_t)((uint64_t)k >> 32); }
SPFE_CV int spfe_cv_key_slot(int64_t k) { return (int)(uint32_t)((uint64_t)k & 0xffffffffu); }
#define SPFE_COVIS_KEY_NONE INT64_MIN /* sorts behind every key of a weight >= 0 */

/* (4): AddConnection as a code; found = cur_slot is in conn[s], old_w its weight there, n = conn_n[s] */
SPFE_CV int spfe_cv_add_code(int found, int old_w, int w, int n, int conn_cap) {
  if (found) return old_w == w ? SPFE_COVIS_CODE_SAME : SPFE_COVIS_CODE_REPLACED;
  return n >= conn_cap ? SPFE_COVIS_CODE_FULL : SPFE_COVIS_CODE_INSERTED;
}

#endif
