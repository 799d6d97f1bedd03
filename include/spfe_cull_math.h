/*
 * spfe_cull_math.h — the contract of keyframe culling on the device (the cull loop of the local mapper and KeyFrame::SetBadFlag on
 * resident rows), shared by the GPU kernels (sp_orb_slam_amd/csrc/cull.hip) and the host C reference of the test suite
 * (tests/cull_ref/cull_ref.c).  Integers only, apart from ONE f32 division: every output is equal byte for byte whatever the order
 * of evaluation.
 *
 * What it restates, in this project's own words:
 *   LocalMapping::KeyFrameCullingOverride           orb_slam2/src/mapping/local_mapper.cpp:979-1032
 *   KeyFrame::SetBadFlag / EraseConnection          orb_slam2/src/type/keyframe.cpp:911-997, :1004-1016
 *   MapPoint::EraseObservation / SetBadFlag         orb_slam2/src/type/mappoint.cpp:122-173
 *
 * The state: the rows kf_mp_of_kp, kf_flags (bit 0 bad, bit 1 SPFE_KF_NOT_ERASE, bit 2 SPFE_KF_TO_BE_ERASED), mp_flags (bit
 * SPFE_PROJ_SEARCHABLE clear = the point is bad), nobs (MapPoint::Observations(), monocular: 1 an observation), the graph of
 * spfe_covis_math.h and the two best_cov tables.  A point p is GOOD when 0 <= p < n_table and mp_flags[p] has SPFE_PROJ_SEARCHABLE.
 *
 * ---- (1) The list (:980-987) -------------------------------------------------------------------------------------------------
 *   n_listed = ord_n[cur] (held to [0, conn_cap]); entry j is ord_slot[cur][j], read ONCE: nothing below reads the graph again
 *   before (6).  An entry is skipped at entry, with a code, pass 0 and counts 0, when its slot is outside [0, n_slots) (WILD, and
 *   the status bit SPFE_CULL_WILD_ENTRY), is origin_slot (ORIGIN: mnId == 0), or has bit 0 of kf_flags set (BAD), tested in that
 *   order.  The others are LIVE, in list order.
 * ---- (2) A pass (:992-1025) --------------------------------------------------------------------------------------------------
 *   Passes are numbered from 1.  For every live entry, in list order: n_mps = the entries of its row that name a good point, n_red
 *   = those of them with nobs[p] >= th_obs, both per ENTRY (a point named twice counts twice, as the votes do); ratio =
 *   (float)n_red / (float)n_mps, correctly rounded (n_mps == 0: NaN, which neither drops nor wins).  ratio < cov_ratio: the entry
 *   leaves the list, code DROPPED.  Otherwise it is offered; the pass's choice is the first in list order with the strictly
 *   greatest ratio above 0.0f.  The block keeps, per entry, the pass that decided it and n_mps / n_red of that pass.
 * ---- (3) The stall rule (this project's own) ----------------------------------------------------------------------------------
 *   A pass that leaves live entries and chooses nothing ends the loop: status SPFE_CULL_STALLED, the live entries get code
 *   STALLED.  (The reference never returns from that state: a keyframe without a good point, or cov_ratio <= 0 at ratio 0.)
 *   Otherwise the loop ends when no entry is live.
 * ---- (4) The choice (:1027-1030, keyframe.cpp:911-920) -------------------------------------------------------------------------
 *   It leaves the list.  With SPFE_KF_NOT_ERASE set: kf_flags |= SPFE_KF_TO_BE_ERASED, code DEFERRED, nothing else changes.
 *   Otherwise code CULLED, the slot is appended to culled_slot[], and (5) runs before the next pass — the next pass reads nobs
 *   and mp_flags as (5) left them.
 * ---- (5) Cull of m, the points (keyframe.cpp:927-929, mappoint.cpp:122-173) ----------------------------------------------------
 *   For every good point p named by row m: nobs[p] -= c, c = the number of entries of row m that name p.  A point with a result
 *   <= 2 loses SPFE_PROJ_SEARCHABLE (its other flag bits stay, and so does nobs[p]).  kf_flags[m] |= 1.  The newly bad points
 *   are appended to bad_point[] in the order of their first entry in row m; the list is cut at bad_cap (n_bad counts all of them,
 *   status SPFE_CULL_BAD_CUT), -1 behind the stored ones.  Equal to the reference wherever a row holds a point once; a row that
 *   holds it twice takes 2 where the reference's observation map (one index a keyframe) takes 1.
 * ---- (6) Graph, per culled keyframe c, in cull order, after the last pass (keyframe.cpp:922-925, :935-993) ----------------------
 *   (a) EraseConnection, literally: for every key s of conn[c] as it stands (inside [0, n_slots), s != c), c leaves conn[s] iff c
 *       is a key of conn[s]; on a removal ord[s] = ALL of conn[s] by spfe_cv_key descending, the whole rows of s written (-1 / 0
 *       behind the counts), s is TOUCHED, and its table rows are rewritten (7).  Nothing is removed from conn[c] on behalf of s:
 *       a link c holds and s does not (or the reverse) stays where it is until (b).
 *   (b) conn[c] and ord[c] go to their preset (counts 0, rows -1 / 0), the table rows of c to -1.  parent[c] and first_conn[c]
 *       stay.
 *   (c) The children of c are the slots s != c with parent[s] == c, ascending.  candidates = {parent[c]} (empty when parent[c] is
 *       outside [0, n_slots): status SPFE_CULL_NO_PARENT — a null dereference in the reference).  One STEP walks the children
 *       left, ascending, skipping those that were bad WHEN c WAS CULLED: bit 0 of kf_flags set before the call, or culled earlier
 *       in it.  A child that is culled LATER in the call is alive here: it is re-parented, joins the candidates and may take its
 *       siblings (this step runs after the last pass, so the flag alone does not say it: spfe_ck_child_is_bad).  For each child
 *       it walks ord_slot[child][0 .. ord_n) in order; an entry that is a candidate is offered with its weight in conn[child] (0
 *       when it is no key there; PRECONDITION, as everywhere in spfe_covis_math.h: the keys of a conn row are ascending and
 *       unique — the kernel looks the weight up by bisection, cull_ref.c takes the first match, and on a row that breaks the
 *       rule the two may differ); the first offer of the step with the strictly greatest weight (> -1) wins: parent[child] =
 *       that entry, the child joins the candidates and leaves the children, one event (child, new parent).  The steps end with
 *       one that finds nothing.  Every child still left, bad ones included, gets parent[c] (-1 when there is none), ascending, an
 *       event each.  The rows are those (a) and (b) of c and of the keyframes culled before c left: it matters when parent(c) is
 *       itself culled later in the call.  Events beyond n_slots are counted (n_reparented) and not stored (SPFE_CULL_EVENT_CUT).
 * ---- (7) Tables ---------------------------------------------------------------------------------------------------------------
 *   The row of every touched slot and every culled slot in each best_cov table given = the first n_best entries of its ord_slot,
 *   -1 padded.  No other row is written.
 * ---- (8) Rows (mappoint.cpp:157-173, EraseMapPointMatch) -------------------------------------------------------------------------
 *   After the last pass every entry that names a newly bad point becomes -1, in every row whose slot is not bad after the call.
 *   Rows of bad slots keep their bytes: the reference keeps the culled keyframe's own mvpMapPoints.
 */
#ifndef SPFE_CULL_MATH_H
#define SPFE_CULL_MATH_H

#include <stdint.h>

#if defined(__HIPCC__)
#define SPFE_CK __host__ __device__ static inline
#else
#define SPFE_CK static inline
#endif

#define SPFE_CULL_CODE_DROPPED 0
#define SPFE_CULL_CODE_CULLED 1
#define SPFE_CULL_CODE_DEFERRED 2
#define SPFE_CULL_CODE_STALLED 3
#define SPFE_CULL_CODE_ORIGIN 4
#define SPFE_CULL_CODE_WILD 5
#define SPFE_CULL_CODE_BAD 6

/* (1): the code an entry is skipped with at entry, or -1: live.  kf_flag is read only for a slot in range. */
SPFE_CK int spfe_ck_entry_in_range(int s, int n_slots) { return s >= 0 && s < n_slots; }
SPFE_CK int spfe_ck_entry_code(int s, int origin_slot, unsigned kf_flag) {
  if (s == origin_slot) return SPFE_CULL_CODE_ORIGIN;
  return (kf_flag & 1u) ? SPFE_CULL_CODE_BAD : -1;
}

/* a good point */
SPFE_CK int spfe_ck_good(int p, int n_table, const uint8_t *mp_flags) { return p >= 0 && p < n_table && (mp_flags[p] & 1u); }

/* (2): the one division */
SPFE_CK float spfe_ck_ratio(int n_red, int n_mps) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fdiv_rn((float)n_red, (float)n_mps);
#else
  return (float)n_red / (float)n_mps;
#endif
}
SPFE_CK int spfe_ck_drops(float ratio, float cov_ratio) { return ratio < cov_ratio; }
/* (2): an offer, as a key whose MAXIMUM is the pass's choice: the ratio's bits (monotonic for ratio > 0) over the list position
 * reversed; 0 = no offer (ratio NaN or not above 0.0f) */
SPFE_CK uint64_t spfe_ck_offer(float ratio, int pos) {
  union { float f; uint32_t u; } b;
  if (!(ratio > 0.0f)) return 0;
  b.f = ratio;
  return ((uint64_t)b.u << 32) | (uint32_t)(0xffffffffu - (uint32_t)pos);
}
SPFE_CK int spfe_ck_offer_pos(uint64_t k) { return (int)(0xffffffffu - (uint32_t)(k & 0xffffffffu)); }

/* (5) */
SPFE_CK int spfe_ck_goes_bad(int nobs_after) { return nobs_after <= 2; }

/* (6c): isBad() of a child at the time the keyframe of place ci in cull order is culled; cull_idx = the child's own place in
 * cull order, -1 when it is not culled in this call (then the flag is the one it had before the call) */
SPFE_CK int spfe_ck_child_is_bad(unsigned kf_flag, int cull_idx, int ci) { return (kf_flag & 1u) && cull_idx < ci; }

/* (6c): an offer of a step, as a key whose MAXIMUM wins: the weight over the walk's position (child index, entry) reversed;
 * INT64_MIN = none.  Weights below 0 are not offered (w > max, max = -1). */
#define SPFE_CULL_STEP_NONE INT64_MIN
SPFE_CK int64_t spfe_ck_step_key(int w, int child_idx, int entry, int conn_cap) {
  if (w < 0) return SPFE_CULL_STEP_NONE;
  return (int64_t)(((uint64_t)(uint32_t)w << 32) | (uint32_t)(0xffffffffu - ((uint32_t)child_idx * (uint32_t)conn_cap + (uint32_t)entry)));
}
SPFE_CK uint32_t spfe_ck_step_walk(int64_t k) { return 0xffffffffu - (uint32_t)((uint64_t)k & 0xffffffffu); }

#endif
