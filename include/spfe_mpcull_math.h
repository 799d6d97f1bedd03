/*
 * spfe_mpcull_math.h — the contract of map-point culling on the device (the second stage of every mapping cycle) and of the three
 * pieces of resident state it needs: the found / visible counters of a map point, the list of recently added points with each
 * point's first keyframe, and the admission of created points into the resident rows.  Shared by the GPU kernels
 * (sp_orb_slam_amd/csrc/mpcull.hip) and the host C reference of the test suite (tests/mpcull_ref/mpcull_ref.c).  Integers only,
 * apart from ONE f32 division: every output is equal byte for byte whatever the order of evaluation.  Monocular.
 *
 * What it restates, in this project's own words:
 *   LocalMapping::MapPointCulling                  orb_slam2/src/mapping/local_mapper.cpp:281-310
 *   LocalMapping::CreateNewMapPoints (the tail)    orb_slam2/src/mapping/local_mapper.cpp:770-787
 *   MapPoint::MapPoint / IncreaseVisible / Found   orb_slam2/src/type/mappoint.cpp:37-53, :191-203
 *   Tracking::TrackLocalMap / SearchLocalPoints    orb_slam2/src/tracking/tracker.cpp:576-588, :772-807
 *
 * The state (struct spfe_mp_life of include/spfe.h), indexed by map-point table row p in [0, n_table):
 *   flags[p]     SPFE_PROJ_SEARCHABLE (= !isBad()) | SPFE_PROJ_OBSERVED      nobs[p]      Observations()
 *   found[p]     mnFound                                                      visible[p]   mnVisible
 *   first_kf[p]  mnFirstKFid as a keyframe ID, not a slot; -1 for a point made from a frame
 *   recent[0 .. recent_n)   mlpRecentAddedMapPoints in push order, -1 behind the count; recent_n is held to [0, recent_cap]
 *
 * ---- (A) Admission of created points (local_mapper.cpp:770-787, mappoint.cpp:37-50) --------------------------------------------
 *  (A1) The blocks: neighbour j of n_neigh has one block of spfe_create_map_points_record_device.  A block with status != 0
 *       contributes nothing and NOTHING but its status is read.  Otherwise cnt[j] = n_new[j], base[j] = point_base[j].
 *  (A2) The test, before anything is written (all or nothing).  SPFE_ADMIT_BAD_RANGE when, for a contributing block, cnt[j] is
 *       outside [0, kmax], neigh_slot[j] is outside [0, n_slots), equals cur_slot or equals the slot of an earlier contributing
 *       block, base[j] < 0 or base[j] + cnt[j] > n_table, or some new_k1[t] / new_k2[t], t < cnt[j], is outside [0, kp_stride).
 *       SPFE_ADMIT_RECENT_OVERFLOW when n_recent_before + sum cnt > recent_cap.  n_needed = n_recent_before + sum cnt (the sum over
 *       the contributing blocks with cnt in [0, kmax]) is the capacity the call asked for.  With either bit nothing but the
 *       block is written.
 *  (A3) For neighbour j in order and t < cnt[j] in order, p = base[j] + t:
 *         rows[cur_slot][new_k1[t]] = p, rows[neigh_slot[j]][new_k2[t]] = p — unconditional, as KeyFrame::AddMapPoint; an entry
 *         whose value before the call was not -1 is DISPLACED (counted, status SPFE_ADMIT_DISPLACED; the displaced point's nobs
 *         is left alone, as in the reference);
 *         xyz[p] = new_xyz[t]; nobs[p] = 2; found[p] = visible[p] = 1; first_kf[p] = cur_kf_id;
 *         flags[p] = SPFE_PROJ_SEARCHABLE | SPFE_PROJ_OBSERVED; recent[n_recent_before + (the points before it)] = p.
 *       PRECONDITION: the (row, keypoint) pairs and the ids of one call are distinct — the creation gives that: a keypoint of the
 *       current keyframe is claimed once over all neighbours, one of a neighbour once in its block, and the ids run on.  On a call
 *       that breaks it the reference's last write in order stands and the kernel's may be any of them.
 *
 * ---- (B) Tracking statistics (tracker.cpp:772-807, :576-588) ---------------------------------------------------------------------
 *   entry[k], after[k], k < n_kp: the frame's holders as table rows before the local-map step and behind it; point_idx[i],
 *   in_view[i], i < point_cap: the local-map list and the search's view flags; outlier[k]: the pose step's.
 *   (B1) visible[r] += 1 for every k with r = entry[k] in [0, n_table) and flags[r] SEARCHABLE                (n_visible_held)
 *   (B2) visible[r] += 1 for every i with in_view[i] != 0 and r = point_idx[i] in [0, n_table)                (n_visible_view)
 *   (B3) found[r]   += 1 for every k with r = after[k] in [0, n_table) and outlier[k] == 0                    (n_found)
 *   A point held by two keypoints is counted twice.  Sums of integers: the order does not matter.
 *
 * ---- (C) The cull loop (local_mapper.cpp:281-310) ----------------------------------------------------------------------------------
 *   n_listed = recent_n held to [0, recent_cap]; entry e names p = recent[e].  The FIRST matching rule gives the entry's code:
 *   (C1) WILD         p outside [0, n_table): removed (status SPFE_MPCULL_WILD_ENTRY).
 *   (C2) ERASED_BAD   p lacks SEARCHABLE at entry, or an EARLIER entry of this call culled it: removed.
 *   (C3) CULLED_RATIO spfe_mc_ratio(found[p], visible[p]) < found_ratio (visible == 0: NaN or infinity, false).
 *   (C4) CULLED_OBS   cur_kf_id - first_kf[p] >= 2 and nobs[p] <= th_obs.
 *   (C5) RETIRED      cur_kf_id - first_kf[p] >= 3: removed, the point stays good.
 *   (C6) KEPT.
 *   (C3)-(C6) read nothing the call writes, so every entry that names p gets the same answer from them; among the entries that
 *   name a culled point the one with the least index is the one that culls, the others are ERASED_BAD.
 *   (C7) A culled point loses SEARCHABLE; its other bits, nobs, found, visible and first_kf stay.  The culled points go to
 *        bad_point[] in list order, cut at bad_cap (n_bad counts all; SPFE_MPCULL_BAD_CUT), -1 behind the stored ones.
 *   (C8) The KEPT entries move to the front of recent[] in their order; recent_n = n_kept; the entries between n_kept and n_listed
 *        become -1.  Entries at and beyond n_listed are not written.
 *   (C9) Every entry of the rows that names a culled point becomes -1 in every row whose slot is not bad; rows of bad slots keep
 *        their bytes.
 */
#ifndef SPFE_MPCULL_MATH_H
#define SPFE_MPCULL_MATH_H

#include <stdint.h>

#if defined(__HIPCC__)
#define SPFE_MC __host__ __device__ static inline
#else
#define SPFE_MC static inline
#endif

#define SPFE_MPCULL_CODE_KEPT 0
#define SPFE_MPCULL_CODE_CULLED_RATIO 1
#define SPFE_MPCULL_CODE_CULLED_OBS 2
#define SPFE_MPCULL_CODE_RETIRED 3
#define SPFE_MPCULL_CODE_ERASED_BAD 4
#define SPFE_MPCULL_CODE_WILD 5

SPFE_MC int spfe_mc_in_range(int p, int n_table) { return p >= 0 && p < n_table; }
SPFE_MC int spfe_mc_good(unsigned flag) { return (flag & 1u) != 0; }

/* (C3): two int-to-float conversions and the one division, correctly rounded */
SPFE_MC float spfe_mc_ratio(int found, int visible) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fdiv_rn((float)found, (float)visible);
#else
  return (float)found / (float)visible;
#endif
}

/* the age in keyframe ids; 64 bits: any two int32 ids have a difference */
SPFE_MC int64_t spfe_mc_age(int cur_kf_id, int first_kf) { return (int64_t)cur_kf_id - (int64_t)first_kf; }

/* (C3)-(C6) for a point that is in range and good at entry */
SPFE_MC int spfe_mc_rule(int found, int visible, int first_kf, int nobs, int cur_kf_id, int th_obs, float found_ratio) {
  const int64_t age = spfe_mc_age(cur_kf_id, first_kf);
  if (spfe_mc_ratio(found, visible) < found_ratio) return SPFE_MPCULL_CODE_CULLED_RATIO;
  if (age >= 2 && nobs <= th_obs) return SPFE_MPCULL_CODE_CULLED_OBS;
  if (age >= 3) return SPFE_MPCULL_CODE_RETIRED;
  return SPFE_MPCULL_CODE_KEPT;
}
SPFE_MC int spfe_mc_culls(int code) { return code == SPFE_MPCULL_CODE_CULLED_RATIO || code == SPFE_MPCULL_CODE_CULLED_OBS; }

/* (A2): what a block's header alone says; 0 = fine */
SPFE_MC int spfe_mc_block_bad(int cnt, int base, int slot, int cur_slot, int kmax, int n_slots, int n_table) {
  if (cnt < 0 || cnt > kmax) return 1;
  if (slot < 0 || slot >= n_slots || slot == cur_slot) return 1;
  if (base < 0 || (int64_t)base + cnt > (int64_t)n_table) return 1;
  return 0;
}
SPFE_MC int spfe_mc_kp_in_range(int k, int kp_stride) { return k >= 0 && k < kp_stride; }

#endif
