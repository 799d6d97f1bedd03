/*
 * spfe_newkf_math.h — the contract of the first step of every mapping cycle on the device, and of the observation lists every
 * map-point refresh takes: the insertion of a new keyframe's row into the resident rows (LocalMapping::ProcessNewKeyFrame without
 * its refresh) and the inverse of the rows for a list of points (what the host iterates mObservations for).  Shared by the GPU
 * kernels (sp_orb_slam_amd/csrc/newkf.hip) and the host C reference of the test suite (tests/newkf_ref/newkf_ref.c).  Integers and
 * copied bytes only: every output is equal byte for byte whatever the order of evaluation.  Monocular.
 *
 * What it restates, in this project's own words:
 *   LocalMapping::ProcessNewKeyFrame               orb_slam2/src/mapping/local_mapper.cpp:255-272
 *   MapPoint::AddObservation / GetObservations     orb_slam2/src/type/mappoint.cpp
 *   Tracking::CreateNewKeyFrame (the outliers)     orb_slam2/src/tracking/tracker.cpp:311-320
 *
 * The state is that of spfe_mpcull_math.h (struct spfe_mp_life): flags, nobs and the recent list are touched here.
 *
 * ---- (I) Insertion of a keyframe's row (local_mapper.cpp:255-272) ------------------------------------------------------------------
 *   frame[i], i < n_kp: the frame's mvpMapPoints as table rows at CreateNewKeyFrame, outliers included.
 *  (I1) The code of keypoint i, the first that applies (spfe_nk_precode, then the first occurrence):
 *         NONE       frame[i] == -1
 *         WILD       frame[i] outside [0, n_table)               (any other negative value included)
 *         BAD_POINT  flags[frame[i]] lacks SPFE_PROJ_SEARCHABLE at entry
 *         ADDED      i is the least keypoint that names this point among those that passed the three tests above
 *         REPEATED   a later keypoint that names the same point
 *  (I2) The test, before anything is written (all or nothing):
 *         ROW_IN_USE       some entry of rows[cur_slot][0 .. kp_stride) is >= 0
 *         BAD_SLOT         kf_flags[cur_slot] has bit 0 set
 *         RECENT_OVERFLOW  n_recent_before + n_repeated > recent_cap   (n_recent_before: recent_n held to [0, recent_cap])
 *       n_needed = n_recent_before + n_repeated is the capacity the call asked for.  A refused call writes the block alone: the
 *       counts and code[] as decided, added_point[] all -1, n_recent_after = n_recent_before.
 *  (I3) Otherwise, for keypoint i in order:
 *         NONE / WILD / BAD_POINT   rows[cur_slot][i] = -1.  DEVIATION: the reference keeps a bad point's pointer in the keyframe;
 *                                   every resident reader relies on rows that name no bad point.
 *         ADDED      rows[cur_slot][i] = p; nobs[p] += 1; flags[p] |= SPFE_PROJ_OBSERVED (what the admission leaves an observed
 *                    point with); added_point[i] = p; with a record and a track table, desc_track[p] = the record's descriptor
 *                    row i as f32 (a bf16 row widened exactly: the 16 bits become the upper half of the f32).
 *         REPEATED   rows[cur_slot][i] = p; nobs[p] += 1; recent[n_recent_before + (the REPEATED keypoints before i)] = p.  The
 *                    push is the reference's own: IsInKeyFrame is true at the later keypoint, so :268 runs.  DEVIATION: the
 *                    reference's mObservations holds ONE entry for the keyframe (the first keypoint); nobs counts row entries,
 *                    the rule of spfe_covis_math.h, so that it stays equal to a fresh count of the rows.
 *       rows[cur_slot][n_kp .. kp_stride) = -1; recent_n = n_recent_before + n_repeated.
 *       added_point[k] = -1 at every k < kp_stride that is not an ADDED keypoint: the array is a point list for (O) as it lies.
 *
 * ---- (O) The observations of a list of points, from one scan of the rows --------------------------------------------------------
 *   entry i of m names p = point_idx[i], or first_row + i without a list.
 *  (O1) The code of entry i (spfe_nk_list_precode, then the first occurrence): EMPTY p == -1; WILD p outside [0, n_table);
 *       REPEATED an earlier entry names p; FIRST otherwise.  Only a FIRST entry has observations; point_idx_out[i] = p there and -1
 *       everywhere else, ref_slot_out[i] = mp_ref_slot[p] there and -1 everywhere else.  Point flags are not read.
 *  (O2) The observations of a FIRST entry: every (slot, keypoint) with rows[slot][keypoint] == p over the slots whose kf_flags
 *       lack bit 0, ascending by spfe_nk_obs_key (slot first, then keypoint: slot order stands for std::map's pointer order).  A row
 *       that names the point twice gives two observations.  Rows of bad slots are never read.
 *  (O3) n_obs_needed = the count of all observations; max_obs = the largest count of one entry; SPFE_LISTOBS_MANY when max_obs >
 *       SPFE_MP_MAX_OBS.  n_obs_needed > obs_cap: SPFE_LISTOBS_OVERFLOW, n_obs = 0, every obs_start 0, obs all -1 (a refresh
 *       behind it finds no observation anywhere and writes nothing).  Otherwise obs_start[i] = the count of the observations of
 *       the entries before i, obs_start[m] = n_obs = n_obs_needed, obs[obs_start[i] ..) the entry's observations, -1 behind n_obs.
 */
#ifndef SPFE_NEWKF_MATH_H
#define SPFE_NEWKF_MATH_H

#include <stdint.h>

#if defined(__HIPCC__)
#define SPFE_NK __host__ __device__ static inline
#else
#define SPFE_NK static inline
#endif

#define SPFE_NEWKF_CODE_NONE 0
#define SPFE_NEWKF_CODE_WILD 1
#define SPFE_NEWKF_CODE_BAD_POINT 2
#define SPFE_NEWKF_CODE_ADDED 3
#define SPFE_NEWKF_CODE_REPEATED 4

#define SPFE_LISTOBS_CODE_EMPTY 0
#define SPFE_LISTOBS_CODE_WILD 1
#define SPFE_LISTOBS_CODE_REPEATED 2
#define SPFE_LISTOBS_CODE_FIRST 3

SPFE_NK int spfe_nk_in_range(int64_t p, int n_table) { return p >= 0 && p < (int64_t)n_table; }

/* (I1) without the first occurrence: NONE or WILD from the entry alone; -1: the flags decide (spfe_nk_code) */
SPFE_NK int spfe_nk_precode(int p, int n_table) {
  if (p == -1) return SPFE_NEWKF_CODE_NONE;
  if (!spfe_nk_in_range(p, n_table)) return SPFE_NEWKF_CODE_WILD;
  return -1;
}
/* (I1) for an entry in range: flag = flags[p] at entry, first = the least keypoint that names p among the good ones */
SPFE_NK int spfe_nk_code(unsigned flag, int i, int first) {
  if (!(flag & 1u)) return SPFE_NEWKF_CODE_BAD_POINT;
  return i == first ? SPFE_NEWKF_CODE_ADDED : SPFE_NEWKF_CODE_REPEATED;
}
SPFE_NK int spfe_nk_in_row(int code) { return code == SPFE_NEWKF_CODE_ADDED || code == SPFE_NEWKF_CODE_REPEATED; }

/* (O1): the point of entry i in 64 bits (first_row + i does not wrap), and its code without the first occurrence */
SPFE_NK int64_t spfe_nk_list_point(const int32_t *point_idx, int first_row, int i) {
  return point_idx ? (int64_t)point_idx[i] : (int64_t)first_row + (int64_t)i;
}
SPFE_NK int spfe_nk_list_precode(int64_t p, int n_table) {
  if (p == -1) return SPFE_LISTOBS_CODE_EMPTY;
  if (!spfe_nk_in_range(p, n_table)) return SPFE_LISTOBS_CODE_WILD;
  return -1;
}

/* (O2): the order of a point's observations */
SPFE_NK uint64_t spfe_nk_obs_key(int slot, int kp) { return ((uint64_t)(uint32_t)slot << 32) | (uint32_t)kp; }

/* a bf16 descriptor element as f32, exactly */
SPFE_NK uint32_t spfe_nk_bf16_bits(uint16_t v) { return (uint32_t)v << 16; }

#endif
