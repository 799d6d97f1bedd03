/* newkf_ref.c — the host reference of a new keyframe on resident state and of the observation lists of the refreshes: a sequential
 * restatement of
 *   LocalMapping::ProcessNewKeyFrame               orb_slam2/src/mapping/local_mapper.cpp:255-272 (without the refresh)
 *   MapPoint::GetObservations as the callers walk it (ProcessNewKeyFrame :264-265, CreateNewMapPoints, SearchInNeighbors, CorrectLoop)
 * on the arrays of include/spfe.h ("a new keyframe on resident state"), with the contract of include/spfe_newkf_math.h.  The
 * insertion edits the state, the row and the track table in place; both write the whole block, every byte; the GPU tests compare all
 * of it byte for byte.  The insertion is ONE walk over the keypoints with an "is in this keyframe" mark per point, as IsInKeyFrame
 * answers it; the listing is two walks over the rows in (slot, keypoint) order.
 * `mutate` switches ONE line to a plausible misreading, so that tests/test_newkf_reference.py can show that its cases tell them
 * apart:
 *   1 the first occurrence is the greatest keypoint            7 a repeated list entry given a range of its own
 *   2 a REPEATED keypoint not pushed to the list               8 ref_slot taken by list position
 *   3 the rows of bad slots read                               9 a bad point kept in the row (the reference's own behaviour)
 *   4 the observations ordered by keypoint first              10 nobs counted once for a point the frame names twice
 *   5 the listing overflows at >=                             11 the list overflows at >=
 *   6 the row's tail behind n_kp not cleared                  12 a row that names a point twice gives one observation
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spfe.h"
#include "../../include/spfe_newkf_math.h"

#define EXPORT __attribute__((visibility("default")))

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

/* (I).  rec_desc: the record's descriptor rows (f32 [.][256], or bf16 [.][256] with desc_bf16), or NULL; desc_track f32
 * [n_table][256] or NULL */
EXPORT void newkf_ref_insert(const spfe_mp_life *l, const int32_t *frame, int n_kp, int cur_slot, int32_t *rows, int kp_stride,
                             const uint8_t *kf_flags, int n_slots, const uint8_t *rec_desc, int desc_bf16, float *desc_track, uint8_t *out,
                             int mutate) {
  uint8_t *flags = (uint8_t *)l->d_mp_flags;
  int32_t *nobs = (int32_t *)l->d_mp_nobs, *recent = (int32_t *)l->d_recent, *recent_n = (int32_t *)l->d_recent_n;
  int32_t *hdr = (int32_t *)out, *code = (int32_t *)(out + SPFE_NEWKF_OFF_CODE), *added = (int32_t *)(out + SPFE_NEWKF_OFF_ADDED_POINT(n_kp));
  int32_t *row = rows + (size_t)cur_slot * kp_stride;
  (void)n_slots;
  memset(out, 0, SPFE_NEWKF_OUT_BYTES(n_kp, kp_stride));
  for (int k = 0; k < kp_stride; ++k) added[k] = -1;
  const int n_before = clampi(*recent_n, 0, l->recent_cap);
  /* (I1): the walk of :258-272 with IsInKeyFrame as a mark */
  uint8_t *in_kf = calloc((size_t)l->n_table, 1);
  int cnt[5] = {0, 0, 0, 0, 0};
  for (int q = 0; q < n_kp; ++q) {
    const int i = mutate == 1 ? n_kp - 1 - q : q;
    const int p = frame[i];
    int c = spfe_nk_precode(p, l->n_table);
    if (c < 0) {
      if (!(flags[p] & SPFE_PROJ_SEARCHABLE)) c = SPFE_NEWKF_CODE_BAD_POINT;
      else if (!in_kf[p]) c = SPFE_NEWKF_CODE_ADDED, in_kf[p] = 1;
      else c = SPFE_NEWKF_CODE_REPEATED;
    }
    code[i] = c;
    ++cnt[c];
  }
  /* (I2) */
  int status = 0;
  for (int k = 0; k < kp_stride; ++k)
    if (row[k] >= 0) status |= SPFE_NEWKF_ROW_IN_USE;
  if (kf_flags[cur_slot] & 1u) status |= SPFE_NEWKF_BAD_SLOT;
  const int n_needed = n_before + cnt[SPFE_NEWKF_CODE_REPEATED];
  if (mutate == 11 ? n_needed >= l->recent_cap : n_needed > l->recent_cap) status |= SPFE_NEWKF_RECENT_OVERFLOW;
  hdr[SPFE_NEWKF_OFF_STATUS / 4] = status;
  for (int c = 0; c < 5; ++c) hdr[SPFE_NEWKF_OFF_N_NONE / 4 + c] = cnt[c];
  hdr[SPFE_NEWKF_OFF_N_RECENT_BEFORE / 4] = n_before;
  hdr[SPFE_NEWKF_OFF_N_RECENT_AFTER / 4] = status ? n_before : n_needed;
  hdr[SPFE_NEWKF_OFF_N_NEEDED / 4] = n_needed;
  /* (I3) */
  if (!status) {
    int at = n_before;
    memset(in_kf, 0, (size_t)l->n_table);
    for (int i = 0; i < n_kp; ++i) {
      const int p = frame[i], c = code[i];
      if (!spfe_nk_in_row(c)) {
        row[i] = mutate == 9 && c == SPFE_NEWKF_CODE_BAD_POINT ? p : -1;
        continue;
      }
      row[i] = p;
      if (!(mutate == 10 && in_kf[p])) nobs[p] += 1;
      in_kf[p] = 1;
      if (c == SPFE_NEWKF_CODE_ADDED) {
        flags[p] = (uint8_t)(flags[p] | SPFE_PROJ_OBSERVED);
        added[i] = p;
        if (rec_desc && desc_track) {
          uint32_t *dst = (uint32_t *)(desc_track + (size_t)p * 256);
          for (int d = 0; d < 256; ++d)
            dst[d] = desc_bf16 ? spfe_nk_bf16_bits(((const uint16_t *)rec_desc)[(size_t)i * 256 + d]) : ((const uint32_t *)rec_desc)[(size_t)i * 256 + d];
        }
      } else if (mutate != 2) {
        recent[at++] = p;
      }
    }
    if (mutate != 6)
      for (int k = n_kp; k < kp_stride; ++k) row[k] = -1;
    *recent_n = mutate == 2 ? n_before : n_needed;
  }
  free(in_kf);
}

/* (O) */
EXPORT void newkf_ref_list(const int32_t *point_idx, int first_row, int m, const int32_t *rows, int kp_stride, const uint8_t *kf_flags, int n_slots,
                           const int32_t *mp_ref_slot, int n_table, int obs_cap, uint8_t *out, int mutate) {
  int32_t *hdr = (int32_t *)out, *pidx = (int32_t *)(out + SPFE_LISTOBS_OFF_POINT_IDX), *obs_start = (int32_t *)(out + SPFE_LISTOBS_OFF_OBS_START(m));
  int32_t *ref_slot = (int32_t *)(out + SPFE_LISTOBS_OFF_REF_SLOT(m)), *obs = (int32_t *)(out + SPFE_LISTOBS_OFF_OBS(m));
  memset(out, 0, SPFE_LISTOBS_OUT_BYTES(m, obs_cap));
  /* (O1) */
  int32_t *entry_of = malloc(sizeof(int32_t) * (size_t)n_table);   /* the entry whose range a row entry goes to */
  int64_t *count = calloc((size_t)m + 1, sizeof(int64_t));
  for (int p = 0; p < n_table; ++p) entry_of[p] = -1;
  int cnt[4] = {0, 0, 0, 0};
  for (int i = 0; i < m; ++i) {
    const int64_t p = spfe_nk_list_point(point_idx, first_row, i);
    int c = spfe_nk_list_precode(p, n_table);
    if (c < 0) c = entry_of[p] < 0 ? SPFE_LISTOBS_CODE_FIRST : SPFE_LISTOBS_CODE_REPEATED;
    ++cnt[c];
    const int is_first = c == SPFE_LISTOBS_CODE_FIRST;
    if (is_first) entry_of[p] = i;
    pidx[i] = is_first ? (int32_t)p : -1;
    ref_slot[i] = is_first ? mp_ref_slot[mutate == 8 ? (i < n_table ? i : n_table - 1) : p] : -1;
    if (mutate == 7 && c == SPFE_LISTOBS_CODE_REPEATED) pidx[i] = (int32_t)p, entry_of[p] = i;   /* the later entry takes the range over */
  }
  /* (O2): two walks over the rows in (slot, keypoint) order: the counts, then the places */
  const int outer = mutate == 4 ? kp_stride : n_slots, inner = mutate == 4 ? n_slots : kp_stride;
  int32_t *last_slot = malloc(sizeof(int32_t) * ((size_t)m + 1));   /* mutation 12 alone */
  int64_t needed = 0, max_obs = 0;
  int overflow = 0;
  for (int pass = 0; pass < 2 && !overflow; ++pass) {
    for (int i = 0; i < m; ++i) last_slot[i] = -1;
    for (int o = 0; o < outer; ++o)
      for (int n = 0; n < inner; ++n) {
        const int s = mutate == 4 ? n : o, k = mutate == 4 ? o : n;
        if ((kf_flags[s] & 1u) && mutate != 3) continue;
        const int p = rows[(size_t)s * kp_stride + k];
        if (!spfe_nk_in_range(p, n_table) || entry_of[p] < 0) continue;
        const int i = entry_of[p];
        if (mutate == 12 && last_slot[i] == s) continue;
        last_slot[i] = s;
        if (pass == 0) {
          ++count[i];
          ++needed;
        } else {
          const int64_t at = count[i]++;
          obs[2 * at] = s;
          obs[2 * at + 1] = k;
        }
      }
    if (pass == 1) break;
    /* (O3) */
    for (int i = 0; i < m; ++i) max_obs = count[i] > max_obs ? count[i] : max_obs;
    overflow = mutate == 5 ? needed >= obs_cap : needed > obs_cap;
    hdr[SPFE_LISTOBS_OFF_STATUS / 4] = (overflow ? SPFE_LISTOBS_OVERFLOW : 0) | (max_obs > SPFE_MP_MAX_OBS ? SPFE_LISTOBS_MANY : 0);
    hdr[SPFE_LISTOBS_OFF_M / 4] = m;
    hdr[SPFE_LISTOBS_OFF_N_FIRST / 4] = cnt[SPFE_LISTOBS_CODE_FIRST];
    hdr[SPFE_LISTOBS_OFF_N_EMPTY / 4] = cnt[SPFE_LISTOBS_CODE_EMPTY];
    hdr[SPFE_LISTOBS_OFF_N_WILD / 4] = cnt[SPFE_LISTOBS_CODE_WILD];
    hdr[SPFE_LISTOBS_OFF_N_REPEATED / 4] = cnt[SPFE_LISTOBS_CODE_REPEATED];
    hdr[SPFE_LISTOBS_OFF_N_OBS / 4] = overflow ? 0 : (int32_t)needed;
    hdr[SPFE_LISTOBS_OFF_N_OBS_NEEDED / 4] = (int32_t)needed;
    hdr[SPFE_LISTOBS_OFF_MAX_OBS / 4] = (int32_t)max_obs;
    hdr[SPFE_LISTOBS_OFF_OBS_CAP / 4] = obs_cap;
    for (int64_t e = 0; e < 2 * (int64_t)obs_cap; ++e) obs[e] = -1;
    if (overflow) break;   /* obs_start: zeros already */
    int64_t at = 0;
    for (int i = 0; i < m; ++i) {   /* count[] becomes the next free place of the range */
      const int64_t c = count[i];
      obs_start[i] = (int32_t)at;
      count[i] = at;
      at += c;
    }
    obs_start[m] = (int32_t)at;
  }
  free(last_slot);
  free(entry_of);
  free(count);
}

/* the header's layout and constants, for the test that holds the Python helpers to them */
EXPORT void newkf_ref_layout(int n_kp, int kp_stride, int m, int obs_cap, int64_t *v) {
  int n = 0;
  v[n++] = SPFE_NEWKF_OFF_CODE;
  v[n++] = (int64_t)SPFE_NEWKF_OFF_ADDED_POINT(n_kp);
  v[n++] = (int64_t)SPFE_NEWKF_OUT_BYTES(n_kp, kp_stride);
  v[n++] = SPFE_LISTOBS_OFF_POINT_IDX;
  v[n++] = (int64_t)SPFE_LISTOBS_OFF_OBS_START(m);
  v[n++] = (int64_t)SPFE_LISTOBS_OFF_REF_SLOT(m);
  v[n++] = (int64_t)SPFE_LISTOBS_OFF_OBS(m);
  v[n++] = (int64_t)SPFE_LISTOBS_OUT_BYTES(m, obs_cap);
  v[n++] = SPFE_NEWKF_ROW_IN_USE; v[n++] = SPFE_NEWKF_BAD_SLOT; v[n++] = SPFE_NEWKF_RECENT_OVERFLOW;
  v[n++] = SPFE_LISTOBS_OVERFLOW; v[n++] = SPFE_LISTOBS_MANY;
  v[n++] = SPFE_NEWKF_OFF_N_NONE; v[n++] = SPFE_NEWKF_OFF_N_RECENT_BEFORE; v[n++] = SPFE_NEWKF_OFF_N_RECENT_AFTER; v[n++] = SPFE_NEWKF_OFF_N_NEEDED;
  v[n++] = SPFE_LISTOBS_OFF_M; v[n++] = SPFE_LISTOBS_OFF_OBS_CAP;
  v[n++] = SPFE_MP_MAX_OBS; v[n++] = SPFE_MP_MAX_POINTS; v[n++] = SPFE_MP_MAX_EDGES;
  v[n++] = SPFE_NEWKF_CODE_REPEATED; v[n++] = SPFE_LISTOBS_CODE_FIRST;
}
