// spfe_localmap.hip — C ABI of the tracker's local map on the device, and its host-array form, on the handle's buffers and streams:
//   Tracking::UpdateLocalKeyFrames (tracker.cpp:868-984) and UpdateLocalPoints (:843-866) on the caller's resident keyframe rows,
//   the count of KeyFrame::getTrackedInCommon (keyframe.cpp:697-724), and the list positions back into table rows.
// The kernels are localmap.hip, the contract include/spfe_localmap_math.h.  The entry points end in _resident and keep the device
// forms' contract (include/spfe.h says why); the per-point scratch is the handle's and grows, as the essential graph's does, in a
// call larger than any before it.
#include "spfe_host.h"
using namespace spfe_host;

namespace {
int lm_vote_check(int kp_stride, int n_slots, int n_table, int n_kp) {
  int rc = rows_check(kp_stride, n_slots);
  if (rc) return rc;
  if ((rc = n_table_check(n_table, 0))) return rc;
  if (n_kp < 0 || n_kp > SPFE_PROJ_MAX_POINTS) return fail(SPFE_EINVAL, "n_kp %d not in [0, %d]", n_kp, SPFE_PROJ_MAX_POINTS);
  return SPFE_OK;
}
int lm_check(int kp_stride, int n_best, int n_slots, int n_table, int n_kp, const spfe_localmap_params *prm) {
  int rc = lm_vote_check(kp_stride, n_slots, n_table, n_kp);
  if (rc) return rc;
  if (n_best < 1 || n_best > SPFE_LOCALMAP_MAX_BEST) return fail(SPFE_EINVAL, "n_best %d not in [1, %d]", n_best, SPFE_LOCALMAP_MAX_BEST);
  if (prm->point_cap < 1 || prm->point_cap > SPFE_PROJ_MAX_POINTS)
    return fail(SPFE_EINVAL, "point_cap %d not in [1, %d]", prm->point_cap, SPFE_PROJ_MAX_POINTS);
  if (n_kp > prm->point_cap) return fail(SPFE_EINVAL, "n_kp %d above point_cap %d", n_kp, prm->point_cap);
  if (prm->max_keyframes < 0) return fail(SPFE_EINVAL, "max_keyframes %d < 0", prm->max_keyframes);
  return SPFE_OK;
}

// The local map on device addresses, wherever they lie: the caller's (the resident form) or the stage's (the host-array form).
int update_local_map(const void *d_kf_mp_of_kp, int kp_stride, const void *d_kf_flags, const void *d_best_cov, int n_best, const void *d_parent,
                     int n_slots, const void *d_mp_flags, int n_table, const void *d_mp_of_kp, int n_kp, const spfe_localmap_params *prm,
                     void *d_out, uint8_t *d_scratch, hipStream_t s) {
  spfe::LocalmapArgs a{};
  a.kf_mp_of_kp = reinterpret_cast<const int *>(d_kf_mp_of_kp);
  a.kp_stride = kp_stride;
  a.kf_flags = reinterpret_cast<const uint8_t *>(d_kf_flags);
  a.best_cov = reinterpret_cast<const int *>(d_best_cov);
  a.n_best = n_best;
  a.parent = reinterpret_cast<const int *>(d_parent);
  a.n_slots = n_slots;
  a.mp_flags = reinterpret_cast<const uint8_t *>(d_mp_flags);
  a.n_table = n_table;
  a.mp_of_kp = reinterpret_cast<const int *>(d_mp_of_kp);
  a.n_kp = n_kp;
  a.max_keyframes = prm->max_keyframes; a.point_cap = prm->point_cap;
  a.out = reinterpret_cast<uint8_t *>(d_out);
  a.votes = reinterpret_cast<int *>(a.out + SPFE_LOCALMAP_OFF_VOTES(n_slots));
  a.total = reinterpret_cast<int *>(a.out + SPFE_LOCALMAP_OFF_TOTAL(n_slots));
  a.scratch = d_scratch;
  HIP_TRY(spfe::launch_localmap(a, s));
  return SPFE_OK;
}
}  // namespace

extern "C" {

int spfe_localmap_lds_point_capacity(spfe_handle h) {
  if (!h) return fail(SPFE_EINVAL, "null argument");
  return spfe::localmap_lds_point_capacity();
}

int spfe_update_local_map_resident(spfe_handle h, const void *d_kf_mp_of_kp, int kp_stride, const void *d_kf_flags, const void *d_best_cov,
                                   int n_best, const void *d_parent, int n_slots, const void *d_mp_flags, int n_table,
                                   const void *d_mp_of_kp, int n_kp, const spfe_localmap_params *prm, void *d_out, void *stream) {
  if (!h || !d_kf_mp_of_kp || !d_kf_flags || !d_best_cov || !d_parent || !prm || !d_out || (n_table > 0 && !d_mp_flags) ||
      (n_kp > 0 && !d_mp_of_kp))
    return fail(SPFE_EINVAL, "null argument");
  int rc = lm_check(kp_stride, n_best, n_slots, n_table, n_kp, prm);
  if (rc) return rc;
  if (misaligned(d_kf_mp_of_kp, 4) || misaligned(d_best_cov, 4) || misaligned(d_parent, 4) || misaligned(d_mp_of_kp, 4) ||
      misaligned(d_out, 16))
    return fail(SPFE_EINVAL, "alignment: the int32 arrays 4 bytes, d_out 16");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = reserve(h, h->lm_scratch, spfe::localmap_scratch_bytes(n_table)))) return rc;
  return update_local_map(d_kf_mp_of_kp, kp_stride, d_kf_flags, d_best_cov, n_best, d_parent, n_slots, d_mp_flags, n_table, d_mp_of_kp, n_kp, prm,
                          d_out, h->lm_scratch.p, stream_of(h, stream));
}

int spfe_count_shared_points_resident(spfe_handle h, const void *d_kf_mp_of_kp, int kp_stride, int n_slots, const void *d_mp_flags,
                                      int n_table, const void *d_mp_of_kp, const void *d_outlier, int n_kp, void *d_votes, void *d_total,
                                      void *stream) {
  if (!h || !d_kf_mp_of_kp || !d_votes || !d_total || (n_table > 0 && !d_mp_flags) || (n_kp > 0 && !d_mp_of_kp))
    return fail(SPFE_EINVAL, "null argument");
  int rc = lm_vote_check(kp_stride, n_slots, n_table, n_kp);
  if (rc) return rc;
  if (misaligned(d_kf_mp_of_kp, 4) || misaligned(d_mp_of_kp, 4) || misaligned(d_votes, 4) || misaligned(d_total, 4))
    return fail(SPFE_EINVAL, "alignment: the int32 arrays 4 bytes");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = reserve(h, h->lm_scratch, spfe::localmap_scratch_bytes(n_table)))) return rc;
  spfe::LocalmapArgs a{};
  a.kf_mp_of_kp = reinterpret_cast<const int *>(d_kf_mp_of_kp);
  a.kp_stride = kp_stride;
  a.n_slots = n_slots;
  a.mp_flags = reinterpret_cast<const uint8_t *>(d_mp_flags);
  a.n_table = n_table;
  a.mp_of_kp = reinterpret_cast<const int *>(d_mp_of_kp);
  a.outlier = reinterpret_cast<const uint8_t *>(d_outlier);
  a.n_kp = n_kp;
  a.votes = reinterpret_cast<int *>(d_votes);
  a.total = reinterpret_cast<int *>(d_total);
  a.scratch = h->lm_scratch.p;
  HIP_TRY(spfe::launch_localmap_count(a, stream_of(h, stream)));
  return SPFE_OK;
}

int spfe_local_map_rows_resident(spfe_handle h, const void *d_point_idx, int point_cap, const void *d_mp_of_kp_list, int n_kp,
                                 void *d_mp_of_kp_rows, void *stream) {
  if (!h || !d_point_idx || (n_kp > 0 && (!d_mp_of_kp_list || !d_mp_of_kp_rows))) return fail(SPFE_EINVAL, "null argument");
  if (point_cap < 1 || point_cap > SPFE_PROJ_MAX_POINTS)
    return fail(SPFE_EINVAL, "point_cap %d not in [1, %d]", point_cap, SPFE_PROJ_MAX_POINTS);
  if (n_kp < 0 || n_kp > SPFE_PROJ_MAX_POINTS) return fail(SPFE_EINVAL, "n_kp %d not in [0, %d]", n_kp, SPFE_PROJ_MAX_POINTS);
  if (misaligned(d_point_idx, 4) || misaligned(d_mp_of_kp_list, 4) || misaligned(d_mp_of_kp_rows, 4))
    return fail(SPFE_EINVAL, "alignment: the int32 arrays 4 bytes");
  HIP_TRY(hipSetDevice(h->cfg.device));
  HIP_TRY(spfe::launch_localmap_rows(reinterpret_cast<const int *>(d_point_idx), point_cap, reinterpret_cast<const int *>(d_mp_of_kp_list),
                                     n_kp, reinterpret_cast<int *>(d_mp_of_kp_rows), stream_of(h, stream)));
  return SPFE_OK;
}

int spfe_update_local_map(spfe_handle h, const int32_t *kf_mp_of_kp, int kp_stride, const uint8_t *kf_flags, const int32_t *best_cov,
                          int n_best, const int32_t *parent, int n_slots, const uint8_t *mp_flags, int n_table, const int32_t *mp_of_kp,
                          int n_kp, const spfe_localmap_params *prm, void *out) {
  if (!h || !kf_mp_of_kp || !kf_flags || !best_cov || !parent || !prm || !out || (n_table > 0 && !mp_flags) || (n_kp > 0 && !mp_of_kp))
    return fail(SPFE_EINVAL, "null argument");
  int rc = lm_check(kp_stride, n_best, n_slots, n_table, n_kp, prm);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t n = (size_t)n_slots, out_b = SPFE_LOCALMAP_OUT_BYTES(n_slots, prm->point_cap, n_kp);
  HostStage st(h);
  const int b_r = st.in(kf_mp_of_kp, n * kp_stride * 4, n * kp_stride * 4, 16), b_f = st.in(kf_flags, n, n, 16),
            b_c = st.in(best_cov, n * n_best * 4, n * n_best * 4, 16), b_p = st.in(parent, n * 4, n * 4, 16),
            b_m = st.in(mp_flags, (size_t)n_table, (size_t)std::max(n_table, 1), 16),
            b_k = st.in(mp_of_kp, (size_t)n_kp * 4, (size_t)std::max(n_kp, 1) * 4, 16),
            b_s = st.in(nullptr, 0, spfe::localmap_scratch_bytes(n_table), 16), b_out = st.out(out_b);   // every byte is written
  if ((rc = st.commit())) return rc;
  if ((rc = update_local_map(st.dev<void>(b_r), kp_stride, st.dev<void>(b_f), st.dev<void>(b_c), n_best, st.dev<void>(b_p), n_slots,
                             st.dev<void>(b_m), n_table, st.dev<void>(b_k), n_kp, prm, st.dev<void>(b_out), st.dev<uint8_t>(b_s), h->stream)))
    return rc;
  if ((rc = st.fetch_to(out, st.dev<void>(b_out), out_b))) return rc;
  return st.sync();
}

}  // extern "C"
