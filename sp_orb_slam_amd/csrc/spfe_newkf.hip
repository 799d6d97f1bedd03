// spfe_newkf.hip — C ABI of a new keyframe on resident state and of the observation lists of the refreshes, and their host-array
// forms, on the handle's buffers and streams:
//   the insertion of the keyframe's row with its counts, flags, list entries and track descriptors (local_mapper.cpp:255-272 without
//   the refresh), and the (d_obs_start, d_obs, d_ref_slot) of any list of points from one scan of the caller's resident rows.
// The kernels are newkf.hip, the contract include/spfe_newkf_math.h.  The entry points end in _resident and keep the device forms'
// contract (include/spfe.h says why); the scratch (h->nk_scratch) grows in a call larger than any before it.
#include "spfe_host.h"
using namespace spfe_host;

namespace {
constexpr unsigned L_INSERT = L_FLAGS | L_NOBS | L_LIST;   // what an insertion touches of the state

int insert_check(spfe_handle h, const spfe_mp_life *l, int n_kp, int cur_slot, int kp_stride, int n_slots, bool with_desc) {
  int rc = life_check(l, L_INSERT);
  if (rc) return rc;
  if ((rc = rows_check(kp_stride, n_slots))) return rc;
  if (n_kp < 0 || n_kp > kp_stride) return fail(SPFE_EINVAL, "n_kp %d not in [0, kp_stride %d]", n_kp, kp_stride);
  if (with_desc && n_kp > h->kmax) return fail(SPFE_EINVAL, "n_kp %d beyond the record's %d descriptor rows", n_kp, h->kmax);
  if (cur_slot < 0 || cur_slot >= n_slots) return fail(SPFE_EINVAL, "cur_slot %d not in [0, %d)", cur_slot, n_slots);
  return SPFE_OK;
}

int list_check(int first_row, int m, int kp_stride, int n_slots, int n_table, int obs_cap) {
  int rc = n_table_check(n_table, 1);
  if (rc) return rc;
  if ((rc = rows_check(kp_stride, n_slots))) return rc;
  if (m < 0 || m > SPFE_MP_MAX_POINTS) return fail(SPFE_EINVAL, "m %d not in [0, %d]", m, SPFE_MP_MAX_POINTS);
  if (obs_cap < 0 || obs_cap > SPFE_MP_MAX_EDGES) return fail(SPFE_EINVAL, "obs_cap %d not in [0, %d]", obs_cap, SPFE_MP_MAX_EDGES);
  if (first_row < 0) return fail(SPFE_EINVAL, "first_row %d < 0", first_row);
  return SPFE_OK;
}

// The two forms on device addresses, wherever they lie (`dl`: the state of device arrays): the caller's or the stage's.
int insert_keyframe(spfe_handle h, const spfe_mp_life *dl, const void *d_frame_mp_of_kp, int n_kp, int cur_slot, void *d_kf_mp_of_kp, int kp_stride,
                    const void *d_kf_flags, int n_slots, const void *d_kf_record, void *d_desc_track, void *d_out, uint8_t *d_scratch, hipStream_t s) {
  spfe::NewKfArgs a{};
  a.life = life_view(dl);
  a.frame = reinterpret_cast<const int *>(d_frame_mp_of_kp);
  a.n_kp = n_kp;
  a.cur_slot = cur_slot;
  a.rows = reinterpret_cast<int *>(d_kf_mp_of_kp);
  a.kp_stride = kp_stride;
  a.n_slots = n_slots;
  a.kf_flags = reinterpret_cast<const uint8_t *>(d_kf_flags);
  a.rec_desc = d_kf_record && d_desc_track ? reinterpret_cast<const uint8_t *>(d_kf_record) + h->rl.off_desc : nullptr;
  a.desc_bf16 = h->rl.desc_bf16;
  a.desc_track = d_kf_record && d_desc_track ? reinterpret_cast<float *>(d_desc_track) : nullptr;
  a.out = reinterpret_cast<uint8_t *>(d_out);
  a.scratch = d_scratch;
  HIP_TRY(spfe::launch_insert_keyframe(a, s));
  return SPFE_OK;
}

int list_observations(const void *d_point_idx, int first_row, int m, const void *d_kf_mp_of_kp, int kp_stride, const void *d_kf_flags, int n_slots,
                      const void *d_mp_ref_slot, int n_table, int obs_cap, void *d_out, uint8_t *d_scratch, hipStream_t s) {
  spfe::ListObsArgs a{};
  a.point_idx = reinterpret_cast<const int *>(d_point_idx);
  a.first_row = first_row;
  a.m = m;
  a.rows = reinterpret_cast<const int *>(d_kf_mp_of_kp);
  a.kp_stride = kp_stride;
  a.n_slots = n_slots;
  a.kf_flags = reinterpret_cast<const uint8_t *>(d_kf_flags);
  a.mp_ref_slot = reinterpret_cast<const int *>(d_mp_ref_slot);
  a.n_table = n_table;
  a.obs_cap = obs_cap;
  a.out = reinterpret_cast<uint8_t *>(d_out);
  a.scratch = d_scratch;
  HIP_TRY(spfe::launch_list_observations(a, s));
  return SPFE_OK;
}
}  // namespace

extern "C" {

int spfe_insert_keyframe_resident(spfe_handle h, const spfe_mp_life *life, const void *d_frame_mp_of_kp, int n_kp, int cur_slot, void *d_kf_mp_of_kp,
                                  int kp_stride, const void *d_kf_flags, int n_slots, const void *d_kf_record, void *d_desc_track, void *d_out,
                                  void *stream) {
  if (!h || !life || (n_kp > 0 && !d_frame_mp_of_kp) || !d_kf_mp_of_kp || !d_kf_flags || !d_out) return fail(SPFE_EINVAL, "null argument");
  int rc = insert_check(h, life, n_kp, cur_slot, kp_stride, n_slots, d_kf_record && d_desc_track);
  if (rc) return rc;
  if (misaligned(d_frame_mp_of_kp, 4) || misaligned(d_kf_mp_of_kp, 4) || misaligned(d_kf_record, 16) || misaligned(d_desc_track, 16) ||
      misaligned(d_out, 16))
    return fail(SPFE_EINVAL, "alignment: the int32 arrays 4 bytes, d_kf_record, d_desc_track and d_out 16");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = reserve(h, h->nk_scratch, spfe::newkf_scratch_bytes(life->n_table)))) return rc;
  return insert_keyframe(h, life, d_frame_mp_of_kp, n_kp, cur_slot, d_kf_mp_of_kp, kp_stride, d_kf_flags, n_slots, d_kf_record, d_desc_track, d_out,
                         h->nk_scratch.p, stream_of(h, stream));
}

int spfe_list_observations_resident(spfe_handle h, const void *d_point_idx, int first_row, int m, const void *d_kf_mp_of_kp, int kp_stride,
                                    const void *d_kf_flags, int n_slots, const void *d_mp_ref_slot, int n_table, int obs_cap, void *d_out,
                                    void *stream) {
  if (!h || !d_kf_mp_of_kp || !d_kf_flags || !d_mp_ref_slot || !d_out) return fail(SPFE_EINVAL, "null argument");
  int rc = list_check(first_row, m, kp_stride, n_slots, n_table, obs_cap);
  if (rc) return rc;
  if (misaligned(d_point_idx, 4) || misaligned(d_kf_mp_of_kp, 4) || misaligned(d_mp_ref_slot, 4) || misaligned(d_out, 16))
    return fail(SPFE_EINVAL, "alignment: the int32 arrays 4 bytes, d_out 16");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = reserve(h, h->nk_scratch, spfe::listobs_scratch_bytes(n_table, m, obs_cap)))) return rc;
  return list_observations(d_point_idx, first_row, m, d_kf_mp_of_kp, kp_stride, d_kf_flags, n_slots, d_mp_ref_slot, n_table, obs_cap, d_out,
                           h->nk_scratch.p, stream_of(h, stream));
}

int spfe_insert_keyframe(spfe_handle h, const spfe_mp_life *life, const int32_t *frame_mp_of_kp, int n_kp, int cur_slot, int32_t *kf_mp_of_kp,
                         int kp_stride, const uint8_t *kf_flags, int n_slots, const void *kf_record, float *desc_track, void *out) {
  if (!h || !life || (n_kp > 0 && !frame_mp_of_kp) || !kf_mp_of_kp || !kf_flags || !out) return fail(SPFE_EINVAL, "null argument");
  const bool with_desc = kf_record && desc_track;
  int rc = insert_check(h, life, n_kp, cur_slot, kp_stride, n_slots, with_desc);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t kb = (size_t)n_kp * 4, rows_b = (size_t)n_slots * kp_stride * 4, out_b = SPFE_NEWKF_OUT_BYTES(n_kp, kp_stride);
  HostStage st(h);
  const LifeStage ls(st, life);
  const int b_f = st.in(frame_mp_of_kp, kb, std::max(kb, (size_t)16), 16), b_rows = st.inout(kf_mp_of_kp, rows_b),
            b_fl = st.in(kf_flags, (size_t)n_slots, std::max((size_t)n_slots, (size_t)16), 16),
            b_rec = st.in(with_desc ? kf_record : nullptr, h->rl.bytes, with_desc ? h->rl.bytes : 16, 256),
            b_dt = st.inout(with_desc ? desc_track : nullptr, (size_t)life->n_table * 1024),
            b_s = st.in(nullptr, 0, spfe::newkf_scratch_bytes(life->n_table), 16), b_out = st.out(out_b);   // every byte is written
  if ((rc = st.commit())) return rc;
  const spfe_mp_life dl = ls.device(st, life);
  if ((rc = insert_keyframe(h, &dl, st.dev<void>(b_f), n_kp, cur_slot, st.dev<void>(b_rows), kp_stride, st.dev<void>(b_fl), n_slots,
                            with_desc ? st.dev<void>(b_rec) : nullptr, with_desc ? st.dev<void>(b_dt) : nullptr, st.dev<void>(b_out),
                            st.dev<uint8_t>(b_s), h->stream)))
    return rc;
  if ((rc = st.fetch_inouts())) return rc;
  if ((rc = st.fetch_to(out, st.dev<void>(b_out), out_b))) return rc;
  return st.sync();
}

int spfe_list_observations(spfe_handle h, const int32_t *point_idx, int first_row, int m, const int32_t *kf_mp_of_kp, int kp_stride,
                           const uint8_t *kf_flags, int n_slots, const int32_t *mp_ref_slot, int n_table, int obs_cap, void *out) {
  if (!h || !kf_mp_of_kp || !kf_flags || !mp_ref_slot || !out) return fail(SPFE_EINVAL, "null argument");
  int rc = list_check(first_row, m, kp_stride, n_slots, n_table, obs_cap);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t mb = (size_t)m * 4, rows_b = (size_t)n_slots * kp_stride * 4, out_b = SPFE_LISTOBS_OUT_BYTES(m, obs_cap);
  HostStage st(h);
  const int b_p = st.in(point_idx, mb, std::max(mb, (size_t)16), 16), b_rows = st.in(kf_mp_of_kp, rows_b, rows_b, 16),
            b_fl = st.in(kf_flags, (size_t)n_slots, std::max((size_t)n_slots, (size_t)16), 16),
            b_rs = st.in(mp_ref_slot, (size_t)n_table * 4, (size_t)n_table * 4, 16),
            b_s = st.in(nullptr, 0, spfe::listobs_scratch_bytes(n_table, m, obs_cap), 16), b_out = st.out(out_b);   // every byte is written
  if ((rc = st.commit())) return rc;
  if ((rc = list_observations(st.dev_if_given<void>(b_p), first_row, m, st.dev<void>(b_rows), kp_stride, st.dev<void>(b_fl), n_slots, st.dev<void>(b_rs),
                              n_table, obs_cap, st.dev<void>(b_out), st.dev<uint8_t>(b_s), h->stream)))
    return rc;
  if ((rc = st.fetch_to(out, st.dev<void>(b_out), out_b))) return rc;
  return st.sync();
}

}  // extern "C"
