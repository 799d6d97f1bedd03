// spfe_mpcull.hip — C ABI of map-point culling on the device and of its resident state, and their host-array forms, on the handle's
// buffers and streams:
//   the preset of the state, the admission of the points spfe_create_map_points_record_device made (local_mapper.cpp:770-787), the
//   found / visible counters of a tracked frame (tracker.cpp:772-807, :576-588) and the cull loop over the recent list
//   (local_mapper.cpp:281-310) on the caller's resident rows, table and state.
// The kernels are mpcull.hip, the contract include/spfe_mpcull_math.h.  The entry points end in _resident and keep the device forms'
// contract (include/spfe.h says why); the scratch (h->mc_scratch) grows in a call larger than any before it.
#include "spfe_host.h"
using namespace spfe_host;

namespace {
int admit_check(const spfe_mp_life *l, int n_neigh, int cur_slot, int kp_stride, int n_slots) {
  int rc = life_check(l, L_ALL);
  if (rc) return rc;
  if ((rc = rows_check(kp_stride, n_slots))) return rc;
  if (n_neigh < 1 || n_neigh > SPFE_TRI_MAX_NEIGHBOURS) return fail(SPFE_EINVAL, "n_neigh %d not in [1, %d]", n_neigh, SPFE_TRI_MAX_NEIGHBOURS);
  if (cur_slot < 0 || cur_slot >= n_slots) return fail(SPFE_EINVAL, "cur_slot %d not in [0, %d)", cur_slot, n_slots);
  return SPFE_OK;
}

int stat_check(const spfe_mp_life *l, int n_kp, int point_cap) {
  int rc = life_check(l, L_FLAGS | L_FOUND | L_VISIBLE);
  if (rc) return rc;
  if (n_kp < 0 || n_kp > SPFE_PROJ_MAX_POINTS) return fail(SPFE_EINVAL, "n_kp %d not in [0, %d]", n_kp, SPFE_PROJ_MAX_POINTS);
  if (point_cap < 1 || point_cap > SPFE_PROJ_MAX_POINTS)
    return fail(SPFE_EINVAL, "point_cap %d not in [1, %d]", point_cap, SPFE_PROJ_MAX_POINTS);
  return SPFE_OK;
}

int cull_check(const spfe_mp_life *l, int kp_stride, int n_slots, const spfe_mpcull_params *prm) {
  int rc = life_check(l, L_ALL);
  if (rc) return rc;
  if ((rc = rows_check(kp_stride, n_slots))) return rc;
  if (prm->th_obs < 0) return fail(SPFE_EINVAL, "th_obs %d < 0", prm->th_obs);
  if (prm->bad_cap < 0 || prm->bad_cap > SPFE_MP_MAX_POINTS)
    return fail(SPFE_EINVAL, "bad_cap %d not in [0, %d]", prm->bad_cap, SPFE_MP_MAX_POINTS);
  return SPFE_OK;
}

// The three forms on device addresses, wherever they lie (`dl`: the state of device arrays): the caller's or the stage's.
int admit_map_points(spfe_handle h, const spfe_mp_life *dl, const void *d_tri_out, int n_neigh, const void *d_neigh_slot, int cur_slot, int cur_kf_id,
                     void *d_kf_mp_of_kp, int kp_stride, int n_slots, void *d_xyz, void *d_out, uint8_t *d_scratch, hipStream_t s) {
  spfe::MpAdmitArgs a{};
  a.life = life_view(dl);
  a.tri = reinterpret_cast<const uint8_t *>(d_tri_out);
  a.tri_stride = SPFE_TRI_OUT_BYTES(h->kmax);
  a.kmax = h->kmax;
  a.n_neigh = n_neigh;
  a.neigh_slot = reinterpret_cast<const int *>(d_neigh_slot);
  a.cur_slot = cur_slot;
  a.cur_kf_id = cur_kf_id;
  a.rows = reinterpret_cast<int *>(d_kf_mp_of_kp);
  a.kp_stride = kp_stride;
  a.n_slots = n_slots;
  a.xyz = reinterpret_cast<float *>(d_xyz);
  a.out = reinterpret_cast<uint8_t *>(d_out);
  a.scratch = d_scratch;
  HIP_TRY(spfe::launch_mp_admit(a, s));
  return SPFE_OK;
}

// (d_in_view, d_outlier: the flag bytes themselves, inside the search's and the pose block or staged)
int track_statistics(const spfe_mp_life *dl, const void *d_mp_of_kp_entry, const void *d_mp_of_kp_after, int n_kp, const void *d_point_idx,
                     int point_cap, const uint8_t *d_in_view, const uint8_t *d_outlier, void *d_out, hipStream_t s) {
  spfe::MpStatArgs a{};
  a.life = life_view(dl);
  a.entry = reinterpret_cast<const int *>(d_mp_of_kp_entry);
  a.after = reinterpret_cast<const int *>(d_mp_of_kp_after);
  a.n_kp = n_kp;
  a.point_idx = reinterpret_cast<const int *>(d_point_idx);
  a.point_cap = point_cap;
  a.in_view = d_in_view;
  a.outlier = d_outlier;
  a.out = reinterpret_cast<uint8_t *>(d_out);
  HIP_TRY(spfe::launch_mp_stat(a, s));
  return SPFE_OK;
}

int cull_map_points(const spfe_mp_life *dl, void *d_kf_mp_of_kp, int kp_stride, const void *d_kf_flags, int n_slots, const spfe_mpcull_params *prm,
                    void *d_out, uint8_t *d_scratch, hipStream_t s) {
  spfe::MpCullArgs a{};
  a.life = life_view(dl);
  a.rows = reinterpret_cast<int *>(d_kf_mp_of_kp);
  a.kp_stride = kp_stride;
  a.n_slots = n_slots;
  a.kf_flags = reinterpret_cast<const uint8_t *>(d_kf_flags);
  a.cur_kf_id = prm->cur_kf_id; a.th_obs = prm->th_obs; a.found_ratio = prm->found_ratio; a.bad_cap = prm->bad_cap;
  a.out = reinterpret_cast<uint8_t *>(d_out);
  a.scratch = d_scratch;
  HIP_TRY(spfe::launch_mp_cull(a, s));
  return SPFE_OK;
}
}  // namespace

extern "C" {

int spfe_mp_life_reset_resident(spfe_handle h, const spfe_mp_life *life, int first_row, int n_rows, int reset_list, void *stream) {
  if (!h || !life) return fail(SPFE_EINVAL, "null argument");
  int rc = life_check(life, L_ALL);
  if (rc) return rc;
  if (first_row < 0 || n_rows < 0 || (long long)first_row + n_rows > life->n_table)
    return fail(SPFE_EINVAL, "rows [%d, %d + %d) not in [0, %d]", first_row, first_row, n_rows, life->n_table);
  if (n_rows == 0 && !reset_list) return fail(SPFE_EINVAL, "nothing to reset");
  HIP_TRY(hipSetDevice(h->cfg.device));
  HIP_TRY(spfe::launch_mp_life_reset(life_view(life), first_row, n_rows, reset_list != 0, stream_of(h, stream)));
  return SPFE_OK;
}

int spfe_admit_map_points_resident(spfe_handle h, const spfe_mp_life *life, const void *d_tri_out, int n_neigh, const void *d_neigh_slot,
                                   int cur_slot, int cur_kf_id, void *d_kf_mp_of_kp, int kp_stride, int n_slots, void *d_xyz, void *d_out,
                                   void *stream) {
  if (!h || !life || !d_tri_out || !d_neigh_slot || !d_kf_mp_of_kp || !d_xyz || !d_out) return fail(SPFE_EINVAL, "null argument");
  int rc = admit_check(life, n_neigh, cur_slot, kp_stride, n_slots);
  if (rc) return rc;
  if (misaligned(d_neigh_slot, 4) || misaligned(d_kf_mp_of_kp, 4) || misaligned(d_xyz, 4) || misaligned(d_tri_out, 16) || misaligned(d_out, 16))
    return fail(SPFE_EINVAL, "alignment: the int32 and f32 arrays 4 bytes, d_tri_out and d_out 16");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = reserve(h, h->mc_scratch, spfe::mpcull_scratch_bytes(life->n_table)))) return rc;
  return admit_map_points(h, life, d_tri_out, n_neigh, d_neigh_slot, cur_slot, cur_kf_id, d_kf_mp_of_kp, kp_stride, n_slots, d_xyz, d_out,
                          h->mc_scratch.p, stream_of(h, stream));
}

int spfe_track_statistics_resident(spfe_handle h, const spfe_mp_life *life, const void *d_mp_of_kp_entry, const void *d_mp_of_kp_after,
                                   int n_kp, const void *d_point_idx, int point_cap, const void *d_proj_out, const void *d_pose_out,
                                   void *d_out, void *stream) {
  if (!h || !life || !d_point_idx || !d_proj_out || !d_pose_out || !d_out || (n_kp > 0 && (!d_mp_of_kp_entry || !d_mp_of_kp_after)))
    return fail(SPFE_EINVAL, "null argument");
  int rc = stat_check(life, n_kp, point_cap);
  if (rc) return rc;
  if (misaligned(d_mp_of_kp_entry, 4) || misaligned(d_mp_of_kp_after, 4) || misaligned(d_point_idx, 4) || misaligned(d_out, 16))
    return fail(SPFE_EINVAL, "alignment: the int32 arrays 4 bytes, d_out 16");
  HIP_TRY(hipSetDevice(h->cfg.device));
  return track_statistics(life, d_mp_of_kp_entry, d_mp_of_kp_after, n_kp, d_point_idx, point_cap,
                          reinterpret_cast<const uint8_t *>(d_proj_out) + SPFE_PROJ_OFF_VIEW,
                          reinterpret_cast<const uint8_t *>(d_pose_out) + SPFE_POSE_OFF_OUTLIER, d_out, stream_of(h, stream));
}

int spfe_cull_map_points_resident(spfe_handle h, const spfe_mp_life *life, void *d_kf_mp_of_kp, int kp_stride, const void *d_kf_flags,
                                  int n_slots, const spfe_mpcull_params *prm, void *d_out, void *stream) {
  if (!h || !life || !d_kf_mp_of_kp || !d_kf_flags || !prm || !d_out) return fail(SPFE_EINVAL, "null argument");
  int rc = cull_check(life, kp_stride, n_slots, prm);
  if (rc) return rc;
  if (misaligned(d_kf_mp_of_kp, 4) || misaligned(d_out, 16)) return fail(SPFE_EINVAL, "alignment: the int32 arrays 4 bytes, d_out 16");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = reserve(h, h->mc_scratch, spfe::mpcull_scratch_bytes(life->n_table)))) return rc;
  return cull_map_points(life, d_kf_mp_of_kp, kp_stride, d_kf_flags, n_slots, prm, d_out, h->mc_scratch.p, stream_of(h, stream));
}

int spfe_admit_map_points(spfe_handle h, const spfe_mp_life *life, const void *tri_out, int n_neigh, const int32_t *neigh_slot, int cur_slot,
                          int cur_kf_id, int32_t *kf_mp_of_kp, int kp_stride, int n_slots, float *xyz, void *out) {
  if (!h || !life || !tri_out || !neigh_slot || !kf_mp_of_kp || !xyz || !out) return fail(SPFE_EINVAL, "null argument");
  int rc = admit_check(life, n_neigh, cur_slot, kp_stride, n_slots);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t tri_b = (size_t)n_neigh * SPFE_TRI_OUT_BYTES(h->kmax), rows_b = (size_t)n_slots * kp_stride * 4, xyz_b = (size_t)life->n_table * 12;
  HostStage st(h);
  const LifeStage ls(st, life);
  const int b_tri = st.in(tri_out, tri_b, tri_b, 256), b_ns = st.in(neigh_slot, (size_t)n_neigh * 4, 16 * 4 * 2, 16),
            b_rows = st.inout(kf_mp_of_kp, rows_b), b_xyz = st.inout(xyz, xyz_b),
            b_s = st.in(nullptr, 0, spfe::mpcull_scratch_bytes(life->n_table), 16), b_out = st.out(SPFE_ADMIT_OUT_BYTES);
  if ((rc = st.commit())) return rc;
  const spfe_mp_life dl = ls.device(st, life);
  if ((rc = admit_map_points(h, &dl, st.dev<void>(b_tri), n_neigh, st.dev<void>(b_ns), cur_slot, cur_kf_id, st.dev<void>(b_rows), kp_stride, n_slots,
                             st.dev<void>(b_xyz), st.dev<void>(b_out), st.dev<uint8_t>(b_s), h->stream)))
    return rc;
  if ((rc = st.fetch_inouts())) return rc;
  if ((rc = st.fetch_to(out, st.dev<void>(b_out), SPFE_ADMIT_OUT_BYTES))) return rc;
  return st.sync();
}

int spfe_track_statistics(spfe_handle h, const spfe_mp_life *life, const int32_t *mp_of_kp_entry, const int32_t *mp_of_kp_after, int n_kp,
                          const int32_t *point_idx, int point_cap, const uint8_t *in_view, const uint8_t *outlier, void *out) {
  if (!h || !life || !point_idx || !in_view || !out || (n_kp > 0 && (!mp_of_kp_entry || !mp_of_kp_after || !outlier)))
    return fail(SPFE_EINVAL, "null argument");
  int rc = stat_check(life, n_kp, point_cap);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t kb = (size_t)n_kp * 4, kc = std::max(kb, (size_t)16);
  HostStage st(h);
  const LifeStage ls(st, life);
  const int b_e = st.in(mp_of_kp_entry, kb, kc, 16), b_a = st.in(mp_of_kp_after, kb, kc, 16),
            b_p = st.in(point_idx, (size_t)point_cap * 4, (size_t)point_cap * 4, 16), b_v = st.in(in_view, (size_t)point_cap, (size_t)point_cap, 16),
            b_o = st.in(outlier, (size_t)n_kp, std::max((size_t)n_kp, (size_t)16), 16), b_out = st.out(SPFE_MPSTAT_OUT_BYTES);
  if ((rc = st.commit())) return rc;
  const spfe_mp_life dl = ls.device(st, life);
  if ((rc = track_statistics(&dl, st.dev<void>(b_e), st.dev<void>(b_a), n_kp, st.dev<void>(b_p), point_cap, st.dev<uint8_t>(b_v), st.dev<uint8_t>(b_o),
                             st.dev<void>(b_out), h->stream)))
    return rc;
  if ((rc = st.fetch_inouts())) return rc;
  if ((rc = st.fetch_to(out, st.dev<void>(b_out), SPFE_MPSTAT_OUT_BYTES))) return rc;
  return st.sync();
}

int spfe_cull_map_points(spfe_handle h, const spfe_mp_life *life, int32_t *kf_mp_of_kp, int kp_stride, const uint8_t *kf_flags, int n_slots,
                         const spfe_mpcull_params *prm, void *out) {
  if (!h || !life || !kf_mp_of_kp || !kf_flags || !prm || !out) return fail(SPFE_EINVAL, "null argument");
  int rc = cull_check(life, kp_stride, n_slots, prm);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t rows_b = (size_t)n_slots * kp_stride * 4, out_b = SPFE_MPCULL_OUT_BYTES(life->recent_cap, prm->bad_cap);
  HostStage st(h);
  const LifeStage ls(st, life);
  const int b_rows = st.inout(kf_mp_of_kp, rows_b), b_f = st.in(kf_flags, (size_t)n_slots, std::max((size_t)n_slots, (size_t)16), 16),
            b_s = st.in(nullptr, 0, spfe::mpcull_scratch_bytes(life->n_table), 16), b_out = st.out(out_b);   // every byte is written
  if ((rc = st.commit())) return rc;
  const spfe_mp_life dl = ls.device(st, life);
  if ((rc = cull_map_points(&dl, st.dev<void>(b_rows), kp_stride, st.dev<void>(b_f), n_slots, prm, st.dev<void>(b_out), st.dev<uint8_t>(b_s), h->stream)))
    return rc;
  if ((rc = st.fetch_inouts())) return rc;
  if ((rc = st.fetch_to(out, st.dev<void>(b_out), out_b))) return rc;
  return st.sync();
}

}  // extern "C"
