// spfe_map.hip — C ABI of the map-point table on the device, and its host-array form, on the handle's buffers and streams:
//   the refresh of a map point   MapPoint::ComputeDistinctiveDescriptors (mappoint.cpp:237-302) and
//                                MapPoint::UpdateNormalAndDepth (:322-364), as the mapper, the optimiser, the loop closer and
//                                the initialiser call them behind every step that changes observations or positions
//   the gather                   table rows -> the point list of the searches
// The kernels are mappoint.hip, the arithmetic include/spfe_mappoint_math.h.
#include "spfe_host.h"
using namespace spfe_host;

namespace {
int mp_check(int m, int E, int n_table, const spfe_mp_params *prm) {
  if (m < 0 || m > SPFE_MP_MAX_POINTS) return fail(SPFE_EINVAL, "m %d not in [0, %d]", m, SPFE_MP_MAX_POINTS);
  if (E < 0 || E > SPFE_MP_MAX_EDGES) return fail(SPFE_EINVAL, "E %d not in [0, %d]", E, SPFE_MP_MAX_EDGES);
  if (n_table < 0) return fail(SPFE_EINVAL, "n_table %d", n_table);
  if (prm->mode == 0 || (prm->mode & ~(SPFE_MP_DESC | SPFE_MP_NORMAL_DEPTH))) return fail(SPFE_EINVAL, "mode %d", prm->mode);
  return SPFE_OK;
}
}  // namespace

extern "C" {

int spfe_mp_lds_obs_capacity(spfe_handle h, int desc_elem_bytes) {
  if (!h) return fail(SPFE_EINVAL, "null argument");
  if (desc_elem_bytes != 2 && desc_elem_bytes != 4) return fail(SPFE_EINVAL, "desc_elem_bytes %d: 2 (bf16) or 4 (f32)", desc_elem_bytes);
  return spfe::mp_lds_obs_capacity(desc_elem_bytes);
}

int spfe_refresh_map_points_device(spfe_handle h, const void *d_kf_records, const void *d_kf_flags, const void *d_Tcw, int n_kf,
                                   const void *d_point_idx, const void *d_obs_start, const void *d_obs, const void *d_ref_slot, int m,
                                   int E, const void *d_xyz, const void *d_flags, void *d_normal, void *d_dist_range, void *d_desc,
                                   int n_table, const spfe_mp_params *prm, void *d_out, void *stream) {
  if (!h || !d_kf_records || !d_kf_flags || !d_Tcw || !d_obs_start || !prm || !d_out || (E > 0 && !d_obs) || (m > 0 && !d_ref_slot) ||
      (n_table > 0 && (!d_xyz || !d_flags || !d_normal || !d_dist_range || !d_desc)))
    return fail(SPFE_EINVAL, "null argument");
  if (n_kf < 1) return fail(SPFE_EINVAL, "n_kf %d < 1", n_kf);
  int rc = mp_check(m, E, n_table, prm);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  spfe::MpArgs a{};
  a.records = reinterpret_cast<const uint8_t *const *>(d_kf_records);
  a.kf_flags = reinterpret_cast<const uint8_t *>(d_kf_flags);
  a.Tcw = reinterpret_cast<const float *>(d_Tcw);
  a.n_kf = n_kf;
  a.off_desc = (long)h->rl.off_desc; a.off_hdr = (long)h->rl.off_hdr;
  a.desc_bf16 = h->rl.desc_bf16; a.kmax = h->kmax;
  a.point_idx = reinterpret_cast<const int *>(d_point_idx);
  a.obs_start = reinterpret_cast<const int *>(d_obs_start);
  a.obs = reinterpret_cast<const int *>(d_obs);
  a.ref_slot = reinterpret_cast<const int *>(d_ref_slot);
  a.m = m; a.E = E;
  a.xyz = reinterpret_cast<const float *>(d_xyz); a.flags = reinterpret_cast<const uint8_t *>(d_flags);
  a.normal = reinterpret_cast<float *>(d_normal); a.dist_range = reinterpret_cast<float *>(d_dist_range);
  a.desc = reinterpret_cast<float *>(d_desc);
  a.n_table = n_table;
  a.mode = prm->mode; a.level_scale = prm->level_scale; a.top_scale = prm->top_scale;
  a.out = reinterpret_cast<uint8_t *>(d_out);
  HIP_TRY(spfe::launch_mp_refresh(a, stream_of(h, stream)));
  return SPFE_OK;
}

int spfe_refresh_map_points(spfe_handle h, const int32_t *obs_start, const float *obs_desc, const uint8_t *obs_good, const float *obs_Ow,
                            int E, const float *ref_Ow, const float *xyz, const uint8_t *flags, int m, const spfe_mp_params *prm,
                            float *normal, float *dist_range, float *desc, void *out) {
  if (!h || !obs_start || !prm || !out || (E > 0 && (!obs_desc || !obs_good || !obs_Ow)) ||
      (m > 0 && (!ref_Ow || !xyz || !flags || !normal || !dist_range || !desc)))
    return fail(SPFE_EINVAL, "null argument");
  int rc = mp_check(m, E, m, prm);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t ne = (size_t)std::max(E, 1), np = (size_t)std::max(m, 1), out_b = SPFE_MP_OUT_BYTES(m);
  HostStage st(h);
  const int b_s = st.in(obs_start, ((size_t)m + 1) * 4, (np + 1) * 4, 16), b_d = st.in(obs_desc, (size_t)E * 1024, ne * 1024, 16),
            b_g = st.in(obs_good, (size_t)E, ne, 16), b_ow = st.in(obs_Ow, (size_t)E * 12, ne * 12, 16),
            b_rw = st.in(ref_Ow, (size_t)m * 12, np * 12, 16), b_p = st.in(xyz, (size_t)m * 12, np * 12, 16),
            b_f = st.in(flags, (size_t)m, np, 16),
            // the outputs start as the caller's: rows that are not written keep their bytes
            b_n = st.in(normal, (size_t)m * 12, np * 12, 16), b_r = st.in(dist_range, (size_t)m * 8, np * 8, 16),
            b_o = st.in(desc, (size_t)m * 1024, np * 1024, 16), b_out = st.out(out_b, out);
  if ((rc = st.commit())) return rc;
  spfe::MpArgs a{};
  a.obs_desc = st.dev<float>(b_d); a.obs_good = st.dev<uint8_t>(b_g);
  a.obs_Ow = st.dev<float>(b_ow); a.ref_Ow = st.dev<float>(b_rw);
  a.obs_start = st.dev<int>(b_s);
  a.m = m; a.E = E;
  a.xyz = st.dev<float>(b_p); a.flags = st.dev<uint8_t>(b_f);
  a.normal = st.dev<float>(b_n); a.dist_range = st.dev<float>(b_r); a.desc = st.dev<float>(b_o);
  a.n_table = m;
  a.mode = prm->mode; a.level_scale = prm->level_scale; a.top_scale = prm->top_scale;
  a.out = st.dev<uint8_t>(b_out);
  HIP_TRY(spfe::launch_mp_refresh(a, h->stream));
  if ((rc = st.fetch_to(normal, a.normal, (size_t)m * 12)) || (rc = st.fetch_to(dist_range, a.dist_range, (size_t)m * 8)) ||
      (rc = st.fetch_to(desc, a.desc, (size_t)m * 1024)) || (rc = st.fetch_to(out, a.out, out_b)))
    return rc;
  return st.sync();
}

int spfe_gather_map_points_device(spfe_handle h, const void *d_idx, int n, const void *d_xyz, const void *d_flags, const void *d_normal,
                                  const void *d_dist_range, const void *d_desc, int n_table, void *d_point_id, void *d_list_xyz,
                                  void *d_list_normal, void *d_list_dist_range, void *d_list_desc, void *d_list_flags, void *stream) {
  if (!h || (n > 0 && (!d_idx || !d_point_id || !d_list_xyz || !d_list_normal || !d_list_dist_range || !d_list_desc || !d_list_flags)) ||
      (n_table > 0 && (!d_xyz || !d_flags || !d_normal || !d_dist_range || !d_desc)))
    return fail(SPFE_EINVAL, "null argument");
  if (n < 0 || n > SPFE_MP_MAX_POINTS) return fail(SPFE_EINVAL, "n %d not in [0, %d]", n, SPFE_MP_MAX_POINTS);
  if (n_table < 0) return fail(SPFE_EINVAL, "n_table %d", n_table);
  HIP_TRY(hipSetDevice(h->cfg.device));
  spfe::MpGatherArgs a{};
  a.idx = reinterpret_cast<const int *>(d_idx);
  a.n = n; a.n_table = n_table;
  a.xyz = reinterpret_cast<const float *>(d_xyz); a.normal = reinterpret_cast<const float *>(d_normal);
  a.dist_range = reinterpret_cast<const float *>(d_dist_range); a.desc = reinterpret_cast<const float *>(d_desc);
  a.flags = reinterpret_cast<const uint8_t *>(d_flags);
  a.o_id = reinterpret_cast<int *>(d_point_id);
  a.o_xyz = reinterpret_cast<float *>(d_list_xyz); a.o_normal = reinterpret_cast<float *>(d_list_normal);
  a.o_dist_range = reinterpret_cast<float *>(d_list_dist_range); a.o_desc = reinterpret_cast<float *>(d_list_desc);
  a.o_flags = reinterpret_cast<uint8_t *>(d_list_flags);
  HIP_TRY(spfe::launch_mp_gather(a, stream_of(h, stream)));
  return SPFE_OK;
}

}  // extern "C"
