// spfe_lba.hip — C ABI of the two forms around the local bundle adjustment on resident state and of their host-array forms, on the
// handle's buffers and streams: the gather of the problem (optimizer.cpp:447-499, :568-658) and the application of the solver's block
// to the rows, the table and the poses (:660-662, :739-773).  The kernels are lba.hip, the contract include/spfe_lba_math.h.  The
// entry points end in _resident and keep the device forms' contract (include/spfe.h says why); the scratch (h->lb_scratch) grows in
// a call larger than any before it.  spfe_local_ba_records_device (spfe_ba.hip) runs between the two and is not touched.
#include "spfe_host.h"
using namespace spfe_host;

namespace {
int arrays_check(int kp_stride, int n_slots, int n_table) {
  const int rc = rows_check(kp_stride, n_slots);
  return rc ? rc : n_table_check(n_table, 1);
}

int caps_check(int kf_cap, int point_cap, int edge_cap) {
  if (kf_cap < 1 || kf_cap > SPFE_BA_MAX_KEYFRAMES) return fail(SPFE_EINVAL, "kf_cap %d not in [1, %d]", kf_cap, SPFE_BA_MAX_KEYFRAMES);
  if (point_cap < 1 || point_cap > SPFE_BA_MAX_POINTS) return fail(SPFE_EINVAL, "point_cap %d not in [1, %d]", point_cap, SPFE_BA_MAX_POINTS);
  if (edge_cap < 1 || edge_cap > SPFE_BA_MAX_EDGES) return fail(SPFE_EINVAL, "edge_cap %d not in [1, %d]", edge_cap, SPFE_BA_MAX_EDGES);
  return SPFE_OK;
}

int gather_check(int conn_cap, int kp_stride, int n_slots, int n_table, const spfe_lba_gather_params *prm) {
  int rc = arrays_check(kp_stride, n_slots, n_table);
  if (rc) return rc;
  if ((rc = caps_check(prm->kf_cap, prm->point_cap, prm->edge_cap))) return rc;
  if (conn_cap < 1 || conn_cap > SPFE_COVIS_MAX_CONN) return fail(SPFE_EINVAL, "conn_cap %d not in [1, %d]", conn_cap, SPFE_COVIS_MAX_CONN);
  if (prm->free_cap < 1 || prm->free_cap > SPFE_BA_MAX_FREE) return fail(SPFE_EINVAL, "free_cap %d not in [1, %d]", prm->free_cap, SPFE_BA_MAX_FREE);
  if (prm->cur_slot < 0 || prm->cur_slot >= n_slots) return fail(SPFE_EINVAL, "cur_slot %d not in [0, %d)", prm->cur_slot, n_slots);
  if (prm->origin_slot < -1 || prm->origin_slot >= n_slots) return fail(SPFE_EINVAL, "origin_slot %d not in [-1, %d)", prm->origin_slot, n_slots);
  return SPFE_OK;
}

int apply_check(int kp_stride, int n_slots, int n_table, const spfe_lba_apply_params *prm) {
  int rc = arrays_check(kp_stride, n_slots, n_table);
  if (rc) return rc;
  if ((rc = caps_check(prm->kf_cap, prm->point_cap, prm->edge_cap))) return rc;
  if (prm->bad_cap < 0 || prm->bad_cap > SPFE_BA_MAX_POINTS) return fail(SPFE_EINVAL, "bad_cap %d not in [0, %d]", prm->bad_cap, SPFE_BA_MAX_POINTS);
  return SPFE_OK;
}

// The two forms on device addresses, wherever they lie: the caller's or the stage's.  d_ord_row: row cur_slot of the graph's ord_slot.
int gather_local_ba(const void *d_ord_row, int conn_cap, const void *d_kf_mp_of_kp, int kp_stride, const void *d_kf_flags, int n_slots,
                    const void *d_mp_flags, const void *d_xyz, int n_table, const void *d_Tcw, const spfe_lba_gather_params *prm, void *d_out,
                    uint8_t *d_scratch, hipStream_t s) {
  spfe::LbaGatherArgs a{};
  a.conn_cap = conn_cap;
  a.kp_stride = kp_stride;
  a.n_slots = n_slots;
  a.n_table = n_table;
  a.cur_slot = prm->cur_slot; a.origin_slot = prm->origin_slot; a.kf_cap = prm->kf_cap; a.free_cap = prm->free_cap;
  a.point_cap = prm->point_cap; a.edge_cap = prm->edge_cap;
  a.ord_row = reinterpret_cast<const int *>(d_ord_row);
  a.rows = reinterpret_cast<const int *>(d_kf_mp_of_kp);
  a.kf_flags = reinterpret_cast<const uint8_t *>(d_kf_flags);
  a.mp_flags = reinterpret_cast<const uint8_t *>(d_mp_flags);
  a.xyz = reinterpret_cast<const float *>(d_xyz);
  a.Tcw = reinterpret_cast<const float *>(d_Tcw);
  a.out = reinterpret_cast<uint8_t *>(d_out);
  a.scratch = d_scratch;
  HIP_TRY(spfe::launch_lba_gather(a, s));
  return SPFE_OK;
}

int apply_local_ba(const void *d_gather, const void *d_ba_out, void *d_kf_mp_of_kp, int kp_stride, const void *d_kf_flags, int n_slots,
                   void *d_mp_flags, void *d_mp_nobs, void *d_mp_ref_slot, void *d_xyz, int n_table, void *d_Tcw, const spfe_lba_apply_params *prm,
                   void *d_out, uint8_t *d_scratch, hipStream_t s) {
  spfe::LbaApplyArgs a{};
  a.kp_stride = kp_stride;
  a.n_slots = n_slots;
  a.n_table = n_table;
  a.kf_cap = prm->kf_cap; a.point_cap = prm->point_cap; a.edge_cap = prm->edge_cap; a.bad_cap = prm->bad_cap;
  a.gather = reinterpret_cast<const uint8_t *>(d_gather);
  a.ba = reinterpret_cast<const uint8_t *>(d_ba_out);
  a.rows = reinterpret_cast<int *>(d_kf_mp_of_kp);
  a.kf_flags = reinterpret_cast<const uint8_t *>(d_kf_flags);
  a.mp_flags = reinterpret_cast<uint8_t *>(d_mp_flags);
  a.nobs = reinterpret_cast<int *>(d_mp_nobs);
  a.ref_slot = reinterpret_cast<int *>(d_mp_ref_slot);
  a.xyz = reinterpret_cast<float *>(d_xyz);
  a.Tcw = reinterpret_cast<float *>(d_Tcw);
  a.out = reinterpret_cast<uint8_t *>(d_out);
  a.scratch = d_scratch;
  HIP_TRY(spfe::launch_lba_apply(a, s));
  return SPFE_OK;
}
}  // namespace

extern "C" {

int spfe_gather_local_ba_resident(spfe_handle h, const void *d_ord_slot, int conn_cap, const void *d_kf_mp_of_kp, int kp_stride,
                                  const void *d_kf_flags, int n_slots, const void *d_mp_flags, const void *d_xyz, int n_table,
                                  const void *d_Tcw, const spfe_lba_gather_params *prm, void *d_out, void *stream) {
  if (!h || !d_ord_slot || !d_kf_mp_of_kp || !d_kf_flags || !d_mp_flags || !d_xyz || !d_Tcw || !prm || !d_out) return fail(SPFE_EINVAL, "null argument");
  int rc = gather_check(conn_cap, kp_stride, n_slots, n_table, prm);
  if (rc) return rc;
  if (misaligned(d_ord_slot, 4) || misaligned(d_kf_mp_of_kp, 4) || misaligned(d_xyz, 4) || misaligned(d_Tcw, 4) || misaligned(d_out, 16))
    return fail(SPFE_EINVAL, "alignment: the int32 and f32 arrays 4 bytes, d_out 16");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = reserve(h, h->lb_scratch, spfe::lba_gather_scratch_bytes(n_table, n_slots, prm->point_cap, prm->edge_cap)))) return rc;
  return gather_local_ba(reinterpret_cast<const int *>(d_ord_slot) + (size_t)prm->cur_slot * conn_cap, conn_cap, d_kf_mp_of_kp, kp_stride, d_kf_flags,
                         n_slots, d_mp_flags, d_xyz, n_table, d_Tcw, prm, d_out, h->lb_scratch.p, stream_of(h, stream));
}

int spfe_apply_local_ba_resident(spfe_handle h, const void *d_gather, const void *d_ba_out, void *d_kf_mp_of_kp, int kp_stride,
                                 const void *d_kf_flags, int n_slots, void *d_mp_flags, void *d_mp_nobs, void *d_mp_ref_slot, void *d_xyz,
                                 int n_table, void *d_Tcw, const spfe_lba_apply_params *prm, void *d_out, void *stream) {
  if (!h || !d_gather || !d_ba_out || !d_kf_mp_of_kp || !d_kf_flags || !d_mp_flags || !d_mp_nobs || !d_mp_ref_slot || !d_xyz || !d_Tcw || !prm ||
      !d_out)
    return fail(SPFE_EINVAL, "null argument");
  int rc = apply_check(kp_stride, n_slots, n_table, prm);
  if (rc) return rc;
  if (misaligned(d_kf_mp_of_kp, 4) || misaligned(d_mp_nobs, 4) || misaligned(d_mp_ref_slot, 4) || misaligned(d_xyz, 4) || misaligned(d_Tcw, 4) ||
      misaligned(d_gather, 16) || misaligned(d_ba_out, 16) || misaligned(d_out, 16))
    return fail(SPFE_EINVAL, "alignment: the int32 and f32 arrays 4 bytes, the blocks 16");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = reserve(h, h->lb_scratch, spfe::lba_apply_scratch_bytes(prm->point_cap, prm->edge_cap)))) return rc;
  return apply_local_ba(d_gather, d_ba_out, d_kf_mp_of_kp, kp_stride, d_kf_flags, n_slots, d_mp_flags, d_mp_nobs, d_mp_ref_slot, d_xyz, n_table, d_Tcw,
                        prm, d_out, h->lb_scratch.p, stream_of(h, stream));
}

int spfe_gather_local_ba(spfe_handle h, const int32_t *ord_row, int conn_cap, const int32_t *kf_mp_of_kp, int kp_stride, const uint8_t *kf_flags,
                         int n_slots, const uint8_t *mp_flags, const float *xyz, int n_table, const float *Tcw,
                         const spfe_lba_gather_params *prm, void *out) {
  if (!h || !ord_row || !kf_mp_of_kp || !kf_flags || !mp_flags || !xyz || !Tcw || !prm || !out) return fail(SPFE_EINVAL, "null argument");
  int rc = gather_check(conn_cap, kp_stride, n_slots, n_table, prm);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t rows_b = (size_t)n_slots * kp_stride * 4, out_b = SPFE_LBA_GATHER_BYTES(prm->kf_cap, prm->point_cap, prm->edge_cap);
  const auto cap = [](size_t b) { return std::max(b, (size_t)16); };
  HostStage st(h);
  const int b_ord = st.in(ord_row, (size_t)conn_cap * 4, cap((size_t)conn_cap * 4), 16), b_rows = st.in(kf_mp_of_kp, rows_b, cap(rows_b), 16),
            b_kf = st.in(kf_flags, (size_t)n_slots, cap((size_t)n_slots), 16), b_mf = st.in(mp_flags, (size_t)n_table, cap((size_t)n_table), 16),
            b_xyz = st.in(xyz, (size_t)n_table * 12, cap((size_t)n_table * 12), 16), b_T = st.in(Tcw, (size_t)n_slots * 64, (size_t)n_slots * 64, 16),
            b_s = st.in(nullptr, 0, spfe::lba_gather_scratch_bytes(n_table, n_slots, prm->point_cap, prm->edge_cap), 16), b_out = st.out(out_b);
  if ((rc = st.commit())) return rc;
  if ((rc = gather_local_ba(st.dev<void>(b_ord), conn_cap, st.dev<void>(b_rows), kp_stride, st.dev<void>(b_kf), n_slots, st.dev<void>(b_mf),
                            st.dev<void>(b_xyz), n_table, st.dev<void>(b_T), prm, st.dev<void>(b_out), st.dev<uint8_t>(b_s), h->stream)))
    return rc;
  if ((rc = st.fetch_to(out, st.dev<void>(b_out), out_b))) return rc;
  return st.sync();
}

int spfe_apply_local_ba(spfe_handle h, const void *gather, const void *ba_out, int32_t *kf_mp_of_kp, int kp_stride, const uint8_t *kf_flags,
                        int n_slots, uint8_t *mp_flags, int32_t *mp_nobs, int32_t *mp_ref_slot, float *xyz, int n_table, float *Tcw,
                        const spfe_lba_apply_params *prm, void *out) {
  if (!h || !gather || !ba_out || !kf_mp_of_kp || !kf_flags || !mp_flags || !mp_nobs || !mp_ref_slot || !xyz || !Tcw || !prm || !out)
    return fail(SPFE_EINVAL, "null argument");
  int rc = apply_check(kp_stride, n_slots, n_table, prm);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  // the solver's block is as long as the gather's header says; a header the device will refuse gives the solver's header alone
  int32_t gh[16];
  memcpy(gh, gather, sizeof gh);
  const int n_kf = gh[SPFE_LBA_OFF_N_KF / 4], n = gh[SPFE_LBA_OFF_N_POINTS / 4], E = gh[SPFE_LBA_OFF_N_EDGES / 4];
  const bool sane = n_kf >= 1 && n_kf <= prm->kf_cap && n >= 0 && n <= prm->point_cap && E >= 0 && E <= prm->edge_cap;
  const size_t ba_b = sane ? SPFE_BA_OUT_BYTES(n_kf, n, E) : 256, g_b = SPFE_LBA_GATHER_BYTES(prm->kf_cap, prm->point_cap, prm->edge_cap),
               rows_b = (size_t)n_slots * kp_stride * 4, nt = (size_t)n_table, out_b = SPFE_LBA_APPLY_BYTES(prm->point_cap, prm->edge_cap, prm->bad_cap);
  HostStage st(h);
  const int b_g = st.in(gather, g_b, g_b, 256), b_ba = st.in(ba_out, ba_b, ba_b, 256), b_rows = st.inout(kf_mp_of_kp, rows_b),
            b_kf = st.in(kf_flags, (size_t)n_slots, std::max((size_t)n_slots, (size_t)16), 16), b_mf = st.inout(mp_flags, nt),
            b_nobs = st.inout(mp_nobs, nt * 4), b_ref = st.inout(mp_ref_slot, nt * 4), b_xyz = st.inout(xyz, nt * 12),
            b_T = st.inout(Tcw, (size_t)n_slots * 64),
            b_s = st.in(nullptr, 0, spfe::lba_apply_scratch_bytes(prm->point_cap, prm->edge_cap), 16), b_out = st.out(out_b);
  if ((rc = st.commit())) return rc;
  if ((rc = apply_local_ba(st.dev<void>(b_g), st.dev<void>(b_ba), st.dev<void>(b_rows), kp_stride, st.dev<void>(b_kf), n_slots, st.dev<void>(b_mf),
                           st.dev<void>(b_nobs), st.dev<void>(b_ref), st.dev<void>(b_xyz), n_table, st.dev<void>(b_T), prm, st.dev<void>(b_out),
                           st.dev<uint8_t>(b_s), h->stream)))
    return rc;
  if ((rc = st.fetch_inouts())) return rc;
  if ((rc = st.fetch_to(out, st.dev<void>(b_out), out_b))) return rc;
  return st.sync();
}

}  // extern "C"
