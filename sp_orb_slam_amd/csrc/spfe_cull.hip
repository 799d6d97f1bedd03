// spfe_cull.hip — C ABI of keyframe culling on the device, and its host-array form, on the handle's buffers and streams:
//   the cull loop of the local mapper (local_mapper.cpp:979-1032) with KeyFrame::SetBadFlag (keyframe.cpp:911-997) on the caller's
//   resident rows, flags, observation counts, graph state and tables, and the observation counts from the rows.
// The kernels are cull.hip, the contract include/spfe_cull_math.h.  The entry points end in _resident and keep the device forms'
// contract (include/spfe.h says why); the scratch (h->ck_scratch) grows in a call larger than any before it.
#include "spfe_host.h"
using namespace spfe_host;

namespace {
int ck_check(const spfe_covis_graph *g, int kp_stride, int n_table, int cur_slot, const spfe_cull_params *prm, int n_best_a,
             int n_best_b) {
  int rc = covis_graph_check(g);
  if (rc) return rc;
  if ((rc = rows_check(kp_stride, g->n_slots))) return rc;
  if ((rc = n_table_check(n_table, 0))) return rc;
  if (cur_slot < 0 || cur_slot >= g->n_slots) return fail(SPFE_EINVAL, "cur_slot %d not in [0, %d)", cur_slot, g->n_slots);
  if (prm->th_obs < 1) return fail(SPFE_EINVAL, "th_obs %d < 1", prm->th_obs);
  if (prm->bad_cap < 0 || prm->bad_cap > SPFE_MP_MAX_POINTS)
    return fail(SPFE_EINVAL, "bad_cap %d not in [0, %d]", prm->bad_cap, SPFE_MP_MAX_POINTS);
  if (prm->origin_slot < -1 || prm->origin_slot >= g->n_slots)
    return fail(SPFE_EINVAL, "origin_slot %d not in [-1, %d)", prm->origin_slot, g->n_slots);
  return n_best_check(n_best_a, n_best_b);
}

// The cull on device addresses, wherever they lie (`dg`: the graph of device arrays; first_conn is not read): the caller's or the stage's.
int cull_keyframes(const spfe_covis_graph *dg, void *d_kf_mp_of_kp, int kp_stride, void *d_kf_flags, void *d_mp_flags, void *d_mp_nobs, int n_table,
                   int cur_slot, const spfe_cull_params *prm, void *d_best_cov_a, int n_best_a, void *d_best_cov_b, int n_best_b, void *d_out,
                   uint8_t *d_scratch, hipStream_t s) {
  const spfe::CovisArgs c = covis_state(dg);
  spfe::CullArgs a{};
  a.n_slots = c.n_slots; a.conn_cap = c.conn_cap;
  a.conn_slot = c.conn_slot; a.conn_w = c.conn_w; a.conn_n = c.conn_n;
  a.ord_slot = c.ord_slot; a.ord_w = c.ord_w; a.ord_n = c.ord_n;
  a.parent = c.parent;
  a.kp_stride = kp_stride;
  a.n_table = n_table;
  a.cur_slot = cur_slot;
  a.th_obs = prm->th_obs; a.cov_ratio = prm->cov_ratio; a.origin_slot = prm->origin_slot; a.bad_cap = prm->bad_cap;
  a.n_best_a = n_best_a;
  a.n_best_b = n_best_b;
  a.kf_mp_of_kp = reinterpret_cast<int *>(d_kf_mp_of_kp);
  a.kf_flags = reinterpret_cast<uint8_t *>(d_kf_flags);
  a.mp_flags = reinterpret_cast<uint8_t *>(d_mp_flags);
  a.nobs = reinterpret_cast<int *>(d_mp_nobs);
  a.best_a = reinterpret_cast<int *>(d_best_cov_a);
  a.best_b = reinterpret_cast<int *>(d_best_cov_b);
  a.out = reinterpret_cast<uint8_t *>(d_out);
  a.scratch = d_scratch;
  HIP_TRY(spfe::launch_cull(a, s));
  return SPFE_OK;
}
}  // namespace

extern "C" {

int spfe_count_observations_resident(spfe_handle h, const void *d_kf_mp_of_kp, int kp_stride, const void *d_kf_flags, int n_slots,
                                     void *d_mp_nobs, int n_table, void *stream) {
  if (!h || !d_kf_mp_of_kp || !d_kf_flags || (n_table > 0 && !d_mp_nobs)) return fail(SPFE_EINVAL, "null argument");
  int rc = rows_check(kp_stride, n_slots);
  if (rc) return rc;
  if ((rc = n_table_check(n_table, 0))) return rc;
  if (misaligned(d_kf_mp_of_kp, 4) || misaligned(d_mp_nobs, 4)) return fail(SPFE_EINVAL, "alignment: the int32 arrays 4 bytes");
  HIP_TRY(hipSetDevice(h->cfg.device));
  HIP_TRY(spfe::launch_count_observations(reinterpret_cast<const int *>(d_kf_mp_of_kp), kp_stride,
                                          reinterpret_cast<const uint8_t *>(d_kf_flags), n_slots, reinterpret_cast<int *>(d_mp_nobs),
                                          n_table, stream_of(h, stream)));
  return SPFE_OK;
}

int spfe_cull_keyframes_resident(spfe_handle h, const spfe_covis_graph *graph, void *d_kf_mp_of_kp, int kp_stride, void *d_kf_flags,
                                 void *d_mp_flags, void *d_mp_nobs, int n_table, int cur_slot, const spfe_cull_params *prm,
                                 void *d_best_cov_a, int n_best_a, void *d_best_cov_b, int n_best_b, void *d_out, void *stream) {
  if (!h || !graph || !d_kf_mp_of_kp || !d_kf_flags || !prm || !d_out || (n_table > 0 && (!d_mp_flags || !d_mp_nobs)))
    return fail(SPFE_EINVAL, "null argument");
  int rc = ck_check(graph, kp_stride, n_table, cur_slot, prm, n_best_a, n_best_b);
  if (rc) return rc;
  if (misaligned(d_kf_mp_of_kp, 4) || misaligned(d_mp_nobs, 4) || misaligned(d_best_cov_a, 4) || misaligned(d_best_cov_b, 4) ||
      misaligned(d_out, 16))
    return fail(SPFE_EINVAL, "alignment: the int32 arrays 4 bytes, d_out 16");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = reserve(h, h->ck_scratch, spfe::cull_scratch_bytes(n_table, graph->n_slots, graph->conn_cap)))) return rc;
  return cull_keyframes(graph, d_kf_mp_of_kp, kp_stride, d_kf_flags, d_mp_flags, d_mp_nobs, n_table, cur_slot, prm, d_best_cov_a, n_best_a,
                        d_best_cov_b, n_best_b, d_out, h->ck_scratch.p, stream_of(h, stream));
}

int spfe_cull_keyframes(spfe_handle h, const spfe_covis_graph *graph, int32_t *kf_mp_of_kp, int kp_stride, uint8_t *kf_flags,
                        uint8_t *mp_flags, int32_t *mp_nobs, int n_table, int cur_slot, const spfe_cull_params *prm, int32_t *best_cov_a,
                        int n_best_a, int32_t *best_cov_b, int n_best_b, void *out) {
  if (!h || !graph || !kf_mp_of_kp || !kf_flags || !prm || !out || (n_table > 0 && (!mp_flags || !mp_nobs)))
    return fail(SPFE_EINVAL, "null argument");
  int rc = ck_check(graph, kp_stride, n_table, cur_slot, prm, n_best_a, n_best_b);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t n = (size_t)graph->n_slots, out_b = SPFE_CULL_OUT_BYTES(graph->n_slots, graph->conn_cap, prm->bad_cap);
  HostStage st(h);
  // everything the call edits: the caller's, uploaded, updated in place and fetched whole (first_conn is not written)
  const GraphStage gs(st, graph, false);
  const int b_a = st.inout(best_cov_a, n * n_best_a * 4), b_b = st.inout(best_cov_b, n * n_best_b * 4), b_r = st.inout(kf_mp_of_kp, n * kp_stride * 4),
            b_f = st.inout(kf_flags, n), b_m = st.inout(mp_flags, (size_t)n_table), b_n = st.inout(mp_nobs, (size_t)n_table * 4);
  const int b_s = st.in(nullptr, 0, spfe::cull_scratch_bytes(n_table, graph->n_slots, graph->conn_cap), 16);
  const int b_out = st.out(out_b);   // every byte is written
  if ((rc = st.commit())) return rc;
  const spfe_covis_graph dg = gs.device(st, graph);
  if ((rc = cull_keyframes(&dg, st.dev<void>(b_r), kp_stride, st.dev<void>(b_f), st.dev<void>(b_m), st.dev<void>(b_n), n_table, cur_slot, prm,
                           st.dev_if_given<void>(b_a), n_best_a, st.dev_if_given<void>(b_b), n_best_b, st.dev<void>(b_out), st.dev<uint8_t>(b_s),
                           h->stream)))
    return rc;
  if ((rc = st.fetch_inouts())) return rc;
  if ((rc = st.fetch_to(out, st.dev<void>(b_out), out_b))) return rc;
  return st.sync();
}

}  // extern "C"
