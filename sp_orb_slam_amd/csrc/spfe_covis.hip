// spfe_covis.hip — C ABI of the covisibility graph on the device, and its host-array form, on the handle's buffers and streams:
//   KeyFrame::UpdateConnections (keyframe.cpp:757-849) with AddConnection / UpdateBestCovisibles (:577-612) on the caller's resident
//   keyframe rows and resident graph state, and the preset of a range of slots.
// The kernels are covis.hip (and localmap.hip's count), the contract include/spfe_covis_math.h.  The entry points end in _resident
// and keep the device forms' contract (include/spfe.h says why); the scratch is the local map's (h->lm_scratch: the two calls
// follow each other on one stream) and grows in a call larger than any before it.
#include "spfe_host.h"
using namespace spfe_host;

int spfe_host::covis_graph_check(const spfe_covis_graph *g) {
  if (!g->d_conn_slot || !g->d_conn_w || !g->d_conn_n || !g->d_ord_slot || !g->d_ord_w || !g->d_ord_n || !g->d_parent || !g->d_first_conn)
    return fail(SPFE_EINVAL, "null argument");
  int rc = n_slots_check(g->n_slots);
  if (rc) return rc;
  if (g->conn_cap < 1 || g->conn_cap > SPFE_COVIS_MAX_CONN)
    return fail(SPFE_EINVAL, "conn_cap %d not in [1, %d]", g->conn_cap, SPFE_COVIS_MAX_CONN);
  if (misaligned(g->d_conn_slot, 4) || misaligned(g->d_conn_w, 4) || misaligned(g->d_conn_n, 4) || misaligned(g->d_ord_slot, 4) ||
      misaligned(g->d_ord_w, 4) || misaligned(g->d_ord_n, 4) || misaligned(g->d_parent, 4))
    return fail(SPFE_EINVAL, "alignment: the int32 arrays 4 bytes");
  return SPFE_OK;
}

spfe::CovisArgs spfe_host::covis_state(const spfe_covis_graph *g) {
  spfe::CovisArgs a{};
  a.n_slots = g->n_slots;
  a.conn_cap = g->conn_cap;
  a.conn_slot = reinterpret_cast<int *>(g->d_conn_slot);
  a.conn_w = reinterpret_cast<int *>(g->d_conn_w);
  a.conn_n = reinterpret_cast<int *>(g->d_conn_n);
  a.ord_slot = reinterpret_cast<int *>(g->d_ord_slot);
  a.ord_w = reinterpret_cast<int *>(g->d_ord_w);
  a.ord_n = reinterpret_cast<int *>(g->d_ord_n);
  a.parent = reinterpret_cast<int *>(g->d_parent);
  a.first_conn = reinterpret_cast<uint8_t *>(g->d_first_conn);
  return a;
}

namespace {
int cv_check(const spfe_covis_graph *g, int kp_stride, int n_table, int cur_slot, const spfe_covis_params *prm, int n_best_a,
             int n_best_b) {
  int rc = covis_graph_check(g);
  if (rc) return rc;
  if ((rc = kp_stride_check(kp_stride))) return rc;
  if ((rc = n_table_check(n_table, 0))) return rc;
  if (cur_slot < 0 || cur_slot >= g->n_slots) return fail(SPFE_EINVAL, "cur_slot %d not in [0, %d)", cur_slot, g->n_slots);
  if (prm->th < 1) return fail(SPFE_EINVAL, "th %d < 1", prm->th);
  if (prm->origin_slot < -1 || prm->origin_slot >= g->n_slots)
    return fail(SPFE_EINVAL, "origin_slot %d not in [-1, %d)", prm->origin_slot, g->n_slots);
  return n_best_check(n_best_a, n_best_b);
}

// UpdateConnections on device addresses, wherever they lie (`dg`: the graph of device arrays): the caller's or the stage's.
int update_connections(const spfe_covis_graph *dg, const void *d_kf_mp_of_kp, int kp_stride, const void *d_kf_flags, const void *d_mp_flags,
                       int n_table, int cur_slot, const spfe_covis_params *prm, void *d_best_cov_a, int n_best_a, void *d_best_cov_b,
                       int n_best_b, void *d_out, uint8_t *d_scratch, hipStream_t s) {
  spfe::CovisArgs a = covis_state(dg);
  a.kf_mp_of_kp = reinterpret_cast<const int *>(d_kf_mp_of_kp);
  a.kp_stride = kp_stride;
  a.kf_flags = reinterpret_cast<const uint8_t *>(d_kf_flags);
  a.mp_flags = reinterpret_cast<const uint8_t *>(d_mp_flags);
  a.n_table = n_table;
  a.cur_slot = cur_slot;
  a.th = prm->th; a.origin_slot = prm->origin_slot;
  a.best_a = reinterpret_cast<int *>(d_best_cov_a);
  a.n_best_a = n_best_a;
  a.best_b = reinterpret_cast<int *>(d_best_cov_b);
  a.n_best_b = n_best_b;
  a.out = reinterpret_cast<uint8_t *>(d_out);
  a.scratch = d_scratch;
  HIP_TRY(spfe::launch_covis(a, s));
  return SPFE_OK;
}
}  // namespace

extern "C" {

int spfe_covis_reset_slots_resident(spfe_handle h, const spfe_covis_graph *graph, int first_slot, int n, void *stream) {
  if (!h || !graph) return fail(SPFE_EINVAL, "null argument");
  int rc = covis_graph_check(graph);
  if (rc) return rc;
  if (first_slot < 0 || n < 1 || first_slot > graph->n_slots - n)
    return fail(SPFE_EINVAL, "slots [%d, %d + %d) not in [0, %d]", first_slot, first_slot, n, graph->n_slots);
  HIP_TRY(hipSetDevice(h->cfg.device));
  HIP_TRY(spfe::launch_covis_reset(covis_state(graph), first_slot, n, stream_of(h, stream)));
  return SPFE_OK;
}

int spfe_update_connections_resident(spfe_handle h, const spfe_covis_graph *graph, const void *d_kf_mp_of_kp, int kp_stride,
                                     const void *d_kf_flags, const void *d_mp_flags, int n_table, int cur_slot,
                                     const spfe_covis_params *prm, void *d_best_cov_a, int n_best_a, void *d_best_cov_b, int n_best_b,
                                     void *d_out, void *stream) {
  if (!h || !graph || !d_kf_mp_of_kp || !d_kf_flags || !prm || !d_out || (n_table > 0 && !d_mp_flags))
    return fail(SPFE_EINVAL, "null argument");
  int rc = cv_check(graph, kp_stride, n_table, cur_slot, prm, n_best_a, n_best_b);
  if (rc) return rc;
  if (misaligned(d_kf_mp_of_kp, 4) || misaligned(d_best_cov_a, 4) || misaligned(d_best_cov_b, 4) || misaligned(d_out, 16))
    return fail(SPFE_EINVAL, "alignment: the int32 arrays 4 bytes, d_out 16");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = reserve(h, h->lm_scratch, spfe::covis_scratch_bytes(n_table, graph->n_slots)))) return rc;
  return update_connections(graph, d_kf_mp_of_kp, kp_stride, d_kf_flags, d_mp_flags, n_table, cur_slot, prm, d_best_cov_a, n_best_a, d_best_cov_b,
                            n_best_b, d_out, h->lm_scratch.p, stream_of(h, stream));
}

int spfe_update_connections(spfe_handle h, const spfe_covis_graph *graph, const int32_t *kf_mp_of_kp, int kp_stride,
                            const uint8_t *kf_flags, const uint8_t *mp_flags, int n_table, int cur_slot, const spfe_covis_params *prm,
                            int32_t *best_cov_a, int n_best_a, int32_t *best_cov_b, int n_best_b, void *out) {
  if (!h || !graph || !kf_mp_of_kp || !kf_flags || !prm || !out || (n_table > 0 && !mp_flags)) return fail(SPFE_EINVAL, "null argument");
  int rc = cv_check(graph, kp_stride, n_table, cur_slot, prm, n_best_a, n_best_b);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t n = (size_t)graph->n_slots, out_b = SPFE_COVIS_OUT_BYTES(graph->n_slots, graph->conn_cap);
  HostStage st(h);
  const int b_r = st.in(kf_mp_of_kp, n * kp_stride * 4, n * kp_stride * 4, 16), b_f = st.in(kf_flags, n, n, 16),
            b_m = st.in(mp_flags, (size_t)n_table, (size_t)std::max(n_table, 1), 16),
            b_s = st.in(nullptr, 0, spfe::covis_scratch_bytes(n_table, graph->n_slots), 16);
  const GraphStage gs(st, graph, true);   // the state and the tables: the caller's, updated in place
  const int b_a = st.inout(best_cov_a, n * n_best_a * 4), b_b = st.inout(best_cov_b, n * n_best_b * 4);
  const int b_out = st.out(out_b);   // every byte is written
  if ((rc = st.commit())) return rc;
  const spfe_covis_graph dg = gs.device(st, graph);
  if ((rc = update_connections(&dg, st.dev<void>(b_r), kp_stride, st.dev<void>(b_f), st.dev<void>(b_m), n_table, cur_slot, prm,
                               st.dev_if_given<void>(b_a), n_best_a, st.dev_if_given<void>(b_b), n_best_b, st.dev<void>(b_out), st.dev<uint8_t>(b_s),
                               h->stream)))
    return rc;
  if ((rc = st.fetch_inouts())) return rc;
  if ((rc = st.fetch_to(out, st.dev<void>(b_out), out_b))) return rc;
  return st.sync();
}

}  // extern "C"
