// spfe_covis.hip — C ABI of the covisibility graph on the device, and its host-array form, on the handle's buffers and streams:
//   KeyFrame::UpdateConnections (keyframe.cpp:757-849) with AddConnection / UpdateBestCovisibles (:577-612) on the caller's resident
//   keyframe rows and resident graph state, and the preset of a range of slots.
// The kernels are covis.hip (and localmap.hip's count), the contract include/spfe_covis_math.h.  The entry points end in _resident
// and keep the device forms' contract (include/spfe.h says why); the scratch is the local map's (h->lm_scratch: the two calls
// follow each other on one stream) and grows in a call larger than any before it.
#include "spfe_host.h"
using namespace spfe_host;

namespace {
bool misaligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

}  // namespace

int spfe_host::covis_graph_check(const spfe_covis_graph *g) {
  if (!g->d_conn_slot || !g->d_conn_w || !g->d_conn_n || !g->d_ord_slot || !g->d_ord_w || !g->d_ord_n || !g->d_parent || !g->d_first_conn)
    return fail(SPFE_EINVAL, "null argument");
  if (g->n_slots < 1 || g->n_slots > SPFE_LOCALMAP_MAX_KEYFRAMES)
    return fail(SPFE_EINVAL, "n_slots %d not in [1, %d]", g->n_slots, SPFE_LOCALMAP_MAX_KEYFRAMES);
  if (g->conn_cap < 1 || g->conn_cap > SPFE_COVIS_MAX_CONN)
    return fail(SPFE_EINVAL, "conn_cap %d not in [1, %d]", g->conn_cap, SPFE_COVIS_MAX_CONN);
  if (misaligned(g->d_conn_slot, 4) || misaligned(g->d_conn_w, 4) || misaligned(g->d_conn_n, 4) || misaligned(g->d_ord_slot, 4) ||
      misaligned(g->d_ord_w, 4) || misaligned(g->d_ord_n, 4) || misaligned(g->d_parent, 4))
    return fail(SPFE_EINVAL, "alignment: the int32 arrays 4 bytes");
  return SPFE_OK;
}

namespace {
int cv_check(const spfe_covis_graph *g, int kp_stride, int n_table, int cur_slot, const spfe_covis_params *prm, int n_best_a,
             int n_best_b) {
  int rc = covis_graph_check(g);
  if (rc) return rc;
  if (kp_stride < 1 || kp_stride > SPFE_LOCALMAP_MAX_STRIDE)
    return fail(SPFE_EINVAL, "kp_stride %d not in [1, %d]", kp_stride, SPFE_LOCALMAP_MAX_STRIDE);
  if (n_table < 0 || n_table > SPFE_MP_MAX_POINTS) return fail(SPFE_EINVAL, "n_table %d not in [0, %d]", n_table, SPFE_MP_MAX_POINTS);
  if (cur_slot < 0 || cur_slot >= g->n_slots) return fail(SPFE_EINVAL, "cur_slot %d not in [0, %d)", cur_slot, g->n_slots);
  if (prm->th < 1) return fail(SPFE_EINVAL, "th %d < 1", prm->th);
  if (prm->origin_slot < -1 || prm->origin_slot >= g->n_slots)
    return fail(SPFE_EINVAL, "origin_slot %d not in [-1, %d)", prm->origin_slot, g->n_slots);
  if (n_best_a < 1 || n_best_a > SPFE_LOCALMAP_MAX_BEST || n_best_b < 1 || n_best_b > SPFE_LOCALMAP_MAX_BEST)
    return fail(SPFE_EINVAL, "n_best %d / %d not in [1, %d]", n_best_a, n_best_b, SPFE_LOCALMAP_MAX_BEST);
  return SPFE_OK;
}

}  // namespace

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
  spfe::CovisArgs a = covis_state(graph);
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
  a.scratch = h->lm_scratch.p;
  HIP_TRY(spfe::launch_covis(a, stream_of(h, stream)));
  return SPFE_OK;
}

int spfe_update_connections(spfe_handle h, const spfe_covis_graph *graph, const int32_t *kf_mp_of_kp, int kp_stride,
                            const uint8_t *kf_flags, const uint8_t *mp_flags, int n_table, int cur_slot, const spfe_covis_params *prm,
                            int32_t *best_cov_a, int n_best_a, int32_t *best_cov_b, int n_best_b, void *out) {
  if (!h || !graph || !kf_mp_of_kp || !kf_flags || !prm || !out || (n_table > 0 && !mp_flags)) return fail(SPFE_EINVAL, "null argument");
  int rc = cv_check(graph, kp_stride, n_table, cur_slot, prm, n_best_a, n_best_b);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t n = (size_t)graph->n_slots, row_b = n * graph->conn_cap * 4, out_b = SPFE_COVIS_OUT_BYTES(graph->n_slots, graph->conn_cap);
  const size_t ta_b = best_cov_a ? n * n_best_a * 4 : 0, tb_b = best_cov_b ? n * n_best_b * 4 : 0;
  HostStage st(h);
  const int b_r = st.in(kf_mp_of_kp, n * kp_stride * 4, n * kp_stride * 4, 16), b_f = st.in(kf_flags, n, n, 16),
            b_m = st.in(mp_flags, (size_t)n_table, (size_t)std::max(n_table, 1), 16),
            b_s = st.in(nullptr, 0, spfe::covis_scratch_bytes(n_table, graph->n_slots), 16);
  // the state and the tables: the caller's, uploaded, updated in place and fetched whole
  void *const host[10] = {graph->d_conn_slot, graph->d_conn_w, graph->d_conn_n, graph->d_ord_slot, graph->d_ord_w,
                          graph->d_ord_n,     graph->d_parent, graph->d_first_conn, best_cov_a,     best_cov_b};
  const size_t bytes[10] = {row_b, row_b, n * 4, row_b, row_b, n * 4, n * 4, n, ta_b, tb_b};
  int blk[10];
  for (int i = 0; i < 10; ++i) blk[i] = st.in(host[i], bytes[i], std::max(bytes[i], (size_t)16), 16);
  const int b_out = st.out(out_b);   // every byte is written
  if ((rc = st.commit())) return rc;
  spfe_covis_graph dg = *graph;
  dg.d_conn_slot = st.dev<void>(blk[0]); dg.d_conn_w = st.dev<void>(blk[1]); dg.d_conn_n = st.dev<void>(blk[2]);
  dg.d_ord_slot = st.dev<void>(blk[3]); dg.d_ord_w = st.dev<void>(blk[4]); dg.d_ord_n = st.dev<void>(blk[5]);
  dg.d_parent = st.dev<void>(blk[6]); dg.d_first_conn = st.dev<void>(blk[7]);
  spfe::CovisArgs a = covis_state(&dg);
  a.kf_mp_of_kp = st.dev<int>(b_r);
  a.kp_stride = kp_stride;
  a.kf_flags = st.dev<uint8_t>(b_f);
  a.mp_flags = st.dev<uint8_t>(b_m);
  a.n_table = n_table;
  a.cur_slot = cur_slot;
  a.th = prm->th; a.origin_slot = prm->origin_slot;
  a.best_a = best_cov_a ? st.dev<int>(blk[8]) : nullptr;
  a.n_best_a = n_best_a;
  a.best_b = best_cov_b ? st.dev<int>(blk[9]) : nullptr;
  a.n_best_b = n_best_b;
  a.out = st.dev<uint8_t>(b_out);
  a.scratch = st.dev<uint8_t>(b_s);
  HIP_TRY(spfe::launch_covis(a, h->stream));
  for (int i = 0; i < 10; ++i)
    if (host[i] && (rc = st.fetch_to(host[i], st.dev<uint8_t>(blk[i]), bytes[i]))) return rc;
  if ((rc = st.fetch_to(out, a.out, out_b))) return rc;
  return st.sync();
}

}  // extern "C"
