// spfe_cull.hip — C ABI of keyframe culling on the device, and its host-array form, on the handle's buffers and streams:
//   the cull loop of the local mapper (local_mapper.cpp:979-1032) with KeyFrame::SetBadFlag (keyframe.cpp:911-997) on the caller's
//   resident rows, flags, observation counts, graph state and tables, and the observation counts from the rows.
// The kernels are cull.hip, the contract include/spfe_cull_math.h.  The entry points end in _resident and keep the device forms'
// contract (include/spfe.h says why); the scratch (h->ck_scratch) grows in a call larger than any before it.
#include "spfe_host.h"
using namespace spfe_host;

namespace {
bool misaligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

int rows_check(int kp_stride, int n_slots, int n_table) {
  if (n_slots < 1 || n_slots > SPFE_LOCALMAP_MAX_KEYFRAMES)
    return fail(SPFE_EINVAL, "n_slots %d not in [1, %d]", n_slots, SPFE_LOCALMAP_MAX_KEYFRAMES);
  if (kp_stride < 1 || kp_stride > SPFE_LOCALMAP_MAX_STRIDE)
    return fail(SPFE_EINVAL, "kp_stride %d not in [1, %d]", kp_stride, SPFE_LOCALMAP_MAX_STRIDE);
  if (n_table < 0 || n_table > SPFE_MP_MAX_POINTS) return fail(SPFE_EINVAL, "n_table %d not in [0, %d]", n_table, SPFE_MP_MAX_POINTS);
  return SPFE_OK;
}

int ck_check(const spfe_covis_graph *g, int kp_stride, int n_table, int cur_slot, const spfe_cull_params *prm, int n_best_a,
             int n_best_b) {
  int rc = covis_graph_check(g);
  if (rc) return rc;
  if ((rc = rows_check(kp_stride, g->n_slots, n_table))) return rc;
  if (cur_slot < 0 || cur_slot >= g->n_slots) return fail(SPFE_EINVAL, "cur_slot %d not in [0, %d)", cur_slot, g->n_slots);
  if (prm->th_obs < 1) return fail(SPFE_EINVAL, "th_obs %d < 1", prm->th_obs);
  if (prm->bad_cap < 0 || prm->bad_cap > SPFE_MP_MAX_POINTS)
    return fail(SPFE_EINVAL, "bad_cap %d not in [0, %d]", prm->bad_cap, SPFE_MP_MAX_POINTS);
  if (prm->origin_slot < -1 || prm->origin_slot >= g->n_slots)
    return fail(SPFE_EINVAL, "origin_slot %d not in [-1, %d)", prm->origin_slot, g->n_slots);
  if (n_best_a < 1 || n_best_a > SPFE_LOCALMAP_MAX_BEST || n_best_b < 1 || n_best_b > SPFE_LOCALMAP_MAX_BEST)
    return fail(SPFE_EINVAL, "n_best %d / %d not in [1, %d]", n_best_a, n_best_b, SPFE_LOCALMAP_MAX_BEST);
  return SPFE_OK;
}

spfe::CullArgs ck_args(const spfe_covis_graph *g, int kp_stride, int n_table, int cur_slot, const spfe_cull_params *prm, int n_best_a,
                       int n_best_b) {
  const spfe::CovisArgs c = covis_state(g);
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
  return a;
}
}  // namespace

extern "C" {

int spfe_count_observations_resident(spfe_handle h, const void *d_kf_mp_of_kp, int kp_stride, const void *d_kf_flags, int n_slots,
                                     void *d_mp_nobs, int n_table, void *stream) {
  if (!h || !d_kf_mp_of_kp || !d_kf_flags || (n_table > 0 && !d_mp_nobs)) return fail(SPFE_EINVAL, "null argument");
  int rc = rows_check(kp_stride, n_slots, n_table);
  if (rc) return rc;
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
  spfe::CullArgs a = ck_args(graph, kp_stride, n_table, cur_slot, prm, n_best_a, n_best_b);
  a.kf_mp_of_kp = reinterpret_cast<int *>(d_kf_mp_of_kp);
  a.kf_flags = reinterpret_cast<uint8_t *>(d_kf_flags);
  a.mp_flags = reinterpret_cast<uint8_t *>(d_mp_flags);
  a.nobs = reinterpret_cast<int *>(d_mp_nobs);
  a.best_a = reinterpret_cast<int *>(d_best_cov_a);
  a.best_b = reinterpret_cast<int *>(d_best_cov_b);
  a.out = reinterpret_cast<uint8_t *>(d_out);
  a.scratch = h->ck_scratch.p;
  HIP_TRY(spfe::launch_cull(a, stream_of(h, stream)));
  return SPFE_OK;
}

int spfe_cull_keyframes(spfe_handle h, const spfe_covis_graph *graph, int32_t *kf_mp_of_kp, int kp_stride, uint8_t *kf_flags,
                        uint8_t *mp_flags, int32_t *mp_nobs, int n_table, int cur_slot, const spfe_cull_params *prm, int32_t *best_cov_a,
                        int n_best_a, int32_t *best_cov_b, int n_best_b, void *out) {
  if (!h || !graph || !kf_mp_of_kp || !kf_flags || !prm || !out || (n_table > 0 && (!mp_flags || !mp_nobs)))
    return fail(SPFE_EINVAL, "null argument");
  int rc = ck_check(graph, kp_stride, n_table, cur_slot, prm, n_best_a, n_best_b);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t n = (size_t)graph->n_slots, row_b = n * graph->conn_cap * 4;
  const size_t out_b = SPFE_CULL_OUT_BYTES(graph->n_slots, graph->conn_cap, prm->bad_cap);
  const size_t ta_b = best_cov_a ? n * n_best_a * 4 : 0, tb_b = best_cov_b ? n * n_best_b * 4 : 0;
  HostStage st(h);
  // everything the call edits: the caller's, uploaded, updated in place and fetched whole (first_conn is not written)
  void *const host[13] = {graph->d_conn_slot, graph->d_conn_w, graph->d_conn_n, graph->d_ord_slot, graph->d_ord_w, graph->d_ord_n,
                          graph->d_parent,    best_cov_a,      best_cov_b,      kf_mp_of_kp,       kf_flags,       mp_flags,
                          mp_nobs};
  const size_t bytes[13] = {row_b, row_b, n * 4, row_b, row_b, n * 4, n * 4, ta_b, tb_b, n * kp_stride * 4, n, (size_t)n_table,
                            (size_t)n_table * 4};
  int blk[13];
  for (int i = 0; i < 13; ++i) blk[i] = st.in(host[i], bytes[i], std::max(bytes[i], (size_t)16), 16);
  const int b_s = st.in(nullptr, 0, spfe::cull_scratch_bytes(n_table, graph->n_slots, graph->conn_cap), 16);
  const int b_out = st.out(out_b);   // every byte is written
  if ((rc = st.commit())) return rc;
  spfe_covis_graph dg = *graph;
  dg.d_conn_slot = st.dev<void>(blk[0]); dg.d_conn_w = st.dev<void>(blk[1]); dg.d_conn_n = st.dev<void>(blk[2]);
  dg.d_ord_slot = st.dev<void>(blk[3]); dg.d_ord_w = st.dev<void>(blk[4]); dg.d_ord_n = st.dev<void>(blk[5]);
  dg.d_parent = st.dev<void>(blk[6]);
  spfe::CullArgs a = ck_args(&dg, kp_stride, n_table, cur_slot, prm, n_best_a, n_best_b);
  a.best_a = best_cov_a ? st.dev<int>(blk[7]) : nullptr;
  a.best_b = best_cov_b ? st.dev<int>(blk[8]) : nullptr;
  a.kf_mp_of_kp = st.dev<int>(blk[9]);
  a.kf_flags = st.dev<uint8_t>(blk[10]);
  a.mp_flags = st.dev<uint8_t>(blk[11]);
  a.nobs = st.dev<int>(blk[12]);
  a.out = st.dev<uint8_t>(b_out);
  a.scratch = st.dev<uint8_t>(b_s);
  HIP_TRY(spfe::launch_cull(a, h->stream));
  for (int i = 0; i < 13; ++i)
    if (host[i] && (rc = st.fetch_to(host[i], st.dev<uint8_t>(blk[i]), bytes[i]))) return rc;
  if ((rc = st.fetch_to(out, a.out, out_b))) return rc;
  return st.sync();
}

}  // extern "C"
