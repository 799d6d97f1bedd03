// spfe_essgraph.hip — C ABI of the loop closer's last steps on the device, and their host-array forms, on the handle's buffers
// and streams:
//   the essential graph          Optimizer::OptimizeEssentialGraph (optimizer.cpp:776-1060)
//   its start values             vScw / NonCorrectedSim3 / CorrectedSim3 as CorrectLoop forms them (loop_closer_vlad.cpp:536-571)
//   the map-point corrections    loop_closer_vlad.cpp:575-606 and optimizer.cpp:1029-1059
// The kernels are essgraph.hip, the arithmetic include/spfe_essgraph_math.h.
#include "spfe_host.h"
#include "../../include/spfe_essgraph_math.h"
using namespace spfe_host;

namespace {
int eg_check(int n, int E, int env_cap, const spfe_essgraph_params *prm) {
  if (n < 1 || n > SPFE_ESSGRAPH_MAX_KEYFRAMES) return fail(SPFE_EINVAL, "n %d not in [1, %d]", n, SPFE_ESSGRAPH_MAX_KEYFRAMES);
  if (E < 0 || E > SPFE_ESSGRAPH_MAX_EDGES) return fail(SPFE_EINVAL, "E %d not in [0, %d]", E, SPFE_ESSGRAPH_MAX_EDGES);
  if (env_cap < 0 || env_cap > SPFE_ESSGRAPH_MAX_BLOCKS) return fail(SPFE_EINVAL, "env_cap %d not in [0, %d]", env_cap, SPFE_ESSGRAPH_MAX_BLOCKS);
  if (prm->iterations < 0 || prm->iterations > 1000) return fail(SPFE_EINVAL, "iterations %d not in [0, 1000]", prm->iterations);
  if (!(prm->lambda_init >= 0.0) || !std::isfinite(prm->lambda_init)) return fail(SPFE_EINVAL, "lambda_init %g", prm->lambda_init);
  return SPFE_OK;
}
spfe::EgArgs eg_args(spfe_handle h, const void *est, const void *meas, const void *flags, int n, const void *edges, int E, int env_cap,
                     const spfe_essgraph_params *prm, void *out) {
  spfe::EgArgs a{};
  a.est = reinterpret_cast<const double *>(est); a.meas = reinterpret_cast<const double *>(meas);
  a.flags = reinterpret_cast<const uint8_t *>(flags);
  a.n = n;
  a.edges = reinterpret_cast<const int *>(edges);
  a.E = E; a.env_cap = env_cap;
  a.iterations = prm->iterations; a.fix_scale = prm->fix_scale != 0; a.lambda_init = prm->lambda_init;
  a.out = reinterpret_cast<uint8_t *>(out);
  a.scratch = h->eg_scratch.p;
  return a;
}
int sim3_check(int n, int n_conn, int cur_slot) {
  if (n < 1 || n > SPFE_ESSGRAPH_MAX_KEYFRAMES) return fail(SPFE_EINVAL, "n %d not in [1, %d]", n, SPFE_ESSGRAPH_MAX_KEYFRAMES);
  if (n_conn < 0 || n_conn > n) return fail(SPFE_EINVAL, "n_conn %d not in [0, %d]", n_conn, n);
  if (cur_slot < -1 || cur_slot >= n) return fail(SPFE_EINVAL, "cur_slot %d not in [-1, %d)", cur_slot, n);
  return SPFE_OK;
}
int correct_check(int n_kf, int m, int n_table) {
  if (m < 0 || m > SPFE_MP_MAX_POINTS) return fail(SPFE_EINVAL, "m %d not in [0, %d]", m, SPFE_MP_MAX_POINTS);
  if (n_kf < 1) return fail(SPFE_EINVAL, "n_kf %d < 1", n_kf);
  if (n_table < 0) return fail(SPFE_EINVAL, "n_table %d", n_table);
  return SPFE_OK;
}
}  // namespace

extern "C" {

int spfe_essential_graph_envelope(int n, const uint8_t *flags, const int32_t *edges, int E, int32_t *first_out, int *n_unknown,
                                  int *n_blocks) {
  if (!flags || !n_unknown || !n_blocks || (E > 0 && !edges)) return fail(SPFE_EINVAL, "null argument");
  if (n < 1 || n > SPFE_ESSGRAPH_MAX_KEYFRAMES) return fail(SPFE_EINVAL, "n %d not in [1, %d]", n, SPFE_ESSGRAPH_MAX_KEYFRAMES);
  if (E < 0 || E > SPFE_ESSGRAPH_MAX_EDGES) return fail(SPFE_EINVAL, "E %d not in [0, %d]", E, SPFE_ESSGRAPH_MAX_EDGES);
  std::vector<int> work((size_t)n), first((size_t)n);
  const long long blocks = spfe_eg_envelope(n, flags, edges, E, nullptr, first.data(), n_unknown, work.data());
  if (first_out)
    for (int u = 0; u < *n_unknown; ++u) first_out[u] = first[u];
  *n_blocks = (int)blocks;   // at most n (n + 1) / 2 < 2^31
  return (int)blocks;
}

int spfe_essgraph_lds_panel_capacity(spfe_handle h) {
  if (!h) return fail(SPFE_EINVAL, "null argument");
  return spfe::eg_lds_panel_capacity();
}

int spfe_essential_graph_sim3_device(spfe_handle h, const void *d_Tcw, const void *d_opt_block, const void *d_Tcw2, const void *d_Twc,
                                     const void *d_conn_slot, int n_conn, int cur_slot, void *d_Scw_est, void *d_Scw_meas, int n,
                                     void *stream) {
  if (!h || !d_Tcw || !d_opt_block || !d_Tcw2 || !d_Twc || !d_Scw_est || !d_Scw_meas || (n_conn > 0 && !d_conn_slot))
    return fail(SPFE_EINVAL, "null argument");
  int rc = sim3_check(n, n_conn, cur_slot);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  const double *S12 = reinterpret_cast<const double *>(reinterpret_cast<const uint8_t *>(d_opt_block) + SPFE_SIM3OPT_OFF_S12);
  HIP_TRY(spfe::launch_eg_sim3(reinterpret_cast<const float *>(d_Tcw), S12, reinterpret_cast<const float *>(d_Tcw2),
                               reinterpret_cast<const float *>(d_Twc), reinterpret_cast<const int *>(d_conn_slot), n_conn, cur_slot,
                               reinterpret_cast<double *>(d_Scw_est), reinterpret_cast<double *>(d_Scw_meas), n, stream_of(h, stream)));
  return SPFE_OK;
}

int spfe_essential_graph_sim3(const float *Tcw, const double *S12, const float *Tcw2, const float *Twc, const int32_t *conn_slot,
                              int n_conn, int cur_slot, double *Scw_est, double *Scw_meas, int n) {
  if (!Tcw || !S12 || !Tcw2 || !Twc || !Scw_est || !Scw_meas || (n_conn > 0 && !conn_slot)) return fail(SPFE_EINVAL, "null argument");
  int rc = sim3_check(n, n_conn, cur_slot);
  if (rc) return rc;
  for (int v = 0; v < n; ++v) {
    spfe_s3o_sim S;
    spfe_eg_from_pose(Tcw + 16 * (size_t)v, &S);
    spfe_eg_store_canon(&S, Scw_est + 8 * (size_t)v);
    spfe_eg_store_canon(&S, Scw_meas + 8 * (size_t)v);
  }
  for (int k = 0; k < n_conn; ++k) {
    const int v = conn_slot[k];
    if (v < 0 || v >= n) continue;
    spfe_s3o_sim P;
    spfe_eg_corrected(S12, Tcw2, Twc, Tcw + 16 * (size_t)v, v == cur_slot, &P);
    spfe_eg_store_canon(&P, Scw_est + 8 * (size_t)v);
  }
  return SPFE_OK;
}

int spfe_optimize_essential_graph_device(spfe_handle h, const void *d_Scw_est, const void *d_Scw_meas, const void *d_flags, int n,
                                         const void *d_edges, int E, int env_cap, const spfe_essgraph_params *prm, void *d_out,
                                         void *stream) {
  if (!h || !d_Scw_est || !d_Scw_meas || !d_flags || !prm || !d_out || (E > 0 && !d_edges)) return fail(SPFE_EINVAL, "null argument");
  int rc = eg_check(n, E, env_cap, prm);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = reserve(h, h->eg_scratch, spfe::eg_scratch_bytes(n, E, env_cap)))) return rc;
  HIP_TRY(spfe::launch_eg_optimize(eg_args(h, d_Scw_est, d_Scw_meas, d_flags, n, d_edges, E, env_cap, prm, d_out), stream_of(h, stream)));
  return SPFE_OK;
}

int spfe_optimize_essential_graph(spfe_handle h, const double *Scw_est, const double *Scw_meas, const uint8_t *flags, int n,
                                  const int32_t *edges, int E, int env_cap, const spfe_essgraph_params *prm, void *out) {
  if (!h || !Scw_est || !Scw_meas || !flags || !prm || !out || (E > 0 && !edges)) return fail(SPFE_EINVAL, "null argument");
  int rc = eg_check(n, E, env_cap, prm);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t out_b = SPFE_ESSGRAPH_OUT_BYTES(n), ne = (size_t)std::max(E, 1);
  HostStage st(h);
  const int b_e = st.in(Scw_est, (size_t)n * 64, (size_t)n * 64, 16), b_m = st.in(Scw_meas, (size_t)n * 64, (size_t)n * 64, 16),
            b_f = st.in(flags, (size_t)n, (size_t)n, 16), b_g = st.in(edges, (size_t)E * 12, ne * 12, 16), b_out = st.out(out_b, out);
  if ((rc = reserve(h, h->eg_scratch, spfe::eg_scratch_bytes(n, E, env_cap))) || (rc = st.commit())) return rc;
  const spfe::EgArgs a = eg_args(h, st.dev<double>(b_e), st.dev<double>(b_m), st.dev<uint8_t>(b_f), n, st.dev<int>(b_g), E, env_cap, prm,
                                 st.dev<uint8_t>(b_out));
  HIP_TRY(spfe::launch_eg_optimize(a, h->stream));
  if ((rc = st.fetch_to(out, a.out, out_b))) return rc;
  return st.sync();
}

int spfe_correct_map_points_device(spfe_handle h, const void *d_S_from, const void *d_S_to, int n_kf, const void *d_ref_slot,
                                   const void *d_point_idx, int m, void *d_xyz, const void *d_flags, int n_table, void *d_code,
                                   void *stream) {
  if (!h || !d_S_from || !d_S_to || (m > 0 && (!d_ref_slot || !d_code)) || (n_table > 0 && (!d_xyz || !d_flags)))
    return fail(SPFE_EINVAL, "null argument");
  int rc = correct_check(n_kf, m, n_table);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  HIP_TRY(spfe::launch_eg_correct(reinterpret_cast<const double *>(d_S_from), reinterpret_cast<const double *>(d_S_to), n_kf,
                                  reinterpret_cast<const int *>(d_ref_slot), reinterpret_cast<const int *>(d_point_idx), m,
                                  reinterpret_cast<float *>(d_xyz), reinterpret_cast<const uint8_t *>(d_flags), n_table,
                                  reinterpret_cast<uint8_t *>(d_code), stream_of(h, stream)));
  return SPFE_OK;
}

int spfe_correct_map_points(spfe_handle h, const double *S_from, const double *S_to, int n_kf, const int32_t *ref_slot,
                            const int32_t *point_idx, int m, float *xyz, const uint8_t *flags, int n_table, uint8_t *code) {
  if (!h || !S_from || !S_to || (m > 0 && (!ref_slot || !code)) || (n_table > 0 && (!xyz || !flags))) return fail(SPFE_EINVAL, "null argument");
  int rc = correct_check(n_kf, m, n_table);
  if (rc) return rc;
  {   // a row listed twice would be corrected twice, in no defined order
    std::vector<uint8_t> seen((size_t)n_table, 0);
    for (int i = 0; i < m; ++i) {
      const int row = point_idx ? point_idx[i] : i;
      if (row < 0 || row >= n_table) continue;
      if (seen[row]) return fail(SPFE_EINVAL, "table row %d is listed twice", row);
      seen[row] = 1;
    }
  }
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t nk = (size_t)n_kf * 64, np = (size_t)std::max(m, 1), nt = (size_t)std::max(n_table, 1);
  HostStage st(h);
  const int b_a = st.in(S_from, nk, nk, 16), b_b = st.in(S_to, nk, nk, 16), b_r = st.in(ref_slot, (size_t)m * 4, np * 4, 16),
            b_i = st.in(point_idx, (size_t)m * 4, np * 4, 16), b_x = st.in(xyz, (size_t)n_table * 12, nt * 12, 16),
            b_f = st.in(flags, (size_t)n_table, nt, 16), b_c = st.in(code, (size_t)m, np, 16);
  if ((rc = st.commit())) return rc;
  HIP_TRY(spfe::launch_eg_correct(st.dev<double>(b_a), st.dev<double>(b_b), n_kf, st.dev<int>(b_r), point_idx ? st.dev<int>(b_i) : nullptr, m,
                                  st.dev<float>(b_x), st.dev<uint8_t>(b_f), n_table, st.dev<uint8_t>(b_c), h->stream));
  if ((rc = st.fetch_to(xyz, st.dev<float>(b_x), (size_t)n_table * 12)) || (rc = st.fetch_to(code, st.dev<uint8_t>(b_c), (size_t)m))) return rc;
  return st.sync();
}

}  // extern "C"
