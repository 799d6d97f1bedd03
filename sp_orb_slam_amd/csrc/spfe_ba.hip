// spfe_ba.hip — C ABI of bundle adjustment on keyframe records resident in HBM, and its host-array form, on the handle's
// buffers and streams:
//   the mapper's local bundle adjustment   Optimizer::LocalBundleAdjustment (optimizer.cpp:445-774) behind SearchInNeighbors
//                                          (local_mapper.cpp:150-186)
//   the initial map's bundle adjustment    Optimizer::BundleAdjustment (optimizer.cpp:51-229) as MonoTracker::CreateInitialMap
//                                          calls it (mono_tracker.cpp:170)
// The kernel is ba.hip, the arithmetic include/spfe_ba_math.h.
#include "spfe_host.h"
using namespace spfe_host;

namespace {
int ba_check(int n_kf, int n, int E, const spfe_ba_params *prm) {
  if (n_kf < 1 || n_kf > SPFE_BA_MAX_KEYFRAMES) return fail(SPFE_EINVAL, "n_kf %d not in [1, %d]", n_kf, SPFE_BA_MAX_KEYFRAMES);
  if (n < 0 || n > SPFE_BA_MAX_POINTS) return fail(SPFE_EINVAL, "n_points %d not in [0, %d]", n, SPFE_BA_MAX_POINTS);
  if (E < 0 || E > SPFE_BA_MAX_EDGES) return fail(SPFE_EINVAL, "n_edges %d not in [0, %d]", E, SPFE_BA_MAX_EDGES);
  if (prm->schedule != SPFE_BA_LOCAL && prm->schedule != SPFE_BA_FULL) return fail(SPFE_EINVAL, "schedule %d", prm->schedule);
  for (int r = 0; r < (prm->schedule == SPFE_BA_LOCAL ? 2 : 1); ++r)   // FULL does not read the second entry
    if (prm->iterations[r] < 0 || prm->iterations[r] > 1000) return fail(SPFE_EINVAL, "iterations[%d] = %d not in [0, 1000]", r, prm->iterations[r]);
  return SPFE_OK;
}
void ba_fill(spfe::BaArgs &a, const spfe_ba_params *prm, int n_kf, int n, int E) {
  a.fx = prm->fx; a.fy = prm->fy; a.cx = prm->cx; a.cy = prm->cy;
  a.schedule = prm->schedule; a.it0 = prm->iterations[0]; a.it1 = prm->iterations[1]; a.robust = prm->robust;
  a.inv_sigma2_full = prm->inv_sigma2;
  a.n_kf = n_kf; a.n = n; a.E = E;
}
}  // namespace

extern "C" {

int spfe_ba_lds_free_capacity(spfe_handle h) {
  if (!h) return fail(SPFE_EINVAL, "null argument");
  return spfe::ba_lds_free_capacity();
}

int spfe_local_ba_records_device(spfe_handle h, const void *const *d_records, int n_kf, const void *d_edges, int E,
                                 const void *d_Tcw, const void *d_fixed, const void *d_xyz, int n, const spfe_ba_params *prm,
                                 const void *d_stop, void *d_out, void *stream) {
  if (!h || !d_records || !d_Tcw || !d_fixed || !prm || !d_out || (E > 0 && !d_edges) || (n > 0 && !d_xyz))
    return fail(SPFE_EINVAL, "null argument");
  int rc = ba_check(n_kf, n, E, prm);
  if (rc) return rc;
  for (int k = 0; k < n_kf; ++k)
    if (!d_records[k]) return fail(SPFE_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = reserve(h, h->ba_scratch, spfe::ba_scratch_bytes(n, E)))) return rc;
  spfe::BaArgs a{};
  ba_fill(a, prm, n_kf, n, E);
  for (int k = 0; k < n_kf; ++k) a.base[k] = reinterpret_cast<const uint8_t *>(d_records[k]);
  a.off_xy = (long)h->rl.off_xy; a.off_cinv = (long)h->rl.off_cinv; a.off_hdr = (long)h->rl.off_hdr;
  a.kmax = h->kmax;
  a.edges = reinterpret_cast<const int *>(d_edges);
  a.Tcw = reinterpret_cast<const float *>(d_Tcw); a.fixed = reinterpret_cast<const uint8_t *>(d_fixed);
  a.xyz = reinterpret_cast<const float *>(d_xyz);
  a.stop = reinterpret_cast<const int *>(d_stop);
  a.out = reinterpret_cast<uint8_t *>(d_out);
  a.scratch = h->ba_scratch.p;
  HIP_TRY(spfe::launch_ba(a, stream_of(h, stream)));
  return SPFE_OK;
}

int spfe_bundle_adjust(spfe_handle h, const int32_t *edges, const float *obs_xy, const float *inv_sigma2, int E, const float *Tcw,
                       const uint8_t *fixed, int n_kf, const float *xyz, int n, const spfe_ba_params *prm, const int32_t *stop,
                       void *out) {
  if (!h || !Tcw || !fixed || !prm || !out || (n > 0 && !xyz)) return fail(SPFE_EINVAL, "null argument");
  int rc = ba_check(n_kf, n, E, prm);
  if (rc) return rc;
  if (E > 0 && (!edges || !obs_xy || (prm->schedule == SPFE_BA_LOCAL && !inv_sigma2))) return fail(SPFE_EINVAL, "null argument");
  int n_free = 0;
  for (int k = 0; k < n_kf; ++k) n_free += fixed[k] == 0;
  if (n_free > SPFE_BA_MAX_FREE) return fail(SPFE_EINVAL, "%d free keyframes, at most %d", n_free, SPFE_BA_MAX_FREE);
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t out_b = SPFE_BA_OUT_BYTES(n_kf, n, E);
  const size_t ne = (size_t)std::max(E, 1), np = (size_t)std::max(n, 1);
  const bool with_w = inv_sigma2 && prm->schedule == SPFE_BA_LOCAL;
  HostStage st(h);
  const int b_e = st.in(edges, (size_t)E * 12, ne * 12, 16), b_xy = st.in(obs_xy, (size_t)E * 8, ne * 8, 16),
            b_w = st.in(with_w ? inv_sigma2 : nullptr, (size_t)E * 8, ne * 8, 16), b_T = st.in(Tcw, (size_t)n_kf * 64, (size_t)n_kf * 64, 16),
            b_f = st.in(fixed, (size_t)n_kf, (size_t)n_kf, 16), b_p = st.in(xyz, (size_t)n * 12, np * 12, 16),
            b_s = st.value<int32_t>(stop ? *stop : 0, 16), b_out = st.out(out_b, out);
  if ((rc = reserve(h, h->ba_scratch, spfe::ba_scratch_bytes(n, E))) || (rc = st.commit())) return rc;
  spfe::BaArgs a{};
  ba_fill(a, prm, n_kf, n, E);
  a.off_hdr = -1;
  a.edges = st.dev<int>(b_e);
  a.obs_xy = st.dev<float>(b_xy);
  a.inv_sigma2 = st.dev<float>(b_w);
  a.Tcw = st.dev<float>(b_T); a.fixed = st.dev<uint8_t>(b_f);
  a.xyz = st.dev<float>(b_p);
  a.stop = st.dev<int>(b_s);
  a.out = st.dev<uint8_t>(b_out);
  a.scratch = h->ba_scratch.p;
  HIP_TRY(spfe::launch_ba(a, h->stream));
  if ((rc = st.fetch_to(out, a.out, out_b))) return rc;
  return st.sync();
}

}  // extern "C"
