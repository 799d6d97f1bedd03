// spfe_loopdet.hip — C ABI of the loop detection, and its host-array form, on the handle's buffers and streams:
//   LoopClosingVLAD::detectLoopCandidates (loop_closer_vlad.cpp:42-118) and the minimum score of detectLoopVLAD (:150-165) for one
//   query keyframe on the caller's resident table of NetVLAD descriptors.
// The kernels are loopdet.hip, the arithmetic include/spfe_loopdet_math.h.
#include "spfe_host.h"
using namespace spfe_host;

namespace {
int loopdet_check(int dim, int n_slots, int cur_slot, int n_conn, int n_cov) {
  if (n_slots < 1 || n_slots > SPFE_LOOPDET_MAX_KEYFRAMES)
    return fail(SPFE_EINVAL, "n_slots %d not in [1, %d]", n_slots, SPFE_LOOPDET_MAX_KEYFRAMES);
  if (dim < 4 || dim > SPFE_GLOBAL_DESC_DIM || dim % 4)
    return fail(SPFE_EINVAL, "dim %d: a multiple of 4 in [4, %d]", dim, SPFE_GLOBAL_DESC_DIM);
  if (cur_slot < 0 || cur_slot >= n_slots) return fail(SPFE_EINVAL, "cur_slot %d not in [0, %d)", cur_slot, n_slots);
  if (n_conn < 0 || n_conn > n_slots) return fail(SPFE_EINVAL, "n_conn %d not in [0, %d]", n_conn, n_slots);
  if (n_cov < 0 || n_cov > n_slots) return fail(SPFE_EINVAL, "n_cov %d not in [0, %d]", n_cov, n_slots);
  return SPFE_OK;
}
}  // namespace

extern "C" {

int spfe_detect_loop_candidates_device(spfe_handle h, const void *d_gdesc, int dim, const void *d_kf_flags, const void *d_in_db,
                                       const void *d_best_cov, int n_slots, int cur_slot, const void *d_connected, int n_conn,
                                       const void *d_covisible, int n_cov, const spfe_loopdet_params *prm, void *d_out, void *stream) {
  if (!h || !d_gdesc || !d_kf_flags || !d_in_db || !d_best_cov || !prm || !d_out || (n_conn > 0 && !d_connected) ||
      (n_cov > 0 && !d_covisible))
    return fail(SPFE_EINVAL, "null argument");
  int rc = loopdet_check(dim, n_slots, cur_slot, n_conn, n_cov);
  if (rc) return rc;
  if ((reinterpret_cast<uintptr_t>(d_gdesc) & 15) || (reinterpret_cast<uintptr_t>(d_out) & 15) ||
      (reinterpret_cast<uintptr_t>(d_best_cov) & 3) || (reinterpret_cast<uintptr_t>(d_connected) & 3) ||
      (reinterpret_cast<uintptr_t>(d_covisible) & 3))
    return fail(SPFE_EINVAL, "alignment: d_gdesc and d_out 16 bytes, d_best_cov and the lists 4");
  HIP_TRY(hipSetDevice(h->cfg.device));
  spfe::LoopdetArgs a{};
  a.gdesc = reinterpret_cast<const float *>(d_gdesc);
  a.dim = dim;
  a.kf_flags = reinterpret_cast<const uint8_t *>(d_kf_flags);
  a.in_db = reinterpret_cast<const uint8_t *>(d_in_db);
  a.best_cov = reinterpret_cast<const int *>(d_best_cov);
  a.n_slots = n_slots; a.cur_slot = cur_slot;
  a.connected = reinterpret_cast<const int *>(d_connected); a.covisible = reinterpret_cast<const int *>(d_covisible);
  a.n_conn = n_conn; a.n_cov = n_cov;
  a.min_score_init = prm->min_score_init; a.min_score_floor = prm->min_score_floor; a.retain_ratio = prm->retain_ratio;
  a.out = reinterpret_cast<uint8_t *>(d_out);
  HIP_TRY(spfe::launch_loopdet(a, stream_of(h, stream)));
  return SPFE_OK;
}

int spfe_detect_loop_candidates(spfe_handle h, const float *gdesc, int dim, const uint8_t *kf_flags, const uint8_t *in_db,
                                const int32_t *best_cov, int n_slots, int cur_slot, const int32_t *connected, int n_conn,
                                const int32_t *covisible, int n_cov, const spfe_loopdet_params *prm, void *out) {
  if (!h || !gdesc || !kf_flags || !in_db || !best_cov || !prm || !out || (n_conn > 0 && !connected) || (n_cov > 0 && !covisible))
    return fail(SPFE_EINVAL, "null argument");
  int rc = loopdet_check(dim, n_slots, cur_slot, n_conn, n_cov);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t n = (size_t)n_slots, out_b = SPFE_LOOPDET_OUT_BYTES(n_slots);
  HostStage st(h);
  const int b_g = st.in(gdesc, n * dim * 4, n * dim * 4, 16), b_f = st.in(kf_flags, n, n, 16), b_d = st.in(in_db, n, n, 16),
            b_c = st.in(best_cov, n * SPFE_LOOPDET_NEIGH * 4, n * SPFE_LOOPDET_NEIGH * 4, 16),
            b_l = st.in(connected, (size_t)n_conn * 4, (size_t)std::max(n_conn, 1) * 4, 16),
            b_v = st.in(covisible, (size_t)n_cov * 4, (size_t)std::max(n_cov, 1) * 4, 16),
            // the block starts as the caller's: what is not written keeps its bytes
            b_out = st.out(out_b, out);
  if ((rc = st.commit())) return rc;
  spfe::LoopdetArgs a{};
  a.gdesc = st.dev<float>(b_g);
  a.dim = dim;
  a.kf_flags = st.dev<uint8_t>(b_f); a.in_db = st.dev<uint8_t>(b_d);
  a.best_cov = st.dev<int>(b_c);
  a.n_slots = n_slots; a.cur_slot = cur_slot;
  a.connected = st.dev<int>(b_l); a.covisible = st.dev<int>(b_v);
  a.n_conn = n_conn; a.n_cov = n_cov;
  a.min_score_init = prm->min_score_init; a.min_score_floor = prm->min_score_floor; a.retain_ratio = prm->retain_ratio;
  a.out = st.dev<uint8_t>(b_out);
  HIP_TRY(spfe::launch_loopdet(a, h->stream));
  if ((rc = st.fetch_to(out, a.out, out_b))) return rc;
  return st.sync();
}

}  // extern "C"
