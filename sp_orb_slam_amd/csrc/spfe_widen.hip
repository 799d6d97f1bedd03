// spfe_widen.hip — C ABI of the rows SURVEY.md §8f widens into that work frame to frame, on the handle's buffers and streams:
// input staging (data_loader.cc:485-521), descriptor matching (sp_matcher.cpp:1636-1674) and the patch-wise association
// (tracker_dust.cpp:113-172).  The tracker's stages on resident records are spfe_track.hip.
#include "spfe_host.h"
using namespace spfe_host;

namespace spfe_host {
constexpr int kPatchMax = 4096;
int patch_check(int kcap) {
  if (spfe::patch_resolve_lds_total(kcap) > 160 * 1024)
    return fail(SPFE_EINVAL, "%d keypoints are too many for the claim stage's LDS (at most %d)", kcap, SPFE_PATCH_MAX_KEYPOINTS);
  return SPFE_OK;
}
int patch_scratch(spfe_handle h) {
  if (h->p_cdist) return SPFE_OK;
  int rc = dev_alloc(h, &h->p_cidx, (size_t)kPatchMax * 4);
  return rc ? rc : dev_alloc(h, &h->p_cdist, (size_t)kPatchMax * 4);
}
spfe::PatchArgs patch_args(spfe_handle h, const RecordView &rec, const void *d_mp_desc, const void *d_mp_uv, int n_points) {
  spfe::PatchArgs a{};
  a.mp_desc = reinterpret_cast<const float *>(d_mp_desc);
  a.mp_uv = reinterpret_cast<const float *>(d_mp_uv);
  a.n_points = n_points;
  a.occ = rec.occ();
  a.hc = h->hc; a.wc = h->wc;
  a.kp_desc = rec.desc();
  a.kp_desc_bf16 = rec.desc_bf16();
  a.k_ptr = rec.hdr();
  a.k_imm = 0;
  return a;
}
int match_scratch(spfe_handle h, int pairs, int cap) {
  if (pairs <= h->m_pairs && cap <= h->m_cap) return SPFE_OK;
  pairs = std::max(pairs, h->m_pairs);
  cap = std::max(cap, h->m_cap);
  h->m_pairs = h->m_cap = 0;
  int rc;
  if ((rc = reserve(h, h->m_best_t, (size_t)pairs * cap * 8)) || (rc = reserve(h, h->m_best_q, (size_t)pairs * cap * 8))) return rc;
  h->m_pairs = pairs;
  h->m_cap = cap;
  return SPFE_OK;
}
spfe::MatchSide record_side(spfe_handle h, const void *d_records) {
  spfe::MatchSide m{reinterpret_cast<const uint8_t *>(d_records), h->rl.bytes, h->rl.off_hdr, h->rl.off_desc, h->kmax};
  m.desc_bf16 = h->rl.desc_bf16;   // (records made with SPFE_FLAG_DESC_BF16: bf16 rows, widened on load)
  return m;
}
}  // namespace spfe_host

namespace {
int enqueue_stage(spfe_handle h, const uint8_t *d_src, int n, uint8_t *d_gray, hipStream_t s) {
  spfe::StageParams p{};
  p.src = d_src;
  p.src_stride = h->st.src_width * h->st.channels;
  p.src_frame_bytes = (size_t)h->st.src_height * p.src_stride;
  p.src_h = h->st.src_height;
  p.src_w = h->st.src_width;
  p.map_x = h->d_map_x;
  p.map_y = h->d_map_y;
  p.rgb = h->st.rgb;
  p.gray = d_gray;
  p.H = h->H;
  p.W = h->W;
  HIP_TRY(spfe::launch_stage_input(p, h->st.channels, n, s));
  return SPFE_OK;
}

constexpr size_t kMatchHdr = 16;  // staging block of the host API: int32 count, pad, then rows
constexpr int kMatchNothing = 1;  // match_stage: a side is empty, the outputs are final

// What spfe_match (k = 1) and spfe_match_knn2 (k = 2) do up to their launch: the argument checks, train_idx / distance [n_query][k]
// preset to "unmatched", staging and scratch for max(n_query, n_train, kmax) rows, and the two blocks (count header, rows)
// uploaded through the caller's `st`.
int match_stage(spfe_handle h, HostStage &st, const float *query, int n_query, const float *train, int n_train, int k,
                int32_t *train_idx, float *distance, spfe::MatchSide *q, spfe::MatchSide *t) {
  if (!h || !train_idx || !distance) return fail(SPFE_EINVAL, "null argument");
  if (n_query < 0 || n_train < 0) return fail(SPFE_EINVAL, "negative descriptor count");
  if ((n_query && !query) || (n_train && !train)) return fail(SPFE_EINVAL, "null descriptor array");
  for (int i = 0; i < k * n_query; ++i) { train_idx[i] = -1; distance[i] = FLT_MAX; }
  if (n_query == 0 || n_train == 0) return kMatchNothing;
  HIP_TRY(hipSetDevice(h->cfg.device));
  const int rows = std::max(std::max(n_query, n_train), h->kmax);
  int rc;
  if ((rc = reserve(h, h->m_out, (size_t)rows * 8)) || (k == 2 && (rc = reserve(h, h->m_out2, (size_t)rows * 16))) ||
      (rc = match_scratch(h, 1, rows)))
    return rc;
  struct Hdr { int32_t n, pad[3]; };
  static_assert(sizeof(Hdr) == kMatchHdr, "the rows follow the header");
  const int b_q = st.value(Hdr{n_query, {}}, 256);
  st.in(query, (size_t)n_query * 1024, (size_t)rows * 1024, 16);
  const int b_t = st.value(Hdr{n_train, {}}, 256);
  st.in(train, (size_t)n_train * 1024, (size_t)rows * 1024, 16);
  if ((rc = st.commit())) return rc;
  *q = spfe::MatchSide{st.dev<uint8_t>(b_q), 0, 0, kMatchHdr, n_query};
  *t = spfe::MatchSide{st.dev<uint8_t>(b_t), 0, 0, kMatchHdr, n_train};
  return SPFE_OK;
}
}  // namespace

extern "C" {

// ---- input staging ------------------------------------------------------
int spfe_set_staging(spfe_handle h, const spfe_staging *st) {
  if (!h || !st) return fail(SPFE_EINVAL, "null argument");
  if (st->channels != 1 && st->channels != 3 && st->channels != 4)
    return fail(SPFE_EINVAL, "staging: %d channels unsupported (1, 3, 4)", st->channels);
  if (st->src_height < h->H || st->src_width < h->W)
    return fail(SPFE_EINVAL, "staging: source %dx%d smaller than the extractor's %dx%d (system.cpp:160 crop)",
                st->src_width, st->src_height, h->W, h->H);
  if (st->src_height > 32767 || st->src_width > 32767) return fail(SPFE_EINVAL, "staging: source too large");
  if ((st->map_x == nullptr) != (st->map_y == nullptr)) return fail(SPFE_EINVAL, "staging: one map is null");
  HIP_TRY(hipSetDevice(h->cfg.device));
  HIP_TRY(hipDeviceSynchronize());
  for (void **p : {(void **)&h->d_map_x, (void **)&h->d_map_y, (void **)&h->d_raw})
    if (*p) { (void)hipFree(*p); *p = nullptr; }
  if (h->h_raw) { (void)hipHostFree(h->h_raw); h->h_raw = nullptr; }
  h->st_set = false;
  const size_t npx = (size_t)st->src_height * st->src_width;
  if (st->map_x) {
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&h->d_map_x), npx * 4));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&h->d_map_y), npx * 4));
    HIP_TRY(hipMemcpy(h->d_map_x, st->map_x, npx * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_map_y, st->map_y, npx * 4, hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&h->d_raw), (size_t)h->B * npx * st->channels));
  HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&h->h_raw), (size_t)h->B * npx * st->channels,
                        hipHostMallocDefault));
  h->st = *st;
  h->st.map_x = h->st.map_y = nullptr;  // the caller's arrays are not kept
  h->st_set = true;
  return SPFE_OK;
}

int spfe_stage_batch_device(spfe_handle h, const void *d_src, int n, void *d_gray, void *stream) {
  if (!h || !d_gray) return fail(SPFE_EINVAL, "null argument");
  if (!h->st_set) return fail(SPFE_EINVAL, "spfe_set_staging has not been called");
  if (!d_src) return fail(SPFE_EEMPTY, "input image is empty");
  if (n < 1 || n > h->B) return fail(SPFE_EINVAL, "batch %d not in [1, %d]", n, h->B);
  HIP_TRY(hipSetDevice(h->cfg.device));
  return enqueue_stage(h, reinterpret_cast<const uint8_t *>(d_src), n, reinterpret_cast<uint8_t *>(d_gray), stream_of(h, stream));
}

int spfe_extract_batch_staged(spfe_handle h, const uint8_t *const *srcs, int stride, int n, spfe_result *outs) {
  if (!h || !outs) return fail(SPFE_EINVAL, "null argument");
  if (!h->st_set) return fail(SPFE_EINVAL, "spfe_set_staging has not been called");
  if (!srcs) return fail(SPFE_EEMPTY, "input image is empty");
  if (n < 1 || n > h->B) return fail(SPFE_EINVAL, "batch %d not in [1, %d]", n, h->B);
  const int row = h->st.src_width * h->st.channels;
  if (stride < row) return fail(SPFE_EINVAL, "stride %d smaller than a source row (%d bytes)", stride, row);
  const size_t frame = (size_t)h->st.src_height * row;
  for (int i = 0; i < n; ++i) {
    if (!srcs[i]) return fail(SPFE_EEMPTY, "input image is empty");  // sp_extractor.cpp:364-365
    for (int y = 0; y < h->st.src_height; ++y)
      memcpy(h->h_raw + i * frame + (size_t)y * row, srcs[i] + (size_t)y * stride, row);
  }
  HIP_TRY(hipSetDevice(h->cfg.device));
  hipStream_t s = h->stream;
  HIP_TRY(hipMemcpyAsync(h->d_raw, h->h_raw, n * frame, hipMemcpyHostToDevice, s));
  int rc = enqueue_stage(h, h->d_raw, n, h->d_img, s);
  if (rc) return rc;
  rc = enqueue(h, h->d_img, n, h->d_records, s);
  if (rc) return rc;
  return finish_host(h, n, outs);
}

int spfe_extract_staged(spfe_handle h, const uint8_t *src, int stride, spfe_result *out) {
  if (!src) return fail(SPFE_EEMPTY, "input image is empty");
  const uint8_t *one[1] = {src};
  return spfe_extract_batch_staged(h, one, stride, 1, out);
}

// ---- patch-wise association (tracker_dust.cpp:113-172) -------------------------------------------
int spfe_match_patches_record_device(spfe_handle h, const void *d_mp_desc, const void *d_mp_uv, int n_points,
                                     const void *d_record, float max_dist, void *d_kp_idx, void *stream) {
  if (!h || !d_record || !d_kp_idx) return fail(SPFE_EINVAL, "null argument");
  if (n_points < 0 || n_points > kPatchMax) return fail(SPFE_EINVAL, "n_points %d not in [0, %d]", n_points, kPatchMax);
  int rc = patch_check(h->kmax);
  if (rc) return rc;
  if (n_points == 0) return SPFE_OK;
  if (!d_mp_desc || !d_mp_uv) return fail(SPFE_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = patch_scratch(h))) return rc;
  const spfe::PatchArgs a = patch_args(h, RecordView(h, d_record), d_mp_desc, d_mp_uv, n_points);
  HIP_TRY(spfe::launch_match_patches(a, h->kmax, max_dist, h->p_cidx, h->p_cdist, reinterpret_cast<int32_t *>(d_kp_idx),
                                     stream_of(h, stream)));
  return SPFE_OK;
}

int spfe_match_patches(spfe_handle h, const float *mp_desc, const float *mp_uv, int n_points,
                       const int16_t *occ_grid, const float *kp_desc, int n_keypoints, float max_dist,
                       int32_t *kp_idx) {
  if (!h || !kp_idx) return fail(SPFE_EINVAL, "null argument");
  if (n_points < 0 || n_points > kPatchMax) return fail(SPFE_EINVAL, "n_points %d not in [0, %d]", n_points, kPatchMax);
  if (n_keypoints < 0 || n_keypoints > 32767) return fail(SPFE_EINVAL, "n_keypoints %d out of range", n_keypoints);
  int rc = patch_check(n_keypoints);   // before anything is written or launched
  if (rc) return rc;
  for (int i = 0; i < n_points; ++i) kp_idx[i] = -1;
  if (n_points == 0 || n_keypoints == 0) return SPFE_OK;
  if (!mp_desc || !mp_uv || !occ_grid || !kp_desc) return fail(SPFE_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if ((rc = patch_scratch(h))) return rc;
  const size_t cells = (size_t)h->hc * h->wc;
  const size_t mp_b = (size_t)n_points * 1024, uv_b = (size_t)n_points * 8, kp_b = (size_t)n_keypoints * 1024;
  HostStage st(h);
  const int b_mp = st.in(mp_desc, mp_b, mp_b, 16), b_uv = st.in(mp_uv, uv_b, uv_b, 4), b_occ = st.in(occ_grid, cells * 2, cells * 2, 16),
            b_kp = st.in(kp_desc, kp_b, kp_b, 16), b_out = st.out((size_t)n_points * 4, nullptr, 4);
  if ((rc = st.commit())) return rc;
  spfe::PatchArgs a{};
  a.mp_desc = st.dev<float>(b_mp);
  a.mp_uv = st.dev<float>(b_uv);
  a.n_points = n_points;
  a.occ = st.dev<int16_t>(b_occ);
  a.hc = h->hc; a.wc = h->wc;
  a.kp_desc = st.dev<float>(b_kp);
  a.k_ptr = nullptr;
  a.k_imm = n_keypoints;
  HIP_TRY(spfe::launch_match_patches(a, n_keypoints, max_dist, h->p_cidx, h->p_cdist, st.dev<int32_t>(b_out), h->stream));
  if ((rc = st.fetch_to(kp_idx, st.dev<int32_t>(b_out), (size_t)n_points * 4))) return rc;
  return st.sync();
}

// ---- descriptor matching ------------------------------------------------
size_t spfe_match_out_bytes(spfe_handle h) { return h ? (size_t)h->kmax * 8 : 0; }

int spfe_match_records_device(spfe_handle h, const void *d_query_records, const void *d_train_records, int n_pairs,
                              int cross_check, void *d_out, void *stream) {
  if (!h || !d_query_records || !d_train_records || !d_out) return fail(SPFE_EINVAL, "null argument");
  if (n_pairs < 1) return fail(SPFE_EINVAL, "n_pairs %d must be >= 1", n_pairs);
  HIP_TRY(hipSetDevice(h->cfg.device));
  int rc = match_scratch(h, n_pairs, h->kmax);
  if (rc) return rc;
  const spfe::MatchSide q = record_side(h, d_query_records), t = record_side(h, d_train_records);
  HIP_TRY(spfe::launch_match(q, t, n_pairs, cross_check != 0, h->m_best_t.as<unsigned long long>(),
                             h->m_best_q.as<unsigned long long>(), reinterpret_cast<uint8_t *>(d_out), (size_t)h->kmax * 8,
                             stream_of(h, stream)));
  return SPFE_OK;
}

int spfe_match(spfe_handle h, const float *query, int n_query, const float *train, int n_train, int cross_check,
               int32_t *train_idx, float *distance) {
  spfe::MatchSide q{}, t{};
  HostStage st(h);
  int rc = match_stage(h, st, query, n_query, train, n_train, 1, train_idx, distance, &q, &t);
  if (rc) return rc == kMatchNothing ? SPFE_OK : rc;
  uint8_t *out = h->m_out.p;
  const size_t col = (size_t)n_query * 4;
  HIP_TRY(spfe::launch_match(q, t, 1, cross_check != 0, h->m_best_t.as<unsigned long long>(),
                             h->m_best_q.as<unsigned long long>(), out, 0, h->stream));
  if ((rc = st.fetch_to(train_idx, out, col)) || (rc = st.fetch_to(distance, out + col, col))) return rc;
  return st.sync();
}

// knnMatch(query, matches, 2): the two nearest train rows of every query, exactly (the FLANN kd-tree the
// reference builds for this is approximate and randomised)
int spfe_match_knn2(spfe_handle h, const float *query, int n_query, const float *train, int n_train,
                    int32_t *train_idx, float *distance) {
  spfe::MatchSide q{}, t{};
  HostStage st(h);
  int rc = match_stage(h, st, query, n_query, train, n_train, 2, train_idx, distance, &q, &t);
  if (rc) return rc == kMatchNothing ? SPFE_OK : rc;
  uint8_t *out = h->m_out2.p;
  const size_t col = (size_t)n_query * 4;
  // scratch: best_q holds the first neighbours, best_t (>= cap entries) the second
  HIP_TRY(spfe::launch_match_knn2(q, t, 1, h->m_best_q.as<unsigned long long>(), h->m_best_t.as<unsigned long long>(),
                                  out, 0, h->stream));
  // device layout idx1 | dist1 | idx2 | dist2 -> host layout [n_query][2]
  std::vector<int32_t> hi(2 * (size_t)n_query);
  std::vector<float> hd(2 * (size_t)n_query);
  if ((rc = st.fetch_to(hi.data(), out, col)) || (rc = st.fetch_to(hd.data(), out + col, col)) ||
      (rc = st.fetch_to(hi.data() + n_query, out + 2 * col, col)) || (rc = st.fetch_to(hd.data() + n_query, out + 3 * col, col)) ||
      (rc = st.sync()))
    return rc;
  for (int i = 0; i < n_query; ++i) {
    train_idx[2 * i] = hi[i]; train_idx[2 * i + 1] = hi[n_query + i];
    distance[2 * i] = hd[i]; distance[2 * i + 1] = hd[n_query + i];
  }
  return SPFE_OK;
}

}  // extern "C"
