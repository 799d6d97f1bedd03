// spfe_kernels.h — launch interface between the host pipeline (spfe_schedule.hip) and
// the gfx950 kernels.  Everything here is internal to libspfe.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

namespace spfe {

// ---------------------------------------------------------------------------
// A kernel that asks for more dynamic LDS than the default limit has the limit raised before its first launch, once per
// launcher (per template instantiation) and device: the launcher keeps a function-local `static LdsLimitOnce`.
// Threads: distinct handles may be driven from distinct host threads (include/spfe.h "Threads"), so two threads can make the
// first launch of one kernel at the same moment.  The flags are atomics: a thread that reads true (acquire) does so after
// the hipFuncSetAttribute of the thread that stored it (release) returned; two threads that both read false both make the
// call, which the HIP runtime serialises and which sets the same value for the same function.  Either way the limit is
// raised before the calling thread's launch, and a failed call leaves the flag clear, so the next launch tries again.
// ---------------------------------------------------------------------------
struct LdsLimitOnce {
  std::atomic<bool> done[64] = {};   // by device ordinal: one process may hold handles on several GPUs
};
inline hipError_t raise_lds_limit(LdsLimitOnce &once, const void *kernel, int bytes) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  const bool slot = dev >= 0 && dev < 64;
  if (slot && once.done[dev].load(std::memory_order_acquire)) return hipSuccess;
  hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) return e;
  if (slot) once.done[dev].store(true, std::memory_order_release);
  return hipSuccess;
}

// ---------------------------------------------------------------------------
// f32 implicit-GEMM convolution on v_mfma_f32_32x32x2_f32 (conv_f32.hip)
// Activations are NHWC f32: element (b,y,x,c) at ((b*H+y)*W+x)*stride + choff + c.
// ---------------------------------------------------------------------------
struct ConvParams {
  const float *in;
  int in_stride, in_choff;
  const float *wpack;  // [nblk][chunk][n-tile(2)][tap][KC][32], K order of spfe_exact_math.h
  const float *bias;   // [nblk*64]
  float *out;
  int out_stride, out_choff, cout_real;
  int B, H, W;  // conv input == conv output size (before the optional 2x2 pool)
  int tiles_x, tiles_y, nblk;
  int num_cus;  // persistent grid size (multiProcessorCount)
  // layer_tag 2 (conv1a fused into conv1b): the u8 frames [B][H][W] and conv1a's taps [9][64] / bias [64];
  // `in` is then unused
  const uint8_t *img;
  const float *w1a, *b1a;
  // conv_bf16_ws.hip: nblk * 8 tile counters (one per XCD and 64-channel block), zero before the launch
  int *tile_ctr;
  // conv_f32.hip: the launch walks work items [item_lo, item_hi) of the list (frame, tile row, tile column, 64-channel
  // block); item_hi = 0: the whole list.  (conv1b's list is cut in two launches with different tile heights, spfe_schedule.hip.)
  int item_lo = 0, item_hi = 0;
};

// cin: 64/128/256; ksize: 3 or 1; pool/relu: fused epilogue; small_tile: 4-row
// tiles (more workgroups for the low-resolution layers).
// tile_mode: 0 = 8-row tiles (4 waves), 1 = 4-row tiles, 2 = 16-row tiles (8 waves, two per SIMD), 3 = 2-row tiles,
// 4 = 16-row tiles of 4 waves x 4 rows (conv1b)
hipError_t launch_conv_f32(const ConvParams &p, int cin, int ksize, bool pool, bool relu,
                           int tile_mode, int layer_tag, hipStream_t s);
// 2x2 / 2 max-pool of an NHWC f32 activation [B][H][W][C] -> [B][H/2][W/2][C] (H, W even, C % 4 == 0)
hipError_t launch_pool2x2_f32(const float *in, float *out, int B, int H, int W, int C, hipStream_t s);
int conv_kc(int ksize);        // K-chunk the kernel stages per barrier (16 for 3x3, 64 for 1x1)

// bf16 3x3 convolutions (conv_bf16.hip): in/out NHWC bf16 (out f32 when out_f32), strides in
// elements; wpack = bf16 slabs of conv_bf16_slab_bytes() each, [nblk][chunk of 32 ch][tap][64][80 B]
hipError_t launch_conv_bf16(const ConvParams &p, int cin, bool pool, bool out_f32, hipStream_t s, int tile_rows = 8);
size_t conv_bf16_slab_bytes();
// wave-specialised variant for the Cin = 64 layers (conv_bf16_ws.hip): wpack = conv_bf16_ws_weight_bytes() per
// 64-channel block, [nblk][tap][cout 64][8 x 16-byte pieces, piece g in slot g ^ ((cout >> 1) & 7)]
hipError_t launch_conv_bf16_ws(const ConvParams &p, bool pool, int layer_tag /* 1 = conv1b, 2 = conv1b with conv1a fused in (p.img / p.w1a / p.b1a) */, hipStream_t s);
size_t conv_bf16_ws_weight_bytes();
// register-resident-weights variant for the Cin = 128 layers (conv_bf16_rw.hip): p.nblk = 128-channel output groups,
// wpack = conv_bf16_rw_weight_bytes() per group in fragment order (conv_bf16_rw_pack_weights from [cout][128][9] bf16),
// bias f32 in channel order; tile_rows 4 | 2; p.tile_ctr: nblk * 8 zeroed counters.  Bit-identical to launch_conv_bf16.
hipError_t launch_conv_bf16_rw(const ConvParams &p, bool pool, int tile_rows, hipStream_t s);
size_t conv_bf16_rw_weight_bytes();
void conv_bf16_rw_pack_weights(const unsigned short *Wb, int cout, unsigned char *dst);
// conv1a of the bf16 mode (conv1a_mfma.h): wtab = the bf16 operand table [2][64][8] (conv1a_bf16_table_bytes()), b64 = bias
hipError_t launch_conv1a_bf16(const uint8_t *img, const void *wtab, const float *b64, void *out, int B, int H,
                              int W, hipStream_t s);
inline size_t conv1a_bf16_table_bytes() { return 2 * 64 * 8 * 2; }

// bf16 mode, the 1x1 heads (head_bf16.hip): out[npix][cout] f32 = in[npix][512] bf16 (channels 0..255 for the
// detector head, cout = 65; 256..511 for the descriptor head, cout = 256) x W^T + bias;
// wpack: head_bf16_weight_bytes(cout) bytes in MFMA fragment order, made by head_bf16_pack_weights from Wb = [cout][256] bf16
hipError_t launch_head1x1_bf16(const void *in_bf16, const void *wpack, const float *bias, float *out, int npix, int cout,
                               hipStream_t s);
// the descriptor head (cout = 256) on the *total (<= max_total) rows of in_bf16 / out that `list` names (device memory,
// select_kernel's FrameBufs::db_list / db_total): "sparse convDb"
hipError_t launch_head1x1_bf16_gather(const void *in_bf16, const void *wpack, const float *bias, float *out, int npix,
                                      const int *list, const int *total, int max_total, int tiles_per_wg, hipStream_t s);
// convDa (3x3, 128 -> 256, ReLU) on the listed cells (da_gather_bf16.hip): feat = conv4b's output [B][hc][wc][128] bf16,
// wpack = convPa|Da in conv_bf16_rw_pack_weights order, out = head activations [B * hc * wc][512] bf16 (channels 256..511)
hipError_t launch_da_gather_bf16(const void *feat, const void *wpack, const float *bias, void *out, const int *list,
                                 const int *total, int max_total, int B, int hc, int wc, int num_cus, hipStream_t s);
size_t head_bf16_weight_bytes(int cout);
void head_bf16_pack_weights(const unsigned short *Wb, int cout, unsigned char *dst);

// f32 mode, the 1x1 heads (head_f32.hip): same shapes, in / out f32, bit-identical to conv_f32.hip's 1x1 path
hipError_t launch_head1x1_f32(const float *in, const float *wpack, const float *bias, float *out, int npix, int cout,
                              hipStream_t s);
// f32 mode, convDa (3x3, 128 -> 256, ReLU) on the listed cells (da_gather_f32.hip), bit-identical to conv_f32.hip's rows:
// feat = conv4b's output [B][hc][wc][128], wpack = da_gather_f32_pack_weights(convDa's OIHW weights), bias = convDa's,
// out = head activations [B * hc * wc][512] (channels 256..511 of the listed rows)
hipError_t launch_da_gather_f32(const float *feat, const float *wpack, const float *bias, float *out, const int *list,
                                const int *total, int max_total, int B, int hc, int wc, int num_cus, hipStream_t s);
size_t da_gather_f32_weight_bytes();
void da_gather_f32_pack_weights(const float *W, float *dst);
hipError_t launch_head1x1_f32_gather(const float *in, const float *wpack, const float *bias, float *out, int npix,
                                     const int *list, const int *total, int max_total, int tiles_per_wg, hipStream_t s);
size_t head_f32_weight_bytes(int cout);
void head_f32_pack_weights(const float *W, int cout, float *dst);

// conv1a: u8 image -> (x * 1/255) -> 3x3 conv 1->64 + bias + relu, NHWC out.
// w: [9][64] (tap-major), b: [64]
hipError_t launch_conv1a(const uint8_t *img, const float *w9x64, const float *b64, float *out, int B,
                         int H, int W, hipStream_t s);

// ---------------------------------------------------------------------------
// detector tail, selection, descriptors (tail_select.hip)
// ---------------------------------------------------------------------------
struct FrameBufs {
  // per-frame strides are implied by H, W; all arrays are [B][...]
  const float *semi;    // [B][C][65]
  const float *coarse;  // [B][C][256]
  float *heat_log;      // [B][H][W]
  float *heat;          // [B][H][W] or null
  float *heat_inv;      // [B][H][W]
  uint32_t *minmax;     // [B][tail_parts][2] float partials of min/max of heat_log
  float *cell_score;    // [B][C]  0 = no candidate
  uint8_t *cell_k;      // [B][C]  arg-max channel
  uint8_t *cell_mask;   // [B][C]  which of the 8 neighbouring cells' candidates can suppress this one (nms_mask_kernel)
  int *kp_cell;         // [B][kmax] cell index of emitted keypoint
  int *sel_slot;        // [B][C] frames of more than 16,384 cells: select_kernel's per-cell slot / index hand-off (else null)
  uint16_t *sel_list;   // [B][C] ... and its tie / layout list
  uint8_t *sel_state;   // [B][C] frames of more than 65,535 cells (select_huge_kernel): the cell states ...
  int *sel_list32;      // [B][C] ... and the tie / layout list with 32-bit cell indices (else null)
  int sel_huge;         // 1: the selection runs as select_huge_kernel
  int *db_list;         // [B * min(4 kmax, C)] global cell indices (b * C + cell) some emitted keypoint's descriptor taps read,
  int *db_total;        // [1] ... and how many: written by select_kernel for the gathered descriptor head (or both null)
  uint8_t *records;     // [B][record_bytes]
  float *heat_consts;   // [B][4] a_heat, b_heat, a_inv, b_inv
};

struct RecordLayout {
  size_t bytes;
  int kmax;
  size_t off_hdr, off_xy, off_resp, off_cov, off_cinv, off_desc, off_occ, off_dd, off_sd;
  int desc_bf16;   // SPFE_FLAG_DESC_BF16: descriptor rows are 256 bf16 (RNE of the f32 descriptor), not 256 f32
};

// scratch of the covariance kernels (cov.hip)
struct CovScratch {
  int *claim;     // [B][H*W] lowest keypoint index whose lone walk popped the pixel
  int *done;      // [B][H*W] lowest FINAL keypoint index that popped the pixel
  int *queue;     // [B][kmax][qcap] per-keypoint pop list (pixel index)
  float *qval;    // [B][kmax][qcap] heat_inv value of each popped pixel
  int *npop;      // [B][kmax]
  int *dirty;     // [B][kmax] keypoints whose lone region meets a lower keypoint's
  int *nxt;       // [B][kmax] next dirty member of the same component (ascending) or -1
  float *nxy;     // [B][kmax][2] keypoint position of nxt
  int *workers;   // [B][kmax] lowest dirty member of each component
  int *counters;  // [B][4] number of dirty keypoints, number of components, overflow slots taken, claim edges listed
  int *edges;     // [B][ecap] int2 (lower claimant, dirty keypoint): the union-find's input, written by the classification (or null)
  int ecap;
  int qcap;
  // walks that outgrow qcap redo themselves in one of ovf_slots per-frame slots of ovf_cap entries
  int *ovf_slot;  // [B][kmax] slot of the keypoint's pop list, or -1
  int *ovf_q;     // [B][ovf_slots][ovf_cap]
  float *ovf_v;
  int ovf_slots, ovf_cap;
  // last resort (cov_fallback_kernel): ONE pop list of fb_cap entries for the whole batch; a flagged frame is redone
  // sequentially, literally, on the device
  int *fb_q;
  float *fb_v;
  int fb_cap;
  // claim / done entries carry the batch's GENERATION in their upper 16 bits (gen = code << 16, the code counts DOWN from
  // 32,766 per chain): an entry of an earlier batch reads as "nobody" and loses every atomicMin against this batch's, so the
  // maps are not cleared per batch (2 x 4 H W bytes per frame: half of what the heat normalisation moved) — only before a
  // frame's first use and when the code wraps (reset_maps; COV_RESET, code 32,767, is never a batch's)
  int gen;
  int reset_maps;
};
#define COV_RESET 0x7fffffff
size_t cov_link_lds(int kmax);
// with_desc: the descriptor sampling (launch_desc) as extra wavefronts of the replay launch, behind `before_replay` if given
// replay_waves: components per replay workgroup, 2 (default) or 8 (bf16 pipelined calls: see cov.hip)
hipError_t launch_cov(const FrameBufs &f, const RecordLayout &r, const CovScratch &cs, int B, int H, int W,
                      hipStream_t s, bool with_desc = false, hipEvent_t before_replay = nullptr, int replay_waves = 2,
                      bool defer_moments = false);   // defer_moments: synchronous calls (cov.hip, cov_replay_kernel)

int tail_parts(int H, int W);  // min/max partials per frame written by the tail kernel
// f32 mode: convPb (1x1, 256 -> 65) + the detector tail in one launch (pbtail_f32.hip), bit-identical to convPb through
// conv_f32.hip followed by launch_tail.  head = [B * C][512] f32 (channels 0..255 = ReLU(convPa)); wpack =
// head_f32_pack_weights(convPb's weights, 65); wdust = convPb's row 64 [256]; bias [>= 65]; semi [B][C][65] is written too
hipError_t launch_pbtail_f32(const float *head, const float *wpack, const float *wdust, const float *bias, float *semi,
                             const FrameBufs &f, const RecordLayout &r, int B, int H, int W, hipStream_t s, int b0 = 0);
// bf16 mode: the same fusion (pbtail_bf16.hip), bit-identical to launch_head1x1_bf16(.., 65, ..) followed by launch_tail.
// head = [B * C][512] bf16; wpack = head_bf16_pack_weights(convPb, 65); zero_ints / nzero as launch_tail's
hipError_t launch_pbtail_bf16(const void *head, const void *wpack, const float *bias, float *semi, const FrameBufs &f,
                              const RecordLayout &r, int B, int H, int W, hipStream_t s, int b0 = 0, int *zero_ints = nullptr,
                              int nzero = 0, int zstride = 32, int force = 0);   // (zero_ints: nzero ints in runs of 32, zstride apart; force: 2 | 4 wavefronts, 0 = by launch size)   // frames [b0, b0 + B) of the batch-wide buffers
// zero_ints / nzero: ints the kernel also clears (the bf16 convolutions' tile-queue counters, for the next call)
hipError_t launch_tail(const FrameBufs &f, const RecordLayout &r, int B, int H, int W, hipStream_t s, int *zero_ints = nullptr, int nzero = 0);
// with_heat_norm: the heat normalisation (launch_heat_norm) rides in the neighbour-mask launch in front of the selection
// lean: the form that keeps only the cell states and neighbour masks in LDS (2 bytes a cell; the per-cell private data in
// FrameBufs::sel_slot / sel_list) also on frames that would fit the all-in-LDS form (9 bytes a cell: 64 KB at 752x480, 143 KB
// at 1280x720 — a whole CU): a pipelined call's selection then starts beside a convolution workgroup instead of waiting for a CU
hipError_t launch_select(const FrameBufs &f, const RecordLayout &r, int B, int H, int W,
                         int num_features, hipStream_t s, const CovScratch *with_heat_norm = nullptr, int kmax_hn = 0,
                         bool lean = false, hipEvent_t done = nullptr, hipEvent_t heat_done = nullptr);
// (heat_done: an event that fires when the heat normalisation — the launch in FRONT of the selection — has completed: the heat
// maps are final there, ~150 us before a single-frame call's record is, and a synchronous host call starts their D2H behind it)
// (also resets the covariance scratch: launch_cov must follow it)
hipError_t launch_heat_norm(const FrameBufs &f, const CovScratch &cs, int kmax, int B, int H, int W, hipStream_t s);
hipError_t launch_desc(const FrameBufs &f, const RecordLayout &r, int B, int H, int W, hipStream_t s);
size_t select_lds_bytes(int H, int W, bool lean = false);
bool select_big(int H, int W);     // more than 16,384 cells: per-cell private data in global scratch (FrameBufs::sel_slot / sel_list)
size_t select_max_cells();         // 65,535: select_kernel
size_t select_huge_max_cells();    // 262,143: select_huge_kernel (frames beyond select_kernel's)
size_t select_huge_lds_bytes(int H, int W);

// ---------------------------------------------------------------------------
// brute-force descriptor matching (match.hip)
// One "side" = `pairs` blocks `stride` bytes apart, each holding an int32 count at off_cnt
// and count x 256 f32 descriptors at off_desc (a record of the extraction path has this
// shape; so has the staging block of the host API).  cap bounds the count.
// ---------------------------------------------------------------------------
struct MatchSide {
  const uint8_t *base;
  size_t stride, off_cnt, off_desc;
  int cap;
  int desc_bf16 = 0;   // rows are 256 bf16 (records made with SPFE_FLAG_DESC_BF16): widened on load, distances in f32 on those values
  // the TRAIN side of a cross-check match (launch_match refuses it elsewhere), and with it the QUERY side (the loop match,
  // sp_matcher_loop.cpp:334-376: a masked query casts no vote and gets no result): row r of pair p takes part iff
  // 0 <= mask[p * cap + r] < mask_n — the result is that of matching against the compacted rows, with the rows' own indices
  // (sp_matcher.cpp:1654-1660: the keyframe's keypoints that hold a map point).  null: every row takes part
  const int *mask = nullptr;
  int mask_n = 0;
  // launch_match_knn2_free only: the row (either side) takes part iff mask[p * cap + r] < 0 — a FREE keypoint, one that holds
  // no map point (sp_matcher.cpp:183-262 matches mDescReamin of both keyframes); mask_n is not read
  int mask_free = 0;
};
// out: per pair `out_stride` bytes: int32 train_idx[query.cap] (-1 = none), float dist[query.cap].
// best_t: [pairs][train.cap], best_q: [pairs][query.cap] scratch.
hipError_t launch_match(const MatchSide &query, const MatchSide &train, int pairs, bool cross_check,
                        unsigned long long *best_t, unsigned long long *best_q, uint8_t *out, size_t out_stride,
                        hipStream_t s);

// mp_of_kp[q] = kf_mp_of_kp[train_idx[q]] for the matched queries below the record's K (values outside [0, n): -1), -1 for
// every other entry of [0, kmax); a record with SPFE_STATUS_COV_OVERFLOW gets -1 throughout (sp_matcher.cpp:1671-1673)
// n 32-bit words at p set to v, as a kernel (match.hip): what the device forms preset is no memset node of a captured graph
hipError_t launch_fill_u32(void *p, uint32_t v, size_t n, hipStream_t s);
hipError_t launch_match_scatter_points(const int32_t *train_idx, const int *kf_mp_of_kp, const int *hdr, int kmax, int n,
                                       int *mp_of_kp, hipStream_t s);

// the two nearest train rows per query (cv::DescriptorMatcher::knnMatch(query, matches, 2)); out per pair:
// idx1[query.cap] | dist1[query.cap] | idx2[query.cap] | dist2[query.cap]
hipError_t launch_match_knn2(const MatchSide &query, const MatchSide &train, int pairs, unsigned long long *best1,
                             unsigned long long *best2, uint8_t *out, size_t out_stride, hipStream_t s);

// The two nearest FREE train rows of every FREE query (both sides with mask_free), as the kernel's own keys: best1 / best2
// [query.cap] = (dist bits << 32 | train row), ~0 where there is none (a held query, fewer train rows).  Held train rows
// compute their distances like any other and never compete; every row keeps its own index.  One pair of records.
hipError_t launch_match_knn2_free(const MatchSide &query, const MatchSide &train, unsigned long long *best1,
                                  unsigned long long *best2, hipStream_t s);

// ---------------------------------------------------------------------------
// new map points between two keyframes (tri.hip; local_mapper.cpp:558-814, sp_matcher.cpp:183-262, :441-469)
// ---------------------------------------------------------------------------
struct TriArgs {
  // the two records (1 = current keyframe, 2 = neighbour): headers, keypoints, cov2_inv
  const int *hdr1, *hdr2;
  const float *xy1, *xy2, *cinv1, *cinv2;
  int kmax;
  int *mp1, *mp2;                  // [kmax] in/out
  const float *Tcw1, *Tcw2;        // [16]
  const float *median_depth;       // the neighbour's scene median depth on the device, or null: no baseline test
  float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2, ratio, epipole_r2;
  double chi2_line, chi2_reproj, cos_parallax_max, min_baseline_depth_ratio;
  int point_base, set_base;        // set_base: *next_id = point_base before this neighbour (else the ids run on)
  int *next_id;                    // device counter: the id of the next new point
  const unsigned long long *best1, *best2;   // launch_match_knn2_free's keys, [kmax]
  uint8_t *out;                    // the SPFE_TRI_OUT_BYTES(kmax) block
};
// the block's int32 fields, the baseline / refusal decision, match12 = -1 and verdict = 0: in FRONT of the search
hipError_t launch_tri_begin(const TriArgs &a, hipStream_t s);
// the pair gate and the triangulation with its ordered compaction: BEHIND the search
hipError_t launch_tri_gate_triangulate(const TriArgs &a, hipStream_t s);

// ---------------------------------------------------------------------------
// loop verification (sim3.hip; loop_closer_vlad.cpp:345-449, sp_matcher_loop.cpp:334-376, sim3_solver.cpp)
// ---------------------------------------------------------------------------
// match12[t] = q for the matched queries q of launch_match's train_idx (q below record 2's count, t below kmax), -1 for every
// other entry of [0, kmax); *n_matches = their number
hipError_t launch_loop_match_invert(const int32_t *train_idx, const int *hdr2, int kmax, int *match12, int *n_matches,
                                    hipStream_t s);
struct Sim3Args {
  int n_cand;                 // candidate j = blockIdx.y / blockIdx.x
  const int *hdr1;            // record 1's header (K1 is read on the device), or null -> k_imm
  int k_imm;
  int kcap;                   // entries of the index arrays and the block's kmax
  const int *match12;         // [n_cand][kcap]
  const int *mp1;             // [kcap] kf1_mp_of_kp
  const int *mp2;             // [n_cand][kcap] kf2_mp_of_kp
  const float *xyz;           // [n][3]
  const uint8_t *flags;       // [n]
  int n;
  const float *Tcw1;          // [16]
  const float *Tcw2;          // [n_cand][16]
  const uint32_t *rnd;        // [n_cand][n_hyp][3]
  int n_hyp;
  float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2, max_err1, max_err2;
  int min_inliers, fix_scale;
  float *scratch;             // [n_cand][kcap][10]: X1c, X2c, P1im1, P2im2 of pair i
  uint8_t *out;               // [n_cand] blocks of SPFE_SIM3_OUT_BYTES(kcap, n_hyp)
};
hipError_t launch_sim3(const Sim3Args &a, hipStream_t s);

// ---------------------------------------------------------------------------
// input staging (stage_input.hip): raw camera frames -> cropped gray u8 frames
// ---------------------------------------------------------------------------
struct StageParams {
  const uint8_t *src;        // [n] frames, src_frame_bytes apart, rows src_stride bytes apart
  size_t src_frame_bytes;
  int src_stride, src_h, src_w;
  const float *map_x, *map_y;  // [src_h][src_w] or null (no remap)
  int rgb;                     // 1: R first
  uint8_t *gray;               // [n][H][W]
  int H, W;
};
hipError_t launch_stage_input(const StageParams &p, int channels, int n, hipStream_t s);

// patch-wise association of projected map points (match.hip; tracker_dust.cpp:113-172)
struct PatchArgs {
  const float *mp_desc;  // [n_points][256]
  const float *mp_uv;    // [n_points][2] projected dust-map position (cells)
  int n_points;
  const int16_t *occ;    // [hc][wc] keypoint index per cell, -1 = empty
  int hc, wc;
  const float *kp_desc;  // [K][256]
  int kp_desc_bf16 = 0;  // ... as bf16 rows (a record made with SPFE_FLAG_DESC_BF16)
  const int *k_ptr;      // K on the device (a record header), or null -> k_imm
  int k_imm;
  // chained form (spfe_track_dust_record_device): map points whose in_view flag is 0 are skipped
  // (tracker_dust.cpp:114-116), and all of them when *gate_ptr < gate_min (the tracker gives up at :97-102)
  const uint8_t *in_view;  // [n_points] or null
  const int *gate_ptr;     // n_inlier of the alignment on the device, or null
  int gate_min;
};
// cand_idx / cand_dist: [n_points][4] scratch; out: [n_points] keypoint index or -1; kcap >= K
// patch_resolve_lds_bytes: the claim workgroup's dynamic LDS; _total: with its static part (at most 160 KB is served)
size_t patch_resolve_lds_bytes(int kcap);
size_t patch_resolve_lds_total(int kcap);
hipError_t launch_match_patches(const PatchArgs &a, int kcap, float max_dist, int *cand_idx, float *cand_dist,
                                int32_t *out, hipStream_t s);

// direct "dust" alignment (dust.hip; optimizer_dust.cpp:170-294): one workgroup, Levenberg-Marquardt over n points
constexpr int DUST_MAX_POINTS = 512;
struct DustArgs {
  const float *dust;   // [hc][wc] dense_dust (device)
  int hc, wc;
  const float *pts;    // [n][3] world positions (device)
  int n;
  const float *Tcw_in; // [16] row-major 4x4 (device)
  float fx, fy, cx, cy;   // full-resolution intrinsics
  int max_iterations;
  double delta, inlier_chi2;
  float *Tcw_out;      // [16]
  unsigned char *inlier;  // [n]
  float *uv;           // [n][2]
  int *counts;         // n_inlier, iterations
  // batched form (one workgroup per frame f = blockIdx.x): byte strides added to dust / pts+Tcw_in / the four outputs;
  // n_dev (or null) = per-frame point counts on the device
  int nframes;
  size_t dust_stride, pts_stride, pose_stride, out_stride;
  const int *n_dev;
  int map_in_lds;   // set by launch_dust_align: the dust map fits in LDS beside the per-point arrays
};
hipError_t launch_dust_align(const DustArgs &a, hipStream_t s);
size_t dust_lds_bytes(int hc, int wc);

// covariance-weighted pose refinement (pose.hip; optimizer_dust.cpp:35-167, optimizer.cpp:231-443): one workgroup per solve
struct PoseArgs {
  const float *kp_xy;      // [K][2] keypoints (the record's, or the host form's observations)
  const float *cinv;       // [K][2] cov2_inv
  const int *mp_of_kp;     // [K] map point per keypoint (-1: none), or null: keypoint j is edge j with map point j
  const float *pts;        // [.][3] world positions
  int n_pts = -1;          // rows of pts: a holder outside [0, n_pts) is no edge (the chains' rule); -1: unknown, every holder
                           // >= 0 is an index (the plain forms: the range is the caller's duty)
  const int *hdr;          // the record header (K, n_candidates, status), or null -> k_imm, status 0
  int k_imm;
  const float *Tcw_in;     // [16] the starting pose
  const float *Tcw_echo;   // [16] the pose written on the chained form's failing paths (null elsewhere)
  float fx, fy, cx, cy;
  int schedule, iterations;
  unsigned char *out;      // the spfe_pose_out_bytes block
  int kmax;                // keypoints per record (the LDS arrays' length)
  // batched form (frame f = blockIdx.x): byte strides added to kp_xy / cinv / hdr, mp_of_kp, pts, Tcw_in, out
  int nframes;
  size_t rec_stride, map_stride, pts_stride, pose_stride, out_stride;
  // chained form: the alignment's n_inlier on the device and the tracker's gates
  const int *gate_inliers;
  int th_ninlier, th_nmatch;
  float th_ratio;
  size_t lds_bytes;        // set by launch_pose_refine
};
hipError_t launch_pose_refine(const PoseArgs &a, hipStream_t s);
// the most edges of a kmax-keypoint solve whose data is staged in LDS (more: read from global memory); -1: kmax unsupported
int pose_lds_edge_capacity(int kmax);
// mp_of_kp[kp_idx[i]] = i for the n associations (mp_of_kp already -1): the chained form's keypoint order
hipError_t launch_pose_scatter(const int *kp_idx, int n, int *mp_of_kp, int kmax, hipStream_t s);

// window search by projection (proj.hip; sp_matcher.cpp:344-432, :1439-1543, frame.cpp:330-420, tracker.cpp:768-832)
struct ProjArgs {
  // the frame: a record (hdr = its header: K and the status are read on the device) or staged host arrays (hdr null -> k_imm)
  const float *kp_xy;      // [K][2]
  const int16_t *occ;      // [hc][wc]
  const float *kp_desc;    // [K][256] f32, or bf16 rows (kp_desc_bf16)
  int kp_desc_bf16;
  const int *hdr;
  int k_imm;
  int refuse_overflow;     // chained form: a record with SPFE_STATUS_COV_OVERFLOW is not searched, mp_of_kp stays as it is
  int hc, wc, kmax;
  float W, H;              // the frame's bounds (mnMaxX, mnMaxY)
  // the map points
  const float *xyz, *normal, *desc;   // [n][3], [n][3], [n][256]
  const uint8_t *flags;               // [n] SPFE_PROJ_SEARCHABLE | SPFE_PROJ_OBSERVED
  int n;
  const int *n_dev;        // per-frame counts on the device (batch form), or null -> n
  int *mp_of_kp;           // [kmax] in/out
  const float *Tcw;        // [16]
  float fx, fy, cx, cy;
  int mode;
  float th, th_dist, view_cos_limit;
  int adaptive;
  float c2;
  uint8_t *out;            // the SPFE_PROJ_OUT_BYTES block
  // batched form (frame f = blockIdx.y / blockIdx.x): byte strides added to kp_xy / occ / kp_desc / hdr, the point arrays,
  // mp_of_kp, Tcw, out
  int nframes;
  size_t rec_stride, xyz_stride, desc_stride, flags_stride, map_stride, pose_stride, out_stride;
  // scratch: per frame `cap` points (the most any frame holds), per point SPFE_PROJ_MAX_CAND candidates in window order
  int cap;
  int *cand_k;             // [nframes][cap][SPFE_PROJ_MAX_CAND] keypoint
  float *cand_d;           // ... its distance
  float *cand_duv;         // ... its squared pixel offset
  int *cand_n;             // [nframes][cap] candidates of the point
  uint8_t *held;           // [nframes][cap] LOCAL_MAP: the point is held by a keypoint on entry
  // gated form (single frame; TrackWithMotionModel's retry, tracker.cpp:503-508): the launches do their work only when
  // *gate_count < gate_min and the record is not refused — mp_of_kp is then taken as all -1 on entry — and write nothing
  // otherwise; *gate_flag (if given) receives 1 / 0.  gate_count may be the n_matches of `out` itself.  null: no gate
  const int *gate_count;
  int gate_min;
  int *gate_flag;
};
size_t proj_resolve_lds_bytes(int kmax);   // the claim workgroup's dynamic LDS
size_t proj_resolve_lds_total(int kmax);   // ... with its static part: at most 160 KB is served
hipError_t launch_proj_search(const ProjArgs &a, hipStream_t s);
// mnMatchesInliers and the verdict of TrackLocalMap into the pose block `pose_out` (tracker.cpp:576-612)
hipError_t launch_local_map_verdict(const int *hdr, int kmax, const int *mp_of_kp, const uint8_t *flags, int n,
                                    const uint8_t *proj_out, int th_ninlier, uint8_t *pose_out, hipStream_t s);

// "Discard outliers" behind PoseOptimization (tracker.cpp:395-410, :519-535) into mp_of_kp and the pose block `pose_out`:
// holders that are outliers are emptied and their flag cleared (n_outliers), the other holders of an OBSERVED point are
// n_inliers; verdict OK when n_inliers >= th_nmatch_opt, else fail_verdict (SPFE_TRACK_FAIL_COV on a refused record).
// n_matches = *n_matches_src, or the holders on entry when null
hipError_t launch_track_discard(const int *hdr, int kmax, int *mp_of_kp, const uint8_t *flags, int n, const int *n_matches_src,
                                int th_nmatch_opt, int fail_verdict, uint8_t *pose_out, hipStream_t s);

// the search of SPMatcher::Fuse (fuse.hip; sp_matcher.cpp:965-1104, keyframe.cpp:1018-1060): map points projected into
// n_targets keyframes, target j = blockIdx.y
constexpr int FUSE_MAX_TARGETS = 128;
struct FuseArgs {
  // target j's arrays lie at base[j] + off_*: a record of the handle's layout, or the host form's staging block.
  // off_hdr < 0: no header, K = k_imm and the status is 0
  const uint8_t *base[FUSE_MAX_TARGETS];
  int n_targets;
  long off_xy, off_occ, off_desc, off_hdr;
  int kp_desc_bf16, k_imm;
  int hc, wc, kmax;
  float W, H;
  const int *kf_mp_of_kp;   // [n_targets][kmax], read only
  const float *Tcw;         // [n_targets][16]
  // the shared point list
  const int *point_id;                            // [n]
  const float *xyz, *normal, *dist_range, *desc;  // [n][3], [n][3], [n][2], [n][256]
  const uint8_t *flags;                           // [n]
  int n, cap;
  float fx, fy, cx, cy, th, th_dist, min_factor, max_factor;
  double chi2, view_cos;
  uint8_t *out;             // [n_targets] blocks of SPFE_FUSE_OUT_BYTES(cap)
};
hipError_t launch_fuse_search(const FuseArgs &a, hipStream_t s);
// its second launch alone: fused_idx and the three int32 fields of every target's block from the reason codes
hipError_t launch_fuse_compact(const FuseArgs &a, hipStream_t s);

// the search of SPMatcher::Fuse(KeyFrame *, cv::Mat Scw, ...) (loopfuse.hip; sp_matcher.cpp:1106-1219) on the same arguments:
// a.Tcw holds the targets' similarities Scw [n_targets][16], a.chi2 is not read.  The search workgroup stages kmax int32 in
// dynamic LDS
size_t loopfuse_lds_bytes(int kmax);
hipError_t launch_loopfuse_search(const FuseArgs &a, hipStream_t s);
// the corrected poses of CorrectLoop (loop_closer_vlad.cpp:536-571, :608-618), one thread per connected keyframe
hipError_t launch_loopfuse_poses(const double *S12, const float *Tcw2, const float *Twc, const float *Tiw, int n_targets,
                                 int cur_index, float *Siw, float *Tiw_corrected, hipStream_t s);

// the guided match under a Sim3 hypothesis (guided.hip; sp_matcher_loop.cpp:7-220): n_jobs (candidate, hypothesis) pairs
// against the current keyframe, job q = blockIdx.z / blockIdx.x
constexpr int GUIDED_MAX_JOBS = 32;
struct GuidedArgs {
  // keyframe 1's arrays lie at base1 + off_*, job q's keyframe 2 at base2[q] + off_*: records of the handle's layout, or the
  // host form's two staging blocks.  off_hdr < 0: no header, K1 = k_imm1, K2 = k_imm2 and the status is 0
  const uint8_t *base1;
  const uint8_t *base2[GUIDED_MAX_JOBS];
  int cand[GUIDED_MAX_JOBS], hyp[GUIDED_MAX_JOBS];   // what the per-candidate arrays and the verify blocks are indexed with
  int n_jobs;
  long off_xy, off_occ, off_desc, off_hdr;
  int kp_desc_bf16, k_imm1, k_imm2;
  int hc, wc, kmax;
  float W, H;
  const int *mp1;           // [kmax] kf1_mp_of_kp
  const int *mp2;           // [n_cand][kmax] kf2_mp_of_kp
  const float *xyz, *dist_range, *desc;   // the map: [n][3], [n][2], [n][256]
  const uint8_t *flags;                   // [n]
  int n;
  const float *Tcw1;        // [16]
  const float *Tcw2;        // [n_cand][16]
  // single form: the transform and the seed as arrays (verify == null)
  const float *T12;         // [13]
  const int *seed12;        // [kmax]
  // batched form: both are read from candidate cand[q]'s verify block, hypothesis hyp[q]
  const uint8_t *verify;    // [n_cand] blocks of SPFE_SIM3_OUT_BYTES(kmax, n_hyp)
  const int *match12;       // [n_cand][kmax]
  int n_hyp;
  float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2, th, th_dist, min_factor, max_factor;
  uint8_t *scratch;         // [n_jobs] blocks of guided_scratch_bytes(kmax): seed | T12, skip | already2
  uint8_t *out;             // [n_jobs] blocks of SPFE_GUIDED_OUT_BYTES(kmax)
};
__host__ __device__ size_t guided_scratch_bytes(int kmax);
hipError_t launch_guided_match(const GuidedArgs &a, hipStream_t s);

// the loop's map points projected into one keyframe (guided.hip; sp_matcher_loop.cpp:222-332): candidates, then the ordered claim
struct LoopProjArgs {
  const float *kp_xy;
  const int16_t *occ;
  const float *kp_desc;
  const int *hdr;           // the record's header, or null -> k_imm, status 0
  int kp_desc_bf16, k_imm;
  int hc, wc, kmax;
  float W, H;
  const float *Scw;         // [16]
  int *matched;             // [kmax] in/out
  const int *point_id;
  const float *xyz, *normal, *dist_range, *desc;
  const uint8_t *flags;
  int n, cap;
  float fx, fy, cx, cy, th, th_dist, min_factor, max_factor;
  double view_cos;
  int *cand_k;              // [cap][SPFE_PROJ_MAX_CAND] scratch: the window's keypoints in window order
  float *cand_d;            // ... and their distances
  int *cand_n;              // [cap]
  uint8_t *out;             // SPFE_LOOPPROJ_OUT_BYTES(cap)
};
size_t loop_proj_lds_bytes(int kmax);   // the claim workgroup's dynamic LDS
size_t loop_proj_lds_total(int kmax);   // ... with its static part: at most 160 KB is served
hipError_t launch_loop_proj(const LoopProjArgs &a, hipStream_t s);

// the Sim3 optimisation of a hypothesis (sim3opt.hip; optimizer.cpp:1062-1252): one workgroup per job, job q = blockIdx.x
struct Sim3OptArgs {
  // keyframe 1's arrays lie at base1 + off_*, job q's keyframe 2 at base2[q] + off_*: records of the handle's layout, or the
  // host form's two staging blocks.  off_hdr < 0: no header, K1 = k_imm1, K2 = k_imm2 and the status is 0
  const uint8_t *base1;
  const uint8_t *base2[GUIDED_MAX_JOBS];
  int cand[GUIDED_MAX_JOBS], hyp[GUIDED_MAX_JOBS];
  int n_jobs;
  long off_xy, off_hdr;
  int k_imm1, k_imm2, kmax;
  const int *mp1;           // [kmax] kf1_mp_of_kp
  const int *mp2;           // [n_cand][kmax] kf2_mp_of_kp
  const float *xyz;         // the map: [n][3]
  const uint8_t *flags;     // [n]
  int n;
  const float *Tcw1;        // [16]
  const float *Tcw2;        // [n_cand][16]
  // single form: the start value and the correspondences as arrays (verify == null)
  const float *T12;         // [13]
  const int *matches12;     // [kmax]
  // batched form: T12[hyp[q]] of candidate cand[q]'s verify block, matches12 of guided block q
  const uint8_t *verify;    // [n_cand] blocks of SPFE_SIM3_OUT_BYTES(kmax, n_hyp)
  const uint8_t *guided;    // [n_jobs] blocks of SPFE_GUIDED_OUT_BYTES(kmax)
  int n_hyp;
  float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2, th2;
  int fix_scale, iterations, min_kept, min_inliers;
  float *scratch;           // [n_jobs] blocks of sim3opt_scratch_bytes(kmax): the edge data of the served correspondences
  uint8_t *out;             // [n_jobs] blocks of SPFE_SIM3OPT_OUT_BYTES(kmax)
  size_t lds_bytes;         // set by launch_sim3opt
};
size_t sim3opt_scratch_bytes(int kmax);
// the most served correspondences of a kmax-keypoint solve whose edge data is staged in LDS; -1: kmax unsupported
int sim3opt_lds_edge_capacity(int kmax);
hipError_t launch_sim3opt(const Sim3OptArgs &a, hipStream_t s);

// bundle adjustment on keyframe records (ba.hip; optimizer.cpp:445-774, :51-229): one workgroup per problem
constexpr int BA_MAX_KEYFRAMES = 128;
struct BaArgs {
  // record form: keyframe k's arrays lie at base[k] + off_*; host form (off_hdr < 0): obs_xy / inv_sigma2 per edge, no K
  const uint8_t *base[BA_MAX_KEYFRAMES];
  long off_xy, off_cinv, off_hdr;
  int kmax;
  const float *obs_xy;      // [E][2] or null
  const float *inv_sigma2;  // [E][2] or null
  const int *edges;         // [E][3] point, keyframe slot, keypoint
  int E;
  const float *Tcw;         // [n_kf][16]
  const uint8_t *fixed;     // [n_kf]
  int n_kf;
  const float *xyz;         // [n][3]
  int n;
  float fx, fy, cx, cy;
  int schedule, it0, it1, robust;
  float inv_sigma2_full;
  const int *stop;          // null or one int
  uint8_t *out;             // SPFE_BA_OUT_BYTES(n_kf, n, E)
  uint8_t *scratch;         // ba_scratch_bytes(n, E)
};
size_t ba_scratch_bytes(int n, int E);
int ba_lds_free_capacity();   // the most free keyframes whose reduced system is kept in LDS
hipError_t launch_ba(const BaArgs &a, hipStream_t s);

// the map-point table (mappoint.hip; mappoint.cpp:237-302, :322-364): m listed points refreshed from the keyframe records
struct MpArgs {
  // the record form: record pointers, flags and poses of the n_kf keyframes, all on the device; rows at base + off_desc
  const uint8_t *const *records;   // [n_kf]; null in the host form
  const uint8_t *kf_flags;         // [n_kf]
  const float *Tcw;                // [n_kf][16]
  int n_kf;
  long off_desc, off_hdr;
  int desc_bf16, kmax;
  // the host form (records == null): the observations already gathered
  const float *obs_desc;           // [E][256]
  const uint8_t *obs_good;         // [E]
  const float *obs_Ow, *ref_Ow;    // [E][3], [m][3]
  // the listed points
  const int *point_idx;            // [m] or null: row i
  const int *obs_start, *obs, *ref_slot;   // [m + 1], [E][2], [m]
  int m, E;
  // the table
  const float *xyz;                // [n_table][3]
  const uint8_t *flags;            // [n_table]
  float *normal, *dist_range, *desc;   // [n_table][3], [n_table][2], [n_table][256]
  int n_table;
  int mode;
  float level_scale, top_scale;
  uint8_t *out;                    // SPFE_MP_OUT_BYTES(m)
};
int mp_lds_obs_capacity(int desc_elem_bytes);
hipError_t launch_mp_refresh(const MpArgs &a, hipStream_t s);
struct MpGatherArgs {
  const int *idx;
  int n, n_table;
  const float *xyz, *normal, *dist_range, *desc;
  const uint8_t *flags;
  int *o_id;
  float *o_xyz, *o_normal, *o_dist_range, *o_desc;
  uint8_t *o_flags;
};
hipError_t launch_mp_gather(const MpGatherArgs &a, hipStream_t s);

// the essential graph over Sim3 and the map corrections (essgraph.hip; optimizer.cpp:776-1060, loop_closer_vlad.cpp:575-606)
struct EgArgs {
  const double *est, *meas;   // [n][8]
  const uint8_t *flags;       // [n]
  int n;
  const int *edges;           // [E][3]
  int E, env_cap;
  int iterations, fix_scale;
  double lambda_init;
  uint8_t *out;               // SPFE_ESSGRAPH_OUT_BYTES(n)
  uint8_t *scratch;           // eg_scratch_bytes(n, E, env_cap)
};
size_t eg_scratch_bytes(int n, int E, int env_cap);
int eg_lds_panel_capacity();   // the most block rows of a column panel staged in LDS
hipError_t launch_eg_optimize(const EgArgs &a, hipStream_t s);
hipError_t launch_eg_sim3(const float *Tcw, const double *S12, const float *Tcw2, const float *Twc, const int *conn_slot, int n_conn,
                          int cur_slot, double *est, double *meas, int n, hipStream_t s);
hipError_t launch_eg_correct(const double *S_from, const double *S_to, int n_kf, const int *ref_slot, const int *point_idx, int m,
                             float *xyz, const uint8_t *flags, int n_table, uint8_t *code, hipStream_t s);

// the loop detection (loopdet.hip; loop_closer_vlad.cpp:42-118, :150-165): roles, scores, decisions of one query
struct LoopdetArgs {
  const float *gdesc;          // [n_slots][dim]
  int dim;
  const uint8_t *kf_flags;     // [n_slots]
  const uint8_t *in_db;        // [n_slots]
  const int *best_cov;         // [n_slots][SPFE_LOOPDET_NEIGH]
  int n_slots, cur_slot;
  const int *connected, *covisible;   // [n_conn], [n_cov]
  int n_conn, n_cov;
  float min_score_init, min_score_floor, retain_ratio;
  uint8_t *out;                // SPFE_LOOPDET_OUT_BYTES(n_slots)
};
hipError_t launch_loopdet(const LoopdetArgs &a, hipStream_t s);

// the tracker's local map (localmap.hip; tracker.cpp:834-984)
struct LocalmapArgs {
  const int *kf_mp_of_kp;      // [n_slots][kp_stride]
  int kp_stride;
  const uint8_t *kf_flags;     // [n_slots]            (null in the count form)
  const int *best_cov;         // [n_slots][n_best]    (null in the count form)
  int n_best;
  const int *parent;           // [n_slots]            (null in the count form)
  int n_slots;
  const uint8_t *mp_flags;     // [n_table]
  int n_table;
  const int *mp_of_kp;         // [n_kp]
  const uint8_t *outlier;      // [n_kp] or null
  int n_kp;
  int max_keyframes, point_cap;
  uint8_t *out;                // SPFE_LOCALMAP_OUT_BYTES(n_slots, point_cap, n_kp); null in the count form
  int *votes, *total;          // [n_slots]: inside `out`, or the count form's own arrays
  uint8_t *scratch;            // localmap_scratch_bytes(n_table)
};
size_t localmap_scratch_bytes(int n_table);
int localmap_lds_point_capacity();
hipError_t launch_localmap(const LocalmapArgs &a, hipStream_t s);         // steps 1-5: seven launches
hipError_t launch_localmap_count(const LocalmapArgs &a, hipStream_t s);   // steps 1-2: three launches
hipError_t launch_localmap_rows(const int *point_idx, int point_cap, const int *list, int n_kp, int *rows, hipStream_t s);
// steps 1-2 with a keyframe row as the frame (covis.hip): n_kp up to SPFE_LOCALMAP_MAX_STRIDE, three launches
hipError_t launch_localmap_count_row(const LocalmapArgs &a, hipStream_t s);

// covis.hip — the covisibility graph (KeyFrame::UpdateConnections) on resident rows; include/spfe_covis_math.h
struct CovisArgs {
  const int *kf_mp_of_kp;      // [n_slots][kp_stride]
  int kp_stride;
  const uint8_t *kf_flags;     // [n_slots]
  const uint8_t *mp_flags;     // [n_table]
  int n_table;
  int n_slots, conn_cap, cur_slot, th, origin_slot;
  int *conn_slot, *conn_w, *conn_n, *ord_slot, *ord_w, *ord_n, *parent;   // the state
  uint8_t *first_conn;
  int *best_a, *best_b;        // [n_slots][n_best_*] or null
  int n_best_a, n_best_b;
  uint8_t *out;                // SPFE_COVIS_OUT_BYTES(n_slots, conn_cap)
  uint8_t *scratch;            // covis_scratch_bytes(n_table, n_slots)
};
size_t covis_scratch_bytes(int n_table, int n_slots);
hipError_t launch_covis(const CovisArgs &a, hipStream_t s);   // steps 1-7: five launches
hipError_t launch_covis_reset(const CovisArgs &a, int first_slot, int n, hipStream_t s);

// cull.hip — keyframe culling (the cull loop and KeyFrame::SetBadFlag) on resident rows; include/spfe_cull_math.h
struct CullArgs {
  int *kf_mp_of_kp;            // [n_slots][kp_stride]   WRITTEN
  int kp_stride;
  uint8_t *kf_flags;           // [n_slots]              WRITTEN
  uint8_t *mp_flags;           // [n_table]              WRITTEN
  int *nobs;                   // [n_table]              WRITTEN
  int n_table;
  int n_slots, conn_cap;
  int *conn_slot, *conn_w, *conn_n, *ord_slot, *ord_w, *ord_n, *parent;   // the state of CovisArgs
  int cur_slot, th_obs;
  float cov_ratio;
  int origin_slot, bad_cap;
  int *best_a;                 // [n_slots][n_best_a] or null
  int n_best_a;
  int *best_b;
  int n_best_b;
  uint8_t *out;                // SPFE_CULL_OUT_BYTES(n_slots, conn_cap, bad_cap)
  uint8_t *scratch;            // cull_scratch_bytes(n_table, n_slots, conn_cap)
};
size_t cull_scratch_bytes(int n_table, int n_slots, int conn_cap);
hipError_t launch_cull(const CullArgs &a, hipStream_t s);   // steps 1-8: four launches
hipError_t launch_count_observations(const int *rows, int kp_stride, const uint8_t *kf_flags, int n_slots, int *nobs, int n_table,
                                     hipStream_t s);         // two launches

// mpcull.hip — map-point culling with its resident state (counters, recent list, admission); include/spfe_mpcull_math.h
struct MpLife {
  uint8_t *flags;              // [n_table]
  int *nobs, *found, *visible, *first_kf;   // [n_table]
  int *recent, *recent_n;      // [recent_cap], [1]
  int n_table, recent_cap;
};
struct MpAdmitArgs {
  MpLife life;
  const uint8_t *tri;          // n_neigh blocks, tri_stride bytes apart
  size_t tri_stride;
  int kmax, n_neigh;
  const int *neigh_slot;       // [n_neigh]
  int cur_slot, cur_kf_id;
  int *rows;                   // [n_slots][kp_stride]   WRITTEN
  int kp_stride, n_slots;
  float *xyz;                  // [n_table][3]           WRITTEN
  uint8_t *out;                // SPFE_ADMIT_OUT_BYTES
  uint8_t *scratch;            // mpcull_scratch_bytes(n_table)
};
struct MpStatArgs {
  MpLife life;
  const int *entry, *after;    // [n_kp]
  int n_kp;
  const int *point_idx;        // [point_cap]
  int point_cap;
  const uint8_t *in_view;      // [point_cap]
  const uint8_t *outlier;      // [n_kp]
  uint8_t *out;                // SPFE_MPSTAT_OUT_BYTES
};
struct MpCullArgs {
  MpLife life;
  int *rows;                   // [n_slots][kp_stride]   WRITTEN
  int kp_stride, n_slots;
  const uint8_t *kf_flags;     // [n_slots]
  int cur_kf_id, th_obs;
  float found_ratio;
  int bad_cap;
  uint8_t *out;                // SPFE_MPCULL_OUT_BYTES(recent_cap, bad_cap)
  uint8_t *scratch;            // mpcull_scratch_bytes(n_table)
};
size_t mpcull_scratch_bytes(int n_table);
hipError_t launch_mp_life_reset(const MpLife &l, int first_row, int n_rows, int reset_list, hipStream_t s);   // one launch
hipError_t launch_mp_admit(const MpAdmitArgs &a, hipStream_t s);   // two launches
hipError_t launch_mp_stat(const MpStatArgs &a, hipStream_t s);     // one launch
hipError_t launch_mp_cull(const MpCullArgs &a, hipStream_t s);     // four launches

// lba.hip — the gather in front of the local bundle adjustment and the application behind it; include/spfe_lba_math.h
struct LbaGatherArgs {
  const int *ord_row;          // [conn_cap]: row cur_slot of the graph's ord_slot
  int conn_cap;
  const int *rows;             // [n_slots][kp_stride]
  int kp_stride, n_slots;
  const uint8_t *kf_flags;     // [n_slots]
  const uint8_t *mp_flags;     // [n_table]
  const float *xyz;            // [n_table][3]
  int n_table;
  const float *Tcw;            // [n_slots][16]
  int cur_slot, origin_slot, kf_cap, free_cap, point_cap, edge_cap;
  uint8_t *out;                // SPFE_LBA_GATHER_BYTES(kf_cap, point_cap, edge_cap)
  uint8_t *scratch;            // lba_gather_scratch_bytes(...)
};
struct LbaApplyArgs {
  const uint8_t *gather;       // the gather's block
  const uint8_t *ba;           // the solver's block
  int *rows;                   // [n_slots][kp_stride]   WRITTEN
  int kp_stride, n_slots;
  const uint8_t *kf_flags;     // [n_slots]
  uint8_t *mp_flags;           // [n_table]              WRITTEN, as nobs, ref_slot, xyz and Tcw
  int *nobs, *ref_slot;
  float *xyz;
  int n_table;
  float *Tcw;                  // [n_slots][16]
  int kf_cap, point_cap, edge_cap, bad_cap;
  uint8_t *out;                // SPFE_LBA_APPLY_BYTES(point_cap, edge_cap, bad_cap)
  uint8_t *scratch;            // lba_apply_scratch_bytes(point_cap, edge_cap)
};
size_t lba_gather_scratch_bytes(int n_table, int n_slots, int point_cap, int edge_cap);
size_t lba_apply_scratch_bytes(int point_cap, int edge_cap);
hipError_t launch_lba_gather(const LbaGatherArgs &a, hipStream_t s);   // ten launches
hipError_t launch_lba_apply(const LbaApplyArgs &a, hipStream_t s);     // five launches

// newkf.hip — the insertion of a new keyframe's row and the observation lists of the refreshes; include/spfe_newkf_math.h
struct NewKfArgs {
  MpLife life;                 // flags, nobs, recent and recent_n are touched
  const int *frame;            // [n_kp]
  int n_kp, cur_slot;
  int *rows;                   // [n_slots][kp_stride]   row cur_slot WRITTEN
  int kp_stride, n_slots;
  const uint8_t *kf_flags;     // [n_slots]
  const uint8_t *rec_desc;     // the record's descriptor rows, or null
  int desc_bf16;
  float *desc_track;           // [n_table][256], or null  WRITTEN
  uint8_t *out;                // SPFE_NEWKF_OUT_BYTES(n_kp, kp_stride)
  uint8_t *scratch;            // newkf_scratch_bytes(n_table)
};
struct ListObsArgs {
  const int *point_idx;        // [m], or null: first_row + i
  int first_row, m;
  const int *rows;             // [n_slots][kp_stride]
  int kp_stride, n_slots;
  const uint8_t *kf_flags;     // [n_slots]
  const int *mp_ref_slot;      // [n_table]
  int n_table, obs_cap;
  uint8_t *out;                // SPFE_LISTOBS_OUT_BYTES(m, obs_cap)
  uint8_t *scratch;            // listobs_scratch_bytes(n_table, m, obs_cap)
};
size_t newkf_scratch_bytes(int n_table);
size_t listobs_scratch_bytes(int n_table, int m, int obs_cap);
hipError_t launch_insert_keyframe(const NewKfArgs &a, hipStream_t s);      // four launches
hipError_t launch_list_observations(const ListObsArgs &a, hipStream_t s);  // six launches

// exact-math probe kernels for tests (device bits vs host bits)
hipError_t launch_math_probe(const float *in, float *out_exp, float *out_log, int n, hipStream_t s);

}  // namespace spfe
