// spfe_host.h — what the host-side translation units of libspfe.so share: the handle, the stage table, allocation and error
// helpers, and the entry points of one unit that another calls.
//   spfe_pack.hip      weight blob -> device tables, buffers, streams, events: build() (the handle's construction)
//   spfe_schedule.hip  the per-batch launch sequence: enqueue() / enqueue_post() (streams, events, ticket parity); what each
//                      convolution launch is to be, it asks conv_plan.h (plain C++, no HIP)
//   spfe_comm.hip      multi-GPU: RCCL all-gather of the records (spfe_comm_*, spfe_allgather_records)
//   spfe_widen.hip     the rows SURVEY.md §8f widens into, frame to frame: input staging, descriptor matching, patch-wise
//                      association (C ABI)
//   spfe_track.hip     the tracker's stages on resident records and their host forms: dust alignment, pose refinement,
//                      projection search, the chains TrackDust / TrackWithMotionModel / trackReferenceKeyFrameANN /
//                      TrackLocalMap, the mapper's CreateNewMapPoints and Fuse search on keyframe records, and the loop closer's
//                      candidate verification and guided match (C ABI)
//   spfe_ba.hip        bundle adjustment on keyframe records and its host form (C ABI)
//   spfe_map.hip       the map-point table: descriptor, normal and depth refreshed from keyframe records, its host form and
//                      the gather into the searches' point list (C ABI)
//   spfe_essgraph.hip  the loop closer's essential graph over Sim3, its start values and the map-point correction (C ABI)
//   spfe_loopdet.hip   the loop detection on the resident table of global descriptors (C ABI)
//   spfe_localmap.hip  the tracker's local map on resident keyframe rows: votes, expansion, ordered point list (C ABI)
//   spfe_covis.hip     the covisibility graph as resident state: KeyFrame::UpdateConnections, the preset of slots (C ABI)
//   spfe_cull.hip      keyframe culling on the resident rows and graph state, the observation counts (C ABI)
//   spfe_mpcull.hip    map-point culling and its resident state (C ABI)
//   spfe_lba.hip       the gather in front of the local bundle adjustment and the application behind it (C ABI)
//   spfe_newkf.hip     the insertion of a new keyframe's row and the observation lists of the refreshes (C ABI)
//                      (the host-array forms of these units stage through HostStage, below, on the handle's one
//                      staging buffer and pinned mirror.  The last six work on the resident map state and are written one way,
//                      one function a form that takes device addresses, fills the *Args struct and launches; the
//                      _resident entry point calls it on the caller's arrays, the twin on a HostStage whose inout() blocks go
//                      back by fetch_inouts().  Their shared range checks, misaligned() and GraphStage stand below.)
//   spfe_api.hip       the C ABI of the path itself: create / destroy / extract* / submit + collect / debug reads / timing
// One handle = one GPU, one stream, one set of buffers (SURVEY.md §8b "Threading"): the object SPExtractor's constructor
// builds (/root/reference/orb_slam2/src/cv/sp_extractor.cpp:342-359) and whose operator() (:361-514) the extract calls replace.
#pragma once
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <functional>
#include <cfloat>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/spfe.h"
#include "../../include/spfe_exact_math.h"
#include "spfe_kernels.h"
#include "conv_plan.h"

// The few RCCL types and signatures the gather needs, declared here so that building libspfe.so needs no RCCL development
// headers: librccl is dlopen'ed by spfe_comm_init (a single-GPU host never loads it).  Values as in rccl.h (NCCL 2 ABI).
extern "C" {
typedef struct ncclComm *ncclComm_t;
#define NCCL_UNIQUE_ID_BYTES 128
typedef struct { char internal[NCCL_UNIQUE_ID_BYTES]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclInt8 = 0, ncclUint8 = 1 } ncclDataType_t;
typedef ncclResult_t (*pfn_ncclGetUniqueId)(ncclUniqueId *);
typedef ncclResult_t (*pfn_ncclCommInitRank)(ncclComm_t *, int, ncclUniqueId, int);
typedef ncclResult_t (*pfn_ncclCommDestroy)(ncclComm_t);
typedef ncclResult_t (*pfn_ncclCommCount)(const ncclComm_t, int *);
typedef ncclResult_t (*pfn_ncclAllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t);
typedef const char *(*pfn_ncclGetErrorString)(ncclResult_t);
}


namespace spfe_host {

using spfe_plan::CallMode;
extern thread_local std::string g_err;
int fail(int code, const char *fmt, ...);

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return ::spfe_host::fail(SPFE_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                  __LINE__);                                                            \
  } while (0)

constexpr int NSTAGE = 15;
extern const char *const kStageNames[NSTAGE];

struct ConvLayer : spfe_plan::LayerShape {   // (the shape the planner reads: cin, ks, pool, relu, H, W = the layer's input resolution, nblk)
  int cout_real;
  float *d_w = nullptr, *d_b = nullptr;
  const float *in = nullptr;
  int in_stride = 0, in_choff = 0;
  float *out = nullptr;
  int out_stride = 0, out_choff = 0;
};

// A device buffer that only grows: reserve() below.
struct DevBuf {
  uint8_t *p = nullptr;
  size_t bytes = 0;
  template <class T>
  T *as() const { return reinterpret_cast<T *>(p); }
};

}  // namespace spfe_host
using spfe_host::ConvLayer;
using spfe_host::NSTAGE;

struct spfe_handle_s {
  spfe_config cfg{};
  int H = 0, W = 0, hc = 0, wc = 0, C = 0, kmax = 0, B = 0;
  hipStream_t stream = nullptr;
  // covariance runs on a side stream: with SPFE_FLAG_ASYNC_COV it overlaps the next
  // call's convolutions (it is latency bound and uses a handful of CUs)
  hipStream_t side = nullptr;
  static constexpr int NTICKET = 4;
  hipEvent_t ev_post[NTICKET] = {}, ev_cov[NTICKET] = {};
  hipEvent_t ev_db = nullptr;    // launch stream: this call's convDb is done (synchronous dense calls launch it behind the detector tail)
  hipEvent_t ev_desc = nullptr;  // side stream: the last call's descriptor sampling (reader of d_coarse) is done
  // f32, batches of >= 2 frames: the layers behind conv1b run as TWO half batches on two streams (SPFE_F32_SPLIT), so that the
  // workgroups of one half's kernel fill the CUs the other half's kernel leaves idle in its last, partial round of work items.
  // (Tried on top and removed: conv1a of call i + 1 on the handle's idle stream beside the later layers of call i — it fits
  // on every CU beside a convolution workgroup, but what it saves as a stage the matrix-bound kernels lose beside it: +-0.)
  // No other stream is created for the convolutions: HIP maps streams onto a few hardware queues, and ONE more stream in the
  // process moved this one onto the launch stream's queue — -4 % instead of +2 %.
  hipStream_t conv2 = nullptr;
  std::vector<hipStream_t> conv2_pool;   // candidates tried so far (kept: destroying one would reshuffle the queue mapping)
  struct Conv2Choice { hipStream_t for_stream, conv2; bool ok; };
  std::vector<Conv2Choice> conv2_known;    // per launch stream seen so far: the candidate that shares no hardware queue with it
  bool conv2_ok = false;                   // or with the side stream (ok = false: none found, no split on that stream)
  long long *probe_stamp = nullptr;        // pinned: the queue probe's device time stamps
  bool split_last = false;                 // the last call issued the layers behind conv1b as two half batches
  int split_probe = -3;                    // outcome of the last probe: 1 free queue found, 0 none, -1 not measurable, -2 stream
                                           // under capture, 2 probe switched off (first candidate trusted), -3 never probed
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // pipelined calls: the launch stream does not wait for the second stream's half batch at the end of a step — the side chain
  // does, and the launch stream only in front of the NEXT call's conv1b (its conv1a runs beside the other half's last kernels)
  bool join_pending = false;
  bool defer_join = true;   // SPFE_DEFER_JOIN=0: the join at the end of the step, on the launch stream
  int split_mode = -1;      // SPFE_SPLIT: -1 = f32 always, bf16 frames of fewer than 10,000 cells (752x480: +2 %; 1280x720: +-0); 0 never; 1 always
  // the other schedule switches (read_switches(), spfe_pack.hip; README "Environment switches"), defaults = the product's order
  bool inline_chain = true, tail_per_half = true, sel_ext_event = true, zero_in_tail = true;
  // TWO SIDE CHAINS IN FLIGHT (round 5).  The side chain of a batch is a serial string of latency-bound kernels on one stream,
  // and what it hands over internally (heat_inv, the covariance scratch, the cell lists, the coarse map) exists once — so
  // chain i + 1 starts when chain i has ended, and on large bf16 frames a chain (0.7 - 1.0 ms beside the convolutions of a
  // 1.0 ms step; its selection cannot even start before conv1b ends: LDS) is as long as the step: the side stream, not the
  // convolutions, then sets the step (1280x720 x 8: 7,530 - 8,290 frames/s depending on how many long replay chains the frames
  // hold).  With a second, complete set of buffers and a second side stream the chains of consecutive batches overlap: the
  // handle owns a TWIN — a whole second handle built from the same configuration — and pipelined device calls alternate
  // between the two (measured first with two handles in one process, tools/microbench/two_chains.py: 7,530 -> 8,115 and
  // 7,745 -> 8,125 frames/s at 1280x720 bf16; 752x480: -3 % bf16, -2 % f32: there the chain is short and a step runs as two
  // half batches).  Tickets stay one sequence: tmap says which of the two ran a ticket, and under which ticket of its own.
  // SPFE_TWO_CHAINS: -1 by workload (bf16 frames of >= 10,000 cells in short calls or beyond select_kernel: make_twin, spfe_api.hip), 0 never, 1 always.
  spfe_handle twin = nullptr;
  bool is_twin = false;
  bool twin_failed = false;                  // the twin could not be built (e.g. out of memory): one side chain, and no second attempt
  int two_chains_env = -1;
  // The parsed weight blob (register_module order), kept for as long as a twin may still be built from it: spfe_config's
  // weights / weights_path are the CALLER's memory and need not outlive spfe_create (the lazily built twin used to
  // read them again at the first spfe_submit_batch) — the stored cfg carries neither.
  std::vector<float> blob;
  long last_seq = 0;                         // value of the process-wide call counter at this handle's last enqueue_post (debug reads
                                             // of a pair come from the one that ran last)
  long g_ticket = 0;                         // tickets handed out by this handle when it has a twin
  struct TicketRef { spfe_handle who; long local; } tmap[8] = {};
  int replay_waves = 0;     // SPFE_REPLAY_WAVES: 0 = by workload
  int sparse_db_env = -1, sparse_da_env = -1, pbtail_env = 1, fuse1a_env = -1, pipe_copy_kernel = -1, cov_ecap_env = -1;
  bool desc_recorded = false;
  long ticket = 0;          // calls so far; call t uses slot t % NTICKET
  bool cov_inflight = false;
  std::vector<void *> dev_allocs;
  std::vector<void *> host_allocs;
  uint8_t *d_img = nullptr;
  float *d_w1a = nullptr, *d_b1a = nullptr;
  unsigned short *d_w1a_tab = nullptr;   // bf16 mode: conv1a's weights as the MFMA operand table of conv1a_mfma.h
  float *act[8] = {};
  float *d_head = nullptr, *d_semi = nullptr, *d_coarse = nullptr;
  unsigned short *d_hd = nullptr;    // bf16 mode: ReLU(convPa) | ReLU(convDa), [B][C][512] bf16 (input of the two bf16 heads)
  unsigned char *d_wdb = nullptr, *d_wpb = nullptr;   // bf16 mode: convDb / convPb weights, head_bf16.hip layout
  float *d_wdb32 = nullptr, *d_wpb32 = nullptr;       // f32 mode: the same for head_f32.hip (SPFE_F32_HEADS=1; default: generic kernel)
  bool f32_heads = false;
  // f32: convPb and the detector tail in one launch (pbtail_f32.hip): the two full 32-channel tiles on the MFMA, the dustbin
  // channel as the contract's fmaf chain on the VALU, the tail on the logits while they are still in LDS.  SPFE_PBTAIL=0:
  // convPb as a launch of the generic kernel + tail_kernel (same bits)
  bool pbtail = true;
  float *d_wpb_dust = nullptr;                        // convPb's row 64 (the dustbin channel), [256]
  // "sparse convDb": the descriptor head runs BEHIND the selection, on the cells some emitted keypoint's bilinear taps read
  // (<= 4 per keypoint: 28 % of a 1280x720 frame at 1000 keypoints), gathered through select_kernel's list; d_coarse keeps
  // the dense layout, only the rows anybody reads are written.  SPFE_SPARSE_DB=0: the dense head in the launch stream.
  bool sparse_db = true;
  bool sparse_db_sync_only = false;   // ... in synchronous calls only (bf16 frames below 10,000 cells; SPFE_SPARSE_DB=2)
  bool sparse_last = false;      // the last call left d_coarse sparse (spfe_debug_read("coarse") completes it on demand)
  // ... and convDa with it (bf16 mode, da_gather_bf16.hip): the dense launch computes convPa only, the descriptor branch
  // runs on the listed cells from conv4b's output on.  SPFE_SPARSE_DA=0: convPa|Da dense, only convDb gathered.
  bool sparse_da = false;
  int sparse_da_mode = 1;        // SPFE_SPARSE_DA: 0 never, 1 synchronous calls only, 2 pipelined calls too (the default of both precisions since round 5)
  bool sparse_da_call = false;   // ... this / the last call
  int *d_db_list = nullptr, *d_db_total = nullptr;
  int db_cap = 0;                // list entries per frame: min(4 kmax, C)
  int db_tiles_per_wg = 4;       // the gathered head's grid = listed tiles / this (a workgroup's weights: 128 KB)
  hipEvent_t ev_sel = nullptr;   // side stream: this call's selection (and its cell list) is done
  hipEvent_t ev_dbs[2] = {};     // by ticket parity: that call's gathered head (reader of the head activations / of conv4b's output) is done
  bool dbs_recorded[2] = {};
  // sparse_da: conv4b's output exists twice (by ticket parity), so that the NEXT call's conv4b does not wait for this
  // call's gathered convDa, which runs behind the selection on the side stream
  float *act7_alt = nullptr;
  float *d_wda32 = nullptr;          // f32 mode: convDa's weights in da_gather_f32.hip's order
  const float *feat_cur = nullptr;   // conv4b's output of the call being enqueued / of the last call
  // what the detector tail (launch stream) hands to the side chain exists twice, by ticket parity: batch i + 1's tail then
  // only has to wait for batch i - 1's side chain, not for batch i's (which runs beside batch i + 1's convolutions)
  float *d_heat_log[2] = {}, *d_heat = nullptr, *d_heat_inv = nullptr;
  float *d_minmax[2] = {}, *d_cell_score[2] = {}, *d_heat_consts = nullptr;
  uint8_t *d_cell_k[2] = {}, *d_cell_mask = nullptr;
  const uint8_t *rec_of[NTICKET] = {};   // record buffer of each ticket (same buffer twice in a row: the old ordering)
  int *d_kp_cell = nullptr;
  // (select_kernel's 2-bytes-a-cell LDS form is for frames above 16,384 cells only.  Forced onto smaller frames in pipelined
  // calls it starts beside a convolution workgroup instead of waiting for a free CU, and that measured as NOT a gain — f32
  // 752x480 2107 / 2116 -> 2085 / 2082 frames/s, conv1b 0.87 -> 0.83 of peak: HISTORY.md "Round 4" — the switch is gone)
  int *d_sel_slot = nullptr;          // frames of more than 16,384 cells: select_kernel's global scratch (tail_select.hip)
  uint16_t *d_sel_list = nullptr;
  // frames of more than 65,535 cells (3840x2160), or SPFE_SELECT_HUGE=1: select_huge_kernel, everything per cell in global scratch
  bool select_huge = false;
  int select_huge_env = 0;
  uint8_t *d_sel_state = nullptr;
  int *d_sel_list32 = nullptr;
  uint8_t *d_records = nullptr;
  spfe::CovScratch cov{};
  int cov_gen_code = 0;        // generation code of the last chain (CovScratch::gen = code << 16); 0: none yet
  int cov_gen_start = 32766;   // SPFE_COV_CAPS field 6 (tests reach the wrap)
  int cov_frames_clean = 0;    // leading frames whose claim / done maps hold tagged (or reset) entries
  int cov_captured_min = 0;    // lowest generation code a captured (hipGraph) call froze; 0: never captured (enqueue_post)
  ConvLayer layers[10];
  spfe_plan::Switches plan_sw{};   // the switches and capabilities above as the planner reads them (conv_plan.h), filled at the end of build()
  spfe::RecordLayout rl{};
  // host side
  uint8_t *h_img = nullptr, *h_records = nullptr;
  float *h_heat = nullptr, *h_heat_inv = nullptr;
  float *own_heat = nullptr, *own_heat_inv = nullptr;   // spfe_set_map_buffers: the library's buffers while h_heat / h_heat_inv
  float *usr_heat = nullptr, *usr_heat_inv = nullptr;   // point at the caller's (registered) memory
  int last_n = 0;
  int host_sync_n = 0;   // frames of the last synchronous host call (spfe_fetch_heat_inv)
  // Synchronous host calls with SPFE_FLAG_HEAT (the drop-in's operator(): Frame clones heat_, frame.cpp:304): the heat maps are
  // final when the heat normalisation ends — ~150 us before a single frame's record is (selection + covariance behind it) — so
  // their D2H (2 x 4 H W bytes: 2.9 MB at 752x480, ~100 us of PCIe) starts THERE, on a copy stream of its own behind the
  // normalisation's completion signal, and runs beside the chain instead of behind it (round 6; SPFE_EARLY_HEAT_COPY=0: behind
  // the record's copy, as before).
  hipStream_t s_heat = nullptr;
  hipEvent_t ev_heat = nullptr, ev_heat_copied1 = nullptr, ev_heat_copied = nullptr;   // normalisation done / heat in host memory / both maps
  bool early_heat_copy = true;   // SPFE_EARLY_HEAT_COPY
  int open_n = 0;                // frames of a call begun by spfe_extract_begin and not yet finished
  bool host_sync_call = false;   // set by the synchronous host entry points around enqueue()
  bool heat_early = false;       // this call's maps were sent ahead: finish_host waits for ev_heat_copied instead of copying
  // ... and the descriptor rows of the record (kmax x 256 floats: 1.0 of a 752x480 record's 1.1 MB) leave right behind the
  // descriptor sampling, on the side stream that ran it, beside the covariance replay (the chain's longest kernel) instead of
  // behind it; finish_host then copies the record's two small ends only.  Inline-chain calls (a synchronous call with the
  // gathered descriptor branch: the single-frame operator()); same switch.
  bool desc_early = false;
  int num_cus = 256;
  // input staging (spfe_set_staging)
  spfe_staging st{};
  bool st_set = false;
  float *d_map_x = nullptr, *d_map_y = nullptr;
  uint8_t *d_raw = nullptr, *h_raw = nullptr;
  std::vector<spfe_host::DevBuf *> grown;   // the DevBufs below that hold memory (reserve(); freed by spfe_destroy)
  // The host-array forms (HostStage below): every one of them stages its arrays in `stage` and reads results back through
  // `stage_host` (pinned, contents not kept on growth, freed by spfe_destroy).  They are synchronous and a handle is one
  // thread's, so no two of them use the pair at once.
  spfe_host::DevBuf stage;
  uint8_t *stage_host = nullptr;
  size_t stage_host_bytes = 0;
  // descriptor matching (spfe_match*): scratch grown on demand; m_out* are the host forms' outputs
  spfe_host::DevBuf m_best_t, m_best_q, m_out, m_out2;
  int m_pairs = 0, m_cap = 0;      // capacity of m_best_* ([pairs][cap])
  int *p_cidx = nullptr;           // patch association scratch: [4096][4] candidates, distances
  float *p_cdist = nullptr;
  unsigned tile2_mask = 0;   // SPFE_TILE2_MASK > 0: f32 layers forced onto 2-row tiles
  bool tile2_auto = true;    // SPFE_TILE2_MASK=0: never choose 2-row tiles
  // f32, a single frame: a POOLED low-resolution layer (conv3b: 180 eight-row items on 256 CUs — one round of the longest
  // items, 70 % of the CUs busy) as UN-pooled 2-row tiles (720 items: three rounds of quarter-size items) into a scratch
  // buffer + a 2x2 max-pool pass (pool2x2_f32_kernel; bias / ReLU / max commute exactly: same bits).  SPFE_POOL_SPLIT:
  // -1 cost model, 0 never, 1 wherever the shapes allow (tests)
  int pool_split = -1;
  float *d_unpooled = nullptr;   // [<= 2 frames][H / 4][W / 4][128]
  int conv1b_split_rows = -1; // ... and, when that launch was cut in a 16-row and an 8-row part, the 16-row part's tile rows ("conv1b_split_rows")
  int conv1b_tile_rows = 8;  // rows per tile of the last call's conv1b launch (f32; spfe_debug_read("conv1b_tile_rows"))
  int tile16x4 = 1;          // SPFE_TILE16X4: conv1b on 16-row tiles of 4 wavefronts x 4 rows (0 never, 1 by the cost model — possibly
                             // cut in a 16-row and an 8-row launch —, 2 always in one launch, 3 cost model without the cut)
  bool fuse1a = false;  // f32: conv1a computed inside conv1b in every call (SPFE_FUSE_CONV1A=1; perf-neutral on batches); unset: single-frame synchronous calls only
  bool fuse1a_bf16 = true;  // bf16: conv1a computed by the producer waves of the wave-specialised conv1b (SPFE_FUSE_CONV1A=0 to split)
  int *pose_map = nullptr;           // spfe_track_dust_refine_record_device: map point per keypoint [kmax] (device)
  // window search by projection (spfe_search_projection*): candidate lists of the map points of a call (all its frames),
  // grown on demand
  spfe_host::DevBuf pj_ck, pj_cn, pj_cd, pj_cq, pj_held;
  int *tri_next = nullptr;           // spfe_create_map_points*: the id of the next new map point (device)
  spfe_host::DevBuf s3_scratch;      // spfe_sim3_* / spfe_loop_verify_*: the pair lists of a call's candidates (device)
  spfe_host::DevBuf gd_scratch;      // spfe_search_by_sim3* / spfe_loop_guided_match_*: seed, transform and mask of a call's jobs (device)
  spfe_host::DevBuf so_scratch;      // spfe_optimize_sim3* / spfe_loop_optimize_sim3_*: the edge data of a call's jobs (device)
  spfe_host::DevBuf ba_scratch;      // spfe_bundle_adjust / spfe_local_ba_records_device: per-point and per-edge arrays, the reduced system (device)
  // pipelined host path (spfe_submit_batch / spfe_collect_batch): NPIPE batches in flight, each with its own
  // pinned input / output staging and device frame / record buffers; H2D and D2H on copy streams
  static constexpr int NPIPE = 3;
  struct PipeSlot {
    uint8_t *h_img = nullptr, *d_img = nullptr, *d_rec = nullptr, *h_rec = nullptr;
    float *h_heat = nullptr, *h_heat_inv = nullptr;
    hipEvent_t ev_h2d = nullptr, ev_done = nullptr;
    long ticket = -1;   // records ticket of the batch in this slot, -1 = free
    int n = 0;
    spfe_handle who = nullptr;   // which of a twin pair ran the batch (its heat maps, its side stream)
  } pipe[NPIPE];
  bool pipe_ready = false, pipe_mode = false;
  hipStream_t s_h2d = nullptr, s_d2h = nullptr;
  long pipe_submitted = 0;
  // RCCL all-gather of the records (spfe_comm_init / spfe_allgather_records): librccl is loaded on demand
  void *rccl_lib = nullptr;
  ncclComm_t comm = nullptr;
  int comm_rank = 0, comm_world = 0;
  hipStream_t comm_stream = nullptr;   // the stream of the collective: the side stream (default) or one of its own
  bool comm_own_stream = false;        // SPFE_COMM_OWN_STREAM=1
  hipEvent_t ev_gather = nullptr;      // the last gather on comm_stream is done
  bool gather_recorded = false;
  pfn_ncclCommInitRank p_ncclCommInitRank = nullptr;
  pfn_ncclCommDestroy p_ncclCommDestroy = nullptr;
  pfn_ncclCommCount p_ncclCommCount = nullptr;
  pfn_ncclAllGather p_ncclAllGather = nullptr;
  pfn_ncclGetErrorString p_ncclGetErrorString = nullptr;
  unsigned ws_mask = 15u;   // bf16 layers (bit i = conv layer i of enqueue(), Cin = 64 only) that may use the wave-specialised kernel
  // (measured and not kept: conv1b / all Cin = 64 layers on fewer workgroups than CUs in pipelined calls, so that the
  // previous batch's selection — 143 KB of LDS, nothing fits beside this kernel's 158 KB — starts beside conv1b: 1280x720
  // x 8 on 224 workgroups +0.3 ... 2 % with conv1b at 0.51 - 0.53 of peak instead of 0.57; 248 / 240 / 208 / 192: -1 / -2
  // / -1 / -3 %.  HISTORY.md "Round 4"; re-measured in round 5)
  int ws_min_items = 11;    // ... when the launch has at least this many (tile, 64-channel block) items per workgroup (pipelined calls)
  int ws_min_items_sync = 5;   // ... the same for synchronous calls
  unsigned char *d_wws[4] = {};  // their weights in conv_bf16_ws.hip's layout
  unsigned char *d_wrw[4] = {};  // bf16 Cin = 128 layers (conv3b, 4a, 4b, Pa|Da): weights in conv_bf16_rw.hip's fragment order
  bool bf16_rw = true;           // SPFE_BF16_RW: register-resident-weights kernel for those layers
  int rw_rows3 = 1;              // SPFE_BF16_RW_ROWS3
  int rw_min4 = 3, rw_min2 = 2;  // ... 4-row tiles from this many tiles per workgroup, 2-row tiles from this many, else conv_bf16.hip
  bool bf16_dyn = true;          // SPFE_BF16_DYN_QUEUE
  int tile16_min_items = 3;      // SPFE_BF16_TILE16_MIN_ITEMS (0 = 8-row tiles only)
  int tile_rows_big = 12;        // SPFE_BF16_TILE_ROWS (12 | 16)
  int *d_tile_ctr = nullptr;     // [8 layers][16] tile-queue counters, zero at the start of every enqueue(): cleared by the previous
                                 // call's detector tail (a launch of its own cost 9 us between two 1 ms steps), or by a launch when that did not happen
  bool tile_ctr_clean = false;
  bool act0_missing = false;  // the last call computed conv1a inside conv1b
  bool bf16 = false;  // SPFE_PRECISION_BF16: all twelve convolutions (1x1 heads included) as bf16 GEMMs with f32 accumulation; f32 tail
  // per-stage timing: a ring of event sets, one set per enqueue() call
  bool timing = false;
  bool timing_all = true;  // false (SPFE_STAGE_TIMING=2): events around the dominant kernel (conv1b) only
  static constexpr int EVSETS = 128;
  std::vector<hipEvent_t> evpool;  // [EVSETS][NSTAGE + 1]
  long calls = 0, calls_at_reset = 0;
  hipEvent_t *ev = nullptr;        // set used by the current call
  spfe_host::DevBuf eg_scratch;      // spfe_optimize_essential_graph*: per-edge and per-keyframe arrays, the envelope twice (device)
  spfe_host::DevBuf lm_scratch;      // spfe_update_local_map_resident / spfe_count_shared_points_resident: the weight table, count and key per point;
                                     // spfe_update_connections_resident: votes and total per slot in front of them (device)
  spfe_host::DevBuf ck_scratch;      // spfe_cull_keyframes_resident: first entry per point, the first pass's counts, children, marks (device)
  spfe_host::DevBuf mc_scratch;      // spfe_cull_map_points_resident / spfe_admit_map_points_resident: first entry and mark per point, the admission's verdict (device)
  spfe_host::DevBuf nk_scratch;      // spfe_insert_keyframe_resident: first keypoint per point; spfe_list_observations_resident: first entry per point,
                                     // counts per entry, the hit list, the placed keys (device)
  spfe_host::DevBuf lb_scratch;      // spfe_gather_local_ba_resident / spfe_apply_local_ba_resident: keys and ranks per point, slot tables, the hit list, marks (device)
};

namespace spfe_host {

template <class T>
int dev_alloc(spfe_handle h, T **p, size_t count) {
  void *q = nullptr;
  HIP_TRY(hipMalloc(&q, count * sizeof(T) + 256));
  h->dev_allocs.push_back(q);
  *p = reinterpret_cast<T *>(q);
  return SPFE_OK;
}
template <class T>
int host_alloc(spfe_handle h, T **p, size_t count) {
  void *q = nullptr;
  HIP_TRY(hipHostMalloc(&q, count * sizeof(T) + 256, hipHostMallocDefault));
  h->host_allocs.push_back(q);
  *p = reinterpret_cast<T *>(q);
  return SPFE_OK;
}

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Grows `b` to at least `bytes` (the old contents are not kept): nothing may still read the old block when it is freed.
inline int reserve(spfe_handle h, DevBuf &b, size_t bytes) {
  if (bytes <= b.bytes) return SPFE_OK;
  HIP_TRY(hipDeviceSynchronize());
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.bytes = 0;
  if (std::find(h->grown.begin(), h->grown.end(), &b) == h->grown.end()) h->grown.push_back(&b);
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&b.p), bytes));
  b.bytes = bytes;
  return SPFE_OK;
}

// The staging of one host-array form, on the handle's one staging buffer and pinned mirror.  The form declares its blocks in
// layout order, commit() reserves the buffer and issues the presets and uploads on h->stream, the kernels run on dev<T>(block),
// results leave through fetch() (the pinned mirror: host<T>(block) after sync()), fetch_to() or, for the inout() blocks,
// fetch_inouts() (straight into the caller's memory), and sync() ends the call.  The object lives until then: inputs passed by
// value are uploaded from inside it.
class HostStage {
 public:
  explicit HostStage(spfe_handle h) : h_(h) {}
  HostStage(const HostStage &) = delete;
  // An input block of `cap` bytes: `bytes` of `src` are uploaded (nothing when src is null or bytes is 0); fill_ff: the whole
  // capacity is set to 0xFF first (index arrays: -1 in the rows beyond those given).  -> the block
  int in(const void *src, size_t bytes, size_t cap, size_t align, bool fill_ff = false) {
    Blk b{};
    b.src = src; b.bytes = src ? bytes : 0; b.cap = cap; b.off = align_up(end_, align); b.ff = fill_ff;
    end_ = b.off + cap;
    blk_.push_back(b);
    return (int)blk_.size() - 1;
  }
  // A small input by value (a header, a flag), kept in this object
  template <class T>
  int value(const T &v, size_t align) {
    static_assert(sizeof(T) <= sizeof(Blk::val), "HostStage::value holds 16 bytes");
    const int b = in(nullptr, 0, sizeof(T), align);
    memcpy(blk_[b].val, &v, sizeof(T));
    blk_[b].bytes = sizeof(T);
    return b;
  }
  // An output block; preset: the caller's block, uploaded first, so that what the kernels do not write stays the caller's
  int out(size_t cap, const void *preset = nullptr, size_t align = 256) { return in(preset, cap, cap, align); }
  // An array the call updates in place: the caller's `bytes` uploaded into a 16-byte aligned block of at least 16 bytes, and
  // copied straight back into the caller's memory by fetch_inouts().  A null `host` uploads and fetches nothing and takes 16 bytes.
  int inout(void *host, size_t bytes) {
    const int b = in(host, bytes, std::max(host ? bytes : 0, (size_t)16), 16);
    blk_[b].back = host;
    return b;
  }
  void pad(size_t align) { end_ = align_up(end_, align); }   // the next block starts a unit of this alignment
  int commit() {
    int rc = reserve(h_, h_->stage, end_);
    if (rc) return rc;
    for (const Blk &b : blk_) {
      if (b.ff) HIP_TRY(hipMemsetAsync(h_->stage.p + b.off, 0xff, b.cap, h_->stream));
      if (b.bytes) HIP_TRY(hipMemcpyAsync(h_->stage.p + b.off, b.src ? b.src : b.val, b.bytes, hipMemcpyHostToDevice, h_->stream));
    }
    return SPFE_OK;
  }
  uint8_t *base() const { return h_->stage.p; }
  size_t off(int b) const { return blk_[b].off; }
  template <class T>
  T *dev(int b) const { return reinterpret_cast<T *>(h_->stage.p + blk_[b].off); }
  template <class T>
  T *dev_if_given(int b) const { return blk_[b].src ? dev<T>(b) : nullptr; }   // null where the caller gave no array
  void fetch(int b, size_t bytes) { blk_[b].fetch = bytes; }
  int fetch_to(void *dst, const void *d_src, size_t bytes) {
    if (bytes) HIP_TRY(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, h_->stream));
    return SPFE_OK;
  }
  int fetch_inouts() {   // behind the launches, in front of sync()
    for (const Blk &b : blk_)
      if (b.back && b.bytes) HIP_TRY(hipMemcpyAsync(b.back, h_->stage.p + b.off, b.bytes, hipMemcpyDeviceToHost, h_->stream));
    return SPFE_OK;
  }
  // The mirror is sized here, where every fetch of the call is known, so that growing it cannot pull it from under a copy.
  int sync() {
    size_t need = 0;
    for (Blk &b : blk_)
      if (b.fetch) { b.moff = need; need = align_up(need + b.fetch, 16); }
    if (need > h_->stage_host_bytes) {
      if (h_->stage_host) (void)hipHostFree(h_->stage_host);
      h_->stage_host = nullptr;
      h_->stage_host_bytes = 0;
      HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&h_->stage_host), need, hipHostMallocDefault));
      h_->stage_host_bytes = need;
    }
    for (const Blk &b : blk_)
      if (b.fetch) HIP_TRY(hipMemcpyAsync(h_->stage_host + b.moff, h_->stage.p + b.off, b.fetch, hipMemcpyDeviceToHost, h_->stream));
    HIP_TRY(hipStreamSynchronize(h_->stream));
    return SPFE_OK;
  }
  template <class T>
  const T *host(int b) const { return reinterpret_cast<const T *>(h_->stage_host + blk_[b].moff); }

 private:
  struct Blk {
    const void *src;
    void *back;   // inout(): where fetch_inouts() copies the block
    size_t bytes, cap, off, fetch, moff;
    bool ff;
    uint8_t val[16];
  };
  spfe_handle h_;
  size_t end_ = 0;
  std::vector<Blk> blk_;
};

// the stream argument of the device entry points: NULL = the handle's own
inline hipStream_t stream_of(spfe_handle h, void *stream) { return stream ? reinterpret_cast<hipStream_t>(stream) : h->stream; }

// One record resident in HBM (or the first of an array of records), by the handle's layout.
struct RecordView {
  const uint8_t *base;
  const spfe::RecordLayout &rl;
  RecordView(spfe_handle h, const void *d_record) : base(reinterpret_cast<const uint8_t *>(d_record)), rl(h->rl) {}
  template <class T>
  const T *at(size_t off) const { return reinterpret_cast<const T *>(base + off); }
  const int *hdr() const { return at<int>(rl.off_hdr); }
  const float *xy() const { return at<float>(rl.off_xy); }
  const float *cinv() const { return at<float>(rl.off_cinv); }
  const float *desc() const { return at<float>(rl.off_desc); }   // bf16 rows when desc_bf16()
  int desc_bf16() const { return rl.desc_bf16; }
  const int16_t *occ() const { return at<int16_t>(rl.off_occ); }
  const float *dense_dust() const { return at<float>(rl.off_dd); }
};

// tickets as the caller of the C ABI sees them (one sequence per handle, twin or not)
inline long api_tickets(const spfe_handle h) { return h->twin ? h->g_ticket : h->ticket; }
inline spfe_handle_s::TicketRef ticket_ref(spfe_handle h, long t) {
  if (!h->twin) return {h, t};
  return h->tmap[t % 8];
}
inline spfe_handle last_caller(spfe_handle h) {   // the one of the pair whose buffers hold the last call's intermediates
  return h->twin && h->twin->last_seq > h->last_seq ? h->twin : h;
}

hipError_t wait_if_pending(hipStream_t s, hipEvent_t ev);
void make_layout(int kmax, int C, bool desc_bf16, spfe::RecordLayout *r);
// spfe_pack.hip
// (sibling: the handle whose twin `h` is to be — weights and environment switches are taken from it, not from the caller's
// pointers or the environment of that later moment)
int build(spfe_handle h, const spfe_config *cfg, spfe_handle sibling = nullptr);
// spfe_schedule.hip
int enqueue(spfe_handle h, const uint8_t *d_images, int n, uint8_t *d_records, hipStream_t s);
CallMode call_mode(const spfe_handle_s *h, int n);
int enqueue_post(spfe_handle h, const CallMode &m, uint8_t *d_records, hipStream_t s, const std::function<int()> *conv_db = nullptr, bool sparse = false, bool fused_pb = false, bool tail_done = false);
spfe::FrameBufs frame_bufs(spfe_handle h, uint8_t *d_records, bool sparse);
int tail_waits(spfe_handle h, uint8_t *d_records, hipStream_t s);
int launch_db_gathered(spfe_handle h, int n, hipStream_t s);
int launch_db_dense(spfe_handle h, int n, hipStream_t s);
int settle_join(spfe_handle h, hipStream_t s);
// spfe_widen.hip: the patch-wise association against a record, for the tracker's chain (spfe_track.hip)
int patch_scratch(spfe_handle h);
int patch_check(int kcap);   // SPFE_EINVAL for more keypoints than the patch association's claim stage holds in LDS
spfe::PatchArgs patch_args(spfe_handle h, const RecordView &rec, const void *d_mp_desc, const void *d_mp_uv, int n_points);
// ... and the descriptor matching of records (spfe_match_records_device), for the reference-keyframe chain: the [pairs][cap]
// scratch of launch_match, and `d_records` as one of its sides
int match_scratch(spfe_handle h, int pairs, int cap);
spfe::MatchSide record_side(spfe_handle h, const void *d_records);
// ---- the units on resident map state (spfe_localmap / covis / cull / mpcull / lba / newkf.hip) ------------------------------------------
inline bool misaligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
// the range checks they share, each with the one message of its range
inline int n_slots_check(int n_slots) {
  if (n_slots < 1 || n_slots > SPFE_LOCALMAP_MAX_KEYFRAMES)
    return fail(SPFE_EINVAL, "n_slots %d not in [1, %d]", n_slots, SPFE_LOCALMAP_MAX_KEYFRAMES);
  return SPFE_OK;
}
inline int kp_stride_check(int kp_stride) {
  if (kp_stride < 1 || kp_stride > SPFE_LOCALMAP_MAX_STRIDE)
    return fail(SPFE_EINVAL, "kp_stride %d not in [1, %d]", kp_stride, SPFE_LOCALMAP_MAX_STRIDE);
  return SPFE_OK;
}
inline int n_table_check(int n_table, int least) {   // least: 0 where a call on an empty table is served, else 1
  if (n_table < least || n_table > SPFE_MP_MAX_POINTS) return fail(SPFE_EINVAL, "n_table %d not in [%d, %d]", n_table, least, SPFE_MP_MAX_POINTS);
  return SPFE_OK;
}
inline int rows_check(int kp_stride, int n_slots) {
  const int rc = n_slots_check(n_slots);
  return rc ? rc : kp_stride_check(kp_stride);
}
inline int n_best_check(int n_best_a, int n_best_b) {
  if (n_best_a < 1 || n_best_a > SPFE_LOCALMAP_MAX_BEST || n_best_b < 1 || n_best_b > SPFE_LOCALMAP_MAX_BEST)
    return fail(SPFE_EINVAL, "n_best %d / %d not in [1, %d]", n_best_a, n_best_b, SPFE_LOCALMAP_MAX_BEST);
  return SPFE_OK;
}
// spfe_covis.hip: the checks and the kernel view of a spfe_covis_graph, for the culling as well (spfe_cull.hip)
int covis_graph_check(const spfe_covis_graph *g);
spfe::CovisArgs covis_state(const spfe_covis_graph *g);
// A spfe_covis_graph of host arrays staged for a host-array form: uploaded, updated in place, fetched whole by fetch_inouts().
// first_conn is staged only where the form writes it; device() is the graph of the staged blocks, behind commit().
struct GraphStage {
  int blk[8] = {};
  bool with_first;
  GraphStage(HostStage &st, const spfe_covis_graph *g, bool first_conn) : with_first(first_conn) {
    const size_t n = (size_t)g->n_slots, row_b = n * g->conn_cap * 4;
    void *const host[8] = {g->d_conn_slot, g->d_conn_w, g->d_conn_n, g->d_ord_slot, g->d_ord_w, g->d_ord_n, g->d_parent, g->d_first_conn};
    const size_t bytes[8] = {row_b, row_b, n * 4, row_b, row_b, n * 4, n * 4, n};
    for (int i = 0; i < (with_first ? 8 : 7); ++i) blk[i] = st.inout(host[i], bytes[i]);
  }
  spfe_covis_graph device(const HostStage &st, const spfe_covis_graph *g) const {
    spfe_covis_graph d = *g;
    d.d_conn_slot = st.dev<void>(blk[0]); d.d_conn_w = st.dev<void>(blk[1]); d.d_conn_n = st.dev<void>(blk[2]);
    d.d_ord_slot = st.dev<void>(blk[3]); d.d_ord_w = st.dev<void>(blk[4]); d.d_ord_n = st.dev<void>(blk[5]);
    d.d_parent = st.dev<void>(blk[6]);
    if (with_first) d.d_first_conn = st.dev<void>(blk[7]);
    return d;
  }
};
// spfe_mp_life (spfe_mpcull.hip, spfe_newkf.hip): which of the state's arrays a form touches, the checks, the kernel view
enum : unsigned { L_FLAGS = 1, L_NOBS = 2, L_FOUND = 4, L_VISIBLE = 8, L_FIRST = 16, L_LIST = 32, L_ALL = 63 };

inline int life_check(const spfe_mp_life *l, unsigned need) {
  int rc = n_table_check(l->n_table, 1);
  if (rc) return rc;
  if (l->recent_cap < 1 || l->recent_cap > SPFE_MP_MAX_POINTS)
    return fail(SPFE_EINVAL, "recent_cap %d not in [1, %d]", l->recent_cap, SPFE_MP_MAX_POINTS);
  if (((need & L_FLAGS) && !l->d_mp_flags) || ((need & L_NOBS) && !l->d_mp_nobs) || ((need & L_FOUND) && !l->d_mp_found) ||
      ((need & L_VISIBLE) && !l->d_mp_visible) || ((need & L_FIRST) && !l->d_mp_first_kf) || ((need & L_LIST) && (!l->d_recent || !l->d_recent_n)))
    return fail(SPFE_EINVAL, "null array in spfe_mp_life");
  if (misaligned(l->d_mp_nobs, 4) || misaligned(l->d_mp_found, 4) || misaligned(l->d_mp_visible, 4) || misaligned(l->d_mp_first_kf, 4) ||
      misaligned(l->d_recent, 4) || misaligned(l->d_recent_n, 4))
    return fail(SPFE_EINVAL, "alignment: the int32 arrays of spfe_mp_life 4 bytes");
  return SPFE_OK;
}

inline spfe::MpLife life_view(const spfe_mp_life *l) {
  spfe::MpLife v{};
  v.flags = reinterpret_cast<uint8_t *>(l->d_mp_flags);
  v.nobs = reinterpret_cast<int *>(l->d_mp_nobs);
  v.found = reinterpret_cast<int *>(l->d_mp_found);
  v.visible = reinterpret_cast<int *>(l->d_mp_visible);
  v.first_kf = reinterpret_cast<int *>(l->d_mp_first_kf);
  v.recent = reinterpret_cast<int *>(l->d_recent);
  v.recent_n = reinterpret_cast<int *>(l->d_recent_n);
  v.n_table = l->n_table;
  v.recent_cap = l->recent_cap;
  return v;
}
// the state's arrays staged for a host-array form: uploaded, updated in place, fetched whole by fetch_inouts()
struct LifeStage {
  int blk[7];
  LifeStage(HostStage &st, const spfe_mp_life *l) {
    const size_t nt = (size_t)l->n_table;
    void *const host[7] = {l->d_mp_flags, l->d_mp_nobs, l->d_mp_found, l->d_mp_visible, l->d_mp_first_kf, l->d_recent, l->d_recent_n};
    const size_t bytes[7] = {nt, nt * 4, nt * 4, nt * 4, nt * 4, (size_t)l->recent_cap * 4, 4};
    for (int i = 0; i < 7; ++i) blk[i] = st.inout(host[i], bytes[i]);
  }
  spfe_mp_life device(const HostStage &st, const spfe_mp_life *l) const {
    spfe_mp_life d = *l;
    d.d_mp_flags = st.dev<void>(blk[0]); d.d_mp_nobs = st.dev<void>(blk[1]); d.d_mp_found = st.dev<void>(blk[2]);
    d.d_mp_visible = st.dev<void>(blk[3]); d.d_mp_first_kf = st.dev<void>(blk[4]); d.d_recent = st.dev<void>(blk[5]);
    d.d_recent_n = st.dev<void>(blk[6]);
    return d;
  }
};
// spfe_api.hip
void view_record(const spfe_handle h, const uint8_t *rec, const float *heat, const float *heat_inv, spfe_result *out);

}  // namespace spfe_host

// spfe_api.hip: D2H of the last synchronous batch's records (+ heat maps) and the result views (not exported: hidden visibility)
extern "C" int finish_host(spfe_handle h, int n, spfe_result *outs);

namespace spfe {
__global__ void copy_records_kernel(uint4 *dst, const uint4 *src, size_t n16);
}
