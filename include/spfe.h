/*
 * spfe.h — C ABI of libspfe.so, the MI355X-native SuperPoint feature front-end.
 *
 * Drop-in boundary for ONE path of HyHuang1995/sp_orb_slam: the extractor call
 *     (*mpORBextractorLeft)(im, cv::Mat(), mvKeys, mDescriptors)
 * (orb_slam2/src/type/frame.cpp:296-314), i.e. SPExtractor::operator()
 * (orb_slam2/src/cv/sp_extractor.cpp:361-514) and everything below it
 * (SPFrontend::forward :79-159, nms :161-250, computeCovariance :252-340).
 * Plain pointers and sizes only: no torch, OpenCV or Eigen types.  The C++
 * adaptor that restores the BaseExtractor signature
 * (include/orb_slam/cv/base_extractor.h:54-56) is include/spfe_extractor.hpp;
 * INTEGRATION.md shows the reference-side change.
 *
 * All functions return SPFE_OK (0) or a negative SPFE_E* code; the message for
 * the last failure on the calling thread is spfe_last_error().
 *
 * Threads.  A handle is one host thread's at a time: it is one stream, one set of buffers and scratch, one staging buffer
 * and pinned mirror, and the library takes no lock around them — calls on one handle are serialised by the caller.  A handle
 * with a twin (SPFE_FLAG_ASYNC_COV, two side chains) is one such unit: the pair belongs to one thread.  Distinct handles are
 * independent and may be used at the same moment from distinct threads (the reference's tracking, local-mapping and
 * loop-closing threads each own theirs), on one device or on several; a handle may be created in one thread and driven from
 * another, as long as the calls do not overlap.
 * spfe_last_error() is per thread (thread-local text): a thread reads the message of ITS last failing call, whatever other
 * threads were refused meanwhile.
 * Process-wide, and safe to reach from any number of threads: the HIP runtime itself; the once-per-kernel raising of the
 * dynamic-LDS limit on a launcher's first use per device (atomic flags, csrc/spfe_kernels.h); the call counter whose stamps
 * tell which of a twin pair ran last (atomic); the environment switches, which are only ever read — the schedule switches
 * when a handle is created (spfe_create; the twin takes its sibling's), SPFE_COMM_OWN_STREAM at every spfe_comm_init.
 * Nothing else is shared between handles.
 * Current device: HIP's current device is per-thread state, so every entry point that touches the device begins with
 * hipSetDevice(cfg.device) and does not put the previous one back: such a call — spfe_create and spfe_destroy included —
 * leaves the CALLING thread's current HIP device at the handle's device.  Calls that are refused on their arguments before
 * that point, and the pure getters (spfe_last_error, spfe_record_bytes, ...), leave it alone.  A caller that allocates on
 * "the current device" behind a library call allocates on the handle's.  (tests/test_gpu_threads.py holds the library to
 * all of this.)
 */
#ifndef SPFE_H
#define SPFE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define SPFE_API __attribute__((visibility("default")))
#else
#define SPFE_API
#endif

#define SPFE_OK 0
#define SPFE_EINVAL (-1)   /* bad argument / size not a multiple of 8 / wrong batch */
#define SPFE_EEMPTY (-2)   /* null or empty image: sp_extractor.cpp:364-365 throws here */
#define SPFE_EHIP (-3)     /* HIP runtime error (no GPU, OOM, launch failure) */
#define SPFE_EWEIGHTS (-4) /* weight blob/file missing or malformed */

/* spfe_config.precision */
#define SPFE_PRECISION_F32 0  /* exact f32 on v_mfma_f32_32x32x2_f32; bit-identical to the CPU oracle */
#define SPFE_PRECISION_BF16 1 /* ALL twelve convolutions — conv1a..conv4b, convPa / convDa and both 1x1 heads convPb /
                                 convDb — on v_mfma_f32_32x32x16_bf16: bf16 activations and weights, f32 accumulate /
                                 bias / ReLU / pool.  The heads read the bf16 ReLU(convPa) / ReLU(convDa) buffer and
                                 write f32 logits / coarse descriptors, so the detector logits carry bf16 rounding.
                                 Softmax, NMS, descriptor sampling, heat and covariance stay f32 (BASELINE configs[3]:
                                 "bf16 conv path with fp32 NMS"): everything behind the logits is bit-exact GIVEN the
                                 logits.  Keypoints / descriptors match the f32 path within tolerance, not bitwise
                                 (keypoint-set Jaccard ~0.93, descriptor cosine >= 0.9999 at 1280x720). */

/* spfe_config.flags */
#define SPFE_FLAG_HEAT 1u /* also produce heat / heat_inv (H*W floats each), sp_extractor.cpp:461-474 */
#define SPFE_FLAG_ASYNC_COV 2u /* spfe_extract_batch_device only: the covariance stage (cov2, cov2_inv, status of
                                  the records) runs on a library-owned side stream and is NOT ordered into the
                                  caller's stream by the call; order it with spfe_wait_records(ticket) before
                                  reading the records.  Lets the latency-bound covariance of batch i overlap the
                                  convolutions of batch i+1.  Pass a different record buffer to consecutive calls. */

#define SPFE_FLAG_DESC_BF16 4u /* the records (and spfe_result) carry the descriptors as bf16 [kmax][256] — the f32
                                  descriptor of sp_extractor.cpp:512-513 rounded to nearest even — instead of f32: a record
                                  shrinks from ~1.1 MB to ~0.6 MB (1000 features), and with it the D2H copy of the host
                                  calls and the all-gather of the multi-GPU path.  spfe_result.desc is NULL then and
                                  spfe_result.desc_bf16 is set; spfe_record_layout.desc_elem_bytes says which.  Everything
                                  else in the record is unchanged.  The entry points that read descriptors from records
                                  (spfe_match_records_device, spfe_match_patches_record_device,
                                  spfe_track_dust_record_device) widen the rows on load: distances are the f32 arithmetic
                                  of the reference on those rounded values. */

#define SPFE_FLAG_LAZY_HEAT_INV 8u /* with SPFE_FLAG_HEAT: the host calls (spfe_extract*, spfe_submit_batch) bring back
                                     `heat` only; spfe_result.heat_inv is NULL and spfe_fetch_heat_inv() copies a frame's
                                     map on demand.  In the reference heat_inv_ is read by computeCovariance alone
                                     (sp_extractor.cpp:508) — which runs on the device here — and by no caller (SURVEY.md
                                     §8b "public but unread elsewhere"), so its 4 H W bytes per frame need not cross PCIe
                                     on every call (752x480: 1.44 MB of the 4.0 MB a call with heat maps brings back). */

/* spfe_result.status / record header word 2 */
#define SPFE_STATUS_COV_OVERFLOW 1 /* Set only when ONE covariance region has more pops than the device's last-resort list
                                      holds (SPFE_COV_FALLBACK_CAP, 4 M by default — the reference's own loop would spend
                                      ~0.1 s in that one BFS): cov2 / cov2_inv of that frame are then not valid.  Everything
                                      short of that is handled on the device, exactly, with status 0, for host calls, device
                                      records and all-gathered records alike: a walk longer than SPFE_COV_QCAP = 1024 pops
                                      reruns in one of SPFE_COV_OVF_SLOTS = 16 lists of SPFE_COV_OVF_CAP = 16384 pops per
                                      frame; a frame that exhausts those (or whose hills leave the staged window) is redone
                                      sequentially by cov_fallback_kernel.  The library has no host compute routine. */

/* ABI of this header.  Bumped whenever a struct below changes size or layout or an entry point changes its signature
 * (4: spfe_result.desc_bf16, spfe_record_layout.desc_elem_bytes — round 3 — and this check).  A caller built against an older
 * header would hand the library arrays of the wrong stride; spfe_check_abi(SPFE_ABI_VERSION, sizeof(spfe_config),
 * sizeof(spfe_result), sizeof(spfe_record_layout)) refuses that up front (the C++ adaptor and the Python loader call it). */
#define SPFE_ABI_VERSION 5

#define SPFE_DESC_DIM 256
#define SPFE_NUM_PARAMS 1300865 /* sp_extractor.cpp:16-43; order = register_module order :46-62 */

typedef struct spfe_handle_s *spfe_handle;

/*
 * Replaces the SPExtractor constructor (sp_extractor.cpp:342-359), which reads
 * tracking::num_features (tracker.cpp:131), camera::height/width and
 * common::model_path (:354-355) from globals.
 */
typedef struct {
  int height;               /* camera::height, multiple of 8 (:70); height x width: up to 262,143 cells of 8x8 and 2^31 bytes of
                               first-layer activations (64 channels a pixel, 4 / 2 bytes each in f32 / bf16 mode) per frame:
                               3840x2160 fits in both */
  int width;                /* camera::width, multiple of 8 */
  int num_features;         /* tracking::num_features; up to num_features+1 keypoints (:211-213); 1 .. 10000 (the
                               covariance link stage keeps 16 bytes per keypoint in one workgroup's LDS; the
                               shipped configurations use 800 - 1000) */
  int max_batch;            /* frames per spfe_extract_batch* call: 1 .. 65535, and max_batch * (height / 8) * (width / 8) * R
                               < 2^31 with R = 2048 bytes (SPFE_PRECISION_F32) or 1024 (SPFE_PRECISION_BF16), the head
                               activations of one cell: the 1x1 heads address a whole call with 32-bit byte offsets.
                               3840x2160: 8 frames in f32, 16 in bf16; 752x480: 185 / 371.  spfe_create refuses larger
                               values with SPFE_EINVAL and names the largest that fits */
  int device;               /* HIP device ordinal */
  int precision;            /* SPFE_PRECISION_* */
  unsigned flags;           /* SPFE_FLAG_* */
  const float *weights;     /* flat fp32 blob, SPFE_NUM_PARAMS floats, or NULL */
  const char *weights_path; /* "SPFW" file (sp_orb_slam_amd/weights.py), used if weights==NULL */
} spfe_config;

/*
 * Everything the caller reads after operator() (frame.cpp:296-314): keypoints,
 * descriptors and the SPExtractor side outputs (sp_extractor.h:61-73).
 * Pointers are library-owned host buffers, valid until the next call on the
 * same handle (the reference hands out cv::Mat headers over freed tensor
 * storage, sp_extractor.cpp:432-433,448-451; this does not).
 */
typedef struct {
  int K;                    /* keypoints emitted, raster order (:220-238) */
  int n_candidates;         /* cells with score >= 0.007 (:122) */
  int status;               /* 0, or SPFE_STATUS_* bits */
  int reserved;
  const float *kp_xy;       /* [K][2] pt.x, pt.y (integer valued); size=1, octave=0, angle=-1 (:231-232) */
  const float *kp_response; /* [K] heat_inv at the keypoint (:271) */
  const float *desc;        /* [K][256] unit-L2 rows, CV_32FC1 (:512-513) */
  const float *cov2;        /* [K][2] (:332) */
  const float *cov2_inv;    /* [K][2] getCov2Inv() (sp_extractor.h:67) */
  const int16_t *occ_grid;  /* [H/8][W/8] CV_16SC1, -1 = empty (:178,227-228) */
  const float *dense_dust;  /* [H/8][W/8] softmax dustbin (:107,450) */
  const float *semi_dust;   /* [H/8][W/8] raw dustbin logit (:106,448) */
  const float *heat;        /* [H][W] or NULL without SPFE_FLAG_HEAT (:467) */
  const float *heat_inv;    /* [H][W] or NULL without SPFE_FLAG_HEAT / with SPFE_FLAG_LAZY_HEAT_INV (:468) */
  const uint16_t *desc_bf16; /* [K][256] bf16 bit patterns with SPFE_FLAG_DESC_BF16 (then desc is NULL), else NULL */
} spfe_result;

SPFE_API int spfe_create(const spfe_config *cfg, spfe_handle *out);
SPFE_API void spfe_destroy(spfe_handle h);

/* SPExtractor::operator() for one CV_8UC1 frame of the configured size.
 * `stride` = bytes between rows (cv::Mat::step). */
SPFE_API int spfe_extract(spfe_handle h, const uint8_t *image, int stride, spfe_result *out);

/* n independent frames (n <= max_batch); outs[i] valid until the next call. */
SPFE_API int spfe_extract_batch(spfe_handle h, const uint8_t *const *images, int stride, int n,
                       spfe_result *outs);

/* The synchronous call in three parts, for a caller that copies the outputs out of the library's buffers (the drop-in
 * class does: the reference's members are deep cv::Mat copies, sp_extractor.cpp:436-474): the two H x W maps are complete
 * after the network's tail, ~0.15 ms before the record (selection, sampling, covariance follow), and their D2H runs beside
 * that work (SPFE_EARLY_HEAT_COPY) — so the caller's own copy of the maps can run beside it too.
 *   spfe_extract_begin   what spfe_extract_batch does up to the end of its enqueueing; returns at once
 *   spfe_extract_maps    blocks until the maps asked for (either argument may be NULL: not asked for) are in host
 *                        memory; *heat / *heat_inv = frame 0's map, frame i at + i * H * W floats (*heat_inv = NULL with
 *                        SPFE_FLAG_LAZY_HEAT_INV).  `heat` arrives first, `heat_inv` behind it: a caller copying both asks
 *                        for heat alone, copies it, then asks for heat_inv.  NULL results (and SPFE_OK) when the maps do not
 *                        travel ahead of the record in this call (no SPFE_FLAG_HEAT, SPFE_EARLY_HEAT_COPY=0):
 *                        spfe_extract_finish delivers them as spfe_extract_batch does.  Optional, any number of times.
 *   spfe_extract_rows    blocks until frame `frame`'s descriptor rows are in host memory — final behind the sampling, while
 *                        the covariance of the call still runs: *K rows of 256 floats at *desc (where spfe_result.desc will
 *                        point).  *desc = NULL (and SPFE_OK) when the rows travel with the record in this call (batches on
 *                        the side-stream chain, SPFE_FLAG_DESC_BF16, SPFE_EARLY_HEAT_COPY=0).  Optional.
 *   spfe_extract_finish  the rest of spfe_extract_batch: blocks, fills outs[0 .. n) (same pointers, same lifetime)
 * begin + finish == spfe_extract_batch, bit for bit.  Between the two no other call on the handle (SPFE_EINVAL from begin
 * while a call is open, from maps / finish when none is). */
SPFE_API int spfe_extract_begin(spfe_handle h, const uint8_t *const *images, int stride, int n);
SPFE_API int spfe_extract_maps(spfe_handle h, const float **heat, const float **heat_inv);
SPFE_API int spfe_extract_rows(spfe_handle h, int frame, int *K, const float **desc);
SPFE_API int spfe_extract_finish(spfe_handle h, spfe_result *outs);

/* Pipelined host path.  spfe_extract_batch is synchronous like the reference's operator() (upload
 * sp_extractor.cpp:379-390, blocking D2H :427-433).  A host that has the next frames while the current ones
 * are being processed (a dataset player, a multi-camera rig, the batch path) submits instead:
 *   spfe_submit_batch   copies the frames into pinned staging, enqueues H2D (copy stream), the whole path
 *                       (compute + side streams) and the D2H of the records (+ heat maps with SPFE_FLAG_HEAT;
 *                       second copy stream), and returns at once with a ticket;
 *   spfe_collect_batch  blocks until that batch is back in host memory; outs[i] are valid until three
 *                       further batches have been submitted.
 * Up to 3 batches may be in flight (submit fails with SPFE_EINVAL when the oldest has not been collected), so
 * the H2D of batch i + 1 and the D2H of batch i - 1 overlap the compute of batch i.  Collect in any order. */
SPFE_API int spfe_submit_batch(spfe_handle h, const uint8_t *const *images, int stride, int n, long *ticket);
SPFE_API int spfe_collect_batch(spfe_handle h, long ticket, spfe_result *outs);

/* Everything after the network (sp_extractor.cpp:105-148 detector tail and
 * descriptor sampling, :461-514 host glue, nms, computeCovariance) for n frames
 * whose raw head outputs the caller provides as HOST arrays: semi [n][H/8][W/8][65]
 * (convPb logits, channels last) and coarse [n][H/8][W/8][256] (convDb output,
 * not normalised).  Used by the tests to drive the selection kernels with
 * hand-made logits; also the entry for a caller with its own network. */
SPFE_API int spfe_postprocess(spfe_handle h, const float *semi, const float *coarse, int n,
                              spfe_result *outs);

/*
 * Device-resident batch path (multi-GPU pipeline): d_images is a DEVICE pointer
 * to n contiguous u8 frames [n][H][W]; d_records is a DEVICE buffer of
 * n * spfe_record_bytes(h) bytes that receives one fixed-stride record per
 * frame (layout: spfe_record_layout).  Work is enqueued on `stream`
 * (hipStream_t, NULL = the handle's own stream) and NOT synchronised: the caller
 * may all-gather d_records with RCCL on the same stream.
 */
typedef struct {
  size_t bytes;    /* record stride, multiple of 256 */
  int kmax;        /* num_features + 1 */
  size_t off_hdr;  /* int32 K, int32 n_candidates, int32 status, int32 reserved */
  size_t off_xy;   /* float [kmax][2] */
  size_t off_resp; /* float [kmax] */
  size_t off_cov;  /* float [kmax][2] */
  size_t off_cinv; /* float [kmax][2] */
  size_t off_desc; /* float [kmax][256]; bf16 [kmax][256] with SPFE_FLAG_DESC_BF16 */
  size_t off_occ;  /* int16 [H/8][W/8] */
  size_t off_dd;   /* float [H/8][W/8] dense_dust */
  size_t off_sd;   /* float [H/8][W/8] semi_dust */
  int desc_elem_bytes; /* 4, or 2 with SPFE_FLAG_DESC_BF16 */
} spfe_record_layout;

SPFE_API int spfe_get_record_layout(spfe_handle h, spfe_record_layout *out);
SPFE_API size_t spfe_record_bytes(spfe_handle h);
SPFE_API int spfe_extract_batch_device(spfe_handle h, const void *d_images, int n, void *d_records,
                              void *stream);
/* (Batches of >= 2 frames issue the layers behind conv1b as two half batches, the second on a library-owned stream that must
 * not share a hardware queue with `stream`: the first call that brings a new `stream` measures that with two 150 us spin
 * kernels that time-stamp themselves on the device clock, and synchronises `stream` once while doing so (a stream under
 * capture is not probed: no split).  The answer is kept per hipStream_t value for the life of the handle — a stream destroyed
 * and re-created at the same address inherits it (a performance matter only).  spfe_debug_read("split_streams") reports the
 * outcome.  SPFE_F32_SPLIT=0 / SPFE_F32_SPLIT_PROBE=0 switch the split / the measurement off.) */
/* Ticket of the most recent spfe_extract_batch_device call on this handle (0, 1, 2, ...), and the
 * ordering point for SPFE_FLAG_ASYNC_COV: makes `stream` (NULL = the handle's stream) wait until the
 * records of call `ticket` (one of the last 4 calls) AND OF EVERY EARLIER CALL are complete (also where the handle runs two
 * side chains on two sets of buffers — large bf16 frames, DESIGN.md 5.1: tickets stay one sequence).  Without the flag the
 * call itself does this and spfe_wait_records is a no-op dependency. */
SPFE_API long spfe_last_ticket(spfe_handle h);
SPFE_API int spfe_wait_records(spfe_handle h, long ticket, void *stream);

/* ---- multi-GPU batch path: RCCL all-gather of the records (BASELINE configs[2]) ----------
 * One process per GPU, one handle per process.  Frames are independent, so a batch shards over ranks with no
 * collective in the data path; the ONLY exchange is this all-gather of the fixed-stride records (K lives in
 * the record header, so no count exchange).  The C++ SLAM host uses these directly; no torch involved.
 *   rank 0: spfe_comm_unique_id(id) -> ship the 128 bytes to every rank (MPI, a socket, a file ...)
 *   every rank: spfe_comm_init(h, id, rank, world)            [ncclCommInitRank on the handle's device]
 *   per batch:  spfe_extract_batch_device(h, imgs, n, d_local, stream); t = spfe_last_ticket(h);
 *               spfe_allgather_records(h, t, d_local, d_all, n);   [d_all: world * n * spfe_record_bytes(h)]
 *               spfe_comm_wait(h, consumer_stream);                [or hipStreamSynchronize(spfe_comm_stream(h))]
 * The collective is issued on the library's side stream, right behind the covariance kernels of the batch it
 * gathers: call spfe_allgather_records for batch i BEFORE enqueueing batch i + 1 (with SPFE_FLAG_ASYNC_COV the gather
 * of batch i then overlaps the convolutions of batch i + 1; called later it still is correct, it just queues behind
 * batch i + 1's covariance).  No stream waits in a hardware queue for an event (a waiting stream of its own can land
 * on the compute stream's hardware queue and stall it; SPFE_COMM_OWN_STREAM=1 restores that form).  d_local / d_all
 * must stay untouched until the gather has completed (order the next writer with spfe_comm_wait).  librccl is loaded on first use (dlopen), so single-GPU users of
 * libspfe.so do not need it.  rank-major output: global frame g = rank * n + i. */
#define SPFE_COMM_ID_BYTES 128
SPFE_API int spfe_comm_unique_id(void *id, size_t cap);
SPFE_API int spfe_comm_init(spfe_handle h, const void *id, int rank, int world);
SPFE_API int spfe_comm_destroy(spfe_handle h);
SPFE_API int spfe_allgather_records(spfe_handle h, long ticket, const void *d_local, void *d_all, int frames_per_rank);
SPFE_API int spfe_comm_wait(spfe_handle h, void *stream);
SPFE_API void *spfe_comm_stream(spfe_handle h); /* hipStream_t of the collective, NULL before spfe_comm_init */
SPFE_API int spfe_comm_count(spfe_handle h, int *count); /* ncclCommCount: the rank count RCCL itself reports */

/* Host view of ONE record that the caller copied to host memory. */
SPFE_API int spfe_view_record(spfe_handle h, const void *host_record, spfe_result *out);

/* Test/diagnostic tap: copy an intermediate device buffer of frame `frame` of
 * the last call to host. Names: "semi" [hc][wc][65], "coarse" [hc][wc][256],
 * "heat_log" [H][W], "feat" [hc][wc][128], "act<i>" layer outputs.
 * The descriptor branch (convDa, convDb: sp_extractor.cpp:99-100) computes only the rows of the coarse map that the
 * emitted keypoints' bilinear taps read (:134-148 reads nothing else); "coarse" completes the map first (one dense
 * pass over the last call's activations), "coarse_sparse" is the map as the call left it, "db_total" [1] int /
 * "db_list" ints the cells it computed (b * hc * wc + cell; frame ignored), "da_gathered" [1] int whether convDa ran on
 * those cells only as well.
 * Returns the number of bytes copied or a negative error. */
SPFE_API long spfe_debug_read(spfe_handle h, const char *name, int frame, void *dst, size_t cap);

/* ---- descriptor matching ------------------------------------------------
 * Replaces  cv::BFMatcher::create(cv::NORM_L2, crossCheck)->match(desc_query, matches)  with
 * desc_train added, as called by SPMatcher::SearchByBruteForce (orb_slam2/src/cv/sp_matcher.cpp:
 * 1642-1674; the distance is SPMatcher::DescriptorDistance, :1636-1640 = L2 norm of a - b).
 * Descriptors are rows of 256 floats.  For every query row i: train_idx[i] = matched train row or
 * -1, distance[i] = its L2 distance (FLT_MAX when unmatched) — i.e. cv::DMatch{queryIdx = i,
 * trainIdx = train_idx[i], distance}, with the unmatched queries (which OpenCV omits) marked -1.
 *   cross_check != 0 (the reference's setting): OpenCV's batchDistance rule — every train row votes
 *     for its nearest query (lowest query index on ties); a query is matched to the closest train
 *     row that voted for it (lowest train index on ties), queries without votes stay unmatched.
 *   cross_check == 0: plain nearest train row per query (lowest index on ties).
 * NaN / infinite distances never match.  n_query or n_train == 0: all -1, SPFE_OK. */
SPFE_API int spfe_match(spfe_handle h, const float *query, int n_query, const float *train, int n_train,
                        int cross_check, int32_t *train_idx, float *distance);
/* Replaces  matcher->knnMatch(desc_query, matches, 2)  on a cv::FlannBasedMatcher that holds desc_train — the k = 2
 * search behind the ratio tests of KeyFrame::matchMps (orb_slam2/src/type/keyframe.cpp:447-470, index built in
 * buildIndexesMps :421-445) and SPMatcher's keyframe matching (src/cv/sp_matcher.cpp:195-215, :264-280) — by the
 * EXACT two nearest train rows (the reference's randomised kd-trees, matching::ntree / nchecks, are approximate:
 * this returns what they approximate, so it has no bit-parity target, only the exact-search oracle's).
 * train_idx / distance: [n_query][2], nearest first; ties -> lower train index; -1 / FLT_MAX when n_train < 2
 * (or a distance is NaN / infinite).  Distances as in spfe_match. */
SPFE_API int spfe_match_knn2(spfe_handle h, const float *query, int n_query, const float *train, int n_train,
                             int32_t *train_idx, float *distance);
/* Device-resident form: matches the descriptors of n_pairs query records against n_pairs train
 * records (both arrays of spfe_record_bytes()-strided records in HBM, e.g. the outputs of two
 * spfe_extract_batch_device calls), reading K from the record headers on the device; no host
 * synchronisation.  d_out: n_pairs blocks of spfe_match_out_bytes(h) bytes, each
 * int32 train_idx[kmax] followed by float distance[kmax] (kmax = num_features + 1; entries >= the
 * query record's K are -1 / FLT_MAX).  stream: hipStream_t (NULL = the handle's stream). */
SPFE_API int spfe_match_records_device(spfe_handle h, const void *d_query_records, const void *d_train_records,
                                       int n_pairs, int cross_check, void *d_out, void *stream);
SPFE_API size_t spfe_match_out_bytes(spfe_handle h);

/* Patch-wise association of projected map points — the loop of Tracker::trackFrameDustKFLocal,
 * orb_slam2/src/tracking/tracker_dust.cpp:113-172 (the caller filters `!in_view || isBad()` points out).
 * Map point i sits at dust-map position (mp_uv[2i], mp_uv[2i+1]) in CELL units (dust_proj_u / _v) and
 * carries descriptor mp_desc[i]; it examines the keypoints of cells (floor(u)+du, floor(v)+dv),
 * du, dv in {0,1}, du outer, and takes the one with the smallest L2 distance below max_dist (0.75 in
 * the reference; first one on ties); a taken keypoint is gone for the map points after it (the
 * reference clears its occ_grid cell).  kp_idx[i] = keypoint index or -1.  Distances are
 * (float) cv::norm(a, b, NORM_L2): squared differences accumulated in double.  Cells outside the grid
 * hold no keypoint (the reference does not check), and a position that does not floor into the grid (negative, at or beyond
 * the last column / row + 1, NaN, infinite) has no candidates.  n_points <= 4096.
 * occ_grid: int16 [height/8][width/8] and kp_desc: [n_keypoints][256] of the frame (spfe_result).
 * The ordered claim keeps 5 bytes per keypoint in one workgroup's 160 KB of LDS (beside 20 bytes of its own): n_keypoints, or
 * num_features + 1 of the record form and of spfe_track_dust_record_device, <= SPFE_PATCH_MAX_KEYPOINTS; beyond it
 * SPFE_EINVAL before anything is written or launched. */
#define SPFE_PATCH_MAX_KEYPOINTS 32764 /* 4 static + 5 * 32764 + 16 dynamic bytes = 163,840 of 163,840 */
SPFE_API int spfe_match_patches(spfe_handle h, const float *mp_desc, const float *mp_uv, int n_points,
                                const int16_t *occ_grid, const float *kp_desc, int n_keypoints, float max_dist,
                                int32_t *kp_idx);
/* The same against ONE record resident in HBM (occ_grid, descriptors and K read on the device);
 * d_mp_desc (float [n_points][256]), d_mp_uv (float [n_points][2]) and d_kp_idx (int32 [n_points]) are device arrays of
 * exactly these sizes; d_record is one record of spfe_record_bytes(h) bytes, of which nothing at and beyond row K of a
 * per-keypoint array is used; enqueued on `stream`, no host synchronisation. */
SPFE_API int spfe_match_patches_record_device(spfe_handle h, const void *d_mp_desc, const void *d_mp_uv,
                                              int n_points, const void *d_record, float max_dist, void *d_kp_idx,
                                              void *stream);

/* ---- direct "dust" alignment ------------------------------------------------
 * Replaces  Optimizer::PoseOptimizationDust(Frame *pFrame, const std::vector<MapPoint *> &mps,
 *                                           std::vector<bool> &is_visible)
 * (orb_slam2/src/mapping/optimizer_dust.cpp:170-294, called from Tracker::trackFrameDustKFLocal,
 * tracker_dust.cpp:91): a 6-DoF Levenberg-Marquardt (g2o: OptimizationAlgorithmLevenberg, one VertexSE3Expmap,
 * one EdgeSE3ProjectDustOnlyPose per map point — src/optimization/types_dust_tracking.cpp:37-140 — with
 * RobustKernelHuber(0.9), optimize(40)) that moves the camera pose so that the map points project onto cells
 * with a low dustbin probability.  dense_dust = Frame::dust_ (the extractor's dense_dust_, [H/8][W/8]);
 * points_xyz[i] = mps[i]->GetWorldPos() (3 floats); Tcw = Frame::mTcw (CV_32F 4x4, row-major); fx..cy =
 * Frame::fx.. (full resolution; the /8 and -3.5 of :223-226 are applied inside).
 * Outputs: Tcw_out (what pFrame->SetPose receives, :287), inlier[i] (is_visible[i] / in_view, :262-266: level 0
 * and chi2 <= inlier_chi2), proj_uv[i] = (dust_proj_u, dust_proj_v) of the inliers (:267-268), *n_inlier (the
 * return value), *iterations (optimize()'s).  n <= SPFE_DUST_MAX_POINTS (the tracker keeps 150-200).
 * Degenerate calls, as g2o behaves: max_iterations == 0 evaluates nothing — every edge keeps level 0 / error 0, so all n
 * points are reported as inliers with proj_uv = (0, 0) and the pose is echoed (use >= 1 for meaningful flags; the
 * reference always passes 40); n == 0 has no active edge — the pose is echoed, *iterations = 0, *n_inlier = 0.
 * The arithmetic is pinned by tests/golden/dust_*.npz (an independent f64 numpy / scipy statement).
 * g2o is not part of the reference snapshot: its algorithm is restated (include/spfe_dust_math.h) — results
 * equal the CPU oracle's up to the device's sin / cos in the exponential map. */
#define SPFE_DUST_MAX_POINTS 512
typedef struct {
  float fx, fy, cx, cy;
  int max_iterations;   /* 40 (:243) */
  double huber_delta;   /* 0.9 (:221) */
  double inlier_chi2;   /* 0.9 (:260) */
} spfe_dust_params;
SPFE_API int spfe_align_dust(spfe_handle h, const float *dense_dust, const float *points_xyz, int n,
                             const float *Tcw, const spfe_dust_params *prm, float *Tcw_out, uint8_t *inlier,
                             float *proj_uv, int *n_inlier, int *iterations);
/* The same against the dense_dust of ONE record resident in HBM; d_points_xyz (float [n][3]) / d_Tcw (float [16]) are device
 * arrays; d_out receives SPFE_DUST_OUT_BYTES: float Tcw_out[16] | int32 n_inlier | int32 iterations | pad to
 * SPFE_DUST_OFF_UV: float proj_uv[512][2] | SPFE_DUST_OFF_INLIER: uint8 inlier[512].  Enqueued on `stream`
 * (NULL = the handle's), no host synchronisation; order it after the record with spfe_wait_records. */
#define SPFE_DUST_OFF_UV 128
#define SPFE_DUST_OFF_INLIER (128 + SPFE_DUST_MAX_POINTS * 8)
#define SPFE_DUST_OUT_BYTES (128 + SPFE_DUST_MAX_POINTS * 9)
SPFE_API int spfe_align_dust_record_device(spfe_handle h, const void *d_record, const void *d_points_xyz, int n,
                                           const void *d_Tcw, const spfe_dust_params *prm, void *d_out,
                                           void *stream);

/* The tracker's per-frame chain behind the extraction, on ONE record resident in HBM — Tracking::trackFrameDustKFLocal,
 * orb_slam2/src/tracking/tracker_dust.cpp:92-172: PoseOptimizationDust(&mCurrentFrame, mps_for_track, is_visible) (:92-94),
 * give up when n_inlier < min_inliers (tracking::dust::th_ninlier, :97-102), else the patch-wise association of the in_view
 * map points at their dust_proj_u / v (:113-172; see spfe_match_patches).  Map point i = d_points_xyz[3 i..] with track
 * descriptor d_mp_desc[256 i..] (MapPoint::getDescTrack()): float [n][3] and float [n][256].  d_dust_out receives the
 * SPFE_DUST_OUT_BYTES block above; d_kp_idx, int32 [n]: d_kp_idx[i] = index of the keypoint map point i takes (mCurrentFrame.mvpMapPoints[idx] = mp), -1 for points that
 * are not in view, find nothing below max_dist (0.75f, :121), or when the alignment had too few inliers.  Three launches behind
 * each other on `stream` (the alignment, then the two of the association: candidates and claim): projections, flags and
 * n_inlier never leave HBM; no host synchronisation.  n <= 512. */
SPFE_API int spfe_track_dust_record_device(spfe_handle h, const void *d_record, const void *d_points_xyz,
                                           const void *d_mp_desc, int n, const void *d_Tcw, const spfe_dust_params *prm,
                                           int min_inliers, float max_dist, void *d_dust_out, void *d_kp_idx, void *stream);

/* The batch path's form: n_frames independent solves in ONE launch, one workgroup each (a single solve is a chain of
 * dependent double-precision operations — latency, not throughput: 256 of them side by side take as long as one).
 * Frame f aligns d_n_points[f] points at d_points_xyz + f * SPFE_DUST_MAX_POINTS * 3 floats, starting from the pose
 * d_Tcw + 16 f, against the dense_dust of record f of d_records (spfe_record_bytes() strided, e.g. the output of
 * spfe_extract_batch_device or the all-gathered array); d_out + f * SPFE_DUST_OUT_BYTES receives the block described
 * above.  Sizes: d_records n_frames * spfe_record_bytes(), d_points_xyz float [n_frames][SPFE_DUST_MAX_POINTS][3] (rows at and
 * beyond d_n_points[f] of a frame are not read), d_n_points int32 [n_frames] (a count outside [0, SPFE_DUST_MAX_POINTS] is
 * clamped on the device), d_Tcw float [n_frames][16], d_out n_frames * SPFE_DUST_OUT_BYTES.  All arrays in device memory;
 * enqueued on `stream`, no host synchronisation. */
SPFE_API int spfe_align_dust_batch_device(spfe_handle h, const void *d_records, int n_frames, const void *d_points_xyz,
                                          const void *d_n_points, const void *d_Tcw, const spfe_dust_params *prm,
                                          void *d_out, void *stream);

/* ---- covariance-weighted pose refinement ---------------------------------------------------------
 * Replaces the pose-only optimisations that consume the covariance stage's cov2_inv as the information matrix of each
 * reprojection edge (g2o EdgeSE3ProjectXYZOnlyPose, Huber delta sqrt(5.991) rounded to float):
 *   SPFE_POSE_DUST_POST     Optimizer::PoseOptimizationDustPost (orb_slam2/src/mapping/optimizer_dust.cpp:35-167,
 *                           tracking/tracker_dust.cpp:183): optimize(10) with Huber, classify chi2 > 7.378, drop the
 *                           kernels, optimize(10) on the inliers from there.
 *   SPFE_POSE_OPTIMIZATION  Optimizer::PoseOptimization, monocular edges (mapping/optimizer.cpp:231-443; TrackLocalMap,
 *                           TrackWithMotionModel): four rounds of optimize(10), each from the INPUT pose, classified with
 *                           5.991f after each (inliers on the error of the last trial, outliers re-evaluated), no kernels
 *                           after round 2, one round only when there are fewer than 10 edges.
 * One edge per keypoint with a map point, in ascending keypoint index; fewer than 3 edges: n_good 0, the pose echoed.  A round
 * without a level-0 edge leaves the pose where it is and reports 0 iterations.  One workgroup per solve (latency); the
 * arithmetic is include/spfe_pose_math.h — results equal its host statement up to the device's sin / cos. */
#define SPFE_POSE_DUST_POST 0
#define SPFE_POSE_OPTIMIZATION 1
typedef struct {
  float fx, fy, cx, cy; /* Frame::fx .. cy (full resolution) */
  int schedule;         /* SPFE_POSE_* */
  int iterations;       /* per optimize() call: 10 in both schedules */
} spfe_pose_params;
/* Host form: n edges in edge order, obs_xy [n][2] (mvKeysUn[i].pt), inv_sigma2 [n][2] (cov2_inv_[i]), points_xyz [n][3]
 * (GetWorldPos()).  Tcw_out (pFrame->SetPose), outlier [n] (mvbOutlier), iterations [4] (per optimize() call, 0 for
 * calls not made), *n_good (the return value: nInitialCorrespondences - nBad).  n <= 10001. */
SPFE_API int spfe_refine_pose(spfe_handle h, const float *obs_xy, const float *inv_sigma2, const float *points_xyz, int n,
                              const float *Tcw, const spfe_pose_params *prm, float *Tcw_out, uint8_t *outlier,
                              int *iterations, int *n_good);
/* The output block of the device forms, spfe_pose_out_bytes(h) bytes (a multiple of 256):
 *   float Tcw_out[16] | int32 n_initial | int32 n_good | int32 iterations[4] | int32 status (SPFE_POSE_STATUS_*) |
 *   int32 verdict (SPFE_TRACK_*; chained forms) | int32 n_matches (chained forms) | int32 n_inliers (the local-map,
 *   motion-model and reference-keyframe chains; not written by the other forms) | int32 widened (SPFE_POSE_OFF_WIDENED: the
 *   motion-model chain only) | int32 n_outliers (SPFE_POSE_OFF_N_OUTLIERS: the motion-model and reference-keyframe chains
 *   only) | pad to SPFE_POSE_OFF_OUTLIER |
 *   uint8 outlier[kmax] per keypoint (mvbOutlier; 0 for keypoints without a map point). */
#define SPFE_POSE_OFF_OUTLIER 128
#define SPFE_POSE_STATUS_COV_OVERFLOW 1 /* the record has SPFE_STATUS_COV_OVERFLOW: cov2_inv invalid, nothing optimised,
                                           the pose echoed, n_initial = n_good = 0 */
#define SPFE_TRACK_OK 0           /* nopt_inlier * 1.0f / n_matches > th_ratio (tracker_dust.cpp:218) */
#define SPFE_TRACK_FAIL_INLIERS 1 /* n_inlier < th_ninlier (:97) */
#define SPFE_TRACK_FAIL_MATCHES 2 /* n_matches < th_nmatch (:174) */
#define SPFE_TRACK_FAIL_RATIO 3   /* the ratio test (:218) */
#define SPFE_TRACK_FAIL_COV 4     /* the record's cov2_inv is invalid (SPFE_POSE_STATUS_COV_OVERFLOW) */
SPFE_API size_t spfe_pose_out_bytes(spfe_handle h);
/* The device forms stage the edge data of a solve in LDS while the edges number at most this (the handle's num_features + 1
 * where everything fits); beyond it every evaluation reads the record and the point array.  The results do not depend on
 * it.  -1 without a handle. */
SPFE_API int spfe_pose_lds_edge_capacity(spfe_handle h);
/* Against ONE record resident in HBM: d_mp_of_kp int32 [kmax] = Frame::mvpMapPoints (-1 or an index into d_points_xyz,
 * [.][3] floats; entries at and beyond the record's K are ignored); kp_xy and cov2_inv are read from the record.  d_Tcw
 * [16] floats, d_out one block above.  This form is not told how many points there are: every value >= 0 below K is taken
 * as a row of d_points_xyz and read — keeping d_mp_of_kp within the array is the caller's duty (d_points_xyz must reach one
 * row past the largest holder; any negative value is "none").  The chains that take n (spfe_track_local_map_record_device
 * and the two fallback chains) apply their own rule.  Enqueued on `stream` (NULL = the handle's), no host synchronisation. */
SPFE_API int spfe_refine_pose_record_device(spfe_handle h, const void *d_record, const void *d_mp_of_kp,
                                            const void *d_points_xyz, const void *d_Tcw, const spfe_pose_params *prm,
                                            void *d_out, void *stream);
/* The batch path's form: n_frames solves in ONE launch, one workgroup each: record f of d_records (spfe_record_bytes()
 * strided), d_mp_of_kp + f * kmax, d_points_xyz + f * points_stride floats, d_Tcw + 16 f, d_out + f * spfe_pose_out_bytes.
 * Sizes: d_mp_of_kp int32 [n_frames][kmax], d_points_xyz float [n_frames][points_stride] (a multiple of 3 floats; of a frame's
 * slice only the rows its holders name are read, and as above the holders' range is the caller's duty), d_Tcw float
 * [n_frames][16], d_out n_frames * spfe_pose_out_bytes(h). */
SPFE_API int spfe_refine_pose_batch_device(spfe_handle h, const void *d_records, int n_frames, const void *d_mp_of_kp,
                                           const void *d_points_xyz, size_t points_stride, const void *d_Tcw,
                                           const spfe_pose_params *prm, void *d_out, void *stream);
/* Tracking::trackFrameDustKFLocal behind the extraction (tracker_dust.cpp:22-228) on ONE resident record: the chain of
 * spfe_track_dust_record_device (alignment, th_ninlier gate, association; d_dust_out and d_kp_idx as there), then
 * n_matches >= th_nmatch (:174), PoseOptimizationDustPost over the associations in keypoint order from the aligned pose
 * (:183), and the ratio test nopt_inlier * 1.0f / n_matches > th_ratio (:218).  d_pose_out receives the block above with
 * the verdict; on every failing path its pose is the input d_Tcw (SetPose(mVelocity * mLastFrame.mTcw), :101, :178, :225).
 * EuRoC's values (orb_ros/cfg/euroc_mono.yaml): th_ratio 0.35, th_ninlier 20, th_nmatch 20.  All kernels back to back on
 * `stream`, no host synchronisation.  dust_prm and the tracker's max_dist as in spfe_track_dust_record_device; pose_prm's
 * schedule must be SPFE_POSE_DUST_POST. */
SPFE_API int spfe_track_dust_refine_record_device(spfe_handle h, const void *d_record, const void *d_points_xyz,
                                                  const void *d_mp_desc, int n, const void *d_Tcw,
                                                  const spfe_dust_params *dust_prm, const spfe_pose_params *pose_prm,
                                                  int th_ninlier, int th_nmatch, float th_ratio, float max_dist,
                                                  void *d_dust_out, void *d_kp_idx, void *d_pose_out, void *stream);

/* ---- local-map tracking: window search by projection and the pose gate -------------------------------
 * Replaces SPMatcher::SearchByProjection in its two most used forms, on what a record holds (kp_xy, occ_grid,
 * descriptors), and with it Tracking::SearchLocalPoints (tracker.cpp:768-832) and Tracking::TrackLocalMap (:561-615):
 *   SPFE_PROJ_LOCAL_MAP   SearchByProjection(Frame &, const vector<MapPoint *> &, th, th_dist)  sp_matcher.cpp:344-432, behind
 *                         Frame::isInFrustum per point (frame.cpp:330-380): view-cosine test, radius 2.5 / 4 by view cosine
 *                         (times th when th != 1), acceptance best <= th_dist, else best < 1.2 c2 / (c2 + duv) (adaptive) or 0.7.
 *                         As SearchLocalPoints does first, keypoints that hold a point without SPFE_PROJ_SEARCHABLE are
 *                         emptied, and a point some keypoint holds on entry is not searched (mnLastFrameSeen).
 *   SPFE_PROJ_LAST_FRAME  SearchByProjection(CurrentFrame, LastFrame, th, bMono = true)  sp_matcher.cpp:1439-1543: no
 *                         view-cosine test, radius th, acceptance best <= 0.7f; the caller passes the last frame's
 *                         non-outlier map points in keypoint order.
 * Map point i: world position xyz[i], unit normal normal[i] (MapPoint::GetNormal; unused in LAST_FRAME mode), track
 * descriptor desc[i] (256 f32, getDescTrack), flags[i] = SPFE_PROJ_SEARCHABLE (!isBad()) | SPFE_PROJ_OBSERVED
 * (Observations() > 0).  mp_of_kp = Frame::mvpMapPoints as indices into the point arrays (-1: none; values outside [0, n)
 * count as none and are left alone), updated in place.  Points are served in index order; a keypoint is blocked while it
 * holds an OBSERVED point; an accepted point writes itself into mp_of_kp[best] (the last writer wins over unobserved holders).
 * The arithmetic — projection, window, distance, tie and acceptance rules, and the cases the reference leaves undefined —
 * is include/spfe_proj_math.h.
 * Outputs per point: kp_of_mp[i] = the keypoint point i took at its turn (-1: none; it still holds it iff
 * mp_of_kp[kp_of_mp[i]] == i), in_view[i] (mbTrackInView: searched and inside the frustum), proj_uv[i] (mTrackProjX / Y) and
 * view_cos[i] (mTrackViewCos) of the in-view points (0 otherwise).  n_matches counts every acceptance (the reference's return
 * value), n_to_match the in-view points (SearchLocalPoints' nToMatch).
 * Capacities: n <= SPFE_PROJ_MAX_POINTS; the largest window radius the parameters can produce (4 th in LOCAL_MAP mode, th in
 * LAST_FRAME mode) <= SPFE_PROJ_MAX_RADIUS; the ordered claim keeps 9 bytes per keypoint in one workgroup's 160 KB of LDS
 * (beside 32 bytes of its own): K of the host-array form, or num_features + 1 of the record forms, <= SPFE_PROJ_MAX_KEYPOINTS.
 * Beyond any of them: SPFE_EINVAL before any launch. */
#define SPFE_PROJ_LOCAL_MAP 0
#define SPFE_PROJ_LAST_FRAME 1
#define SPFE_PROJ_SEARCHABLE 1u
#define SPFE_PROJ_OBSERVED 2u
#define SPFE_PROJ_MAX_POINTS 8192
#define SPFE_PROJ_MAX_KEYPOINTS 18200 /* 16 static + 9 * 18200 + 16 dynamic bytes = 163,832 of 163,840 */
#define SPFE_PROJ_MAX_RADIUS 32 /* pixels */
/* cells lo = floor((u - r) / 8) .. hi = ceil((u + r) / 8): 2 r / 8 cells, one more at either end, and one for the rounding of
 * the two f32 quotients */
#define SPFE_PROJ_MAX_CELLS_AXIS (2 * SPFE_PROJ_MAX_RADIUS / 8 + 3)
#define SPFE_PROJ_MAX_CAND (SPFE_PROJ_MAX_CELLS_AXIS * SPFE_PROJ_MAX_CELLS_AXIS) /* one keypoint per cell */
typedef struct {
  float fx, fy, cx, cy; /* Frame::fx .. cy (full resolution) */
  int mode;             /* SPFE_PROJ_* */
  float th;             /* tracking::map::th_window_size 1 (5 after a relocalisation, tracker.cpp:818-819);
                           TrackWithMotionModel: 15, then 30 (tracker.cpp:495-506) */
  float th_dist;        /* TH_HIGH 0.7 (LOCAL_MAP) */
  float view_cos_limit; /* tracking::map::th_view_cos 0.5 (LOCAL_MAP) */
  int adaptive;         /* tracking::map::match_adaptive (on in the shipped configurations) */
  float c2_thresh;      /* tracking::dust::c2_thresh 81 */
} spfe_proj_params;
/* Host-array form: kp_xy [K][2], occ_grid int16 [H/8][W/8] and kp_desc [K][256] f32 of the frame (spfe_result); n points;
 * mp_of_kp [K] in/out; Tcw [16] row-major.  kp_of_mp [n], in_view [n], proj_uv [n][2], view_cos [n] (each may be NULL). */
SPFE_API int spfe_search_projection(spfe_handle h, const float *kp_xy, const int16_t *occ_grid, const float *kp_desc, int K,
                                    const float *xyz, const float *normal, const float *desc, const uint8_t *flags, int n,
                                    int32_t *mp_of_kp, const float *Tcw, const spfe_proj_params *prm, int32_t *kp_of_mp,
                                    uint8_t *in_view, float *proj_uv, float *view_cos, int *n_matches, int *n_to_match);
/* The output block of the device forms, spfe_proj_out_bytes(h) = SPFE_PROJ_OUT_BYTES bytes:
 *   int32 n_matches | int32 n_to_match | int32 n | pad to SPFE_PROJ_OFF_KP: int32 kp_of_mp[SPFE_PROJ_MAX_POINTS] |
 *   SPFE_PROJ_OFF_UV: float proj_uv[SPFE_PROJ_MAX_POINTS][2] | SPFE_PROJ_OFF_COS: float view_cos[SPFE_PROJ_MAX_POINTS] |
 *   SPFE_PROJ_OFF_VIEW: uint8 in_view[SPFE_PROJ_MAX_POINTS]; entries at and beyond n are not written. */
#define SPFE_PROJ_OFF_KP 64
#define SPFE_PROJ_OFF_UV (SPFE_PROJ_OFF_KP + SPFE_PROJ_MAX_POINTS * 4)
#define SPFE_PROJ_OFF_COS (SPFE_PROJ_OFF_UV + SPFE_PROJ_MAX_POINTS * 8)
#define SPFE_PROJ_OFF_VIEW (SPFE_PROJ_OFF_COS + SPFE_PROJ_MAX_POINTS * 4)
#define SPFE_PROJ_OUT_BYTES ((SPFE_PROJ_OFF_VIEW + SPFE_PROJ_MAX_POINTS + 255) / 256 * 256)
SPFE_API size_t spfe_proj_out_bytes(spfe_handle h);
/* Against ONE record resident in HBM: K, kp_xy, occ_grid and the descriptors (f32, or bf16 with SPFE_FLAG_DESC_BF16: widened
 * exactly) are read on the device; d_xyz / d_normal (float [n][3]; d_normal may be NULL in LAST_FRAME mode) / d_desc (float
 * [n][256]) / d_flags (uint8 [n]) / d_Tcw (float [16]) and d_mp_of_kp — the int32 [kmax] array
 * spfe_refine_pose_record_device takes, updated in place; a value outside [0, n) is never used as an index — are device
 * arrays of exactly these sizes; d_out one block above.  Three launches back to
 * back on `stream` (NULL = the handle's), no host synchronisation. */
SPFE_API int spfe_search_projection_record_device(spfe_handle h, const void *d_record, const void *d_xyz,
                                                  const void *d_normal, const void *d_desc, const void *d_flags, int n,
                                                  void *d_mp_of_kp, const void *d_Tcw, const spfe_proj_params *prm,
                                                  void *d_out, void *stream);
/* The batch path's form: n_frames searches in the same three launches.  Frame f: record f of d_records (spfe_record_bytes()
 * strided), d_n_points[f] (int32, <= SPFE_PROJ_MAX_POINTS: larger counts are clamped on the device) points at
 * d_xyz / d_normal + f * points_stride * 3 floats, d_desc + f * points_stride * 256 floats, d_flags + f * points_stride bytes,
 * d_mp_of_kp + f * kmax, d_Tcw + 16 f, d_out + f * SPFE_PROJ_OUT_BYTES.  points_stride <= SPFE_PROJ_MAX_POINTS.
 * Sizes: d_xyz / d_normal float [n_frames][points_stride][3], d_desc float [n_frames][points_stride][256], d_flags uint8
 * [n_frames][points_stride] (rows at and beyond d_n_points[f] of a frame's slice are not read), d_n_points int32 [n_frames],
 * d_mp_of_kp int32 [n_frames][kmax], d_Tcw float [n_frames][16], d_out n_frames * SPFE_PROJ_OUT_BYTES. */
SPFE_API int spfe_search_projection_batch_device(spfe_handle h, const void *d_records, int n_frames, const void *d_xyz,
                                                 const void *d_normal, const void *d_desc, const void *d_flags,
                                                 const void *d_n_points, size_t points_stride, void *d_mp_of_kp,
                                                 const void *d_Tcw, const spfe_proj_params *prm, void *d_out, void *stream);
/* Tracking::TrackLocalMap (tracker.cpp:561-615) on ONE resident record: the search above in SPFE_PROJ_LOCAL_MAP mode
 * (SearchLocalPoints), Optimizer::PoseOptimization — the pose kernel with SPFE_POSE_OPTIMIZATION over the updated d_mp_of_kp,
 * from d_Tcw — and mnMatchesInliers (:576-588): the keypoints that hold a map point, are not outliers, and whose point has
 * SPFE_PROJ_OBSERVED.  d_pose_out receives the pose block with int32 verdict = SPFE_TRACK_OK when n_inliers >= th_ninlier
 * (the caller passes tracking::map::th_ninlier_low, or th_ninlier_high shortly after a relocalisation), else
 * SPFE_TRACK_FAIL_LOCAL_INLIERS; int32 n_matches = the search's; and, behind it at byte 64 + 36, int32 n_inliers.  The pose
 * is NOT reset on failure: TrackLocalMap keeps what PoseOptimization set.  A record with SPFE_STATUS_COV_OVERFLOW is refused
 * as the pose forms refuse it: nothing searched, d_mp_of_kp untouched, the pose echoed, SPFE_TRACK_FAIL_COV.  All launches
 * back to back on `stream`, no host synchronisation.  pose_prm's schedule must be SPFE_POSE_OPTIMIZATION, proj_prm's mode
 * SPFE_PROJ_LOCAL_MAP.
 * The holder rule of the chain, the same in every step: a value of d_mp_of_kp outside [0, n) counts as none.  The search
 * leaves it alone (unless a point takes the keypoint), PoseOptimization makes no edge of it — it is not in n_initial, its
 * outlier flag stays 0, no row of d_xyz is read for it —, and it is no inlier.  With n == 0 every holder is such a value.
 * The arrays are those of spfe_search_projection_record_device, at its sizes; d_proj_out SPFE_PROJ_OUT_BYTES, d_pose_out
 * spfe_pose_out_bytes(h). */
#define SPFE_TRACK_FAIL_LOCAL_INLIERS 5 /* mnMatchesInliers < th_ninlier (tracker.cpp:607-612) */
#define SPFE_POSE_OFF_N_INLIERS (64 + 36)
SPFE_API int spfe_track_local_map_record_device(spfe_handle h, const void *d_record, const void *d_xyz, const void *d_normal,
                                                const void *d_desc, const void *d_flags, int n, void *d_mp_of_kp,
                                                const void *d_Tcw, const spfe_proj_params *proj_prm,
                                                const spfe_pose_params *pose_prm, int th_ninlier, void *d_proj_out,
                                                void *d_pose_out, void *stream);

/* ---- the tracker's fallback steps: TrackWithMotionModel and trackReferenceKeyFrameANN ---------------
 * Tracking::track() (tracker.cpp:182-233) tries trackFrameDustKFLocal (spfe_track_dust_refine_record_device), on failure
 * TrackWithMotionModel, on failure trackReferenceKeyFrameANN, and after any success TrackLocalMap
 * (spfe_track_local_map_record_device).  The two fallbacks, each as ONE call on a resident record: every launch back to back
 * on `stream` (NULL = the handle's), no host synchronisation, no host decision; the post-call state is the reference's.
 * Both end in Optimizer::PoseOptimization from d_Tcw (pose_prm's schedule must be SPFE_POSE_OPTIMIZATION) and the
 * reference's "Discard outliers" loop (tracker.cpp:519-535, :395-410): every keypoint that holds a point and is an outlier
 * gets d_mp_of_kp[k] = -1 and outlier[k] = 0 (n_outliers counts them), n_inliers counts the remaining holders whose point has
 * SPFE_PROJ_OBSERVED, and the verdict is SPFE_TRACK_OK when n_inliers >= th_nmatch_opt (tracking::motion::th_nmatch_opt, 10).
 * The pose is NOT reset on failure: the reference keeps what PoseOptimization set.  A record with SPFE_STATUS_COV_OVERFLOW
 * is refused: nothing searched or matched, d_mp_of_kp all -1, the pose echoed, all counts 0, SPFE_TRACK_FAIL_COV.
 * d_mp_of_kp, int32 [kmax], is an OUTPUT here: what it held on entry is not read, all kmax entries are written.  What the
 * chain itself writes there lies in [0, n) or is -1, and PoseOptimization applies the holder rule stated at
 * spfe_track_local_map_record_device.  d_xyz float [n][3], d_desc float [n][256], d_flags uint8 [n], d_Tcw float [16]. */
#define SPFE_TRACK_FAIL_MOTION_INLIERS 6 /* TrackWithMotionModel: nmatchesMap < th_nmatch_opt (tracker.cpp:558) */
#define SPFE_TRACK_FAIL_REFKF_INLIERS 7  /* trackReferenceKeyFrameANN: nmatchesMap < th_nmatch_opt (tracker.cpp:416) */
#define SPFE_POSE_OFF_WIDENED (64 + 40)    /* int32: 1 when the search with 2 th stands, else 0 */
#define SPFE_POSE_OFF_N_OUTLIERS (64 + 44) /* int32: keypoints the discard loop emptied */
/* Tracking::TrackWithMotionModel (tracker.cpp:480-559) on ONE resident record.  d_xyz / d_desc / d_flags: the last frame's
 * non-outlier map points in keypoint order, as spfe_search_projection_record_device takes them in SPFE_PROJ_LAST_FRAME mode
 * (proj_prm's mode; proj_prm->th = tracking::motion::th_window_size, 15); d_Tcw = mVelocity * mLastFrame.mTcw.
 *   d_mp_of_kp = -1 (:489); the search with radius th (:499); if its n_matches < th_nmatch_proj
 *   (tracking::motion::th_nmatch_proj, 20), decided on the device: d_mp_of_kp = -1 again and the search with 2 th (:503-508)
 *   — of the first search nothing remains then, neither in d_mp_of_kp nor in d_proj_out; PoseOptimization (:517); the discard
 *   loop (:520-535); verdict SPFE_TRACK_OK or SPFE_TRACK_FAIL_MOTION_INLIERS (:558).
 * d_mp_of_kp and d_proj_out equal, bit for bit, what spfe_search_projection_record_device leaves when it is called with th,
 * its n_matches is read on the host, and it is called again on a cleared d_mp_of_kp with 2 th when that is too small.
 * The pose block's n_matches is that of the search that stands, `widened` says which (a refused record: 0).  A discarded
 * keypoint is still recoverable: kp_of_mp[i] of d_proj_out names it, and d_mp_of_kp[kp_of_mp[i]] != i.  2 th beyond
 * SPFE_PROJ_MAX_RADIUS, a wrong mode or schedule, or a null argument: SPFE_EINVAL before any launch.  Records made with
 * SPFE_FLAG_DESC_BF16 are accepted, as the search accepts them. */
SPFE_API int spfe_track_motion_model_record_device(spfe_handle h, const void *d_record, const void *d_xyz, const void *d_desc,
                                                   const void *d_flags, int n, void *d_mp_of_kp, const void *d_Tcw,
                                                   const spfe_proj_params *proj_prm, const spfe_pose_params *pose_prm,
                                                   int th_nmatch_proj, int th_nmatch_opt, void *d_proj_out, void *d_pose_out,
                                                   void *stream);
/* Tracking::trackReferenceKeyFrameANN (tracker.cpp:372-417) with SPMatcher::SearchByBruteForce(KeyFrame *, Frame &, ...)
 * (sp_matcher.cpp:1642-1674) on ONE resident record and the reference keyframe's record d_kf_record (a record of the SAME
 * handle: same layout, same descriptor format).  d_kf_mp_of_kp, int32 [kmax]: the keyframe's GetMapPointMatches() as indices
 * into d_xyz / d_flags (n points; flags as above, only SPFE_PROJ_OBSERVED is read), -1 for none and for isBad() points; values
 * outside [0, n) count as -1, entries at and beyond the keyframe's K are ignored.  d_Tcw = mLastFrame.mTcw.
 *   The train set is the keyframe's descriptor rows whose keypoint holds a point, in ascending keypoint order (:1654-1660);
 *   the cross-check L2 match of all K rows of the current record against it (:1662-1669) equals spfe_match on those rows
 *   compacted on the host; d_mp_of_kp[q] = d_kf_mp_of_kp[indices_train[train_idx[q]]], -1 for unmatched queries and at and
 *   beyond K (:1671-1673); PoseOptimization (:393); the discard loop (:395-410); verdict SPFE_TRACK_OK or
 *   SPFE_TRACK_FAIL_REFKF_INLIERS (:416).
 * The pose block's n_matches is the number of matched queries (nmatches at :388); `widened` is not written.  An empty train
 * set gives d_mp_of_kp all -1, the pose echoed and the failure verdict. */
SPFE_API int spfe_track_reference_kf_record_device(spfe_handle h, const void *d_record, const void *d_kf_record,
                                                   const void *d_kf_mp_of_kp, const void *d_xyz, const void *d_flags, int n,
                                                   void *d_mp_of_kp, const void *d_Tcw, const spfe_pose_params *pose_prm,
                                                   int th_nmatch_opt, void *d_pose_out, void *stream);

/* ---- mapping: new map points between the current keyframe and its neighbours ----------------------
 * LocalMapping::CreateNewMapPointsOverride (local_mapper.cpp:558-814) with mapping::matching_method 1
 * (SPMatcher::SearchForTriByFlann, sp_matcher.cpp:183-262; methods 0 and 2 are not provided) on resident records: the
 * neighbour's free keypoints (mp_of_kp < 0) take their exact two nearest free rows of the current keyframe, the pairs pass the
 * ratio, epipole and epipolar-line gates (the latter with the record's cov2_inv), every kept pair is triangulated and gated on
 * parallax, depth and the covariance-weighted reprojection error.  include/spfe_tri_math.h is the arithmetic contract, null
 * vector of the 4x4 system included; the results are those of tests/tri_ref/tri_ref.c bit for bit.
 * Keyframe 1 = the current keyframe, keyframe 2 = the neighbour; both records of the SAME handle (same layout, same descriptor
 * format; SPFE_FLAG_DESC_BF16 rows are widened exactly).  d_mp1_of_kp / d_mp2_of_kp: int32 [kmax], in/out: a value < 0 means
 * free; the keypoints of every new point t (t = 0 .. n_new - 1, in ascending k1) receive point_base + t. */
typedef struct spfe_tri_params {
  float fx1, fy1, cx1, cy1;        /* the current keyframe's intrinsics */
  float fx2, fy2, cx2, cy2;        /* the neighbours' */
  float ratio;                     /* 0.7f: d0 < ratio * d1 */
  float epipole_r2;                /* 100: a query within this squared distance of the epipole is refused */
  double chi2_line;                /* 3.84 */
  double chi2_reproj;              /* 5.991 */
  double cos_parallax_max;         /* 0.9998 */
  double min_baseline_depth_ratio; /* 0.01 (the chain form's skip) */
} spfe_tri_params;
#define SPFE_TRI_MAX_NEIGHBOURS 32
/* per-pair verdicts (verdict[k1]); 0: k1 holds no match */
#define SPFE_TRI_VERDICT_NEW 1
#define SPFE_TRI_VERDICT_PARALLAX 2
#define SPFE_TRI_VERDICT_DEGENERATE 3
#define SPFE_TRI_VERDICT_DEPTH 4
#define SPFE_TRI_VERDICT_REPROJ 5
#define SPFE_TRI_STATUS_COV_OVERFLOW 1 /* status: one of the two records carries SPFE_STATUS_COV_OVERFLOW: refused */
/* The output block of ONE neighbour, spfe_tri_out_bytes(h) bytes (a multiple of 256): int32 fields, then per-keypoint arrays
 * of the handle's kmax entries.  match12[k1] = the neighbour's keypoint matched to k1 or -1, verdict[k1] as above; new_xyz
 * [.][3] f32, new_k1, new_k2: the new points in id order — entries at and beyond n_new are NOT written.  n_matches counts every
 * accepted query (the reference's nmatches), also those a later query overwrote.  point_base: the id of this neighbour's first
 * new point.  A neighbour skipped by the baseline test writes the int32 fields only (all counts 0, skipped 1); a refused one
 * (status != 0) writes `status` and nothing else. */
#define SPFE_TRI_OFF_N_MATCHES 0
#define SPFE_TRI_OFF_N_NEW 4
#define SPFE_TRI_OFF_N_REJ_PARALLAX 8
#define SPFE_TRI_OFF_N_REJ_DEPTH 12
#define SPFE_TRI_OFF_N_REJ_REPROJ 16
#define SPFE_TRI_OFF_N_REJ_DEGENERATE 20
#define SPFE_TRI_OFF_SKIPPED 24
#define SPFE_TRI_OFF_STATUS 28
#define SPFE_TRI_OFF_POINT_BASE 32
#define SPFE_TRI_OFF_MATCH12 64
#define SPFE_TRI_OFF_VERDICT(kmax) (64 + 4 * (size_t)(kmax))
#define SPFE_TRI_OFF_NEW_XYZ(kmax) (64 + 8 * (size_t)(kmax))
#define SPFE_TRI_OFF_NEW_K1(kmax) (64 + 20 * (size_t)(kmax))
#define SPFE_TRI_OFF_NEW_K2(kmax) (64 + 24 * (size_t)(kmax))
#define SPFE_TRI_OUT_BYTES(kmax) ((64 + 28 * (size_t)(kmax) + 255) / 256 * 256)
SPFE_API size_t spfe_tri_out_bytes(spfe_handle h);
/* One neighbour: the 2-NN search, the gate, the triangulation and the ordered compaction, all launches back to back on
 * `stream` (NULL = the handle's), no host synchronisation.  d_Tcw1 / d_Tcw2: f32 [16] row-major on the device.  No baseline
 * test is made (no median depth is given).  Null arguments or a negative point_base: SPFE_EINVAL before any launch. */
SPFE_API int spfe_create_map_points_pair_record_device(spfe_handle h, const void *d_record1, const void *d_record2,
                                                       void *d_mp1_of_kp, void *d_mp2_of_kp, const void *d_Tcw1,
                                                       const void *d_Tcw2, const spfe_tri_params *prm, int point_base,
                                                       void *d_out, void *stream);
/* The loop over the neighbours (local_mapper.cpp:592-800) as one call.  d_records2: a HOST array of n_neigh device pointers,
 * one per neighbour record — a keyframe keeps the record it was extracted into, so the neighbours of the covisibility graph
 * are scattered allocations, not a strided array.  Neighbour j uses d_mp2_of_kp + j * kmax, d_Tcw2 + 16 j, d_median_depth[j]
 * (f32 on the device: KeyFrame::ComputeSceneMedianDepth(2)) and writes d_out + j * spfe_tri_out_bytes(h).  It is skipped ON
 * THE DEVICE when baseline / median_depth[j] < min_baseline_depth_ratio (:607-611), sees d_mp1_of_kp as neighbours 0 .. j-1
 * left it, and its ids run on behind theirs.  The result equals, bit for bit, the pair form called per neighbour with the
 * skip decided on the host.  A refused neighbour (SPFE_STATUS_COV_OVERFLOW) is skipped with its status set; a refused current
 * keyframe refuses every neighbour.  n_neigh outside [1, SPFE_TRI_MAX_NEIGHBOURS] or a null argument: SPFE_EINVAL before any
 * launch. */
SPFE_API int spfe_create_map_points_record_device(spfe_handle h, const void *d_record1, const void *const *d_records2,
                                                  int n_neigh, void *d_mp1_of_kp, void *d_mp2_of_kp, const void *d_Tcw1,
                                                  const void *d_Tcw2, const void *d_median_depth,
                                                  const spfe_tri_params *prm, int point_base, void *d_out, void *stream);

/* ---- mapping: the search of SPMatcher::Fuse, map points projected into keyframe records ---------
 * LocalMapping::SearchInNeighbors (local_mapper.cpp:816-904) calls SPMatcher::Fuse(KeyFrame *, const vector<MapPoint *> &,
 * th = 3) (sp_matcher.cpp:965-1104) once per target keyframe and once back into the current one.  The SEARCH of Fuse runs
 * here, on resident records; what Fuse does with a find (Replace, AddObservation, the comparison of observation counts:
 * :1086-1099) needs the whole observation graph and stays with the host, which walks fused_idx[0 .. n_fused) in order.
 * include/spfe_fuse_math.h is the arithmetic contract; the results are those of tests/fuse_ref/fuse_ref.c bit for bit.
 * Monocular only.
 * The target: a record, its pose d_Tcw (f32 [16] row-major) and d_kf_mp_of_kp (int32 [kmax]: the opaque non-negative id of
 * the map point keypoint k holds, or -1; entries at and beyond K are ignored).  It is READ ONLY: one call's result is a
 * function of its inputs, and the host pushes the entries its walk changes back itself.
 * The points, n <= n_cap <= SPFE_PROJ_MAX_POINTS of them: point_id int32 [n] (>= 0), xyz f32 [n][3], normal f32 [n][3]
 * (GetNormal(), not normalised), dist_range f32 [n][2] (mfMinDistance, mfMaxDistance), desc f32 [n][256] (GetDescriptor()),
 * flags uint8 [n] (SPFE_PROJ_SEARCHABLE = !isBad(); other bits are ignored).
 * Records with SPFE_STATUS_COV_OVERFLOW are ACCEPTED: that bit says that cov2 / cov2_inv of the frame are not valid and
 * nothing else — keypoints, occupancy grid and descriptor rows are complete — and Fuse reads no covariance (the level's
 * inverse sigma^2 is 1).  The record's status word is passed through into the block's `status` for the caller's information. */
typedef struct spfe_fuse_params {
  float fx, fy, cx, cy; /* the target keyframes' intrinsics */
  float th;             /* 3: the window radius in pixels; <= SPFE_PROJ_MAX_RADIUS */
  float th_dist;        /* 0.3f (TH_LOW): a best distance above it is refused */
  double chi2;          /* 5.99 */
  double view_cos;      /* 0.5 */
  float min_factor;     /* 0.8f (GetMinDistanceInvariance) */
  float max_factor;     /* 1.2f (GetMaxDistanceInvariance) */
} spfe_fuse_params;
#define SPFE_FUSE_MAX_TARGETS 128 /* 20 covisible keyframes and 5 second neighbours of each: 120 */
/* reason[i]: the first step of spfe_fuse_math.h that refused point i, or SPFE_FUSE_PROPOSED */
#define SPFE_FUSE_SKIP_BAD 1
#define SPFE_FUSE_SKIP_IN_KF 2
#define SPFE_FUSE_BEHIND 3
#define SPFE_FUSE_OUTSIDE 4
#define SPFE_FUSE_RANGE 5
#define SPFE_FUSE_ANGLE 6
#define SPFE_FUSE_NO_CANDIDATE 7
#define SPFE_FUSE_TOO_FAR 8
#define SPFE_FUSE_PROPOSED 9
/* The output block of ONE target over a point capacity n_cap, SPFE_FUSE_OUT_BYTES(n_cap) bytes (a multiple of 256):
 * int32 n_fused | n | status, then at their offsets int32 kp_of_mp[n_cap] (the best keypoint of a proposed point, else -1),
 * f32 best_dist[n_cap] (its distance, else 0), int32 holder[n_cap] (kf_mp_of_kp[kp_of_mp] on entry: -1 = the keypoint is
 * free; -1 for points that are not proposed), int32 fused_idx[n_cap] (the indices of the proposed points, ascending: the
 * first n_fused entries) and uint8 reason[n_cap].  Entries at and beyond n (fused_idx: n_fused) are NOT written. */
#define SPFE_FUSE_OFF_N_FUSED 0
#define SPFE_FUSE_OFF_N 4
#define SPFE_FUSE_OFF_STATUS 8
#define SPFE_FUSE_OFF_KP_OF_MP 64
#define SPFE_FUSE_OFF_BEST_DIST(cap) (64 + 4 * (size_t)(cap))
#define SPFE_FUSE_OFF_HOLDER(cap) (64 + 8 * (size_t)(cap))
#define SPFE_FUSE_OFF_FUSED_IDX(cap) (64 + 12 * (size_t)(cap))
#define SPFE_FUSE_OFF_REASON(cap) (64 + 16 * (size_t)(cap))
#define SPFE_FUSE_OUT_BYTES(cap) ((64 + 17 * (size_t)(cap) + 255) / 256 * 256)
/* Host arrays, synchronous: the target as kp_xy [K][2], occ_grid [H / 8][W / 8] of the handle's frame size, kp_desc [K][256]
 * f32, kf_mp_of_kp [K].  The outputs (each may be NULL) have n entries, fused_idx *n_fused valid ones. */
SPFE_API int spfe_fuse_search(spfe_handle h, const float *kp_xy, const int16_t *occ_grid, const float *kp_desc, int K,
                              const int32_t *kf_mp_of_kp, const float *Tcw, const int32_t *point_id, const float *xyz,
                              const float *normal, const float *dist_range, const float *desc, const uint8_t *flags, int n,
                              const spfe_fuse_params *prm, int32_t *kp_of_mp, float *best_dist, int32_t *holder,
                              uint8_t *reason, int32_t *fused_idx, int *n_fused);
/* One target record: two launches on `stream` (NULL = the handle's), no host synchronisation.  This is also the reverse
 * direction, Fuse(mpCurrentKeyFrame, vpFuseCandidates) (:888), with the current keyframe as the target; more than
 * SPFE_PROJ_MAX_POINTS candidates go in chunks, which is exact because a call changes nothing.  n outside [0, n_cap], n_cap
 * outside [1, SPFE_PROJ_MAX_POINTS], th not in (0, SPFE_PROJ_MAX_RADIUS] or a null argument (the point arrays may be null
 * when n == 0): SPFE_EINVAL before any launch. */
SPFE_API int spfe_fuse_record_device(spfe_handle h, const void *d_record, const void *d_kf_mp_of_kp, const void *d_Tcw,
                                     const void *d_point_id, const void *d_xyz, const void *d_normal,
                                     const void *d_dist_range, const void *d_desc, const void *d_flags, int n, int n_cap,
                                     const spfe_fuse_params *prm, void *d_out, void *stream);
/* The loop over the targets (local_mapper.cpp:854-860) as one call: the same two launches whatever n_targets is.
 * d_records: a HOST array of n_targets device pointers, one per target record (as in spfe_create_map_points_record_device,
 * a keyframe keeps the record it was extracted into); target j uses d_kf_mp_of_kp + j * kmax, d_Tcw + 16 j, the ONE shared
 * point list, and writes d_out + j * SPFE_FUSE_OUT_BYTES(n_cap).  Every target's block equals, byte for byte, the one-target
 * form called with the same inputs.  n_targets outside [1, SPFE_FUSE_MAX_TARGETS], a null record pointer, or what the
 * one-target form refuses: SPFE_EINVAL before any launch. */
SPFE_API int spfe_fuse_targets_record_device(spfe_handle h, const void *const *d_records, int n_targets,
                                             const void *d_kf_mp_of_kp, const void *d_Tcw, const void *d_point_id,
                                             const void *d_xyz, const void *d_normal, const void *d_dist_range,
                                             const void *d_desc, const void *d_flags, int n, int n_cap,
                                             const spfe_fuse_params *prm, void *d_out, void *stream);

/* ---- loop closing: verification of the loop candidates, masked match and Sim3 RANSAC -------------
 * The front half of LoopClosingVLAD::ComputeSim3 (loop_closer_vlad.cpp:345-449) on resident records: per candidate keyframe
 * SPMatcher::SearchByBruteForce(KeyFrame *, KeyFrame *, ...) (sp_matcher_loop.cpp:334-376) — the cross-check L2 match between
 * the rows of the two keyframes that hold a map point — and the hypotheses of a Sim3Solver (sim3_solver.cpp).
 * include/spfe_sim3_math.h is the arithmetic contract (the draws are an INPUT, the eigenvector of Horn's 4x4 matrix is defined
 * there); the results are those of tests/sim3_ref/sim3_ref.c bit for bit.  Keyframe 1 = the current keyframe, keyframe 2 = the
 * candidate.  SearchBySim3Override and SearchByProjectionLoop run behind it on the same records (the guided match and the
 * loop-point search below), and Optimizer::OptimizeSim3 between them (the Sim3 optimisation below).  The NetVLAD candidate
 * detection in front of it is spfe_detect_loop_candidates_device (the detection, further down), CorrectLoop the loop fusion and
 * the essential graph; the host walks the returns. */
typedef struct spfe_sim3_params {
  float fx1, fy1, cx1, cy1; /* the current keyframe's intrinsics */
  float fx2, fy2, cx2, cy2; /* the candidate's */
  float max_err1, max_err2; /* 9.0f: mvnMaxError1/2 are vectors of size_t, 9.210 * sigma2 (= 1) is truncated */
  int min_inliers;          /* 20 (SetRansacParameters(0.99, 20, 300)) */
  int fix_scale;            /* 0 for monocular */
} spfe_sim3_params;
#define SPFE_SIM3_MAX_CANDIDATES 16
#define SPFE_SIM3_MAX_HYPOTHESES 512 /* the reference asks for 300 at the most */
/* The output block of ONE candidate over kmax keypoints and a capacity of hyp_cap hypotheses (the entry points use hyp_cap =
 * n_hyp), SPFE_SIM3_OUT_BYTES(kmax, hyp_cap) bytes (a multiple of 256; the block is 8-byte aligned):
 *   int32 N (pairs) | n_returns | best_h (-1: none) | best_count | n_hyp, then at their offsets
 *   int32 k1[kmax]            mvnIndices1: the keypoint of keyframe 1 of pair i — the first N entries
 *   int32 count[hyp_cap]      inliers of hypothesis h — the first n_hyp
 *   int32 return_idx[hyp_cap] the hypotheses that return a transform, ascending — the first n_returns
 *   f32   T12[hyp_cap][13]    s, R[9] row-major, t[3] — the first n_hyp
 *   uint64 inliers[hyp_cap][SPFE_SIM3_WORDS(kmax)]   bit (i & 63) of word i >> 6: pair i is an inlier — the first n_hyp rows,
 *                             every word of a row
 * Everything else is NOT written.  With N < max(3, min_inliers) nothing is evaluated: the five fields (best_h = -1) and n_hyp
 * zero counts are written, T12 and the inlier words are not.  best_h / best_count are taken over all n_hyp hypotheses: the
 * last h whose count is the largest. */
#define SPFE_SIM3_OFF_N 0
#define SPFE_SIM3_OFF_N_RETURNS 4
#define SPFE_SIM3_OFF_BEST_H 8
#define SPFE_SIM3_OFF_BEST_COUNT 12
#define SPFE_SIM3_OFF_N_HYP 16
#define SPFE_SIM3_OFF_K1 64
#define SPFE_SIM3_WORDS(kmax) (((size_t)(kmax) + 63) / 64)
#define SPFE_SIM3_OFF_COUNT(kmax) (64 + 4 * (size_t)(kmax))
#define SPFE_SIM3_OFF_RETURN_IDX(kmax, hyp_cap) (64 + 4 * (size_t)(kmax) + 4 * (size_t)(hyp_cap))
#define SPFE_SIM3_OFF_T12(kmax, hyp_cap) (64 + 4 * (size_t)(kmax) + 8 * (size_t)(hyp_cap))
#define SPFE_SIM3_OFF_INLIERS(kmax, hyp_cap) ((64 + 4 * (size_t)(kmax) + 60 * (size_t)(hyp_cap) + 7) / 8 * 8)
#define SPFE_SIM3_OUT_BYTES(kmax, hyp_cap) \
  ((SPFE_SIM3_OFF_INLIERS(kmax, hyp_cap) + 8 * (size_t)(hyp_cap) * SPFE_SIM3_WORDS(kmax) + 255) / 256 * 256)
/* SearchByBruteForce between two resident records of the SAME handle (SPFE_FLAG_DESC_BF16 rows are widened exactly): train =
 * the rows of record 1 with d_kf1_mp_of_kp[k] >= 0, queries = the rows of record 2 with d_kf2_mp_of_kp[k] >= 0 (int32 [kmax]
 * each, read only), cross-check.  A masked row computes its distances and neither votes nor receives a result: the result is
 * that of spfe_match on the rows of both sides compacted on the host, every row keeping its keypoint index, ties by order.
 * d_match12: int32 [kmax], match12[k1] = the candidate's keypoint k2 or -1 (all kmax entries are written); d_n_matches: int32,
 * the reference's nmatches.  Records with SPFE_STATUS_COV_OVERFLOW are accepted, as the fuse search accepts them: no
 * covariance is read.  All launches on `stream` (NULL = the handle's), no host synchronisation. */
SPFE_API int spfe_loop_match_record_device(spfe_handle h, const void *d_record1, const void *d_record2,
                                           const void *d_kf1_mp_of_kp, const void *d_kf2_mp_of_kp, void *d_match12,
                                           void *d_n_matches, void *stream);
/* The Sim3Solver of one candidate on device arrays; no record is read.  K1 keypoints of keyframe 1 (0 <= K1 <= kmax);
 * d_match12, d_kf1_mp_of_kp, d_kf2_mp_of_kp: int32 [kmax] of the handle; the map: d_xyz f32 [n][3], d_flags uint8 [n]
 * (SPFE_PROJ_SEARCHABLE = !isBad()), n <= SPFE_PROJ_MAX_POINTS; d_Tcw1 / d_Tcw2 f32 [16]; d_rand_u32 uint32 [n_hyp][3].
 * Three launches (pairs, hypotheses, select) on `stream`; d_out: SPFE_SIM3_OUT_BYTES(kmax, n_hyp) bytes.
 * Entries of d_match12 and d_kf1_mp_of_kp at and beyond K1 are ignored.  A holder outside [0, n) and a match12[k1] outside
 * [0, kmax) are no pair.  The form has no K2: match12[k1] anywhere in [0, kmax) is followed into d_kf2_mp_of_kp, so ALL kmax
 * entries of that array must be an id or -1 — the caller's duty. */
SPFE_API int spfe_sim3_ransac_device(spfe_handle h, int K1, const void *d_match12, const void *d_kf1_mp_of_kp,
                                     const void *d_kf2_mp_of_kp, const void *d_xyz, const void *d_flags, int n,
                                     const void *d_Tcw1, const void *d_Tcw2, const void *d_rand_u32, int n_hyp,
                                     const spfe_sim3_params *prm, void *d_out, void *stream);
/* Host arrays, synchronous: match12 and kf1_mp_of_kp int32 [K1], kf2_mp_of_kp int32 [K2], K1, K2 <= 32767.  out receives the
 * block SPFE_SIM3_OUT_BYTES(max(K1, K2, 1), n_hyp). */
SPFE_API int spfe_sim3_ransac(spfe_handle h, int K1, const int32_t *match12, const int32_t *kf1_mp_of_kp, int K2,
                              const int32_t *kf2_mp_of_kp, const float *xyz, const uint8_t *flags, int n, const float *Tcw1,
                              const float *Tcw2, const uint32_t *rand_u32, int n_hyp, const spfe_sim3_params *prm, void *out);
/* The loop over the candidates (:367-391 and every hypothesis of :395-449) as one call.  d_records2: a HOST array of n_cand
 * device pointers, as in spfe_create_map_points_record_device.  Candidate j uses d_kf2_mp_of_kp + j * kmax, d_Tcw2 + 16 j,
 * d_rand_u32 + j * 3 * n_hyp, and writes d_match12 + j * kmax, d_n_matches + j and d_out + j * SPFE_SIM3_OUT_BYTES(kmax,
 * n_hyp).  Match, pairs, hypotheses and select run back to back on `stream` without host synchronisation or copies; scratch
 * is allocated before the first launch.  Every block, match12 and n_matches equal, byte for byte, the two single forms called
 * per candidate.  Entries of d_kf1_mp_of_kp at and beyond K1, and of candidate j's d_kf2_mp_of_kp at and beyond its K2, are
 * ignored.  The match reads a holder only as >= 0, so a holder >= n is a row of the match; the solver makes no pair of it.
 * n_cand outside [1, SPFE_SIM3_MAX_CANDIDATES], n_hyp outside [1, SPFE_SIM3_MAX_HYPOTHESES], n outside
 * [0, SPFE_PROJ_MAX_POINTS], min_inliers < 0 or a null argument: SPFE_EINVAL before any launch (in all forms). */
SPFE_API int spfe_loop_verify_records_device(spfe_handle h, const void *d_record1, const void *const *d_records2, int n_cand,
                                             const void *d_kf1_mp_of_kp, const void *d_kf2_mp_of_kp, const void *d_xyz,
                                             const void *d_flags, int n, const void *d_Tcw1, const void *d_Tcw2,
                                             const void *d_rand_u32, int n_hyp, const spfe_sim3_params *prm, void *d_match12,
                                             void *d_n_matches, void *d_out, void *stream);
/* Sim3Solver::SetRansacParameters' iteration limit (sim3_solver.cpp:114-138), plain C on the host with the reference's libm
 * calls: max(1, min(ceil(log(1 - probability) / log(1 - pow(eps, 3))), max_iterations)), eps = (float)min_inliers / N; 1 when
 * N == min_inliers.  N < min_inliers (the solver never iterates; the reference's value is undefined there): 1.  No handle. */
SPFE_API int spfe_sim3_iteration_limit(int N, double probability, int min_inliers, int max_iterations);

/* ---- loop closing: the guided match under a Sim3 hypothesis (SearchBySim3Override) ----------------
 * SPMatcher::SearchBySim3Override (sp_matcher_loop.cpp:7-220) as LoopClosingVLAD::ComputeSim3 calls it for a returning
 * hypothesis (loop_closer_vlad.cpp:418-432): the map points of each keyframe are taken through the similarity into the other
 * keyframe, matched in a window of radius th against the descriptor rows of that keyframe's record, and the two directions
 * must agree.  include/spfe_guided_math.h is the arithmetic contract (the masks, the nine steps and their reason codes, the
 * agreement, th_dist, and the one departure: each direction projects with its target's intrinsics); the results are those
 * of tests/guided_ref/guided_ref.c bit for bit.  Keyframe 1 = the current keyframe, keyframe 2 = the candidate.  Monocular
 * only.  Optimizer::OptimizeSim3 reads matches12 from the block on the device (spfe_loop_optimize_sim3_records_device).
 * The map: d_xyz f32 [n][3], d_flags uint8 [n] (SPFE_PROJ_SEARCHABLE = !isBad()), d_dist_range f32 [n][2] (mfMinDistance,
 * mfMaxDistance), d_desc f32 [n][256] (GetDescriptor()), n <= SPFE_PROJ_MAX_POINTS; d_kf1_mp_of_kp / d_kf2_mp_of_kp int32
 * [kmax]: indices into the map or -1, as in spfe_sim3_ransac_device.  Every input is READ ONLY.
 * Records with SPFE_STATUS_COV_OVERFLOW are ACCEPTED, as the fuse search accepts them (no covariance is read); the block's
 * status is the OR of the two records' status words. */
typedef struct spfe_guided_params {
  float fx1, fy1, cx1, cy1; /* the current keyframe's intrinsics (direction 2 -> 1 projects with them) */
  float fx2, fy2, cx2, cy2; /* the candidate's (direction 1 -> 2) */
  float th;                 /* 7.5: the window radius in pixels; <= SPFE_PROJ_MAX_RADIUS */
  float th_dist;            /* 0.7f: a best distance above it is refused */
  float min_factor;         /* 0.8f (GetMinDistanceInvariance) */
  float max_factor;         /* 1.2f (GetMaxDistanceInvariance) */
} spfe_guided_params;
#define SPFE_GUIDED_MAX_JOBS 32
/* reason1[i1] / reason2[i2]: the first step of spfe_guided_math.h that refused the keypoint, or SPFE_GUIDED_MATCHED */
#define SPFE_GUIDED_NO_POINT 1
#define SPFE_GUIDED_ALREADY 2
#define SPFE_GUIDED_SKIP_BAD 3
#define SPFE_GUIDED_BEHIND 4
#define SPFE_GUIDED_OUTSIDE 5
#define SPFE_GUIDED_RANGE 6
#define SPFE_GUIDED_NO_CANDIDATE 7
#define SPFE_GUIDED_TOO_FAR 8
#define SPFE_GUIDED_MATCHED 9
#define SPFE_GUIDED_STATUS_NOT_EVALUATED 0x100 /* batched form: the verify block named by the job holds no hypotheses */
/* The output block of ONE job over kmax keypoints, SPFE_GUIDED_OUT_BYTES(kmax) bytes (a multiple of 256):
 * int32 n_found | n_total | n_seed | status, then at their offsets int32 match1[kmax] (vnMatch1: keyframe 2's keypoint of a
 * MATCHED i1, else -1), int32 match2[kmax] (vnMatch2), f32 dist1[kmax], dist2[kmax] (the best distance of a MATCHED keypoint,
 * else 0), int32 matches12[kmax] (ALL kmax entries are written: -1 at and beyond K1), uint8 reason1[kmax], reason2[kmax].
 * Entries at and beyond K1 (match1, dist1, reason1) / K2 (match2, dist2, reason2) are NOT written. */
#define SPFE_GUIDED_OFF_N_FOUND 0
#define SPFE_GUIDED_OFF_N_TOTAL 4
#define SPFE_GUIDED_OFF_N_SEED 8
#define SPFE_GUIDED_OFF_STATUS 12
#define SPFE_GUIDED_OFF_MATCH1 64
#define SPFE_GUIDED_OFF_MATCH2(kmax) (64 + 4 * (size_t)(kmax))
#define SPFE_GUIDED_OFF_DIST1(kmax) (64 + 8 * (size_t)(kmax))
#define SPFE_GUIDED_OFF_DIST2(kmax) (64 + 12 * (size_t)(kmax))
#define SPFE_GUIDED_OFF_MATCHES12(kmax) (64 + 16 * (size_t)(kmax))
#define SPFE_GUIDED_OFF_REASON1(kmax) (64 + 20 * (size_t)(kmax))
#define SPFE_GUIDED_OFF_REASON2(kmax) (64 + 21 * (size_t)(kmax))
#define SPFE_GUIDED_OUT_BYTES(kmax) ((64 + 22 * (size_t)(kmax) + 255) / 256 * 256)
/* Host arrays, synchronous: keyframe i as kp_xy [Ki][2], occ_grid [H / 8][W / 8] of the handle's frame size, kp_desc
 * [Ki][256] f32, kf_mp_of_kp [Ki]; K1, K2 <= 32767; T12 f32 [13] (s, R row-major, t), seed12 int32 [K1].  `out` is the block
 * over kmax = max(K1, K2, 1); what the call does not write keeps the caller's bytes. */
SPFE_API int spfe_search_by_sim3(spfe_handle h, const float *kp_xy1, const int16_t *occ_grid1, const float *kp_desc1, int K1,
                                 const int32_t *kf1_mp_of_kp, const float *kp_xy2, const int16_t *occ_grid2,
                                 const float *kp_desc2, int K2, const int32_t *kf2_mp_of_kp, const float *xyz,
                                 const uint8_t *flags, const float *dist_range, const float *desc, int n, const float *Tcw1,
                                 const float *Tcw2, const float *T12, const int32_t *seed12, const spfe_guided_params *prm,
                                 void *out);
/* Two resident records of the SAME handle: three launches (prepare, search, agree) on `stream` (NULL = the handle's), no host
 * synchronisation; scratch is allocated before the first launch.  d_T12 f32 [13], d_seed12 int32 [kmax] (entries at and
 * beyond K1 are ignored, as are those of d_kf1_mp_of_kp, and those of d_kf2_mp_of_kp at and beyond K2; a holder outside [0, n)
 * is SPFE_GUIDED_NO_POINT; a negative seed is none, a seed >= K2 marks its k1 as matched already and is carried into
 * matches12, but marks no keypoint of keyframe 2); d_out: SPFE_GUIDED_OUT_BYTES(kmax) bytes.  n outside
 * [0, SPFE_PROJ_MAX_POINTS], th not in (0, SPFE_PROJ_MAX_RADIUS] or a null argument (the map arrays may be null when n == 0): SPFE_EINVAL before any launch. */
SPFE_API int spfe_search_by_sim3_record_device(spfe_handle h, const void *d_record1, const void *d_record2,
                                               const void *d_kf1_mp_of_kp, const void *d_kf2_mp_of_kp, const void *d_xyz,
                                               const void *d_flags, const void *d_dist_range, const void *d_desc, int n,
                                               const void *d_Tcw1, const void *d_Tcw2, const void *d_T12, const void *d_seed12,
                                               const spfe_guided_params *prm, void *d_out, void *stream);
/* The guided matches of n_jobs returning hypotheses as one call behind spfe_loop_verify_records_device, the same three
 * launches whatever n_jobs is.  d_records2: a HOST array of n_cand device pointers; jobs: a HOST array int32 [n_jobs][2] of
 * (candidate, hypothesis).  Job q = (j, hyp) uses d_kf2_mp_of_kp + j * kmax, d_Tcw2 + 16 j, d_match12 + j * kmax and candidate
 * j's verify block d_verify_out + j * SPFE_SIM3_OUT_BYTES(kmax, n_hyp), from which T12[hyp] and the seed are read ON THE
 * DEVICE: seed12[k1[i]] = match12[k1[i]] for every pair i whose inlier bit of hypothesis hyp is set.  It writes d_out + q *
 * SPFE_GUIDED_OUT_BYTES(kmax); every job's block equals, byte for byte, the single form fed with that hypothesis decoded on
 * the host; entries of d_match12 + j * kmax and of the holder arrays at and beyond K1 (K2) are ignored as there.  A verify
 * block that was not evaluated (best_h < 0: too few pairs) gives n_found = n_total = n_seed = 0, matches12
 * all -1 and SPFE_GUIDED_STATUS_NOT_EVALUATED in status; nothing else of the block is written.  n_jobs outside
 * [1, SPFE_GUIDED_MAX_JOBS], n_cand outside [1, SPFE_SIM3_MAX_CANDIDATES], n_hyp outside [1, SPFE_SIM3_MAX_HYPOTHESES], a job
 * naming a candidate >= n_cand or a hypothesis >= n_hyp (or a negative one), or what the single form refuses: SPFE_EINVAL
 * before any launch. */
SPFE_API int spfe_loop_guided_match_records_device(spfe_handle h, const void *d_record1, const void *const *d_records2,
                                                   int n_cand, const int32_t *jobs, int n_jobs, const void *d_kf1_mp_of_kp,
                                                   const void *d_kf2_mp_of_kp, const void *d_xyz, const void *d_flags,
                                                   const void *d_dist_range, const void *d_desc, int n, const void *d_Tcw1,
                                                   const void *d_Tcw2, const void *d_match12, const void *d_verify_out,
                                                   int n_hyp, const spfe_guided_params *prm, void *d_out, void *stream);

/* ---- loop closing: the loop's map points projected into the current keyframe (SearchByProjectionLoop) ----
 * SPMatcher::SearchByProjectionLoop (sp_matcher_loop.cpp:222-332) behind the accepted candidate: the map points of the loop
 * (a LIST, as in the fuse search: point_id int32 [n] unique and >= 0, xyz, normal, dist_range, desc, flags) are projected with
 * the similarity d_Scw (f32 [16] row-major) into ONE record and claim its keypoints in list order.  d_matched int32 [kmax] is
 * IN/OUT: the id keypoint k holds or -1 (mvpCurrentMatchedPoints); entries at and beyond K are ignored and left alone, an entry
 * changes only from -1 to the id of a MATCHED point.  include/spfe_guided_math.h (b) is the contract; the result is that of
 * the sequential loop, tests/guided_ref/guided_ref.c bit for bit.  Records with SPFE_STATUS_COV_OVERFLOW are accepted. */
typedef struct spfe_loop_proj_params {
  float fx, fy, cx, cy; /* the keyframe's intrinsics */
  float th;             /* 10: the window radius in pixels; <= SPFE_PROJ_MAX_RADIUS */
  float th_dist;        /* 0.7f */
  double view_cos;      /* 0.5 */
  float min_factor;     /* 0.8f */
  float max_factor;     /* 1.2f */
} spfe_loop_proj_params;
#define SPFE_LOOPPROJ_SKIP_BAD 1
#define SPFE_LOOPPROJ_ALREADY_FOUND 2
#define SPFE_LOOPPROJ_BEHIND 3
#define SPFE_LOOPPROJ_OUTSIDE 4
#define SPFE_LOOPPROJ_RANGE 5
#define SPFE_LOOPPROJ_ANGLE 6
#define SPFE_LOOPPROJ_NO_CANDIDATE 7
#define SPFE_LOOPPROJ_TOO_FAR 8
#define SPFE_LOOPPROJ_MATCHED 9
/* The ordered claim keeps 5 bytes per keypoint in one workgroup's 160 KB of LDS (beside 96 bytes of its own): K of the
 * host-array form, or num_features + 1 of the record form, <= SPFE_LOOPPROJ_MAX_KEYPOINTS; beyond it SPFE_EINVAL before any
 * launch. */
#define SPFE_LOOPPROJ_MAX_KEYPOINTS 32748 /* 80 static + 5 * 32748 + 16 dynamic bytes = 163,836 of 163,840 */
/* The output block over a point capacity n_cap, SPFE_LOOPPROJ_OUT_BYTES(n_cap) bytes (a multiple of 256): int32 n_matched | n |
 * status, then int32 kp_of_mp[n_cap] (the keypoint a MATCHED point took, else -1), f32 best_dist[n_cap] (its distance, else
 * 0), int32 matched_idx[n_cap] (the indices of the MATCHED points, ascending: the first n_matched) and uint8 reason[n_cap].
 * Entries at and beyond n (matched_idx: n_matched) are NOT written. */
#define SPFE_LOOPPROJ_OFF_N_MATCHED 0
#define SPFE_LOOPPROJ_OFF_N 4
#define SPFE_LOOPPROJ_OFF_STATUS 8
#define SPFE_LOOPPROJ_OFF_KP_OF_MP 64
#define SPFE_LOOPPROJ_OFF_BEST_DIST(cap) (64 + 4 * (size_t)(cap))
#define SPFE_LOOPPROJ_OFF_MATCHED_IDX(cap) (64 + 8 * (size_t)(cap))
#define SPFE_LOOPPROJ_OFF_REASON(cap) (64 + 12 * (size_t)(cap))
#define SPFE_LOOPPROJ_OUT_BYTES(cap) ((64 + 13 * (size_t)(cap) + 255) / 256 * 256)
/* Host arrays, synchronous: kp_xy [K][2], occ_grid of the handle's frame, kp_desc [K][256] f32, matched int32 [K] in/out.  The
 * outputs (each may be NULL) have n entries, matched_idx *n_matched valid ones. */
SPFE_API int spfe_search_loop_points(spfe_handle h, const float *kp_xy, const int16_t *occ_grid, const float *kp_desc, int K,
                                     const float *Scw, int32_t *matched, const int32_t *point_id, const float *xyz,
                                     const float *normal, const float *dist_range, const float *desc, const uint8_t *flags, int n,
                                     const spfe_loop_proj_params *prm, int32_t *kp_of_mp, float *best_dist, uint8_t *reason,
                                     int32_t *matched_idx, int *n_matched);
/* One resident record: two launches (candidates, claim) on `stream`, no host synchronisation, scratch allocated before the
 * first launch.  More than SPFE_PROJ_MAX_POINTS points go in chunks with d_matched carried from call to call (exact: the ids
 * are unique).  n outside [0, n_cap], n_cap outside [1, SPFE_PROJ_MAX_POINTS], th not in (0, SPFE_PROJ_MAX_RADIUS], more
 * keypoints than the claim stage's LDS holds, or a null argument (the point arrays may be null when n == 0): SPFE_EINVAL
 * before any launch. */
SPFE_API int spfe_search_loop_points_record_device(spfe_handle h, const void *d_record, const void *d_Scw, void *d_matched,
                                                   const void *d_point_id, const void *d_xyz, const void *d_normal,
                                                   const void *d_dist_range, const void *d_desc, const void *d_flags, int n,
                                                   int n_cap, const spfe_loop_proj_params *prm, void *d_out, void *stream);

/* ---- loop closing: the Sim3 optimisation of a hypothesis (Optimizer::OptimizeSim3) -----------------------
 * Optimizer::OptimizeSim3 (mapping/optimizer.cpp:1062-1252) as LoopClosingVLAD::ComputeSim3 calls it behind the guided match
 * (loop_closer_vlad.cpp:434-445): the correspondences matches12 of the guided match, two reprojection edges each, a
 * Levenberg-Marquardt solve over the seven parameters of S12 with numeric Jacobians, outlier removal, a second solve.
 * include/spfe_sim3opt_math.h is the arithmetic contract; integers, verdicts and iteration counts are those of
 * tests/sim3opt_ref/sim3opt_ref.c, the transform agrees up to the device's sin / cos / exp in the applied updates.  One
 * workgroup per solve.  Keyframe 1 = the current keyframe, keyframe 2 = the candidate.  Monocular edges only.  The map is
 * d_xyz f32 [n][3], d_flags uint8 [n] (SPFE_PROJ_SEARCHABLE = !isBad()), n <= SPFE_PROJ_MAX_POINTS; every input is READ ONLY.
 * Records with SPFE_STATUS_COV_OVERFLOW are ACCEPTED (no covariance is read); the block's status is the OR of the two
 * records' status words. */
typedef struct spfe_sim3opt_params {
  float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
  float th2;            /* 10 */
  int fix_scale;        /* 0 for monocular */
  int iterations;       /* 5; the second call runs 2 * iterations when nBad > 0 */
  int min_kept;         /* 10 */
  int min_inliers;      /* 20: `accepted` */
} spfe_sim3opt_params;
/* verdict[k1] */
#define SPFE_SIM3OPT_NONE 0     /* matches12[k1] < 0, or k1 >= K1 */
#define SPFE_SIM3OPT_SKIPPED 1  /* not served: no point, a bad point, an id or k2 out of range; matches12 left as it is */
#define SPFE_SIM3OPT_REMOVED 2  /* bad after the first optimize(): matches12 = -1 */
#define SPFE_SIM3OPT_OUTLIER 3  /* bad after the second: matches12 = -1 */
#define SPFE_SIM3OPT_INLIER 4
#define SPFE_SIM3OPT_KEPT 5     /* survived the first round of a solve that stopped there (fewer than min_kept left) */
#define SPFE_SIM3OPT_STATUS_NOT_EVALUATED 0x100 /* batched form: the guided block of the job was not evaluated */
/* The output block of ONE solve over kmax keypoints, SPFE_SIM3OPT_OUT_BYTES(kmax) bytes (a multiple of 256):
 *   int32 n_corr | n_bad | n_in | accepted (n_in >= min_inliers) | iterations[2] | trials[2] | status, then at their offsets
 *   f64 S12[13]   s, R row-major (from the quaternion), t; the widened input when n_corr - n_bad < min_kept
 *   f32 T12_out[13]   the same cast to float (the input's bits when echoed)
 *   f32 Scw[16]   S12 * Sim3(Rcw2, tcw2, 1) as a row-major 4x4 (s R | t): the d_Scw of spfe_search_loop_points_record_device
 *   int32 matches12_out[kmax]   ALL kmax entries are written, -1 at and beyond K1
 *   int32 matched[kmax]   kf2_mp_of_kp[matches12_out[k1]], or -1: the d_matched of spfe_search_loop_points_record_device
 *   uint8 verdict[kmax] */
#define SPFE_SIM3OPT_OFF_N_CORR 0
#define SPFE_SIM3OPT_OFF_N_BAD 4
#define SPFE_SIM3OPT_OFF_N_IN 8
#define SPFE_SIM3OPT_OFF_ACCEPTED 12
#define SPFE_SIM3OPT_OFF_ITERATIONS 16
#define SPFE_SIM3OPT_OFF_TRIALS 24
#define SPFE_SIM3OPT_OFF_STATUS 32
#define SPFE_SIM3OPT_OFF_S12 64
#define SPFE_SIM3OPT_OFF_T12 168
#define SPFE_SIM3OPT_OFF_SCW 224
#define SPFE_SIM3OPT_OFF_MATCHES12 320
#define SPFE_SIM3OPT_OFF_MATCHED(kmax) (320 + 4 * (size_t)(kmax))
#define SPFE_SIM3OPT_OFF_VERDICT(kmax) (320 + 8 * (size_t)(kmax))
#define SPFE_SIM3OPT_OUT_BYTES(kmax) ((320 + 9 * (size_t)(kmax) + 255) / 256 * 256)
/* The solve keeps 3 bytes per keypoint in one workgroup's 160 KB of LDS (every kmax up to 32767 fits).  The edge data of a
 * correspondence (40 bytes) is staged in LDS too while that of all served correspondences fits, and is read from a scratch
 * array otherwise; the result does not depend on which.  spfe_sim3opt_lds_edge_capacity: the most served correspondences of a
 * solve over kmax keypoints (kmax <= 0: the handle's records) whose data is staged in LDS; -1: kmax unsupported. */
SPFE_API int spfe_sim3opt_lds_edge_capacity(spfe_handle h, int kmax);
/* Host arrays, synchronous: kp_xy1 [K1][2], kf1_mp_of_kp int32 [K1], matches12 int32 [K1], kp_xy2 [K2][2], kf2_mp_of_kp int32
 * [K2], Tcw1 / Tcw2 f32 [16], T12 f32 [13] (s, R row-major, t).  `out` receives the block over kmax = max(K1, K2, 1). */
SPFE_API int spfe_optimize_sim3(spfe_handle h, const float *kp_xy1, int K1, const int32_t *kf1_mp_of_kp, const float *kp_xy2,
                                int K2, const int32_t *kf2_mp_of_kp, const float *xyz, const uint8_t *flags, int n,
                                const float *Tcw1, const float *Tcw2, const float *T12, const int32_t *matches12,
                                const spfe_sim3opt_params *prm, void *out);
/* Two resident records of the SAME handle: one launch on `stream` (NULL = the handle's), no host synchronisation; scratch is
 * allocated before the launch.  d_T12 f32 [13], d_matches12 int32 [kmax] (entries at and beyond K1 are ignored, as are those
 * of d_kf1_mp_of_kp, and those of d_kf2_mp_of_kp at and beyond K2); d_out: SPFE_SIM3OPT_OUT_BYTES(kmax) bytes.  n
 * outside [0, SPFE_PROJ_MAX_POINTS], iterations < 1 or a null argument (the map arrays may be null when n == 0): SPFE_EINVAL
 * before any launch. */
SPFE_API int spfe_optimize_sim3_record_device(spfe_handle h, const void *d_record1, const void *d_record2,
                                              const void *d_kf1_mp_of_kp, const void *d_kf2_mp_of_kp, const void *d_xyz,
                                              const void *d_flags, int n, const void *d_Tcw1, const void *d_Tcw2,
                                              const void *d_T12, const void *d_matches12, const spfe_sim3opt_params *prm,
                                              void *d_out, void *stream);
/* The solves of n_jobs hypotheses as ONE launch behind spfe_loop_guided_match_records_device, with the same d_records2, jobs,
 * d_verify_out, n_hyp and d_guided_out.  Job q = (j, hyp) reads T12[hyp] from candidate j's verify block and matches12 from
 * guided block q ON THE DEVICE, uses d_kf2_mp_of_kp + j * kmax and d_Tcw2 + 16 j, and writes d_out + q *
 * SPFE_SIM3OPT_OUT_BYTES(kmax); every job's block equals, byte for byte, the record form fed with that job's T12 and
 * matches12 decoded on the host (the holder arrays beyond K1 / K2 are ignored as there).  A guided block with
 * SPFE_GUIDED_STATUS_NOT_EVALUATED gives all counts 0, accepted 0,
 * iterations and trials 0, matches12_out and matched all -1 and SPFE_SIM3OPT_STATUS_NOT_EVALUATED in status; nothing else of
 * the block is written.  n_jobs outside [1, SPFE_GUIDED_MAX_JOBS], n_cand outside [1, SPFE_SIM3_MAX_CANDIDATES], n_hyp outside
 * [1, SPFE_SIM3_MAX_HYPOTHESES], a job naming a candidate >= n_cand or a hypothesis >= n_hyp (or a negative one), or what the
 * record form refuses: SPFE_EINVAL before any launch. */
SPFE_API int spfe_loop_optimize_sim3_records_device(spfe_handle h, const void *d_record1, const void *const *d_records2,
                                                    int n_cand, const int32_t *jobs, int n_jobs, const void *d_kf1_mp_of_kp,
                                                    const void *d_kf2_mp_of_kp, const void *d_xyz, const void *d_flags, int n,
                                                    const void *d_Tcw1, const void *d_Tcw2, const void *d_verify_out, int n_hyp,
                                                    const void *d_guided_out, const spfe_sim3opt_params *prm, void *d_out,
                                                    void *stream);

/* ---- loop closing: the fusion step of CorrectLoop (SearchAndFuse) and the corrected poses ---------------------
 * LoopClosingVLAD::SearchAndFuse (loop_closer_vlad.cpp:701-726) calls SPMatcher::Fuse(KeyFrame *, cv::Mat Scw, const
 * vector<MapPoint *> &, th = 4, vpReplacePoint) (sp_matcher.cpp:1106-1219) once per keyframe connected to the current one (and
 * for the current one) with the whole list mvpLoopMapPoints and that keyframe's corrected Sim3.  The SEARCH of that Fuse runs
 * here, on resident records; AddObservation / AddMapPoint and pRep->Replace(loopMP) need the observation graph and stay with
 * the host, which walks fused_idx[0 .. n_fused) in order (INTEGRATION.md has the recipe).  It is NOT the mapper's Fuse above: the
 * camera comes out of a similarity (R and t divided by the scale), there is no chi-square gate, best starts at FLT_MAX and the
 * threshold is TH_HIGH.  include/spfe_loopfuse_math.h is the arithmetic contract; the results are those of
 * tests/loopfuse_ref/loopfuse_ref.c bit for bit.  Monocular only.
 * The target: a record, its similarity d_Scw (f32 [16] row-major, [s R | t]) and d_kf_mp_of_kp (int32 [kmax], READ ONLY, as
 * in the fuse search).  The points: the LIST of the fuse search (point_id >= 0, xyz, normal, dist_range, desc, flags), n <=
 * n_cap <= SPFE_PROJ_MAX_POINTS.  Records with SPFE_STATUS_COV_OVERFLOW are ACCEPTED (no covariance is read) and the record's
 * status word is passed through into the block's `status`. */
typedef struct spfe_loop_fuse_params {
  float fx, fy, cx, cy; /* the target keyframes' intrinsics */
  float th;             /* 4: the window radius in pixels; <= SPFE_PROJ_MAX_RADIUS */
  float th_dist;        /* 0.7f (TH_HIGH): a best distance above it is refused */
  double view_cos;      /* 0.5 */
  float min_factor;     /* 0.8f (GetMinDistanceInvariance) */
  float max_factor;     /* 1.2f (GetMaxDistanceInvariance) */
} spfe_loop_fuse_params;
/* reason[i] and the output block of ONE target ARE the fuse search's: the same codes, the same layout. */
#define SPFE_LOOPFUSE_SKIP_BAD SPFE_FUSE_SKIP_BAD
#define SPFE_LOOPFUSE_SKIP_IN_KF SPFE_FUSE_SKIP_IN_KF
#define SPFE_LOOPFUSE_BEHIND SPFE_FUSE_BEHIND
#define SPFE_LOOPFUSE_OUTSIDE SPFE_FUSE_OUTSIDE
#define SPFE_LOOPFUSE_RANGE SPFE_FUSE_RANGE
#define SPFE_LOOPFUSE_ANGLE SPFE_FUSE_ANGLE
#define SPFE_LOOPFUSE_NO_CANDIDATE SPFE_FUSE_NO_CANDIDATE /* the window holds no keypoint */
#define SPFE_LOOPFUSE_TOO_FAR SPFE_FUSE_TOO_FAR           /* ... also a window whose distances are all NaN */
#define SPFE_LOOPFUSE_PROPOSED SPFE_FUSE_PROPOSED
#define SPFE_LOOPFUSE_OFF_N_FUSED SPFE_FUSE_OFF_N_FUSED
#define SPFE_LOOPFUSE_OFF_N SPFE_FUSE_OFF_N
#define SPFE_LOOPFUSE_OFF_STATUS SPFE_FUSE_OFF_STATUS
#define SPFE_LOOPFUSE_OFF_KP_OF_MP SPFE_FUSE_OFF_KP_OF_MP
#define SPFE_LOOPFUSE_OFF_BEST_DIST(cap) SPFE_FUSE_OFF_BEST_DIST(cap)
#define SPFE_LOOPFUSE_OFF_HOLDER(cap) SPFE_FUSE_OFF_HOLDER(cap)
#define SPFE_LOOPFUSE_OFF_FUSED_IDX(cap) SPFE_FUSE_OFF_FUSED_IDX(cap)
#define SPFE_LOOPFUSE_OFF_REASON(cap) SPFE_FUSE_OFF_REASON(cap)
#define SPFE_LOOPFUSE_OUT_BYTES(cap) SPFE_FUSE_OUT_BYTES(cap)
/* A search workgroup serves one target and this many consecutive points (for information: tests step around it). */
#define SPFE_LOOPFUSE_STRIP 64
/* Host arrays, synchronous: the target as kp_xy [K][2], occ_grid [H / 8][W / 8] of the handle's frame size, kp_desc [K][256]
 * f32, kf_mp_of_kp [K], K <= 32767; Scw f32 [16].  The outputs (each may be NULL) have n entries, fused_idx *n_fused valid
 * ones. */
SPFE_API int spfe_loop_fuse_search(spfe_handle h, const float *kp_xy, const int16_t *occ_grid, const float *kp_desc, int K,
                                   const int32_t *kf_mp_of_kp, const float *Scw, const int32_t *point_id, const float *xyz,
                                   const float *normal, const float *dist_range, const float *desc, const uint8_t *flags, int n,
                                   const spfe_loop_fuse_params *prm, int32_t *kp_of_mp, float *best_dist, int32_t *holder,
                                   uint8_t *reason, int32_t *fused_idx, int *n_fused);
/* One target record: two launches on `stream` (NULL = the handle's), no host synchronisation.  d_out:
 * SPFE_LOOPFUSE_OUT_BYTES(n_cap) bytes; entries at and beyond n (fused_idx: n_fused) are NOT written.  More than
 * SPFE_PROJ_MAX_POINTS points go in chunks, which is exact because a call changes nothing.  n outside [0, n_cap], n_cap
 * outside [1, SPFE_PROJ_MAX_POINTS], th not in (0, SPFE_PROJ_MAX_RADIUS] or a null argument (the point arrays may be null
 * when n == 0): SPFE_EINVAL before any launch. */
SPFE_API int spfe_loop_fuse_record_device(spfe_handle h, const void *d_record, const void *d_kf_mp_of_kp, const void *d_Scw,
                                          const void *d_point_id, const void *d_xyz, const void *d_normal,
                                          const void *d_dist_range, const void *d_desc, const void *d_flags, int n, int n_cap,
                                          const spfe_loop_fuse_params *prm, void *d_out, void *stream);
/* The loop over the connected keyframes (loop_closer_vlad.cpp:704-714) as one call: the same two launches whatever n_targets
 * is.  d_records: a HOST array of n_targets device pointers; target j uses d_kf_mp_of_kp + j * kmax, d_Scw + 16 j (f32
 * [n_targets][16]: the d_Siw of spfe_loop_corrected_poses_device), the ONE shared point list, and writes d_out + j *
 * SPFE_LOOPFUSE_OUT_BYTES(n_cap).  Every target's block equals, byte for byte, the one-target form called with the same
 * inputs.  More than SPFE_FUSE_MAX_TARGETS targets go in chunks (exact: a call changes nothing).  n_targets outside [1,
 * SPFE_FUSE_MAX_TARGETS], a null record pointer, or what the one-target form refuses: SPFE_EINVAL before any launch. */
SPFE_API int spfe_loop_fuse_targets_record_device(spfe_handle h, const void *const *d_records, int n_targets,
                                                  const void *d_kf_mp_of_kp, const void *d_Scw, const void *d_point_id,
                                                  const void *d_xyz, const void *d_normal, const void *d_dist_range,
                                                  const void *d_desc, const void *d_flags, int n, int n_cap,
                                                  const spfe_loop_fuse_params *prm, void *d_out, void *stream);
/* The corrected poses of CorrectLoop (loop_closer_vlad.cpp:536-571, :608-618; spfe_loopfuse_math.h (b)): for each of the
 * n_targets connected keyframes with pose Tiw[j] (f32 [n_targets][16]), Siw[j] = toCvMat(Sim3(Tiw[j] * Twc) * Scw) — what
 * SearchAndFuse hands to Fuse — and Tiw_corrected[j] = [R | t / s] of the same product; Scw = S12 * Sim3(Rcw2, tcw2, 1) in
 * double.  Entry cur_index (the current keyframe itself; -1: it is not in the list) takes Scw without a product.  Twc is the
 * current keyframe's GetPoseInverse(), Tcw2 the matched keyframe's pose, both f32 [16].
 * The device form is one launch on `stream`, no host synchronisation: it reads S12 (f64 [13]) at d_opt_block +
 * SPFE_SIM3OPT_OFF_S12, so d_opt_block is an optimise block (8-byte aligned), and d_Siw is directly the d_Scw of
 * spfe_loop_fuse_targets_record_device: the two calls on one stream are the chain.  The host form is a pure function with the
 * same bits.  n_targets outside [1, SPFE_FUSE_MAX_TARGETS], cur_index outside [-1, n_targets) or a null argument:
 * SPFE_EINVAL before any launch. */
SPFE_API int spfe_loop_corrected_poses_device(spfe_handle h, const void *d_opt_block, const void *d_Tcw2, const void *d_Twc,
                                              const void *d_Tiw, int n_targets, int cur_index, void *d_Siw,
                                              void *d_Tiw_corrected, void *stream);
SPFE_API int spfe_loop_corrected_poses(const double *S12, const float *Tcw2, const float *Twc, const float *Tiw, int n_targets,
                                       int cur_index, float *Siw, float *Tiw_corrected);

/* ---- local mapping: bundle adjustment on keyframe records (Schur, Levenberg) ------------------------------------
 * Optimizer::LocalBundleAdjustment (mapping/optimizer.cpp:445-774) as the mapping thread runs it behind SearchInNeighbors
 * (local_mapper.cpp:150-186), and Optimizer::BundleAdjustment (optimizer.cpp:51-229) as MonoTracker::CreateInitialMap runs it
 * (mono_tracker.cpp:170); monocular edges, one camera.  include/spfe_ba_math.h is the arithmetic contract (vertices, edges,
 * the order of every sum, the stale-error rule, the corner cases); integers, verdicts, iteration and trial counts are those of
 * tests/ba_ref/ba_ref.c.  One workgroup per problem, the whole schedule in one launch.  Every input is READ ONLY and the device
 * writes nothing into the map: EraseMapPointMatch / EraseObservation, SetPose, SetWorldPos and UpdateNormalAndDepth stay with
 * the host, which walks erase_idx (INTEGRATION.md has the recipe).
 * Limits, by what one problem keeps:
 *   SPFE_BA_MAX_KEYFRAMES 128   free + fixed, as SPFE_FUSE_MAX_TARGETS: the record pointers are a kernel argument (1 KB) and the
 *                               poses with their backups lie in LDS (128 x 2 x 56 B = 14 KB)
 *   SPFE_BA_MAX_FREE 64         Hpp and bp in LDS (64 x 27 x 8 B = 13.5 KB), four vectors of the 384 unknowns (12 KB); the reduced
 *                               system of 384 x 384 doubles (1.2 MB) then lies in scratch
 *   SPFE_BA_MAX_POINTS 16384    24 doubles + 2 ints a point in scratch: 3.3 MB
 *   SPFE_BA_MAX_EDGES 131072    W (144 B), chi2, observation + information, level, unknown and list entry an edge in scratch: 23.2 MB */
#define SPFE_BA_MAX_KEYFRAMES 128
#define SPFE_BA_MAX_FREE 64
#define SPFE_BA_MAX_POINTS 16384
#define SPFE_BA_MAX_EDGES 131072
#define SPFE_BA_LOCAL 0 /* LocalBundleAdjustment: two rounds, information from cov2_inv, classification, erase list */
#define SPFE_BA_FULL 1  /* BundleAdjustment: one round, information inv_sigma2 * I, no classification */
typedef struct spfe_ba_params {
  float fx, fy, cx, cy;
  int schedule;      /* SPFE_BA_LOCAL | SPFE_BA_FULL */
  int iterations[2]; /* LOCAL: 5, 10; FULL: n, 0 (the second is neither read nor checked); each one read in [0, 1000] */
  int robust;        /* FULL only: Huber with (double)(float)sqrt(5.99); LOCAL is always robust in its first round */
  float inv_sigma2;  /* FULL only: mvInvLevelSigma2[octave], 1 with one pyramid level */
} spfe_ba_params;
/* verdict[e] */
#define SPFE_BA_SKIPPED 0     /* not served: point, slot or keypoint out of range; also every edge of a call that optimised nothing */
#define SPFE_BA_INLIER 1
#define SPFE_BA_LEVEL1_KEPT 2 /* level 1 after the first round, passes the final test */
#define SPFE_BA_ERASE 3       /* in vToErase */
/* status bits (the low bits carry the OR of the records' status words in the record form) */
#define SPFE_BA_STATUS_UNSORTED 0x100
#define SPFE_BA_STATUS_COV_OVERFLOW 0x200  /* LOCAL: a keyframe record carries SPFE_STATUS_COV_OVERFLOW; FULL reads no covariance */
#define SPFE_BA_STATUS_STOPPED_EARLY 0x400 /* *d_stop != 0 on entry */
#define SPFE_BA_STATUS_STOPPED 0x800       /* *d_stop != 0 read before a later iteration */
#define SPFE_BA_STATUS_TOO_MANY_FREE 0x1000 /* record form: more than SPFE_BA_MAX_FREE entries of d_fixed are 0 */
/* The output block, SPFE_BA_OUT_BYTES(n_kf, n, E) bytes (a multiple of 256; bytes not named here keep the caller's):
 *   int32 n_kf | n_free | n_points | n_edges | n_served | iterations[2] | trials[2] | n_level1 | n_erase | status
 *   f64 chi2_entry (the robust chi2 of the first iteration) | chi2_exit (the chi2 the last round holds) | lambda (its last value)
 *   f32 Tcw_out[n_kf][16]   spfe_se3_to_f32 of the estimate; a fixed keyframe's input bit for bit
 *   f32 xyz_out[n][3]
 *   uint8 verdict[E]
 *   int32 erase_idx[E]      n_erase valid entries, in edge order
 * With SPFE_BA_STATUS_UNSORTED, _COV_OVERFLOW, _TOO_MANY_FREE or _STOPPED_EARLY nothing is optimised: Tcw_out and xyz_out are
 * the inputs bit for bit, every verdict is SKIPPED, n_served and the counts behind it are 0. */
#define SPFE_BA_OFF_N_KF 0
#define SPFE_BA_OFF_N_FREE 4
#define SPFE_BA_OFF_N_POINTS 8
#define SPFE_BA_OFF_N_EDGES 12
#define SPFE_BA_OFF_N_SERVED 16
#define SPFE_BA_OFF_ITERATIONS 20
#define SPFE_BA_OFF_TRIALS 28
#define SPFE_BA_OFF_N_LEVEL1 36
#define SPFE_BA_OFF_N_ERASE 40
#define SPFE_BA_OFF_STATUS 44
#define SPFE_BA_OFF_CHI2 64
#define SPFE_BA_OFF_LAMBDA 80
#define SPFE_BA_OFF_TCW 128
#define SPFE_BA_OFF_XYZ(n_kf) (128 + 64 * (size_t)(n_kf))
#define SPFE_BA_OFF_VERDICT(n_kf, n) (128 + 64 * (size_t)(n_kf) + 12 * (size_t)(n))
#define SPFE_BA_OFF_ERASE(n_kf, n, E) (SPFE_BA_OFF_VERDICT(n_kf, n) + ((size_t)(E) + 3) / 4 * 4)
#define SPFE_BA_OUT_BYTES(n_kf, n, E) ((SPFE_BA_OFF_ERASE(n_kf, n, E) + 4 * (size_t)(E) + 255) / 256 * 256)
/* The reduced camera system (6 n_free squared doubles) lies in the workgroup's LDS while it fits beside the poses, Hpp and the
 * partial sums, and in the handle's scratch otherwise; the result does not depend on which.  The most free keyframes of a problem
 * whose system is kept in LDS: */
SPFE_API int spfe_ba_lds_free_capacity(spfe_handle h);
/* Host arrays, synchronous.  edges int32 [E][3] = (point, keyframe slot, keypoint), obs_xy f32 [E][2], inv_sigma2 f32 [E][2]
 * (read by LOCAL only; may be NULL for FULL), Tcw f32 [n_kf][16], fixed uint8 [n_kf], xyz f32 [n][3].  stop: NULL or one int32
 * read when the call starts.  `out` receives the block.  n_kf outside [1, SPFE_BA_MAX_KEYFRAMES], more than SPFE_BA_MAX_FREE
 * keyframes with fixed == 0, n outside [0, SPFE_BA_MAX_POINTS], E outside [0, SPFE_BA_MAX_EDGES], an unknown schedule,
 * iterations outside [0, 1000] or a null argument (edges / obs_xy / inv_sigma2 may be null when E == 0, xyz when n == 0):
 * SPFE_EINVAL before any launch, `out` untouched. */
SPFE_API int spfe_bundle_adjust(spfe_handle h, const int32_t *edges, const float *obs_xy, const float *inv_sigma2, int E,
                                const float *Tcw, const uint8_t *fixed, int n_kf, const float *xyz, int n,
                                const spfe_ba_params *prm, const int32_t *stop, void *out);
/* n_kf resident records of the SAME handle: d_records is a HOST array of n_kf device pointers; the observation and cov2_inv of
 * edge e are read from record edges[e][1] at keypoint edges[e][2], nothing is uploaded.  d_edges int32 [E][3], d_Tcw f32
 * [n_kf][16], d_fixed uint8 [n_kf], d_xyz f32 [n][3], d_stop: NULL or a device-visible int32 read on entry, before every
 * iteration and once between the two rounds (bDoMore).  One launch on `stream` (NULL = the handle's), no host
 * synchronisation; scratch is allocated before the launch.  d_out: SPFE_BA_OUT_BYTES(n_kf, n, E) bytes.  Refusals as above,
 * except that d_fixed is read on the device: more than SPFE_BA_MAX_FREE free keyframes give SPFE_BA_STATUS_TOO_MANY_FREE and
 * nothing is optimised. */
SPFE_API int spfe_local_ba_records_device(spfe_handle h, const void *const *d_records, int n_kf, const void *d_edges, int E,
                                          const void *d_Tcw, const void *d_fixed, const void *d_xyz, int n,
                                          const spfe_ba_params *prm, const void *d_stop, void *d_out, void *stream);

/* ---- the map-point table: descriptor, normal and depth refreshed from resident records -------------------------
 * MapPoint::ComputeDistinctiveDescriptors (type/mappoint.cpp:237-302) and MapPoint::UpdateNormalAndDepth (:322-364), which the
 * reference calls behind every step that changes a point's observations or position (CreateNewMapPoints, SearchInNeighbors'
 * Fuse loops, every bundle adjustment, CorrectLoop, CreateInitialMap).  include/spfe_mappoint_math.h is the arithmetic contract;
 * every output is that of tests/mp_ref/mp_ref.c bit for bit.
 * The TABLE is five device arrays of n_table rows that the caller owns and keeps: xyz f32 [.][3], flags uint8 [.]
 * (SPFE_PROJ_SEARCHABLE = !isBad()), normal f32 [.][3], dist_range f32 [.][2] = (mfMinDistance, mfMaxDistance), desc f32
 * [.][256].  A refresh reads xyz and flags and writes normal, dist_range and desc IN PLACE at the rows of the listed points;
 * it reads no array it writes, so duplicate entries in the list are harmless.  spfe_gather_map_points_device turns table rows
 * into the point LIST the searches take (spfe_fuse_*, spfe_search_loop_points*, spfe_loop_fuse_*,
 * spfe_track_local_map_record_device), so that nothing is uploaded between a refresh and the next search.  AddObservation /
 * EraseObservation / Replace stay host bookkeeping; what they produce is the CSR below (INTEGRATION.md has the recipe).
 * The keyframes: d_kf_records is a DEVICE array of n_kf record pointers (not a kernel argument: a map's keyframe count has no
 * bound of 128, and the caller appends 8 bytes per new keyframe), d_kf_flags uint8 [n_kf] (bit 0 = isBad()), d_Tcw f32
 * [n_kf][16].  A bad keyframe's record pointer may be null; its pose is still read by part (b).
 * The listed points, as a CSR: d_obs_start int32 [m + 1] (ascending, within [0, E]), d_obs int32 [E][2] = (keyframe slot,
 * keypoint) in the order the reference iterates mObservations, d_ref_slot int32 [m] (the slot of mpRefKF), d_point_idx int32
 * [m] (the table row of listed point i) or NULL: row i.
 * code[i], the first that applies:
 *   SKIP_BAD    the table row's flags lack SPFE_PROJ_SEARCHABLE                                       nothing written
 *   NO_OBS      no observation                                                                         nothing written
 *   INVALID     point_idx[i] outside [0, n_table), obs_start not ascending within [0, E], ref_slot or an observation's slot
 *               outside [0, n_kf), a good keyframe's record pointer null, or a keypoint outside [0, K of its record) (not
 *               tested where a bad keyframe's record pointer is null).  Such an index is never followed.  nothing written
 *   NO_GOOD_KF  no observation in a good keyframe                     descriptor kept, normal / dist_range written
 *   TOO_MANY    more than SPFE_MP_MAX_OBS good rows: the host does it descriptor kept, normal / dist_range written
 *   REFRESHED   descriptor, normal and dist_range written
 * mode: SPFE_MP_DESC | SPFE_MP_NORMAL_DEPTH; a part that is not asked for is not written (behind a bundle adjustment only the
 * second is wanted), and NO_GOOD_KF / TOO_MANY are codes of the descriptor: without SPFE_MP_DESC such a point is REFRESHED. */
#define SPFE_MP_MAX_POINTS 262144
#define SPFE_MP_MAX_EDGES 4194304
#define SPFE_MP_MAX_OBS 256
#define SPFE_MP_DESC 1
#define SPFE_MP_NORMAL_DEPTH 2
#define SPFE_MP_SKIP_BAD 1
#define SPFE_MP_NO_OBS 2
#define SPFE_MP_INVALID 3
#define SPFE_MP_NO_GOOD_KF 4
#define SPFE_MP_TOO_MANY 5
#define SPFE_MP_REFRESHED 6
typedef struct spfe_mp_params {
  int mode;          /* SPFE_MP_DESC | SPFE_MP_NORMAL_DEPTH, not 0 */
  float level_scale; /* mvScaleFactors[level of the reference observation]: 1 with one pyramid level */
  float top_scale;   /* mvScaleFactors[nLevels - 1]: 1 */
} spfe_mp_params;
/* The output block, SPFE_MP_OUT_BYTES(m) bytes (a multiple of 256; bytes not named here keep the caller's):
 *   int32 m | n_desc_written | n_nd_written | status   status: the OR of the status words of the table's records (0 in the
 *                                                      host form); records with SPFE_STATUS_COV_OVERFLOW are ACCEPTED
 *   int32 best_obs[m]     the chosen row as an index into the point's OWN observation list; -1 where no descriptor was written
 *   int32 n_good[m]       N; 0 under SKIP_BAD, NO_OBS and INVALID
 *   f32   best_median[m]  BestMedian (FLT_MAX where no row took over); 0 where no descriptor was written
 *   uint8 code[m] */
#define SPFE_MP_OFF_M 0
#define SPFE_MP_OFF_N_DESC 4
#define SPFE_MP_OFF_N_ND 8
#define SPFE_MP_OFF_STATUS 12
#define SPFE_MP_OFF_BEST_OBS 16
#define SPFE_MP_OFF_N_GOOD(m) (16 + 4 * (size_t)(m))
#define SPFE_MP_OFF_BEST_MEDIAN(m) (16 + 8 * (size_t)(m))
#define SPFE_MP_OFF_CODE(m) (16 + 12 * (size_t)(m))
#define SPFE_MP_OUT_BYTES(m) ((16 + 13 * (size_t)(m) + 255) / 256 * 256)
/* Scheduling, for information (tests step around these): a workgroup serves SPFE_MP_CHUNK consecutive listed points; a point of
 * at most SPFE_MP_WAVE_OBS good rows is served by one wavefront, a larger one by the whole workgroup, which stages the rows in
 * LDS while they fit — spfe_mp_lds_obs_capacity(h, 4) f32 rows, (h, 2) bf16 rows — and reads them from the records beyond that.
 * The result does not depend on which path served a point. */
#define SPFE_MP_CHUNK 16
#define SPFE_MP_WAVE_OBS 16
SPFE_API int spfe_mp_lds_obs_capacity(spfe_handle h, int desc_elem_bytes);
/* The record form: two launches on `stream` (NULL = the handle's) whatever m is, no host synchronisation, no allocation.
 * Extents: d_kf_records 8 n_kf bytes, d_kf_flags n_kf, d_Tcw 64 n_kf, d_point_idx 4 m (or NULL), d_obs_start 4 (m + 1), d_obs
 * 8 E, d_ref_slot 4 m, d_xyz 12 n_table, d_flags n_table, d_normal 12 n_table, d_dist_range 8 n_table, d_desc 1024 n_table,
 * d_out SPFE_MP_OUT_BYTES(m); every record spfe_record_bytes.  m outside [0, SPFE_MP_MAX_POINTS], E outside [0,
 * SPFE_MP_MAX_EDGES], n_kf < 1, n_table < 0, a mode that is 0 or has an unknown bit, or a null argument (d_point_idx may always
 * be null; d_obs when E == 0; d_ref_slot when m == 0; the table arrays when n_table == 0): SPFE_EINVAL before any launch, the
 * outputs untouched. */
SPFE_API int spfe_refresh_map_points_device(spfe_handle h, const void *d_kf_records, const void *d_kf_flags, const void *d_Tcw,
                                            int n_kf, const void *d_point_idx, const void *d_obs_start, const void *d_obs,
                                            const void *d_ref_slot, int m, int E, const void *d_xyz, const void *d_flags,
                                            void *d_normal, void *d_dist_range, void *d_desc, int n_table,
                                            const spfe_mp_params *prm, void *d_out, void *stream);
/* Host arrays, synchronous, the observations already gathered: obs_start int32 [m + 1], obs_desc f32 [E][256] (the row of every
 * observation), obs_good uint8 [E] (the keyframe is not bad), obs_Ow f32 [E][3] and ref_Ow f32 [m][3] (camera centres as
 * spfe_proj_cam_from_f32 forms them), xyz f32 [m][3], flags uint8 [m].  Outputs normal f32 [m][3], dist_range f32 [m][2], desc
 * f32 [m][256] — rows that are not written keep the caller's — and `out`, the block.  The same bits as the record form on the
 * same data; INVALID is left to obs_start.  Limits and refusals as above (obs_desc / obs_good / obs_Ow may be null when E == 0,
 * the per-point arrays when m == 0). */
SPFE_API int spfe_refresh_map_points(spfe_handle h, const int32_t *obs_start, const float *obs_desc, const uint8_t *obs_good,
                                     const float *obs_Ow, int E, const float *ref_Ow, const float *xyz, const uint8_t *flags, int m,
                                     const spfe_mp_params *prm, float *normal, float *dist_range, float *desc, void *out);
/* Table rows d_idx int32 [n] -> the point LIST of the searches, contiguous: point_id int32 [n] (= idx[i]), xyz f32 [n][3], normal
 * f32 [n][3], dist_range f32 [n][2], desc f32 [n][256], flags uint8 [n].  An index outside [0, n_table) is not followed: its row
 * is all zero — flags 0, not searchable — under its own point_id.  One launch on `stream`, no host synchronisation.  n outside
 * [0, SPFE_MP_MAX_POINTS], n_table < 0 or a null argument (all arrays may be null when n == 0, the table arrays when n_table ==
 * 0): SPFE_EINVAL before the launch. */
SPFE_API int spfe_gather_map_points_device(spfe_handle h, const void *d_idx, int n, const void *d_xyz, const void *d_flags,
                                           const void *d_normal, const void *d_dist_range, const void *d_desc, int n_table,
                                           void *d_point_id, void *d_list_xyz, void *d_list_normal, void *d_list_dist_range,
                                           void *d_list_desc, void *d_list_flags, void *stream);

/* ---- loop closing: the essential graph over Sim3 and the map corrections --------------------------------------------------
 * Optimizer::OptimizeEssentialGraph (mapping/optimizer.cpp:776-1060) and the two map-point corrections of
 * LoopClosingVLAD::CorrectLoop (loop_closer_vlad.cpp:575-606, optimizer.cpp:1029-1059).  include/spfe_essgraph_math.h is the
 * arithmetic contract (vertices, edges, Sim3::log, the order of every sum, the block skyline Cholesky, the schedule); integers
 * and counts are those of tests/eg_ref/eg_ref.c.  Which edges exist, UpdateConnections, AddLoopEdge and mnCorrectedByKF stay with
 * the host (INTEGRATION.md has the recipe).
 * The graph: Scw_est / Scw_meas f64 [n][8] = q(x, y, z, w), t, s per slot; flags uint8 [n], bit 0 = fixed; edges int32 [E][3] =
 * (i, j, kind), kind 0: measured on Scw_est, 1: on Scw_meas.  An edge with a slot outside [0, n), i == j or another kind is never
 * followed (n_skipped).  The slot order is the elimination order.
 * Limits: n in [1, SPFE_ESSGRAPH_MAX_KEYFRAMES], E in [0, SPFE_ESSGRAPH_MAX_EDGES], env_cap in [0, SPFE_ESSGRAPH_MAX_BLOCKS]
 * (the envelope exists twice at 392 bytes a block: 617 MB at the limit, beside 924 bytes an edge — 242 MB — and 2,064 bytes a
 * keyframe — 34 MB: under 1 GiB of scratch in all), iterations in [0, 1000], lambda_init >= 0 and finite. */
#define SPFE_ESSGRAPH_MAX_KEYFRAMES 16384
#define SPFE_ESSGRAPH_MAX_EDGES 262144
#define SPFE_ESSGRAPH_MAX_BLOCKS 786432
#define SPFE_ESSGRAPH_OK 0
#define SPFE_ESSGRAPH_EMPTY 1              /* no unknown: estimates echoed, poses recovered */
#define SPFE_ESSGRAPH_ENVELOPE_OVERFLOW 2  /* env_blocks > env_cap: nothing solved, estimates echoed, poses recovered */
typedef struct spfe_essgraph_params {
  int iterations;     /* 20 */
  int fix_scale;      /* 0 (monocular) */
  double lambda_init; /* 1e-16 */
} spfe_essgraph_params;
/* The output block, SPFE_ESSGRAPH_OUT_BYTES(n) bytes (a multiple of 256; bytes not named here are not written):
 *   int32 status, n_unknown, n_edges_followed, n_skipped, env_blocks, iterations, trials, n_solve_failed
 *   f64   chi2_initial, chi2_final, lambda_final     (EMPTY / ENVELOPE_OVERFLOW: 0, 0, lambda_init; iterations = trials = 0)
 *   f64   Sim3 [n][8]     the optimised Scw, as the inputs are laid out
 *   f32   Tiw  [n][16]    [R | t / s; 0 0 0 1] of the same */
#define SPFE_ESSGRAPH_OFF_STATUS 0
#define SPFE_ESSGRAPH_OFF_N_UNKNOWN 4
#define SPFE_ESSGRAPH_OFF_N_FOLLOWED 8
#define SPFE_ESSGRAPH_OFF_N_SKIPPED 12
#define SPFE_ESSGRAPH_OFF_ENV_BLOCKS 16
#define SPFE_ESSGRAPH_OFF_ITERATIONS 20
#define SPFE_ESSGRAPH_OFF_TRIALS 24
#define SPFE_ESSGRAPH_OFF_N_SOLVE_FAILED 28
#define SPFE_ESSGRAPH_OFF_CHI2_INITIAL 32
#define SPFE_ESSGRAPH_OFF_CHI2_FINAL 40
#define SPFE_ESSGRAPH_OFF_LAMBDA_FINAL 48
#define SPFE_ESSGRAPH_OFF_SIM3 64
#define SPFE_ESSGRAPH_OFF_TIW(n) (64 + 64 * (size_t)(n))
#define SPFE_ESSGRAPH_OUT_BYTES(n) ((64 + 128 * (size_t)(n) + 255) / 256 * 256)
/* The symbolic step, pure host C: the unknowns (non-fixed slots with a followed edge, in slot order) and first_out[u] (may be
 * NULL; room for n), the least unknown adjacent to u or u itself -> the block count of the envelope the device will need, from
 * which the host sizes env_cap (and may try another slot order); < 0: SPFE_EINVAL. */
SPFE_API int spfe_essential_graph_envelope(int n, const uint8_t *flags, const int32_t *edges, int E, int32_t *first_out,
                                           int *n_unknown, int *n_blocks);
/* The most block rows of one column panel of the factorisation that are staged in LDS; a longer panel is read from the
 * envelope.  The result does not depend on which path ran. */
SPFE_API int spfe_essgraph_lds_panel_capacity(spfe_handle h);
/* The graph's start values from the poses, two launches on `stream`: for every slot Scw_est = Scw_meas = Sim3(Rcw, tcw, 1) of
 * d_Tcw f32 [n][16] (for a connected slot: the pose BEFORE the correction); then for the n_conn slots of d_conn_slot int32 (each
 * at most once; one outside [0, n) is not followed) Scw_est = Sim3(Tiw * Twc) * Scw in double, Scw = S12 * Sim3(Rcw2, tcw2, 1)
 * with S12 read at d_opt_block + SPFE_SIM3OPT_OFF_S12 — what spfe_loop_corrected_poses_device forms before it narrows; slot
 * cur_slot (-1: none) takes Scw itself.  The host form is a pure function with the same bits.  n outside the limit, n_conn
 * outside [0, n], cur_slot outside [-1, n) or a null argument (d_conn_slot may be null when n_conn == 0): SPFE_EINVAL before any
 * launch. */
SPFE_API int spfe_essential_graph_sim3_device(spfe_handle h, const void *d_Tcw, const void *d_opt_block, const void *d_Tcw2,
                                              const void *d_Twc, const void *d_conn_slot, int n_conn, int cur_slot, void *d_Scw_est,
                                              void *d_Scw_meas, int n, void *stream);
SPFE_API int spfe_essential_graph_sim3(const float *Tcw, const double *S12, const float *Tcw2, const float *Twc,
                                       const int32_t *conn_slot, int n_conn, int cur_slot, double *Scw_est, double *Scw_meas, int n);
/* The optimisation: launches on `stream` (NULL = the handle's), no host synchronisation; the scratch is allocated before the
 * first launch.  Extents: d_Scw_est, d_Scw_meas 64 n, d_flags n, d_edges 12 E, d_out SPFE_ESSGRAPH_OUT_BYTES(n); every input is
 * READ ONLY.  Beyond a limit, n < 1, or a null argument (d_edges may be null when E == 0): SPFE_EINVAL before any launch, d_out
 * untouched. */
SPFE_API int spfe_optimize_essential_graph_device(spfe_handle h, const void *d_Scw_est, const void *d_Scw_meas, const void *d_flags,
                                                  int n, const void *d_edges, int E, int env_cap, const spfe_essgraph_params *prm,
                                                  void *d_out, void *stream);
/* ... on host arrays, synchronous; the same bytes. */
SPFE_API int spfe_optimize_essential_graph(spfe_handle h, const double *Scw_est, const double *Scw_meas, const uint8_t *flags, int n,
                                           const int32_t *edges, int E, int env_cap, const spfe_essgraph_params *prm, void *out);
/* The map-point correction, one launch, one thread per listed point: row = d_point_idx[i] (NULL: row i) of the table, r =
 * d_ref_slot[i]; xyz[row] = inverse(S_to[r]).map(S_from[r].map(xyz[row])) in place, S_from / S_to f64 [n_kf][8].  code uint8 [m],
 * the first that applies:
 *   INVALID    the row lies outside [0, n_table)                 nothing read or written
 *   SKIP_BAD   the row's flags lack SPFE_PROJ_SEARCHABLE          nothing written
 *   INVALID    r lies outside [0, n_kf)                           nothing written
 *   CORRECTED
 * A row may be listed at most once per call (the reference's mnCorrectedByKF guarantees it); the host form checks it and
 * refuses, the device form does not.  Chains, nothing uploaded in between: spfe_essential_graph_sim3_device, this with
 * (Scw_meas, Scw_est), spfe_refresh_map_points_device(SPFE_MP_NORMAL_DEPTH); and spfe_optimize_essential_graph_device, this
 * with (Scw_est, d_out + SPFE_ESSGRAPH_OFF_SIM3), a refresh with d_Tcw = d_out + SPFE_ESSGRAPH_OFF_TIW(n).
 * m outside [0, SPFE_MP_MAX_POINTS], n_kf < 1, n_table < 0 or a null argument (d_point_idx may always be null; the per-point
 * arrays when m == 0; the table when n_table == 0): SPFE_EINVAL before the launch, outputs untouched. */
#define SPFE_EGC_SKIP_BAD 1
#define SPFE_EGC_INVALID 2
#define SPFE_EGC_CORRECTED 3
SPFE_API int spfe_correct_map_points_device(spfe_handle h, const void *d_S_from, const void *d_S_to, int n_kf, const void *d_ref_slot,
                                            const void *d_point_idx, int m, void *d_xyz, const void *d_flags, int n_table,
                                            void *d_code, void *stream);
SPFE_API int spfe_correct_map_points(spfe_handle h, const double *S_from, const double *S_to, int n_kf, const int32_t *ref_slot,
                                     const int32_t *point_idx, int m, float *xyz, const uint8_t *flags, int n_table, uint8_t *code);

/* ---- loop closing: the detection, NetVLAD retrieval and the scoring of its candidates ----------------------------------------
 * LoopClosingVLAD::detectLoopCandidates (loop_closer_vlad.cpp:42-118) and the minimum score of detectLoopVLAD (:150-165): the one
 * step of the loop thread that runs for EVERY keyframe.  include/spfe_loopdet_math.h is the arithmetic contract (the sum of the
 * dot product is defined there); the block is that of tests/loopdet_ref/loopdet_ref.c bit for bit.  The consistency groups
 * (:187-241) need the covisibility sets of the graph and stay with the host (INTEGRATION.md has the recipe).
 * The caller keeps on the device, indexed by keyframe SLOT — slot order is the order of db_frames —:
 *   d_gdesc    f32   [n_slots][dim]    the global descriptors, one row appended per keyframe
 *   d_kf_flags uint8 [n_slots]         bit 0 = isBad() (the array of the map-point refresh)
 *   d_in_db    uint8 [n_slots]         non-zero = a member of db_frames
 *   d_best_cov int32 [n_slots][SPFE_LOOPDET_NEIGH]   GetBestCovisibilityKeyFrames(10) in order, -1 padded
 * and gives per query the current keyframe's slot, d_connected int32 [n_conn] = GetConnectedKeyFrames() and d_covisible int32
 * [n_cov] = GetVectorCovisibleKeyFrames(), as slots in any order.  What the call does:
 *   role     a slot is RETRIEVED when it is a db member, is not listed as connected and is not cur_slot — isBad() is not tested,
 *            as in the reference —; it is COVISIBLE when it is listed so and not bad.  A slot with a role is scored once.
 *   min      cov_min_score = the least score of the COVISIBLE slots (+inf: none); min_score = max(min(min_score_init,
 *            cov_min_score), min_score_floor)
 *   pass     the RETRIEVED slots with score > min_score, ascending: pass_slot
 *   acc      per entry acc = best = its score; the entries of its d_best_cov row that passed add their scores in row order and
 *            take over best_slot on a strictly greater score; best_acc_score = the greatest acc, from min_score
 *   retain   min_score_to_retain = retain_ratio * best_acc_score; the entries with acc > min_score_to_retain give their
 *            best_slot, the first occurrence only, in order: cand_slot, cand_acc (the acc of that entry)
 * A list entry outside [0, n_slots) and a row entry outside [0, n_slots) are never followed (-1 is the padding; anything else
 * sets a status bit), and cur_slot is never retrieved even where d_in_db says so.  Every comparison is on f32: a NaN score never
 * passes and never lowers the minimum. */
#define SPFE_LOOPDET_NEIGH 10
#define SPFE_LOOPDET_MAX_KEYFRAMES 65536
#define SPFE_GLOBAL_DESC_DIM 4096
#define SPFE_LOOPDET_BAD_LIST_INDEX 1 /* status: d_connected / d_covisible held a value outside [0, n_slots) */
#define SPFE_LOOPDET_BAD_NEIGHBOUR 2  /* status: the row of an entry that passed held a value outside [-1, n_slots) */
#define SPFE_LOOPDET_NO_SCORE_BITS 0x7FC00000u
typedef struct spfe_loopdet_params {
  float min_score_init;  /* 0.2f */
  float min_score_floor; /* 0.2f (ORB-SLAM2 itself: 0) */
  float retain_ratio;    /* 0.75f */
} spfe_loopdet_params;
/* The output block, SPFE_LOOPDET_OUT_BYTES(n_slots) bytes (a multiple of 256, 16-byte aligned):
 *   int32 status (0 or SPFE_LOOPDET_BAD_* bits), n_scored (slots with a role), n_pass, n_cand
 *   f32   cov_min_score, min_score, best_acc_score, min_score_to_retain
 *   f32   score     [n_slots]   the dot where one was formed, the bits SPFE_LOOPDET_NO_SCORE_BITS elsewhere
 *   int32 pass_slot [n_pass], f32 acc_score [n_pass], int32 best_slot [n_pass]
 *   int32 cand_slot [n_cand], f32 cand_acc [n_cand]
 * and the two working arrays of the call, written whole:
 *   int32 first_pos [n_slots]   the least position in pass_slot of a retained entry whose best keyframe this slot is, INT32_MAX
 *                               where there is none
 *   uint8 role      [n_slots]   SPFE_LOOPDET_ROLE_DB (1) | SPFE_LOOPDET_ROLE_COV (2)
 * Each of the five lists has room for n_slots entries; the entries beyond the valid count, and the bytes behind `role`, are not
 * written. */
#define SPFE_LOOPDET_OFF_STATUS 0
#define SPFE_LOOPDET_OFF_N_SCORED 4
#define SPFE_LOOPDET_OFF_N_PASS 8
#define SPFE_LOOPDET_OFF_N_CAND 12
#define SPFE_LOOPDET_OFF_COV_MIN_SCORE 16
#define SPFE_LOOPDET_OFF_MIN_SCORE 20
#define SPFE_LOOPDET_OFF_BEST_ACC_SCORE 24
#define SPFE_LOOPDET_OFF_MIN_SCORE_TO_RETAIN 28
#define SPFE_LOOPDET_OFF_SCORE 32
#define SPFE_LOOPDET_OFF_PASS_SLOT(n) (32 + 4 * (size_t)(n))
#define SPFE_LOOPDET_OFF_ACC_SCORE(n) (32 + 8 * (size_t)(n))
#define SPFE_LOOPDET_OFF_BEST_SLOT(n) (32 + 12 * (size_t)(n))
#define SPFE_LOOPDET_OFF_CAND_SLOT(n) (32 + 16 * (size_t)(n))
#define SPFE_LOOPDET_OFF_CAND_ACC(n) (32 + 20 * (size_t)(n))
#define SPFE_LOOPDET_OFF_FIRST_POS(n) (32 + 24 * (size_t)(n))
#define SPFE_LOOPDET_OFF_ROLE(n) (32 + 28 * (size_t)(n))
#define SPFE_LOOPDET_OUT_BYTES(n) ((32 + 29 * (size_t)(n) + 255) / 256 * 256)
/* The record form: three launches on `stream` (NULL = the handle's) whatever n_slots is — roles, scores, decisions —, no host
 * synchronisation, no allocation; a row of d_gdesc is read from HBM at most once.  The query is row cur_slot of d_gdesc: append
 * it with an asynchronous copy on the same stream and call.  Extents: d_gdesc 4 dim n_slots bytes, d_kf_flags n_slots, d_in_db
 * n_slots, d_best_cov 40 n_slots, d_connected 4 n_conn, d_covisible 4 n_cov, d_out SPFE_LOOPDET_OUT_BYTES(n_slots); every input is
 * READ ONLY.  n_slots outside [1, SPFE_LOOPDET_MAX_KEYFRAMES], dim outside [4, SPFE_GLOBAL_DESC_DIM] or no multiple of 4, cur_slot
 * outside [0, n_slots), n_conn or n_cov outside [0, n_slots], d_gdesc or d_out not 16-byte aligned, or a null argument (a list may be
 * null when its count is 0):
 * SPFE_EINVAL before any launch, d_out untouched. */
SPFE_API int spfe_detect_loop_candidates_device(spfe_handle h, const void *d_gdesc, int dim, const void *d_kf_flags,
                                                const void *d_in_db, const void *d_best_cov, int n_slots, int cur_slot,
                                                const void *d_connected, int n_conn, const void *d_covisible, int n_cov,
                                                const spfe_loopdet_params *prm, void *d_out, void *stream);
/* ... on host arrays, synchronous; the same bytes (what the call does not write keeps the caller's). */
SPFE_API int spfe_detect_loop_candidates(spfe_handle h, const float *gdesc, int dim, const uint8_t *kf_flags, const uint8_t *in_db,
                                         const int32_t *best_cov, int n_slots, int cur_slot, const int32_t *connected, int n_conn,
                                         const int32_t *covisible, int n_cov, const spfe_loopdet_params *prm, void *out);

/* ---- the tracker's local map: keyframe votes, expansion, ordered point list --------------------------------------------------
 * Tracking::UpdateLocalMap (tracker.cpp:834-984), the one host step left between the tracking calls of a frame, on arrays the
 * caller keeps resident; include/spfe_localmap_math.h is the contract (integers only), and the block is that of
 * tests/localmap_ref/localmap_ref.c byte for byte.  The vote is also KeyFrame::getTrackedInCommon (keyframe.cpp:697-724).
 * THE NAMES END IN _resident, NOT IN _device: the table of tests/graph_forms.py is closed at the 37 forms above.  The contract of
 * the device forms holds all the same — launches on the caller's stream, no host synchronisation, no host decision, scratch sized
 * before the first launch (the handle's, grown by a call larger than any before it: make the largest call first, outside a
 * capture), presets done by a kernel — and tests/test_gpu_local_map_chain.py captures and replays them.
 * The caller keeps on the device, indexed by keyframe SLOT as in the refresh and the loop detection:
 *   d_kf_mp_of_kp int32 [n_slots][kp_stride]   GetMapPointMatches() as map-point table rows, -1 for none; entries at and beyond the
 *                                              keyframe's K stay -1.  A value outside [0, n_table) counts as none, never followed.
 *   d_kf_flags    uint8 [n_slots]              bit 0 = isBad()
 *   d_best_cov    int32 [n_slots][n_best]      GetBestCovisibilityKeyFrames(n_best) as slots, -1 padded; n_best in 1..32 (the
 *                                              reference: 20).  A table of its own: the loop detector's has 10 columns.
 *   d_parent      int32 [n_slots]              GetParent() as a slot, -1 for none
 *   d_mp_flags    uint8 [n_table]              the map-point table's flags (SPFE_PROJ_SEARCHABLE = !isBad())
 *   d_mp_of_kp    int32 [n_kp]                 the current frame's mvpMapPoints as table rows
 * kp_stride is the row pitch in entries: any value in [1, SPFE_LOCALMAP_MAX_STRIDE], no multiple of 4 needed.
 * What the call does (spfe_localmap_math.h (1)-(5)): the frame's holders and their weights, votes and total per slot, the voted
 * set V in ascending slot order and ref_slot, the sequential expansion with the reference's quirks, and the point list — the held
 * points first, then the points of the local keyframes in the reference's order — cut at point_cap. */
#define SPFE_LOCALMAP_MAX_KEYFRAMES 65536
#define SPFE_LOCALMAP_MAX_STRIDE 16384
#define SPFE_LOCALMAP_MAX_BEST 32
#define SPFE_LOCALMAP_NO_VOTES 1  /* status: V is empty; no local keyframes, the list holds the held points only */
#define SPFE_LOCALMAP_TRUNCATED 2 /* status: n_points_total > point_cap */
#define SPFE_LOCALMAP_BAD_SLOT 4  /* status: a d_best_cov or d_parent entry that the walk read was outside [-1, n_slots) */
typedef struct spfe_localmap_params {
  int max_keyframes; /* 80 */
  int point_cap;     /* n_kp <= point_cap <= SPFE_PROJ_MAX_POINTS */
} spfe_localmap_params;
/* The output block, SPFE_LOCALMAP_OUT_BYTES(n_slots, point_cap, n_kp) bytes (a multiple of 256, 16-byte aligned), EVERY byte
 * written by every call:
 *   int32 n_voted, n_local_kf, ref_slot, n_held, n_points, n_points_total, status, 0
 *   int32 local_kf     [n_slots]     L in order, -1 behind n_local_kf
 *   int32 votes        [n_slots], int32 total [n_slots]
 *   int32 point_idx    [point_cap]   table rows, -1 in EVERY entry at and beyond n_points
 *   int32 mp_of_kp_list[n_kp]        the frame's holders as list positions, -1 for none
 * and zeros up to the multiple of 256. */
#define SPFE_LOCALMAP_OFF_N_VOTED 0
#define SPFE_LOCALMAP_OFF_N_LOCAL_KF 4
#define SPFE_LOCALMAP_OFF_REF_SLOT 8
#define SPFE_LOCALMAP_OFF_N_HELD 12
#define SPFE_LOCALMAP_OFF_N_POINTS 16
#define SPFE_LOCALMAP_OFF_N_POINTS_TOTAL 20
#define SPFE_LOCALMAP_OFF_STATUS 24
#define SPFE_LOCALMAP_OFF_LOCAL_KF 32
#define SPFE_LOCALMAP_OFF_VOTES(s) (32 + 4 * (size_t)(s))
#define SPFE_LOCALMAP_OFF_TOTAL(s) (32 + 8 * (size_t)(s))
#define SPFE_LOCALMAP_OFF_POINT_IDX(s) (32 + 12 * (size_t)(s))
#define SPFE_LOCALMAP_OFF_MP_OF_KP_LIST(s, p) (32 + 12 * (size_t)(s) + 4 * (size_t)(p))
#define SPFE_LOCALMAP_OUT_BYTES(s, p, k) ((32 + 12 * (size_t)(s) + 4 * (size_t)(p) + 4 * (size_t)(k) + 255) / 256 * 256)
/* Points whose weight table the vote kernel holds in LDS (one byte a point); beyond it the table is read from global memory,
 * where it sits in L2.  The result does not depend on which. */
SPFE_API int spfe_localmap_lds_point_capacity(spfe_handle h);
/* Steps (1) to (5) into d_out.  Seven launches on `stream` (NULL = the handle's) whatever the sizes are — presets, the frame, the
 * vote, the expansion, the keys, the counts, the list —, no host synchronisation; because the tail of point_idx is -1 and the
 * gather turns such an index into an all-zero, unsearchable row, spfe_gather_map_points_device (n = point_cap) and
 * spfe_track_local_map_record_device (n = point_cap) follow with no count coming back to the host.  Extents: d_kf_mp_of_kp
 * 4 kp_stride n_slots bytes, d_kf_flags n_slots, d_best_cov 4 n_best n_slots, d_parent 4 n_slots, d_mp_flags n_table, d_mp_of_kp
 * 4 n_kp, d_out SPFE_LOCALMAP_OUT_BYTES(n_slots, point_cap, n_kp); every input is READ ONLY.  n_slots outside
 * [1, SPFE_LOCALMAP_MAX_KEYFRAMES], kp_stride outside [1, SPFE_LOCALMAP_MAX_STRIDE], n_best outside
 * [1, SPFE_LOCALMAP_MAX_BEST], n_table outside [0, SPFE_MP_MAX_POINTS], n_kp outside [0, point_cap], point_cap outside
 * [1, SPFE_PROJ_MAX_POINTS], max_keyframes < 0, an int32 array not 4-byte or d_out not 16-byte aligned, or a null argument (an array
 * of a zero count may be null): SPFE_EINVAL before any launch, d_out untouched. */
SPFE_API int spfe_update_local_map_resident(spfe_handle h, const void *d_kf_mp_of_kp, int kp_stride, const void *d_kf_flags,
                                            const void *d_best_cov, int n_best, const void *d_parent, int n_slots,
                                            const void *d_mp_flags, int n_table, const void *d_mp_of_kp, int n_kp,
                                            const spfe_localmap_params *prm, void *d_out, void *stream);
/* Steps (1) and (2) alone, the keypoints with a non-zero d_outlier byte left out of the set: votes[ref] / total[ref] is
 * ratio_in_common of NeedNewKeyFrameOverride (tracker.cpp:624-635), and votes is the count KeyFrame::UpdateConnections takes.
 * Three launches.  Extents: d_kf_mp_of_kp 4 kp_stride n_slots bytes, d_mp_flags n_table, d_mp_of_kp 4 n_kp, d_outlier n_kp (or
 * NULL: no outliers), d_votes 4 n_slots, d_total 4 n_slots; the ranges of the call above, n_kp in [0, SPFE_PROJ_MAX_POINTS]. */
SPFE_API int spfe_count_shared_points_resident(spfe_handle h, const void *d_kf_mp_of_kp, int kp_stride, int n_slots,
                                               const void *d_mp_flags, int n_table, const void *d_mp_of_kp, const void *d_outlier,
                                               int n_kp, void *d_votes, void *d_total, void *stream);
/* List positions back into table rows behind TrackLocalMap, so that the frame's state stays in table rows for the next frame:
 * rows[k] = point_idx[list[k]] where list[k] is in [0, point_cap), -1 elsewhere.  One launch.  Extents: d_point_idx 4 point_cap
 * bytes, d_mp_of_kp_list 4 n_kp, d_mp_of_kp_rows 4 n_kp (written whole); n_kp in [0, SPFE_PROJ_MAX_POINTS], point_cap in
 * [1, SPFE_PROJ_MAX_POINTS]. */
SPFE_API int spfe_local_map_rows_resident(spfe_handle h, const void *d_point_idx, int point_cap, const void *d_mp_of_kp_list,
                                          int n_kp, void *d_mp_of_kp_rows, void *stream);
/* spfe_update_local_map_resident on host arrays, synchronous; the same bytes in the block. */
SPFE_API int spfe_update_local_map(spfe_handle h, const int32_t *kf_mp_of_kp, int kp_stride, const uint8_t *kf_flags,
                                   const int32_t *best_cov, int n_best, const int32_t *parent, int n_slots, const uint8_t *mp_flags,
                                   int n_table, const int32_t *mp_of_kp, int n_kp, const spfe_localmap_params *prm, void *out);

/* ---- the covisibility graph: KeyFrame::UpdateConnections on resident rows -------------------------------------------------------
 * KeyFrame::UpdateConnections (keyframe.cpp:757-849) with AddConnection / UpdateBestCovisibles (:577-612): the routine whose
 * products — GetBestCovisibilityKeyFrames, GetVectorCovisibleKeyFrames, GetConnectedKeyFrames, GetParent — the local map, the
 * loop detection and the mapper's neighbour lists read.  The graph is resident state that this call maintains, so d_best_cov,
 * d_parent, d_connected and d_covisible of the calls above are produced where they are consumed.
 * include/spfe_covis_math.h is the contract (integers only); state, tables and block are those of tests/covis_ref/covis_ref.c
 * byte for byte.  The names end in _resident for the reason given above, and the device forms' contract holds: launches on the
 * caller's stream, no host synchronisation, no host decision, the handle's scratch grown by a call larger than any before it
 * (make the largest call first, outside a capture), presets done by a kernel.
 * The state, caller-allocated, indexed by keyframe slot like d_kf_mp_of_kp:
 *   d_conn_slot, d_conn_w int32 [n_slots][conn_cap]  mConnectedKeyFrameWeights: keys ascending by slot, -1 / 0 behind conn_n
 *   d_conn_n              int32 [n_slots]
 *   d_ord_slot, d_ord_w   int32 [n_slots][conn_cap]  mvpOrderedConnectedKeyFrames / mvOrderedWeights, -1 / 0 behind ord_n
 *   d_ord_n               int32 [n_slots]
 *   d_parent              int32 [n_slots]            mpParent as a slot, -1 for none: the array spfe_update_local_map_resident reads
 *   d_first_conn          uint8 [n_slots]            mbFirstConnection
 * conn_cap in [1, SPFE_COVIS_MAX_CONN]: a row of (weight, slot) keys fits in one workgroup's LDS.  For the keyframe at slot c,
 * d_conn_slot + c * conn_cap and d_ord_slot + c * conn_cap are the d_connected and d_covisible lists of the loop detection (count
 * min(conn_cap, n_slots): its lists skip -1). */
#define SPFE_COVIS_MAX_CONN 4096
#define SPFE_COVIS_NO_SHARED 1      /* status: no keyframe shares a point with cur_slot; no state changed */
#define SPFE_COVIS_CUR_OVERFLOW 2   /* status: n_counter > conn_cap; no state changed, n_counter is the capacity needed */
#define SPFE_COVIS_NEIGH_OVERFLOW 4 /* status: n_overflow linked neighbours were full (code 3) and kept their rows */
typedef struct spfe_covis_graph {
  void *d_conn_slot, *d_conn_w, *d_conn_n;
  void *d_ord_slot, *d_ord_w, *d_ord_n;
  void *d_parent, *d_first_conn;
  int n_slots, conn_cap;
} spfe_covis_graph;
typedef struct spfe_covis_params {
  int th;          /* 15 in the reference; >= 1 */
  int origin_slot; /* the keyframe with mnId == 0 (never given a parent), or -1 */
} spfe_covis_params;
/* The output block, SPFE_COVIS_OUT_BYTES(n_slots, conn_cap) bytes (a multiple of 256, 16-byte aligned), EVERY byte written by
 * every call:
 *   int32 status, n_counter, n_linked, n_changed, n_overflow, max_slot, max_count, parent_set
 *   int32 counter    [n_slots]
 *   int32 linked_slot[conn_cap]   P ascending, -1 behind n_linked
 *   int32 linked_code[conn_cap]   0 same weight, 1 replaced, 2 inserted, 3 full; -1 behind n_linked
 * and zeros up to the multiple of 256.  n_changed counts codes 1 and 2, n_overflow code 3; parent_set is the slot written into
 * d_parent[cur_slot], or -1. */
#define SPFE_COVIS_OFF_STATUS 0
#define SPFE_COVIS_OFF_N_COUNTER 4
#define SPFE_COVIS_OFF_N_LINKED 8
#define SPFE_COVIS_OFF_N_CHANGED 12
#define SPFE_COVIS_OFF_N_OVERFLOW 16
#define SPFE_COVIS_OFF_MAX_SLOT 20
#define SPFE_COVIS_OFF_MAX_COUNT 24
#define SPFE_COVIS_OFF_PARENT_SET 28
#define SPFE_COVIS_OFF_COUNTER 32
#define SPFE_COVIS_OFF_LINKED_SLOT(s) (32 + 4 * (size_t)(s))
#define SPFE_COVIS_OFF_LINKED_CODE(s, c) (32 + 4 * (size_t)(s) + 4 * (size_t)(c))
#define SPFE_COVIS_OUT_BYTES(s, c) ((32 + 4 * (size_t)(s) + 8 * (size_t)(c) + 255) / 256 * 256)
/* The preset of the slots [first_slot, first_slot + n): counts 0, rows -1 / 0, parent -1, first_conn 1.  One launch (no memset
 * node in a capture).  The range outside [0, n_slots], n < 1, conn_cap outside [1, SPFE_COVIS_MAX_CONN], a null or misaligned
 * array: SPFE_EINVAL before the launch. */
SPFE_API int spfe_covis_reset_slots_resident(spfe_handle h, const spfe_covis_graph *graph, int first_slot, int n, void *stream);
/* UpdateConnections of the keyframe at cur_slot (spfe_covis_math.h (1)-(7)).  Five launches on `stream` (NULL = the handle's)
 * whatever the sizes are — the three of spfe_count_shared_points_resident on row cur_slot, one workgroup for the current keyframe
 * (counter, maximum, P, its own rows, parent, tables, the block), and a fixed grid of one workgroup a linked neighbour (lookup,
 * insert or replace, a bitonic sort of the row's keys in LDS, rows and tables) —, no host synchronisation.  d_best_cov_a [n_slots]
 * [n_best_a] and d_best_cov_b [n_slots][n_best_b] are the two tables of step (7) (the local map's 20 columns, the loop
 * detection's 10); either may be NULL, each n_best lies in [1, SPFE_LOCALMAP_MAX_BEST] all the same.  d_kf_mp_of_kp, d_kf_flags
 * and d_mp_flags are READ ONLY.  Extents: d_kf_mp_of_kp 4 kp_stride n_slots bytes, d_kf_flags n_slots, d_mp_flags n_table, the
 * state as above, the tables 4 n_best n_slots, d_out SPFE_COVIS_OUT_BYTES(n_slots, conn_cap).  n_slots, kp_stride and n_table
 * outside the ranges of spfe_update_local_map_resident, cur_slot outside [0, n_slots), conn_cap outside
 * [1, SPFE_COVIS_MAX_CONN], th < 1, origin_slot outside [-1, n_slots), an n_best out of range, an int32 array not 4-byte or
 * d_out not 16-byte aligned, or a null argument (d_mp_flags may be null when n_table is 0): SPFE_EINVAL before any launch, d_out
 * and the state untouched. */
SPFE_API int spfe_update_connections_resident(spfe_handle h, const spfe_covis_graph *graph, const void *d_kf_mp_of_kp, int kp_stride,
                                              const void *d_kf_flags, const void *d_mp_flags, int n_table, int cur_slot,
                                              const spfe_covis_params *prm, void *d_best_cov_a, int n_best_a, void *d_best_cov_b,
                                              int n_best_b, void *d_out, void *stream);
/* The same on host arrays, synchronous: the pointers of `graph` and the two tables are HOST arrays, updated in place; the same
 * bytes in state, tables and block. */
SPFE_API int spfe_update_connections(spfe_handle h, const spfe_covis_graph *graph, const int32_t *kf_mp_of_kp, int kp_stride,
                                     const uint8_t *kf_flags, const uint8_t *mp_flags, int n_table, int cur_slot,
                                     const spfe_covis_params *prm, int32_t *best_cov_a, int n_best_a, int32_t *best_cov_b,
                                     int n_best_b, void *out);

/* ---- keyframe culling: the cull loop of the local mapper and KeyFrame::SetBadFlag on resident rows ---------------------------------
 * LocalMapping::KeyFrameCullingOverride (local_mapper.cpp:979-1032) with the KeyFrame::SetBadFlag it calls (keyframe.cpp:911-997):
 * the last stage of the mapping cycle, and the one that EDITS the arrays every other resident form reads.  include/spfe_cull_math.h
 * is the contract, in numbered steps; rows, flags, observation counts, graph state, tables and block are those of
 * tests/cull_ref/cull_ref.c byte for byte.  The names end in _resident as above, and the device forms' contract holds: launches on
 * the caller's stream, a fixed number of them, no host synchronisation, no host decision, the handle's scratch grown by a call
 * larger than any before it (make the largest call first, outside a capture), presets done by a kernel.
 * d_kf_flags gains two bits here; every other form tests bit 0 alone. */
#define SPFE_KF_BAD 1u          /* bit 0: the slot holds no keyframe, or a culled one */
#define SPFE_KF_NOT_ERASE 2u    /* bit 1: mbNotErase, an INPUT of the cull: the keyframe is chosen and not culled */
#define SPFE_KF_TO_BE_ERASED 4u /* bit 2: mbToBeErased, SET by the cull on a chosen keyframe with bit 1 */
#define SPFE_CULL_STALLED 1      /* status: a pass chose nothing and left keyframes in the list (spfe_cull_math.h (3)) */
#define SPFE_CULL_WILD_ENTRY 2   /* status: the list named a slot outside [0, n_slots) */
#define SPFE_CULL_BAD_CUT 4      /* status: more than bad_cap points went bad; n_bad counts them all */
#define SPFE_CULL_EVENT_CUT 8    /* status: more than n_slots re-parenting events; n_reparented counts them all */
#define SPFE_CULL_NO_PARENT 16   /* status: a culled keyframe had no parent; its left-over children got -1 */
typedef struct spfe_cull_params {
  int th_obs;      /* mapping::kf_culling_num_obs: 3 by default, 5 in the shipped settings; >= 1 */
  float cov_ratio; /* mapping::kf_culling_cov_ratio: 0.9 / 0.95 */
  int origin_slot; /* the keyframe with mnId == 0 (never culled), or -1 */
  int bad_cap;     /* entries of bad_point[] in the block, in [0, SPFE_MP_MAX_POINTS] */
} spfe_cull_params;
/* The output block, SPFE_CULL_OUT_BYTES(n_slots, conn_cap, bad_cap) bytes (a multiple of 256, 16-byte aligned), EVERY byte written
 * by every call:
 *   int32 status, n_listed, n_passes, n_culled, n_deferred, n_touched, n_reparented, n_events, n_bad, n_bad_stored, 0 x 6
 *   int32 entry_slot [conn_cap]   the list as it was read, -1 behind n_listed
 *   int32 entry_code [conn_cap]   SPFE_CULL_CODE_* of spfe_cull_math.h, -1 behind n_listed
 *   int32 entry_pass [conn_cap]   the pass that decided the entry (from 1; 0 = skipped at entry), -1 behind n_listed
 *   int32 entry_mps  [conn_cap]   n_mps and n_red of that pass, 0 for a skipped entry and behind n_listed
 *   int32 entry_red  [conn_cap]
 *   int32 culled_slot[conn_cap]   in cull order, -1 behind n_culled
 *   int32 touched_slot[n_slots]   the neighbours that lost a link, ascending, -1 behind n_touched
 *   int32 event_child[n_slots], event_parent[n_slots]   the re-parenting events in the order they happen (the host's ChangeParent:
 *                                 AddChild / EraseChild, mTcp), -1 behind n_events = min(n_reparented, n_slots)
 *   int32 bad_point  [bad_cap]    the newly bad points (cull order, then first entry in the culled row), -1 behind n_bad_stored
 * and zeros up to the multiple of 256. */
#define SPFE_CULL_OFF_STATUS 0
#define SPFE_CULL_OFF_N_LISTED 4
#define SPFE_CULL_OFF_N_PASSES 8
#define SPFE_CULL_OFF_N_CULLED 12
#define SPFE_CULL_OFF_N_DEFERRED 16
#define SPFE_CULL_OFF_N_TOUCHED 20
#define SPFE_CULL_OFF_N_REPARENTED 24
#define SPFE_CULL_OFF_N_EVENTS 28
#define SPFE_CULL_OFF_N_BAD 32
#define SPFE_CULL_OFF_N_BAD_STORED 36
#define SPFE_CULL_OFF_ENTRY_SLOT 64
#define SPFE_CULL_OFF_ENTRY_CODE(c) (64 + 4 * (size_t)(c))
#define SPFE_CULL_OFF_ENTRY_PASS(c) (64 + 8 * (size_t)(c))
#define SPFE_CULL_OFF_ENTRY_MPS(c) (64 + 12 * (size_t)(c))
#define SPFE_CULL_OFF_ENTRY_RED(c) (64 + 16 * (size_t)(c))
#define SPFE_CULL_OFF_CULLED_SLOT(c) (64 + 20 * (size_t)(c))
#define SPFE_CULL_OFF_TOUCHED_SLOT(c) (64 + 24 * (size_t)(c))
#define SPFE_CULL_OFF_EVENT_CHILD(s, c) (64 + 24 * (size_t)(c) + 4 * (size_t)(s))
#define SPFE_CULL_OFF_EVENT_PARENT(s, c) (64 + 24 * (size_t)(c) + 8 * (size_t)(s))
#define SPFE_CULL_OFF_BAD_POINT(s, c) (64 + 24 * (size_t)(c) + 12 * (size_t)(s))
#define SPFE_CULL_OUT_BYTES(s, c, b) ((64 + 24 * (size_t)(c) + 12 * (size_t)(s) + 4 * (size_t)(b) + 255) / 256 * 256)
/* d_mp_nobs int32 [n_table], the resident array that stands for MapPoint::Observations(): nobs[p] = the entries that name p over
 * all rows of the slots whose bit 0 of d_kf_flags is clear; values outside [0, n_table) name nothing.  The WHOLE array is written,
 * zeros included.  TWO launches (a preset and a count by integer atomic additions, whose sum does not depend on their order), no
 * memset node in a capture.  It is the array's start value and its consistency check; between culls the caller keeps it up with
 * single-entry writes, as for d_parent.  Extents: d_kf_mp_of_kp 4 kp_stride n_slots, d_kf_flags n_slots, d_mp_nobs 4 n_table.
 * n_slots, kp_stride and n_table outside the ranges of spfe_update_local_map_resident, a null argument (d_mp_nobs may be null when
 * n_table is 0) or an int32 array not 4-byte aligned: SPFE_EINVAL before any launch. */
SPFE_API int spfe_count_observations_resident(spfe_handle h, const void *d_kf_mp_of_kp, int kp_stride, const void *d_kf_flags,
                                              int n_slots, void *d_mp_nobs, int n_table, void *stream);
/* The cull loop over the covisible keyframes of cur_slot (spfe_cull_math.h (1)-(8)).  THIS CALL WRITES d_kf_mp_of_kp, d_kf_flags,
 * d_mp_flags AND d_mp_nobs — the arrays every other form only reads —, the graph state and the two tables.  FOUR launches on
 * `stream` (NULL = the handle's) whatever the sizes are: a multi-workgroup kernel with the scratch's presets and the first pass's
 * counts, a wavefront a list entry; ONE workgroup for the passes, the culls and the ordered lists; ONE workgroup for the graph in
 * cull order (link removal with a rank sort of the neighbour's keys in LDS, rows and tables, the re-parenting steps, the touched
 * list); and a multi-workgroup scan of all rows that erases the newly bad points and leaves at once when there is none.  No
 * workgroup waits for another inside a kernel.  d_best_cov_a / d_best_cov_b as in spfe_update_connections_resident, either may be
 * NULL.  Extents: as there, plus d_mp_nobs 4 n_table and d_out SPFE_CULL_OUT_BYTES(n_slots, conn_cap, bad_cap).  The ranges of
 * spfe_update_connections_resident, th_obs < 1, bad_cap outside [0, SPFE_MP_MAX_POINTS], origin_slot outside [-1, n_slots), an
 * int32 array not 4-byte or d_out not 16-byte aligned, or a null argument (d_mp_flags and d_mp_nobs may be null when n_table is 0):
 * SPFE_EINVAL before any launch, d_out and the state untouched. */
SPFE_API int spfe_cull_keyframes_resident(spfe_handle h, const spfe_covis_graph *graph, void *d_kf_mp_of_kp, int kp_stride,
                                          void *d_kf_flags, void *d_mp_flags, void *d_mp_nobs, int n_table, int cur_slot,
                                          const spfe_cull_params *prm, void *d_best_cov_a, int n_best_a, void *d_best_cov_b,
                                          int n_best_b, void *d_out, void *stream);
/* The same on host arrays, synchronous: the pointers of `graph`, the rows, the flags, the counts and the two tables are HOST
 * arrays, updated in place; the same bytes everywhere. */
SPFE_API int spfe_cull_keyframes(spfe_handle h, const spfe_covis_graph *graph, int32_t *kf_mp_of_kp, int kp_stride,
                                 uint8_t *kf_flags, uint8_t *mp_flags, int32_t *mp_nobs, int n_table, int cur_slot,
                                 const spfe_cull_params *prm, int32_t *best_cov_a, int n_best_a, int32_t *best_cov_b, int n_best_b,
                                 void *out);

/* ---- map-point culling: the counters, the recent list, the admission of created points and the cull loop on resident state --------
 * LocalMapping::MapPointCulling (local_mapper.cpp:281-310), the second stage of every mapping cycle, with the state it reads made
 * resident: mnFound / mnVisible (kept up per frame behind TrackLocalMap), mlpRecentAddedMapPoints and mnFirstKFid, and the link
 * between the points spfe_create_map_points_record_device leaves in its blocks and the arrays every resident form reads.
 * include/spfe_mpcull_math.h is the contract, in lettered steps; state, rows, table, list and blocks are those of
 * tests/mpcull_ref/mpcull_ref.c byte for byte.  The names end in _resident as above, and the device forms' contract holds: launches
 * on the caller's stream, a fixed number of them, no host synchronisation, no host decision, the handle's scratch grown by a call
 * larger than any before it (make the largest call first, outside a capture), presets done by a kernel.
 * The state, caller-allocated, indexed by map-point table row:
 *   d_mp_flags   uint8 [n_table]     SPFE_PROJ_SEARCHABLE (= !isBad()) | SPFE_PROJ_OBSERVED: the table's flags
 *   d_mp_nobs    int32 [n_table]     Observations(): the array of spfe_count_observations_resident
 *   d_mp_found   int32 [n_table]     mnFound             d_mp_visible int32 [n_table]   mnVisible
 *   d_mp_first_kf int32 [n_table]    mnFirstKFid as a keyframe ID (not a slot), -1 for a point made from a frame
 *   d_recent     int32 [recent_cap]  the recent list in push order, -1 behind the count;  d_recent_n int32 [1]
 * n_table and recent_cap in [1, SPFE_MP_MAX_POINTS].  Counter values beyond INT32_MAX are not served. */
typedef struct spfe_mp_life {
  void *d_mp_flags, *d_mp_nobs, *d_mp_found, *d_mp_visible, *d_mp_first_kf;
  void *d_recent, *d_recent_n;
  int n_table, recent_cap;
} spfe_mp_life;
#define SPFE_ADMIT_RECENT_OVERFLOW 1 /* status: n_needed > recent_cap; nothing written but the block */
#define SPFE_ADMIT_BAD_RANGE 2       /* status: a count, id, keypoint or neighbour slot out of range; nothing written but the block */
#define SPFE_ADMIT_DISPLACED 4       /* status: n_displaced row entries held something before the call */
/* The block of an admission, SPFE_ADMIT_OUT_BYTES (16-byte aligned), EVERY byte written by every call:
 *   int32 status, n_admitted, n_recent_before, n_recent_after, n_displaced, n_needed, 0, 0
 *   int32 admitted[SPFE_TRI_MAX_NEIGHBOURS]   per neighbour, 0 for a refused block, behind n_neigh and in a refused call
 * and zeros up to 256. */
#define SPFE_ADMIT_OFF_STATUS 0
#define SPFE_ADMIT_OFF_N_ADMITTED 4
#define SPFE_ADMIT_OFF_N_RECENT_BEFORE 8
#define SPFE_ADMIT_OFF_N_RECENT_AFTER 12
#define SPFE_ADMIT_OFF_N_DISPLACED 16
#define SPFE_ADMIT_OFF_N_NEEDED 20
#define SPFE_ADMIT_OFF_ADMITTED 32
#define SPFE_ADMIT_OUT_BYTES 256
/* The block of the statistics, SPFE_MPSTAT_OUT_BYTES (16-byte aligned), every byte written:
 *   int32 n_visible_held, n_visible_view, n_found, and zeros up to 256. */
#define SPFE_MPSTAT_OFF_N_VISIBLE_HELD 0
#define SPFE_MPSTAT_OFF_N_VISIBLE_VIEW 4
#define SPFE_MPSTAT_OFF_N_FOUND 8
#define SPFE_MPSTAT_OUT_BYTES 256
#define SPFE_MPCULL_BAD_CUT 1    /* status: more than bad_cap points were culled; n_bad counts them all */
#define SPFE_MPCULL_WILD_ENTRY 2 /* status: the list named a point outside [0, n_table) */
typedef struct spfe_mpcull_params {
  int cur_kf_id;     /* mnId of the current keyframe */
  int th_obs;        /* 2 monocular; >= 0 */
  float found_ratio; /* 0.25f */
  int bad_cap;       /* entries of bad_point[] in the block, in [0, SPFE_MP_MAX_POINTS] */
} spfe_mpcull_params;
/* The block of a cull, SPFE_MPCULL_OUT_BYTES(recent_cap, bad_cap) bytes (a multiple of 256, 16-byte aligned), EVERY byte written
 * by every call:
 *   int32 status, n_listed, n_kept, n_culled_ratio, n_culled_obs, n_retired, n_erased_bad, n_wild, n_bad, n_bad_stored, 0 x 6
 *   int32 entry_point[recent_cap]   the list as it was read, -1 behind n_listed
 *   int32 entry_code [recent_cap]   SPFE_MPCULL_CODE_* of spfe_mpcull_math.h, -1 behind n_listed
 *   int32 bad_point  [bad_cap]      the culled points in list order (Map::EraseMapPoint is the host's), -1 behind n_bad_stored
 * and zeros up to the multiple of 256. */
#define SPFE_MPCULL_OFF_STATUS 0
#define SPFE_MPCULL_OFF_N_LISTED 4
#define SPFE_MPCULL_OFF_N_KEPT 8
#define SPFE_MPCULL_OFF_N_CULLED_RATIO 12
#define SPFE_MPCULL_OFF_N_CULLED_OBS 16
#define SPFE_MPCULL_OFF_N_RETIRED 20
#define SPFE_MPCULL_OFF_N_ERASED_BAD 24
#define SPFE_MPCULL_OFF_N_WILD 28
#define SPFE_MPCULL_OFF_N_BAD 32
#define SPFE_MPCULL_OFF_N_BAD_STORED 36
#define SPFE_MPCULL_OFF_ENTRY_POINT 64
#define SPFE_MPCULL_OFF_ENTRY_CODE(r) (64 + 4 * (size_t)(r))
#define SPFE_MPCULL_OFF_BAD_POINT(r) (64 + 8 * (size_t)(r))
#define SPFE_MPCULL_OUT_BYTES(r, b) ((64 + 8 * (size_t)(r) + 4 * (size_t)(b) + 255) / 256 * 256)
/* The preset of the table rows [first_row, first_row + n_rows) — flags 0, nobs 0, found 0, visible 0, first_kf -1 — and, with
 * reset_list != 0, of the list: every entry of d_recent -1, d_recent_n 0.  ONE launch (no memset node in a capture).  Extents: the
 * state as above.  The range outside [0, n_table], n_rows < 0, n_rows == 0 without reset_list, n_table or recent_cap out of range,
 * a null or misaligned array: SPFE_EINVAL before the launch. */
SPFE_API int spfe_mp_life_reset_resident(spfe_handle h, const spfe_mp_life *life, int first_row, int n_rows, int reset_list,
                                         void *stream);
/* Admission of the points of one spfe_create_map_points_record_device call (spfe_mpcull_math.h (A)): d_tri_out is that call's
 * d_out, n_neigh blocks spfe_tri_out_bytes(h) apart with ids used as table rows; d_neigh_slot int32 [n_neigh] the neighbours'
 * slots.  THIS CALL WRITES d_kf_mp_of_kp, d_xyz (f32 [n_table][3]) and the state.  TWO launches on `stream` (NULL = the
 * handle's) whatever the sizes are: a multi-workgroup kernel in which every workgroup derives the prefix offsets of the blocks and
 * makes the all-or-nothing test itself and then writes its share with plain vector stores, and one workgroup for the count of the
 * list and the block.  Extents: d_tri_out n_neigh spfe_tri_out_bytes(h), of which a refused block's status alone and otherwise
 * the int32 fields and the first n_new entries of new_xyz / new_k1 / new_k2 are read; d_neigh_slot 4 n_neigh; d_kf_mp_of_kp
 * 4 kp_stride n_slots; d_xyz 12 n_table; the state as above; d_out SPFE_ADMIT_OUT_BYTES.  n_slots and kp_stride outside the ranges
 * of spfe_update_local_map_resident, n_table or recent_cap outside [1, SPFE_MP_MAX_POINTS], n_neigh outside
 * [1, SPFE_TRI_MAX_NEIGHBOURS], cur_slot outside [0, n_slots), an int32 or f32 array not 4-byte or a block not 16-byte aligned, or a
 * null argument: SPFE_EINVAL before any launch, state and block untouched. */
SPFE_API int spfe_admit_map_points_resident(spfe_handle h, const spfe_mp_life *life, const void *d_tri_out, int n_neigh,
                                            const void *d_neigh_slot, int cur_slot, int cur_kf_id, void *d_kf_mp_of_kp, int kp_stride,
                                            int n_slots, void *d_xyz, void *d_out, void *stream);
/* IncreaseVisible / IncreaseFound of one tracked frame (spfe_mpcull_math.h (B)), behind spfe_track_local_map_record_device
 * (n = point_cap) and spfe_local_map_rows_resident, which the caller gives a SECOND array so that both sets of holders exist:
 * d_mp_of_kp_entry the frame's holders as table rows before the local-map step, d_mp_of_kp_after the rows behind it.  d_point_idx
 * is the local map's list, d_proj_out the search's block (the bytes SPFE_PROJ_OFF_VIEW .. + point_cap are read), d_pose_out the
 * pose block (the bytes SPFE_POSE_OFF_OUTLIER .. + n_kp are read).  The verdict is not consulted: the reference increments before
 * it decides.  WRITES d_mp_found and d_mp_visible by integer atomic additions, whose sum does not depend on their order; the list,
 * the other state arrays and d_mp_nobs are not touched (d_recent, d_recent_n, d_mp_nobs and d_mp_first_kf may be null here).  ONE
 * launch.  Extents: d_mp_of_kp_entry / d_mp_of_kp_after 4 n_kp, d_point_idx 4 point_cap, d_proj_out SPFE_PROJ_OFF_VIEW +
 * point_cap, d_pose_out SPFE_POSE_OFF_OUTLIER + n_kp, d_out SPFE_MPSTAT_OUT_BYTES.  n_kp outside [0, SPFE_PROJ_MAX_POINTS],
 * point_cap outside [1, SPFE_PROJ_MAX_POINTS], n_table out of range, a misaligned or null argument (the two holder arrays may be
 * null when n_kp is 0): SPFE_EINVAL before the launch. */
SPFE_API int spfe_track_statistics_resident(spfe_handle h, const spfe_mp_life *life, const void *d_mp_of_kp_entry,
                                            const void *d_mp_of_kp_after, int n_kp, const void *d_point_idx, int point_cap,
                                            const void *d_proj_out, const void *d_pose_out, void *d_out, void *stream);
/* The cull loop over the recent list (spfe_mpcull_math.h (C)).  THIS CALL WRITES d_mp_flags, d_recent, d_recent_n and
 * d_kf_mp_of_kp; d_kf_flags and the other state arrays are read only.  FOUR launches on `stream` (NULL = the handle's) whatever the
 * sizes are: the preset of the scratch (first entry and mark per point); a multi-workgroup decision kernel (a code per entry, the
 * first entry of every culled point by an integer atomic minimum); ONE workgroup for the duplicates, the stable compaction of the
 * list across chunks, the flag clears, bad_point[] and the block; and a multi-workgroup scan of all rows that erases the culled
 * points with 16-byte loads from each row's first aligned boundary and leaves at once when there is none.  No workgroup waits for
 * another inside a kernel.  Extents: d_kf_mp_of_kp 4 kp_stride n_slots, d_kf_flags n_slots, the state as above, d_out
 * SPFE_MPCULL_OUT_BYTES(recent_cap, bad_cap).  The ranges of spfe_admit_map_points_resident, th_obs < 0, bad_cap outside
 * [0, SPFE_MP_MAX_POINTS], an int32 array not 4-byte or d_out not 16-byte aligned, or a null argument: SPFE_EINVAL before any launch,
 * state and block untouched. */
SPFE_API int spfe_cull_map_points_resident(spfe_handle h, const spfe_mp_life *life, void *d_kf_mp_of_kp, int kp_stride,
                                           const void *d_kf_flags, int n_slots, const spfe_mpcull_params *prm, void *d_out,
                                           void *stream);
/* The three on host arrays, synchronous: the pointers of `life`, the rows, the table and the blocks are HOST arrays, the state
 * updated in place; the same bytes everywhere.  tri_out: the n_neigh blocks as downloaded. */
SPFE_API int spfe_admit_map_points(spfe_handle h, const spfe_mp_life *life, const void *tri_out, int n_neigh, const int32_t *neigh_slot,
                                   int cur_slot, int cur_kf_id, int32_t *kf_mp_of_kp, int kp_stride, int n_slots, float *xyz, void *out);
SPFE_API int spfe_track_statistics(spfe_handle h, const spfe_mp_life *life, const int32_t *mp_of_kp_entry,
                                   const int32_t *mp_of_kp_after, int n_kp, const int32_t *point_idx, int point_cap,
                                   const uint8_t *in_view, const uint8_t *outlier, void *out);
SPFE_API int spfe_cull_map_points(spfe_handle h, const spfe_mp_life *life, int32_t *kf_mp_of_kp, int kp_stride,
                                  const uint8_t *kf_flags, int n_slots, const spfe_mpcull_params *prm, void *out);

/* ---- local bundle adjustment on resident state: the gather in front of the solver and the application behind it --------------------
 * Optimizer::LocalBundleAdjustment's gathering (optimizer.cpp:447-499, :568-658) and its map edits (:660-662, :739-773) on the
 * arrays the other resident forms keep, around spfe_local_ba_records_device, which is unchanged.  include/spfe_lba_math.h is the
 * contract, in lettered steps; blocks and every edited array are those of tests/lba_ref/lba_ref.c byte for byte.  The names end in
 * _resident as above, and the device forms' contract holds: launches on the caller's stream, a fixed number of them, no host
 * synchronisation, no host decision, the handle's scratch grown by a call larger than any before it (make the largest call first,
 * outside a capture), presets done by a kernel.  The chain on one stream:
 *   spfe_gather_local_ba_resident -> the host reads the block's header and kf_slot[] (64 + 4 kf_cap bytes: the ONE host read of the
 *   chain; it gives n_kf, n_points, n_edges and picks the record pointers) -> spfe_local_ba_records_device with d_edges, d_Tcw,
 *   d_fixed and d_xyz pointing INTO the gather block -> spfe_apply_local_ba_resident -> spfe_refresh_map_points_device
 *   (SPFE_MP_NORMAL_DEPTH) with d_point_idx from the gather block and d_obs_start / d_obs / d_ref_slot from the apply block.
 * One more caller-kept array: d_mp_ref_slot int32 [n_table], mpRefKF as a slot, kept up by the caller like d_parent: the host
 * writes the creating keyframe's slot for every admitted point (the admission itself does not), the application moves it. */
#define SPFE_LBA_LOCAL_CUT 1     /* gather status: the local list was cut at kf_cap or free_cap */
#define SPFE_LBA_POINT_CUT 2     /* gather status: n_points_all > point_cap */
#define SPFE_LBA_FIXED_CUT 4     /* gather status: more fixed keyframes than kf_cap - n_local */
#define SPFE_LBA_EDGE_OVERFLOW 8 /* gather status: n_obs_needed > edge_cap; obs_start, obs and edges are -1 */
#define SPFE_LBA_NOT_APPLIED 1   /* apply status: refused (spfe_lba_math.h (A0)); nothing but the block written */
#define SPFE_LBA_BAD_CUT 2       /* apply status: more than bad_cap points went bad; n_bad counts them all */
#define SPFE_LBA_WILD 4          /* apply status: an erase index, edge or observation of the blocks named nothing and was skipped */
typedef struct spfe_lba_gather_params {
  int cur_slot;    /* the keyframe being processed, in [0, n_slots) */
  int origin_slot; /* the keyframe with mnId == 0 (fixed), or -1 */
  int kf_cap;      /* local + fixed keyframes, in [1, SPFE_BA_MAX_KEYFRAMES] */
  int free_cap;    /* free keyframes, in [1, SPFE_BA_MAX_FREE] */
  int point_cap;   /* in [1, SPFE_BA_MAX_POINTS] */
  int edge_cap;    /* observations (and so edges), in [1, SPFE_BA_MAX_EDGES] */
} spfe_lba_gather_params;
typedef struct spfe_lba_apply_params {
  int kf_cap, point_cap, edge_cap; /* those of the gather whose block is applied */
  int bad_cap;                     /* entries of bad_point[] in the block, in [0, SPFE_BA_MAX_POINTS] */
} spfe_lba_apply_params;
/* The gather's block, SPFE_LBA_GATHER_BYTES(kf_cap, point_cap, edge_cap) bytes (a multiple of 256, 16-byte aligned, every array
 * inside it 16-byte aligned), EVERY byte written by every call:
 *   int32 status, n_local, n_free, n_fixed, n_kf, n_points, n_points_all, n_obs, n_edges, n_obs_needed, 0 x 6
 *   int32 kf_slot [kf_cap]        local ++ fixed as global slots, -1 behind n_kf
 *   uint8 fixed   [kf_cap]        the solver's d_fixed, 0 behind n_kf
 *   f32   Tcw     [kf_cap][16]    the solver's d_Tcw, 0 behind n_kf
 *   int32 point_idx[point_cap]    table rows, -1 behind n_points
 *   f32   xyz     [point_cap][3]  the solver's d_xyz, 0 behind n_points
 *   int32 obs_start[point_cap+1]  -1 behind n_points + 1 entries
 *   int32 obs     [edge_cap][2]   (global slot, keypoint), -1 behind n_obs
 *   int32 edges   [edge_cap][3]   the solver's d_edges: (point, BA slot, keypoint), -1 behind n_edges
 * and zeros up to the multiple of 256. */
#define SPFE_LBA_PAD16(v) (((size_t)(v) + 15) / 16 * 16)
#define SPFE_LBA_OFF_STATUS 0
#define SPFE_LBA_OFF_N_LOCAL 4
#define SPFE_LBA_OFF_N_FREE 8
#define SPFE_LBA_OFF_N_FIXED 12
#define SPFE_LBA_OFF_N_KF 16
#define SPFE_LBA_OFF_N_POINTS 20
#define SPFE_LBA_OFF_N_POINTS_ALL 24
#define SPFE_LBA_OFF_N_OBS 28
#define SPFE_LBA_OFF_N_EDGES 32
#define SPFE_LBA_OFF_N_OBS_NEEDED 36
#define SPFE_LBA_OFF_KF_SLOT 64
#define SPFE_LBA_OFF_FIXED(k) (64 + SPFE_LBA_PAD16(4 * (size_t)(k)))
#define SPFE_LBA_OFF_TCW(k) (SPFE_LBA_OFF_FIXED(k) + SPFE_LBA_PAD16(k))
#define SPFE_LBA_OFF_POINT_IDX(k) (SPFE_LBA_OFF_TCW(k) + 64 * (size_t)(k))
#define SPFE_LBA_OFF_XYZ(k, p) (SPFE_LBA_OFF_POINT_IDX(k) + SPFE_LBA_PAD16(4 * (size_t)(p)))
#define SPFE_LBA_OFF_OBS_START(k, p) (SPFE_LBA_OFF_XYZ(k, p) + SPFE_LBA_PAD16(12 * (size_t)(p)))
#define SPFE_LBA_OFF_OBS(k, p) (SPFE_LBA_OFF_OBS_START(k, p) + SPFE_LBA_PAD16(4 * ((size_t)(p) + 1)))
#define SPFE_LBA_OFF_EDGES(k, p, e) (SPFE_LBA_OFF_OBS(k, p) + SPFE_LBA_PAD16(8 * (size_t)(e)))
#define SPFE_LBA_GATHER_BYTES(k, p, e) ((SPFE_LBA_OFF_EDGES(k, p, e) + 12 * (size_t)(e) + 255) / 256 * 256)
/* The application's block, SPFE_LBA_APPLY_BYTES(point_cap, edge_cap, bad_cap) bytes (a multiple of 256, 16-byte aligned, every
 * array 16-byte aligned), EVERY byte written by every call:
 *   int32 status, n_erased, n_bad, n_bad_stored, n_ref_moved, n_obs_after, 0 x 10
 *   int32 bad_point [bad_cap]       the newly bad points as table rows in point order (Map::EraseMapPoint is the host's), -1 behind
 *   int32 obs_start [point_cap+1]   the refresh's d_obs_start: n_points + 1 entries, -1 behind (refused: zeros, then -1)
 *   int32 obs       [edge_cap][2]   the refresh's d_obs, -1 behind n_obs_after
 *   int32 ref_slot  [point_cap]     the refresh's d_ref_slot, -1 behind n_points
 * and zeros up to the multiple of 256. */
#define SPFE_LBA_APPLY_OFF_STATUS 0
#define SPFE_LBA_APPLY_OFF_N_ERASED 4
#define SPFE_LBA_APPLY_OFF_N_BAD 8
#define SPFE_LBA_APPLY_OFF_N_BAD_STORED 12
#define SPFE_LBA_APPLY_OFF_N_REF_MOVED 16
#define SPFE_LBA_APPLY_OFF_N_OBS_AFTER 20
#define SPFE_LBA_APPLY_OFF_BAD_POINT 64
#define SPFE_LBA_APPLY_OFF_OBS_START(b) (64 + SPFE_LBA_PAD16(4 * (size_t)(b)))
#define SPFE_LBA_APPLY_OFF_OBS(p, b) (SPFE_LBA_APPLY_OFF_OBS_START(b) + SPFE_LBA_PAD16(4 * ((size_t)(p) + 1)))
#define SPFE_LBA_APPLY_OFF_REF_SLOT(p, e, b) (SPFE_LBA_APPLY_OFF_OBS(p, b) + SPFE_LBA_PAD16(8 * (size_t)(e)))
#define SPFE_LBA_APPLY_BYTES(p, e, b) ((SPFE_LBA_APPLY_OFF_REF_SLOT(p, e, b) + 4 * (size_t)(p) + 255) / 256 * 256)
/* The gather (spfe_lba_math.h (G1)-(G6)).  Every input is READ ONLY.  d_ord_slot / conn_cap are those of the spfe_covis_graph:
 * row cur_slot alone is read, up to its first -1 or conn_cap.  TEN launches on `stream` (NULL = the handle's) whatever the sizes
 * are: the presets of the scratch; ONE workgroup for the local list (first entry of a slot by an integer atomic minimum, an ordered
 * rank, the prefix cut); the first occurrence of every point of the local rows by an integer atomic minimum on its key; ONE
 * workgroup for the stable compaction of the points; the scan of ALL rows — a wavefront a row, 16-byte loads from the row's first
 * aligned boundary, any row pitch — against a dense rank map, which counts per point, collects the hits and keeps the least
 * listed point of every non-local row; the fixed list by a rank count over those keys; the edge counts; ONE workgroup for the two
 * prefix sums, the header, the poses and the tails; the hits scattered into their points' ranges; and a wavefront a point that
 * orders its range by (slot, keypoint) and writes obs[] and edges[].  No workgroup waits for another inside a kernel, and no
 * output depends on the order of the atomics.  Extents: d_ord_slot 4 conn_cap n_slots bytes, d_kf_mp_of_kp 4 kp_stride n_slots,
 * d_kf_flags n_slots, d_mp_flags n_table, d_xyz 12 n_table, d_Tcw 64 n_slots, d_out SPFE_LBA_GATHER_BYTES(kf_cap, point_cap,
 * edge_cap).  n_slots and kp_stride outside the ranges of spfe_update_local_map_resident, n_table outside [1, SPFE_MP_MAX_POINTS],
 * conn_cap outside [1, SPFE_COVIS_MAX_CONN], cur_slot outside [0, n_slots), origin_slot outside [-1, n_slots), a capacity outside
 * the range its field names, an int32 or f32 array not 4-byte or d_out not 16-byte aligned, or a null argument: SPFE_EINVAL
 * before any launch, d_out untouched. */
SPFE_API int spfe_gather_local_ba_resident(spfe_handle h, const void *d_ord_slot, int conn_cap, const void *d_kf_mp_of_kp,
                                           int kp_stride, const void *d_kf_flags, int n_slots, const void *d_mp_flags,
                                           const void *d_xyz, int n_table, const void *d_Tcw, const spfe_lba_gather_params *prm,
                                           void *d_out, void *stream);
/* The application (spfe_lba_math.h (A0)-(A6)) of the solver's block d_ba_out to the problem of the gather block d_gather, both
 * where they lie on the device; their counts are read there, and every index in them is tested before it is followed.  THIS CALL
 * WRITES d_kf_mp_of_kp, d_mp_flags, d_mp_nobs, d_mp_ref_slot, d_xyz and d_Tcw; d_kf_flags is read only.  FIVE launches on `stream`
 * whatever the sizes are: the preset of the marks; a thread an erase entry (the observation it names marked, its row entry -1); a
 * thread a point, the ONE owner of that point's nobs, flags, ref_slot and position; ONE workgroup for the prefix sum, bad_point[]
 * and the header; and the lists, the poses and the tails.  Extents: d_gather SPFE_LBA_GATHER_BYTES(kf_cap, point_cap, edge_cap),
 * d_ba_out SPFE_BA_OUT_BYTES(n_kf, n_points, n_edges) of the gather's header (the first 128 bytes alone are read when the call is
 * refused), d_kf_mp_of_kp 4 kp_stride n_slots, d_kf_flags n_slots, d_mp_flags n_table, d_mp_nobs / d_mp_ref_slot 4 n_table, d_xyz
 * 12 n_table, d_Tcw 64 n_slots, d_out SPFE_LBA_APPLY_BYTES(point_cap, edge_cap, bad_cap).  The ranges of the gather, bad_cap
 * outside [0, SPFE_BA_MAX_POINTS], a misaligned or null argument: SPFE_EINVAL before any launch, everything untouched. */
SPFE_API int spfe_apply_local_ba_resident(spfe_handle h, const void *d_gather, const void *d_ba_out, void *d_kf_mp_of_kp,
                                          int kp_stride, const void *d_kf_flags, int n_slots, void *d_mp_flags, void *d_mp_nobs,
                                          void *d_mp_ref_slot, void *d_xyz, int n_table, void *d_Tcw,
                                          const spfe_lba_apply_params *prm, void *d_out, void *stream);
/* The two on host arrays, synchronous, the same bytes everywhere.  ord_row: row cur_slot of the graph's ord_slot, conn_cap
 * entries.  gather / ba_out: the blocks as downloaded; the arrays the application writes are updated in place. */
SPFE_API int spfe_gather_local_ba(spfe_handle h, const int32_t *ord_row, int conn_cap, const int32_t *kf_mp_of_kp, int kp_stride,
                                  const uint8_t *kf_flags, int n_slots, const uint8_t *mp_flags, const float *xyz, int n_table,
                                  const float *Tcw, const spfe_lba_gather_params *prm, void *out);
SPFE_API int spfe_apply_local_ba(spfe_handle h, const void *gather, const void *ba_out, int32_t *kf_mp_of_kp, int kp_stride,
                                 const uint8_t *kf_flags, int n_slots, uint8_t *mp_flags, int32_t *mp_nobs, int32_t *mp_ref_slot,
                                 float *xyz, int n_table, float *Tcw, const spfe_lba_apply_params *prm, void *out);

/* ---- a new keyframe on resident state: the insertion of its row, and the observation lists of the refreshes ------------------------
 * LocalMapping::ProcessNewKeyFrame (local_mapper.cpp:255-272) without its refresh, and the CSR every
 * spfe_refresh_map_points_device call takes (d_obs_start, d_obs, d_ref_slot) from ONE scan of the resident rows, for any list of
 * points: with the two a host that keeps the resident arrays needs no mObservations for a refresh of the mapping cycle.
 * include/spfe_newkf_math.h is the contract, in lettered steps; blocks and every edited array are those of
 * tests/newkf_ref/newkf_ref.c byte for byte.  The names end in _resident as above, and the device forms' contract holds: launches
 * on the caller's stream, a fixed number of them, no host synchronisation, no host decision, the handle's scratch grown by a call
 * larger than any before it (make the largest call first, outside a capture), presets done by a kernel, no workgroup waits for
 * another inside a kernel, and no output byte depends on the order of an atomic (integer minima and sums; where an atomic hands out
 * places a later kernel orders what was placed). */
#define SPFE_NEWKF_ROW_IN_USE 1      /* status: the row of cur_slot holds an entry >= 0; nothing written but the block */
#define SPFE_NEWKF_BAD_SLOT 2        /* status: d_kf_flags[cur_slot] has bit 0 set; nothing written but the block */
#define SPFE_NEWKF_RECENT_OVERFLOW 4 /* status: n_needed > recent_cap; nothing written but the block */
/* The block of an insertion, SPFE_NEWKF_OUT_BYTES(n_kp, kp_stride) bytes (a multiple of 256, 16-byte aligned), EVERY byte written
 * by every call:
 *   int32 status, n_none, n_wild, n_bad_point, n_added, n_repeated, n_recent_before, n_recent_after, n_needed, 0 x 7
 *   int32 code[n_kp]             SPFE_NEWKF_CODE_* of spfe_newkf_math.h (the count of code c is the int32 at 4 + 4 c)
 *   int32 added_point[kp_stride] at the next 16-byte boundary: the point at an ADDED keypoint, -1 everywhere else and in a refused
 *                                call — a point list for spfe_list_observations_resident as it lies (m = kp_stride)
 * and zeros in between and up to the multiple of 256. */
#define SPFE_NEWKF_OFF_STATUS 0
#define SPFE_NEWKF_OFF_N_NONE 4
#define SPFE_NEWKF_OFF_N_WILD 8
#define SPFE_NEWKF_OFF_N_BAD_POINT 12
#define SPFE_NEWKF_OFF_N_ADDED 16
#define SPFE_NEWKF_OFF_N_REPEATED 20
#define SPFE_NEWKF_OFF_N_RECENT_BEFORE 24
#define SPFE_NEWKF_OFF_N_RECENT_AFTER 28
#define SPFE_NEWKF_OFF_N_NEEDED 32
#define SPFE_NEWKF_OFF_CODE 64
#define SPFE_NEWKF_OFF_ADDED_POINT(k) (64 + (4 * (size_t)(k) + 15) / 16 * 16)
#define SPFE_NEWKF_OUT_BYTES(k, s) ((SPFE_NEWKF_OFF_ADDED_POINT(k) + 4 * (size_t)(s) + 255) / 256 * 256)
/* The insertion (spfe_newkf_math.h (I)).  d_frame_mp_of_kp int32 [n_kp]: the frame's mvpMapPoints as table rows at
 * CreateNewKeyFrame, outliers included (what spfe_local_map_rows_resident leaves).  The host has set the slot's flag, record
 * pointer and pose; the row of cur_slot is empty (every entry < 0), as spfe_covis_reset_slots_resident's caller presets it.  THIS
 * CALL WRITES row cur_slot of d_kf_mp_of_kp, d_mp_nobs, d_mp_flags, d_recent, d_recent_n and, where BOTH are given, d_desc_track
 * (f32 [n_table][256], the descriptor the dust tracker matches a point with) from d_kf_record, the keyframe's record: row i of its
 * descriptors at an ADDED keypoint i, a bf16 row widened exactly.  d_mp_found, d_mp_visible and d_mp_first_kf of `life` are not
 * touched and may be null.  All or nothing, tested on the device; the block carries n_needed so that the host can grow the list.
 * FOUR launches on `stream` (NULL = the handle's) whatever the sizes are: the preset of the scratch (first keypoint per point); the
 * first keypoint of every good point by an integer atomic minimum; ONE workgroup for the test, the codes, the row, the counts, the
 * list and the block (nobs by integer atomic additions, whose sum does not depend on their order); and the descriptor rows, a
 * wavefront a keypoint, which leaves at once without the two arrays.  Extents: d_frame_mp_of_kp 4 n_kp, d_kf_mp_of_kp 4 kp_stride
 * n_slots (row cur_slot alone is read and written), d_kf_flags n_slots (byte cur_slot alone is read), the state as in
 * spfe_mp_life, d_kf_record spfe_record_bytes (the descriptor rows [0, n_kp) alone are read), d_desc_track 1024 n_table, d_out
 * SPFE_NEWKF_OUT_BYTES(n_kp, kp_stride).  n_slots and kp_stride outside the ranges of spfe_update_local_map_resident, n_table or
 * recent_cap outside [1, SPFE_MP_MAX_POINTS], n_kp outside [0, kp_stride] (or, with both descriptor arrays, beyond the handle's
 * kmax), cur_slot outside [0, n_slots), an int32 or f32 array not 4-byte or d_out not 16-byte aligned, or a null argument
 * (d_frame_mp_of_kp may be null when n_kp is 0; d_kf_record and d_desc_track may always be): SPFE_EINVAL before any launch, state,
 * rows and block untouched. */
SPFE_API int spfe_insert_keyframe_resident(spfe_handle h, const spfe_mp_life *life, const void *d_frame_mp_of_kp, int n_kp,
                                           int cur_slot, void *d_kf_mp_of_kp, int kp_stride, const void *d_kf_flags, int n_slots,
                                           const void *d_kf_record, void *d_desc_track, void *d_out, void *stream);
#define SPFE_LISTOBS_OVERFLOW 1 /* status: n_obs_needed > obs_cap; n_obs 0, every obs_start 0, obs all -1 */
#define SPFE_LISTOBS_MANY 2     /* status: max_obs > SPFE_MP_MAX_OBS: the refresh answers TOO_MANY for such a point */
/* The block of a listing, SPFE_LISTOBS_OUT_BYTES(m, obs_cap) bytes (a multiple of 256, 16-byte aligned), EVERY byte written by
 * every call; each array starts at a 16-byte boundary:
 *   int32 status, m, n_first, n_empty, n_wild, n_repeated, n_obs, n_obs_needed, max_obs, obs_cap, 0 x 6
 *   int32 point_idx[m]       the point at a FIRST entry, -1 at every other one
 *   int32 obs_start[m + 1]   ascending within [0, n_obs]; an entry that is not FIRST has an empty range
 *   int32 ref_slot[m]        d_mp_ref_slot[point] at a FIRST entry, -1 at every other one
 *   int32 obs[obs_cap][2]    (keyframe slot, keypoint), -1 behind n_obs
 * and zeros in between and up to the multiple of 256.  spfe_refresh_map_points_device takes the four arrays as pointers INTO the
 * block with E = obs_cap: it reads obs_start[i] and obs_start[i + 1] of entry i alone and no observation outside such a range, so
 * the -1 tail of obs[] is never followed; an entry of -1 in point_idx answers SPFE_MP_INVALID there and writes nothing. */
#define SPFE_LISTOBS_OFF_STATUS 0
#define SPFE_LISTOBS_OFF_M 4
#define SPFE_LISTOBS_OFF_N_FIRST 8
#define SPFE_LISTOBS_OFF_N_EMPTY 12
#define SPFE_LISTOBS_OFF_N_WILD 16
#define SPFE_LISTOBS_OFF_N_REPEATED 20
#define SPFE_LISTOBS_OFF_N_OBS 24
#define SPFE_LISTOBS_OFF_N_OBS_NEEDED 28
#define SPFE_LISTOBS_OFF_MAX_OBS 32
#define SPFE_LISTOBS_OFF_OBS_CAP 36
#define SPFE_LISTOBS_OFF_POINT_IDX 64
#define SPFE_LISTOBS_OFF_OBS_START(m) (64 + (4 * (size_t)(m) + 15) / 16 * 16)
#define SPFE_LISTOBS_OFF_REF_SLOT(m) (SPFE_LISTOBS_OFF_OBS_START(m) + (4 * ((size_t)(m) + 1) + 15) / 16 * 16)
#define SPFE_LISTOBS_OFF_OBS(m) (SPFE_LISTOBS_OFF_REF_SLOT(m) + (4 * (size_t)(m) + 15) / 16 * 16)
#define SPFE_LISTOBS_OUT_BYTES(m, e) ((SPFE_LISTOBS_OFF_OBS(m) + 8 * (size_t)(e) + 255) / 256 * 256)
/* The listing (spfe_newkf_math.h (O)).  d_point_idx int32 [m], or NULL: entry i names table row first_row + i (first_row is not
 * read with a list).  An entry of -1 is empty, one outside [0, n_table) is empty and counted, a later entry that names a point
 * already listed is empty and counted (the first entry refreshes the point: two writers of one table row do not exist) — so a whole
 * row of d_kf_mp_of_kp (m = kp_stride) and the insertion's added_point are valid lists.  Point flags are not read: the refresh
 * answers SKIP_BAD itself.  Everything is READ ONLY but d_out.  SIX launches on `stream` (NULL = the handle's) whatever the sizes
 * are: the preset of the scratch (a dense first-entry map over n_table, the counts); the first entry of every point by an integer
 * atomic minimum; the scan of ALL rows of slots that are not bad, a wavefront a row with 16-byte loads from the row's first aligned
 * boundary, the hits appended to an unordered list (a wavefront claims its places with one atomic addition); ONE workgroup for the
 * prefix sum, the per-entry arrays and the header; the scatter into each point's range; and an order pass that is exact for any
 * count per point (a wavefront serves a point of at most 256 observations, the workgroup a larger one, each counting smaller (slot,
 * keypoint) keys).  Extents: d_point_idx 4 m, d_kf_mp_of_kp 4 kp_stride n_slots, d_kf_flags n_slots, d_mp_ref_slot 4 n_table,
 * d_out SPFE_LISTOBS_OUT_BYTES(m, obs_cap).  m outside [0, SPFE_MP_MAX_POINTS], obs_cap outside [0, SPFE_MP_MAX_EDGES], n_table
 * outside [1, SPFE_MP_MAX_POINTS], first_row < 0, n_slots and kp_stride outside the ranges of spfe_update_local_map_resident, an
 * int32 array not 4-byte or d_out not 16-byte aligned, or a null argument (d_point_idx may always be null): SPFE_EINVAL before any
 * launch, d_out untouched. */
SPFE_API int spfe_list_observations_resident(spfe_handle h, const void *d_point_idx, int first_row, int m,
                                             const void *d_kf_mp_of_kp, int kp_stride, const void *d_kf_flags, int n_slots,
                                             const void *d_mp_ref_slot, int n_table, int obs_cap, void *d_out, void *stream);
/* The two on host arrays, synchronous, the same bytes everywhere: the pointers of `life`, the rows and the blocks are HOST arrays,
 * state, rows and desc_track updated in place.  kf_record: the record as downloaded (spfe_record_bytes), or NULL. */
SPFE_API int spfe_insert_keyframe(spfe_handle h, const spfe_mp_life *life, const int32_t *frame_mp_of_kp, int n_kp, int cur_slot,
                                  int32_t *kf_mp_of_kp, int kp_stride, const uint8_t *kf_flags, int n_slots, const void *kf_record,
                                  float *desc_track, void *out);
SPFE_API int spfe_list_observations(spfe_handle h, const int32_t *point_idx, int first_row, int m, const int32_t *kf_mp_of_kp,
                                    int kp_stride, const uint8_t *kf_flags, int n_slots, const int32_t *mp_ref_slot, int n_table,
                                    int obs_cap, void *out);

/* ---- input staging -----------------------------------------------------
 * Replaces, per frame, the host OpenCV sequence in front of the extractor:
 *   cv::remap(mono, mono, m1, m2, cv::INTER_LINEAR)       orb_slam2/src/io/data_loader.cc:519-521
 *   mono(cv::Rect(0, 0, camera::width, camera::height))   orb_slam2/src/system.cpp:160-161
 *   cvtColor(im, im, CV_BGR2GRAY / CV_RGB2GRAY / CV_BGRA2GRAY / CV_RGBA2GRAY)
 *                                                         orb_slam2/src/tracking/mono_tracker.cpp:18-28
 * with one gather kernel that writes the gray H x W frame conv1a reads (OpenCV 3.x integer
 * arithmetic: 5-bit sub-pixel positions, 15-bit bilinear weights, BORDER_CONSTANT 0; gray =
 * (1868 B + 9617 G + 4899 R + 8192) >> 14).  The maps are the CV_32FC1 pair of
 * cv::initUndistortRectifyMap (data_loader.cc:485-486), src_height x src_width, copied to the
 * device once; map_x == map_y == NULL means "no remap" (crop + gray only).  src_height >= height
 * and src_width >= width of the handle (the crop keeps the top-left corner).
 * Map entries that are not finite, or whose 32-fold is outside [-2^31, 2^31), read the border (the pixel is 0), as cvRound
 * gives on x86 (cvtss2si answers INT_MIN: position -32768): NaN, +-inf, 1e10, 67108864.0.  Kernel and oracle test the range
 * before they convert. */
typedef struct spfe_staging {
  int src_height, src_width; /* camera image == map size */
  int channels;              /* 1, 3 or 4 interleaved 8-bit channels (cv::imread gives 3: BGR) */
  int rgb;                   /* 0: blue first (mbRGB == false), 1: red first */
  const float *map_x, *map_y;
} spfe_staging;
SPFE_API int spfe_set_staging(spfe_handle h, const spfe_staging *st);
/* spfe_extract / spfe_extract_batch on raw camera frames (stride in bytes >= src_width * channels) */
SPFE_API int spfe_extract_staged(spfe_handle h, const uint8_t *src, int stride, spfe_result *out);
SPFE_API int spfe_extract_batch_staged(spfe_handle h, const uint8_t *const *srcs, int stride, int n,
                                       spfe_result *outs);
/* Device form: n packed raw frames [n][src_height][src_width][channels] in HBM -> gray frames
 * [n][height][width] (d_gray, ready for spfe_extract_batch_device), enqueued on `stream`. */
SPFE_API int spfe_stage_batch_device(spfe_handle h, const void *d_src, int n, void *d_gray, void *stream);

/* Per-stage GPU time (ms, HIP events recorded on the launch stream around every
 * kernel), averaged over the calls since spfe_stage_reset (the library keeps the
 * last 128 calls).  Enabled by SPFE_STAGE_TIMING=1 in the environment at
 * spfe_create (SPFE_STAGE_TIMING=2: only the dominant kernel, conv1b, is bracketed — two events
 * per call instead of sixteen; the other stages then read 0); returns the number of stages written (names: spfe_stage_name). */
SPFE_API int spfe_stage_times(spfe_handle h, float *ms, int cap);
SPFE_API int spfe_stage_reset(spfe_handle h);
SPFE_API const char *spfe_stage_name(int i);

/* heat_inv (sp_extractor.cpp:468) of frame `frame` of the LAST synchronous host call (spfe_extract, spfe_extract_batch,
 * spfe_extract_staged) on this handle, copied to the library's pinned buffer on demand: *out is a view valid until the next
 * call on the handle.  Meant for handles created with SPFE_FLAG_LAZY_HEAT_INV (without it the map is in spfe_result already;
 * the call works all the same).  SPFE_EINVAL without SPFE_FLAG_HEAT, before the first call, or for a frame the call did not hold. */
SPFE_API int spfe_fetch_heat_inv(spfe_handle h, int frame, const float **out);

/* The H x W maps of the synchronous host calls (spfe_extract*, spfe_postprocess, the three-part call) straight into memory of
 * the caller: heat / heat_inv = max_batch * H * W floats each, page-locked by the library for as long as they are set
 * (hipHostRegister; the caller keeps them allocated until the next spfe_set_map_buffers or spfe_destroy), and what
 * spfe_result.heat / .heat_inv (and spfe_extract_maps, spfe_fetch_heat_inv) point at from then on.  NULL = the library's own
 * buffer for that map again.  For a caller whose outputs are deep copies anyway — the drop-in class keeps heat_ / heat_inv_ as
 * cv::Mat members the reference fills per call (sp_extractor.cpp:461-474): with the members' own storage set here the maps
 * land in them by DMA and the copies (2 x 1.44 MB at 752x480) disappear from the call.  The pipelined host path
 * (spfe_submit_batch) keeps its own buffers.  SPFE_EINVAL without SPFE_FLAG_HEAT or while a call is open. */
SPFE_API int spfe_set_map_buffers(spfe_handle h, float *heat, float *heat_inv);

/* Test hook: evaluates the device forms of spfe_expf(x) and spfe_logf(|x|)
 * (include/spfe_exact_math.h) on n host floats, so tests can compare GPU bits
 * with host bits. */
SPFE_API int spfe_math_probe(const float *in, float *out_exp, float *out_log, int n);

SPFE_API const char *spfe_last_error(void);
SPFE_API const char *spfe_version(void);
SPFE_API int spfe_abi_version(void); /* SPFE_ABI_VERSION of the header the library was built from */
SPFE_API int spfe_check_abi(int abi_version, size_t sizeof_config, size_t sizeof_result, size_t sizeof_record_layout);

#ifdef __cplusplus
}
#endif
#endif /* SPFE_H */
