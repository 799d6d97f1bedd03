// host_main.cpp — drives the C ABI of include/spfe.h over the stub HIP runtime (hip_stub.cpp), as a plain executable built
// with a sanitizer (Makefile).  argv[1] = scenario, argv[2] = an "SPFW" weight file.  Exit status 0 only if every check of the
// scenario held and the stub counted no violation.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include "hip_stub.h"
#include "spfe.h"

static std::atomic<int> g_failed{0};
static const char *g_weights = nullptr;   // the "SPFW" file
static std::vector<float> g_blob;          // ... and its floats, read once: most creates take the pointer

#define CHECK(cond, ...)                                              \
  do {                                                                \
    if (!(cond)) {                                                    \
      ++g_failed;                                                     \
      fprintf(stderr, "CHECK failed %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);                                   \
      fprintf(stderr, "\n");                                          \
    }                                                                 \
  } while (0)

// A heap block of exactly n elements: the sanitizer's red zone starts where the documented size ends.
template <class T>
struct Exact {
  T *p;
  size_t n;
  explicit Exact(size_t count, int fill = 0) : p(static_cast<T *>(malloc(count ? count * sizeof(T) : 1))), n(count) {
    memset(p, fill, count ? count * sizeof(T) : 1);
  }
  Exact(const Exact &) = delete;
  ~Exact() { free(p); }
  T &operator[](size_t i) { return p[i]; }
  operator T *() { return p; }
};

static spfe_config config(int H, int W, int precision, unsigned flags, int max_batch, int nf = 100) {
  spfe_config c{};
  c.height = H; c.width = W; c.num_features = nf; c.max_batch = max_batch; c.device = 0;
  c.precision = precision; c.flags = flags;
  // every third create reads the file, the others the blob in memory
  static std::atomic<int> turn{0};
  const bool from_file = g_blob.empty() || turn.fetch_add(1) % 3 == 0;
  c.weights = from_file ? nullptr : g_blob.data(); c.weights_path = from_file ? g_weights : nullptr;
  return c;
}

static void expect_clean(const char *what) {
  CHECK(stub_live_ranges() == 0, "%s: %ld live ranges", what, stub_live_ranges());
  CHECK(stub_live_streams() == 0, "%s: %ld live streams", what, stub_live_streams());
  CHECK(stub_live_events() == 0, "%s: %ld live events", what, stub_live_events());
  CHECK(stub_violations() == 0, "%s: %ld violations", what, stub_violations());
}

static std::atomic<uint64_t> g_sink{0};
// reads every byte: memory the library hands out must be live up to its documented extent
static void touch(const void *p, size_t bytes) {
  const volatile uint8_t *q = static_cast<const volatile uint8_t *>(p);
  uint64_t s = 0;
  for (size_t i = 0; i < bytes; ++i) s += q[i];
  g_sink.fetch_add(s, std::memory_order_relaxed);
}
// (no kernel ran: K is 0 everywhere.  The per-keypoint views are read up to the capacity the record gives them, kmax rows:
// a ring slot or a mirror that is short or gone shows there)
static void touch_result(const spfe_result &r, int H, int W, unsigned flags, const char *what, int kmax = 101) {
  const size_t C = (size_t)(H / 8) * (W / 8), K = (size_t)kmax;
  CHECK(r.K == 0 && r.status == 0, "%s: K %d status %d from an all-zero record", what, r.K, r.status);
  CHECK(r.kp_xy && r.kp_response && r.cov2 && r.cov2_inv && r.occ_grid && r.dense_dust && r.semi_dust, "%s: null view", what);
  CHECK((r.desc != nullptr) != ((flags & SPFE_FLAG_DESC_BF16) != 0) && (r.desc_bf16 != nullptr) == ((flags & SPFE_FLAG_DESC_BF16) != 0), "%s: desc views", what);
  touch(r.kp_xy, K * 8); touch(r.kp_response, K * 4); touch(r.cov2, K * 8); touch(r.cov2_inv, K * 8);
  if (r.desc) touch(r.desc, K * 1024);
  if (r.desc_bf16) touch(r.desc_bf16, K * 512);
  touch(r.occ_grid, C * 2); touch(r.dense_dust, C * 4); touch(r.semi_dust, C * 4);
  const bool heat = (flags & SPFE_FLAG_HEAT) != 0, inv = heat && !(flags & SPFE_FLAG_LAZY_HEAT_INV);
  CHECK((r.heat != nullptr) == heat && (r.heat_inv != nullptr) == inv, "%s: heat views", what);
  if (r.heat) touch(r.heat, (size_t)H * W * 4);
  if (r.heat_inv) touch(r.heat_inv, (size_t)H * W * 4);
}

// n frames of H rows of `stride` bytes, each a heap block that ends with the last pixel of the last row
struct Frames {
  std::vector<uint8_t *> ptr;
  Frames(int n, int H, int row_bytes, int stride) {
    for (int i = 0; i < n; ++i) {
      const size_t bytes = (size_t)(H - 1) * stride + row_bytes;
      uint8_t *p = static_cast<uint8_t *>(malloc(bytes));
      for (size_t k = 0; k < bytes; ++k) p[k] = (uint8_t)(k * 7 + i);
      ptr.push_back(p);
    }
  }
  Frames(const Frames &) = delete;
  ~Frames() { for (uint8_t *p : ptr) free(p); }
  const uint8_t *const *data() const { return ptr.data(); }
};

static spfe_handle make(int H, int W, int precision, unsigned flags, int B, int nf = 100) {
  spfe_config c = config(H, W, precision, flags, B, nf);
  spfe_handle h = nullptr;
  const int rc = spfe_create(&c, &h);
  CHECK(rc == SPFE_OK && h, "create %dx%d p%d flags %u B%d -> %d (%s)", W, H, precision, flags, B, rc, spfe_last_error());
  return h;
}

// ---- host_calls --------------------------------------------------------------------------------------------------------
static void host_calls_on(int precision, unsigned flags, bool quick) {
  const int H = 64, W = 96, B = 3;
  const size_t C = (size_t)(H / 8) * (W / 8), HW = (size_t)H * W;
  spfe_handle h = make(H, W, precision, flags, B);
  if (!h) return;
  char what[64];
  snprintf(what, sizeof(what), "host_calls p%d flags %u", precision, flags);
  std::vector<spfe_result> out(B);
  {
    Frames one(1, H, W, W);
    CHECK(spfe_extract(h, one.ptr[0], W, &out[0]) == SPFE_OK, "%s: extract: %s", what, spfe_last_error());
    touch_result(out[0], H, W, flags, what);
    CHECK(spfe_extract(h, nullptr, W, &out[0]) == SPFE_EEMPTY, "%s: null image", what);
    CHECK(spfe_extract(h, one.ptr[0], W - 1, &out[0]) == SPFE_EINVAL, "%s: short stride", what);
  }
  {
    Frames wide(B, H, W, W + 40);
    CHECK(spfe_extract_batch(h, wide.data(), W + 40, B, out.data()) == SPFE_OK, "%s: extract_batch: %s", what, spfe_last_error());
    for (auto &r : out) touch_result(r, H, W, flags, what);
    CHECK(spfe_extract_batch(h, wide.data(), W + 40, B + 1, out.data()) == SPFE_EINVAL, "%s: batch above max_batch", what);
    if (flags & SPFE_FLAG_HEAT) {
      const float *inv = nullptr;
      for (int f = 0; f < B; ++f) {
        CHECK(spfe_fetch_heat_inv(h, f, &inv) == SPFE_OK && inv, "%s: fetch_heat_inv(%d): %s", what, f, spfe_last_error());
        if (inv) touch(inv, HW * 4);
      }
      CHECK(spfe_fetch_heat_inv(h, B, &inv) == SPFE_EINVAL, "%s: fetch_heat_inv beyond the call", what);
    }
    // the call in three parts
    CHECK(spfe_extract_begin(h, wide.data(), W + 40, 2) == SPFE_OK, "%s: begin: %s", what, spfe_last_error());
    CHECK(spfe_extract_begin(h, wide.data(), W + 40, 2) == SPFE_EINVAL, "%s: begin while open", what);
    const float *heat = nullptr, *heat_inv = nullptr;
    CHECK(spfe_extract_maps(h, &heat, nullptr) == SPFE_OK, "%s: maps(heat)", what);
    if (heat) touch(heat, 2 * HW * 4);
    CHECK(spfe_extract_maps(h, &heat, &heat_inv) == SPFE_OK, "%s: maps(both)", what);
    if (heat_inv) touch(heat_inv, 2 * HW * 4);
    for (int f = 0; f < 2; ++f) {
      int K = -1;
      const float *desc = nullptr;
      CHECK(spfe_extract_rows(h, f, &K, &desc) == SPFE_OK && K == 0, "%s: rows(%d)", what, f);
      if (desc) touch(desc, (size_t)K * 1024);
    }
    int K = 0;
    const float *desc = nullptr;
    CHECK(spfe_extract_rows(h, 2, &K, &desc) == SPFE_EINVAL, "%s: rows of a frame not in the call", what);
    CHECK(spfe_extract_finish(h, out.data()) == SPFE_OK, "%s: finish: %s", what, spfe_last_error());
    for (int f = 0; f < 2; ++f) touch_result(out[f], H, W, flags, what);
    CHECK(spfe_extract_finish(h, out.data()) == SPFE_EINVAL, "%s: finish without begin", what);
  }
  if (flags & SPFE_FLAG_HEAT) {   // the maps straight into caller memory of exactly the documented size
    Exact<float> heat(B * HW), heat_inv(B * HW);
    Frames fr(B, H, W, W);
    CHECK(spfe_set_map_buffers(h, heat, heat_inv) == SPFE_OK, "%s: set_map_buffers: %s", what, spfe_last_error());
    CHECK(stub_live_ranges_of(STUB_REGISTERED) == 2, "%s: %ld registered blocks", what, stub_live_ranges_of(STUB_REGISTERED));
    CHECK(spfe_extract_batch(h, fr.data(), W, B, out.data()) == SPFE_OK, "%s: extract into caller maps", what);
    CHECK(out[0].heat == heat.p && out[B - 1].heat == heat.p + (B - 1) * HW, "%s: heat view is not the caller's buffer", what);
    if (!(flags & SPFE_FLAG_LAZY_HEAT_INV)) CHECK(out[1].heat_inv == heat_inv.p + HW, "%s: heat_inv view", what);
    const float *inv = nullptr;
    CHECK(spfe_fetch_heat_inv(h, B - 1, &inv) == SPFE_OK && inv == heat_inv.p + (B - 1) * HW, "%s: lazy fetch into the caller's buffer", what);
    CHECK(spfe_set_map_buffers(h, heat, nullptr) == SPFE_OK, "%s: set_map_buffers(heat, null)", what);
    CHECK(stub_live_ranges_of(STUB_REGISTERED) == 1, "%s: heat_inv not unregistered", what);
    CHECK(spfe_extract(h, fr.ptr[0], W, &out[0]) == SPFE_OK, "%s: extract with one caller map", what);
    touch_result(out[0], H, W, flags, what);
    if (!quick) {
      CHECK(spfe_set_map_buffers(h, nullptr, nullptr) == SPFE_OK, "%s: set_map_buffers(null, null)", what);
      CHECK(stub_live_ranges_of(STUB_REGISTERED) == 0, "%s: maps not unregistered", what);
      CHECK(spfe_extract(h, fr.ptr[0], W, &out[0]) == SPFE_OK && out[0].heat != heat.p, "%s: own maps again", what);
    }   // (quick: the caller's heat buffer is still set when the handle is destroyed)
    spfe_destroy(quick ? h : nullptr);
    if (quick) { expect_clean(what); return; }
  } else {
    CHECK(spfe_set_map_buffers(h, nullptr, nullptr) == SPFE_EINVAL, "%s: set_map_buffers without heat", what);
  }
  {
    Exact<float> semi(B * C * 65), coarse(B * C * 256);
    CHECK(spfe_postprocess(h, semi, coarse, B, out.data()) == SPFE_OK, "%s: postprocess: %s", what, spfe_last_error());
    for (auto &r : out) touch_result(r, H, W, flags, what);
    CHECK(spfe_postprocess(h, semi, coarse, 0, out.data()) == SPFE_EINVAL, "%s: postprocess of no frame", what);
  }
  // staging: with and without maps, 1 / 3 / 4 channels, padded stride
  const int hs = 72, ws = 104;
  Frames gray(1, H, W, W);
  CHECK(spfe_extract_staged(h, gray.ptr[0], W, &out[0]) == SPFE_EINVAL, "%s: staged before set_staging", what);
  for (int with_maps = 0; with_maps < 2; ++with_maps)
    for (int cn : {1, 3, 4}) {
      Exact<float> mx((size_t)hs * ws), my((size_t)hs * ws);
      for (int y = 0; y < hs; ++y)
        for (int x = 0; x < ws; ++x) { mx[(size_t)y * ws + x] = x + 0.25f; my[(size_t)y * ws + x] = y - 0.5f; }
      spfe_staging st{};
      st.src_height = hs; st.src_width = ws; st.channels = cn; st.rgb = cn == 4;
      st.map_x = with_maps ? mx.p : nullptr; st.map_y = with_maps ? my.p : nullptr;
      CHECK(spfe_set_staging(h, &st) == SPFE_OK, "%s: set_staging cn %d maps %d: %s", what, cn, with_maps, spfe_last_error());
      const int stride = ws * cn + 24;
      Frames raw(B, hs, ws * cn, stride), tight(1, hs, ws * cn, ws * cn);
      CHECK(spfe_extract_staged(h, tight.ptr[0], ws * cn, &out[0]) == SPFE_OK, "%s: extract_staged cn %d: %s", what, cn, spfe_last_error());
      touch_result(out[0], H, W, flags, what);
      CHECK(spfe_extract_batch_staged(h, raw.data(), stride, B, out.data()) == SPFE_OK, "%s: extract_batch_staged cn %d: %s", what, cn, spfe_last_error());
      for (auto &r : out) touch_result(r, H, W, flags, what);
      CHECK(spfe_extract_batch_staged(h, raw.data(), ws * cn - 1, B, out.data()) == SPFE_EINVAL, "%s: staged short stride", what);
    }
  {
    spfe_staging bad{};
    bad.src_height = H - 8; bad.src_width = ws; bad.channels = 3;
    CHECK(spfe_set_staging(h, &bad) == SPFE_EINVAL, "%s: source smaller than the frame", what);
    bad.src_height = hs; bad.channels = 2;
    CHECK(spfe_set_staging(h, &bad) == SPFE_EINVAL, "%s: two channels", what);
  }
  {   // a record the caller copied to host memory, and the diagnostics
    Exact<uint8_t> rec(spfe_record_bytes(h));
    spfe_result v{};
    CHECK(spfe_view_record(h, rec, &v) == SPFE_OK && v.K == 0 && v.heat == nullptr, "%s: view_record", what);
    Exact<float> semi(C * 65);
    CHECK(spfe_debug_read(h, "semi", 0, semi, C * 65 * 4) == (long)(C * 65 * 4), "%s: debug_read(semi): %s", what, spfe_last_error());
    CHECK(spfe_debug_read(h, "semi", 0, semi, C * 65 * 4 - 1) < 0, "%s: debug_read into a short buffer", what);
    Exact<uint8_t> img(HW);
    CHECK(spfe_debug_read(h, "image", B - 1, img, HW) == (long)HW, "%s: debug_read(image)", what);
    float ms[32];
    const int ns = spfe_stage_times(h, ms, 32);
    CHECK(ns <= 32, "%s: stage_times wrote %d", what, ns);
    (void)spfe_stage_reset(h);
    CHECK(spfe_stage_name(0)[0] != 0 && spfe_stage_name(-1)[0] == 0, "%s: stage names", what);
  }
  spfe_destroy(h);
  expect_clean(what);
}

static void scenario_host_calls() {
  host_calls_on(SPFE_PRECISION_F32, 0, false);
  host_calls_on(SPFE_PRECISION_F32, SPFE_FLAG_HEAT, false);
  host_calls_on(SPFE_PRECISION_F32, SPFE_FLAG_HEAT | SPFE_FLAG_LAZY_HEAT_INV, false);
  host_calls_on(SPFE_PRECISION_F32, SPFE_FLAG_HEAT, true);
  host_calls_on(SPFE_PRECISION_BF16, SPFE_FLAG_HEAT | SPFE_FLAG_DESC_BF16, false);
  host_calls_on(SPFE_PRECISION_BF16, SPFE_FLAG_HEAT | SPFE_FLAG_LAZY_HEAT_INV | SPFE_FLAG_ASYNC_COV, false);
  Exact<float> in(5), e(5), l(5);
  for (int i = 0; i < 5; ++i) in[i] = 0.5f * i - 1.0f;
  CHECK(spfe_math_probe(in, e, l, 5) == SPFE_OK, "math_probe: %s", spfe_last_error());
  CHECK(spfe_version()[0] != 0 && spfe_abi_version() == SPFE_ABI_VERSION, "version");
  expect_clean("host_calls end");
}

// ---- pipeline ----------------------------------------------------------------------------------------------------------
static void pipeline_on(int H, int W, int precision, unsigned flags, int B) {
  char what[64];
  snprintf(what, sizeof(what), "pipeline %dx%d p%d flags %u", W, H, precision, flags);
  spfe_handle h = make(H, W, precision, flags, B);
  if (!h) return;
  Frames fr(B, H, W, W), wide(B, H, W, W + 32);
  std::vector<spfe_result> out[6];
  for (auto &o : out) o.resize(B);
  long t[8] = {};
  for (int s = 0; s < 3; ++s)
    CHECK(spfe_submit_batch(h, s == 1 ? wide.data() : fr.data(), s == 1 ? W + 32 : W, B, &t[s]) == SPFE_OK, "%s: submit %d: %s", what, s, spfe_last_error());
  CHECK(t[0] != t[1] && t[1] != t[2] && t[0] != t[2], "%s: tickets %ld %ld %ld", what, t[0], t[1], t[2]);
  const long launches = stub_launch_count();
  CHECK(spfe_submit_batch(h, fr.data(), W, B, &t[3]) == SPFE_EINVAL, "%s: fourth submit accepted", what);
  CHECK(stub_launch_count() == launches, "%s: the refused submit launched", what);
  CHECK(spfe_collect_batch(h, t[1], out[1].data()) == SPFE_OK, "%s: collect 1 (out of order): %s", what, spfe_last_error());
  CHECK(spfe_submit_batch(h, fr.data(), W, B, &t[3]) == SPFE_EINVAL, "%s: submit into the oldest batch's slot", what);
  CHECK(spfe_collect_batch(h, t[0], out[0].data()) == SPFE_OK, "%s: collect 0", what);
  CHECK(spfe_submit_batch(h, fr.data(), W, B, &t[3]) == SPFE_OK, "%s: submit 3: %s", what, spfe_last_error());
  CHECK(spfe_submit_batch(h, fr.data(), W, B > 1 ? B - 1 : 1, &t[4]) == SPFE_OK, "%s: short batch: %s", what, spfe_last_error());
  // two further batches submitted since batch 1 was collected, one since batch 0... both still "valid until three further"
  for (int f = 0; f < B; ++f) { touch_result(out[0][f], H, W, flags, what); touch_result(out[1][f], H, W, flags, what); }
  CHECK(spfe_collect_batch(h, t[2], out[2].data()) == SPFE_OK, "%s: collect 2", what);
  CHECK(spfe_collect_batch(h, t[3], out[3].data()) == SPFE_OK, "%s: collect 3", what);
  CHECK(spfe_collect_batch(h, t[4], out[4].data()) == SPFE_OK, "%s: collect 4", what);
  CHECK(spfe_collect_batch(h, t[4], out[5].data()) != SPFE_OK, "%s: a ticket collected twice", what);
  CHECK(spfe_collect_batch(h, 12345, out[5].data()) != SPFE_OK, "%s: an unknown ticket", what);
  for (int f = 0; f < B; ++f) touch_result(out[2][f], H, W, flags, what);
  for (int f = 0; f < (B > 1 ? B - 1 : 1); ++f) touch_result(out[4][f], H, W, flags, what);
  // three further submits behind the collection of batch 4: its views have been handed on to a later batch, but they are
  // still the ring's storage
  for (int s = 5; s < 8; ++s) {
    CHECK(spfe_submit_batch(h, fr.data(), W, B, &t[s]) == SPFE_OK, "%s: submit %d: %s", what, s, spfe_last_error());
    if (s < 7) CHECK(spfe_collect_batch(h, t[s], out[5].data()) == SPFE_OK, "%s: collect %d", what, s);
  }
  touch_result(out[4][0], H, W, flags, what);
  touch_result(out[3][B - 1], H, W, flags, what);
  // a synchronous call between pipelined ones, then destroy with two batches in flight
  CHECK(spfe_collect_batch(h, t[7], out[5].data()) == SPFE_OK, "%s: collect 7", what);
  CHECK(spfe_extract(h, fr.ptr[0], W, &out[5][0]) == SPFE_OK, "%s: extract between submits: %s", what, spfe_last_error());
  CHECK(spfe_submit_batch(h, fr.data(), W, B, &t[0]) == SPFE_OK && spfe_submit_batch(h, wide.data(), W + 32, B, &t[1]) == SPFE_OK, "%s: last submits", what);
  spfe_destroy(h);
  expect_clean(what);
}

static void scenario_pipeline() {
  pipeline_on(120, 160, SPFE_PRECISION_F32, 0, 3);
  pipeline_on(120, 160, SPFE_PRECISION_F32, SPFE_FLAG_HEAT, 3);
  pipeline_on(64, 96, SPFE_PRECISION_BF16, SPFE_FLAG_HEAT | SPFE_FLAG_LAZY_HEAT_INV | SPFE_FLAG_DESC_BF16, 1);
  pipeline_on(720, 1280, SPFE_PRECISION_BF16, SPFE_FLAG_HEAT, 2);   // the twin is built by the first submit
}

// ---- alloc_failure -----------------------------------------------------------------------------------------------------
static void scenario_alloc_failure() {
  struct Cfg { int H, W, precision; unsigned flags; int B; int malloc_step; };
  // The f32 configuration fails at every n of every call.  The bf16 one makes the same calls with a few more tables: its hipMalloc
  // fails at every other n.  The twin's (800x800: the smallest frame that gets one) repeats the bf16 build twice over, handle and
  // twin: its hipMalloc fails at n = 1, 2, 3 and then at every 20th; what it adds is the failure that the library absorbs by
  // giving up the twin.
  const Cfg cfgs[] = {{64, 96, SPFE_PRECISION_F32, SPFE_FLAG_HEAT, 2, 1}, {64, 96, SPFE_PRECISION_BF16, SPFE_FLAG_DESC_BF16, 1, 2},
                      {800, 800, SPFE_PRECISION_BF16, SPFE_FLAG_ASYNC_COV, 2, 20}};
  for (const Cfg &c : cfgs)
    for (const char *api : {"hipMalloc", "hipHostMalloc", "hipStreamCreateWithFlags", "hipEventCreateWithFlags"}) {
      int n = 1, refused = 0, degraded = 0, tried = 0;
      const bool is_malloc = std::string(api) == "hipMalloc";
      for (;; n += n < 3 || !is_malloc ? 1 : c.malloc_step, ++tried) {
        spfe_config cfg = config(c.H, c.W, c.precision, c.flags, c.B);
        spfe_handle h = nullptr;
        stub_fail_after(api, n);
        const int rc = spfe_create(&cfg, &h);
        const bool fired = stub_fail_fired();
        stub_fail_after(api, 0);
        if (!fired) {   // fewer than n calls of this API: the create that nothing disturbed
          CHECK(rc == SPFE_OK && h, "alloc_failure %s: undisturbed create -> %d", api, rc);
          spfe_destroy(h);
          expect_clean("alloc_failure undisturbed");
          break;
        }
        if (rc == SPFE_OK) {   // the one failure the library may absorb: the twin's build (two side chains unavailable)
          int failed = 0;
          CHECK(h && spfe_debug_read(h, "twin_failed", 0, &failed, sizeof(failed)) == 4 && failed == 1,
                "alloc_failure %s #%d: create succeeded although a call failed, and not by giving up the twin", api, n);
          ++degraded;
          spfe_destroy(h);
        } else {
          CHECK(rc == SPFE_EHIP && !h && spfe_last_error()[0], "alloc_failure %s #%d: rc %d handle %p", api, n, rc, (void *)h);
          ++refused;
        }
        char what[80];
        snprintf(what, sizeof(what), "alloc_failure %dx%d %s #%d", c.W, c.H, api, n);
        expect_clean(what);
        if (n > 4000) { CHECK(false, "alloc_failure %s: no end", api); break; }
      }
      printf("alloc_failure %dx%d p%d flags %u: %s failed at %d of its calls (the last: #%d): %d creates refused, %d without the twin\n", c.W,
             c.H, c.precision, c.flags, api, tried, n - 1, refused, degraded);
      CHECK(refused > 0, "alloc_failure %s: never reached", api);
      CHECK(c.malloc_step < 20 || degraded > 0, "alloc_failure %s: no failure fell into the twin's build", api);
    }
  // the first host-array call that grows the staging buffer (hipMalloc) and its pinned mirror (hipHostMalloc)
  const int nq = 5, nt = 7;
  Exact<float> q((size_t)nq * 256), t((size_t)nt * 256);
  Exact<int32_t> idx(nq);
  Exact<float> dist(nq);
  for (const char *api : {"hipMalloc", "hipHostMalloc", "hipDeviceSynchronize", "hipMemcpyAsync", "hipLaunchKernel"}) {
    for (int n = 1;; ++n) {
      spfe_handle h = make(64, 96, SPFE_PRECISION_F32, 0, 1);
      if (!h) break;
      stub_fail_after(api, n);
      const int rc = spfe_match(h, q, nq, t, nt, 1, idx, dist);
      const bool fired = stub_fail_fired();
      stub_fail_after(api, 0);
      if (fired) {
        CHECK(rc == SPFE_EHIP, "alloc_failure spfe_match %s #%d: rc %d", api, n, rc);
        CHECK(spfe_match(h, q, nq, t, nt, 1, idx, dist) == SPFE_OK, "alloc_failure spfe_match %s #%d: the call after the failure: %s", api, n, spfe_last_error());
      } else {
        CHECK(rc == SPFE_OK, "alloc_failure spfe_match undisturbed: %d", rc);
      }
      spfe_destroy(h);
      expect_clean("alloc_failure spfe_match");
      if (!fired || n > 200) break;
    }
  }
}

// ---- stub_selfcheck ----------------------------------------------------------------------------------------------------
static void scenario_stub_selfcheck() {
  std::vector<uint8_t> host(64, 3);
  void *d = stub_malloc_in_block(32, 32);   // 32 "device" bytes in front of 32 bytes that are the stub's own
  CHECK(stub_live_ranges() == 1 && stub_live_ranges_of(STUB_DEVICE) == 1, "one live range");
  CHECK(hipMemcpy(d, host.data(), 32, hipMemcpyHostToDevice) == hipSuccess && stub_violations() == 0, "a copy that fits");
  CHECK(hipMemcpy(d, host.data(), 33, hipMemcpyHostToDevice) != hipSuccess && stub_violations() == 1, "H2D one byte past the range: %ld", stub_violations());
  CHECK(hipMemcpy(host.data(), static_cast<char *>(d) + 1, 32, hipMemcpyDeviceToHost) != hipSuccess && stub_violations() == 2, "D2H one byte past");
  CHECK(hipMemsetAsync(static_cast<char *>(d) + 31, 0, 2, nullptr) != hipSuccess && stub_violations() == 3, "memset one byte past");
  CHECK(hipMemcpy2DAsync(host.data(), 8, d, 8, 8, 4, hipMemcpyDeviceToHost, nullptr) == hipSuccess && stub_violations() == 3, "2D copy that fits");
  CHECK(hipMemcpy2DAsync(host.data(), 8, d, 9, 8, 4, hipMemcpyDeviceToHost, nullptr) != hipSuccess && stub_violations() == 4, "2D copy whose last row leaves");
  CHECK(hipMemcpy(host.data(), host.data() + 32, 8, hipMemcpyDeviceToHost) != hipSuccess && stub_violations() == 5, "D2H from host memory");
  CHECK(hipFree(d) == hipSuccess && stub_violations() == 5 && stub_live_ranges() == 0, "free");
  CHECK(hipFree(d) != hipSuccess && stub_violations() == 6, "double free counted: %ld", stub_violations());
  void *p = nullptr;
  CHECK(hipHostMalloc(&p, 16, 0) == hipSuccess && hipFree(p) != hipSuccess && stub_violations() == 7, "hipFree of pinned memory");
  CHECK(hipHostFree(p) == hipSuccess && hipHostFree(p) != hipSuccess && stub_violations() == 8, "double hipHostFree");
  CHECK(hipMalloc(&p, 100) == hipSuccess && p, "hipMalloc");
  for (int i = 0; i < 100; ++i) CHECK(static_cast<uint8_t *>(p)[i] == 0, "device memory starts as zero");
  CHECK(hipFree(p) == hipSuccess, "free");
  const long launches = stub_launch_count();
  CHECK(hipLaunchKernel(reinterpret_cast<const void *>(&scenario_stub_selfcheck), dim3(4, 0, 1), dim3(64), nullptr, 0, nullptr) != hipSuccess &&
        stub_violations() == 9, "zero grid dimension counted: %ld", stub_violations());
  CHECK(hipLaunchKernel(reinterpret_cast<const void *>(&scenario_stub_selfcheck), dim3(1), dim3(32, 33), nullptr, 0, nullptr) != hipSuccess &&
        stub_violations() == 10, "block above 1024 threads");
  CHECK(hipLaunchKernel(reinterpret_cast<const void *>(&scenario_stub_selfcheck), dim3(1), dim3(64), nullptr, 160 * 1024 + 1, nullptr) != hipSuccess &&
        stub_violations() == 11, "dynamic LDS above 160 KB");
  CHECK(hipLaunchKernel(reinterpret_cast<const void *>(&scenario_stub_selfcheck), dim3(2, 3, 4), dim3(1024), nullptr, 160 * 1024, nullptr) == hipSuccess &&
        stub_violations() == 11, "a launch at the limits");
  CHECK(stub_launch_count() == launches + 4, "launch log");
  const StubLaunch last = stub_launches().back();
  CHECK(last.grid[0] == 2 && last.grid[1] == 3 && last.grid[2] == 4 && last.block[0] == 1024 && last.lds == 160 * 1024 && last.stream == nullptr, "launch record");
  hipStream_t s = nullptr;
  hipEvent_t e = nullptr;
  CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess, "stream, event");
  CHECK(stub_live_streams() == 1 && stub_live_events() == 1, "live stream and event");
  stub_fail_after("hipMalloc", 2);
  CHECK(hipMalloc(&p, 8) == hipSuccess && hipFree(p) == hipSuccess && hipMalloc(&p, 8) == hipErrorOutOfMemory && !p && stub_fail_fired(), "fail_after: the second call");
  CHECK(hipMalloc(&p, 8) == hipSuccess && hipFree(p) == hipSuccess, "fail_after: once only");
  CHECK(hipStreamDestroy(s) == hipSuccess && hipEventDestroy(e) == hipSuccess && stub_live_streams() == 0 && stub_live_events() == 0, "destroy");
  CHECK(stub_violations() == 11 && stub_live_ranges() == 0, "end: %ld violations, %ld ranges", stub_violations(), stub_live_ranges());
  {   // a large block (a mapping of its own): zero, writable to its last byte, held to its size by the registry all the same
    const size_t big = (3u << 20) + 5;
    uint8_t *b = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void **>(&b), big) == hipSuccess && b && b[0] == 0 && b[big - 1] == 0, "a large block");
    b[0] = b[big - 1] = 7;
    CHECK(hipMemset(b, 1, big) == hipSuccess && b[big - 1] == 1 && stub_violations() == 11, "memset of a whole large block");
    CHECK(hipMemset(b + 1, 1, big) != hipSuccess && stub_violations() == 12, "memset one byte past a large block");
    CHECK(hipFree(b) == hipSuccess && stub_live_ranges() == 0 && hipFree(b) != hipSuccess && stub_violations() == 13, "free and double free of a large block");
  }
  stub_reset_violations();
}

// ---- threads -----------------------------------------------------------------------------------------------------------
// Four threads, each with a handle of its own, make every call for the first time in the process at the same moment: the
// launchers' once-per-kernel LDS flags, the call counter and the lazily opened RCCL are the state they share.
static const float kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

static void small_host_forms(spfe_handle h, int H, int W, const char *what) {
  const int nq = 9, nt = 12, n = 20;
  Exact<float> q((size_t)nq * 256), t((size_t)nt * 256), dist(nq);
  Exact<int32_t> idx(nq);
  CHECK(spfe_match(h, q, nq, t, nt, 1, idx, dist) == SPFE_OK, "%s: match: %s", what, spfe_last_error());
  Exact<float> dust((size_t)(H / 8) * (W / 8)), pts((size_t)n * 3), Tout(16), uv((size_t)n * 2);
  Exact<uint8_t> inl(n);
  for (int i = 0; i < n; ++i) { pts[3 * i] = 0.1f * i; pts[3 * i + 1] = 0.05f * i; pts[3 * i + 2] = 2.0f; }
  spfe_dust_params dp{};
  dp.fx = dp.fy = 100; dp.cx = W / 2.0f; dp.cy = H / 2.0f; dp.max_iterations = 40; dp.huber_delta = 0.9; dp.inlier_chi2 = 0.9;
  int n_in = -1, iters = -1;
  CHECK(spfe_align_dust(h, dust, pts, n, kIdentity, &dp, Tout, inl, uv, &n_in, &iters) == SPFE_OK, "%s: align_dust: %s", what, spfe_last_error());
  Exact<float> obs((size_t)n * 2), isig((size_t)n * 2);
  Exact<uint8_t> outl(n);
  spfe_pose_params pp{};
  pp.fx = pp.fy = 100; pp.cx = W / 2.0f; pp.cy = H / 2.0f; pp.schedule = SPFE_POSE_OPTIMIZATION; pp.iterations = 10;
  int its[4] = {}, good = -1;
  CHECK(spfe_refine_pose(h, obs, isig, pts, n, kIdentity, &pp, Tout, outl, its, &good) == SPFE_OK, "%s: refine_pose: %s", what, spfe_last_error());
}

static void scenario_threads() {
  const int NT = 4, H = 64, W = 96, B = 2;
  std::atomic<int> arrived{0};
  auto barrier = [&](int step) {   // every thread reaches step `step` before one goes on
    arrived.fetch_add(1);
    while (arrived.load() < NT * step) std::this_thread::yield();
  };
  std::vector<std::thread> th;
  for (int i = 0; i < NT; ++i)
    th.emplace_back([&, i] {
      char what[32];
      snprintf(what, sizeof(what), "thread %d", i);
      barrier(1);
      spfe_handle h = make(H, W, i & 1 ? SPFE_PRECISION_BF16 : SPFE_PRECISION_F32, SPFE_FLAG_HEAT, B);
      if (!h) {   // (the CHECK has spoken; the others must not wait for this thread)
        for (int step = 2; step <= 6; ++step) barrier(step);
        return;
      }
      std::vector<spfe_result> out(B);
      Frames fr(B, H, W, W + 8);
      barrier(2);
      CHECK(spfe_extract_batch(h, fr.data(), W + 8, B, out.data()) == SPFE_OK, "%s: extract_batch: %s", what, spfe_last_error());
      for (auto &r : out) touch_result(r, H, W, SPFE_FLAG_HEAT, what);
      barrier(3);
      long t = -1;
      CHECK(spfe_submit_batch(h, fr.data(), W + 8, B, &t) == SPFE_OK && spfe_collect_batch(h, t, out.data()) == SPFE_OK, "%s: submit, collect", what);
      barrier(4);
      small_host_forms(h, H, W, what);
      barrier(5);
      uint8_t id[SPFE_COMM_ID_BYTES] = {};
      CHECK(spfe_comm_init(h, id, 0, 1) == SPFE_EHIP, "%s: comm_init without RCCL", what);   // (the lazily opened library: one dlopen)
      CHECK(spfe_extract(h, nullptr, W, &out[0]) == SPFE_EEMPTY && strstr(spfe_last_error(), "empty"), "%s: the thread's own error text", what);
      barrier(6);
      spfe_destroy(h);
    });
  for (auto &t : th) t.join();
  expect_clean("threads");
}

// ---- host_forms --------------------------------------------------------------------------------------------------------
// Every form on host arrays at n = 0, 1, a middle size, the documented maximum and the maximum plus one; every array a heap
// block of exactly the documented size.  The last must be refused with SPFE_EINVAL before any launch.
#define REFUSED(call, ...)                                                                                     \
  do {                                                                                                         \
    const long launches_ = stub_launch_count(), transfers_ = stub_transfers_total();                           \
    const int rc_ = (call);                                                                                    \
    CHECK(rc_ == SPFE_EINVAL, __VA_ARGS__);                                                                    \
    CHECK(stub_launch_count() == launches_, "a refused call launched %ld kernels", stub_launch_count() - launches_); \
    CHECK(stub_transfers_total() == transfers_, "a refused call copied");                                      \
  } while (0)
#define ACCEPTED(call, ...)                                              \
  do {                                                                   \
    const int rc_ = (call);                                              \
    CHECK(rc_ == SPFE_OK, __VA_ARGS__);                                  \
    if (rc_) fprintf(stderr, "  rc %d: %s\n", rc_, spfe_last_error());   \
  } while (0)

struct FrameArrays {   // a frame of K keypoints as the host-array forms take it
  int K;
  Exact<float> kp_xy, kp_desc;
  Exact<int16_t> occ;
  Exact<int32_t> mp_of_kp;
  FrameArrays(int K_, int H, int W) : K(K_), kp_xy((size_t)K_ * 2), kp_desc((size_t)K_ * 256), occ((size_t)(H / 8) * (W / 8), 0xff), mp_of_kp(K_, 0xff) {
    for (int k = 0; k < K; ++k) { kp_xy[2 * k] = (float)(k % W); kp_xy[2 * k + 1] = (float)(k / W % H); }
  }
};
struct PointArrays {   // a list of n map points
  int n;
  Exact<int32_t> id;
  Exact<float> xyz, normal, range, desc;
  Exact<uint8_t> flags;
  explicit PointArrays(int n_) : n(n_), id(n_), xyz((size_t)n_ * 3), normal((size_t)n_ * 3), range((size_t)n_ * 2), desc((size_t)n_ * 256), flags(n_) {
    for (int i = 0; i < n; ++i) { id[i] = i; xyz[3 * i] = 0.01f * (i % 50); xyz[3 * i + 1] = 0.01f * (i % 31); xyz[3 * i + 2] = 2.0f; normal[3 * i + 2] = -1; range[2 * i] = 0.5f; range[2 * i + 1] = 8; flags[i] = SPFE_PROJ_SEARCHABLE; }
  }
};
struct PointOutputs {
  Exact<int32_t> kp_of_mp, holder, idx;
  Exact<float> best, uv, cosv;
  Exact<uint8_t> reason;
  explicit PointOutputs(int n) : kp_of_mp(n), holder(n), idx(n), best(n), uv((size_t)n * 2), cosv(n), reason(n) {}
};

static void forms_match(spfe_handle h) {
  for (int nq : {0, 1, 77, 1500})
    for (int nt : {0, 1, 130}) {
      Exact<float> q((size_t)nq * 256), t((size_t)nt * 256), d1(nq), d2((size_t)nq * 2);
      Exact<int32_t> i1(nq), i2((size_t)nq * 2);
      ACCEPTED(spfe_match(h, q, nq, t, nt, nq & 1, i1, d1), "match %d x %d", nq, nt);
      ACCEPTED(spfe_match_knn2(h, q, nq, t, nt, i2, d2), "knn2 %d x %d", nq, nt);
      if (nq) CHECK(i1[nq - 1] == -1 || nt > 0, "match %d x %d: unmatched entries are -1", nq, nt);
    }
  Exact<float> q(256), d(2);
  Exact<int32_t> i(2);
  REFUSED(spfe_match(h, q, -1, q, 1, 1, i, d), "match: negative n_query");
  REFUSED(spfe_match_knn2(h, q, 1, q, -1, i, d), "knn2: negative n_train");
  REFUSED(spfe_match(h, nullptr, 1, q, 1, 1, i, d), "match: null query");
}

static void forms_patches(spfe_handle h, int H, int W) {
  for (int n : {0, 1, 300, 4096, 4097})
    for (int K : {0, 1, 500, SPFE_PATCH_MAX_KEYPOINTS, SPFE_PATCH_MAX_KEYPOINTS + 1}) {
      if (n == 4096 && K == 500) continue;   // (the two maxima are reached together and each with a small partner)
      const bool too_many = n > 4096 || K > SPFE_PATCH_MAX_KEYPOINTS;
      if ((K >= SPFE_PATCH_MAX_KEYPOINTS) && n != 1 && n != 4096) continue;
      FrameArrays f(K, H, W);
      Exact<float> desc((size_t)n * 256), uv((size_t)n * 2);
      Exact<int32_t> idx(n);
      if (too_many) REFUSED(spfe_match_patches(h, desc, uv, n, f.occ, f.kp_desc, K, 0.75f, idx), "patches n %d K %d", n, K);
      else ACCEPTED(spfe_match_patches(h, desc, uv, n, f.occ, f.kp_desc, K, 0.75f, idx), "patches n %d K %d", n, K);
    }
}

static void forms_dust_pose(spfe_handle h, int H, int W) {
  spfe_dust_params dp{};
  dp.fx = dp.fy = 100; dp.cx = W / 2.0f; dp.cy = H / 2.0f; dp.max_iterations = 40; dp.huber_delta = 0.9; dp.inlier_chi2 = 0.9;
  Exact<float> dust((size_t)(H / 8) * (W / 8)), Tout(16);
  for (int n : {0, 1, 150, SPFE_DUST_MAX_POINTS, SPFE_DUST_MAX_POINTS + 1}) {
    Exact<float> pts((size_t)n * 3), uv((size_t)n * 2);
    Exact<uint8_t> inl(n);
    int n_in = -1, it = -1;
    if (n > SPFE_DUST_MAX_POINTS) REFUSED(spfe_align_dust(h, dust, pts, n, kIdentity, &dp, Tout, inl, uv, &n_in, &it), "align_dust n %d", n);
    else ACCEPTED(spfe_align_dust(h, dust, pts, n, kIdentity, &dp, Tout, inl, uv, &n_in, &it), "align_dust n %d", n);
  }
  spfe_pose_params pp{};
  pp.fx = pp.fy = 100; pp.cx = W / 2.0f; pp.cy = H / 2.0f; pp.schedule = SPFE_POSE_DUST_POST; pp.iterations = 10;
  for (int n : {0, 1, 700, 10001, 10002}) {
    Exact<float> obs((size_t)n * 2), isig((size_t)n * 2), pts((size_t)n * 3);
    Exact<uint8_t> outl(n);
    int its[4] = {}, good = -1;
    pp.schedule = n & 1 ? SPFE_POSE_OPTIMIZATION : SPFE_POSE_DUST_POST;
    if (n > 10001) REFUSED(spfe_refine_pose(h, obs, isig, pts, n, kIdentity, &pp, Tout, outl, its, &good), "refine_pose n %d", n);
    else ACCEPTED(spfe_refine_pose(h, obs, isig, pts, n, kIdentity, &pp, Tout, outl, its, &good), "refine_pose n %d", n);
  }
  pp.schedule = 7;
  Exact<float> one(3);
  Exact<uint8_t> o1(1);
  int its[4], good;
  REFUSED(spfe_refine_pose(h, one, one, one, 1, kIdentity, &pp, Tout, o1, its, &good), "refine_pose: schedule 7");
}

// the four searches that project a list of map points into one frame
static void forms_point_searches(spfe_handle h, int H, int W) {
  spfe_proj_params pj{};
  pj.fx = pj.fy = 100; pj.cx = W / 2.0f; pj.cy = H / 2.0f; pj.mode = SPFE_PROJ_LOCAL_MAP; pj.th = 1; pj.th_dist = 0.7f; pj.view_cos_limit = 0.5f; pj.adaptive = 1; pj.c2_thresh = 81;
  spfe_fuse_params fu{};
  fu.fx = fu.fy = 100; fu.cx = W / 2.0f; fu.cy = H / 2.0f; fu.th = 3; fu.th_dist = 0.3f; fu.chi2 = 5.99; fu.view_cos = 0.5; fu.min_factor = 0.8f; fu.max_factor = 1.2f;
  spfe_loop_proj_params lp{};
  lp.fx = lp.fy = 100; lp.cx = W / 2.0f; lp.cy = H / 2.0f; lp.th = 10; lp.th_dist = 0.7f; lp.view_cos = 0.5; lp.min_factor = 0.8f; lp.max_factor = 1.2f;
  spfe_loop_fuse_params lf{};
  lf.fx = lf.fy = 100; lf.cx = W / 2.0f; lf.cy = H / 2.0f; lf.th = 4; lf.th_dist = 0.7f; lf.view_cos = 0.5; lf.min_factor = 0.8f; lf.max_factor = 1.2f;
  struct Case { int n, K; };
  const int PM = SPFE_PROJ_MAX_POINTS;
  // n at its five sizes against a middle frame; K at its five sizes against a middle list
  const Case proj_cases[] = {{0, 300}, {1, 300}, {900, 300}, {PM, 300}, {PM + 1, 300}, {200, 0}, {200, 1}, {200, SPFE_PROJ_MAX_KEYPOINTS}, {200, SPFE_PROJ_MAX_KEYPOINTS + 1}};
  for (const Case &c : proj_cases) {
    FrameArrays f(c.K, H, W);
    PointArrays p(c.n);
    PointOutputs o(c.n);
    Exact<uint8_t> in_view(c.n);
    int nm = -1, ntm = -1;
    pj.mode = c.n & 1 ? SPFE_PROJ_LAST_FRAME : SPFE_PROJ_LOCAL_MAP;
    const bool bad = c.n > PM || c.K > SPFE_PROJ_MAX_KEYPOINTS;
    if (bad) REFUSED(spfe_search_projection(h, f.kp_xy, f.occ, f.kp_desc, c.K, p.xyz, p.normal, p.desc, p.flags, c.n, f.mp_of_kp, kIdentity, &pj, o.kp_of_mp, in_view, o.uv, o.cosv, &nm, &ntm), "search_projection n %d K %d", c.n, c.K);
    else ACCEPTED(spfe_search_projection(h, f.kp_xy, f.occ, f.kp_desc, c.K, p.xyz, p.normal, p.desc, p.flags, c.n, f.mp_of_kp, kIdentity, &pj, o.kp_of_mp, in_view, o.uv, o.cosv, &nm, &ntm), "search_projection n %d K %d", c.n, c.K);
  }
  pj.th = 9; pj.mode = SPFE_PROJ_LOCAL_MAP;   // 4 th above SPFE_PROJ_MAX_RADIUS
  {
    FrameArrays f(10, H, W);
    PointArrays p(10);
    PointOutputs o(10);
    int nm, ntm;
    REFUSED(spfe_search_projection(h, f.kp_xy, f.occ, f.kp_desc, 10, p.xyz, p.normal, p.desc, p.flags, 10, f.mp_of_kp, kIdentity, &pj, o.kp_of_mp, o.reason, o.uv, o.cosv, &nm, &ntm), "search_projection: radius above the limit");
  }
  const Case fuse_cases[] = {{0, 300}, {1, 300}, {900, 300}, {PM, 300}, {PM + 1, 300}, {200, 0}, {200, 1}, {200, 32767}, {200, 32768}};
  for (const Case &c : fuse_cases) {
    FrameArrays f(c.K, H, W);
    PointArrays p(c.n);
    PointOutputs o(c.n);
    int nf = -1;
    const bool bad = c.n > PM || c.K > 32767;
    if (bad) {
      REFUSED(spfe_fuse_search(h, f.kp_xy, f.occ, f.kp_desc, c.K, f.mp_of_kp, kIdentity, p.id, p.xyz, p.normal, p.range, p.desc, p.flags, c.n, &fu, o.kp_of_mp, o.best, o.holder, o.reason, o.idx, &nf), "fuse_search n %d K %d", c.n, c.K);
      REFUSED(spfe_loop_fuse_search(h, f.kp_xy, f.occ, f.kp_desc, c.K, f.mp_of_kp, kIdentity, p.id, p.xyz, p.normal, p.range, p.desc, p.flags, c.n, &lf, o.kp_of_mp, o.best, o.holder, o.reason, o.idx, &nf), "loop_fuse_search n %d K %d", c.n, c.K);
    } else {
      ACCEPTED(spfe_fuse_search(h, f.kp_xy, f.occ, f.kp_desc, c.K, f.mp_of_kp, kIdentity, p.id, p.xyz, p.normal, p.range, p.desc, p.flags, c.n, &fu, o.kp_of_mp, o.best, o.holder, o.reason, o.idx, &nf), "fuse_search n %d K %d", c.n, c.K);
      ACCEPTED(spfe_loop_fuse_search(h, f.kp_xy, f.occ, f.kp_desc, c.K, f.mp_of_kp, kIdentity, p.id, p.xyz, p.normal, p.range, p.desc, p.flags, c.n, &lf, o.kp_of_mp, o.best, o.holder, o.reason, o.idx, &nf), "loop_fuse_search n %d K %d", c.n, c.K);
      // the outputs may each be null
      ACCEPTED(spfe_loop_fuse_search(h, f.kp_xy, f.occ, f.kp_desc, c.K, f.mp_of_kp, kIdentity, p.id, p.xyz, p.normal, p.range, p.desc, p.flags, c.n, &lf, nullptr, nullptr, nullptr, o.reason, nullptr, &nf), "loop_fuse_search, null outputs, n %d K %d", c.n, c.K);
    }
  }
  const Case loop_cases[] = {{0, 300}, {1, 300}, {900, 300}, {PM, 300}, {PM + 1, 300}, {200, 0}, {200, 1}, {200, SPFE_LOOPPROJ_MAX_KEYPOINTS}, {200, SPFE_LOOPPROJ_MAX_KEYPOINTS + 1}};
  for (const Case &c : loop_cases) {
    FrameArrays f(c.K, H, W);
    PointArrays p(c.n);
    PointOutputs o(c.n);
    int nm = -1;
    const bool bad = c.n > PM || c.K > SPFE_LOOPPROJ_MAX_KEYPOINTS;
    if (bad) REFUSED(spfe_search_loop_points(h, f.kp_xy, f.occ, f.kp_desc, c.K, kIdentity, f.mp_of_kp, p.id, p.xyz, p.normal, p.range, p.desc, p.flags, c.n, &lp, o.kp_of_mp, o.best, o.reason, o.idx, &nm), "search_loop_points n %d K %d", c.n, c.K);
    else ACCEPTED(spfe_search_loop_points(h, f.kp_xy, f.occ, f.kp_desc, c.K, kIdentity, f.mp_of_kp, p.id, p.xyz, p.normal, p.range, p.desc, p.flags, c.n, &lp, o.kp_of_mp, o.best, o.reason, o.idx, &nm), "search_loop_points n %d K %d", c.n, c.K);
  }
}

// the loop closer's three forms on a pair of keyframes, and bundle adjustment
static void forms_loop_pair(spfe_handle h, int H, int W) {
  const int PM = SPFE_PROJ_MAX_POINTS;
  static const float T12[13] = {1, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  spfe_sim3_params sp{};
  sp.fx1 = sp.fy1 = sp.fx2 = sp.fy2 = 100; sp.cx1 = sp.cx2 = W / 2.0f; sp.cy1 = sp.cy2 = H / 2.0f; sp.max_err1 = sp.max_err2 = 9; sp.min_inliers = 20; sp.fix_scale = 0;
  spfe_guided_params gp{};
  gp.fx1 = gp.fy1 = gp.fx2 = gp.fy2 = 100; gp.cx1 = gp.cx2 = W / 2.0f; gp.cy1 = gp.cy2 = H / 2.0f; gp.th = 7.5f; gp.th_dist = 0.7f; gp.min_factor = 0.8f; gp.max_factor = 1.2f;
  spfe_sim3opt_params op{};
  op.fx1 = op.fy1 = op.fx2 = op.fy2 = 100; op.cx1 = op.cx2 = W / 2.0f; op.cy1 = op.cy2 = H / 2.0f; op.th2 = 10; op.fix_scale = 0; op.iterations = 5; op.min_kept = 10; op.min_inliers = 20;
  struct Case { int K1, K2, n, n_hyp; };
  const Case cases[] = {{0, 0, 0, 1},      {1, 1, 1, 1},        {200, 150, 400, 40}, {32767, 150, 400, 40}, {150, 32767, 400, SPFE_SIM3_MAX_HYPOTHESES},
                        {200, 150, PM, 40}, {32768, 150, 400, 40}, {150, 32768, 400, 40}, {200, 150, PM + 1, 40}};
  for (const Case &c : cases) {
    const int kmax = std::max(std::max(c.K1, c.K2), 1);
    FrameArrays f1(c.K1, H, W), f2(c.K2, H, W);
    PointArrays p(c.n);
    Exact<int32_t> match12(c.K1, 0xff);
    Exact<uint32_t> rnd((size_t)c.n_hyp * 3);
    for (int k = 0; k < c.K1 && k < c.K2 && k < c.n; ++k) { match12[k] = k; f1.mp_of_kp[k] = k; f2.mp_of_kp[k] = k; }
    const bool bad = c.K1 > 32767 || c.K2 > 32767 || c.n > PM;
    {
      Exact<uint8_t> out(SPFE_SIM3_OUT_BYTES(kmax, c.n_hyp));
      if (bad) REFUSED(spfe_sim3_ransac(h, c.K1, match12, f1.mp_of_kp, c.K2, f2.mp_of_kp, p.xyz, p.flags, c.n, kIdentity, kIdentity, rnd, c.n_hyp, &sp, out), "sim3_ransac K1 %d K2 %d n %d", c.K1, c.K2, c.n);
      else ACCEPTED(spfe_sim3_ransac(h, c.K1, match12, f1.mp_of_kp, c.K2, f2.mp_of_kp, p.xyz, p.flags, c.n, kIdentity, kIdentity, rnd, c.n_hyp, &sp, out), "sim3_ransac K1 %d K2 %d n %d", c.K1, c.K2, c.n);
    }
    {
      Exact<uint8_t> out(SPFE_GUIDED_OUT_BYTES(kmax));
      if (bad) REFUSED(spfe_search_by_sim3(h, f1.kp_xy, f1.occ, f1.kp_desc, c.K1, f1.mp_of_kp, f2.kp_xy, f2.occ, f2.kp_desc, c.K2, f2.mp_of_kp, p.xyz, p.flags, p.range, p.desc, c.n, kIdentity, kIdentity, T12, match12, &gp, out), "search_by_sim3 K1 %d K2 %d n %d", c.K1, c.K2, c.n);
      else ACCEPTED(spfe_search_by_sim3(h, f1.kp_xy, f1.occ, f1.kp_desc, c.K1, f1.mp_of_kp, f2.kp_xy, f2.occ, f2.kp_desc, c.K2, f2.mp_of_kp, p.xyz, p.flags, p.range, p.desc, c.n, kIdentity, kIdentity, T12, match12, &gp, out), "search_by_sim3 K1 %d K2 %d n %d", c.K1, c.K2, c.n);
    }
    {
      Exact<uint8_t> out(SPFE_SIM3OPT_OUT_BYTES(kmax));
      if (bad) REFUSED(spfe_optimize_sim3(h, f1.kp_xy, c.K1, f1.mp_of_kp, f2.kp_xy, c.K2, f2.mp_of_kp, p.xyz, p.flags, c.n, kIdentity, kIdentity, T12, match12, &op, out), "optimize_sim3 K1 %d K2 %d n %d", c.K1, c.K2, c.n);
      else ACCEPTED(spfe_optimize_sim3(h, f1.kp_xy, c.K1, f1.mp_of_kp, f2.kp_xy, c.K2, f2.mp_of_kp, p.xyz, p.flags, c.n, kIdentity, kIdentity, T12, match12, &op, out), "optimize_sim3 K1 %d K2 %d n %d", c.K1, c.K2, c.n);
    }
  }
  {
    FrameArrays f(10, H, W);
    PointArrays p(10);
    Exact<uint32_t> rnd((size_t)(SPFE_SIM3_MAX_HYPOTHESES + 1) * 3);
    Exact<uint8_t> out(SPFE_SIM3_OUT_BYTES(10, SPFE_SIM3_MAX_HYPOTHESES + 1));
    REFUSED(spfe_sim3_ransac(h, 10, f.mp_of_kp, f.mp_of_kp, 10, f.mp_of_kp, p.xyz, p.flags, 10, kIdentity, kIdentity, rnd, SPFE_SIM3_MAX_HYPOTHESES + 1, &sp, out), "sim3_ransac: 513 hypotheses");
    REFUSED(spfe_sim3_ransac(h, 10, f.mp_of_kp, f.mp_of_kp, 10, f.mp_of_kp, p.xyz, p.flags, 10, kIdentity, kIdentity, rnd, 0, &sp, out), "sim3_ransac: no hypothesis");
  }
  CHECK(spfe_sim3_iteration_limit(100, 0.99, 20, 300) >= 1 && spfe_sim3_iteration_limit(10, 0.99, 20, 300) == 1, "sim3_iteration_limit");
  CHECK(spfe_sim3opt_lds_edge_capacity(h, 0) > 0 && spfe_ba_lds_free_capacity(h) > 0 && spfe_pose_lds_edge_capacity(h) > 0, "the capacity getters");
  // the loop's corrected poses (no handle)
  for (int nt : {0, 1, 20, SPFE_FUSE_MAX_TARGETS, SPFE_FUSE_MAX_TARGETS + 1}) {
    Exact<double> S12(13);
    S12[0] = 1; S12[1] = S12[5] = S12[9] = 1;
    Exact<float> Tiw((size_t)nt * 16), Siw((size_t)nt * 16), Tc((size_t)nt * 16);
    for (int i = 0; i < nt; ++i) for (int d = 0; d < 4; ++d) Tiw[(size_t)i * 16 + 5 * d] = 1;
    const int rc = spfe_loop_corrected_poses(S12, kIdentity, kIdentity, Tiw, nt, nt ? nt - 1 : 0, Siw, Tc);
    CHECK(nt >= 1 && nt <= SPFE_FUSE_MAX_TARGETS ? rc == SPFE_OK : rc == SPFE_EINVAL, "loop_corrected_poses n_targets %d -> %d (%s)", nt, rc, spfe_last_error());
  }
}

static void forms_ba(spfe_handle h, int H, int W) {
  spfe_ba_params bp{};
  bp.fx = bp.fy = 100; bp.cx = W / 2.0f; bp.cy = H / 2.0f; bp.schedule = SPFE_BA_LOCAL; bp.iterations[0] = 5; bp.iterations[1] = 10; bp.robust = 1; bp.inv_sigma2 = 1;
  struct Case { int n_kf, n, E, n_free; };
  const Case cases[] = {{1, 0, 0, 0},  {1, 1, 1, 1},  {12, 300, 2000, 5},  {SPFE_BA_MAX_KEYFRAMES, 300, 2000, SPFE_BA_MAX_FREE},  {12, SPFE_BA_MAX_POINTS, 2000, 5},
                        {12, 300, SPFE_BA_MAX_EDGES, 5},  {SPFE_BA_MAX_KEYFRAMES + 1, 300, 2000, 5},  {SPFE_BA_MAX_KEYFRAMES, 300, 2000, SPFE_BA_MAX_FREE + 1},
                        {12, SPFE_BA_MAX_POINTS + 1, 2000, 5},  {12, 300, SPFE_BA_MAX_EDGES + 1, 5},  {0, 0, 0, 0}};
  for (const Case &c : cases) {
    Exact<int32_t> edges((size_t)c.E * 3);
    Exact<float> obs((size_t)c.E * 2), isig((size_t)c.E * 2), Tcw((size_t)c.n_kf * 16), xyz((size_t)c.n * 3);
    Exact<uint8_t> fixed(c.n_kf, 1), out(SPFE_BA_OUT_BYTES(c.n_kf, c.n, c.E));
    for (int i = 0; i < c.n_free && i < c.n_kf; ++i) fixed[i] = 0;
    for (int k = 0; k < c.n_kf; ++k) for (int d = 0; d < 4; ++d) Tcw[(size_t)k * 16 + 5 * d] = 1;
    for (int e = 0; e < c.E; ++e) { edges[3 * e] = c.n ? (int)((size_t)e * c.n / c.E) : 0; edges[3 * e + 1] = e % std::max(c.n_kf, 1); edges[3 * e + 2] = e % 50; isig[2 * e] = isig[2 * e + 1] = 1; }
    for (int i = 0; i < c.n; ++i) xyz[3 * i + 2] = 2;
    bp.schedule = c.E & 1 ? SPFE_BA_FULL : SPFE_BA_LOCAL;
    const bool bad = c.n_kf < 1 || c.n_kf > SPFE_BA_MAX_KEYFRAMES || c.n > SPFE_BA_MAX_POINTS || c.E > SPFE_BA_MAX_EDGES || c.n_free > SPFE_BA_MAX_FREE;
    if (bad) REFUSED(spfe_bundle_adjust(h, edges, obs, isig, c.E, Tcw, fixed, c.n_kf, xyz, c.n, &bp, nullptr, out), "bundle_adjust n_kf %d n %d E %d free %d", c.n_kf, c.n, c.E, c.n_free);
    else ACCEPTED(spfe_bundle_adjust(h, edges, obs, isig, c.E, Tcw, fixed, c.n_kf, xyz, c.n, &bp, nullptr, out), "bundle_adjust n_kf %d n %d E %d free %d", c.n_kf, c.n, c.E, c.n_free);
    if (bad) for (size_t i = 0; i < out.n; ++i) if (out[i]) { CHECK(false, "bundle_adjust: a refused call wrote `out`"); break; }
  }
  Exact<float> T(16), x(3);
  Exact<uint8_t> fx(1), out(SPFE_BA_OUT_BYTES(1, 1, 0));
  bp.schedule = SPFE_BA_LOCAL; bp.iterations[0] = 1001;
  REFUSED(spfe_bundle_adjust(h, nullptr, nullptr, nullptr, 0, T, fx, 1, x, 1, &bp, nullptr, out), "bundle_adjust: 1001 iterations");
  bp.iterations[0] = 5; bp.schedule = 2;
  REFUSED(spfe_bundle_adjust(h, nullptr, nullptr, nullptr, 0, T, fx, 1, x, 1, &bp, nullptr, out), "bundle_adjust: schedule 2");
}

// the map-point table, the essential graph and the loop detection
static void forms_map_graph(spfe_handle h) {
  spfe_mp_params mp{};
  mp.mode = SPFE_MP_DESC | SPFE_MP_NORMAL_DEPTH; mp.level_scale = 1; mp.top_scale = 1;
  // (E at SPFE_MP_MAX_EDGES would need 4 GiB of observation rows: the edge count is taken to 40,000 and to the limit plus one)
  struct MpCase { int m, E; };
  const MpCase mp_cases[] = {{0, 0}, {1, 1}, {500, 4000}, {SPFE_MP_MAX_POINTS, 40000}, {SPFE_MP_MAX_POINTS + 1, 10}, {10, SPFE_MP_MAX_EDGES + 1}};
  for (const MpCase &c : mp_cases) {
    const bool bad = c.m > SPFE_MP_MAX_POINTS || c.E > SPFE_MP_MAX_EDGES;
    const int E = bad && c.E > SPFE_MP_MAX_EDGES ? 10 : c.E;   // rows allocated (a refused call reads none)
    Exact<int32_t> start((size_t)c.m + 1);
    for (int i = 0; i <= c.m; ++i) start[i] = c.m ? (int)((size_t)i * c.E / c.m) : 0;
    Exact<float> od((size_t)E * 256), ow((size_t)E * 3), rw((size_t)c.m * 3), xyz((size_t)c.m * 3), nrm((size_t)c.m * 3), rng((size_t)c.m * 2), desc((size_t)c.m * 256);
    Exact<uint8_t> good(E, 1), flags(c.m, 1), out(SPFE_MP_OUT_BYTES(c.m));
    if (bad) REFUSED(spfe_refresh_map_points(h, start, od, good, ow, c.E, rw, xyz, flags, c.m, &mp, nrm, rng, desc, out), "refresh_map_points m %d E %d", c.m, c.E);
    else ACCEPTED(spfe_refresh_map_points(h, start, od, good, ow, c.E, rw, xyz, flags, c.m, &mp, nrm, rng, desc, out), "refresh_map_points m %d E %d", c.m, c.E);
  }
  CHECK(spfe_mp_lds_obs_capacity(h, 4) > 0 && spfe_mp_lds_obs_capacity(h, 2) >= spfe_mp_lds_obs_capacity(h, 4), "mp_lds_obs_capacity");
  // the essential graph: a chain with a loop edge
  spfe_essgraph_params ep{};
  ep.iterations = 20; ep.fix_scale = 0; ep.lambda_init = 1e-16;
  struct EgCase { int n, E; };
  const EgCase eg_cases[] = {{1, 0}, {2, 1}, {70, 90}, {SPFE_ESSGRAPH_MAX_KEYFRAMES, 20000}, {300, SPFE_ESSGRAPH_MAX_EDGES}, {SPFE_ESSGRAPH_MAX_KEYFRAMES + 1, 10}, {300, SPFE_ESSGRAPH_MAX_EDGES + 1}, {0, 0}};
  for (const EgCase &c : eg_cases) {
    const int n = c.n;
    Exact<double> est((size_t)n * 8), meas((size_t)n * 8);
    Exact<uint8_t> flags(n), out(SPFE_ESSGRAPH_OUT_BYTES(n));
    Exact<int32_t> edges((size_t)c.E * 3), first(n);
    for (int i = 0; i < n; ++i) { est[(size_t)i * 8 + 3] = meas[(size_t)i * 8 + 3] = 1; est[(size_t)i * 8 + 7] = meas[(size_t)i * 8 + 7] = 1; }
    if (n) flags[0] = 1;
    for (int e = 0; e < c.E; ++e) { edges[3 * e] = n > 1 ? e % (n - 1) : 0; edges[3 * e + 1] = n > 1 ? e % (n - 1) + 1 : 0; edges[3 * e + 2] = e & 1; }
    const bool bad = n < 1 || n > SPFE_ESSGRAPH_MAX_KEYFRAMES || c.E > SPFE_ESSGRAPH_MAX_EDGES;
    int unknown = -1, blocks = -1;
    const int erc = spfe_essential_graph_envelope(n, flags, edges, c.E, first, &unknown, &blocks);
    CHECK(bad ? erc < 0 : erc >= 0, "essential_graph_envelope n %d E %d -> %d", n, c.E, erc);
    const int env_cap = bad ? 16 : blocks;
    if (bad) REFUSED(spfe_optimize_essential_graph(h, est, meas, flags, n, edges, c.E, env_cap, &ep, out), "optimize_essential_graph n %d E %d", n, c.E);
    else ACCEPTED(spfe_optimize_essential_graph(h, est, meas, flags, n, edges, c.E, env_cap, &ep, out), "optimize_essential_graph n %d E %d", n, c.E);
    // the start values and the map correction on the same sizes
    Exact<float> Tcw((size_t)n * 16);
    Exact<double> S12(13);
    S12[0] = 1; S12[1] = S12[5] = S12[9] = 1;
    Exact<int32_t> conn(n ? 1 : 0);
    const int src = spfe_essential_graph_sim3(Tcw, S12, kIdentity, kIdentity, conn, n ? 1 : 0, n ? 0 : -1, est, meas, n);
    CHECK(n < 1 || n > SPFE_ESSGRAPH_MAX_KEYFRAMES ? src == SPFE_EINVAL : src == SPFE_OK, "essential_graph_sim3 n %d -> %d (%s)", n, src, spfe_last_error());
  }
  {
    Exact<double> one(8);
    Exact<uint8_t> f(1), out(SPFE_ESSGRAPH_OUT_BYTES(1));
    REFUSED(spfe_optimize_essential_graph(h, one, one, f, 1, nullptr, 0, SPFE_ESSGRAPH_MAX_BLOCKS + 1, &ep, out), "optimize_essential_graph: env_cap above the limit");
    ep.iterations = 1001;
    REFUSED(spfe_optimize_essential_graph(h, one, one, f, 1, nullptr, 0, 0, &ep, out), "optimize_essential_graph: 1001 iterations");
  }
  for (int m : {0, 1, 900, SPFE_MP_MAX_POINTS, SPFE_MP_MAX_POINTS + 1}) {
    const int n_kf = 5, n_table = m > SPFE_MP_MAX_POINTS ? 16 : m + 3, rows = m > SPFE_MP_MAX_POINTS ? 16 : m;
    Exact<double> from((size_t)n_kf * 8), to((size_t)n_kf * 8);
    for (int k = 0; k < n_kf; ++k) { from[k * 8 + 3] = to[k * 8 + 3] = 1; from[k * 8 + 7] = to[k * 8 + 7] = 1; }
    Exact<int32_t> ref(rows), idx(rows);
    for (int i = 0; i < rows; ++i) { ref[i] = i % n_kf; idx[i] = rows - 1 - i; }
    Exact<float> xyz((size_t)n_table * 3);
    Exact<uint8_t> flags(n_table, 1), code(rows);
    if (m > SPFE_MP_MAX_POINTS) REFUSED(spfe_correct_map_points(h, from, to, n_kf, ref, idx, m, xyz, flags, n_table, code), "correct_map_points m %d", m);
    else {
      ACCEPTED(spfe_correct_map_points(h, from, to, n_kf, ref, idx, m, xyz, flags, n_table, code), "correct_map_points m %d", m);
      ACCEPTED(spfe_correct_map_points(h, from, to, n_kf, ref, nullptr, m, xyz, flags, n_table, code), "correct_map_points m %d, rows in order", m);
    }
  }
  // the loop detection
  spfe_loopdet_params lp{};
  lp.min_score_init = 0.2f; lp.min_score_floor = 0.2f; lp.retain_ratio = 0.75f;
  struct LdCase { int n_slots, dim; };
  const LdCase ld_cases[] = {{1, 4}, {50, 4096}, {SPFE_LOOPDET_MAX_KEYFRAMES, 64}, {SPFE_LOOPDET_MAX_KEYFRAMES + 1, 64}, {50, SPFE_GLOBAL_DESC_DIM + 4}, {50, 6}, {0, 64}};
  for (const LdCase &c : ld_cases) {
    const bool bad = c.n_slots < 1 || c.n_slots > SPFE_LOOPDET_MAX_KEYFRAMES || c.dim < 4 || c.dim > SPFE_GLOBAL_DESC_DIM || c.dim % 4;
    const int ns = bad ? 8 : c.n_slots, n_conn = std::min(ns, 7), n_cov = std::min(ns, 5);
    float *g = nullptr;
    CHECK(posix_memalign(reinterpret_cast<void **>(&g), 16, (size_t)ns * c.dim * 4) == 0, "gdesc");   // (the form asks for 16-byte alignment)
    memset(g, 0, (size_t)ns * c.dim * 4);
    uint8_t *out = nullptr;
    CHECK(posix_memalign(reinterpret_cast<void **>(&out), 16, SPFE_LOOPDET_OUT_BYTES(ns)) == 0, "out");
    Exact<uint8_t> kf(ns), db(ns, 1);
    Exact<int32_t> best((size_t)ns * SPFE_LOOPDET_NEIGH, 0xff), conn(n_conn), cov(n_cov);
    for (int i = 0; i < n_cov; ++i) cov[i] = ns - 1 - i;
    if (bad) REFUSED(spfe_detect_loop_candidates(h, g, c.dim, kf, db, best, c.n_slots, 0, conn, n_conn, cov, n_cov, &lp, out), "detect_loop_candidates n_slots %d dim %d", c.n_slots, c.dim);
    else ACCEPTED(spfe_detect_loop_candidates(h, g, c.dim, kf, db, best, c.n_slots, ns - 1, conn, n_conn, cov, n_cov, &lp, out), "detect_loop_candidates n_slots %d dim %d", c.n_slots, c.dim);
    free(g);
    free(out);
  }
}

// the local map, the covisibility graph, the culling and the counts, on host arrays
struct Graph {
  Exact<int32_t> conn_slot, conn_w, conn_n, ord_slot, ord_w, ord_n, parent;
  Exact<uint8_t> first;
  spfe_covis_graph g{};
  Graph(int n_slots, int conn_cap, int alloc_slots, int alloc_cap)
      : conn_slot((size_t)alloc_slots * alloc_cap, 0xff), conn_w((size_t)alloc_slots * alloc_cap), conn_n(alloc_slots), ord_slot((size_t)alloc_slots * alloc_cap, 0xff),
        ord_w((size_t)alloc_slots * alloc_cap), ord_n(alloc_slots), parent(alloc_slots, 0xff), first(alloc_slots, 1) {
    g.d_conn_slot = conn_slot.p; g.d_conn_w = conn_w.p; g.d_conn_n = conn_n.p; g.d_ord_slot = ord_slot.p; g.d_ord_w = ord_w.p; g.d_ord_n = ord_n.p;
    g.d_parent = parent.p; g.d_first_conn = first.p; g.n_slots = n_slots; g.conn_cap = conn_cap;
  }
};
static void *aligned_block(size_t bytes) {
  void *p = nullptr;
  if (posix_memalign(&p, 16, bytes)) return nullptr;
  memset(p, 0, bytes);
  return p;
}

static void forms_resident_state(spfe_handle h) {
  struct Case { int n_slots, kp_stride, n_table, n_kp, point_cap, n_best, conn_cap; };
  const int PM = SPFE_PROJ_MAX_POINTS;
  const Case cases[] = {{1, 1, 0, 0, 1, 1, 1},
                        {40, 37, 500, 30, 600, 20, 16},
                        {SPFE_LOCALMAP_MAX_KEYFRAMES, 3, 1000, 100, 1000, 2, 4},
                        {6, SPFE_LOCALMAP_MAX_STRIDE, SPFE_MP_MAX_POINTS, PM, PM, SPFE_LOCALMAP_MAX_BEST, SPFE_COVIS_MAX_CONN},
                        {SPFE_LOCALMAP_MAX_KEYFRAMES + 1, 3, 1000, 100, 1000, 2, 4},
                        {40, SPFE_LOCALMAP_MAX_STRIDE + 1, 500, 30, 600, 20, 16},
                        {40, 37, SPFE_MP_MAX_POINTS + 1, 30, 600, 20, 16},
                        {40, 37, 500, 601, 600, 20, 16},
                        {40, 37, 500, 30, PM + 1, 20, 16},
                        {40, 37, 500, 30, 600, SPFE_LOCALMAP_MAX_BEST + 1, 16},
                        {40, 37, 500, 30, 600, 20, SPFE_COVIS_MAX_CONN + 1},
                        {0, 37, 500, 30, 600, 20, 16}};
  for (const Case &c : cases) {
    const bool bad_lm = c.n_slots < 1 || c.n_slots > SPFE_LOCALMAP_MAX_KEYFRAMES || c.kp_stride > SPFE_LOCALMAP_MAX_STRIDE || c.n_table > SPFE_MP_MAX_POINTS ||
                        c.n_kp > c.point_cap || c.point_cap > PM || c.n_best > SPFE_LOCALMAP_MAX_BEST;
    const bool bad_cv = c.n_slots < 1 || c.n_slots > SPFE_LOCALMAP_MAX_KEYFRAMES || c.kp_stride > SPFE_LOCALMAP_MAX_STRIDE || c.n_table > SPFE_MP_MAX_POINTS ||
                        c.n_best > SPFE_LOCALMAP_MAX_BEST || c.conn_cap > SPFE_COVIS_MAX_CONN;
    // a refused call reads nothing: its arrays are those of the middle case
    const bool any_bad = bad_lm || bad_cv;
    const int ns = any_bad ? 40 : c.n_slots, st = any_bad ? 37 : c.kp_stride, nt = any_bad ? 500 : c.n_table, nk = any_bad ? 30 : c.n_kp;
    const int pc = any_bad ? 600 : c.point_cap, nb = any_bad ? 20 : c.n_best, cc = any_bad ? 16 : c.conn_cap;
    Exact<int32_t> rows((size_t)ns * st, 0xff), best((size_t)ns * nb, 0xff), best_b((size_t)ns * SPFE_LOOPDET_NEIGH, 0xff), parent(ns, 0xff), mp_of_kp(nk, 0xff), nobs(nt);
    Exact<uint8_t> kf_flags(ns), mp_flags(nt, 1);
    for (int s = 0; s < ns && nt; ++s) for (int k = 0; k < st && k < 40; ++k) rows[(size_t)s * st + k] = (s * 7 + k) % nt;
    for (int k = 0; k < nk && nt; ++k) mp_of_kp[k] = k % nt;
    spfe_localmap_params lm{};
    lm.max_keyframes = 80; lm.point_cap = c.point_cap;
    {
      void *out = aligned_block(SPFE_LOCALMAP_OUT_BYTES(ns, pc, nk));
      if (bad_lm) REFUSED(spfe_update_local_map(h, rows, c.kp_stride, kf_flags, best, c.n_best, parent, c.n_slots, mp_flags, c.n_table, mp_of_kp, c.n_kp, &lm, out), "update_local_map slots %d stride %d table %d kp %d cap %d best %d", c.n_slots, c.kp_stride, c.n_table, c.n_kp, c.point_cap, c.n_best);
      else ACCEPTED(spfe_update_local_map(h, rows, c.kp_stride, kf_flags, best, c.n_best, parent, c.n_slots, mp_flags, c.n_table, mp_of_kp, c.n_kp, &lm, out), "update_local_map slots %d stride %d table %d kp %d cap %d best %d", c.n_slots, c.kp_stride, c.n_table, c.n_kp, c.point_cap, c.n_best);
      free(out);
    }
    if (bad_lm && !bad_cv) continue;   // (a frame too large for the local map alone: the graph forms take no frame)
    Graph gr(c.n_slots, c.conn_cap, ns, cc);
    spfe_covis_params cv{};
    cv.th = 15; cv.origin_slot = 0;
    {
      void *out = aligned_block(SPFE_COVIS_OUT_BYTES(ns, cc));
      const int cur = ns - 1;
      if (bad_cv) REFUSED(spfe_update_connections(h, &gr.g, rows, c.kp_stride, kf_flags, mp_flags, c.n_table, c.n_slots > 0 ? cur : 0, &cv, best, c.n_best, best_b, SPFE_LOOPDET_NEIGH, out), "update_connections slots %d stride %d table %d best %d conn_cap %d", c.n_slots, c.kp_stride, c.n_table, c.n_best, c.conn_cap);
      else ACCEPTED(spfe_update_connections(h, &gr.g, rows, c.kp_stride, kf_flags, mp_flags, c.n_table, cur, &cv, best, c.n_best, best_b, SPFE_LOOPDET_NEIGH, out), "update_connections slots %d stride %d table %d best %d conn_cap %d", c.n_slots, c.kp_stride, c.n_table, c.n_best, c.conn_cap);
      free(out);
    }
    spfe_cull_params cu{};
    cu.th_obs = 3; cu.cov_ratio = 0.9f; cu.origin_slot = 0; cu.bad_cap = std::min(nt, 1000);
    {
      void *out = aligned_block(SPFE_CULL_OUT_BYTES(ns, cc, cu.bad_cap));
      const int cur = ns - 1;
      if (bad_cv) REFUSED(spfe_cull_keyframes(h, &gr.g, rows, c.kp_stride, kf_flags, mp_flags, nobs, c.n_table, c.n_slots > 0 ? cur : 0, &cu, best, c.n_best, best_b, SPFE_LOOPDET_NEIGH, out), "cull_keyframes slots %d stride %d table %d best %d conn_cap %d", c.n_slots, c.kp_stride, c.n_table, c.n_best, c.conn_cap);
      else ACCEPTED(spfe_cull_keyframes(h, &gr.g, rows, c.kp_stride, kf_flags, mp_flags, nobs, c.n_table, cur, &cu, best, c.n_best, best_b, SPFE_LOOPDET_NEIGH, out), "cull_keyframes slots %d stride %d table %d best %d conn_cap %d", c.n_slots, c.kp_stride, c.n_table, c.n_best, c.conn_cap);
      free(out);
    }
  }
  {
    Graph gr(4, 4, 4, 4);
    Exact<int32_t> rows(16, 0xff), nobs(8);
    Exact<uint8_t> kf(4), mpf(8, 1);
    spfe_cull_params cu{};
    cu.th_obs = 0; cu.cov_ratio = 0.9f; cu.origin_slot = -1; cu.bad_cap = 8;
    void *out = aligned_block(SPFE_CULL_OUT_BYTES(4, 4, 8));
    REFUSED(spfe_cull_keyframes(h, &gr.g, rows, 4, kf, mpf, nobs, 8, 1, &cu, nullptr, 1, nullptr, 1, out), "cull_keyframes: th_obs 0");
    cu.th_obs = 3; cu.bad_cap = SPFE_MP_MAX_POINTS + 1;
    REFUSED(spfe_cull_keyframes(h, &gr.g, rows, 4, kf, mpf, nobs, 8, 1, &cu, nullptr, 1, nullptr, 1, out), "cull_keyframes: bad_cap above the limit");
    free(out);
  }
}

// map-point culling (admission, statistics, cull loop) and the two forms around the local BA, on host arrays
struct Life {
  Exact<uint8_t> flags;
  Exact<int32_t> nobs, found, visible, first_kf, recent, recent_n;
  spfe_mp_life l{};
  Life(int n_table, int recent_cap, int alloc_table, int alloc_recent)
      : flags(alloc_table, 1), nobs(alloc_table), found(alloc_table), visible(alloc_table), first_kf(alloc_table, 0xff), recent(alloc_recent, 0xff), recent_n(1) {
    l.d_mp_flags = flags.p; l.d_mp_nobs = nobs.p; l.d_mp_found = found.p; l.d_mp_visible = visible.p; l.d_mp_first_kf = first_kf.p;
    l.d_recent = recent.p; l.d_recent_n = recent_n.p; l.n_table = n_table; l.recent_cap = recent_cap;
  }
};

static void forms_map_point_culling(spfe_handle h) {
  struct Case { int n_slots, kp_stride, n_table, recent_cap, n_neigh, n_kp, point_cap, bad_cap; };
  const int PM = SPFE_PROJ_MAX_POINTS, MP = SPFE_MP_MAX_POINTS;
  const Case mid = {40, 37, 500, 300, 3, 30, 600, 100};
  const Case cases[] = {{1, 1, 1, 1, 1, 0, 1, 0},
                        mid,
                        {SPFE_LOCALMAP_MAX_KEYFRAMES, 3, 1000, 1000, SPFE_TRI_MAX_NEIGHBOURS, PM, PM, 1000},
                        {6, SPFE_LOCALMAP_MAX_STRIDE, MP, MP, 2, 100, 600, MP},
                        {SPFE_LOCALMAP_MAX_KEYFRAMES + 1, 37, 500, 300, 3, 30, 600, 100},
                        {40, SPFE_LOCALMAP_MAX_STRIDE + 1, 500, 300, 3, 30, 600, 100},
                        {40, 37, MP + 1, 300, 3, 30, 600, 100},
                        {40, 37, 500, MP + 1, 3, 30, 600, 100},
                        {40, 37, 500, 300, SPFE_TRI_MAX_NEIGHBOURS + 1, 30, 600, 100},
                        {40, 37, 500, 300, 3, PM + 1, 600, 100},
                        {40, 37, 500, 300, 3, 30, PM + 1, 100},
                        {40, 37, 500, 300, 3, 30, 600, MP + 1},
                        {0, 37, 500, 300, 3, 30, 600, 100},
                        {40, 37, 0, 300, 3, 30, 600, 100}};
  const size_t tri_bytes = spfe_tri_out_bytes(h);
  for (const Case &c : cases) {
    const bool bad_life = c.n_table < 1 || c.n_table > MP || c.recent_cap < 1 || c.recent_cap > MP;
    const bool bad_rows = c.n_slots < 1 || c.n_slots > SPFE_LOCALMAP_MAX_KEYFRAMES || c.kp_stride > SPFE_LOCALMAP_MAX_STRIDE;
    const bool bad_admit = bad_life || bad_rows || c.n_neigh > SPFE_TRI_MAX_NEIGHBOURS;
    const bool bad_stat = bad_life || c.n_kp > PM || c.point_cap > PM;
    const bool bad_cull = bad_life || bad_rows || c.bad_cap > MP;
    // a refused call reads nothing: its arrays are those of the middle case
    const Case &a = bad_admit || bad_stat || bad_cull ? mid : c;
    Life life(c.n_table, c.recent_cap, a.n_table, a.recent_cap);
    Exact<int32_t> rows((size_t)a.n_slots * a.kp_stride, 0xff);
    Exact<uint8_t> kf_flags(a.n_slots);
    {
      Exact<uint8_t> tri((size_t)a.n_neigh * tri_bytes);
      Exact<int32_t> neigh(a.n_neigh);
      Exact<float> xyz((size_t)a.n_table * 3);
      void *out = aligned_block(SPFE_ADMIT_OUT_BYTES);
      if (bad_admit) REFUSED(spfe_admit_map_points(h, &life.l, tri, c.n_neigh, neigh, 0, 7, rows, c.kp_stride, c.n_slots, xyz, out), "admit_map_points slots %d stride %d table %d recent %d neigh %d", c.n_slots, c.kp_stride, c.n_table, c.recent_cap, c.n_neigh);
      else ACCEPTED(spfe_admit_map_points(h, &life.l, tri, c.n_neigh, neigh, 0, 7, rows, c.kp_stride, c.n_slots, xyz, out), "admit_map_points slots %d stride %d table %d recent %d neigh %d", c.n_slots, c.kp_stride, c.n_table, c.recent_cap, c.n_neigh);
      free(out);
    }
    {
      Exact<int32_t> entry(a.n_kp, 0xff), after(a.n_kp, 0xff), point_idx(a.point_cap, 0xff);
      Exact<uint8_t> in_view(a.point_cap), outlier(a.n_kp);
      void *out = aligned_block(SPFE_MPSTAT_OUT_BYTES);
      if (bad_stat) REFUSED(spfe_track_statistics(h, &life.l, entry, after, c.n_kp, point_idx, c.point_cap, in_view, outlier, out), "track_statistics table %d recent %d kp %d cap %d", c.n_table, c.recent_cap, c.n_kp, c.point_cap);
      else ACCEPTED(spfe_track_statistics(h, &life.l, entry, after, c.n_kp, point_idx, c.point_cap, in_view, outlier, out), "track_statistics table %d recent %d kp %d cap %d", c.n_table, c.recent_cap, c.n_kp, c.point_cap);
      free(out);
    }
    {
      spfe_mpcull_params cu{};
      cu.cur_kf_id = 9; cu.th_obs = 2; cu.found_ratio = 0.25f; cu.bad_cap = c.bad_cap;
      void *out = aligned_block(SPFE_MPCULL_OUT_BYTES(a.recent_cap, a.bad_cap));
      if (bad_cull) REFUSED(spfe_cull_map_points(h, &life.l, rows, c.kp_stride, kf_flags, c.n_slots, &cu, out), "cull_map_points slots %d stride %d table %d recent %d bad_cap %d", c.n_slots, c.kp_stride, c.n_table, c.recent_cap, c.bad_cap);
      else ACCEPTED(spfe_cull_map_points(h, &life.l, rows, c.kp_stride, kf_flags, c.n_slots, &cu, out), "cull_map_points slots %d stride %d table %d recent %d bad_cap %d", c.n_slots, c.kp_stride, c.n_table, c.recent_cap, c.bad_cap);
      free(out);
    }
  }
}

static void forms_local_ba_resident(spfe_handle h) {
  struct Case { int n_slots, kp_stride, n_table, conn_cap, kf_cap, free_cap, point_cap, edge_cap, bad_cap; };
  const Case mid = {40, 37, 500, 16, 20, 10, 300, 2000, 50};
  const Case cases[] = {{1, 1, 1, 1, 1, 1, 1, 1, 0},
                        mid,
                        {SPFE_LOCALMAP_MAX_KEYFRAMES, 3, 1000, SPFE_COVIS_MAX_CONN, SPFE_BA_MAX_KEYFRAMES, SPFE_BA_MAX_FREE, SPFE_BA_MAX_POINTS, SPFE_BA_MAX_EDGES, SPFE_BA_MAX_POINTS},
                        {6, SPFE_LOCALMAP_MAX_STRIDE, SPFE_MP_MAX_POINTS, 16, 20, 10, 300, 2000, 50},
                        {SPFE_LOCALMAP_MAX_KEYFRAMES + 1, 37, 500, 16, 20, 10, 300, 2000, 50},
                        {40, SPFE_LOCALMAP_MAX_STRIDE + 1, 500, 16, 20, 10, 300, 2000, 50},
                        {40, 37, SPFE_MP_MAX_POINTS + 1, 16, 20, 10, 300, 2000, 50},
                        {40, 37, 500, SPFE_COVIS_MAX_CONN + 1, 20, 10, 300, 2000, 50},
                        {40, 37, 500, 16, SPFE_BA_MAX_KEYFRAMES + 1, 10, 300, 2000, 50},
                        {40, 37, 500, 16, 20, SPFE_BA_MAX_FREE + 1, 300, 2000, 50},
                        {40, 37, 500, 16, 20, 10, SPFE_BA_MAX_POINTS + 1, 2000, 50},
                        {40, 37, 500, 16, 20, 10, 300, SPFE_BA_MAX_EDGES + 1, 50},
                        {40, 37, 500, 16, 20, 10, 300, 2000, SPFE_BA_MAX_POINTS + 1},
                        {0, 37, 500, 16, 20, 10, 300, 2000, 50},
                        {40, 37, 0, 16, 20, 10, 300, 2000, 50}};
  for (const Case &c : cases) {
    const bool bad_arrays = c.n_slots < 1 || c.n_slots > SPFE_LOCALMAP_MAX_KEYFRAMES || c.kp_stride > SPFE_LOCALMAP_MAX_STRIDE || c.n_table < 1 || c.n_table > SPFE_MP_MAX_POINTS;
    const bool bad_caps = c.kf_cap > SPFE_BA_MAX_KEYFRAMES || c.point_cap > SPFE_BA_MAX_POINTS || c.edge_cap > SPFE_BA_MAX_EDGES;
    const bool bad_gather = bad_arrays || bad_caps || c.conn_cap > SPFE_COVIS_MAX_CONN || c.free_cap > SPFE_BA_MAX_FREE;
    const bool bad_apply = bad_arrays || bad_caps || c.bad_cap > SPFE_BA_MAX_POINTS;
    // a refused call reads nothing: its arrays are those of the middle case
    const Case &a = bad_gather || bad_apply ? mid : c;
    Exact<int32_t> rows((size_t)a.n_slots * a.kp_stride, 0xff), nobs(a.n_table), ref_slot(a.n_table, 0xff);
    Exact<uint8_t> kf_flags(a.n_slots), mp_flags(a.n_table, 1);
    Exact<float> xyz((size_t)a.n_table * 3), Tcw((size_t)a.n_slots * 16);
    const size_t g_bytes = SPFE_LBA_GATHER_BYTES(a.kf_cap, a.point_cap, a.edge_cap);
    uint8_t *gather = static_cast<uint8_t *>(aligned_block(g_bytes));
    {
      Exact<int32_t> ord_row(a.conn_cap, 0xff);
      spfe_lba_gather_params gp{};
      gp.cur_slot = 0; gp.origin_slot = -1; gp.kf_cap = c.kf_cap; gp.free_cap = c.free_cap; gp.point_cap = c.point_cap; gp.edge_cap = c.edge_cap;
      if (bad_gather) REFUSED(spfe_gather_local_ba(h, ord_row, c.conn_cap, rows, c.kp_stride, kf_flags, c.n_slots, mp_flags, xyz, c.n_table, Tcw, &gp, gather), "gather_local_ba slots %d stride %d table %d conn_cap %d caps %d %d %d %d", c.n_slots, c.kp_stride, c.n_table, c.conn_cap, c.kf_cap, c.free_cap, c.point_cap, c.edge_cap);
      else ACCEPTED(spfe_gather_local_ba(h, ord_row, c.conn_cap, rows, c.kp_stride, kf_flags, c.n_slots, mp_flags, xyz, c.n_table, Tcw, &gp, gather), "gather_local_ba slots %d stride %d table %d conn_cap %d caps %d %d %d %d", c.n_slots, c.kp_stride, c.n_table, c.conn_cap, c.kf_cap, c.free_cap, c.point_cap, c.edge_cap);
    }
    if (bad_gather && !bad_apply) { free(gather); continue; }   // (a list or a free count too large for the gather alone: the application takes neither)
    // the gather's header as a full problem: the solver's block is as long as it says
    memset(gather, 0, g_bytes);
    int32_t hdr[16] = {};
    hdr[SPFE_LBA_OFF_N_KF / 4] = a.kf_cap; hdr[SPFE_LBA_OFF_N_POINTS / 4] = a.point_cap; hdr[SPFE_LBA_OFF_N_EDGES / 4] = a.edge_cap;
    memcpy(gather, hdr, sizeof hdr);
    Exact<uint8_t> ba_out(SPFE_BA_OUT_BYTES(a.kf_cap, a.point_cap, a.edge_cap));
    spfe_lba_apply_params ap{};
    ap.kf_cap = c.kf_cap; ap.point_cap = c.point_cap; ap.edge_cap = c.edge_cap; ap.bad_cap = c.bad_cap;
    void *out = aligned_block(SPFE_LBA_APPLY_BYTES(a.point_cap, a.edge_cap, a.bad_cap));
    if (bad_apply) REFUSED(spfe_apply_local_ba(h, gather, ba_out, rows, c.kp_stride, kf_flags, c.n_slots, mp_flags, nobs, ref_slot, xyz, c.n_table, Tcw, &ap, out), "apply_local_ba slots %d stride %d table %d caps %d %d %d bad_cap %d", c.n_slots, c.kp_stride, c.n_table, c.kf_cap, c.point_cap, c.edge_cap, c.bad_cap);
    else ACCEPTED(spfe_apply_local_ba(h, gather, ba_out, rows, c.kp_stride, kf_flags, c.n_slots, mp_flags, nobs, ref_slot, xyz, c.n_table, Tcw, &ap, out), "apply_local_ba slots %d stride %d table %d caps %d %d %d bad_cap %d", c.n_slots, c.kp_stride, c.n_table, c.kf_cap, c.point_cap, c.edge_cap, c.bad_cap);
    free(out);
    free(gather);
  }
  {   // a gather header the device would refuse (more keyframes than kf_cap): the solver's block is then its 256-byte header alone
    const Case &a = mid;
    Exact<int32_t> rows((size_t)a.n_slots * a.kp_stride, 0xff), nobs(a.n_table), ref_slot(a.n_table, 0xff);
    Exact<uint8_t> kf_flags(a.n_slots), mp_flags(a.n_table, 1), ba_out(256);
    Exact<float> xyz((size_t)a.n_table * 3), Tcw((size_t)a.n_slots * 16);
    uint8_t *gather = static_cast<uint8_t *>(aligned_block(SPFE_LBA_GATHER_BYTES(a.kf_cap, a.point_cap, a.edge_cap)));
    int32_t hdr[16] = {};
    hdr[SPFE_LBA_OFF_N_KF / 4] = a.kf_cap + 1; hdr[SPFE_LBA_OFF_N_POINTS / 4] = a.point_cap; hdr[SPFE_LBA_OFF_N_EDGES / 4] = a.edge_cap;
    memcpy(gather, hdr, sizeof hdr);
    spfe_lba_apply_params ap{};
    ap.kf_cap = a.kf_cap; ap.point_cap = a.point_cap; ap.edge_cap = a.edge_cap; ap.bad_cap = a.bad_cap;
    void *out = aligned_block(SPFE_LBA_APPLY_BYTES(a.point_cap, a.edge_cap, a.bad_cap));
    ACCEPTED(spfe_apply_local_ba(h, gather, ba_out, rows, a.kp_stride, kf_flags, a.n_slots, mp_flags, nobs, ref_slot, xyz, a.n_table, Tcw, &ap, out), "apply_local_ba: a gather header the device refuses");
    free(out);
    free(gather);
  }
}

static void scenario_host_forms() {
  const int H = 64, W = 96;
  spfe_handle h = make(H, W, SPFE_PRECISION_F32, 0, 1);
  if (!h) return;
  // two forms of different staging needs, one behind the other on one handle, before the buffer has grown to its largest
  small_host_forms(h, H, W, "host_forms interleaved, first round");
  forms_match(h);
  small_host_forms(h, H, W, "host_forms interleaved, second round");
  forms_patches(h, H, W);
  forms_dust_pose(h, H, W);
  forms_point_searches(h, H, W);
  forms_loop_pair(h, H, W);
  small_host_forms(h, H, W, "host_forms interleaved, third round");
  forms_ba(h, H, W);
  forms_map_graph(h);
  small_host_forms(h, H, W, "host_forms interleaved, fourth round");
  forms_resident_state(h);
  forms_map_point_culling(h);
  forms_local_ba_resident(h);
  small_host_forms(h, H, W, "host_forms interleaved, last round");
  spfe_destroy(h);
  expect_clean("host_forms");
}

// ---- device_forms ------------------------------------------------------------------------------------------------------
// Every *_device and *_resident form on stub device buffers and a stream of the caller's: a valid call makes the number of
// launches its header states (the table of tests/graph_forms.py) and neither copies nor memsets on the caller's stream; an
// invalid call launches nothing.  (Kernels do not run here: what is held is the host side of the contract.)
struct Dev {
  void *p = nullptr;
  explicit Dev(size_t bytes) { CHECK(hipMalloc(&p, bytes ? bytes : 1) == hipSuccess, "hipMalloc(%zu)", bytes); }
  Dev(const Dev &) = delete;
  ~Dev() { (void)hipFree(p); }
  operator void *() const { return p; }
};

static hipStream_t g_caller = nullptr;
#define DEVFORM(name, expected, valid, invalid)                                                                              \
  do {                                                                                                                       \
    const long l0_ = stub_launch_count(), t0_ = stub_transfers_on(g_caller);                                                 \
    const int rc_ = (valid);                                                                                                 \
    CHECK(rc_ == SPFE_OK, "%s: valid call -> %d (%s)", name, rc_, spfe_last_error());                                        \
    CHECK(stub_launch_count() - l0_ == (expected), "%s: %ld launches, the header states %d", name, stub_launch_count() - l0_, (int)(expected)); \
    CHECK(stub_transfers_on(g_caller) == t0_, "%s: %ld copies or memsets on the caller's stream", name, stub_transfers_on(g_caller) - t0_); \
    const std::vector<StubLaunch> log_ = stub_launches();                                                                     \
    for (size_t i_ = (size_t)l0_; i_ < log_.size(); ++i_)                                                                    \
      CHECK(log_[i_].stream == (void *)g_caller, "%s: kernel %s launched on another stream", name, log_[i_].kernel.c_str()); \
    const long l1_ = stub_launch_count(), x1_ = stub_transfers_total();                                                      \
    const int rci_ = (invalid);                                                                                              \
    CHECK(rci_ == SPFE_EINVAL || rci_ == SPFE_EEMPTY, "%s: invalid call -> %d", name, rci_);                                  \
    CHECK(stub_launch_count() == l1_ && stub_transfers_total() == x1_, "%s: the invalid call launched or copied", name);     \
  } while (0)

static void device_forms_body() {
  const int H = 64, W = 96, B = 3, nf = 100, kmax = nf + 1, PM = SPFE_PROJ_MAX_POINTS;
  spfe_handle h = make(H, W, SPFE_PRECISION_F32, 0, B, nf);
  if (!h) return;
  CHECK(hipStreamCreateWithFlags(&g_caller, hipStreamNonBlocking) == hipSuccess, "caller stream");
  void *S = g_caller;
  const size_t rb = spfe_record_bytes(h), C = (size_t)(H / 8) * (W / 8);
  Dev rec(B * rb), rec2(B * rb), imgs((size_t)B * H * W);
  {   // records from the extraction itself on the caller's stream
    const long t0 = stub_transfers_on(g_caller);
    CHECK(spfe_extract_batch_device(h, imgs, B, rec, S) == SPFE_OK, "extract_batch_device: %s", spfe_last_error());
    CHECK(spfe_extract_batch_device(h, imgs, B, rec2, S) == SPFE_OK, "extract_batch_device: %s", spfe_last_error());
    CHECK(spfe_wait_records(h, spfe_last_ticket(h), S) == SPFE_OK, "wait_records");
    CHECK(spfe_wait_records(h, spfe_last_ticket(h) + 1, S) == SPFE_EINVAL, "wait_records on a ticket not yet given");
    CHECK(spfe_extract_batch_device(h, imgs, B + 1, rec, S) == SPFE_EINVAL, "extract_batch_device above max_batch");
    printf("device_forms: spfe_extract_batch_device issued %ld copies or memsets on the caller's stream\n", stub_transfers_on(g_caller) - t0);
  }
  const int n = 300;
  Dev xyz((size_t)PM * 12), normal((size_t)PM * 12), range((size_t)PM * 8), desc((size_t)PM * 1024), flags(PM), pid((size_t)PM * 4);
  Dev Tcw(64 * 128), T12(13 * 8), mp_of_kp((size_t)B * kmax * 4), mp_of_kp2((size_t)SPFE_TRI_MAX_NEIGHBOURS * kmax * 4), kp_idx((size_t)PM * 4);
  spfe_dust_params dp{};
  dp.fx = dp.fy = 100; dp.cx = W / 2.0f; dp.cy = H / 2.0f; dp.max_iterations = 40; dp.huber_delta = 0.9; dp.inlier_chi2 = 0.9;
  spfe_pose_params pp{};
  pp.fx = pp.fy = 100; pp.cx = W / 2.0f; pp.cy = H / 2.0f; pp.schedule = SPFE_POSE_OPTIMIZATION; pp.iterations = 10;
  spfe_pose_params pd = pp;
  pd.schedule = SPFE_POSE_DUST_POST;
  spfe_proj_params pj{};
  pj.fx = pj.fy = 100; pj.cx = W / 2.0f; pj.cy = H / 2.0f; pj.mode = SPFE_PROJ_LOCAL_MAP; pj.th = 1; pj.th_dist = 0.7f; pj.view_cos_limit = 0.5f; pj.adaptive = 1; pj.c2_thresh = 81;
  spfe_proj_params pl = pj;
  pl.mode = SPFE_PROJ_LAST_FRAME; pl.th = 15;
  // staging, matching, patches
  {
    spfe_staging st{};
    st.src_height = H + 8; st.src_width = W + 8; st.channels = 3;
    CHECK(spfe_set_staging(h, &st) == SPFE_OK, "set_staging");
    Dev src((size_t)B * (H + 8) * (W + 8) * 3), gray((size_t)B * H * W);
    DEVFORM("stage_batch_device", 1, spfe_stage_batch_device(h, src, B, gray, S), spfe_stage_batch_device(h, src, B + 1, gray, S));
    Dev mout(2 * spfe_match_out_bytes(h));
    DEVFORM("match_records_device", 5, spfe_match_records_device(h, rec, rec2, 2, 1, mout, S), spfe_match_records_device(h, rec, nullptr, 2, 1, mout, S));
    DEVFORM("match_patches_record_device", 2, spfe_match_patches_record_device(h, desc, range, n, rec, 0.75f, kp_idx, S),
            spfe_match_patches_record_device(h, desc, range, 4097, rec, 0.75f, kp_idx, S));
  }
  // dust and pose
  Dev dust_out((size_t)B * SPFE_DUST_OUT_BYTES), pose_out((size_t)B * spfe_pose_out_bytes(h)), proj_out((size_t)B * SPFE_PROJ_OUT_BYTES), npts(B * 4);
  Dev dpts((size_t)B * SPFE_DUST_MAX_POINTS * 12);
  DEVFORM("align_dust_record_device", 1, spfe_align_dust_record_device(h, rec, dpts, 200, Tcw, &dp, dust_out, S),
          spfe_align_dust_record_device(h, rec, dpts, SPFE_DUST_MAX_POINTS + 1, Tcw, &dp, dust_out, S));
  DEVFORM("align_dust_batch_device", 1, spfe_align_dust_batch_device(h, rec, B, dpts, npts, Tcw, &dp, dust_out, S),
          spfe_align_dust_batch_device(h, rec, 0, dpts, npts, Tcw, &dp, dust_out, S));
  DEVFORM("refine_pose_record_device", 1, spfe_refine_pose_record_device(h, rec, mp_of_kp, xyz, Tcw, &pp, pose_out, S),
          spfe_refine_pose_record_device(h, rec, nullptr, xyz, Tcw, &pp, pose_out, S));
  DEVFORM("refine_pose_batch_device", 1, spfe_refine_pose_batch_device(h, rec, B, mp_of_kp, xyz, 1000, Tcw, &pp, pose_out, S),
          spfe_refine_pose_batch_device(h, rec, 0, mp_of_kp, xyz, 1000, Tcw, &pp, pose_out, S));
  DEVFORM("track_dust_record_device", 3, spfe_track_dust_record_device(h, rec, dpts, desc, 200, Tcw, &dp, 10, 0.75f, dust_out, kp_idx, S),
          spfe_track_dust_record_device(h, rec, dpts, desc, SPFE_DUST_MAX_POINTS + 1, Tcw, &dp, 10, 0.75f, dust_out, kp_idx, S));
  DEVFORM("track_dust_refine_record_device", 6, spfe_track_dust_refine_record_device(h, rec, dpts, desc, 200, Tcw, &dp, &pd, 10, 10, 0.5f, 0.75f, dust_out, kp_idx, pose_out, S),
          spfe_track_dust_refine_record_device(h, rec, dpts, desc, 200, Tcw, &dp, nullptr, 10, 10, 0.5f, 0.75f, dust_out, kp_idx, pose_out, S));
  // projection search and the tracking chains
  DEVFORM("search_projection_record_device", 3, spfe_search_projection_record_device(h, rec, xyz, normal, desc, flags, n, mp_of_kp, Tcw, &pj, proj_out, S),
          spfe_search_projection_record_device(h, rec, xyz, normal, desc, flags, PM + 1, mp_of_kp, Tcw, &pj, proj_out, S));
  DEVFORM("search_projection_batch_device", 3, spfe_search_projection_batch_device(h, rec, B, xyz, normal, desc, flags, npts, 1000, mp_of_kp, Tcw, &pj, proj_out, S),
          spfe_search_projection_batch_device(h, rec, B, xyz, normal, desc, flags, npts, PM + 1, mp_of_kp, Tcw, &pj, proj_out, S));
  DEVFORM("track_local_map_record_device", 5, spfe_track_local_map_record_device(h, rec, xyz, normal, desc, flags, n, mp_of_kp, Tcw, &pj, &pp, 30, proj_out, pose_out, S),
          spfe_track_local_map_record_device(h, rec, xyz, normal, desc, flags, PM + 1, mp_of_kp, Tcw, &pj, &pp, 30, proj_out, pose_out, S));
  DEVFORM("track_motion_model_record_device", 7, spfe_track_motion_model_record_device(h, rec, xyz, desc, flags, n, mp_of_kp, Tcw, &pl, &pp, 20, 10, proj_out, pose_out, S),
          spfe_track_motion_model_record_device(h, rec, xyz, desc, flags, n, mp_of_kp, Tcw, &pj, &pp, 20, 10, proj_out, pose_out, S));
  DEVFORM("track_reference_kf_record_device", 8, spfe_track_reference_kf_record_device(h, rec, rec2, mp_of_kp2, xyz, flags, n, mp_of_kp, Tcw, &pp, 10, pose_out, S),
          spfe_track_reference_kf_record_device(h, rec, nullptr, mp_of_kp2, xyz, flags, n, mp_of_kp, Tcw, &pp, 10, pose_out, S));
  // map-point creation and fusion
  spfe_tri_params tp{};
  tp.fx1 = tp.fy1 = tp.fx2 = tp.fy2 = 100; tp.cx1 = tp.cx2 = W / 2.0f; tp.cy1 = tp.cy2 = H / 2.0f; tp.ratio = 0.7f; tp.epipole_r2 = 100; tp.chi2_line = 3.84; tp.chi2_reproj = 5.991;
  tp.cos_parallax_max = 0.9998; tp.min_baseline_depth_ratio = 0.01;
  const void *recs2[SPFE_FUSE_MAX_TARGETS + 1];
  for (auto &r : recs2) r = (void *)rec2;
  {
    Dev tri_out(4 * SPFE_TRI_OUT_BYTES(kmax)), median(4 * 4);
    DEVFORM("create_map_points_pair_record_device", 7, spfe_create_map_points_pair_record_device(h, rec, rec2, mp_of_kp, mp_of_kp2, Tcw, Tcw, &tp, 0, tri_out, S),
            spfe_create_map_points_pair_record_device(h, rec, rec2, mp_of_kp, mp_of_kp2, Tcw, Tcw, &tp, -1, tri_out, S));
    DEVFORM("create_map_points_record_device", 14, spfe_create_map_points_record_device(h, rec, recs2, 2, mp_of_kp, mp_of_kp2, Tcw, Tcw, median, &tp, 0, tri_out, S),
            spfe_create_map_points_record_device(h, rec, recs2, SPFE_TRI_MAX_NEIGHBOURS + 1, mp_of_kp, mp_of_kp2, Tcw, Tcw, median, &tp, 0, tri_out, S));
  }
  spfe_fuse_params fu{};
  fu.fx = fu.fy = 100; fu.cx = W / 2.0f; fu.cy = H / 2.0f; fu.th = 3; fu.th_dist = 0.3f; fu.chi2 = 5.99; fu.view_cos = 0.5; fu.min_factor = 0.8f; fu.max_factor = 1.2f;
  spfe_loop_fuse_params lf{};
  lf.fx = lf.fy = 100; lf.cx = W / 2.0f; lf.cy = H / 2.0f; lf.th = 4; lf.th_dist = 0.7f; lf.view_cos = 0.5; lf.min_factor = 0.8f; lf.max_factor = 1.2f;
  {
    const int cap = 512;
    Dev fout(2 * SPFE_FUSE_OUT_BYTES(cap));
    DEVFORM("fuse_record_device", 2, spfe_fuse_record_device(h, rec, mp_of_kp, Tcw, pid, xyz, normal, range, desc, flags, n, cap, &fu, fout, S),
            spfe_fuse_record_device(h, rec, mp_of_kp, Tcw, pid, xyz, normal, range, desc, flags, cap + 1, cap, &fu, fout, S));
    DEVFORM("fuse_targets_record_device", 2, spfe_fuse_targets_record_device(h, recs2, 2, mp_of_kp, Tcw, pid, xyz, normal, range, desc, flags, n, cap, &fu, fout, S),
            spfe_fuse_targets_record_device(h, recs2, SPFE_FUSE_MAX_TARGETS + 1, mp_of_kp, Tcw, pid, xyz, normal, range, desc, flags, n, cap, &fu, fout, S));
    DEVFORM("loop_fuse_record_device", 2, spfe_loop_fuse_record_device(h, rec, mp_of_kp, Tcw, pid, xyz, normal, range, desc, flags, n, cap, &lf, fout, S),
            spfe_loop_fuse_record_device(h, rec, mp_of_kp, Tcw, pid, xyz, normal, range, desc, flags, n, PM + 1, &lf, fout, S));
    DEVFORM("loop_fuse_targets_record_device", 2, spfe_loop_fuse_targets_record_device(h, recs2, 2, mp_of_kp, Tcw, pid, xyz, normal, range, desc, flags, n, cap, &lf, fout, S),
            spfe_loop_fuse_targets_record_device(h, recs2, 0, mp_of_kp, Tcw, pid, xyz, normal, range, desc, flags, n, cap, &lf, fout, S));
    spfe_loop_proj_params lp{};
    lp.fx = lp.fy = 100; lp.cx = W / 2.0f; lp.cy = H / 2.0f; lp.th = 10; lp.th_dist = 0.7f; lp.view_cos = 0.5; lp.min_factor = 0.8f; lp.max_factor = 1.2f;
    Dev lout(SPFE_LOOPPROJ_OUT_BYTES(cap));
    DEVFORM("search_loop_points_record_device", 2, spfe_search_loop_points_record_device(h, rec, Tcw, mp_of_kp, pid, xyz, normal, range, desc, flags, n, cap, &lp, lout, S),
            spfe_search_loop_points_record_device(h, rec, Tcw, mp_of_kp, pid, xyz, normal, range, desc, flags, cap + 1, cap, &lp, lout, S));
  }
  // loop verification, guided match and Sim3
  {
    const int n_hyp = 40, n_cand = 2, n_jobs = 3;
    spfe_sim3_params sp{};
    sp.fx1 = sp.fy1 = sp.fx2 = sp.fy2 = 100; sp.cx1 = sp.cx2 = W / 2.0f; sp.cy1 = sp.cy2 = H / 2.0f; sp.max_err1 = sp.max_err2 = 9; sp.min_inliers = 20;
    spfe_guided_params gp{};
    gp.fx1 = gp.fy1 = gp.fx2 = gp.fy2 = 100; gp.cx1 = gp.cx2 = W / 2.0f; gp.cy1 = gp.cy2 = H / 2.0f; gp.th = 7.5f; gp.th_dist = 0.7f; gp.min_factor = 0.8f; gp.max_factor = 1.2f;
    spfe_sim3opt_params op{};
    op.fx1 = op.fy1 = op.fx2 = op.fy2 = 100; op.cx1 = op.cx2 = W / 2.0f; op.cy1 = op.cy2 = H / 2.0f; op.th2 = 10; op.iterations = 5; op.min_kept = 10; op.min_inliers = 20;
    Dev match12((size_t)n_cand * kmax * 4), n_matches(n_cand * 4), rnd((size_t)n_cand * n_hyp * 12), vout(n_cand * SPFE_SIM3_OUT_BYTES(kmax, n_hyp));
    Dev gout(n_jobs * SPFE_GUIDED_OUT_BYTES(kmax)), oout(n_jobs * SPFE_SIM3OPT_OUT_BYTES(kmax));
    const int32_t jobs[2 * 3] = {0, 0, 1, 0, 1, 5}, bad_jobs[2 * 3] = {0, 0, 2, 0, 1, 5};
    DEVFORM("loop_match_record_device", 6, spfe_loop_match_record_device(h, rec, rec2, mp_of_kp, mp_of_kp2, match12, n_matches, S),
            spfe_loop_match_record_device(h, rec, rec2, mp_of_kp, mp_of_kp2, nullptr, n_matches, S));
    DEVFORM("sim3_ransac_device", 3, spfe_sim3_ransac_device(h, kmax, match12, mp_of_kp, mp_of_kp2, xyz, flags, n, Tcw, Tcw, rnd, n_hyp, &sp, vout, S),
            spfe_sim3_ransac_device(h, kmax, match12, mp_of_kp, mp_of_kp2, xyz, flags, n, Tcw, Tcw, rnd, SPFE_SIM3_MAX_HYPOTHESES + 1, &sp, vout, S));
    DEVFORM("loop_verify_records_device", 15, spfe_loop_verify_records_device(h, rec, recs2, n_cand, mp_of_kp, mp_of_kp2, xyz, flags, n, Tcw, Tcw, rnd, n_hyp, &sp, match12, n_matches, vout, S),
            spfe_loop_verify_records_device(h, rec, recs2, SPFE_SIM3_MAX_CANDIDATES + 1, mp_of_kp, mp_of_kp2, xyz, flags, n, Tcw, Tcw, rnd, n_hyp, &sp, match12, n_matches, vout, S));
    DEVFORM("search_by_sim3_record_device", 3, spfe_search_by_sim3_record_device(h, rec, rec2, mp_of_kp, mp_of_kp2, xyz, flags, range, desc, n, Tcw, Tcw, T12, match12, &gp, gout, S),
            spfe_search_by_sim3_record_device(h, rec, rec2, mp_of_kp, mp_of_kp2, xyz, flags, range, desc, PM + 1, Tcw, Tcw, T12, match12, &gp, gout, S));
    DEVFORM("loop_guided_match_records_device", 3, spfe_loop_guided_match_records_device(h, rec, recs2, n_cand, jobs, n_jobs, mp_of_kp, mp_of_kp2, xyz, flags, range, desc, n, Tcw, Tcw, match12, vout, n_hyp, &gp, gout, S),
            spfe_loop_guided_match_records_device(h, rec, recs2, n_cand, bad_jobs, n_jobs, mp_of_kp, mp_of_kp2, xyz, flags, range, desc, n, Tcw, Tcw, match12, vout, n_hyp, &gp, gout, S));
    DEVFORM("optimize_sim3_record_device", 1, spfe_optimize_sim3_record_device(h, rec, rec2, mp_of_kp, mp_of_kp2, xyz, flags, n, Tcw, Tcw, T12, match12, &op, oout, S),
            spfe_optimize_sim3_record_device(h, rec, rec2, mp_of_kp, mp_of_kp2, xyz, flags, -1, Tcw, Tcw, T12, match12, &op, oout, S));
    DEVFORM("loop_optimize_sim3_records_device", 1, spfe_loop_optimize_sim3_records_device(h, rec, recs2, n_cand, jobs, n_jobs, mp_of_kp, mp_of_kp2, xyz, flags, n, Tcw, Tcw, vout, n_hyp, gout, &op, oout, S),
            spfe_loop_optimize_sim3_records_device(h, rec, recs2, n_cand, jobs, SPFE_GUIDED_MAX_JOBS + 1, mp_of_kp, mp_of_kp2, xyz, flags, n, Tcw, Tcw, vout, n_hyp, gout, &op, oout, S));
    Dev Siw(20 * 64), Tic(20 * 64);
    DEVFORM("loop_corrected_poses_device", 1, spfe_loop_corrected_poses_device(h, oout, Tcw, Tcw, Tcw, 20, 3, Siw, Tic, S),
            spfe_loop_corrected_poses_device(h, oout, Tcw, Tcw, Tcw, SPFE_FUSE_MAX_TARGETS + 1, 3, Siw, Tic, S));
    // the essential graph behind it
    const int ng = 70, E = 90;
    Dev est((size_t)ng * 64), meas((size_t)ng * 64), gfl(ng), edges((size_t)E * 12), eg_out(SPFE_ESSGRAPH_OUT_BYTES(ng)), conn(ng * 4), code(n);
    spfe_essgraph_params ep{};
    ep.iterations = 20; ep.lambda_init = 1e-16;
    DEVFORM("essential_graph_sim3_device", 2, spfe_essential_graph_sim3_device(h, Tcw, oout, Tcw, Tcw, conn, 5, 3, est, meas, ng, S),
            spfe_essential_graph_sim3_device(h, Tcw, oout, Tcw, Tcw, conn, ng + 1, 3, est, meas, ng, S));
    DEVFORM("optimize_essential_graph_device", 4, spfe_optimize_essential_graph_device(h, est, meas, gfl, ng, edges, E, 400, &ep, eg_out, S),
            spfe_optimize_essential_graph_device(h, est, meas, gfl, 0, edges, E, 400, &ep, eg_out, S));
    DEVFORM("correct_map_points_device", 1, spfe_correct_map_points_device(h, est, meas, ng, mp_of_kp, nullptr, n, xyz, flags, PM, code, S),
            spfe_correct_map_points_device(h, est, meas, 0, mp_of_kp, nullptr, n, xyz, flags, PM, code, S));
  }
  // bundle adjustment and the map-point table
  {
    const int n_kf = 3, E = 500, m = 200;
    spfe_ba_params bp{};
    bp.fx = bp.fy = 100; bp.cx = W / 2.0f; bp.cy = H / 2.0f; bp.schedule = SPFE_BA_LOCAL; bp.iterations[0] = 5; bp.iterations[1] = 10; bp.robust = 1; bp.inv_sigma2 = 1;
    Dev edges((size_t)E * 12), fixed(n_kf), bout(SPFE_BA_OUT_BYTES(n_kf, n, E));
    DEVFORM("local_ba_records_device", 1, spfe_local_ba_records_device(h, recs2, n_kf, edges, E, Tcw, fixed, xyz, n, &bp, nullptr, bout, S),
            spfe_local_ba_records_device(h, recs2, SPFE_BA_MAX_KEYFRAMES + 1, edges, E, Tcw, fixed, xyz, n, &bp, nullptr, bout, S));
    spfe_mp_params mp{};
    mp.mode = SPFE_MP_DESC | SPFE_MP_NORMAL_DEPTH; mp.level_scale = mp.top_scale = 1;
    Dev kf_recs(8 * n_kf), kf_flags(n_kf), obs_start((m + 1) * 4), obs((size_t)E * 8), ref(m * 4), mout(SPFE_MP_OUT_BYTES(m));
    DEVFORM("refresh_map_points_device", 2, spfe_refresh_map_points_device(h, kf_recs, kf_flags, Tcw, n_kf, nullptr, obs_start, obs, ref, m, E, xyz, flags, normal, range, desc, PM, &mp, mout, S),
            spfe_refresh_map_points_device(h, kf_recs, kf_flags, Tcw, 0, nullptr, obs_start, obs, ref, m, E, xyz, flags, normal, range, desc, PM, &mp, mout, S));
    Dev lx((size_t)m * 12), ln((size_t)m * 12), lr((size_t)m * 8), ld((size_t)m * 1024), lfl(m), lid(m * 4);
    DEVFORM("gather_map_points_device", 1, spfe_gather_map_points_device(h, ref, m, xyz, flags, normal, range, desc, PM, lid, lx, ln, lr, ld, lfl, S),
            spfe_gather_map_points_device(h, ref, SPFE_MP_MAX_POINTS + 1, xyz, flags, normal, range, desc, PM, lid, lx, ln, lr, ld, lfl, S));
  }
  // loop detection and the resident state
  {
    const int ns = 40, st = 37, nt = 500, nk = 30, pc = 600, nb = 20, cc = 16, dim = 256;
    spfe_loopdet_params lp{};
    lp.min_score_init = 0.2f; lp.min_score_floor = 0.2f; lp.retain_ratio = 0.75f;
    Dev gdesc((size_t)ns * dim * 4), kf_flags(ns), in_db(ns), best10((size_t)ns * 40), conn(ns * 4), cov(ns * 4), ld_out(SPFE_LOOPDET_OUT_BYTES(ns));
    DEVFORM("detect_loop_candidates_device", 3, spfe_detect_loop_candidates_device(h, gdesc, dim, kf_flags, in_db, best10, ns, ns - 1, conn, 5, cov, 5, &lp, ld_out, S),
            spfe_detect_loop_candidates_device(h, gdesc, dim + 2, kf_flags, in_db, best10, ns, ns - 1, conn, 5, cov, 5, &lp, ld_out, S));
    spfe_localmap_params lm{};
    lm.max_keyframes = 80; lm.point_cap = pc;
    Dev rows((size_t)ns * st * 4), best((size_t)ns * nb * 4), parent(ns * 4), mp_flags(nt), frame(nk * 4), outlier(nk), votes(ns * 4), total(ns * 4), nobs(nt * 4);
    Dev lm_out(SPFE_LOCALMAP_OUT_BYTES(ns, pc, nk)), rows_out(nk * 4);
    DEVFORM("update_local_map_resident", 7, spfe_update_local_map_resident(h, rows, st, kf_flags, best, nb, parent, ns, mp_flags, nt, frame, nk, &lm, lm_out, S),
            spfe_update_local_map_resident(h, rows, st, kf_flags, best, SPFE_LOCALMAP_MAX_BEST + 1, parent, ns, mp_flags, nt, frame, nk, &lm, lm_out, S));
    DEVFORM("count_shared_points_resident", 3, spfe_count_shared_points_resident(h, rows, st, ns, mp_flags, nt, frame, outlier, nk, votes, total, S),
            spfe_count_shared_points_resident(h, rows, st, ns, mp_flags, nt, frame, outlier, PM + 1, votes, total, S));
    DEVFORM("local_map_rows_resident", 1, spfe_local_map_rows_resident(h, lm_out, pc, frame, nk, rows_out, S),
            spfe_local_map_rows_resident(h, lm_out, 0, frame, nk, rows_out, S));
    Dev cs((size_t)ns * cc * 4), cw((size_t)ns * cc * 4), cn(ns * 4), os((size_t)ns * cc * 4), ow((size_t)ns * cc * 4), on(ns * 4), first(ns);
    spfe_covis_graph g{};
    g.d_conn_slot = cs; g.d_conn_w = cw; g.d_conn_n = cn; g.d_ord_slot = os; g.d_ord_w = ow; g.d_ord_n = on; g.d_parent = parent; g.d_first_conn = first; g.n_slots = ns; g.conn_cap = cc;
    spfe_covis_graph gbad = g;
    gbad.conn_cap = SPFE_COVIS_MAX_CONN + 1;
    spfe_covis_params cv{};
    cv.th = 15; cv.origin_slot = 0;
    spfe_cull_params cu{};
    cu.th_obs = 3; cu.cov_ratio = 0.9f; cu.origin_slot = 0; cu.bad_cap = 100;
    Dev cv_out(SPFE_COVIS_OUT_BYTES(ns, cc)), cu_out(SPFE_CULL_OUT_BYTES(ns, cc, 100));
    DEVFORM("covis_reset_slots_resident", 1, spfe_covis_reset_slots_resident(h, &g, 0, ns, S), spfe_covis_reset_slots_resident(h, &g, 1, ns, S));
    DEVFORM("update_connections_resident", 5, spfe_update_connections_resident(h, &g, rows, st, kf_flags, mp_flags, nt, ns - 1, &cv, best, nb, best10, 10, cv_out, S),
            spfe_update_connections_resident(h, &gbad, rows, st, kf_flags, mp_flags, nt, ns - 1, &cv, best, nb, best10, 10, cv_out, S));
    DEVFORM("count_observations_resident", 2, spfe_count_observations_resident(h, rows, st, kf_flags, ns, nobs, nt, S),
            spfe_count_observations_resident(h, rows, 0, kf_flags, ns, nobs, nt, S));
    DEVFORM("cull_keyframes_resident", 4, spfe_cull_keyframes_resident(h, &g, rows, st, kf_flags, mp_flags, nobs, nt, ns - 1, &cu, best, nb, best10, 10, cu_out, S),
            spfe_cull_keyframes_resident(h, &g, rows, st, kf_flags, mp_flags, nobs, nt, ns, &cu, best, nb, best10, 10, cu_out, S));
    // map-point culling and the forms around the local BA
    const int rcap = 300, nn = 3;
    Dev found(nt * 4), visible(nt * 4), first_kf(nt * 4), recent(rcap * 4), recent_n(4), ref_slot(nt * 4), txyz((size_t)nt * 12), poses((size_t)ns * 64);
    spfe_mp_life life{};
    life.d_mp_flags = mp_flags; life.d_mp_nobs = nobs; life.d_mp_found = found; life.d_mp_visible = visible; life.d_mp_first_kf = first_kf;
    life.d_recent = recent; life.d_recent_n = recent_n; life.n_table = nt; life.recent_cap = rcap;
    DEVFORM("mp_life_reset_resident", 1, spfe_mp_life_reset_resident(h, &life, 0, nt, 1, S), spfe_mp_life_reset_resident(h, &life, 0, 0, 0, S));
    Dev tri((size_t)nn * spfe_tri_out_bytes(h)), neigh(nn * 4), ad_out(SPFE_ADMIT_OUT_BYTES);
    DEVFORM("admit_map_points_resident", 2, spfe_admit_map_points_resident(h, &life, tri, nn, neigh, ns - 1, 7, rows, st, ns, txyz, ad_out, S),
            spfe_admit_map_points_resident(h, &life, tri, SPFE_TRI_MAX_NEIGHBOURS + 1, neigh, ns - 1, 7, rows, st, ns, txyz, ad_out, S));
    Dev after(nk * 4), point_idx(pc * 4), st_out(SPFE_MPSTAT_OUT_BYTES);
    DEVFORM("track_statistics_resident", 1, spfe_track_statistics_resident(h, &life, frame, after, nk, point_idx, pc, proj_out, pose_out, st_out, S),
            spfe_track_statistics_resident(h, &life, frame, after, PM + 1, point_idx, pc, proj_out, pose_out, st_out, S));
    spfe_mpcull_params mc{};
    mc.cur_kf_id = 9; mc.th_obs = 2; mc.found_ratio = 0.25f; mc.bad_cap = 100;
    spfe_mpcull_params mc_bad = mc;
    mc_bad.bad_cap = SPFE_MP_MAX_POINTS + 1;
    Dev mc_out(SPFE_MPCULL_OUT_BYTES(rcap, 100));
    DEVFORM("cull_map_points_resident", 4, spfe_cull_map_points_resident(h, &life, rows, st, kf_flags, ns, &mc, mc_out, S),
            spfe_cull_map_points_resident(h, &life, rows, st, kf_flags, ns, &mc_bad, mc_out, S));
    spfe_lba_gather_params gp{};
    gp.cur_slot = ns - 1; gp.origin_slot = 0; gp.kf_cap = 20; gp.free_cap = 10; gp.point_cap = 300; gp.edge_cap = 2000;
    spfe_lba_gather_params gp_bad = gp;
    gp_bad.free_cap = SPFE_BA_MAX_FREE + 1;
    Dev lg_out(SPFE_LBA_GATHER_BYTES(20, 300, 2000)), lb_ba(SPFE_BA_OUT_BYTES(20, 300, 2000)), la_out(SPFE_LBA_APPLY_BYTES(300, 2000, 50));
    DEVFORM("gather_local_ba_resident", 10, spfe_gather_local_ba_resident(h, os, cc, rows, st, kf_flags, ns, mp_flags, txyz, nt, poses, &gp, lg_out, S),
            spfe_gather_local_ba_resident(h, os, cc, rows, st, kf_flags, ns, mp_flags, txyz, nt, poses, &gp_bad, lg_out, S));
    spfe_lba_apply_params ap{};
    ap.kf_cap = 20; ap.point_cap = 300; ap.edge_cap = 2000; ap.bad_cap = 50;
    spfe_lba_apply_params ap_bad = ap;
    ap_bad.bad_cap = SPFE_BA_MAX_POINTS + 1;
    DEVFORM("apply_local_ba_resident", 5, spfe_apply_local_ba_resident(h, lg_out, lb_ba, rows, st, kf_flags, ns, mp_flags, nobs, ref_slot, txyz, nt, poses, &ap, la_out, S),
            spfe_apply_local_ba_resident(h, lg_out, lb_ba, rows, st, kf_flags, ns, mp_flags, nobs, ref_slot, txyz, nt, poses, &ap_bad, la_out, S));
  }
  CHECK(spfe_tri_out_bytes(h) == SPFE_TRI_OUT_BYTES(kmax) && spfe_proj_out_bytes(h) == SPFE_PROJ_OUT_BYTES && spfe_essgraph_lds_panel_capacity(h) > 0 &&
        spfe_localmap_lds_point_capacity(h) > 0 && spfe_match_out_bytes(h) == (size_t)kmax * 8, "the size and capacity getters");
  spfe_destroy(h);
  CHECK(hipStreamDestroy(g_caller) == hipSuccess, "caller stream");
  g_caller = nullptr;
}

static void scenario_device_forms() {
  device_forms_body();   // (its device buffers are freed when it returns)
  expect_clean("device_forms");
}

// ---- the multi-GPU entry points without RCCL -------------------------------------------------------------------------------
static void comm_without_rccl() {
  spfe_handle h = make(64, 96, SPFE_PRECISION_F32, 0, 1);
  if (!h) return;
  uint8_t id[SPFE_COMM_ID_BYTES] = {};
  int count = -1;
  CHECK(spfe_comm_unique_id(id, sizeof(id)) == SPFE_EHIP && strstr(spfe_last_error(), "librccl"), "comm_unique_id without RCCL: %s", spfe_last_error());
  CHECK(spfe_comm_unique_id(id, 64) == SPFE_EINVAL, "comm_unique_id into 64 bytes");
  CHECK(spfe_comm_init(h, id, 0, 1) == SPFE_EHIP && strstr(spfe_last_error(), "librccl"), "comm_init without RCCL: %s", spfe_last_error());
  CHECK(spfe_comm_init(h, id, 1, 1) == SPFE_EINVAL, "comm_init rank 1 of 1");
  CHECK(spfe_comm_stream(h) == nullptr, "comm_stream before init");
  CHECK(spfe_comm_count(h, &count) != SPFE_OK, "comm_count before init");
  CHECK(spfe_allgather_records(h, 0, nullptr, nullptr, 1) != SPFE_OK, "allgather before init");
  CHECK(spfe_comm_wait(h, nullptr) == SPFE_OK, "comm_wait with no gather to wait for: %s", spfe_last_error());
  CHECK(spfe_comm_destroy(h) == SPFE_OK, "comm_destroy before init");
  spfe_destroy(h);
  expect_clean("comm without RCCL");
}

// ---- lifecycle ---------------------------------------------------------------------------------------------------------
static void scenario_lifecycle() {
  const unsigned all = SPFE_FLAG_HEAT | SPFE_FLAG_ASYNC_COV | SPFE_FLAG_LAZY_HEAT_INV | SPFE_FLAG_DESC_BF16;
  const unsigned flag_sets[] = {SPFE_FLAG_HEAT, SPFE_FLAG_ASYNC_COV, SPFE_FLAG_LAZY_HEAT_INV, SPFE_FLAG_DESC_BF16, all};
  const int sizes[][2] = {{16, 16}, {64, 96}, {480, 752}, {720, 1280}};
  const int batches[] = {1, 3, 8};
  int twins = 0, creates = 0;
  double seconds[4] = {};
  // The whole product of the issue's lists: five flag sets, two precisions, four sizes, three batch sizes.
  for (int precision : {SPFE_PRECISION_F32, SPFE_PRECISION_BF16})
    for (unsigned flags : flag_sets) {
      for (auto &hw : sizes)
        for (int B : batches) {
          ++creates;
          const auto t0 = std::chrono::steady_clock::now();
          char what[96];
          snprintf(what, sizeof(what), "lifecycle %dx%d p%d flags %u B%d", hw[1], hw[0], precision, flags, B);
          spfe_config c = config(hw[0], hw[1], precision, flags, B);
          spfe_handle h = nullptr;
          const int rc = spfe_create(&c, &h);
          CHECK(rc == SPFE_OK && h, "%s: create -> %d (%s)", what, rc, spfe_last_error());
          if (rc) continue;
          int two = 0;
          CHECK(spfe_debug_read(h, "two_chains", 0, &two, sizeof(two)) == (long)sizeof(int), "%s: two_chains", what);
          twins += two;
          spfe_record_layout rl{};
          CHECK(spfe_get_record_layout(h, &rl) == SPFE_OK && rl.bytes == spfe_record_bytes(h) && rl.kmax == c.num_features + 1, "%s: layout", what);
          CHECK(rl.desc_elem_bytes == ((flags & SPFE_FLAG_DESC_BF16) ? 2 : 4), "%s: desc_elem_bytes", what);
          spfe_destroy(h);
          expect_clean(what);
          seconds[&hw - sizes] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }
    }
  printf("lifecycle: seconds at the four sizes: %.2f %.2f %.2f %.2f\n", seconds[0], seconds[1], seconds[2], seconds[3]);
  CHECK(creates == 2 * 5 * 4 * 3, "lifecycle made %d creates, the product is 120", creates);
  printf("lifecycle: %d creates, %d with a twin\n", creates, twins);
  CHECK(twins > 0, "no configuration got the twin handle (1280x720 bf16 with SPFE_FLAG_ASYNC_COV should)");
  spfe_destroy(nullptr);
  spfe_handle h = nullptr;
  spfe_config bad = config(20, 16, SPFE_PRECISION_F32, 0, 1);
  CHECK(spfe_create(&bad, &h) == SPFE_EINVAL && !h, "height 20 accepted");
  {
    // The whole-call limit of spfe_config::max_batch: at most 65,535 frames and max_batch * cells * R < 2^31 (R = 2048 bytes
    // in f32, 1024 in bf16).  The largest accepted value plus one is refused with the limit in the message and before
    // anything is allocated; the two largest documented workloads are accepted.
    struct Edge { int H, W, precision, largest; };
    const Edge edges[] = {{16, 16, SPFE_PRECISION_F32, 65535},     {16, 16, SPFE_PRECISION_BF16, 65535},
                          {136, 200, SPFE_PRECISION_F32, 2467},    {136, 200, SPFE_PRECISION_BF16, 4934},
                          {2160, 3840, SPFE_PRECISION_F32, 8},     {2160, 3840, SPFE_PRECISION_BF16, 16}};
    for (const Edge &e : edges) {
      const size_t cells = (size_t)(e.H / 8) * (e.W / 8), R = e.precision == SPFE_PRECISION_BF16 ? 1024 : 2048;
      CHECK((size_t)e.largest == std::min<size_t>(65535, (((size_t)1 << 31) - 1) / (cells * R)), "edge table %dx%d", e.W, e.H);
      const long mallocs = stub_calls("hipMalloc"), pinned = stub_calls("hipHostMalloc"), streams = stub_calls("hipStreamCreateWithFlags");
      spfe_config c = config(e.H, e.W, e.precision, 0, e.largest + 1, 1);
      CHECK(spfe_create(&c, &h) == SPFE_EINVAL && !h, "max_batch %d at %dx%d p%d accepted", e.largest + 1, e.W, e.H, e.precision);
      char want[64];
      snprintf(want, sizeof(want), "precision is %d", e.largest);
      const std::string msg = spfe_last_error();
      CHECK(msg.find(want) != std::string::npos && msg.find("65535") != std::string::npos && msg.find("2^31") != std::string::npos,
            "max_batch %d at %dx%d p%d: message '%s' does not name the limits", e.largest + 1, e.W, e.H, e.precision, msg.c_str());
      CHECK(stub_calls("hipMalloc") == mallocs && stub_calls("hipHostMalloc") == pinned && stub_calls("hipStreamCreateWithFlags") == streams,
            "max_batch %d at %dx%d p%d was refused after allocations", e.largest + 1, e.W, e.H, e.precision);
      if (h) { spfe_destroy(h); h = nullptr; }
    }
    for (const Edge &e : {edges[4], edges[5], edges[0]}) {   // 3840x2160 x 8 (f32) and x 16 (bf16); 16x16 x 65,535
      spfe_config c = config(e.H, e.W, e.precision, 0, e.largest, 1);
      const int rc = spfe_create(&c, &h);
      CHECK(rc == SPFE_OK && h, "max_batch %d at %dx%d p%d -> %d (%s)", e.largest, e.W, e.H, e.precision, rc, spfe_last_error());
      spfe_destroy(h);
      h = nullptr;
      expect_clean("largest accepted max_batch");
    }
  }
  CHECK(spfe_check_abi(SPFE_ABI_VERSION, sizeof(spfe_config), sizeof(spfe_result), sizeof(spfe_record_layout)) == SPFE_OK, "abi");
  comm_without_rccl();
  expect_clean("lifecycle end");
}

int main(int argc, char **argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s <scenario> <weights.spfw>\n", argv[0]);
    return 2;
  }
  const std::string sc = argv[1];
  g_weights = argv[2];
  if (FILE *f = fopen(g_weights, "rb")) {   // 16-byte header {"SPFW", u32 version, u64 count}, then the floats
    g_blob.resize(SPFE_NUM_PARAMS);
    if (fseek(f, 16, SEEK_SET) != 0 || fread(g_blob.data(), 4, SPFE_NUM_PARAMS, f) != SPFE_NUM_PARAMS) g_blob.clear();
    fclose(f);
  }
  if (sc == "lifecycle") scenario_lifecycle();
  else if (sc == "host_calls") scenario_host_calls();
  else if (sc == "pipeline") scenario_pipeline();
  else if (sc == "alloc_failure") scenario_alloc_failure();
  else if (sc == "host_forms") scenario_host_forms();
  else if (sc == "device_forms") scenario_device_forms();
  else if (sc == "threads") scenario_threads();
  else if (sc == "stub_selfcheck") scenario_stub_selfcheck();
  else {
    fprintf(stderr, "unknown scenario %s\n", sc.c_str());
    return 2;
  }
  CHECK(stub_violations() == 0, "%ld stub violations", stub_violations());
  if (sc != "alloc_failure")   // (there a launch is made to fail behind its raised limit on purpose)
    CHECK(stub_raised_not_launched() == 0, "a launcher raised its kernel's LDS limit and the launch never reached the runtime");
  printf("%s: %s (%d failed checks, %ld launches logged)\n", sc.c_str(), g_failed.load() ? "FAILED" : "ok", g_failed.load(), stub_launch_count());
  return g_failed.load() ? 1 : 0;
}
