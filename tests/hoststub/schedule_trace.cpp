// schedule_trace.cpp — prints what the frame schedule (csrc/spfe_schedule.hip) issues, as text: for each configuration below a
// handle is created over the stub HIP runtime (hip_stub.cpp, HIP_STUB_TRACE + HIP_STUB_EMULATE_PROBE), three consecutive calls
// are made (the tile-queue counters' state, the last call's split and the ticket parity carry over from call to call) and the
// stub's log of each is printed: every launch with its template arguments, grid, block, LDS, stream and convolution geometry,
// every event record / wait / query and asynchronous copy.  tests/test_schedule_trace.py holds the output against
// tests/golden/schedule_trace.txt.gz.  Only include/spfe.h and hip_stub.h are used.  argv[1] = an "SPFW" weight file.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include "hip_stub.h"
#include "spfe.h"

extern char **environ;

enum Mode { SYNC, ASYNC_COV, PIPELINED, HOST_HEAT };
static const char *const kModeNames[] = {"sync", "async_cov", "pipelined", "host_heat"};
struct Config { int precision, H, W, n; Mode mode; const char *env; };   // env: "NAME=VALUE[ NAME=VALUE]" or null

static int g_failed = 0;

static void run(const Config &c, const char *weights) {
  std::vector<std::string> drop;
  for (char **e = environ; *e; ++e)
    if (!strncmp(*e, "SPFE_", 5)) drop.push_back(std::string(*e, strcspn(*e, "=")));
  for (const std::string &name : drop) unsetenv(name.c_str());
  for (std::string rest = c.env ? c.env : ""; !rest.empty();) {
    const std::string kv = rest.substr(0, rest.find(' '));
    rest.erase(0, kv.size() + 1);
    setenv(kv.substr(0, kv.find('=')).c_str(), kv.substr(kv.find('=') + 1).c_str(), 1);
  }
  printf("== %s %dx%d n=%d %s %s\n", c.precision == SPFE_PRECISION_BF16 ? "bf16" : "f32", c.H, c.W, c.n, kModeNames[c.mode], c.env ? c.env : "-");
  spfe_config cfg{};
  cfg.height = c.H; cfg.width = c.W; cfg.num_features = 100; cfg.max_batch = c.n; cfg.device = 0;
  cfg.precision = c.precision;
  cfg.flags = c.mode == ASYNC_COV ? SPFE_FLAG_ASYNC_COV : c.mode == HOST_HEAT ? SPFE_FLAG_HEAT : 0u;
  cfg.weights_path = weights;
  spfe_handle h = nullptr;
  if (spfe_create(&cfg, &h) != SPFE_OK || !h) {
    printf("create failed: %s\n", spfe_last_error());
    ++g_failed;
    return;
  }
  const size_t frame = (size_t)c.H * c.W;
  void *d_images = nullptr;
  std::vector<uint8_t> host(c.mode == PIPELINED || c.mode == HOST_HEAT ? frame * c.n : 0, 7);
  std::vector<const uint8_t *> frames;
  for (int i = 0; i < c.n && !host.empty(); ++i) frames.push_back(host.data() + i * frame);
  std::vector<spfe_result> out(c.n);
  if (hipMalloc(&d_images, frame * c.n) != hipSuccess) { ++g_failed; return; }
  (void)stub_trace_take(true);   // (what spfe_create issued is not the schedule's)
  long tickets[3] = {};
  for (int call = 0; call < 3; ++call) {
    int rc;
    if (c.mode == PIPELINED) rc = spfe_submit_batch(h, frames.data(), c.W, c.n, &tickets[call]);
    else if (c.mode == HOST_HEAT) rc = spfe_extract_batch(h, frames.data(), c.W, c.n, out.data());
    else rc = spfe_extract_batch_device(h, d_images, c.n, nullptr, nullptr);
    int rows = 0, cut = 0, split[2] = {};
    spfe_debug_read(h, "conv1b_tile_rows", 0, &rows, sizeof(rows));
    spfe_debug_read(h, "conv1b_split_rows", 0, &cut, sizeof(cut));
    spfe_debug_read(h, "split_streams", 0, split, sizeof(split));
    printf("-- call %d rc %d conv1b_tile_rows %d conv1b_split_rows %d split_streams %d %d\n", call, rc, rows, cut, split[0], split[1]);
    fputs(stub_trace_take(false).c_str(), stdout);
    if (rc != SPFE_OK) { printf("call failed: %s\n", spfe_last_error()); ++g_failed; }
  }
  if (c.mode == PIPELINED) {
    for (int call = 0; call < 3; ++call)
      if (spfe_collect_batch(h, tickets[call], out.data()) != SPFE_OK) { printf("collect failed: %s\n", spfe_last_error()); ++g_failed; }
    printf("-- collected\n");
    fputs(stub_trace_take(false).c_str(), stdout);
  }
  spfe_destroy(h);
  (void)hipFree(d_images);
  if (stub_violations()) { printf("stub violations: %ld\n", stub_violations()); ++g_failed; stub_reset_violations(); }
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: schedule_trace <weights.spfw>\n"); return 2; }
  setenv("HIP_STUB_TRACE", "1", 1);
  setenv("HIP_STUB_EMULATE_PROBE", "1", 1);
  const int F = SPFE_PRECISION_F32, B = SPFE_PRECISION_BF16;
  std::vector<Config> cs = {
      // f32: sizes and batches, synchronous device calls
      {F, 96, 64, 1, SYNC, nullptr}, {F, 480, 752, 1, SYNC, nullptr}, {F, 480, 752, 2, SYNC, nullptr}, {F, 480, 752, 3, SYNC, nullptr},
      {F, 480, 752, 8, SYNC, nullptr}, {F, 480, 640, 8, SYNC, nullptr}, {F, 720, 1280, 8, SYNC, nullptr}, {F, 2160, 3840, 1, SYNC, nullptr},
      {F, 480, 752, 8, ASYNC_COV, nullptr}, {F, 480, 752, 8, PIPELINED, nullptr},
      // (beyond the issue's list) the synchronous host call with heat maps, whose early copies the stage-event predicate gates,
      // and a pipelined single frame
      {F, 480, 752, 1, HOST_HEAT, nullptr}, {F, 480, 752, 1, HOST_HEAT, "SPFE_STAGE_TIMING=1"}, {F, 480, 752, 1, PIPELINED, nullptr},
      // bf16: sizes and batches
      {B, 96, 24, 1, SYNC, nullptr}, {B, 96, 64, 1, SYNC, nullptr}, {B, 480, 752, 1, SYNC, nullptr}, {B, 480, 752, 8, SYNC, nullptr},
      {B, 720, 1280, 8, SYNC, nullptr}, {B, 2160, 3840, 1, SYNC, nullptr}, {B, 720, 1280, 8, PIPELINED, nullptr},
      // (beyond the issue's list) bf16 half batches under the async flag: the per-half tails and tile-queue counters
      {B, 480, 752, 8, ASYNC_COV, nullptr}, {B, 480, 752, 8, PIPELINED, nullptr},
  };
  static const char *const f32_switches[] = {
      "SPFE_STAGE_TIMING=1", "SPFE_STAGE_TIMING=2", "SPFE_TILE16X4=0", "SPFE_TILE16X4=2", "SPFE_TILE16X4=3", "SPFE_TILE2_MASK=0",
      "SPFE_TILE2_MASK=0x7e", "SPFE_POOL_SPLIT=0", "SPFE_POOL_SPLIT=1", "SPFE_FUSE_CONV1A=0", "SPFE_FUSE_CONV1A=1", "SPFE_F32_HEADS=1",
      "SPFE_PBTAIL=0", "SPFE_SPARSE_DB=0", "SPFE_SPARSE_DB=1", "SPFE_SPARSE_DB=2", "SPFE_SPARSE_DA=0", "SPFE_SPARSE_DA=1",
      "SPFE_SPARSE_DA=2", "SPFE_SPLIT=0", "SPFE_SPLIT=1", "SPFE_TAIL_PER_HALF=0", "SPFE_DEFER_JOIN=0", "SPFE_INLINE_CHAIN=0",
      "SPFE_SEL_EXT_EVENT=0"};
  for (const char *e : f32_switches)
    for (int n : {8, 1}) cs.push_back({F, 480, 752, n, SYNC, e});
  // (beyond the issue's list) the switches that act on pipelined calls only, there
  for (const char *e : {"SPFE_TAIL_PER_HALF=0", "SPFE_DEFER_JOIN=0", "SPFE_SPARSE_DA=1", "SPFE_SPARSE_DB=2", "SPFE_PBTAIL=0"})
    cs.push_back({F, 480, 752, 8, ASYNC_COV, e});
  static const char *const bf16_switches[] = {"SPFE_BF16_WS=0", "SPFE_BF16_RW=0", "SPFE_BF16_DYN_QUEUE=0", "SPFE_BF16_TILE_ROWS=16,1",
                                              "SPFE_PBTAIL=2", "SPFE_ZERO_IN_TAIL=0", "SPFE_REPLAY_WAVES=8", "SPFE_FUSE_CONV1A=0"};
  for (const char *e : bf16_switches) {
    cs.push_back({B, 720, 1280, 8, SYNC, e});
    cs.push_back({B, 480, 752, 1, SYNC, e});
  }
  // (beyond the issue's list) bf16 without the register-resident weights and without the taller tiles; the streamed-weight
  // kernel on a small frame (static order: too few items for the queue); half batches without the per-half tail and with SPFE_PBTAIL=0
  for (const char *e : {"SPFE_BF16_RW=0", "SPFE_PBTAIL=0", "SPFE_TAIL_PER_HALF=0", "SPFE_BF16_WS=0", "SPFE_ZERO_IN_TAIL=0"})
    cs.push_back({B, 480, 752, 8, SYNC, e});
  cs.push_back({B, 96, 64, 2, SYNC, "SPFE_BF16_RW=0"});
  cs.push_back({F, 96, 64, 2, SYNC, nullptr});
  cs.push_back({B, 720, 1280, 8, SYNC, "SPFE_BF16_RW=1,3,2,0"});
  cs.push_back({B, 240, 320, 2, SYNC, nullptr});
  cs.push_back({B, 720, 1280, 8, SYNC, "SPFE_BF16_RW=0 SPFE_BF16_TILE_ROWS=16,1"});   // (16-row tiles of the streamed-weight kernel)
  for (const Config &c : cs) run(c, argv[1]);
  printf("== end: %d failed\n", g_failed);
  return g_failed ? 1 : 0;
}
