// conv_plan.h — what one convolution launch of the frame schedule will be, decided without touching HIP: kernel family, tile
// height, work-list geometry, tile queue, first-layer mode.  spfe_schedule.hip (enqueue) asks plan_conv() and carries the plan
// out; tests/hoststub/plan_check.cpp asks it alone.  Plain C++: no HIP type, no handle, no allocation; same inputs, same plan.
#pragma once
#include <algorithm>
#include <cstddef>

namespace spfe_plan {

// One enqueue() call as the decisions see it; made once per call (call_mode(), spfe_schedule.hip), read by enqueue_post() too.
struct CallMode {
  bool pipelined;      // the side chain overlaps the next call: SPFE_FLAG_ASYNC_COV, or a spfe_submit_batch step
  bool stage_events;   // SPFE_STAGE_TIMING=1: an event behind every stage, the table's launch order
  int cus;             // workgroups of a persistent grid
  bool bf16;
  int n;               // frames of the call (a launch may cover half of them)
  bool sparse_da;      // convDa runs gathered behind the selection: the dense convPa|Da launch computes convPa only
};
// What read_switches() set on the handle (same names), and what build() packed or allocated, as far as a plan depends on it.
struct Switches {
  bool fuse1a; int fuse1a_env; bool fuse1a_bf16; int tile16x4; bool tile2_auto; unsigned tile2_mask; int pool_split;
  bool pbtail, f32_heads; int ws_min_items, ws_min_items_sync; bool bf16_rw; int rw_min4, rw_min2, rw_rows3;
  bool bf16_dyn; int tile16_min_items, tile_rows_big;
  bool has_ws[4], has_rw[4];   // bf16: wave-specialised weights of layer k (Cin = 64), register-resident ones of layer 4 + k (Cin = 128)
  size_t unpooled_elems;       // floats of the un-pooled scratch buffer, 0: none
};
struct LayerShape { int cin = 0, ks = 0; bool pool = false, relu = false; int H = 0, W = 0, nblk = 0; };   // (H x W: the layer's input)
enum class Family {
  InTail,                          // nothing here: convPb rides in the detector tail's launch (pbtail_f32.hip / pbtail_bf16.hip)
  F32, F32PoolSplit, F32Split16,   // conv_f32.hip: one launch | un-pooled 2-row tiles + pool pass | conv1b cut in a 16- and an 8-row launch
  Bf16Ws, Bf16Rw, Bf16Streamed,    // conv_bf16_ws.hip (wave-specialised, Cin = 64) | conv_bf16_rw.hip (weights in registers) | conv_bf16.hip
  Head,                            // a 1x1 head as a GEMM over all cells: head_bf16.hip, head_f32.hip (SPFE_F32_HEADS=1)
};
struct ConvPlan {
  Family family = Family::F32;
  int tile = 0, rows = 8;     // f32: conv_f32.hip's tile_mode and its rows per tile; bf16: rows per tile, twice
  int tiles_x = 0, tiles_y = 0, nblk = 0;
  bool queue = false;         // bf16: work items in tile-queue order
  int first = 0;              // layer 0: 1 = conv1b, 2 = conv1b computes conv1a itself; 0 elsewhere
  long split16_rows = -1;     // F32Split16: the first split16_rows tile rows (of 16) of the batch as 16-row tiles: items [0, hi16) of
  int tiles_y16 = 0, hi16 = 0, lo8 = 0, hi8 = 0;   // that list (tiles_y16 a frame), the rest as items [lo8, hi8) of the 8-row list
};

// rows per tile of conv_f32.hip's tile_mode (the planner's copy of that file's conv_tile_rows(); launch_conv_f32 picks the kernels by it)
inline int f32_tile_rows(int tile_mode) { return tile_mode == 1 ? 4 : tile_mode == 2 || tile_mode == 4 ? 16 : tile_mode == 3 ? 2 : 8; }

// Critical path of a layer over the persistent grid, in rounds of 4-row items: 8-row tiles do 4 MFMAs per K step and wave
// (better hidden side work: 2.0 x 0.93 of a 4-row item), 4-row tiles give twice the work items, 2-row items cost 0.56 of a
// 4-row one (measured, batch 1: conv4a / 4b 45 -> 27 us, convPa|Da 80 -> 64, conv3a 46 -> 38)
struct TileCosts { double big, small, tiny; };
inline TileCosts tile_costs(long tx, int H, long nblk, int n, long g) {
  const long r8 = (tx * ((H + 7) / 8) * nblk * n + g - 1) / g, r4 = (tx * ((H + 3) / 4) * nblk * n + g - 1) / g;
  return {(double)r8 * 2.0 * 0.93, (double)r4, (double)((tx * ((H + 1) / 2) * nblk * n + g - 1) / g) * 0.56};
}

inline ConvPlan plan_conv_bf16(const LayerShape &L, int i, int n, const CallMode &m, const Switches &sw) {
  ConvPlan c;
  if (i >= 8) { c.family = i == 8 && sw.pbtail ? Family::InTail : Family::Head; return c; }
  // 8-row tiles; convPa|Da (i == 7) write bf16 for the bf16 heads
  c.tiles_x = (L.W + 31) / 32; c.tiles_y = (L.H + 7) / 8; c.nblk = L.nblk;
  c.tile = c.rows = 8;
  c.first = i == 0 ? 1 : 0;
  const long items = (long)c.tiles_x * c.tiles_y * n, grid_ws = m.cus & ~15, grid = std::max(8L, grid_ws);
  // the wave-specialised kernel has the higher rate but ~8 us more start-up (512-thread workgroups, two barriers before the
  // first MFMA): it takes the launches with enough work items per workgroup (tools/microbench/conv_ws_probe: the crossover
  // is at ~10 items; the bar is picked per call: spfe_pack.hip).  On conv1b its producer waves compute conv1a (first = 2)
  if (i < 4 && sw.has_ws[i] && L.W >= 32 &&
      items * c.nblk >= (long)(m.pipelined ? sw.ws_min_items : sw.ws_min_items_sync) * std::max(16L, grid_ws)) {
    c.family = Family::Bf16Ws;
    c.queue = true;
    if (i == 0 && sw.fuse1a_bf16) c.first = 2;
    return c;
  }
  if (i == 7 && m.sparse_da) c.nblk = L.nblk / 2;   // convPa only: convDa runs gathered, behind the selection (da_gather_bf16.hip)
  // Cin = 128: weights resident in registers (conv_bf16_rw.hip) when every workgroup of a 128-channel group gets enough
  // tiles; 4-row tiles, or 2-row tiles for the small launches (twice the tiles)
  if (L.cin == 128 && i >= 4 && sw.bf16_rw && sw.has_rw[i - 4] && L.W >= 32 && !(L.W & 1) && !(L.pool && (L.H & 1))) {
    const int ncg = c.nblk / 2;
    const long wgs = std::max(8L * ncg, (long)(m.cus / (8 * ncg)) * 8 * ncg) / ncg;
    const long t4 = (long)c.tiles_x * ((L.H + 3) / 4) * n, t2 = (long)c.tiles_x * ((L.H + 1) / 2) * n;
    int tr = t4 >= (long)sw.rw_min4 * wgs ? 4 : t2 >= (long)sw.rw_min2 * wgs ? 2 : 0;
    // layers without a pool may take 3-row tiles: whichever of 4 / 3 rows needs fewer row-rounds on the slowest workgroup
    // (convPa|Da at 1280x720 x 8: 920 four-row tiles over 64 workgroups = 15 rounds of 4 rows, 1200 three-row tiles = 19 of 3)
    if (tr == 4 && !L.pool && sw.rw_rows3 && (((long)c.tiles_x * ((L.H + 2) / 3) * n + wgs - 1) / wgs) * 3 < ((t4 + wgs - 1) / wgs) * 4) tr = 3;
    if (tr) {
      c.family = Family::Bf16Rw;
      c.tile = c.rows = tr; c.nblk = ncg; c.tiles_y = (L.H + tr - 1) / tr;
      c.queue = true;
      return c;
    }
  }
  // streamed weights (conv_bf16.hip).  Taller tiles for the Cin = 128 layers when that still leaves every workgroup >=
  // tile16_min_items items (MT = 3 / 4: a stage's weight chunk feeds 1.5x / 2x the MFMAs).  Measured: 12-row tiles (layers
  // without a pool) -3...5 % on convPa|Da; 16-row tiles need 512 VGPRs + spills and lose 35 %: not the default.
  c.family = Family::Bf16Streamed;
  const int tr = sw.tile_rows_big > 0 ? sw.tile_rows_big : 16;
  if (L.cin == 128 && sw.tile16_min_items > 0 && (tr == 16 || !L.pool) &&
      (long)c.tiles_x * ((L.H + tr - 1) / tr) * n * c.nblk >= (long)sw.tile16_min_items * grid) {
    c.tile = c.rows = tr;
    c.tiles_y = (L.H + tr - 1) / tr;
  }
  // work items in queue order (CtlB::dyn; SPFE_BF16_DYN_QUEUE=0: static); launches with a handful of items per workgroup stay
  // static: the queue costs them more than it balances
  c.queue = L.cin == 128 && sw.bf16_dyn && (long)c.tiles_x * c.tiles_y * n * c.nblk >= 5L * grid;
  return c;
}

// The launch of layer i (0 = conv1b ... 7 = convPa|Da, 8 = convPb, 9 = convDb) on n frames of a call.
inline ConvPlan plan_conv(const LayerShape &L, int i, int n, const CallMode &m, const Switches &sw) {
  if (m.bf16) return plan_conv_bf16(L, i, n, m, sw);
  ConvPlan c;
  if (i == 8 && sw.pbtail) { c.family = Family::InTail; return c; }
  if (i >= 8 && sw.f32_heads) { c.family = Family::Head; return c; }
  // conv1b computes conv1a's outputs itself — on request (SPFE_FUSE_CONV1A=1; perf-neutral on batches), and by default in
  // single-frame synchronous calls, where a launch and its boundary less are worth 5 us (752x480: p50 0.7266 -> 0.7213 ms)
  const bool fused = i == 0 && (sw.fuse1a || (sw.fuse1a_env < 0 && m.n == 1 && !m.pipelined && !m.stage_events));
  const long tx = (L.W + 31) / 32, g = m.cus, ty8 = (L.H + 7) / 8, ty16 = (L.H + 15) / 16;
  c.tiles_x = (int)tx;
  c.nblk = i == 7 && m.sparse_da ? L.nblk / 2 : L.nblk;   // (convPa alone when convDa runs gathered: da_gather_f32.hip)
  c.first = i == 0 ? (fused ? 2 : 1) : 0;
  // tile height per layer and batch: the one with the shorter critical path; the 1x1 heads run on 4-row tiles
  bool small_tile = L.ks != 3, tiny_tile = false;
  if (L.ks == 3) {
    const TileCosts t = tile_costs(tx, L.H, c.nblk, n, g);
    small_tile = t.small < t.big;
    // 2-row tiles (layers without a pool): a single frame's low-resolution layers are 90 ... 360 four-row items on 256
    // CUs — one round of long items with CUs idle; at 8 frames per call the model keeps the taller tiles
    if (!L.pool && L.relu && !fused && sw.tile2_auto) tiny_tile = t.tiny < std::min(t.small, t.big);
    // a pooled layer as un-pooled 2-row tiles + a pool pass (single-frame calls: one scratch buffer; spfe_handle_s::pool_split);
    // 0.12: the pool pass — ~6 us against the ~50 us of a 4-row round at K = 1152
    if (L.pool && L.relu && i > 0 && i < 7 && sw.unpooled_elems && sw.pool_split != 0 && m.n == 1 && !(L.H & 1) && !(L.W & 1) &&
        (size_t)n * L.H * L.W * (64 * L.nblk) <= sw.unpooled_elems &&
        (sw.pool_split > 0 || t.tiny + 0.12 < std::min(t.small, t.big) - 0.02)) {
      c.family = Family::F32PoolSplit;
      c.tile = 3; c.rows = 2; c.tiles_y = (L.H + 1) / 2; c.nblk = L.nblk;
      return c;
    }
  }
  c.tile = small_tile && !fused ? 1 : 0;   // (the fused first layer exists for 8-row tiles only)
  // conv1b: 16-row tiles of 4 wavefronts x 4 rows x 64 channels (6 operand reads per 8 MFMAs instead of 8; bit-identical):
  // measured on conv1b 2.2 ... 2.5 % per tile (640x480: 0.863 -> 0.882 of peak; 752x480: the coarser list costs 45 -> 46
  // round equivalents and it still gains 0.3 %; whole path +0.6 ... 0.8 %) — taken when its rounds are not more than 2.5 %
  // longer than the 8-row list's.  SPFE_TILE16X4=0: never, 2: always (one launch)
  // ... and when neither list divides well, BOTH: the first k tile rows (of 16) of the batch as 16-row tiles, the rest as
  // 8-row tiles in a second launch — 752x480 x 8: 224 of 240 tile rows = 21 rounds exactly + 768 eight-row tiles = 3
  // rounds exactly = 45 round equivalents, 42 of them at the 16-row rate (46 with 16-row tiles alone).  SPFE_TILE16X4=3:
  // no second launch
  if (i == 0 && !fused && L.pool && sw.tile16x4 && (c.tile == 0 || sw.tile16x4 == 2)) {
    const long r8 = (tx * ty8 * n + g - 1) / g, r16 = (tx * ty16 * n + g - 1) / g;
    const double k16 = 0.975, c8 = (double)r8, c16 = 2.0 * r16 * k16;   // (a 16-row item against two 8-row ones)
    double best = std::min(c8, c16);
    if (c16 < c8 || sw.tile16x4 == 2) c.tile = 4;
    if (sw.tile16x4 == 1 && r8 >= 8)   // (large launches only: the second launch costs a kernel boundary)
      for (long k = ty16 * n - 1; k > 0 && k >= ty16 * n - 4 * ty16; --k) {   // (frames before k / ty16 whole, k % ty16 tile rows of that frame)
        const long rows8 = (ty8 - std::min(2 * (k % ty16), ty8)) + (n - k / ty16 - 1) * ty8;
        const double cost = 2.0 * ((tx * k + g - 1) / g) * k16 + (double)((tx * rows8 + g - 1) / g) + 0.3;
        if (cost < best - 0.2) { best = cost; c.split16_rows = k; }
      }
  }
  if (tiny_tile && c.tile != 2 && c.tile != 4) c.tile = 3;
  if (L.ks == 3 && !L.pool && L.relu && ((sw.tile2_mask >> i) & 1)) c.tile = 3;
  c.rows = f32_tile_rows(c.tile);
  c.tiles_y = (L.H + c.rows - 1) / c.rows;
  if (c.split16_rows > 0) {
    const long k = c.split16_rows;
    c.family = Family::F32Split16;
    c.rows = 16; c.tiles_y = (int)ty8; c.tiles_y16 = (int)ty16;
    c.hi16 = (int)(tx * k); c.lo8 = (int)((k / ty16 * ty8 + std::min(2 * (k % ty16), ty8)) * tx); c.hi8 = (int)(tx * ty8 * n);
  }
  return c;
}

}  // namespace spfe_plan
