// plan_check.cpp — the convolution planner (csrc/conv_plan.h) alone, built with a plain C++ compiler and no HIP include path.
// argv[1] = the schedule trace (schedule_trace.cpp's output, tests/golden/schedule_trace.txt.gz unpacked).  For every section
// of the trace that runs the default switches in a synchronous call (and the f32 sections under the async flag) the ten layers
// are planned — whole batch, or conv1b whole and the rest as the two half batches n / 2 and n - n / 2 where the trace says the
// call was split — and each plan is held against the launch the trace shows for it: kernel family, template arguments (tile
// rows, first-layer mode, pool), frames, tile list, 64-channel blocks, item range, tile queue.  Layer 0's first-layer mode must
// say whether a conv1a launch stands in front.  Exit status 0: every plan matched.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "conv_plan.h"

using namespace spfe_plan;

struct Seen { std::string kernel; std::vector<int> targs; int B, tx, ty, nblk, lo, hi; bool queue; };
struct Want { std::string kernel; int i, B; ConvPlan c; int ty, lo, hi, tile; };

static int g_failed = 0, g_checked = 0;
#define FAIL(...) do { ++g_failed; printf(__VA_ARGS__); printf("\n"); } while (0)

static int field(const std::string &line, const char *key, int k = 0) {   // the k-th integer behind " key "
  size_t at = line.find(std::string(" ") + key + " ");
  if (at == std::string::npos) return -999;
  std::istringstream in(line.substr(at + strlen(key) + 2));
  int v = -999;
  for (int j = 0; j <= k; ++j) in >> v;
  return v;
}

static bool parse_launch(const std::string &line, Seen *s) {
  if (line.compare(0, 7, "launch ") || line.find(" tiles ") == std::string::npos) return false;
  const std::string name = line.substr(7, line.find(" grid ") - 7);
  s->kernel = name.substr(0, name.find('<'));
  s->targs.clear();
  if (name.find('<') != std::string::npos) {
    std::istringstream in(name.substr(name.find('<') + 1));
    for (std::string t; std::getline(in, t, ',');) {
      while (!t.empty() && (t[0] == ' ')) t.erase(0, 1);
      s->targs.push_back(t.compare(0, 4, "true") == 0 ? 1 : t.compare(0, 5, "false") == 0 ? 0 : atoi(t.c_str()));
    }
  }
  s->B = field(line, "B"); s->tx = field(line, "tiles", 0); s->ty = field(line, "tiles", 1); s->nblk = field(line, "nblk");
  s->lo = field(line, "items", 0); s->hi = field(line, "items", 1);
  s->queue = line.find(" ctr 0") == std::string::npos || line.find(" ctr 0/") != std::string::npos;
  return true;
}

static LayerShape layer(int i, int H, int W) {
  static const int cin[10] = {64, 64, 64, 64, 128, 128, 128, 128, 256, 256}, down[10] = {1, 2, 2, 4, 4, 8, 8, 8, 8, 8};
  static const int nblk[10] = {1, 1, 1, 2, 2, 2, 2, 8, 2, 4};
  static const bool pool[10] = {true, false, true, false, true, false, false, false, false, false};
  return LayerShape{cin[i], i < 8 ? 3 : 1, pool[i], i < 8, H / down[i], W / down[i], nblk[i]};
}

// What spfe_create leaves on a handle whose environment sets no switch: a copy, by hand, of the defaults in read_switches() /
// build() (spfe_pack.hip) and of the members' initialisers (spfe_host.h).  A changed default there changes the recorded trace;
// this table and the sparse_da of the CallMode below then follow by hand (the sections with switches set are the trace test's).
static Switches defaults(bool bf16, int H, int W, int max_batch) {
  Switches sw{};
  sw.fuse1a = false; sw.fuse1a_env = -1; sw.fuse1a_bf16 = bf16;
  sw.tile16x4 = 1; sw.tile2_auto = true; sw.tile2_mask = 0; sw.pool_split = -1;
  sw.pbtail = true; sw.f32_heads = false;
  sw.ws_min_items = 11; sw.ws_min_items_sync = 5;
  sw.bf16_rw = true; sw.rw_min4 = 3; sw.rw_min2 = 2; sw.rw_rows3 = 1;
  sw.bf16_dyn = true; sw.tile16_min_items = 3; sw.tile_rows_big = 12;
  for (int k = 0; k < 4; ++k) sw.has_ws[k] = sw.has_rw[k] = bf16;
  sw.unpooled_elems = !bf16 && !(H & 15) && !(W & 15) ? (size_t)std::min(max_batch, 2) * (H / 2) * (W / 2) * 64 : 0;
  return sw;
}

static void expect(std::vector<Want> *out, int i, int frames, int H, int W, const CallMode &m, const Switches &sw) {
  const ConvPlan c = plan_conv(layer(i, H, W), i, frames, m, sw);
  Want w{"", i, frames, c, c.tiles_y, 0, 0, c.tile};
  switch (c.family) {
    case Family::InTail: case Family::Head: return;   // (no convolution launch)
    case Family::Bf16Ws: w.kernel = "spfe::ws::conv_bf16_ws_kernel"; break;
    case Family::Bf16Rw: w.kernel = "spfe::rw::conv_bf16_rw_kernel"; break;
    case Family::Bf16Streamed: w.kernel = "spfe::conv_bf16_kernel"; break;
    default: w.kernel = "spfe::conv_f32_kernel"; break;
  }
  if (c.family == Family::F32Split16) {
    Want a = w;
    a.ty = c.tiles_y16; a.hi = c.hi16; a.tile = 4;
    out->push_back(a);
    w.lo = c.lo8; w.hi = c.hi8; w.tile = 0;
  }
  out->push_back(w);
}

static void check(const std::string &title, const Want &w, const Seen &s) {
  ++g_checked;
  const LayerShape L = layer(w.i, 8, 8);
  bool ok = w.kernel == s.kernel && w.B == s.B && w.c.tiles_x == s.tx && w.ty == s.ty && w.c.nblk == s.nblk && w.lo == s.lo &&
            w.hi == s.hi && w.c.queue == s.queue;
  const bool pooled = w.c.family == Family::F32PoolSplit ? false : L.pool;
  // <LAYER, CIN, KS, KC, WM, WN, MT, NT, POOL, RELU>: WM x MT rows per tile; the first layer's own instantiations (LAYER 1 | 2)
  // exist for 8- and 16-row tiles, on 4-row tiles conv1b is the generic kernel (launch_conv_f32)
  const int layer_tag = w.c.family == Family::F32Split16 ? 1 : w.c.family == Family::F32 && w.tile != 1 ? w.c.first : 0;
  if (ok && w.kernel == "spfe::conv_f32_kernel")
    ok = s.targs.size() == 10 && s.targs[0] == layer_tag &&
         s.targs[4] * s.targs[6] == f32_tile_rows(w.tile) && s.targs[1] == L.cin && s.targs[8] == pooled;
  if (ok && w.kernel == "spfe::ws::conv_bf16_ws_kernel") ok = s.targs.size() == 2 && s.targs[0] == L.pool && s.targs[1] == w.c.first;
  if (ok && w.kernel == "spfe::rw::conv_bf16_rw_kernel") ok = s.targs.size() == 2 && s.targs[0] == w.c.rows && s.targs[1] == L.pool;
  if (ok && w.kernel == "spfe::conv_bf16_kernel")   // <CIN, POOL, OUT_F32, MT>: 4 MT rows per tile
    ok = s.targs.size() == 4 && s.targs[0] == L.cin && s.targs[1] == L.pool && 4 * s.targs[3] == w.c.rows;
  if (!ok)
    FAIL("%s: layer %d on %d frames: planned %s tile %d tiles %d x %d nblk %d items [%d, %d) queue %d first %d, the trace shows %s B %d tiles %d x %d nblk %d items [%d, %d) queue %d",
         title.c_str(), w.i, w.B, w.kernel.c_str(), w.tile, w.c.tiles_x, w.ty, w.c.nblk, w.lo, w.hi, (int)w.c.queue, w.c.first,
         s.kernel.c_str(), s.B, s.tx, s.ty, s.nblk, s.lo, s.hi, (int)s.queue);
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: plan_check <schedule trace>\n"); return 2; }
  std::ifstream in(argv[1]);
  std::vector<std::string> lines;
  for (std::string l; std::getline(in, l);) lines.push_back(l);
  int sections = 0, halves = 0;
  for (size_t at = 0; at < lines.size(); ++at) {
    char prec[8], mode[16], env[64];
    int H, W, n;
    if (sscanf(lines[at].c_str(), "== %7s %dx%d n=%d %15s %63s", prec, &H, &W, &n, mode, env) != 6) continue;
    const bool bf16 = !strcmp(prec, "bf16"), sync = !strcmp(mode, "sync");
    if (strcmp(env, "-") || !(sync || (!bf16 && !strcmp(mode, "async_cov")))) continue;
    ++sections;
    CallMode m{!sync, false, 256, bf16, n, true};   // (the gathered convDa is the default of both precisions in these calls)
    const Switches sw = defaults(bf16, H, W, n);
    for (int call = 0; call < 3; ++call) {
      while (++at < lines.size() && lines[at].compare(0, 8, "-- call ")) {}
      const int split = field(lines[at], "split_streams", 1);
      std::vector<Seen> seen;
      bool conv1a = false;
      for (size_t k = at + 1; k < lines.size() && lines[k].compare(0, 2, "--") && lines[k].compare(0, 2, "=="); ++k) {
        Seen s;
        if (parse_launch(lines[k], &s)) seen.push_back(s);
        conv1a |= lines[k].find("launch spfe::conv1a_") == 0;
      }
      std::vector<Want> want;
      expect(&want, 0, n, H, W, m, sw);
      // (convDb runs gathered in these calls, nine layers on the launch streams; asked all the same: bf16 the head GEMM, f32 —
      // SPFE_F32_HEADS unset — the generic kernel on 4-row tiles)
      const ConvPlan db = plan_conv(layer(9, H, W), 9, n, m, sw);
      if (bf16 ? db.family != Family::Head : db.family != Family::F32 || db.tile != 1) FAIL("layer 9: family %d tile %d", (int)db.family, db.tile);
      for (int i = 1; i < 9; ++i) {
        if (!split) { expect(&want, i, n, H, W, m, sw); continue; }
        expect(&want, i, n / 2, H, W, m, sw);
        expect(&want, i, n - n / 2, H, W, m, sw);
        ++halves;
      }
      const std::string title = lines[at].substr(0, 9) + " of " + prec + " " + std::to_string(H) + "x" + std::to_string(W) + " n=" + std::to_string(n) + " " + mode;
      if (want.size() != seen.size()) { FAIL("%s: %zu convolution launches planned, the trace shows %zu", title.c_str(), want.size(), seen.size()); continue; }
      for (size_t k = 0; k < want.size(); ++k) check(title, want[k], seen[k]);
      // layer 0's plan is the answer to "does conv1b compute conv1a?": no conv1a launch exactly then
      if (conv1a == (plan_conv(layer(0, H, W), 0, n, m, sw).first == 2)) FAIL("%s: conv1a launched: %d, layer 0 planned first-layer mode %d", title.c_str(), (int)conv1a, want[0].c.first);
    }
  }
  printf("plan_check: %d sections, %d launches held against their plans, %d half-batch layers, %d mismatches\n", sections, g_checked, halves, g_failed);
  return g_failed || sections < 15 || halves == 0 ? 1 : 0;
}
