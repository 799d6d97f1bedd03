// row_walk_check.cpp — the row split and the row walk of csrc/resident_rows.h alone, built with a plain C++ compiler and no HIP include
// path.  Rows lie 0, 4, 8 and 12 bytes off a 16-byte boundary, strides are 1 .. 67, 101, 1000 and 1001; every row sits between two
// poisoned words, and the walk is the header's own code, run thread by thread for 64 and for 256 threads, in both variants.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "resident_rows.h"

static int g_failed = 0;
#define CHECK(cond, ...)                                            \
  do {                                                              \
    if (!(cond)) {                                                  \
      if (++g_failed <= 20) {                                       \
        fprintf(stderr, "CHECK failed %s:%d: %s: ", __FILE__, __LINE__, #cond); \
        fprintf(stderr, __VA_ARGS__);                               \
        fprintf(stderr, "\n");                                      \
      }                                                             \
    }                                                               \
  } while (0)

constexpr int POISON = 0x7badbad7;

// every thread of the T walks the row; entry k holds k, so a read outside the row shows as a value that is no index of it
template <int T, bool UNIFORM>
static void walk_case(const int *row, int stride, int off) {
  std::vector<int> visits(stride, 0);
  long calls = 0, empty = 0;
  std::vector<long> calls_of(T, 0);
  for (int t = 0; t < T; ++t)
    spfe::row_walk<T, UNIFORM>(row, stride, t, [&](int k, int p) {
      ++calls;
      ++calls_of[t];
      if (UNIFORM && p == -1) {
        ++empty;
        return;
      }
      CHECK(k >= 0 && k < stride, "T %d uniform %d off %d stride %d: k %d outside the row", T, (int)UNIFORM, off, stride, k);
      CHECK(p == k, "T %d uniform %d off %d stride %d: entry %d read as %d", T, (int)UNIFORM, off, stride, k, p);
      if (k >= 0 && k < stride) ++visits[k];
    });
  for (int k = 0; k < stride; ++k)
    CHECK(visits[k] == 1, "T %d uniform %d off %d stride %d: entry %d visited %d times", T, (int)UNIFORM, off, stride, k, visits[k]);
  if (UNIFORM) {   // every thread made the same number of calls: a step is taken by all T or by none (a ballot hangs otherwise)
    const spfe::RowSplit sp = spfe::row_split(row, stride);
    const long steps = (sp.head ? 1 : 0) + 4 * (long)((sp.nvec + T - 1) / T) + (stride - sp.tail0 ? 1 : 0);
    for (int t = 0; t < T; ++t)
      CHECK(calls_of[t] == steps, "T %d off %d stride %d: thread %d made %ld calls, the row has %ld steps", T, off, stride, t, calls_of[t], steps);
    CHECK(calls - empty == stride, "T %d off %d stride %d: %ld calls, %ld without an entry", T, off, stride, calls, empty);
  } else {
    CHECK(calls == stride && empty == 0, "T %d off %d stride %d: %ld calls", T, off, stride, calls);
  }
}

int main() {
  std::vector<int> strides;
  for (int s = 1; s <= 67; ++s) strides.push_back(s);
  for (int s : {101, 1000, 1001}) strides.push_back(s);
  int cases = 0;
  for (int off = 0; off < 4; ++off)   // ints off the boundary: 0, 4, 8, 12 bytes
    for (int stride : strides) {
      // [poison x (4 + off)] [row] [poison x 8] in a 16-byte aligned block: the row starts 4 * off bytes off a boundary
      void *mem = nullptr;
      if (posix_memalign(&mem, 16, sizeof(int) * (size_t)(4 + off + stride + 8))) return 2;
      int *blk = static_cast<int *>(mem), *row = blk + 4 + off;
      for (int i = 0; i < 4 + off + stride + 8; ++i) blk[i] = POISON;
      for (int k = 0; k < stride; ++k) row[k] = k;
      const spfe::RowSplit sp = spfe::row_split(row, stride);
      CHECK(sp.head >= 0 && sp.head <= 3 && sp.head <= stride, "off %d stride %d: head %d", off, stride, sp.head);
      CHECK(sp.nvec >= 0 && (sp.nvec == 0 || reinterpret_cast<uintptr_t>(row + sp.head) % 16 == 0), "off %d stride %d: the vectors start off a boundary", off, stride);
      CHECK(sp.tail0 == sp.head + 4 * sp.nvec && sp.tail0 <= stride && stride - sp.tail0 < 4, "off %d stride %d: tail0 %d", off, stride, sp.tail0);
      walk_case<64, false>(row, stride, off);
      walk_case<64, true>(row, stride, off);
      walk_case<256, false>(row, stride, off);
      walk_case<256, true>(row, stride, off);
      free(mem);
      ++cases;
    }
  CHECK(spfe::groups_for(0, 256, 8) == 1 && spfe::groups_for(257, 256, 8) == 2 && spfe::groups_for(1u << 20, 256, 8) == 8, "groups_for");
  CHECK(spfe::clamp_int(-3, 0, 5) == 0 && spfe::clamp_int(9, 0, 5) == 5 && spfe::clamp_int(4, 0, 5) == 4, "clamp_int");
  printf("row_walk_check: %d rows, %d failed checks\n", cases, g_failed);
  return g_failed ? 1 : 0;
}
