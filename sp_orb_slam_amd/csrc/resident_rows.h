// resident_rows.h — what the kernels over the resident map state (localmap.hip, covis.hip, cull.hip, mpcull.hip, lba.hip, newkf.hip) share beyond
// wave_ops.h: the grid of a launcher, the integer clamp, and the walk over one keyframe row with 16-byte loads.
// A row is kp_stride int32 entries at any 4-byte aligned address (rows of 1001 entries start 0, 4, 8 or 12 bytes off a 16-byte
// boundary), and nothing outside [row, row + stride) may be read: the last row ends where the caller's allocation ends.  So the walk
// is the scalar head in front of the row's first boundary, the vectors, and the scalar tail behind the last whole vector; it stands
// here once, and tests/hoststub/row_walk_check.cpp runs it on the CPU over every base and stride where it can go wrong.
// Plain C++ apart from the attributes: like conv_plan.h, a host compiler without HIP includes it.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SPFE_ROWS_FN __host__ __device__ __forceinline__
#else
#define SPFE_ROWS_FN inline
#endif

namespace spfe {

// workgroups of `wg` items for `work` items: at least one, at most `cap`
inline unsigned groups_for(size_t work, int wg, int cap) {
  const size_t g = (work + wg - 1) / wg;
  return (unsigned)(g < 1 ? 1 : (g > (size_t)cap ? (size_t)cap : g));
}

SPFE_ROWS_FN int clamp_int(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// `head` entries in front of the row's first 16-byte boundary (<= 3, and <= stride), `nvec` whole vectors from there on, and the
// entries from `tail0` on behind them (< 4)
struct RowSplit {
  int head, nvec, tail0;
};
SPFE_ROWS_FN RowSplit row_split(const int *row, int stride) {
  const int to_boundary = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u) >> 2);
  RowSplit r;
  r.head = to_boundary < stride ? to_boundary : stride;
  r.nvec = (stride - r.head) >> 2;
  r.tail0 = r.head + 4 * r.nvec;
  return r;
}

#if defined(__HIPCC__)
using RowVec = int4;
#else
struct alignas(16) RowVec {
  int x, y, z, w;
};
#endif

// Thread t of the T that share a row calls f(k, row[k]) for its entries k: all T together, every k in [0, stride) once.
// UNIFORM: every thread calls f in every step the T take, with p = -1 where it has no entry (f may ballot or meet a barrier); the
// steps are the head when there is one, the four entries of a vector each for every T vectors, the tail when there is one.
template <int T, bool UNIFORM = false, class F>
SPFE_ROWS_FN void row_walk(const int *row, int stride, int t, F &&f) {
  const RowSplit sp = row_split(row, stride);
  const RowVec *vrow = reinterpret_cast<const RowVec *>(row + sp.head);
  if constexpr (UNIFORM) {
    const int n_tail = stride - sp.tail0;
    if (sp.head) f(t, t < sp.head ? row[t] : -1);
    for (int v0 = 0; v0 < sp.nvec; v0 += T) {
      const int v = v0 + t, k = sp.head + 4 * v;
      const RowVec q = v < sp.nvec ? vrow[v] : RowVec{-1, -1, -1, -1};
      f(k, q.x);
      f(k + 1, q.y);
      f(k + 2, q.z);
      f(k + 3, q.w);
    }
    if (n_tail) f(sp.tail0 + t, t < n_tail ? row[sp.tail0 + t] : -1);
  } else {
    if (t < sp.head) f(t, row[t]);
    for (int v = t; v < sp.nvec; v += T) {
      const RowVec q = vrow[v];
      const int k = sp.head + 4 * v;
      f(k, q.x);
      f(k + 1, q.y);
      f(k + 2, q.z);
      f(k + 3, q.w);
    }
    if (sp.tail0 + t < stride) f(sp.tail0 + t, row[sp.tail0 + t]);
  }
}

}  // namespace spfe
