// lba.hip — the local bundle adjustment's surroundings on resident state: the gather of the problem (optimizer.cpp:447-499, :568-658)
// and the application of the solver's result to the rows, the table and the poses (:660-662, :739-773).  The contract is
// include/spfe_lba_math.h (integers and copied bytes); the host statement the tests hold these kernels to is
// tests/lba_ref/lba_ref.c: the blocks and every edited array are equal byte for byte.  The solver itself is ba.hip, untouched.
//
// The launches, whatever the sizes are:
//   gather  lba_preset_kernel   multi-workgroup: the block zeroed, the scratch's presets.
//           lba_local_kernel    ONE workgroup: (G1) — the first entry of a slot in the ord row by atomicMin, ordered ranks, the cut.
//           lba_first_kernel    multi-workgroup: the key of every point of the local rows by atomicMin.
//           lba_points_kernel   ONE workgroup over chunks of the local rows: the stable compaction of the first occurrences (G2).
//           lba_scan_kernel     multi-workgroup, a wavefront a row of ALL slots that are not bad, 16-byte loads from the row's first
//                               aligned boundary: a hit is an entry whose point is listed; counts per point by atomicAdd, the hits
//                               appended to an unordered list (a wavefront claims its places with one atomicAdd), the least listed
//                               point of a non-local row (G4's key).
//           lba_fixed_kernel    multi-workgroup, a thread a slot: its place among the non-local observers by counting smaller keys.
//           lba_ecount_kernel   multi-workgroup, a thread a hit: the edges of every point (its hits in slots with a BA slot).
//           lba_place_kernel    ONE workgroup: the two prefix sums, the header, the poses, the tails of the lists.
//           lba_scatter_kernel  multi-workgroup, a thread a hit: into its point's range, in any order.
//           lba_order_kernel    multi-workgroup, a wavefront a point: the place of every entry of the range by counting smaller
//                               (slot, keypoint) keys — the output does not depend on the order of the scatter —, obs[] and edges[].
//   apply   lba_apply_preset    multi-workgroup: the block zeroed, the marks.
//           lba_apply_mark      a thread an erase entry: the observation it names marked, its row entry -1.
//           lba_apply_point     a thread a point, the ONE owner of its nobs, flags, ref_slot and position.
//           lba_apply_finish    ONE workgroup: the prefix sum of the remaining observations, bad_point[], the header.
//           lba_apply_lists     multi-workgroup: the post-erase lists, the poses, the tails.
// No workgroup waits for another: the order between the kernels of a call is the launch boundary.  Every sum of atomics is a sum or
// a minimum of integers; where an atomic hands out places (the hit list, the scatter) a later kernel orders what was placed.
#include <algorithm>
#include <climits>

#include "../../include/spfe.h"
#include "../../include/spfe_lba_math.h"
#include "spfe_kernels.h"
#include "wave_ops.h"
#include "resident_rows.h"

namespace spfe {

namespace {
constexpr int LB_WG = 256;
constexpr int LB_GRID = 1024;
constexpr int LB_ONE = 1024;            // the one-workgroup kernels
constexpr int LB_ONE_WAVES = LB_ONE / 64;
constexpr int NONE = SPFE_LBA_KEY_NONE;
// misc[] of the gather
constexpr int G_NLOCAL = 0, G_NFREE = 1, G_STATUS = 2, G_NPOINTS = 3, G_NPOINTS_ALL = 4, G_NHITS = 5, G_NFIXED_ALL = 6, G_INTS = 16;
// misc[] of the application
constexpr int A_WILD = 0, A_NERASED = 1, A_NMOVED = 2, A_INTS = 16;

struct GScratch {
  int *key, *rank;                       // [n_table]
  int *first_ord, *ba_of, *fkey;         // [n_slots]
  int *cnt, *ecnt, *fill, *estart;       // [point_cap]
  int4 *hits;                            // [edge_cap] (point, slot, keypoint, 0), unordered
  unsigned long long *placed;            // [edge_cap] obs keys, a point's range unordered
  int *misc;
};
__host__ __device__ inline GScratch g_scratch(uint8_t *b, int n_table, int n_slots, int point_cap, int edge_cap) {
  GScratch s;
  auto take = [&b](size_t bytes) { uint8_t *p = b; b += pad16(bytes); return p; };
  s.key = reinterpret_cast<int *>(take(4 * (size_t)n_table));
  s.rank = reinterpret_cast<int *>(take(4 * (size_t)n_table));
  s.first_ord = reinterpret_cast<int *>(take(4 * (size_t)n_slots));
  s.ba_of = reinterpret_cast<int *>(take(4 * (size_t)n_slots));
  s.fkey = reinterpret_cast<int *>(take(4 * (size_t)n_slots));
  s.cnt = reinterpret_cast<int *>(take(4 * (size_t)point_cap));
  s.ecnt = reinterpret_cast<int *>(take(4 * (size_t)point_cap));
  s.fill = reinterpret_cast<int *>(take(4 * (size_t)point_cap));
  s.estart = reinterpret_cast<int *>(take(4 * (size_t)point_cap));
  s.hits = reinterpret_cast<int4 *>(take(16 * (size_t)edge_cap));
  s.placed = reinterpret_cast<unsigned long long *>(take(8 * (size_t)edge_cap));
  s.misc = reinterpret_cast<int *>(take(4 * (size_t)G_INTS));
  return s;
}
__device__ __forceinline__ GScratch g_scratch(const LbaGatherArgs &a) { return g_scratch(a.scratch, a.n_table, a.n_slots, a.point_cap, a.edge_cap); }

// the gather's block
struct GBlock {
  int *hdr, *kf_slot;
  uint8_t *fixed;
  float *Tcw;
  int *point_idx;
  float *xyz;
  int *obs_start, *obs, *edges;
};
__device__ __forceinline__ GBlock g_block(uint8_t *o, int k, int p, int e) {
  GBlock b;
  b.hdr = reinterpret_cast<int *>(o);
  b.kf_slot = reinterpret_cast<int *>(o + SPFE_LBA_OFF_KF_SLOT);
  b.fixed = o + SPFE_LBA_OFF_FIXED(k);
  b.Tcw = reinterpret_cast<float *>(o + SPFE_LBA_OFF_TCW(k));
  b.point_idx = reinterpret_cast<int *>(o + SPFE_LBA_OFF_POINT_IDX(k));
  b.xyz = reinterpret_cast<float *>(o + SPFE_LBA_OFF_XYZ(k, p));
  b.obs_start = reinterpret_cast<int *>(o + SPFE_LBA_OFF_OBS_START(k, p));
  b.obs = reinterpret_cast<int *>(o + SPFE_LBA_OFF_OBS(k, p));
  b.edges = reinterpret_cast<int *>(o + SPFE_LBA_OFF_EDGES(k, p, e));
  return b;
}
__device__ __forceinline__ GBlock g_block(const LbaGatherArgs &a) { return g_block(a.out, a.kf_cap, a.point_cap, a.edge_cap); }

__device__ __forceinline__ void zero_block(uint8_t *out, size_t bytes, size_t tid, size_t nth) {   // bytes: a multiple of 256
  int4 *o = reinterpret_cast<int4 *>(out);
  for (size_t i = tid; i < bytes / 16; i += nth) o[i] = make_int4(0, 0, 0, 0);
}
}  // namespace

// ---- (G) --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LB_WG) void lba_preset_kernel(LbaGatherArgs a) {
  const GScratch sc = g_scratch(a);
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
  zero_block(a.out, SPFE_LBA_GATHER_BYTES(a.kf_cap, a.point_cap, a.edge_cap), tid, nth);
  for (size_t p = tid; p < (size_t)a.n_table; p += nth) {
    sc.key[p] = NONE;
    sc.rank[p] = -1;
  }
  for (size_t s = tid; s < (size_t)a.n_slots; s += nth) {
    sc.first_ord[s] = NONE;
    sc.ba_of[s] = -1;
    sc.fkey[s] = NONE;
  }
  for (size_t i = tid; i < (size_t)a.point_cap; i += nth) sc.cnt[i] = sc.ecnt[i] = sc.fill[i] = sc.estart[i] = 0;
  if (tid < (size_t)G_INTS) sc.misc[tid] = 0;
}

__global__ __launch_bounds__(LB_ONE) void lba_local_kernel(LbaGatherArgs a) {
  __shared__ int wt_a[LB_ONE_WAVES], wt_b[LB_ONE_WAVES];
  __shared__ int sh_end, sh_local, sh_free, sh_cut;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const GScratch sc = g_scratch(a);
  const GBlock blk = g_block(a);
  const int cur_fixed = a.cur_slot == a.origin_slot;
  if (tid == 0) {
    sh_end = a.conn_cap;
    sh_local = 1;
    sh_free = cur_fixed ? 0 : 1;
    sh_cut = 0;
  }
  __syncthreads();
  for (int j = tid; j < a.conn_cap; j += LB_ONE)
    if (a.ord_row[j] == -1) atomicMin(&sh_end, j);
  __syncthreads();
  const int end = sh_end;
  for (int j = tid; j < end; j += LB_ONE) {
    const int s = a.ord_row[j];
    if (spfe_lb_in_range(s, a.n_slots) && s != a.cur_slot && !(a.kf_flags[s] & 1u)) atomicMin(&sc.first_ord[s], j);
  }
  __threadfence();
  __syncthreads();
  int kept_before = 0, free_before = 0;
  for (int base = 0; base < end; base += LB_ONE) {   // uniform
    const int j = base + tid;
    int s = -1;
    bool keep = false;
    if (j < end) {
      s = a.ord_row[j];
      keep = spfe_lb_in_range(s, a.n_slots) && s != a.cur_slot && !(a.kf_flags[s] & 1u) && load_agent(&sc.first_ord[s]) == j;
    }
    const bool is_fixed = s == a.origin_slot;
    int tk, tf;
    const int rk = wg_ordered_rank<LB_ONE>(keep, lane, wave, wt_a, &tk);
    const int rf = wg_ordered_rank<LB_ONE>(keep && !is_fixed, lane, wave, wt_b, &tf);
    if (keep) {
      const int pos = 1 + kept_before + rk, free_in = (cur_fixed ? 0 : 1) + free_before + rf;   // the list and the free count in front of it
      if (spfe_lb_local_fits(pos, free_in, is_fixed, a.kf_cap, a.free_cap)) {   // monotone: nothing fits behind an entry that does not
        blk.kf_slot[pos] = s;
        blk.fixed[pos] = is_fixed ? 1 : 0;
        sc.ba_of[s] = pos;
        atomicMax(&sh_local, pos + 1);
        atomicMax(&sh_free, free_in + (is_fixed ? 0 : 1));
      } else {
        sh_cut = 1;
      }
    }
    kept_before += tk;
    free_before += tf;
    __syncthreads();
  }
  if (tid == 0) {
    blk.kf_slot[0] = a.cur_slot;
    blk.fixed[0] = cur_fixed ? 1 : 0;
    sc.ba_of[a.cur_slot] = 0;
    sc.misc[G_NLOCAL] = sh_local;
    sc.misc[G_NFREE] = sh_free;
    sc.misc[G_STATUS] = sh_cut ? SPFE_LBA_LOCAL_CUT : 0;
  }
}

// entry idx = list position * kp_stride + keypoint of the local rows: the table row it names when that is a point (G2) may list, else -1
__device__ __forceinline__ int lba_local_entry(const LbaGatherArgs &a, const int *kf_slot, int idx) {
  const int b = idx / a.kp_stride, k = idx - b * a.kp_stride, s = kf_slot[b];
  if (a.kf_flags[s] & 1u) return -1;   // cur_slot alone can be bad here
  const int p = a.rows[(size_t)s * a.kp_stride + k];
  return spfe_lb_in_range(p, a.n_table) && spfe_lb_good(a.mp_flags[p]) ? p : -1;
}

__global__ __launch_bounds__(LB_WG) void lba_first_kernel(LbaGatherArgs a) {
  const GScratch sc = g_scratch(a);
  const GBlock blk = g_block(a);
  const int total = sc.misc[G_NLOCAL] * a.kp_stride;   // <= 128 * 16384
  for (int idx = blockIdx.x * LB_WG + threadIdx.x; idx < total; idx += gridDim.x * LB_WG) {
    const int p = lba_local_entry(a, blk.kf_slot, idx);
    if (p >= 0) atomicMin(&sc.key[p], idx);
  }
}

__global__ __launch_bounds__(LB_ONE) void lba_points_kernel(LbaGatherArgs a) {
  __shared__ int wt[LB_ONE_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const GScratch sc = g_scratch(a);
  const GBlock blk = g_block(a);
  const int total = sc.misc[G_NLOCAL] * a.kp_stride;
  int n_all = 0;
  for (int base = 0; base < total; base += LB_ONE) {   // uniform
    const int idx = base + tid;
    int p = -1;
    if (idx < total) {
      p = lba_local_entry(a, blk.kf_slot, idx);
      if (p >= 0 && sc.key[p] != idx) p = -1;
    }
    int t;
    const int pos = n_all + wg_ordered_rank<LB_ONE>(p >= 0, lane, wave, wt, &t);
    if (p >= 0 && pos < a.point_cap) {
      blk.point_idx[pos] = p;
      sc.rank[p] = pos;
      blk.xyz[3 * (size_t)pos] = a.xyz[3 * (size_t)p];
      blk.xyz[3 * (size_t)pos + 1] = a.xyz[3 * (size_t)p + 1];
      blk.xyz[3 * (size_t)pos + 2] = a.xyz[3 * (size_t)p + 2];
    }
    n_all += t;
    __syncthreads();
  }
  const int n = n_all < a.point_cap ? n_all : a.point_cap;
  for (int i = n + tid; i < a.point_cap; i += LB_ONE) blk.point_idx[i] = -1;   // xyz behind n: zero already
  if (tid == 0) {
    sc.misc[G_NPOINTS] = n;
    sc.misc[G_NPOINTS_ALL] = n_all;
    if (n_all > a.point_cap) sc.misc[G_STATUS] |= SPFE_LBA_POINT_CUT;
  }
}

// one entry of a row in the scan, by the whole wavefront: every lane calls it, with p = -1 where it has no entry
__device__ __forceinline__ void lba_scan_entry(const LbaGatherArgs &a, const GScratch &sc, int s, int k, int p, int lane, int *least) {
  const int i = spfe_lb_in_range(p, a.n_table) ? sc.rank[p] : -1;
  const bool hit = i >= 0;
  const unsigned long long votes = __ballot(hit);
  if (votes == 0) return;   // uniform
  int base = 0;
  const int leader = __ffsll((long long)votes) - 1;
  if (lane == leader) base = atomicAdd(&sc.misc[G_NHITS], __popcll(votes));
  base = __shfl(base, leader, 64);
  if (hit) {
    atomicAdd(&sc.cnt[i], 1);
    const long long at = (long long)base + __popcll(votes & ((1ull << lane) - 1ull));
    if (at < a.edge_cap) sc.hits[at] = make_int4(i, s, k, 0);
    *least = i < *least ? i : *least;
  }
}

__global__ __launch_bounds__(LB_WG) void lba_scan_kernel(LbaGatherArgs a) {
  const GScratch sc = g_scratch(a);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, stride = a.kp_stride;
  const int waves = LB_WG / 64;
  for (int s = blockIdx.x * waves + wave; s < a.n_slots; s += gridDim.x * waves) {   // uniform over the wavefront
    if (a.kf_flags[s] & 1u) continue;
    const int *row = a.rows + (size_t)s * stride;
    int least = NONE;
    row_walk<64, true>(row, stride, lane, [&](int k, int p) { lba_scan_entry(a, sc, s, k, p, lane, &least); });
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const int o = __shfl_xor(least, off, 64);
      least = o < least ? o : least;
    }
    if (lane == 0 && least != NONE && sc.ba_of[s] < 0) sc.fkey[s] = least;   // ba_of: the local list alone so far
  }
}

__global__ __launch_bounds__(LB_WG) void lba_fixed_kernel(LbaGatherArgs a) {
  const GScratch sc = g_scratch(a);
  const GBlock blk = g_block(a);
  const int room = a.kf_cap - sc.misc[G_NLOCAL], n_local = sc.misc[G_NLOCAL];
  for (int s = blockIdx.x * LB_WG + threadIdx.x; s < a.n_slots; s += gridDim.x * LB_WG) {
    const int mine = sc.fkey[s];
    if (mine == NONE) continue;
    atomicAdd(&sc.misc[G_NFIXED_ALL], 1);
    const uint64_t key = spfe_lb_fixed_key(mine, s);
    int r = 0;
    for (int t = 0; t < a.n_slots && r < room; ++t) {
      const int f = sc.fkey[t];
      r += f != NONE && spfe_lb_fixed_key(f, t) < key;
    }
    if (r < room) {
      blk.kf_slot[n_local + r] = s;
      blk.fixed[n_local + r] = 1;
      sc.ba_of[s] = n_local + r;
    }
  }
}

__global__ __launch_bounds__(LB_WG) void lba_ecount_kernel(LbaGatherArgs a) {
  const GScratch sc = g_scratch(a);
  const int n_hits = sc.misc[G_NHITS];
  if (n_hits > a.edge_cap) return;   // (G5): overflow
  for (int h = blockIdx.x * LB_WG + threadIdx.x; h < n_hits; h += gridDim.x * LB_WG) {
    const int4 q = sc.hits[h];
    if (sc.ba_of[q.y] >= 0) atomicAdd(&sc.ecnt[q.x], 1);
  }
}

__global__ __launch_bounds__(LB_ONE) void lba_place_kernel(LbaGatherArgs a) {
  __shared__ int wcnt[LB_ONE_WAVES];
  const int tid = threadIdx.x;
  const GScratch sc = g_scratch(a);
  const GBlock blk = g_block(a);
  const int n_local = sc.misc[G_NLOCAL], n = sc.misc[G_NPOINTS], n_hits = sc.misc[G_NHITS];
  const bool overflow = n_hits > a.edge_cap;
  const int room = a.kf_cap - n_local, fixed_all = sc.misc[G_NFIXED_ALL], n_fixed = fixed_all < room ? fixed_all : room, n_kf = n_local + n_fixed;
  int obs_total = 0, edge_total = 0;
  for (int base = 0; base < n; base += LB_ONE) {   // uniform
    const int i = base + tid, c = i < n ? sc.cnt[i] : 0, e = i < n ? sc.ecnt[i] : 0;
    int tc, te;
    const int oc = wg_ordered_offset<LB_ONE>(c, wcnt, &tc), oe = wg_ordered_offset<LB_ONE>(e, wcnt, &te);
    if (i < n) {
      blk.obs_start[i] = overflow ? -1 : obs_total + oc;
      sc.estart[i] = edge_total + oe;
    }
    obs_total += tc;
    edge_total += te;
  }
  if (tid == 0) blk.obs_start[n] = overflow ? -1 : obs_total;
  for (int i = n + 1 + tid; i <= a.point_cap; i += LB_ONE) blk.obs_start[i] = -1;
  for (int b = n_kf + tid; b < a.kf_cap; b += LB_ONE) blk.kf_slot[b] = -1;   // fixed and Tcw behind n_kf: zero already
  for (int t = tid; t < n_kf * 16; t += LB_ONE) blk.Tcw[t] = a.Tcw[(size_t)blk.kf_slot[t >> 4] * 16 + (t & 15)];   // kf_slot: earlier kernels'
  if (tid < 16) {
    int v = 0;
    if (tid == SPFE_LBA_OFF_STATUS / 4)
      v = sc.misc[G_STATUS] | (fixed_all > room ? SPFE_LBA_FIXED_CUT : 0) | (overflow ? SPFE_LBA_EDGE_OVERFLOW : 0);
    if (tid == SPFE_LBA_OFF_N_LOCAL / 4) v = n_local;
    if (tid == SPFE_LBA_OFF_N_FREE / 4) v = sc.misc[G_NFREE];
    if (tid == SPFE_LBA_OFF_N_FIXED / 4) v = n_fixed;
    if (tid == SPFE_LBA_OFF_N_KF / 4) v = n_kf;
    if (tid == SPFE_LBA_OFF_N_POINTS / 4) v = n;
    if (tid == SPFE_LBA_OFF_N_POINTS_ALL / 4) v = sc.misc[G_NPOINTS_ALL];
    if (tid == SPFE_LBA_OFF_N_OBS / 4) v = overflow ? 0 : obs_total;
    if (tid == SPFE_LBA_OFF_N_EDGES / 4) v = overflow ? 0 : edge_total;
    if (tid == SPFE_LBA_OFF_N_OBS_NEEDED / 4) v = n_hits;
    blk.hdr[tid] = v;
  }
}

__global__ __launch_bounds__(LB_WG) void lba_scatter_kernel(LbaGatherArgs a) {
  const GScratch sc = g_scratch(a);
  const GBlock blk = g_block(a);
  const int n_hits = sc.misc[G_NHITS];
  if (n_hits > a.edge_cap) return;
  for (int h = blockIdx.x * LB_WG + threadIdx.x; h < n_hits; h += gridDim.x * LB_WG) {
    const int4 q = sc.hits[h];
    const int at = blk.obs_start[q.x] + atomicAdd(&sc.fill[q.x], 1);   // inside [obs_start[i], obs_start[i + 1]): cnt[i] hits name i
    sc.placed[at] = spfe_lb_obs_key(q.y, q.z);
  }
}

__global__ __launch_bounds__(LB_WG) void lba_order_kernel(LbaGatherArgs a) {
  const GScratch sc = g_scratch(a);
  const GBlock blk = g_block(a);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = LB_WG / 64;
  const bool overflow = sc.misc[G_NHITS] > a.edge_cap;
  const int n = sc.misc[G_NPOINTS], n_obs = blk.hdr[SPFE_LBA_OFF_N_OBS / 4], n_edges = blk.hdr[SPFE_LBA_OFF_N_EDGES / 4];
  if (!overflow) {
    for (int i = blockIdx.x * waves + wave; i < n; i += gridDim.x * waves) {
      const int first = blk.obs_start[i], len = blk.obs_start[i + 1] - first, e0 = sc.estart[i];
      for (int e = lane; e < len; e += 64) {
        const unsigned long long key = sc.placed[first + e];
        const int slot = (int)(key >> 32), kp = (int)(uint32_t)key, b = sc.ba_of[slot];
        int r = 0, re = 0;
        for (int t = 0; t < len; ++t) {   // the keys of a range are distinct: a (slot, keypoint) pair is one row entry
          const unsigned long long o = sc.placed[first + t];
          const bool below = o < key;
          r += below;
          re += below && sc.ba_of[(int)(o >> 32)] >= 0;
        }
        blk.obs[2 * (size_t)(first + r)] = slot;
        blk.obs[2 * (size_t)(first + r) + 1] = kp;
        if (b >= 0) {
          int *ed = blk.edges + 3 * (size_t)(e0 + re);
          ed[0] = i;
          ed[1] = b;
          ed[2] = kp;
        }
      }
    }
  }
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
  for (size_t t = 2 * (size_t)n_obs + tid; t < 2 * (size_t)a.edge_cap; t += nth) blk.obs[t] = -1;
  for (size_t t = 3 * (size_t)n_edges + tid; t < 3 * (size_t)a.edge_cap; t += nth) blk.edges[t] = -1;
}

// ---- (A) --------------------------------------------------------------------------------------------------------------------------
namespace {
struct AScratch {
  uint8_t *mark;      // [edge_cap] the observation is erased
  uint8_t *went_bad;  // [point_cap]
  int *rem;           // [point_cap] remaining observations of a point that stays good
  int *misc;
};
__host__ __device__ inline AScratch a_scratch(uint8_t *b, int point_cap, int edge_cap) {
  AScratch s;
  s.mark = b;
  b += pad16((size_t)edge_cap);
  s.went_bad = b;
  b += pad16((size_t)point_cap);
  s.rem = reinterpret_cast<int *>(b);
  b += pad16(4 * (size_t)point_cap);
  s.misc = reinterpret_cast<int *>(b);
  return s;
}
// the two blocks as the application reads them; ok = (A0) passed, and then every count lies inside its capacity
struct AView {
  bool ok;
  int n_local, n_kf, n, n_obs, n_edges, n_erase;
  const int *kf_slot, *point_idx, *obs_start, *obs, *edges, *erase_idx;
  const float *Tcw_out, *xyz_out;
};
__device__ __forceinline__ AView a_view(const LbaApplyArgs &a) {
  AView v;
  const int *g = reinterpret_cast<const int *>(a.gather), *s = reinterpret_cast<const int *>(a.ba);
  const int g_status = g[SPFE_LBA_OFF_STATUS / 4], s_status = s[SPFE_BA_OFF_STATUS / 4];
  v.n_local = g[SPFE_LBA_OFF_N_LOCAL / 4];
  v.n_kf = g[SPFE_LBA_OFF_N_KF / 4];
  v.n = g[SPFE_LBA_OFF_N_POINTS / 4];
  v.n_obs = g[SPFE_LBA_OFF_N_OBS / 4];
  v.n_edges = g[SPFE_LBA_OFF_N_EDGES / 4];
  v.n_erase = s[SPFE_BA_OFF_N_ERASE / 4];
  v.ok = !(s_status & (SPFE_BA_STATUS_UNSORTED | SPFE_BA_STATUS_COV_OVERFLOW | SPFE_BA_STATUS_TOO_MANY_FREE | SPFE_BA_STATUS_STOPPED_EARLY)) &&
         !(g_status & SPFE_LBA_EDGE_OVERFLOW) && s[SPFE_BA_OFF_N_KF / 4] == v.n_kf && s[SPFE_BA_OFF_N_POINTS / 4] == v.n &&
         s[SPFE_BA_OFF_N_EDGES / 4] == v.n_edges && v.n_local >= 1 && v.n_local <= v.n_kf && v.n_kf <= a.kf_cap && v.n >= 0 &&
         v.n <= a.point_cap && v.n_edges >= 0 && v.n_edges <= v.n_obs && v.n_obs <= a.edge_cap && v.n_erase >= 0 && v.n_erase <= v.n_edges;
  if (!v.ok) v.n_local = v.n_kf = v.n = v.n_obs = v.n_edges = v.n_erase = 0;
  v.kf_slot = reinterpret_cast<const int *>(a.gather + SPFE_LBA_OFF_KF_SLOT);
  v.point_idx = reinterpret_cast<const int *>(a.gather + SPFE_LBA_OFF_POINT_IDX(a.kf_cap));
  v.obs_start = reinterpret_cast<const int *>(a.gather + SPFE_LBA_OFF_OBS_START(a.kf_cap, a.point_cap));
  v.obs = reinterpret_cast<const int *>(a.gather + SPFE_LBA_OFF_OBS(a.kf_cap, a.point_cap));
  v.edges = reinterpret_cast<const int *>(a.gather + SPFE_LBA_OFF_EDGES(a.kf_cap, a.point_cap, a.edge_cap));
  v.Tcw_out = reinterpret_cast<const float *>(a.ba + SPFE_BA_OFF_TCW);
  v.xyz_out = reinterpret_cast<const float *>(a.ba + SPFE_BA_OFF_XYZ(v.n_kf));
  v.erase_idx = reinterpret_cast<const int *>(a.ba + SPFE_BA_OFF_ERASE(v.n_kf, v.n, v.n_edges));
  return v;
}
// (A1): the observations of listed point i as [*first, *first + *len), empty when obs_start is not ascending inside [0, n_obs]
__device__ __forceinline__ bool a_range(const AView &v, int i, int *first, int *len) {
  const int lo = v.obs_start[i], hi = v.obs_start[i + 1];
  const bool fine = lo >= 0 && lo <= hi && hi <= v.n_obs;
  *first = fine ? lo : 0;
  *len = fine ? hi - lo : 0;
  return fine;
}
__device__ __forceinline__ bool a_valid_obs(const LbaApplyArgs &a, int slot, int kp) {
  return spfe_lb_in_range(slot, a.n_slots) && !(a.kf_flags[slot] & 1u) && spfe_lb_in_range(kp, a.kp_stride);
}
struct ABlock {
  int *hdr, *bad_point, *obs_start, *obs, *ref_slot;
};
__device__ __forceinline__ ABlock a_block(const LbaApplyArgs &a) {
  ABlock b;
  b.hdr = reinterpret_cast<int *>(a.out);
  b.bad_point = reinterpret_cast<int *>(a.out + SPFE_LBA_APPLY_OFF_BAD_POINT);
  b.obs_start = reinterpret_cast<int *>(a.out + SPFE_LBA_APPLY_OFF_OBS_START(a.bad_cap));
  b.obs = reinterpret_cast<int *>(a.out + SPFE_LBA_APPLY_OFF_OBS(a.point_cap, a.bad_cap));
  b.ref_slot = reinterpret_cast<int *>(a.out + SPFE_LBA_APPLY_OFF_REF_SLOT(a.point_cap, a.edge_cap, a.bad_cap));
  return b;
}
}  // namespace

__global__ __launch_bounds__(LB_WG) void lba_apply_preset(LbaApplyArgs a) {
  const AScratch sc = a_scratch(a.scratch, a.point_cap, a.edge_cap);
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
  zero_block(a.out, SPFE_LBA_APPLY_BYTES(a.point_cap, a.edge_cap, a.bad_cap), tid, nth);
  for (size_t e = tid; e < (size_t)a.edge_cap; e += nth) sc.mark[e] = 0;
  for (size_t i = tid; i < (size_t)a.point_cap; i += nth) {
    sc.went_bad[i] = 0;
    sc.rem[i] = 0;
  }
  if (tid < (size_t)A_INTS) sc.misc[tid] = 0;
}

__global__ __launch_bounds__(LB_WG) void lba_apply_mark(LbaApplyArgs a) {
  const AScratch sc = a_scratch(a.scratch, a.point_cap, a.edge_cap);
  const AView v = a_view(a);
  for (int j = blockIdx.x * LB_WG + threadIdx.x; j < v.n_erase; j += gridDim.x * LB_WG) {
    const int e = v.erase_idx[j];
    bool followed = false;
    if (spfe_lb_in_range(e, v.n_edges)) {
      const int i = v.edges[3 * (size_t)e], b = v.edges[3 * (size_t)e + 1], kp = v.edges[3 * (size_t)e + 2];
      if (spfe_lb_in_range(i, v.n) && spfe_lb_in_range(b, v.n_kf) && spfe_lb_in_range(v.point_idx[i], a.n_table)) {
        const int slot = v.kf_slot[b];
        if (a_valid_obs(a, slot, kp)) {
          int first, len;
          a_range(v, i, &first, &len);
          for (int t = first; t < first + len; ++t) {
            if (v.obs[2 * (size_t)t] == slot && v.obs[2 * (size_t)t + 1] == kp) {
              sc.mark[t] = 1;   // the same value from every entry that names it
              a.rows[(size_t)slot * a.kp_stride + kp] = -1;
              followed = true;
              break;
            }
          }
        }
      }
    }
    if (!followed) sc.misc[A_WILD] = 1;
  }
}

__global__ __launch_bounds__(LB_WG) void lba_apply_point(LbaApplyArgs a) {
  const AScratch sc = a_scratch(a.scratch, a.point_cap, a.edge_cap);
  const AView v = a_view(a);
  const ABlock blk = a_block(a);
  for (int i = blockIdx.x * LB_WG + threadIdx.x; i < v.n; i += gridDim.x * LB_WG) {
    const int p = v.point_idx[i];
    if (!spfe_lb_in_range(p, a.n_table)) {
      sc.misc[A_WILD] = 1;
      blk.ref_slot[i] = -1;
      continue;
    }
    a.xyz[3 * (size_t)p] = v.xyz_out[3 * (size_t)i];   // (A5)
    a.xyz[3 * (size_t)p + 1] = v.xyz_out[3 * (size_t)i + 1];
    a.xyz[3 * (size_t)p + 2] = v.xyz_out[3 * (size_t)i + 2];
    int first, len;
    if (!a_range(v, i, &first, &len)) sc.misc[A_WILD] = 1;
    const int ref = a.ref_slot[p];
    int k = 0, remaining = 0, least = -1, ref_hit = 0;
    for (int t = first; t < first + len; ++t) {
      const int slot = v.obs[2 * (size_t)t], kp = v.obs[2 * (size_t)t + 1];
      if (!a_valid_obs(a, slot, kp)) {
        sc.misc[A_WILD] = 1;
        continue;
      }
      if (sc.mark[t]) {
        ++k;
        ref_hit |= slot == ref;
      } else {
        if (remaining == 0) least = slot;
        ++remaining;
      }
    }
    if (k) atomicAdd(&sc.misc[A_NERASED], k);
    int ref_now = ref;
    if (spfe_lb_good(a.mp_flags[p])) {   // (A2), (A3): this thread owns nobs, flags and ref_slot of p
      const int after = a.nobs[p] - k;
      if (k) a.nobs[p] = after;
      if (spfe_lb_goes_bad(k, after)) {
        a.mp_flags[p] = (uint8_t)(a.mp_flags[p] & ~1u);
        sc.went_bad[i] = 1;
        for (int t = first; t < first + len; ++t) {
          const int slot = v.obs[2 * (size_t)t], kp = v.obs[2 * (size_t)t + 1];
          if (a_valid_obs(a, slot, kp) && !sc.mark[t]) a.rows[(size_t)slot * a.kp_stride + kp] = -1;
        }
      } else {
        sc.rem[i] = remaining;
        if (ref_hit && remaining > 0) {
          a.ref_slot[p] = ref_now = least;
          atomicAdd(&sc.misc[A_NMOVED], 1);
        }
      }
    }
    blk.ref_slot[i] = ref_now;
  }
}

__global__ __launch_bounds__(LB_ONE) void lba_apply_finish(LbaApplyArgs a) {
  __shared__ int wcnt[LB_ONE_WAVES], wt[LB_ONE_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const AScratch sc = a_scratch(a.scratch, a.point_cap, a.edge_cap);
  const AView v = a_view(a);
  const ABlock blk = a_block(a);
  int total = 0, n_bad = 0;
  for (int base = 0; base < v.n; base += LB_ONE) {   // uniform
    const int i = base + tid, c = i < v.n ? sc.rem[i] : 0;
    const bool bad = i < v.n && sc.went_bad[i];
    int tc, tb;
    const int oc = wg_ordered_offset<LB_ONE>(c, wcnt, &tc);
    const int rb = wg_ordered_rank<LB_ONE>(bad, lane, wave, wt, &tb);
    if (i < v.n) blk.obs_start[i] = total + oc;
    if (bad && n_bad + rb < a.bad_cap) blk.bad_point[n_bad + rb] = v.point_idx[i];
    total += tc;
    n_bad += tb;
    __syncthreads();
  }
  if (tid == 0) blk.obs_start[v.n] = total;
  for (int i = v.n + 1 + tid; i <= a.point_cap; i += LB_ONE) blk.obs_start[i] = -1;
  for (int i = v.n + tid; i < a.point_cap; i += LB_ONE) blk.ref_slot[i] = -1;
  const int stored = n_bad < a.bad_cap ? n_bad : a.bad_cap;
  for (int j = stored + tid; j < a.bad_cap; j += LB_ONE) blk.bad_point[j] = -1;
  if (tid < 16) {
    int x = 0;
    if (tid == SPFE_LBA_APPLY_OFF_STATUS / 4)
      x = (v.ok ? 0 : SPFE_LBA_NOT_APPLIED) | (n_bad > a.bad_cap ? SPFE_LBA_BAD_CUT : 0) | (sc.misc[A_WILD] ? SPFE_LBA_WILD : 0);
    if (tid == SPFE_LBA_APPLY_OFF_N_ERASED / 4) x = sc.misc[A_NERASED];
    if (tid == SPFE_LBA_APPLY_OFF_N_BAD / 4) x = n_bad;
    if (tid == SPFE_LBA_APPLY_OFF_N_BAD_STORED / 4) x = stored;
    if (tid == SPFE_LBA_APPLY_OFF_N_REF_MOVED / 4) x = sc.misc[A_NMOVED];
    if (tid == SPFE_LBA_APPLY_OFF_N_OBS_AFTER / 4) x = total;
    blk.hdr[tid] = x;
  }
}

__global__ __launch_bounds__(LB_WG) void lba_apply_lists(LbaApplyArgs a) {
  const AScratch sc = a_scratch(a.scratch, a.point_cap, a.edge_cap);
  const AView v = a_view(a);
  const ABlock blk = a_block(a);
  const int tid = blockIdx.x * LB_WG + threadIdx.x, nth = gridDim.x * LB_WG;
  for (int i = tid; i < v.n; i += nth) {
    if (sc.rem[i] == 0) continue;
    int first, len, at = blk.obs_start[i];
    a_range(v, i, &first, &len);
    for (int t = first; t < first + len; ++t) {
      const int slot = v.obs[2 * (size_t)t], kp = v.obs[2 * (size_t)t + 1];
      if (!a_valid_obs(a, slot, kp) || sc.mark[t]) continue;
      blk.obs[2 * (size_t)at] = slot;
      blk.obs[2 * (size_t)at + 1] = kp;
      ++at;
    }
  }
  const int n_after = blk.hdr[SPFE_LBA_APPLY_OFF_N_OBS_AFTER / 4];
  for (size_t t = 2 * (size_t)n_after + tid; t < 2 * (size_t)a.edge_cap; t += nth) blk.obs[t] = -1;
  for (int t = tid; t < v.n_local * 16; t += nth) {   // (A4)
    const int slot = v.kf_slot[t >> 4];
    if (spfe_lb_in_range(slot, a.n_slots)) a.Tcw[(size_t)slot * 16 + (t & 15)] = v.Tcw_out[t];
  }
}

size_t lba_gather_scratch_bytes(int n_table, int n_slots, int point_cap, int edge_cap) {
  return pad16(4 * (size_t)n_table) * 2 + pad16(4 * (size_t)n_slots) * 3 + pad16(4 * (size_t)point_cap) * 4 + pad16(16 * (size_t)edge_cap) +
         pad16(8 * (size_t)edge_cap) + pad16(4 * (size_t)G_INTS);
}
size_t lba_apply_scratch_bytes(int point_cap, int edge_cap) {
  return pad16((size_t)edge_cap) + pad16((size_t)point_cap) + pad16(4 * (size_t)point_cap) + pad16(4 * (size_t)A_INTS);
}

hipError_t launch_lba_gather(const LbaGatherArgs &a, hipStream_t s) {
  if (a.n_table < 1 || a.n_slots < 1 || a.kp_stride < 1 || a.conn_cap < 1 || a.cur_slot < 0 || a.cur_slot >= a.n_slots || a.kf_cap < 1 ||
      a.kf_cap > SPFE_BA_MAX_KEYFRAMES || a.free_cap < 1 || a.point_cap < 1 || a.edge_cap < 1 || !a.out || !a.scratch)
    return hipErrorInvalidValue;
  const size_t block = SPFE_LBA_GATHER_BYTES(a.kf_cap, a.point_cap, a.edge_cap);
  const size_t preset = std::max(std::max((size_t)a.n_table, (size_t)a.n_slots), std::max((size_t)a.point_cap, block / 16));
  const unsigned rows = groups_for((size_t)a.n_slots, LB_WG / 64, LB_GRID);
  hipLaunchKernelGGL(lba_preset_kernel, dim3(groups_for(preset, LB_WG, LB_GRID)), dim3(LB_WG), 0, s, a);
  hipLaunchKernelGGL(lba_local_kernel, dim3(1), dim3(LB_ONE), 0, s, a);
  hipLaunchKernelGGL(lba_first_kernel, dim3(groups_for((size_t)a.kf_cap * a.kp_stride, LB_WG, LB_GRID)), dim3(LB_WG), 0, s, a);
  hipLaunchKernelGGL(lba_points_kernel, dim3(1), dim3(LB_ONE), 0, s, a);
  hipLaunchKernelGGL(lba_scan_kernel, dim3(rows), dim3(LB_WG), 0, s, a);
  hipLaunchKernelGGL(lba_fixed_kernel, dim3(groups_for((size_t)a.n_slots, LB_WG, LB_GRID)), dim3(LB_WG), 0, s, a);
  hipLaunchKernelGGL(lba_ecount_kernel, dim3(groups_for((size_t)a.edge_cap, LB_WG, LB_GRID)), dim3(LB_WG), 0, s, a);
  hipLaunchKernelGGL(lba_place_kernel, dim3(1), dim3(LB_ONE), 0, s, a);
  hipLaunchKernelGGL(lba_scatter_kernel, dim3(groups_for((size_t)a.edge_cap, LB_WG, LB_GRID)), dim3(LB_WG), 0, s, a);
  hipLaunchKernelGGL(lba_order_kernel, dim3(groups_for((size_t)a.point_cap, LB_WG / 64, LB_GRID)), dim3(LB_WG), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_lba_apply(const LbaApplyArgs &a, hipStream_t s) {
  if (a.n_table < 1 || a.n_slots < 1 || a.kp_stride < 1 || a.kf_cap < 1 || a.kf_cap > SPFE_BA_MAX_KEYFRAMES || a.point_cap < 1 ||
      a.edge_cap < 1 || a.bad_cap < 0 || !a.out || !a.scratch || !a.gather || !a.ba)
    return hipErrorInvalidValue;
  const size_t block = SPFE_LBA_APPLY_BYTES(a.point_cap, a.edge_cap, a.bad_cap);
  const size_t preset = std::max(std::max((size_t)a.edge_cap, (size_t)a.point_cap), block / 16);
  hipLaunchKernelGGL(lba_apply_preset, dim3(groups_for(preset, LB_WG, LB_GRID)), dim3(LB_WG), 0, s, a);
  hipLaunchKernelGGL(lba_apply_mark, dim3(groups_for((size_t)a.edge_cap, LB_WG, LB_GRID)), dim3(LB_WG), 0, s, a);
  hipLaunchKernelGGL(lba_apply_point, dim3(groups_for((size_t)a.point_cap, LB_WG, LB_GRID)), dim3(LB_WG), 0, s, a);
  hipLaunchKernelGGL(lba_apply_finish, dim3(1), dim3(LB_ONE), 0, s, a);
  hipLaunchKernelGGL(lba_apply_lists, dim3(groups_for(std::max((size_t)a.point_cap, 2 * (size_t)a.edge_cap), LB_WG, LB_GRID)), dim3(LB_WG), 0, s, a);
  return hipGetLastError();
}

}  // namespace spfe
