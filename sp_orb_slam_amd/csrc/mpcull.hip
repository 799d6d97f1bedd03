// mpcull.hip — map-point culling on the device (local_mapper.cpp:281-310) with the resident state it reads: the found / visible
// counters of a map point, the recent list with each point's first keyframe id, and the admission of the points
// spfe_create_map_points_record_device leaves in its blocks into the rows and the table.  The contract is
// include/spfe_mpcull_math.h (integers and one f32 division); the host statement the tests hold these kernels to is
// tests/mpcull_ref/mpcull_ref.c: state, rows, table, list and the blocks are equal byte for byte.
//
// The launches, whatever the sizes are:
//   reset      mp_reset_kernel    multi-workgroup: the preset of a row range and of the list.
//   admission  mp_admit_kernel    multi-workgroup: EVERY workgroup reads the <= 32 block headers, derives the prefix offsets and makes
//                                 the whole all-or-nothing test itself (so the verdict is uniform and nobody waits for anybody), then
//                                 writes its share of the points with plain vector stores.  It reads d_recent_n and does not write it.
//              mp_admit_finish    ONE small workgroup: the displaced count summed, the block, d_recent_n.
//   statistics mp_stat_kernel     multi-workgroup over keypoints and list positions: integer atomic additions (the sum does not
//                                 depend on their order); workgroup 0 also counts all items for the block, without atomics.
//   cull       mp_first_kernel    multi-workgroup: the preset of the scratch (first entry and mark per point).
//              mp_decide_kernel   multi-workgroup: a code per entry from state that no kernel of the call has written yet, and the
//                                 first entry of every culled point by atomicMin.
//              mp_compact_kernel  ONE workgroup over chunks of the list: the duplicates (an entry that is not the first of its culled
//                                 point is ERASED_BAD), the stable compaction of the kept entries and of bad_point[] by ordered ranks
//                                 with the totals carried from chunk to chunk, the flag clears, the marks, the block.
//              mp_rows_kernel     multi-workgroup: every entry that names a marked point becomes -1 in the rows of the slots that are
//                                 not bad — 16-byte loads from the row's first aligned boundary, any row pitch —; it leaves at once
//                                 when nothing was culled.
// No workgroup waits for another: the order between the kernels of a call is the launch boundary.
#include <algorithm>
#include <climits>

#include "../../include/spfe.h"
#include "../../include/spfe_mpcull_math.h"
#include "spfe_kernels.h"
#include "wave_ops.h"
#include "resident_rows.h"

namespace spfe {

namespace {
constexpr int MP_WG = 256;
constexpr int MP_GRID = 1024;
constexpr int MA_GRID = 64;          // workgroups of an admission: each repeats the test, so few
constexpr int MC_WG = 1024;          // the compaction's one workgroup: a chunk of the list
constexpr int MC_WAVES = MC_WG / 64;
constexpr int MP_FIRST_NONE = INT_MAX;
// the admission's verdict in the scratch, behind first[] and mark[]: int32 fields
constexpr int MA_STATUS = 0, MA_NEEDED = 1, MA_BEFORE = 2, MA_TOTAL = 3, MA_CNT = 4, MA_DISPLACED = 64, MA_INTS = MA_DISPLACED + MA_GRID;

struct MpScratch {
  int *first;       // [n_table] the least list index that names a culled point
  uint8_t *mark;    // [n_table] 1: culled in this call
  int *misc;        // [MA_INTS]
};
__host__ __device__ inline MpScratch mp_scratch(uint8_t *base, int n_table) {
  MpScratch s;
  s.first = reinterpret_cast<int *>(base);
  base += pad16(4 * (size_t)n_table);
  s.mark = base;
  base += pad16((size_t)n_table);
  s.misc = reinterpret_cast<int *>(base);
  return s;
}
__device__ __forceinline__ const int *tri_i32(const uint8_t *blk, size_t off) { return reinterpret_cast<const int *>(blk + off); }
}  // namespace

__global__ __launch_bounds__(MP_WG) void mp_reset_kernel(MpLife l, int first_row, int n_rows, int reset_list) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < (size_t)n_rows; i += nth) {
    const size_t p = (size_t)first_row + i;
    l.flags[p] = 0;
    l.nobs[p] = 0;
    l.found[p] = 0;
    l.visible[p] = 0;
    l.first_kf[p] = -1;
  }
  if (reset_list) {
    for (size_t e = tid; e < (size_t)l.recent_cap; e += nth) l.recent[e] = -1;
    if (tid == 0) *l.recent_n = 0;
  }
}

// ---- (A) --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MP_WG) void mp_admit_kernel(MpAdmitArgs a) {
  __shared__ int cnt[SPFE_TRI_MAX_NEIGHBOURS], base[SPFE_TRI_MAX_NEIGHBOURS], slot[SPFE_TRI_MAX_NEIGHBOURS];
  __shared__ int off[SPFE_TRI_MAX_NEIGHBOURS + 1], contrib[SPFE_TRI_MAX_NEIGHBOURS];
  __shared__ int sh_status, sh_disp;
  __shared__ long long sh_needed;
  const int tid = threadIdx.x;
  int *misc = mp_scratch(a.scratch, a.life.n_table).misc;
  const int n_before = clamp_int(*a.life.recent_n, 0, a.life.recent_cap);   // written by mp_admit_finish only
  // (A1) the headers; a refused block's status alone is read
  if (tid < SPFE_TRI_MAX_NEIGHBOURS) {
    int c = 0, b = 0, s = -1, used = 0;
    if (tid < a.n_neigh) {
      const uint8_t *blk = a.tri + (size_t)tid * a.tri_stride;
      if (*tri_i32(blk, SPFE_TRI_OFF_STATUS) == 0) {
        c = *tri_i32(blk, SPFE_TRI_OFF_N_NEW);
        b = *tri_i32(blk, SPFE_TRI_OFF_POINT_BASE);
        s = a.neigh_slot[tid];
        used = 1;
      }
    }
    cnt[tid] = c;
    base[tid] = b;
    slot[tid] = s;
    contrib[tid] = used;
  }
  if (tid == 0) sh_disp = 0;
  __syncthreads();
  // (A2) the headers' part and the prefix offsets, by one thread: 32 blocks
  if (tid == 0) {
    int bad = 0;
    long long total = 0;
    off[0] = 0;
    for (int j = 0; j < SPFE_TRI_MAX_NEIGHBOURS; ++j) {
      if (contrib[j]) {
        if (spfe_mc_block_bad(cnt[j], base[j], slot[j], a.cur_slot, a.kmax, a.n_slots, a.life.n_table)) bad = 1;
        for (int i = 0; i < j; ++i) bad |= contrib[i] && slot[i] == slot[j];
        if (cnt[j] >= 0 && cnt[j] <= a.kmax) total += cnt[j];
      }
      off[j + 1] = (int)(total < INT_MAX ? total : INT_MAX);
    }
    sh_needed = (long long)n_before + total;
    sh_status = (bad ? SPFE_ADMIT_BAD_RANGE : 0) | (sh_needed > a.life.recent_cap ? SPFE_ADMIT_RECENT_OVERFLOW : 0);
  }
  __syncthreads();
  const int total = off[SPFE_TRI_MAX_NEIGHBOURS];
  int status = sh_status;
  // ... and the keypoints' part, by the whole workgroup, when the counts can be trusted
  int bad_k = 0;
  if (!(status & SPFE_ADMIT_BAD_RANGE)) {
    for (int j = 0; j < a.n_neigh; ++j) {   // uniform
      const int c = off[j + 1] - off[j];
      const uint8_t *blk = a.tri + (size_t)j * a.tri_stride;
      const int *k1 = tri_i32(blk, SPFE_TRI_OFF_NEW_K1(a.kmax)), *k2 = tri_i32(blk, SPFE_TRI_OFF_NEW_K2(a.kmax));
      for (int t = tid; t < c; t += MP_WG) bad_k |= !spfe_mc_kp_in_range(k1[t], a.kp_stride) || !spfe_mc_kp_in_range(k2[t], a.kp_stride);
    }
  }
  if (__syncthreads_or(bad_k)) status |= SPFE_ADMIT_BAD_RANGE;
  const bool refused = (status & (SPFE_ADMIT_BAD_RANGE | SPFE_ADMIT_RECENT_OVERFLOW)) != 0;
  if (blockIdx.x == 0) {
    if (tid == 0) {
      misc[MA_STATUS] = status;
      misc[MA_NEEDED] = (int)(sh_needed < INT_MAX ? sh_needed : INT_MAX);
      misc[MA_BEFORE] = n_before;
      misc[MA_TOTAL] = refused ? 0 : total;
    }
    if (tid < SPFE_TRI_MAX_NEIGHBOURS) misc[MA_CNT + tid] = refused ? 0 : off[tid + 1] - off[tid];
  }
  if (refused) {   // uniform over the grid: every workgroup made the same test on the same bytes
    if (tid == 0) misc[MA_DISPLACED + blockIdx.x] = 0;
    return;
  }
  // (A3) this workgroup's share
  int disp = 0;
  for (int i = blockIdx.x * MP_WG + tid; i < total; i += gridDim.x * MP_WG) {
    int j = 0;
    while (off[j + 1] <= i) ++j;   // <= 32 steps; blocks of count 0 are passed over
    const int t = i - off[j], p = base[j] + t;
    const uint8_t *blk = a.tri + (size_t)j * a.tri_stride;
    const int k1 = tri_i32(blk, SPFE_TRI_OFF_NEW_K1(a.kmax))[t], k2 = tri_i32(blk, SPFE_TRI_OFF_NEW_K2(a.kmax))[t];
    const float *x = reinterpret_cast<const float *>(blk + SPFE_TRI_OFF_NEW_XYZ(a.kmax)) + 3 * (size_t)t;
    int *e1 = a.rows + (size_t)a.cur_slot * a.kp_stride + k1, *e2 = a.rows + (size_t)slot[j] * a.kp_stride + k2;
    disp += (*e1 != -1) + (*e2 != -1);
    *e1 = p;
    *e2 = p;
    a.xyz[3 * (size_t)p] = x[0];
    a.xyz[3 * (size_t)p + 1] = x[1];
    a.xyz[3 * (size_t)p + 2] = x[2];
    a.life.nobs[p] = 2;
    a.life.found[p] = 1;
    a.life.visible[p] = 1;
    a.life.first_kf[p] = a.cur_kf_id;
    a.life.flags[p] = (uint8_t)(SPFE_PROJ_SEARCHABLE | SPFE_PROJ_OBSERVED);
    a.life.recent[n_before + i] = p;
  }
  disp = wave_sum(disp);
  if ((tid & 63) == 0 && disp) atomicAdd(&sh_disp, disp);   // LDS, integers
  __syncthreads();
  if (tid == 0) misc[MA_DISPLACED + blockIdx.x] = sh_disp;
}

__global__ __launch_bounds__(64) void mp_admit_finish(MpAdmitArgs a, int grid) {
  const int tid = threadIdx.x;
  const int *misc = mp_scratch(a.scratch, a.life.n_table).misc;
  int *out = reinterpret_cast<int *>(a.out);
  int d = 0;
  for (int g = tid; g < grid; g += 64) d += misc[MA_DISPLACED + g];
  d = wave_sum(d);
  const int status = misc[MA_STATUS], total = misc[MA_TOTAL], before = misc[MA_BEFORE];
  int v = 0;
  if (tid == SPFE_ADMIT_OFF_STATUS / 4) v = status | (d ? SPFE_ADMIT_DISPLACED : 0);
  if (tid == SPFE_ADMIT_OFF_N_ADMITTED / 4) v = total;
  if (tid == SPFE_ADMIT_OFF_N_RECENT_BEFORE / 4) v = before;
  if (tid == SPFE_ADMIT_OFF_N_RECENT_AFTER / 4) v = before + total;
  if (tid == SPFE_ADMIT_OFF_N_DISPLACED / 4) v = d;
  if (tid == SPFE_ADMIT_OFF_N_NEEDED / 4) v = misc[MA_NEEDED];
  if (tid >= SPFE_ADMIT_OFF_ADMITTED / 4 && tid < SPFE_ADMIT_OFF_ADMITTED / 4 + SPFE_TRI_MAX_NEIGHBOURS)
    v = misc[MA_CNT + tid - SPFE_ADMIT_OFF_ADMITTED / 4];
  out[tid] = v;   // 64 int32 = SPFE_ADMIT_OUT_BYTES
  if (tid == 0 && total > 0) *a.life.recent_n = before + total;
}
static_assert(SPFE_ADMIT_OUT_BYTES == 64 * 4 && SPFE_ADMIT_OFF_ADMITTED / 4 + SPFE_TRI_MAX_NEIGHBOURS <= 64, "the block is one wavefront's");

// ---- (B) --------------------------------------------------------------------------------------------------------------------------
// item i: a keypoint (i < n_kp: (B1) and (B3)) or a list position (i - n_kp: (B2)); the counts it adds, and with ADD the additions
template <bool ADD>
__device__ __forceinline__ void mp_stat_item(const MpStatArgs &a, int i, int *held, int *view, int *found) {
  const int nt = a.life.n_table;
  if (i < a.n_kp) {
    const int r = a.entry[i], q = a.after[i];
    if (spfe_mc_in_range(r, nt) && spfe_mc_good(a.life.flags[r])) {
      ++*held;
      if (ADD) atomicAdd(&a.life.visible[r], 1);
    }
    if (spfe_mc_in_range(q, nt) && a.outlier[i] == 0) {
      ++*found;
      if (ADD) atomicAdd(&a.life.found[q], 1);
    }
  } else {
    const int pos = i - a.n_kp;
    if (a.in_view[pos] != 0) {
      const int r = a.point_idx[pos];
      if (spfe_mc_in_range(r, nt)) {
        ++*view;
        if (ADD) atomicAdd(&a.life.visible[r], 1);
      }
    }
  }
}

__global__ __launch_bounds__(MP_WG) void mp_stat_kernel(MpStatArgs a) {
  __shared__ int sums[3];
  const int tid = threadIdx.x, n = a.n_kp + a.point_cap;
  int held = 0, view = 0, found = 0;
  for (int i = blockIdx.x * MP_WG + tid; i < n; i += gridDim.x * MP_WG) mp_stat_item<true>(a, i, &held, &view, &found);
  if (blockIdx.x != 0) return;
  // the block: workgroup 0 counts every item itself (flags are not written here, so the counts are the additions made)
  held = view = found = 0;
  if (tid < 3) sums[tid] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += MP_WG) mp_stat_item<false>(a, i, &held, &view, &found);
  held = wave_sum(held);
  view = wave_sum(view);
  found = wave_sum(found);
  if ((tid & 63) == 0) {
    atomicAdd(&sums[0], held);
    atomicAdd(&sums[1], view);
    atomicAdd(&sums[2], found);
  }
  __syncthreads();
  int *out = reinterpret_cast<int *>(a.out);
  for (int i = tid; i < SPFE_MPSTAT_OUT_BYTES / 4; i += MP_WG) out[i] = i < 3 ? sums[i] : 0;
}
static_assert(SPFE_MPSTAT_OFF_N_VISIBLE_HELD == 0 && SPFE_MPSTAT_OFF_N_VISIBLE_VIEW == 4 && SPFE_MPSTAT_OFF_N_FOUND == 8, "sums[] order");

// ---- (C) --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MP_WG) void mp_first_kernel(MpCullArgs a) {
  const MpScratch sc = mp_scratch(a.scratch, a.life.n_table);
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
  for (size_t p = tid; p < (size_t)a.life.n_table; p += nth) {
    sc.first[p] = MP_FIRST_NONE;
    sc.mark[p] = 0;
  }
}

__global__ __launch_bounds__(MP_WG) void mp_decide_kernel(MpCullArgs a) {
  const MpScratch sc = mp_scratch(a.scratch, a.life.n_table);
  const MpLife &l = a.life;
  int *e_point = reinterpret_cast<int *>(a.out + SPFE_MPCULL_OFF_ENTRY_POINT), *e_code = reinterpret_cast<int *>(a.out + SPFE_MPCULL_OFF_ENTRY_CODE(l.recent_cap));
  const int n = clamp_int(*l.recent_n, 0, l.recent_cap);   // rewritten by mp_compact_kernel only
  for (int e = blockIdx.x * MP_WG + threadIdx.x; e < l.recent_cap; e += gridDim.x * MP_WG) {
    int p = -1, code = -1;
    if (e < n) {
      p = l.recent[e];
      if (!spfe_mc_in_range(p, l.n_table)) {
        code = SPFE_MPCULL_CODE_WILD;
      } else if (!spfe_mc_good(l.flags[p])) {   // flags are cleared behind this kernel: this is the state at entry
        code = SPFE_MPCULL_CODE_ERASED_BAD;
      } else {
        code = spfe_mc_rule(l.found[p], l.visible[p], l.first_kf[p], l.nobs[p], a.cur_kf_id, a.th_obs, a.found_ratio);
        if (spfe_mc_culls(code)) atomicMin(&sc.first[p], e);
      }
    }
    e_point[e] = p;
    e_code[e] = code;
  }
}

__global__ __launch_bounds__(MC_WG) void mp_compact_kernel(MpCullArgs a) {
  __shared__ int wt_keep[MC_WAVES], wt_bad[MC_WAVES];
  __shared__ int wsum[MC_WAVES][6];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const MpScratch sc = mp_scratch(a.scratch, a.life.n_table);
  const MpLife &l = a.life;
  const int cap = l.recent_cap;
  int *hdr = reinterpret_cast<int *>(a.out);
  const int *e_point = reinterpret_cast<const int *>(a.out + SPFE_MPCULL_OFF_ENTRY_POINT);
  int *e_code = reinterpret_cast<int *>(a.out + SPFE_MPCULL_OFF_ENTRY_CODE(cap));
  int *bad_point = reinterpret_cast<int *>(a.out + SPFE_MPCULL_OFF_BAD_POINT(cap));
  const int n = clamp_int(*l.recent_n, 0, cap);
  int kept = 0, n_bad = 0;
  int c[6] = {0, 0, 0, 0, 0, 0};
  for (int base = 0; base < n; base += MC_WG) {   // uniform
    const int e = base + tid;
    int p = -1, code = -1;
    if (e < n) {
      p = e_point[e];
      code = e_code[e];
      if (spfe_mc_culls(code) && sc.first[p] != e) {   // (C2): an earlier entry culls this point
        code = SPFE_MPCULL_CODE_ERASED_BAD;
        e_code[e] = code;
      }
#pragma unroll
      for (int k = 0; k < 6; ++k) c[k] += code == k;
    }
    const bool keep = code == SPFE_MPCULL_CODE_KEPT, bad = spfe_mc_culls(code);
    int tk, tb;
    const int rk = wg_ordered_rank<MC_WG>(keep, lane, wave, wt_keep, &tk);
    const int rb = wg_ordered_rank<MC_WG>(bad, lane, wave, wt_bad, &tb);
    if (keep) l.recent[kept + rk] = p;   // kept + rk <= e, and p was read from the block: no entry is read after it is written
    if (bad) {                           // the first entry of p, and the only one with a culling code: one writer a point
      l.flags[p] = (uint8_t)(l.flags[p] & ~SPFE_PROJ_SEARCHABLE);
      sc.mark[p] = 1;
      if (n_bad + rb < a.bad_cap) bad_point[n_bad + rb] = p;
    }
    kept += tk;
    n_bad += tb;
    __syncthreads();   // the wavefront totals are rewritten by the next chunk
  }
  // the tails and the block
  for (int e = kept + tid; e < n; e += MC_WG) l.recent[e] = -1;
  const int stored = n_bad < a.bad_cap ? n_bad : a.bad_cap;
  for (int j = stored + tid; j < a.bad_cap; j += MC_WG) bad_point[j] = -1;
  {
    const size_t end = SPFE_MPCULL_OFF_BAD_POINT(cap) + 4 * (size_t)a.bad_cap, all = SPFE_MPCULL_OUT_BYTES(cap, a.bad_cap);
    for (size_t b = end + tid; b < all; b += MC_WG) a.out[b] = 0;
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int s = wave_sum(c[k]);
    if (lane == 0) wsum[wave][k] = s;
  }
  __syncthreads();   // also: every thread has read *recent_n
  if (tid < 16) {
    int t[6] = {0, 0, 0, 0, 0, 0};
    for (int w = 0; w < MC_WAVES; ++w)
      for (int k = 0; k < 6; ++k) t[k] += wsum[w][k];
    int v = 0;
    if (tid == SPFE_MPCULL_OFF_STATUS / 4)
      v = (n_bad > a.bad_cap ? SPFE_MPCULL_BAD_CUT : 0) | (t[SPFE_MPCULL_CODE_WILD] ? SPFE_MPCULL_WILD_ENTRY : 0);
    if (tid == SPFE_MPCULL_OFF_N_LISTED / 4) v = n;
    if (tid == SPFE_MPCULL_OFF_N_KEPT / 4) v = kept;
    if (tid == SPFE_MPCULL_OFF_N_CULLED_RATIO / 4) v = t[SPFE_MPCULL_CODE_CULLED_RATIO];
    if (tid == SPFE_MPCULL_OFF_N_CULLED_OBS / 4) v = t[SPFE_MPCULL_CODE_CULLED_OBS];
    if (tid == SPFE_MPCULL_OFF_N_RETIRED / 4) v = t[SPFE_MPCULL_CODE_RETIRED];
    if (tid == SPFE_MPCULL_OFF_N_ERASED_BAD / 4) v = t[SPFE_MPCULL_CODE_ERASED_BAD];
    if (tid == SPFE_MPCULL_OFF_N_WILD / 4) v = t[SPFE_MPCULL_CODE_WILD];
    if (tid == SPFE_MPCULL_OFF_N_BAD / 4) v = n_bad;
    if (tid == SPFE_MPCULL_OFF_N_BAD_STORED / 4) v = stored;
    hdr[tid] = v;
  }
  if (tid == 0) *l.recent_n = kept;
}

__global__ __launch_bounds__(MP_WG) void mp_rows_kernel(MpCullArgs a) {
  if (reinterpret_cast<const int *>(a.out)[SPFE_MPCULL_OFF_N_BAD / 4] == 0) return;
  const uint8_t *mark = mp_scratch(a.scratch, a.life.n_table).mark;
  const int nt = a.life.n_table, stride = a.kp_stride, tid = threadIdx.x;
  for (int s = blockIdx.x; s < a.n_slots; s += gridDim.x) {
    if (a.kf_flags[s] & 1u) continue;
    int *row = a.rows + (size_t)s * stride;
    row_walk<MP_WG>(row, stride, tid, [&](int k, int p) {
      if (spfe_mc_in_range(p, nt) && mark[p]) row[k] = -1;
    });
  }
}

size_t mpcull_scratch_bytes(int n_table) { return pad16(4 * (size_t)n_table) + pad16((size_t)n_table) + pad16(4 * (size_t)MA_INTS); }

namespace {
bool life_ok(const MpLife &l) {
  return l.n_table >= 1 && l.n_table <= SPFE_MP_MAX_POINTS && l.recent_cap >= 1 && l.recent_cap <= SPFE_MP_MAX_POINTS;
}
}  // namespace

hipError_t launch_mp_life_reset(const MpLife &l, int first_row, int n_rows, int reset_list, hipStream_t s) {
  if (!life_ok(l) || first_row < 0 || n_rows < 0 || (long long)first_row + n_rows > l.n_table) return hipErrorInvalidValue;
  const size_t work = std::max((size_t)n_rows, reset_list ? (size_t)l.recent_cap : (size_t)0);
  hipLaunchKernelGGL(mp_reset_kernel, dim3(groups_for(work, MP_WG, MP_GRID)), dim3(MP_WG), 0, s, l, first_row, n_rows, reset_list);
  return hipGetLastError();
}

hipError_t launch_mp_admit(const MpAdmitArgs &a, hipStream_t s) {
  if (!life_ok(a.life) || a.n_neigh < 1 || a.n_neigh > SPFE_TRI_MAX_NEIGHBOURS || a.kmax < 1 || a.kp_stride < 1 || a.n_slots < 1 ||
      a.cur_slot < 0 || a.cur_slot >= a.n_slots || !a.out || !a.scratch)
    return hipErrorInvalidValue;
  const int grid = (int)groups_for((size_t)a.n_neigh * a.kmax, MP_WG, MA_GRID);
  hipLaunchKernelGGL(mp_admit_kernel, dim3((unsigned)grid), dim3(MP_WG), 0, s, a);
  hipLaunchKernelGGL(mp_admit_finish, dim3(1), dim3(64), 0, s, a, grid);
  return hipGetLastError();
}

hipError_t launch_mp_stat(const MpStatArgs &a, hipStream_t s) {
  if (!life_ok(a.life) || a.n_kp < 0 || a.n_kp > SPFE_PROJ_MAX_POINTS || a.point_cap < 1 || a.point_cap > SPFE_PROJ_MAX_POINTS || !a.out)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(mp_stat_kernel, dim3(groups_for((size_t)a.n_kp + a.point_cap, MP_WG, MP_GRID)), dim3(MP_WG), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_mp_cull(const MpCullArgs &a, hipStream_t s) {
  if (!life_ok(a.life) || a.kp_stride < 1 || a.n_slots < 1 || a.th_obs < 0 || a.bad_cap < 0 || !a.out || !a.scratch)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(mp_first_kernel, dim3(groups_for((size_t)a.life.n_table, MP_WG, MP_GRID)), dim3(MP_WG), 0, s, a);
  hipLaunchKernelGGL(mp_decide_kernel, dim3(groups_for((size_t)a.life.recent_cap, MP_WG, MP_GRID)), dim3(MP_WG), 0, s, a);
  hipLaunchKernelGGL(mp_compact_kernel, dim3(1), dim3(MC_WG), 0, s, a);
  hipLaunchKernelGGL(mp_rows_kernel, dim3(groups_for((size_t)a.n_slots, 1, MP_GRID)), dim3(MP_WG), 0, s, a);
  return hipGetLastError();
}

}  // namespace spfe
