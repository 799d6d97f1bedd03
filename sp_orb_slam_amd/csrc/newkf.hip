// newkf.hip — a new keyframe on resident state: the insertion of its row (local_mapper.cpp:255-272 without the refresh) and the
// observation lists every map-point refresh takes, from one scan of the rows.  The contract is include/spfe_newkf_math.h (integers
// and copied bytes); the host statement the tests hold these kernels to is tests/newkf_ref/newkf_ref.c: the blocks and every edited
// array are equal byte for byte.
//
// The launches, whatever the sizes are:
//   insertion  nk_preset_kernel   multi-workgroup: the first keypoint per point preset.
//              nk_first_kernel    multi-workgroup: the least keypoint that names a good point, by atomicMin.
//              nk_insert_kernel   ONE workgroup: the row of cur_slot tested, a code per keypoint and the counts (pass 1), the verdict,
//                                 then the row, nobs (integer atomicAdd: two keypoints may name one point), the flags (the ADDED
//                                 keypoint is the one writer of its point's), the list by ordered ranks, added_point[], the block.
//              nk_desc_kernel     multi-workgroup, a wavefront an ADDED keypoint: its record row into desc_track; leaves at once
//                                 without the two arrays.
//   listing    lo_preset_kernel   multi-workgroup: the first-entry map over n_table, the counts.
//              lo_first_kernel    multi-workgroup: the first entry of every listed point by atomicMin.
//              lo_scan_kernel     multi-workgroup, a wavefront a row of ALL slots that are not bad, 16-byte loads from the row's first
//                                 aligned boundary: a hit is an entry whose point is listed; counts per entry by atomicAdd, the hits
//                                 appended to an unordered list (a wavefront claims its places with one atomicAdd).
//              lo_place_kernel    ONE workgroup over chunks of the list: the codes, the prefix sum, point_idx[], obs_start[],
//                                 ref_slot[], the header, the zeros between the arrays.
//              lo_scatter_kernel  multi-workgroup, a thread a hit: into its entry's range, in any order.
//              lo_order_kernel    multi-workgroup: the place of every observation of a range by counting smaller (slot, keypoint)
//                                 keys — exact for any count, and independent of the scatter's order —, a wavefront a range of at most
//                                 LO_WAVE_MAX, the workgroup a larger one; the -1 tail of obs[].
// No workgroup waits for another: the order between the kernels of a call is the launch boundary.
#include <algorithm>
#include <climits>

#include "../../include/spfe.h"
#include "../../include/spfe_newkf_math.h"
#include "spfe_kernels.h"
#include "wave_ops.h"
#include "resident_rows.h"

namespace spfe {

namespace {
constexpr int NK_WG = 256;
constexpr int NK_WAVES = NK_WG / 64;
constexpr int NK_GRID = 1024;
constexpr int NK_ONE = 1024;            // the one-workgroup kernels
constexpr int NK_ONE_WAVES = NK_ONE / 64;
constexpr int NK_NONE = INT_MAX;
constexpr int LO_WAVE_MAX = 256;        // the largest range a wavefront orders
constexpr int L_NHITS = 0, L_INTS = 16; // misc[] of the listing

__device__ __forceinline__ int *blk_i32(uint8_t *out, size_t off) { return reinterpret_cast<int *>(out + off); }
__device__ __forceinline__ void zero_bytes(uint8_t *out, size_t from, size_t to, int tid, int nth) {
  for (size_t b = from + tid; b < to; b += nth) out[b] = 0;
}

struct LScratch {
  int *rank;                   // [n_table] the least list entry that names the point
  int *cnt, *fill;             // [m]
  int4 *hits;                  // [obs_cap] (entry, slot, keypoint, 0), unordered
  unsigned long long *placed;  // [obs_cap] obs keys, an entry's range unordered
  int *misc;
};
__host__ __device__ inline LScratch l_scratch(uint8_t *b, int n_table, int m, int obs_cap) {
  LScratch s;
  auto take = [&b](size_t bytes) { uint8_t *p = b; b += pad16(bytes); return p; };
  s.rank = reinterpret_cast<int *>(take(4 * (size_t)n_table));
  s.cnt = reinterpret_cast<int *>(take(4 * (size_t)m));
  s.fill = reinterpret_cast<int *>(take(4 * (size_t)m));
  s.hits = reinterpret_cast<int4 *>(take(16 * (size_t)obs_cap));
  s.placed = reinterpret_cast<unsigned long long *>(take(8 * (size_t)obs_cap));
  s.misc = reinterpret_cast<int *>(take(4 * (size_t)L_INTS));
  return s;
}
__device__ __forceinline__ LScratch l_scratch(const ListObsArgs &a) { return l_scratch(a.scratch, a.n_table, a.m, a.obs_cap); }
}  // namespace

// ---- (I) --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NK_WG) void nk_preset_kernel(NewKfArgs a) {
  int *first = reinterpret_cast<int *>(a.scratch);
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
  for (size_t p = tid; p < (size_t)a.life.n_table; p += nth) first[p] = NK_NONE;
}

__global__ __launch_bounds__(NK_WG) void nk_first_kernel(NewKfArgs a) {
  int *first = reinterpret_cast<int *>(a.scratch);
  for (int i = blockIdx.x * NK_WG + threadIdx.x; i < a.n_kp; i += gridDim.x * NK_WG) {
    const int p = a.frame[i];
    if (spfe_nk_precode(p, a.life.n_table) < 0 && (a.life.flags[p] & SPFE_PROJ_SEARCHABLE)) atomicMin(&first[p], i);
  }
}

__global__ __launch_bounds__(NK_ONE) void nk_insert_kernel(NewKfArgs a) {
  __shared__ int wt[NK_ONE_WAVES];
  __shared__ int wsum[NK_ONE_WAVES][5];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const MpLife &l = a.life;
  const int *first = reinterpret_cast<const int *>(a.scratch);
  int *hdr = blk_i32(a.out, 0), *e_code = blk_i32(a.out, SPFE_NEWKF_OFF_CODE), *added = blk_i32(a.out, SPFE_NEWKF_OFF_ADDED_POINT(a.n_kp));
  int *row = a.rows + (size_t)a.cur_slot * a.kp_stride;
  const int n_before = clamp_int(*l.recent_n, 0, l.recent_cap);   // rewritten at the end of this kernel only
  // (I2) the row
  int used = 0;
  for (int k = tid; k < a.kp_stride; k += NK_ONE) used |= row[k] >= 0;
  used = __syncthreads_or(used);
  // (I1) the codes and their counts: nothing read here is written before the barrier below
  int c[5] = {0, 0, 0, 0, 0};
  for (int i = tid; i < a.n_kp; i += NK_ONE) {
    const int p = a.frame[i];
    int code = spfe_nk_precode(p, l.n_table);
    if (code < 0) code = spfe_nk_code(l.flags[p], i, first[p]);
    e_code[i] = code;
#pragma unroll
    for (int k = 0; k < 5; ++k) c[k] += code == k;
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int s = wave_sum(c[k]);
    if (lane == 0) wsum[wave][k] = s;
  }
  __syncthreads();
  int t[5] = {0, 0, 0, 0, 0};
  for (int w = 0; w < NK_ONE_WAVES; ++w)
#pragma unroll
    for (int k = 0; k < 5; ++k) t[k] += wsum[w][k];
  const int n_needed = n_before + t[SPFE_NEWKF_CODE_REPEATED];   // <= 262144 + 16384
  const int status = (used ? SPFE_NEWKF_ROW_IN_USE : 0) | ((a.kf_flags[a.cur_slot] & 1u) ? SPFE_NEWKF_BAD_SLOT : 0) |
                     (n_needed > l.recent_cap ? SPFE_NEWKF_RECENT_OVERFLOW : 0);
  const bool refused = status != 0;   // uniform
  // (I3): keypoint i is the thread's that gave it its code
  int n_rep = 0;
  for (int base = 0; base < a.n_kp; base += NK_ONE) {   // uniform
    const int i = base + tid;
    int code = -1, p = -1;
    if (i < a.n_kp) {
      code = e_code[i];
      p = a.frame[i];
    }
    const bool rep = !refused && code == SPFE_NEWKF_CODE_REPEATED;
    int tot;
    const int rk = wg_ordered_rank<NK_ONE>(rep, lane, wave, wt, &tot);
    if (i < a.n_kp) {
      added[i] = !refused && code == SPFE_NEWKF_CODE_ADDED ? p : -1;
      if (!refused) {
        const bool in_row = spfe_nk_in_row(code) != 0;
        row[i] = in_row ? p : -1;
        if (in_row) atomicAdd(&l.nobs[p], 1);
        if (code == SPFE_NEWKF_CODE_ADDED) l.flags[p] = (uint8_t)(l.flags[p] | SPFE_PROJ_OBSERVED);   // the one writer of flags[p]
        if (rep) l.recent[n_before + n_rep + rk] = p;   // < n_needed <= recent_cap
      }
    }
    n_rep += tot;
    __syncthreads();   // the wavefront totals are rewritten by the next chunk
  }
  for (int k = a.n_kp + tid; k < a.kp_stride; k += NK_ONE) {
    added[k] = -1;
    if (!refused) row[k] = -1;
  }
  zero_bytes(a.out, SPFE_NEWKF_OFF_CODE + 4 * (size_t)a.n_kp, SPFE_NEWKF_OFF_ADDED_POINT(a.n_kp), tid, NK_ONE);
  zero_bytes(a.out, SPFE_NEWKF_OFF_ADDED_POINT(a.n_kp) + 4 * (size_t)a.kp_stride, SPFE_NEWKF_OUT_BYTES(a.n_kp, a.kp_stride), tid, NK_ONE);
  if (tid < 16) {
    int v = 0;
    if (tid == SPFE_NEWKF_OFF_STATUS / 4) v = status;
    if (tid >= SPFE_NEWKF_OFF_N_NONE / 4 && tid <= SPFE_NEWKF_OFF_N_REPEATED / 4) v = t[tid - SPFE_NEWKF_OFF_N_NONE / 4];
    if (tid == SPFE_NEWKF_OFF_N_RECENT_BEFORE / 4) v = n_before;
    if (tid == SPFE_NEWKF_OFF_N_RECENT_AFTER / 4) v = refused ? n_before : n_needed;
    if (tid == SPFE_NEWKF_OFF_N_NEEDED / 4) v = n_needed;
    hdr[tid] = v;
  }
  if (tid == 0 && !refused) *l.recent_n = n_needed;   // every thread read it in front of the first barrier
}
static_assert(SPFE_NEWKF_OFF_N_NONE == 4 + 4 * SPFE_NEWKF_CODE_NONE && SPFE_NEWKF_OFF_N_REPEATED == 4 + 4 * SPFE_NEWKF_CODE_REPEATED,
              "the counts lie in code order");

__global__ __launch_bounds__(NK_WG) void nk_desc_kernel(NewKfArgs a) {
  if (!a.rec_desc || !a.desc_track) return;
  const int *added = reinterpret_cast<const int *>(a.out + SPFE_NEWKF_OFF_ADDED_POINT(a.n_kp));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = blockIdx.x * NK_WAVES + wave; i < a.n_kp; i += gridDim.x * NK_WAVES) {   // uniform over the wavefront
    const int p = added[i];
    if (!spfe_nk_in_range(p, a.life.n_table)) continue;
    float4 v;
    if (a.desc_bf16) {
      const ushort4 q = reinterpret_cast<const ushort4 *>(a.rec_desc + (size_t)i * 512)[lane];
      v = make_float4(__uint_as_float(spfe_nk_bf16_bits(q.x)), __uint_as_float(spfe_nk_bf16_bits(q.y)), __uint_as_float(spfe_nk_bf16_bits(q.z)),
                      __uint_as_float(spfe_nk_bf16_bits(q.w)));
    } else {
      v = reinterpret_cast<const float4 *>(a.rec_desc + (size_t)i * 1024)[lane];
    }
    reinterpret_cast<float4 *>(a.desc_track + (size_t)p * 256)[lane] = v;
  }
}

// ---- (O) --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NK_WG) void lo_preset_kernel(ListObsArgs a) {
  const LScratch sc = l_scratch(a);
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
  for (size_t p = tid; p < (size_t)a.n_table; p += nth) sc.rank[p] = NK_NONE;
  for (size_t i = tid; i < (size_t)a.m; i += nth) sc.cnt[i] = sc.fill[i] = 0;
  if (tid < (size_t)L_INTS) sc.misc[tid] = 0;
}

__global__ __launch_bounds__(NK_WG) void lo_first_kernel(ListObsArgs a) {
  const LScratch sc = l_scratch(a);
  for (int i = blockIdx.x * NK_WG + threadIdx.x; i < a.m; i += gridDim.x * NK_WG) {
    const int64_t p = spfe_nk_list_point(a.point_idx, a.first_row, i);
    if (spfe_nk_list_precode(p, a.n_table) < 0) atomicMin(&sc.rank[p], i);
  }
}

// one entry of a row in the scan, by the whole wavefront: every lane calls it, with p = -1 where it has no entry
__device__ __forceinline__ void lo_scan_entry(const ListObsArgs &a, const LScratch &sc, int s, int k, int p, int lane) {
  int i = spfe_nk_in_range(p, a.n_table) ? sc.rank[p] : NK_NONE;
  const bool hit = i != NK_NONE;
  const unsigned long long votes = __ballot(hit);
  if (votes == 0) return;   // uniform
  int base = 0;
  const int leader = __ffsll((long long)votes) - 1;
  if (lane == leader) base = atomicAdd(&sc.misc[L_NHITS], __popcll(votes));
  base = __shfl(base, leader, 64);
  if (hit) {
    atomicAdd(&sc.cnt[i], 1);
    const long long at = (long long)base + __popcll(votes & ((1ull << lane) - 1ull));
    if (at < a.obs_cap) sc.hits[at] = make_int4(i, s, k, 0);
  }
}

__global__ __launch_bounds__(NK_WG) void lo_scan_kernel(ListObsArgs a) {
  const LScratch sc = l_scratch(a);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, stride = a.kp_stride;
  for (int s = blockIdx.x * NK_WAVES + wave; s < a.n_slots; s += gridDim.x * NK_WAVES) {   // uniform over the wavefront
    if (a.kf_flags[s] & 1u) continue;
    const int *row = a.rows + (size_t)s * stride;
    row_walk<64, true>(row, stride, lane, [&](int k, int p) { lo_scan_entry(a, sc, s, k, p, lane); });
  }
}

__global__ __launch_bounds__(NK_ONE) void lo_place_kernel(ListObsArgs a) {
  __shared__ int wcnt[NK_ONE_WAVES];
  __shared__ int wsum[NK_ONE_WAVES][5];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = a.m;
  const LScratch sc = l_scratch(a);
  int *hdr = blk_i32(a.out, 0), *point_idx = blk_i32(a.out, SPFE_LISTOBS_OFF_POINT_IDX), *obs_start = blk_i32(a.out, SPFE_LISTOBS_OFF_OBS_START(m)),
      *ref_slot = blk_i32(a.out, SPFE_LISTOBS_OFF_REF_SLOT(m));
  const int n_hits = sc.misc[L_NHITS];
  const bool overflow = n_hits > a.obs_cap;
  int total = 0, mx = 0;
  int c[4] = {0, 0, 0, 0};
  for (int base = 0; base < m; base += NK_ONE) {   // uniform
    const int i = base + tid;
    int code = -1, n = 0;
    int64_t p = -1;
    if (i < m) {
      p = spfe_nk_list_point(a.point_idx, a.first_row, i);
      code = spfe_nk_list_precode(p, a.n_table);
      if (code < 0) code = sc.rank[p] == i ? SPFE_LISTOBS_CODE_FIRST : SPFE_LISTOBS_CODE_REPEATED;
      if (code == SPFE_LISTOBS_CODE_FIRST) n = sc.cnt[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) c[k] += code == k;
      mx = n > mx ? n : mx;
    }
    int tc;
    const int off = wg_ordered_offset<NK_ONE>(n, wcnt, &tc);
    if (i < m) {
      const bool is_first = code == SPFE_LISTOBS_CODE_FIRST;
      point_idx[i] = is_first ? (int)p : -1;
      ref_slot[i] = is_first ? a.mp_ref_slot[p] : -1;
      obs_start[i] = overflow ? 0 : total + off;
    }
    total += tc;
  }
  if (tid == 0) obs_start[m] = overflow ? 0 : total;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int s = wave_sum(c[k]);
    if (lane == 0) wsum[wave][k] = s;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const int o = __shfl_xor(mx, off, 64);
    mx = o > mx ? o : mx;
  }
  if (lane == 0) wsum[wave][4] = mx;
  __syncthreads();
  if (tid < 16) {
    int t[4] = {0, 0, 0, 0}, max_obs = 0;
    for (int w = 0; w < NK_ONE_WAVES; ++w) {
      for (int k = 0; k < 4; ++k) t[k] += wsum[w][k];
      max_obs = wsum[w][4] > max_obs ? wsum[w][4] : max_obs;
    }
    int v = 0;
    if (tid == SPFE_LISTOBS_OFF_STATUS / 4) v = (overflow ? SPFE_LISTOBS_OVERFLOW : 0) | (max_obs > SPFE_MP_MAX_OBS ? SPFE_LISTOBS_MANY : 0);
    if (tid == SPFE_LISTOBS_OFF_M / 4) v = m;
    if (tid == SPFE_LISTOBS_OFF_N_FIRST / 4) v = t[SPFE_LISTOBS_CODE_FIRST];
    if (tid == SPFE_LISTOBS_OFF_N_EMPTY / 4) v = t[SPFE_LISTOBS_CODE_EMPTY];
    if (tid == SPFE_LISTOBS_OFF_N_WILD / 4) v = t[SPFE_LISTOBS_CODE_WILD];
    if (tid == SPFE_LISTOBS_OFF_N_REPEATED / 4) v = t[SPFE_LISTOBS_CODE_REPEATED];
    if (tid == SPFE_LISTOBS_OFF_N_OBS / 4) v = overflow ? 0 : total;
    if (tid == SPFE_LISTOBS_OFF_N_OBS_NEEDED / 4) v = n_hits;
    if (tid == SPFE_LISTOBS_OFF_MAX_OBS / 4) v = max_obs;
    if (tid == SPFE_LISTOBS_OFF_OBS_CAP / 4) v = a.obs_cap;
    hdr[tid] = v;
  }
  zero_bytes(a.out, SPFE_LISTOBS_OFF_POINT_IDX + 4 * (size_t)m, SPFE_LISTOBS_OFF_OBS_START(m), tid, NK_ONE);
  zero_bytes(a.out, SPFE_LISTOBS_OFF_OBS_START(m) + 4 * ((size_t)m + 1), SPFE_LISTOBS_OFF_REF_SLOT(m), tid, NK_ONE);
  zero_bytes(a.out, SPFE_LISTOBS_OFF_REF_SLOT(m) + 4 * (size_t)m, SPFE_LISTOBS_OFF_OBS(m), tid, NK_ONE);
  zero_bytes(a.out, SPFE_LISTOBS_OFF_OBS(m) + 8 * (size_t)a.obs_cap, SPFE_LISTOBS_OUT_BYTES(m, a.obs_cap), tid, NK_ONE);
}

__global__ __launch_bounds__(NK_WG) void lo_scatter_kernel(ListObsArgs a) {
  const LScratch sc = l_scratch(a);
  const int *obs_start = reinterpret_cast<const int *>(a.out + SPFE_LISTOBS_OFF_OBS_START(a.m));
  const int n_hits = sc.misc[L_NHITS];
  if (n_hits > a.obs_cap) return;
  for (int h = blockIdx.x * NK_WG + threadIdx.x; h < n_hits; h += gridDim.x * NK_WG) {
    const int4 q = sc.hits[h];
    const int at = obs_start[q.x] + atomicAdd(&sc.fill[q.x], 1);   // inside [obs_start[i], obs_start[i + 1]): cnt[i] hits name i
    sc.placed[at] = spfe_nk_obs_key(q.y, q.z);
  }
}

// the observations of the range [first, first + len) into their places: thread t of T takes every T-th of them
template <int T>
__device__ __forceinline__ void lo_order_range(const unsigned long long *placed, int *obs, int first, int len, int t) {
  for (int e = t; e < len; e += T) {
    const unsigned long long key = placed[first + e];
    int r = 0;
    for (int o = 0; o < len; ++o) r += placed[first + o] < key;   // the keys of a range are distinct: a (slot, keypoint) pair is one row entry
    obs[2 * (size_t)(first + r)] = (int)(key >> 32);
    obs[2 * (size_t)(first + r) + 1] = (int)(uint32_t)key;
  }
}

__global__ __launch_bounds__(NK_WG) void lo_order_kernel(ListObsArgs a) {
  const LScratch sc = l_scratch(a);
  const int *hdr = reinterpret_cast<const int *>(a.out), *obs_start = reinterpret_cast<const int *>(a.out + SPFE_LISTOBS_OFF_OBS_START(a.m));
  int *obs = blk_i32(a.out, SPFE_LISTOBS_OFF_OBS(a.m));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n_obs = hdr[SPFE_LISTOBS_OFF_N_OBS / 4], max_obs = hdr[SPFE_LISTOBS_OFF_MAX_OBS / 4];
  if (n_obs > 0) {   // 0 under an overflow
    for (int i = blockIdx.x * NK_WAVES + wave; i < a.m; i += gridDim.x * NK_WAVES) {   // uniform over the wavefront
      const int first = obs_start[i], len = obs_start[i + 1] - first;
      if (len > 0 && len <= LO_WAVE_MAX) lo_order_range<64>(sc.placed, obs, first, len, lane);
    }
    if (max_obs > LO_WAVE_MAX) {   // uniform over the grid
      for (int i = blockIdx.x; i < a.m; i += gridDim.x) {   // uniform over the workgroup
        const int first = obs_start[i], len = obs_start[i + 1] - first;
        if (len > LO_WAVE_MAX) lo_order_range<NK_WG>(sc.placed, obs, first, len, threadIdx.x);
      }
    }
  }
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
  for (size_t t = 2 * (size_t)n_obs + tid; t < 2 * (size_t)a.obs_cap; t += nth) obs[t] = -1;
}

size_t newkf_scratch_bytes(int n_table) { return pad16(4 * (size_t)n_table); }
size_t listobs_scratch_bytes(int n_table, int m, int obs_cap) {
  return pad16(4 * (size_t)n_table) + 2 * pad16(4 * (size_t)m) + pad16(16 * (size_t)obs_cap) + pad16(8 * (size_t)obs_cap) + pad16(4 * (size_t)L_INTS);
}

hipError_t launch_insert_keyframe(const NewKfArgs &a, hipStream_t s) {
  const MpLife &l = a.life;
  if (l.n_table < 1 || l.n_table > SPFE_MP_MAX_POINTS || l.recent_cap < 1 || l.recent_cap > SPFE_MP_MAX_POINTS || a.kp_stride < 1 || a.n_slots < 1 ||
      a.n_kp < 0 || a.n_kp > a.kp_stride || a.cur_slot < 0 || a.cur_slot >= a.n_slots || !a.out || !a.scratch)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(nk_preset_kernel, dim3(groups_for((size_t)l.n_table, NK_WG, NK_GRID)), dim3(NK_WG), 0, s, a);
  hipLaunchKernelGGL(nk_first_kernel, dim3(groups_for((size_t)a.n_kp, NK_WG, NK_GRID)), dim3(NK_WG), 0, s, a);
  hipLaunchKernelGGL(nk_insert_kernel, dim3(1), dim3(NK_ONE), 0, s, a);
  hipLaunchKernelGGL(nk_desc_kernel, dim3(groups_for((size_t)a.n_kp, NK_WAVES, NK_GRID)), dim3(NK_WG), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_list_observations(const ListObsArgs &a, hipStream_t s) {
  if (a.n_table < 1 || a.n_table > SPFE_MP_MAX_POINTS || a.m < 0 || a.m > SPFE_MP_MAX_POINTS || a.obs_cap < 0 || a.obs_cap > SPFE_MP_MAX_EDGES ||
      a.first_row < 0 || a.kp_stride < 1 || a.n_slots < 1 || !a.out || !a.scratch)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(lo_preset_kernel, dim3(groups_for(std::max((size_t)a.n_table, (size_t)a.m), NK_WG, NK_GRID)), dim3(NK_WG), 0, s, a);
  hipLaunchKernelGGL(lo_first_kernel, dim3(groups_for((size_t)a.m, NK_WG, NK_GRID)), dim3(NK_WG), 0, s, a);
  hipLaunchKernelGGL(lo_scan_kernel, dim3(groups_for((size_t)a.n_slots, NK_WAVES, NK_GRID)), dim3(NK_WG), 0, s, a);
  hipLaunchKernelGGL(lo_place_kernel, dim3(1), dim3(NK_ONE), 0, s, a);
  hipLaunchKernelGGL(lo_scatter_kernel, dim3(groups_for((size_t)a.obs_cap, NK_WG, NK_GRID)), dim3(NK_WG), 0, s, a);
  hipLaunchKernelGGL(lo_order_kernel, dim3(groups_for(std::max((size_t)a.m, (size_t)a.obs_cap / 32), NK_WAVES, NK_GRID)), dim3(NK_WG), 0, s, a);
  return hipGetLastError();
}

}  // namespace spfe
