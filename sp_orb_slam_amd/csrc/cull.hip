// cull.hip — keyframe culling on the device: the cull loop of the local mapper (local_mapper.cpp:979-1032) with KeyFrame::SetBadFlag
// (keyframe.cpp:911-997) on the caller's resident rows, flags, observation counts and graph state.  The contract is
// include/spfe_cull_math.h (integers and one f32 division); the host statement the tests hold these kernels to is
// tests/cull_ref/cull_ref.c: rows, flags, counts, state, tables and the whole block are equal byte for byte.
//
// FOUR launches whatever the sizes are:
//   ck_first_kernel  multi-workgroup: the presets of the scratch (first entry per point, candidate and touched marks) and the first
//                    pass's counts, a wavefront a list entry, a wave reduction, no atomics.
//   ck_loop_kernel   ONE workgroup: the list, the passes (from the second on it re-reads only the rows still in the list, a wavefront
//                    a row), the choice as a maximum of (ratio, position) keys, and the cull of the chosen keyframe's points.  The
//                    decrement of nobs and the first entry of a point are integer atomics whose result does not depend on their
//                    order; the ordered list of bad points is a ranked compaction.
//   ck_graph_kernel  ONE workgroup: per culled keyframe, in cull order, the removal of its link from each neighbour (the neighbour's
//                    keys in LDS, a rank sort straight into ord and the tables; a wavefront a neighbour while its map has at most
//                    256 keys, the whole workgroup on a larger one), the preset of its own rows, and the re-parenting
//                    steps (a wavefront a child, the offer as a maximum of (weight, walk position) keys); then the touched list.
//   ck_rows_kernel   multi-workgroup: every entry that names a newly bad point becomes -1 in the rows of the slots that are not bad;
//                    it leaves at once when no point went bad.
// No workgroup waits for another: the order between the four is the launch boundary.  What one workgroup writes to global memory and
// reads again (mp_flags, the graph rows) is ordered by the barrier alone; nobs and the first-entry marks, which atomics change in L2,
// are read back past the vector cache (ck_sync, load_agent).  spfe_count_observations_resident is ck_zero_kernel + ck_nobs_kernel.
#include <algorithm>
#include <climits>

#include "../../include/spfe.h"
#include "../../include/spfe_covis_math.h"
#include "../../include/spfe_cull_math.h"
#include "spfe_kernels.h"
#include "wave_ops.h"
#include "resident_rows.h"

namespace spfe {

namespace {
constexpr int CK_WG = 1024;
constexpr int CK_WAVES = CK_WG / 64;
constexpr int CK_GRID = 1024;
constexpr int CK_WAVE_KEYS = SPFE_COVIS_MAX_CONN / CK_WAVES;   // a neighbour map up to this size is one wavefront's work
constexpr int CK_FIRST_NONE = INT_MAX;   // first[p]: no entry of the row being culled names p
constexpr int CK_FIRST_BAD = -1;         // first[p]: p went bad in this call

struct CkScratch {
  int *first;        // [n_table]
  int *cnt_mps;      // [conn_cap] the first pass's counts per list entry
  int *cnt_red;      // [conn_cap]
  int *child;        // [n_slots]
  uint8_t *cand;     // [n_slots]
  uint8_t *touched;  // [n_slots]
  int *cull_idx;     // [n_slots] the place of a slot in cull order, -1: not culled in this call
};
__host__ __device__ inline CkScratch ck_scratch(uint8_t *base, int n_table, int n_slots, int conn_cap) {
  CkScratch s;
  s.first = reinterpret_cast<int *>(base);
  base += pad16(4 * (size_t)n_table);
  s.cnt_mps = reinterpret_cast<int *>(base);
  s.cnt_red = s.cnt_mps + conn_cap;
  base += pad16(8 * (size_t)conn_cap);
  s.child = reinterpret_cast<int *>(base);
  base += pad16(4 * (size_t)n_slots);
  s.cand = base;
  base += pad16((size_t)n_slots);
  s.touched = base;
  base += pad16((size_t)n_slots);
  s.cull_idx = reinterpret_cast<int *>(base);
  return s;
}

// What ONE workgroup writes to global memory and reads again.  Plain stores are ordered for the workgroup's own later loads by
// __syncthreads() (a release and an acquire at workgroup scope around the barrier; the wavefronts of a workgroup share one vector
// cache).  No device-scope fence is used: on this part it writes the L2 back, tens of microseconds a time.  The two arrays that are
// changed by atomics, which execute in L2, are read back past the vector cache.
__device__ __forceinline__ void ck_sync() { __syncthreads(); }

// the workgroup's maximum, the same in every thread; two barriers
__device__ __forceinline__ uint64_t ck_block_max_u64(uint64_t v, uint64_t *wkey) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint64_t o = ck_shfl_xor_u64(v, off);
    v = o > v ? o : v;
  }
  if ((threadIdx.x & 63) == 0) wkey[threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t m = 0;
#pragma unroll
  for (int w = 0; w < CK_WAVES; ++w) m = wkey[w] > m ? wkey[w] : m;
  __syncthreads();
  return m;
}
// signed keys through the same reduction: the order of int64 is that of the bits with the sign flipped
__device__ __forceinline__ uint64_t ck_ord(int64_t k) { return (uint64_t)k ^ 0x8000000000000000ull; }
__device__ __forceinline__ int64_t ck_unord(uint64_t u) { return (int64_t)(u ^ 0x8000000000000000ull); }

// (2): n_mps and n_red of one row, by one wavefront; the same sums in every lane
template <bool PAST_L1>
__device__ __forceinline__ void ck_count_row(const int *row, int stride, const uint8_t *mp_flags, const int *nobs, int n_table,
                                             int th_obs, int lane, int *n_mps, int *n_red) {
  int m = 0, r = 0;
  for (int k = lane; k < stride; k += 64) {
    const int p = row[k];
    if (spfe_ck_good(p, n_table, mp_flags)) {
      ++m;
      r += (PAST_L1 ? load_agent(nobs + p) : nobs[p]) >= th_obs;
    }
  }
  *n_mps = wave_sum(m);
  *n_red = wave_sum(r);
}

__device__ __forceinline__ void ck_table_row(int *table, int cols, int slot, int j, int v) {
  if (table && j < cols) table[(size_t)slot * cols + j] = v;
}

// Who runs an erase.  A group supplies its size, a thread's index in it, the sync that orders the group's LDS writes before its own
// later reads, and the least `found` of its threads (the same in every one of them, behind such a sync).
// ONE wavefront on its own part of the key array: wavefront scope only.  It runs inside a loop whose trip count differs between the
// wavefronts of a workgroup, where a workgroup barrier would never be reached by all of them.
struct CkWaveGroup {
  static constexpr int SIZE = 64;
  int idx;
  __device__ __forceinline__ void sync() const { wave_sync(); }
  __device__ __forceinline__ int least(int found) const {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const int o = __shfl_xor(found, off, 64);
      found = o < found ? o : found;
    }
    wave_sync();
    return found;
  }
};
// the whole workgroup on all of the key array, every call uniform
struct CkBlockGroup {
  static constexpr int SIZE = CK_WG;
  int idx;
  int *sh_found;
  __device__ __forceinline__ void sync() const { __syncthreads(); }
  __device__ __forceinline__ int least(int found) const {
    if (idx == 0) *sh_found = INT_MAX;
    __syncthreads();
    if (found != INT_MAX) atomicMin(sh_found, found);   // the slots of a row are unique: one thread at most
    __syncthreads();
    const int r = *sh_found;
    __syncthreads();
    return r;
  }
};

// (6a) for one neighbour s of the culled keyframe c, the neighbour's cn keys in the group's key array: the lookup, the removal, the
// rank sort straight into ord and the tables, the tails
template <class Group>
__device__ void ck_erase(const CullArgs &a, uint8_t *touched, int64_t *key, int s, int c, int cn, const Group g) {
  const int cap = a.conn_cap;
  int *cs = a.conn_slot + (size_t)s * cap, *cw = a.conn_w + (size_t)s * cap;
  int *os = a.ord_slot + (size_t)s * cap, *ow = a.ord_w + (size_t)s * cap;
  int found = INT_MAX;
  for (int i = g.idx; i < cn; i += Group::SIZE) {
    const int t = cs[i];
    key[i] = spfe_cv_key(cw[i], t);
    if (t == c) found = i;
  }
  found = g.least(found);
  if (found == INT_MAX) return;   // the same in every thread of the group
  for (int i = found + 1 + g.idx; i < cn; i += Group::SIZE) {   // the tail one place down, from the LDS copy
    cs[i - 1] = spfe_cv_key_slot(key[i]);
    cw[i - 1] = spfe_cv_key_w(key[i]);
  }
  if (g.idx == 0) {
    cs[cn - 1] = -1;
    cw[cn - 1] = 0;
    a.conn_n[s] = cn - 1;
    a.ord_n[s] = cn - 1;
    touched[s] = 1;
    key[found] = SPFE_COVIS_KEY_NONE;   // the threads above read the keys behind it only
  }
  g.sync();
  // ord[s] = all of conn[s] by key descending: the place of a key is the number of greater keys (they are unique)
  for (int i = g.idx; i < cn; i += Group::SIZE) {
    const int64_t k = key[i];
    if (k == SPFE_COVIS_KEY_NONE) continue;
    int rank = 0;
    for (int j = 0; j < cn; ++j) rank += key[j] > k;
    os[rank] = spfe_cv_key_slot(k);
    ow[rank] = spfe_cv_key_w(k);
    ck_table_row(a.best_a, a.n_best_a, s, rank, spfe_cv_key_slot(k));
    ck_table_row(a.best_b, a.n_best_b, s, rank, spfe_cv_key_slot(k));
  }
  for (int j = cn - 1 + g.idx; j < cap; j += Group::SIZE) {
    os[j] = -1;
    ow[j] = 0;
  }
  for (int j = cn - 1 + g.idx; j < SPFE_LOCALMAP_MAX_BEST; j += Group::SIZE) {
    ck_table_row(a.best_a, a.n_best_a, s, j, -1);
    ck_table_row(a.best_b, a.n_best_b, s, j, -1);
  }
  // the keys are the group's next neighbour's; behind the workgroup's, the rows of s are read again as a later keyframe's neighbour
  // or as a child
  g.sync();
}

}  // namespace

__global__ __launch_bounds__(256) void ck_zero_kernel(int *v, int n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * blockDim.x) v[i] = 0;
}

__global__ __launch_bounds__(256) void ck_nobs_kernel(const int *rows, int stride, const uint8_t *kf_flags, int n_slots, int *nobs,
                                                      int n_table) {
  for (int s = blockIdx.x; s < n_slots; s += gridDim.x) {
    if (kf_flags[s] & 1u) continue;
    const int *row = rows + (size_t)s * stride;
    for (int k = threadIdx.x; k < stride; k += blockDim.x) {
      const int p = row[k];
      if (p >= 0 && p < n_table) atomicAdd(&nobs[p], 1);
    }
  }
}

__global__ __launch_bounds__(256) void ck_first_kernel(CullArgs a) {
  const CkScratch sc = ck_scratch(a.scratch, a.n_table, a.n_slots, a.conn_cap);
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
  for (size_t p = tid; p < (size_t)a.n_table; p += nth) sc.first[p] = CK_FIRST_NONE;
  for (size_t s = tid; s < (size_t)a.n_slots; s += nth) {
    sc.cand[s] = 0;
    sc.touched[s] = 0;
    sc.cull_idx[s] = -1;
  }
  const int lane = threadIdx.x & 63, n_listed = clamp_int(a.ord_n[a.cur_slot], 0, a.conn_cap);
  const int *list = a.ord_slot + (size_t)a.cur_slot * a.conn_cap;
  for (size_t j = tid >> 6; j < (size_t)n_listed; j += nth >> 6) {   // a wavefront an entry
    const int s = list[j];
    int m = 0, r = 0;
    if (spfe_ck_entry_in_range(s, a.n_slots))
      ck_count_row<false>(a.kf_mp_of_kp + (size_t)s * a.kp_stride, a.kp_stride, a.mp_flags, a.nobs, a.n_table, a.th_obs, lane, &m, &r);
    if (lane == 0) {
      sc.cnt_mps[j] = m;
      sc.cnt_red[j] = r;
    }
  }
}

__global__ __launch_bounds__(CK_WG) void ck_loop_kernel(CullArgs a) {
  __shared__ int live[SPFE_COVIS_MAX_CONN], l_mps[SPFE_COVIS_MAX_CONN], l_red[SPFE_COVIS_MAX_CONN];
  __shared__ int wcnt[CK_WAVES];
  __shared__ uint64_t wkey[CK_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = a.n_slots, cap = a.conn_cap, stride = a.kp_stride;
  const CkScratch sc = ck_scratch(a.scratch, a.n_table, n, cap);
  int *hdr = reinterpret_cast<int *>(a.out);
  int *e_slot = reinterpret_cast<int *>(a.out + SPFE_CULL_OFF_ENTRY_SLOT), *e_code = reinterpret_cast<int *>(a.out + SPFE_CULL_OFF_ENTRY_CODE(cap));
  int *e_pass = reinterpret_cast<int *>(a.out + SPFE_CULL_OFF_ENTRY_PASS(cap)), *e_mps = reinterpret_cast<int *>(a.out + SPFE_CULL_OFF_ENTRY_MPS(cap));
  int *e_red = reinterpret_cast<int *>(a.out + SPFE_CULL_OFF_ENTRY_RED(cap)), *culled = reinterpret_cast<int *>(a.out + SPFE_CULL_OFF_CULLED_SLOT(cap));
  int *bad_point = reinterpret_cast<int *>(a.out + SPFE_CULL_OFF_BAD_POINT(n, cap));
  const int *list = a.ord_slot + (size_t)a.cur_slot * cap;   // not written before ck_graph_kernel
  const int n_listed = clamp_int(a.ord_n[a.cur_slot], 0, cap);

  // the block: header and the zeros behind the last array (the header's counts come at the end), the tails of the lists
  for (int i = tid; i < 16; i += CK_WG) hdr[i] = 0;
  {
    const size_t end = SPFE_CULL_OFF_BAD_POINT(n, cap) + 4 * (size_t)a.bad_cap, all = SPFE_CULL_OUT_BYTES(n, cap, a.bad_cap);
    for (size_t b = end + tid; b < all; b += CK_WG) a.out[b] = 0;
  }
  for (int j = tid; j < cap; j += CK_WG) culled[j] = -1;
  for (int j = tid; j < a.bad_cap; j += CK_WG) bad_point[j] = -1;

  // (1) the list
  int n_live = 0, wild = 0;
  for (int base = 0; base < cap; base += CK_WG) {
    const int j = base + tid;
    int code = -1, s = -1, is_live = 0;
    if (j < n_listed) {
      s = list[j];
      if (!spfe_ck_entry_in_range(s, n)) {
        code = SPFE_CULL_CODE_WILD;
        wild = 1;
      } else {
        code = spfe_ck_entry_code(s, a.origin_slot, a.kf_flags[s]);
        is_live = code < 0;
      }
    }
    if (j < cap) {
      e_slot[j] = s;
      e_code[j] = code;
      e_pass[j] = j < n_listed ? 0 : -1;
      e_mps[j] = 0;
      e_red[j] = 0;
    }
    int total;
    const int r = wg_ordered_offset<CK_WG>(is_live, wcnt, &total);
    if (is_live) live[n_live + r] = j;
    n_live += total;
  }
  int status = __syncthreads_or(wild) ? SPFE_CULL_WILD_ENTRY : 0;
  int n_passes = 0, n_culled = 0, n_deferred = 0, n_bad = 0;

  while (n_live > 0) {   // uniform
    ++n_passes;
    // (2) the counts: the first pass's are ck_first_kernel's
    if (n_passes == 1) {
      for (int i = tid; i < n_live; i += CK_WG) {
        l_mps[i] = sc.cnt_mps[live[i]];
        l_red[i] = sc.cnt_red[live[i]];
      }
    } else {
      for (int i = wave; i < n_live; i += CK_WAVES) {
        int m, r;
        ck_count_row<true>(a.kf_mp_of_kp + (size_t)list[live[i]] * stride, stride, a.mp_flags, a.nobs, a.n_table, a.th_obs, lane, &m, &r);
        if (lane == 0) {
          l_mps[i] = m;
          l_red[i] = r;
        }
      }
    }
    __syncthreads();
    // drops and the choice
    uint64_t offer = 0;
    for (int i = tid; i < n_live; i += CK_WG) {
      const int j = live[i];
      const float ratio = spfe_ck_ratio(l_red[i], l_mps[i]);
      e_mps[j] = l_mps[i];
      e_red[j] = l_red[i];
      e_pass[j] = n_passes;
      if (spfe_ck_drops(ratio, a.cov_ratio)) {
        e_code[j] = SPFE_CULL_CODE_DROPPED;
      } else {
        const uint64_t k = spfe_ck_offer(ratio, i);
        offer = k > offer ? k : offer;
      }
    }
    offer = ck_block_max_u64(offer, wkey);
    const int chosen = offer ? spfe_ck_offer_pos(offer) : -1;   // a position in live[]
    const int chosen_j = chosen >= 0 ? live[chosen] : -1;
    __syncthreads();
    // the list without the dropped and the chosen, in order
    int kept = 0;
    for (int base = 0; base < n_live; base += CK_WG) {
      const int i = base + tid;
      int keep = 0, j = -1;
      if (i < n_live) {
        j = live[i];
        keep = i != chosen && !spfe_ck_drops(spfe_ck_ratio(l_red[i], l_mps[i]), a.cov_ratio);
      }
      int total;
      const int r = wg_ordered_offset<CK_WG>(keep, wcnt, &total);   // the barrier inside: every read of the chunk is before its writes
      if (keep) live[kept + r] = j;
      kept += total;
    }
    n_live = kept;
    __syncthreads();
    if (chosen < 0) {
      if (n_live > 0) {   // (3)
        status |= SPFE_CULL_STALLED;
        for (int i = tid; i < n_live; i += CK_WG) e_code[live[i]] = SPFE_CULL_CODE_STALLED;
      }
      break;
    }
    // (4)
    const int m = list[chosen_j];
    const unsigned fl = a.kf_flags[m];
    if (fl & SPFE_KF_NOT_ERASE) {
      if (tid == 0) {
        a.kf_flags[m] = (uint8_t)(fl | SPFE_KF_TO_BE_ERASED);
        e_code[chosen_j] = SPFE_CULL_CODE_DEFERRED;
      }
      ++n_deferred;
      continue;
    }
    // (5) the points of row m: every entry takes 1 and offers its index as the first
    const int *row = a.kf_mp_of_kp + (size_t)m * stride;
    for (int k = tid; k < stride; k += CK_WG) {
      const int p = row[k];
      if (spfe_ck_good(p, a.n_table, a.mp_flags)) {
        atomicSub(&a.nobs[p], 1);
        atomicMin(&sc.first[p], k);
      }
    }
    ck_sync();
    // the first entry of a point decides for it, and it alone writes the point's flag and mark
    for (int base = 0; base < stride; base += CK_WG) {
      const int k = base + tid;
      int p = -1, owner = 0, bad = 0;
      if (k < stride) {
        p = row[k];
        owner = p >= 0 && p < a.n_table && load_agent(sc.first + p) == k;
        bad = owner && spfe_ck_goes_bad(load_agent(a.nobs + p));
      }
      int total;
      const int r = wg_ordered_offset<CK_WG>(bad, wcnt, &total);
      if (bad) {
        if (n_bad + r < a.bad_cap) bad_point[n_bad + r] = p;
        a.mp_flags[p] = (uint8_t)(a.mp_flags[p] & ~SPFE_PROJ_SEARCHABLE);
        store_agent(sc.first + p, CK_FIRST_BAD);
      } else if (owner) {
        store_agent(sc.first + p, CK_FIRST_NONE);
      }
      n_bad += total;
    }
    if (tid == 0) {
      a.kf_flags[m] = (uint8_t)(fl | 1u);
      e_code[chosen_j] = SPFE_CULL_CODE_CULLED;
      culled[n_culled] = m;
    }
    ++n_culled;
    ck_sync();
  }
  if (tid == 0) {
    hdr[SPFE_CULL_OFF_STATUS / 4] = status | (n_bad > a.bad_cap ? SPFE_CULL_BAD_CUT : 0);
    hdr[SPFE_CULL_OFF_N_LISTED / 4] = n_listed;
    hdr[SPFE_CULL_OFF_N_PASSES / 4] = n_passes;
    hdr[SPFE_CULL_OFF_N_CULLED / 4] = n_culled;
    hdr[SPFE_CULL_OFF_N_DEFERRED / 4] = n_deferred;
    hdr[SPFE_CULL_OFF_N_BAD / 4] = n_bad;
    hdr[SPFE_CULL_OFF_N_BAD_STORED / 4] = n_bad < a.bad_cap ? n_bad : a.bad_cap;
  }
}

__global__ __launch_bounds__(CK_WG) void ck_graph_kernel(CullArgs a) {
  __shared__ int64_t key[SPFE_COVIS_MAX_CONN];
  __shared__ int wcnt[CK_WAVES];
  __shared__ uint64_t wkey[CK_WAVES];
  __shared__ int sh_found, sh_large;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = a.n_slots, cap = a.conn_cap;
  const CkScratch sc = ck_scratch(a.scratch, a.n_table, n, cap);
  int *hdr = reinterpret_cast<int *>(a.out);
  const int *culled = reinterpret_cast<const int *>(a.out + SPFE_CULL_OFF_CULLED_SLOT(cap));
  int *touched_slot = reinterpret_cast<int *>(a.out + SPFE_CULL_OFF_TOUCHED_SLOT(cap));
  int *ev_c = reinterpret_cast<int *>(a.out + SPFE_CULL_OFF_EVENT_CHILD(n, cap)), *ev_p = reinterpret_cast<int *>(a.out + SPFE_CULL_OFF_EVENT_PARENT(n, cap));
  const int n_culled = clamp_int(hdr[SPFE_CULL_OFF_N_CULLED / 4], 0, cap);
  for (int s = tid; s < n; s += CK_WG) {
    ev_c[s] = -1;
    ev_p[s] = -1;
  }
  for (int ci = tid; ci < n_culled; ci += CK_WG) atomicMax(&sc.cull_idx[culled[ci]], ci);   // a slot is culled once: one writer
  __syncthreads();
  int status = 0, n_ev = 0;

  for (int ci = 0; ci < n_culled; ++ci) {   // (6), uniform throughout
    const int c = culled[ci];
    int *ccs = a.conn_slot + (size_t)c * cap, *ccw = a.conn_w + (size_t)c * cap;
    int *cos = a.ord_slot + (size_t)c * cap, *cow = a.ord_w + (size_t)c * cap;
    const int cn_c = clamp_int(a.conn_n[c], 0, cap);
    // (a) the neighbours are distinct slots: a wavefront each while the map fits its part of the keys ...
    if (tid == 0) sh_large = 0;
    __syncthreads();
    for (int q = wave; q < cn_c; q += CK_WAVES) {
      const int s = ccs[q];
      if (!spfe_ck_entry_in_range(s, n) || s == c) continue;
      const int cn = clamp_int(a.conn_n[s], 0, cap);
      if (cn <= CK_WAVE_KEYS)
        ck_erase(a, sc.touched, key + wave * CK_WAVE_KEYS, s, c, cn, CkWaveGroup{lane});
      else if (lane == 0)
        sh_large = 1;
    }
    ck_sync();
    // ... and the whole workgroup on each larger one, when there is any (a map that lost a key above is still no larger than
    // CK_WAVE_KEYS); the flag is next written behind the barriers of (c)
    for (int q = 0; q < (sh_large ? cn_c : 0); ++q) {
      const int s = ccs[q];
      if (!spfe_ck_entry_in_range(s, n) || s == c) continue;
      const int cn = clamp_int(a.conn_n[s], 0, cap);
      if (cn <= CK_WAVE_KEYS) continue;
      ck_erase(a, sc.touched, key, s, c, cn, CkBlockGroup{tid, &sh_found});
    }
    // (b)
    for (int j = tid; j < cap; j += CK_WG) {
      ccs[j] = -1;
      ccw[j] = 0;
      cos[j] = -1;
      cow[j] = 0;
    }
    for (int j = tid; j < SPFE_LOCALMAP_MAX_BEST; j += CK_WG) {
      ck_table_row(a.best_a, a.n_best_a, c, j, -1);
      ck_table_row(a.best_b, a.n_best_b, c, j, -1);
    }
    if (tid == 0) {
      a.conn_n[c] = 0;
      a.ord_n[c] = 0;
    }
    // (c) the children, ascending
    const int pc = a.parent[c], p0 = spfe_ck_entry_in_range(pc, n) ? pc : -1;
    if (p0 < 0) status |= SPFE_CULL_NO_PARENT;
    int n_child = 0;
    for (int base = 0; base < n; base += CK_WG) {
      const int s = base + tid;
      const int is_child = s < n && s != c && a.parent[s] == c;
      int total;
      const int r = wg_ordered_offset<CK_WG>(is_child, wcnt, &total);
      if (is_child) sc.child[n_child + r] = s;
      n_child += total;
    }
    if (tid == 0 && p0 >= 0 && n_child > 0) sc.cand[p0] = 1;
    ck_sync();
    if (n_child == 0) continue;
    for (;;) {   // one step
      uint64_t best = ck_ord(SPFE_CULL_STEP_NONE);
      for (int ai = wave; ai < n_child; ai += CK_WAVES) {   // a wavefront a child
        const int s = sc.child[ai];
        if (s < 0 || spfe_ck_child_is_bad(a.kf_flags[s], load_agent(sc.cull_idx + s), ci)) continue;
        const int on = clamp_int(a.ord_n[s], 0, cap), cn = clamp_int(a.conn_n[s], 0, cap);
        const int *os = a.ord_slot + (size_t)s * cap, *cs = a.conn_slot + (size_t)s * cap, *cw = a.conn_w + (size_t)s * cap;
        for (int i = lane; i < on; i += 64) {
          const int e = os[i];
          if (!spfe_ck_entry_in_range(e, n) || !sc.cand[e]) continue;
          int lo = 0, hi = cn;   // GetWeight: the keys of conn ascend
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cs[mid] < e) lo = mid + 1; else hi = mid;
          }
          const int w = lo < cn && cs[lo] == e ? cw[lo] : 0;
          const uint64_t k = ck_ord(spfe_ck_step_key(w, ai, i, cap));
          best = k > best ? k : best;
        }
      }
      best = ck_block_max_u64(best, wkey);
      const int64_t won = ck_unord(best);
      if (won == SPFE_CULL_STEP_NONE) break;
      const uint32_t walk = spfe_ck_step_walk(won);
      const int ai = (int)(walk / (uint32_t)cap), i = (int)(walk % (uint32_t)cap);
      if (tid == 0) {
        const int s = sc.child[ai], np = a.ord_slot[(size_t)s * cap + i];
        a.parent[s] = np;
        sc.cand[s] = 1;
        sc.child[ai] = -1;
        if (n_ev < n) {
          ev_c[n_ev] = s;
          ev_p[n_ev] = np;
        }
      }
      ++n_ev;
      ck_sync();
    }
    // the children left over, bad ones included, go to the parent of c
    for (int base = 0; base < n_child; base += CK_WG) {
      const int ai = base + tid;
      const int s = ai < n_child ? sc.child[ai] : -1;
      int total;
      const int r = wg_ordered_offset<CK_WG>(s >= 0, wcnt, &total);
      if (s >= 0) {
        a.parent[s] = p0;
        if (n_ev + r < n) {
          ev_c[n_ev + r] = s;
          ev_p[n_ev + r] = p0;
        }
      }
      n_ev += total;
    }
    for (int s = tid; s < n; s += CK_WG) sc.cand[s] = 0;
    ck_sync();
  }

  // the touched neighbours, ascending
  int n_touched = 0;
  for (int base = 0; base < n; base += CK_WG) {
    const int s = base + tid;
    const int t = s < n && sc.touched[s];
    int total;
    const int r = wg_ordered_offset<CK_WG>(t, wcnt, &total);
    if (t) touched_slot[n_touched + r] = s;
    n_touched += total;
  }
  for (int s = n_touched + tid; s < n; s += CK_WG) touched_slot[s] = -1;
  if (tid == 0) {
    hdr[SPFE_CULL_OFF_STATUS / 4] |= status | (n_ev > n ? SPFE_CULL_EVENT_CUT : 0);
    hdr[SPFE_CULL_OFF_N_TOUCHED / 4] = n_touched;
    hdr[SPFE_CULL_OFF_N_REPARENTED / 4] = n_ev;
    hdr[SPFE_CULL_OFF_N_EVENTS / 4] = n_ev < n ? n_ev : n;
  }
}

__global__ __launch_bounds__(256) void ck_rows_kernel(CullArgs a) {
  if (reinterpret_cast<const int *>(a.out)[SPFE_CULL_OFF_N_BAD / 4] == 0) return;
  const int *first = ck_scratch(a.scratch, a.n_table, a.n_slots, a.conn_cap).first;
  for (int s = blockIdx.x; s < a.n_slots; s += gridDim.x) {
    if (a.kf_flags[s] & 1u) continue;
    int *row = a.kf_mp_of_kp + (size_t)s * a.kp_stride;
    for (int k = threadIdx.x; k < a.kp_stride; k += blockDim.x) {
      const int p = row[k];
      if (p >= 0 && p < a.n_table && first[p] == CK_FIRST_BAD) row[k] = -1;
    }
  }
}

size_t cull_scratch_bytes(int n_table, int n_slots, int conn_cap) {
  return pad16(4 * (size_t)n_table) + pad16(8 * (size_t)conn_cap) + 2 * pad16(4 * (size_t)n_slots) + 2 * pad16((size_t)n_slots);
}

hipError_t launch_count_observations(const int *rows, int kp_stride, const uint8_t *kf_flags, int n_slots, int *nobs, int n_table,
                                     hipStream_t s) {
  if (kp_stride < 1 || n_slots < 1 || n_table < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ck_zero_kernel, dim3(groups_for((size_t)n_table, 256, CK_GRID)), dim3(256), 0, s, nobs, n_table);
  hipLaunchKernelGGL(ck_nobs_kernel, dim3(groups_for((size_t)n_slots, 1, CK_GRID)), dim3(256), 0, s, rows, kp_stride, kf_flags, n_slots, nobs,
                     n_table);
  return hipGetLastError();
}

hipError_t launch_cull(const CullArgs &a, hipStream_t s) {
  if (a.conn_cap < 1 || a.conn_cap > SPFE_COVIS_MAX_CONN || a.n_slots < 1 || a.cur_slot < 0 || a.cur_slot >= a.n_slots || a.kp_stride < 1 ||
      a.n_table < 0 || a.th_obs < 1 || a.bad_cap < 0 || !a.out || !a.scratch ||
      (a.best_a && (a.n_best_a < 1 || a.n_best_a > SPFE_LOCALMAP_MAX_BEST)) ||
      (a.best_b && (a.n_best_b < 1 || a.n_best_b > SPFE_LOCALMAP_MAX_BEST)))
    return hipErrorInvalidValue;
  // the presets need a thread a point or a slot at most CK_GRID x 256 apart; the counts a wavefront a list entry
  const size_t work = std::max({(size_t)a.n_table, (size_t)a.n_slots, (size_t)a.conn_cap * 64});
  hipLaunchKernelGGL(ck_first_kernel, dim3(groups_for(work, 256, CK_GRID)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(ck_loop_kernel, dim3(1), dim3(CK_WG), 0, s, a);
  hipLaunchKernelGGL(ck_graph_kernel, dim3(1), dim3(CK_WG), 0, s, a);
  hipLaunchKernelGGL(ck_rows_kernel, dim3(groups_for((size_t)a.n_slots, 1, CK_GRID)), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace spfe
