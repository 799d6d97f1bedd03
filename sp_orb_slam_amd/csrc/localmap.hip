// localmap.hip — the tracker's local map on the device: Tracking::UpdateLocalKeyFrames (tracker.cpp:868-984) and UpdateLocalPoints
// (:843-866) on the caller's resident keyframe rows, and the count of KeyFrame::getTrackedInCommon (keyframe.cpp:697-724).  The
// contract is include/spfe_localmap_math.h (integers only); the host statement the tests hold these kernels to is
// tests/localmap_ref/localmap_ref.c: the whole block is equal byte for byte.
//
// SEVEN launches whatever the sizes are (the count form: the first three; the rows form: one of its own):
//   lm_preset_kernel   the weight table's bytes (bit 7 = SEARCHABLE, weight 0), the per-point count and key scratch, the block's
//                      header and the zero bytes behind its last array: no memset node.
//   lm_frame_kernel    one workgroup: the holders of the frame (count and first keypoint per point by atomics), the held points as
//                      an ordered compaction, the holders as list positions, and the weights into the table.
//   lm_vote_kernel     THE HOT ONE.  A wavefront a keyframe row, sixteen rows a workgroup; the row is read with 16-byte loads from
//                      its first 16-byte boundary on, head and tail one entry a lane (rows of 1001 entries are not aligned, and
//                      nothing is read outside a row); the weight table out of LDS while it fits, out of global memory (L2)
//                      beyond; votes and total are a wave reduction that lane 0 stores.  No atomics.
//   lm_expand_kernel   one workgroup: V as an ordered compaction of the slots, ref_slot as a (vote, slot) reduction, then the
//                      sequential walk — the marks are a bit a slot in LDS, the candidates of a best_cov row one lane each and a
//                      ballot, the child search a workgroup-wide minimum over d_parent.
//   lm_key_kernel      the key of every point of the local keyframes' rows by atomicMin (spfe_localmap_math.h (5)).
//   lm_count_kernel    LM_LIST_GRID workgroups, a contiguous chunk of the entries each: how many entries own their point's key.
//   lm_list_kernel     the same chunks: a workgroup's offset is the sum of the counts before it, inside it a scan a tile; then the
//                      -1 tail of point_idx and the header's counts.
// Nothing synchronises with the host, and only plain vector stores and vector atomics write.
#include "../../include/spfe.h"
#include "../../include/spfe_localmap_math.h"
#include "spfe_kernels.h"
#include "wave_ops.h"
#include "resident_rows.h"

namespace spfe {

namespace {
constexpr int LM_WG = 1024;
constexpr int LM_WAVES = LM_WG / 64;
constexpr int LM_LIST_GRID = 256;
constexpr int LM_LDS_POINTS = 128 * 1024;   // the table in LDS: a byte a point
constexpr int LM_VOTE_GRID_LDS = 256, LM_VOTE_GRID = 1024;
static_assert(SPFE_LOCALMAP_MAX_KEYFRAMES % 32 == 0 && SPFE_PROJ_MAX_POINTS % LM_WG == 0, "shapes");
static_assert((long long)SPFE_LOCALMAP_MAX_KEYFRAMES * SPFE_LOCALMAP_MAX_STRIDE + SPFE_PROJ_MAX_POINTS < (1ll << 31), "a key is an int");

// the scratch: the table's bytes (16-byte padded), then count / key per point, then the list's counts
struct LmScratch {
  uint8_t *table;
  int *count, *key, *blockcnt;
};
__host__ __device__ inline LmScratch lm_scratch(uint8_t *base, int n_table) {
  LmScratch s;
  s.table = base;
  s.count = reinterpret_cast<int *>(base + pad16((size_t)n_table));
  s.key = s.count + n_table;
  s.blockcnt = s.key + n_table;
  return s;
}
}  // namespace

__global__ __launch_bounds__(256) void lm_preset_kernel(LocalmapArgs a) {
  const LmScratch sc = lm_scratch(a.scratch, a.n_table);
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
  for (size_t p = tid; p < (size_t)a.n_table; p += nth) {
    sc.table[p] = (uint8_t)spfe_lm_table_byte(a.mp_flags[p], 0);
    sc.count[p] = 0;
    sc.key[p] = SPFE_LOCALMAP_NO_KEY;
  }
  if (tid < LM_LIST_GRID) sc.blockcnt[tid] = 0;
  if (a.out) {
    int *hdr = reinterpret_cast<int *>(a.out);
    if (tid < 8) hdr[tid] = 0;
    const size_t end = SPFE_LOCALMAP_OFF_MP_OF_KP_LIST(a.n_slots, a.point_cap) + 4 * (size_t)a.n_kp;
    const size_t all = SPFE_LOCALMAP_OUT_BYTES(a.n_slots, a.point_cap, a.n_kp);
    for (size_t b = end + tid; b < all; b += nth) a.out[b] = 0;
  }
}

// One workgroup.  Holders -> count, first keypoint (key), the held list, the list positions, the weights.
__global__ __launch_bounds__(LM_WG) void lm_frame_kernel(LocalmapArgs a) {
  __shared__ int wcnt[LM_WAVES];
  const LmScratch sc = lm_scratch(a.scratch, a.n_table);
  const int tid = threadIdx.x, n_kp = a.n_kp;
  int *point_idx = a.out ? reinterpret_cast<int *>(a.out + SPFE_LOCALMAP_OFF_POINT_IDX(a.n_slots)) : nullptr;
  int *list = a.out ? reinterpret_cast<int *>(a.out + SPFE_LOCALMAP_OFF_MP_OF_KP_LIST(a.n_slots, a.point_cap)) : nullptr;
  // the holders: every later phase reads the count and the key behind a barrier, with atomic loads of the same scope
  for (int k = tid; k < n_kp; k += LM_WG) {
    const int p = a.mp_of_kp[k];
    if (!spfe_lm_in_table(p, a.n_table) || !(a.mp_flags[p] & 1u) || (a.outlier && a.outlier[k])) continue;
    atomicAdd(&sc.count[p], 1);
    atomicMin(&sc.key[p], k);
  }
  __syncthreads();
  int n_held = 0;
  for (int base = 0; base < n_kp; base += LM_WG) {
    const int k = base + tid;
    int p = -1;
    bool holds = false, first = false;
    if (k < n_kp) {
      p = a.mp_of_kp[k];
      holds = spfe_lm_in_table(p, a.n_table) && (a.mp_flags[p] & 1u) && !(a.outlier && a.outlier[k]);
      first = holds && load_agent(&sc.key[p]) == k;
    }
    int total;
    const int r = n_held + wg_ordered_offset<LM_WG>(first ? 1 : 0, wcnt, &total);
    if (first) {
      const int c = load_agent(&sc.count[p]);
      sc.table[p] = (uint8_t)spfe_lm_table_byte(1u, c);
      store_agent(&sc.count[p], r);   // from here on: the point's list position
      if (point_idx) point_idx[r] = p;   // n_held <= n_kp <= point_cap
    }
    n_held += total;
  }
  if (!a.out) return;
  __syncthreads();
  for (int k = tid; k < n_kp; k += LM_WG) {
    const int p = a.mp_of_kp[k];
    const bool holds = spfe_lm_in_table(p, a.n_table) && (a.mp_flags[p] & 1u) && !(a.outlier && a.outlier[k]);
    list[k] = holds ? load_agent(&sc.count[p]) : -1;
  }
  if (tid == 0) reinterpret_cast<int *>(a.out)[SPFE_LOCALMAP_OFF_N_HELD / 4] = n_held;
}

// votes and total of one entry's point, added to the lane's sums
template <bool LDS>
__device__ __forceinline__ void lm_add(int p, int n_table, const uint8_t *tab, int &votes, int &total) {
  if (!spfe_lm_in_table(p, n_table)) return;
  const unsigned b = tab[p];
  votes += spfe_lm_weight(b);
  total += spfe_lm_searchable(b);
}

template <bool LDS>
__global__ __launch_bounds__(LM_WG) void lm_vote_kernel(LocalmapArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lm_tab[];
  const LmScratch sc = lm_scratch(a.scratch, a.n_table);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_table = a.n_table, stride = a.kp_stride;
  const uint8_t *tab = sc.table;
  if (LDS) {
    const int n16 = (int)(pad16((size_t)n_table) / 16);   // the scratch's table is padded to 16 bytes
    const uint4 *src = reinterpret_cast<const uint4 *>(sc.table);
    uint4 *dst = reinterpret_cast<uint4 *>(lm_tab);
    for (int i = threadIdx.x; i < n16; i += LM_WG) dst[i] = src[i];
    __syncthreads();
    tab = lm_tab;
  }
  for (int s = blockIdx.x * LM_WAVES + wave; s < a.n_slots; s += gridDim.x * LM_WAVES) {   // wave-uniform
    const int *row = a.kf_mp_of_kp + (size_t)s * stride;
    int votes = 0, total = 0;
    row_walk<64>(row, stride, lane, [&](int, int p) { lm_add<LDS>(p, n_table, tab, votes, total); });
    votes = wave_sum(votes);
    total = wave_sum(total);
    if (lane == 0) {
      a.votes[s] = votes;
      a.total[s] = total;
    }
  }
}

__global__ __launch_bounds__(LM_WG) void lm_expand_kernel(LocalmapArgs a) {
  __shared__ unsigned mark[SPFE_LOCALMAP_MAX_KEYFRAMES / 32];
  __shared__ int wcnt[LM_WAVES], wv[LM_WAVES], ws[LM_WAVES];
  __shared__ int sh_n_local, sh_stop, sh_status;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = a.n_slots;
  int *hdr = reinterpret_cast<int *>(a.out);
  int *local_kf = reinterpret_cast<int *>(a.out + SPFE_LOCALMAP_OFF_LOCAL_KF);
  for (int w = tid; w < (n + 31) / 32; w += LM_WG) mark[w] = 0u;
  __syncthreads();
  // V, ascending, and the reference keyframe
  int n_voted = 0, bv = 0, bs = -1;
  for (int base = 0; base < n; base += LM_WG) {
    const int s = base + tid;
    const int v = s < n ? a.votes[s] : 0;
    const bool f = s < n && v > 0 && !(a.kf_flags[s] & 1u);
    int total;
    const int r = n_voted + wg_ordered_offset<LM_WG>(f ? 1 : 0, wcnt, &total);
    if (f) {
      local_kf[r] = s;
      atomicOr(&mark[s >> 5], 1u << (s & 31));
      if (spfe_lm_ref_beats(v, s, bv, bs)) {
        bv = v;
        bs = s;
      }
    }
    n_voted += total;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const int ov = __shfl_xor(bv, off, 64), os = __shfl_xor(bs, off, 64);
    if (spfe_lm_ref_beats(ov, os, bv, bs)) {
      bv = ov;
      bs = os;
    }
  }
  if (lane == 0) {
    wv[wave] = bv;
    ws[wave] = bs;
  }
  for (int j = n_voted + tid; j < n; j += LM_WG) local_kf[j] = -1;   // the pushes below overwrite, behind a barrier
  if (tid == 0) {
    sh_n_local = n_voted;
    sh_stop = 0;
    sh_status = n_voted == 0 ? SPFE_LOCALMAP_NO_VOTES : 0;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < LM_WAVES; ++w)
      if (spfe_lm_ref_beats(wv[w], ws[w], bv, bs)) {
        bv = wv[w];
        bs = ws[w];
      }
    hdr[SPFE_LOCALMAP_OFF_N_VOTED / 4] = n_voted;
    hdr[SPFE_LOCALMAP_OFF_REF_SLOT / 4] = bs;
  }
  __syncthreads();   // wv / ws are the child search's from here on

  // the walk over V as it stood; every branch below is uniform over the workgroup
  for (int i = 0; i < n_voted; ++i) {
    const int stop = sh_stop, n_local = sh_n_local;
    __syncthreads();   // every thread has read them before thread 0 writes them again
    if (stop || spfe_lm_full(n_local, a.max_keyframes)) break;
    const int v = local_kf[i];
    if (wave == 0) {   // the first candidate of the best_cov row
      const int s = lane < a.n_best ? a.best_cov[(size_t)v * a.n_best + lane] : -1;
      const bool in = s >= 0 && s < n;
      const bool ok = in && !(a.kf_flags[s] & 1u) && !((mark[s >> 5] >> (s & 31)) & 1u);
      const bool wild = lane < a.n_best && (s < -1 || s >= n);
      const unsigned long long okm = __ballot(ok), wildm = __ballot(wild);
      const int first = okm ? __ffsll((long long)okm) - 1 : 64;
      const int sf = __shfl(s, first & 63, 64);
      if (lane == 0) {
        const unsigned long long before = first >= 64 ? ~0ull : ((1ull << first) - 1ull);
        if (wildm & before) sh_status |= SPFE_LOCALMAP_BAD_SLOT;
        if (okm) {
          local_kf[sh_n_local] = sf;
          sh_n_local = sh_n_local + 1;
          mark[sf >> 5] |= 1u << (sf & 31);
        }
      }
    }
    __syncthreads();
    // the lowest unmarked good child
    int c = n;
    for (int s = tid; s < n; s += LM_WG)
      if (a.parent[s] == v && !(a.kf_flags[s] & 1u) && !((mark[s >> 5] >> (s & 31)) & 1u)) {
        c = s;
        break;   // a thread's slots ascend
      }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const int o = __shfl_xor(c, off, 64);
      c = o < c ? o : c;
    }
    if (lane == 0) ws[wave] = c;
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < LM_WAVES; ++w) c = ws[w] < c ? ws[w] : c;
      int nl = sh_n_local;
      if (c < n) {
        local_kf[nl++] = c;
        mark[c >> 5] |= 1u << (c & 31);
      }
      const int p = a.parent[v];
      if (p < -1 || p >= n) {
        sh_status |= SPFE_LOCALMAP_BAD_SLOT;
      } else if (p >= 0 && !((mark[p >> 5] >> (p & 31)) & 1u)) {   // not tested for bad; ends the whole walk
        local_kf[nl++] = p;
        mark[p >> 5] |= 1u << (p & 31);
        sh_stop = 1;
      }
      sh_n_local = nl;
    }
    __syncthreads();
  }
  if (tid == 0) {
    hdr[SPFE_LOCALMAP_OFF_N_LOCAL_KF / 4] = n_voted == 0 ? 0 : sh_n_local;
    hdr[SPFE_LOCALMAP_OFF_STATUS / 4] = sh_status;
  }
}

namespace {
// entry e of the local keyframes' rows: the table row it names when that row is SEARCHABLE, else -1
__device__ __forceinline__ int lm_entry_point(const LocalmapArgs &a, const LmScratch &sc, const int *local_kf, int e) {
  const int i = e / a.kp_stride, k = e - i * a.kp_stride;
  const int p = a.kf_mp_of_kp[(size_t)local_kf[i] * a.kp_stride + k];
  if (!spfe_lm_in_table(p, a.n_table) || !spfe_lm_searchable(sc.table[p])) return -1;
  return p;
}
}  // namespace

__global__ __launch_bounds__(256) void lm_key_kernel(LocalmapArgs a) {
  const LmScratch sc = lm_scratch(a.scratch, a.n_table);
  const int *hdr = reinterpret_cast<const int *>(a.out);
  const int *local_kf = reinterpret_cast<const int *>(a.out + SPFE_LOCALMAP_OFF_LOCAL_KF);
  const int N = hdr[SPFE_LOCALMAP_OFF_N_LOCAL_KF / 4] * a.kp_stride;   // <= 2^30
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < N; e += gridDim.x * blockDim.x) {
    const int p = lm_entry_point(a, sc, local_kf, e);
    if (p >= 0) atomicMin(&sc.key[p], a.n_kp + e);   // n_kp + i kp_stride + k; a held point's key is below n_kp and stays
  }
}

__global__ __launch_bounds__(LM_WG) void lm_count_kernel(LocalmapArgs a) {
  __shared__ int wcnt[LM_WAVES];
  const LmScratch sc = lm_scratch(a.scratch, a.n_table);
  const int *hdr = reinterpret_cast<const int *>(a.out);
  const int *local_kf = reinterpret_cast<const int *>(a.out + SPFE_LOCALMAP_OFF_LOCAL_KF);
  const int N = hdr[SPFE_LOCALMAP_OFF_N_LOCAL_KF / 4] * a.kp_stride;
  const int chunk = (N + LM_LIST_GRID - 1) / LM_LIST_GRID;
  const long long lo = (long long)blockIdx.x * chunk;
  const int e0 = (int)(lo < N ? lo : N), e1 = (int)(lo + chunk < N ? lo + chunk : N);
  int c = 0;
  for (int e = e0 + threadIdx.x; e < e1; e += LM_WG) {
    const int p = lm_entry_point(a, sc, local_kf, e);
    c += p >= 0 && load_agent(&sc.key[p]) == a.n_kp + e;
  }
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    c = 0;
    for (int w = 0; w < LM_WAVES; ++w) c += wcnt[w];
    sc.blockcnt[blockIdx.x] = c;
  }
}

__global__ __launch_bounds__(LM_WG) void lm_list_kernel(LocalmapArgs a) {
  __shared__ int wcnt[LM_WAVES];
  const LmScratch sc = lm_scratch(a.scratch, a.n_table);
  int *hdr = reinterpret_cast<int *>(a.out);
  const int *local_kf = reinterpret_cast<const int *>(a.out + SPFE_LOCALMAP_OFF_LOCAL_KF);
  int *point_idx = reinterpret_cast<int *>(a.out + SPFE_LOCALMAP_OFF_POINT_IDX(a.n_slots));
  const int N = hdr[SPFE_LOCALMAP_OFF_N_LOCAL_KF / 4] * a.kp_stride, n_held = hdr[SPFE_LOCALMAP_OFF_N_HELD / 4];
  const int chunk = (N + LM_LIST_GRID - 1) / LM_LIST_GRID;
  const long long lo = (long long)blockIdx.x * chunk;
  const int e0 = (int)(lo < N ? lo : N), e1 = (int)(lo + chunk < N ? lo + chunk : N);
  int at = n_held, all = n_held;
  for (int b = 0; b < LM_LIST_GRID; ++b) {   // uniform loads
    const int k = sc.blockcnt[b];
    at += b < (int)blockIdx.x ? k : 0;
    all += k;
  }
  for (int base = e0; base < e1; base += LM_WG) {
    const int e = base + threadIdx.x;
    int p = -1;
    if (e < e1) {
      p = lm_entry_point(a, sc, local_kf, e);
      if (p >= 0 && load_agent(&sc.key[p]) != a.n_kp + e) p = -1;
    }
    int total;
    const int r = at + wg_ordered_offset<LM_WG>(p >= 0 ? 1 : 0, wcnt, &total);
    if (p >= 0 && r < a.point_cap) point_idx[r] = p;
    at += total;
  }
  const int n_points = all < a.point_cap ? all : a.point_cap;
  for (int j = n_points + blockIdx.x * LM_WG + threadIdx.x; j < a.point_cap; j += LM_LIST_GRID * LM_WG) point_idx[j] = -1;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    hdr[SPFE_LOCALMAP_OFF_N_POINTS / 4] = n_points;
    hdr[SPFE_LOCALMAP_OFF_N_POINTS_TOTAL / 4] = all;
    if (all > a.point_cap) hdr[SPFE_LOCALMAP_OFF_STATUS / 4] = hdr[SPFE_LOCALMAP_OFF_STATUS / 4] | SPFE_LOCALMAP_TRUNCATED;
  }
}

__global__ __launch_bounds__(256) void lm_rows_kernel(const int *point_idx, int point_cap, const int *list, int n_kp, int *rows) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_kp) return;
  const int l = list[k];
  rows[k] = l >= 0 && l < point_cap ? point_idx[l] : -1;
}

size_t localmap_scratch_bytes(int n_table) { return pad16((size_t)n_table) + 8 * (size_t)n_table + 4 * LM_LIST_GRID; }
int localmap_lds_point_capacity() { return LM_LDS_POINTS; }

namespace {
bool lm_sizes_ok(const LocalmapArgs &a) {
  return a.n_slots >= 1 && a.n_slots <= SPFE_LOCALMAP_MAX_KEYFRAMES && a.kp_stride >= 1 && a.kp_stride <= SPFE_LOCALMAP_MAX_STRIDE &&
         a.n_table >= 0 && a.n_table <= SPFE_MP_MAX_POINTS && a.n_kp >= 0 &&
         a.n_kp <= SPFE_PROJ_MAX_POINTS;
}
hipError_t lm_first_three(const LocalmapArgs &a, hipStream_t s) {
  const unsigned pre = groups_for((size_t)(a.n_table > 8 ? a.n_table : 8), 256, 1024);   // at least LM_LIST_GRID threads
  hipLaunchKernelGGL(lm_preset_kernel, dim3(pre), dim3(256), 0, s, a);
  hipLaunchKernelGGL(lm_frame_kernel, dim3(1), dim3(LM_WG), 0, s, a);
  if (a.n_table <= LM_LDS_POINTS) {
    const size_t lds = pad16((size_t)(a.n_table > 0 ? a.n_table : 1));
    if (lds > 48 * 1024) {   // beyond the default dynamic-LDS limit: raise it
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(lm_vote_kernel<true>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, LM_LDS_POINTS);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(lm_vote_kernel<true>, dim3(groups_for((size_t)a.n_slots, LM_WAVES, LM_VOTE_GRID_LDS)), dim3(LM_WG), lds, s, a);
  } else {
    hipLaunchKernelGGL(lm_vote_kernel<false>, dim3(groups_for((size_t)a.n_slots, LM_WAVES, LM_VOTE_GRID)), dim3(LM_WG), 0, s, a);
  }
  return hipGetLastError();
}
}  // namespace

hipError_t launch_localmap_count(const LocalmapArgs &a, hipStream_t s) {
  if (!lm_sizes_ok(a) || a.out) return hipErrorInvalidValue;
  return lm_first_three(a, s);
}

// The count with a keyframe row as the frame: the frame kernel's loops have no limit of their own when there is no block, so
// n_kp may be a whole row.
hipError_t launch_localmap_count_row(const LocalmapArgs &a, hipStream_t s) {
  LocalmapArgs b = a;
  b.n_kp = 0;
  if (!lm_sizes_ok(b) || a.out || a.n_kp < 0 || a.n_kp > SPFE_LOCALMAP_MAX_STRIDE) return hipErrorInvalidValue;
  return lm_first_three(a, s);
}

hipError_t launch_localmap(const LocalmapArgs &a, hipStream_t s) {
  if (!lm_sizes_ok(a) || !a.out || a.n_best < 1 || a.n_best > SPFE_LOCALMAP_MAX_BEST || a.point_cap < 1 ||
      a.point_cap > SPFE_PROJ_MAX_POINTS || a.n_kp > a.point_cap || a.max_keyframes < 0)
    return hipErrorInvalidValue;
  hipError_t e = lm_first_three(a, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(lm_expand_kernel, dim3(1), dim3(LM_WG), 0, s, a);
  hipLaunchKernelGGL(lm_key_kernel, dim3(LM_LIST_GRID), dim3(256), 0, s, a);
  hipLaunchKernelGGL(lm_count_kernel, dim3(LM_LIST_GRID), dim3(LM_WG), 0, s, a);
  hipLaunchKernelGGL(lm_list_kernel, dim3(LM_LIST_GRID), dim3(LM_WG), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_localmap_rows(const int *point_idx, int point_cap, const int *list, int n_kp, int *rows, hipStream_t s) {
  if (n_kp < 0 || point_cap < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(lm_rows_kernel, dim3(n_kp ? (n_kp + 255) / 256 : 1), dim3(256), 0, s, point_idx, point_cap, list, n_kp, rows);
  return hipGetLastError();
}

}  // namespace spfe
