// covis.hip — the covisibility graph on the device: KeyFrame::UpdateConnections (keyframe.cpp:757-849) with AddConnection /
// UpdateBestCovisibles (:577-612) on the caller's resident keyframe rows and resident graph state.  The contract is
// include/spfe_covis_math.h (integers only); the host statement the tests hold these kernels to is tests/covis_ref/covis_ref.c:
// the state, the tables and the whole block are equal byte for byte.
//
// FIVE launches whatever the sizes are:
//   lm_preset_kernel, lm_frame_kernel, lm_vote_kernel   localmap.hip's count with row cur_slot as the frame: votes per slot into
//                      the scratch (the weight table in LDS while it fits, no atomics in the vote).
//   cv_current_kernel  one workgroup: counter = votes with cur_slot and the bad slots at 0, n_counter, the slots at or above th and
//                      the maximum as a (count, slot) reduction; then, unless the call is empty or overflows, conn[cur] and P as
//                      ordered compactions of the slots, P's keys sorted in LDS into ord[cur], the parent, the table rows of
//                      cur_slot, and all of the block but the codes of P.
//   cv_neigh_kernel    THE PARALLEL ONE.  CV_NEIGH_GRID workgroups stride over P, n_linked read from the block: the neighbour's
//                      map into LDS as (weight, slot) keys, the lookup of cur_slot and its place as a count of the lower slots,
//                      replace or insert (the shifted tail is stored from the LDS copy), a bitonic sort of the keys, then ord and
//                      the table rows.  The neighbours are distinct from each other and from cur_slot: no two workgroups write one
//                      row.  n_changed, n_overflow and the overflow bit are vector atomics on the block's header.
// cv_reset_kernel is the preset of a range of slots.  Nothing synchronises with the host; the state is written by plain vector
// stores only.
#include "../../include/spfe.h"
#include "../../include/spfe_covis_math.h"
#include "spfe_kernels.h"
#include "wave_ops.h"
#include "resident_rows.h"

namespace spfe {

namespace {
constexpr int CV_WG = 1024;
constexpr int CV_WAVES = CV_WG / 64;
constexpr int CV_NEIGH_GRID = 64;
static_assert(SPFE_COVIS_MAX_CONN * 8 <= 32 * 1024 && (SPFE_COVIS_MAX_CONN & (SPFE_COVIS_MAX_CONN - 1)) == 0, "a row of keys in LDS");

__device__ __forceinline__ int cv_pow2(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

// key[0, n2) into DESCENDING order, n2 a power of two; the whole workgroup calls it, behind a barrier, and leaves behind one.
// The keys of a row are unique, so any correct sort gives these bytes.
__device__ void cv_sort_desc(int64_t *key, int n2) {
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n2; i += CV_WG) {
        const int l = i ^ j;
        if (l > i) {
          const int64_t x = key[i], y = key[l];
          if ((i & k) == 0 ? x < y : x > y) {
            key[i] = y;
            key[l] = x;
          }
        }
      }
      __syncthreads();
    }
}

// the first `cols` of the n1 sorted keys' slots as the row `slot` of a best_cov table, -1 padded
__device__ __forceinline__ void cv_table_row(int *table, int cols, int slot, const int64_t *key, int n1) {
  if (!table) return;
  for (int j = threadIdx.x; j < cols; j += CV_WG) table[(size_t)slot * cols + j] = j < n1 ? spfe_cv_key_slot(key[j]) : -1;
}

// the scratch: votes and total per slot (16-byte padded), then the count's own (localmap.hip)
struct CvScratch {
  int *votes, *total;
  uint8_t *lm;
};
__host__ __device__ inline CvScratch cv_scratch(uint8_t *base, int n_slots) {
  CvScratch s;
  s.votes = reinterpret_cast<int *>(base);
  s.total = s.votes + n_slots;
  s.lm = base + pad16(8 * (size_t)n_slots);
  return s;
}
}  // namespace

__global__ __launch_bounds__(256) void cv_reset_kernel(CovisArgs a, int first_slot, int n) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
  const size_t lo = (size_t)first_slot * a.conn_cap, cnt = (size_t)n * a.conn_cap;
  for (size_t i = tid; i < cnt; i += nth) {
    a.conn_slot[lo + i] = -1;
    a.conn_w[lo + i] = 0;
    a.ord_slot[lo + i] = -1;
    a.ord_w[lo + i] = 0;
  }
  for (size_t i = tid; i < (size_t)n; i += nth) {
    const size_t s = (size_t)first_slot + i;
    a.conn_n[s] = 0;
    a.ord_n[s] = 0;
    a.parent[s] = -1;
    a.first_conn[s] = 1;
  }
}

__global__ __launch_bounds__(CV_WG) void cv_current_kernel(CovisArgs a) {
  __shared__ int64_t key[SPFE_COVIS_MAX_CONN];
  __shared__ int wcnt[CV_WAVES], wn[CV_WAVES], wa[CV_WAVES], wc[CV_WAVES], ws[CV_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = a.n_slots, cur = a.cur_slot, cap = a.conn_cap, th = a.th;
  const int *votes = cv_scratch(a.scratch, n).votes;
  int *hdr = reinterpret_cast<int *>(a.out);
  int *counter = reinterpret_cast<int *>(a.out + SPFE_COVIS_OFF_COUNTER);
  int *linked_slot = reinterpret_cast<int *>(a.out + SPFE_COVIS_OFF_LINKED_SLOT(n));
  int *linked_code = reinterpret_cast<int *>(a.out + SPFE_COVIS_OFF_LINKED_CODE(n, cap));

  // (1)-(3): the counter, its counts and the maximum
  int nc = 0, na = 0, bc = 0, bs = -1;
  for (int s = tid; s < n; s += CV_WG) {
    const int c = spfe_cv_counter(votes[s], s, cur, a.kf_flags[s]);
    counter[s] = c;
    nc += c > 0;
    na += c >= th;
    if (spfe_cv_max_beats(c, s, bc, bs)) {
      bc = c;
      bs = s;
    }
  }
  nc = wave_sum(nc);
  na = wave_sum(na);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const int oc = __shfl_xor(bc, off, 64), os = __shfl_xor(bs, off, 64);
    if (spfe_cv_max_beats(oc, os, bc, bs)) {
      bc = oc;
      bs = os;
    }
  }
  if (lane == 0) {
    wn[wave] = nc;
    wa[wave] = na;
    wc[wave] = bc;
    ws[wave] = bs;
  }
  __syncthreads();
  nc = 0, na = 0, bc = 0, bs = -1;
#pragma unroll
  for (int w = 0; w < CV_WAVES; ++w) {   // every thread: the same result
    nc += wn[w];
    na += wa[w];
    if (spfe_cv_max_beats(wc[w], ws[w], bc, bs)) {
      bc = wc[w];
      bs = ws[w];
    }
  }
  // the zeros behind the last array
  {
    const size_t end = SPFE_COVIS_OFF_LINKED_CODE(n, cap) + 4 * (size_t)cap, all = SPFE_COVIS_OUT_BYTES(n, cap);
    for (size_t b = end + tid; b < all; b += CV_WG) a.out[b] = 0;
  }
  const int status = nc == 0 ? SPFE_COVIS_NO_SHARED : (nc > cap ? SPFE_COVIS_CUR_OVERFLOW : 0);
  if (status) {   // (2): uniform; no state changes, and the neighbour kernel finds n_linked = 0
    for (int j = tid; j < cap; j += CV_WG) {
      linked_slot[j] = -1;
      linked_code[j] = -1;
    }
    if (tid == 0) {
      hdr[SPFE_COVIS_OFF_STATUS / 4] = status;
      hdr[SPFE_COVIS_OFF_N_COUNTER / 4] = nc;
      hdr[SPFE_COVIS_OFF_N_LINKED / 4] = 0;
      hdr[SPFE_COVIS_OFF_N_CHANGED / 4] = 0;
      hdr[SPFE_COVIS_OFF_N_OVERFLOW / 4] = 0;
      hdr[SPFE_COVIS_OFF_MAX_SLOT / 4] = bs;
      hdr[SPFE_COVIS_OFF_MAX_COUNT / 4] = bc;
      hdr[SPFE_COVIS_OFF_PARENT_SET / 4] = -1;
    }
    return;
  }

  // (5) conn[cur] and (3) P, both in slot order; a thread reads back the counters it stored itself
  int *cs = a.conn_slot + (size_t)cur * cap, *cw = a.conn_w + (size_t)cur * cap;
  int at_c = 0, at_p = 0;
  for (int base = 0; base < n; base += CV_WG) {
    const int s = base + tid;
    const int c = s < n ? counter[s] : 0;
    const bool fc = c > 0, fp = fc && spfe_cv_linked(c, s, th, na, bs);
    int total;
    const int r = wg_ordered_offset<CV_WG>((fc ? 1 : 0) | (fp ? 1 << 16 : 0), wcnt, &total);   // two counts of at most 1024 each
    if (fc) {
      const int rc = at_c + (r & 0xffff);
      cs[rc] = s;   // at_c ends at nc <= cap
      cw[rc] = c;
    }
    if (fp) {
      const int rp = at_p + (r >> 16);
      linked_slot[rp] = s;
      key[rp] = spfe_cv_key(c, s);
    }
    at_c += total & 0xffff;
    at_p += total >> 16;
  }
  const int n_linked = at_p;   // 1 <= n_linked <= nc
  for (int j = nc + tid; j < cap; j += CV_WG) {
    cs[j] = -1;
    cw[j] = 0;
  }
  for (int j = n_linked + tid; j < cap; j += CV_WG) {
    linked_slot[j] = -1;
    linked_code[j] = -1;
  }
  const int n2 = cv_pow2(n_linked);
  for (int j = n_linked + tid; j < n2; j += CV_WG) key[j] = SPFE_COVIS_KEY_NONE;
  __syncthreads();
  cv_sort_desc(key, n2);
  int *os = a.ord_slot + (size_t)cur * cap, *ow = a.ord_w + (size_t)cur * cap;
  for (int j = tid; j < cap; j += CV_WG) {
    os[j] = j < n_linked ? spfe_cv_key_slot(key[j]) : -1;
    ow[j] = j < n_linked ? spfe_cv_key_w(key[j]) : 0;
  }
  cv_table_row(a.best_a, a.n_best_a, cur, key, n_linked);   // (7)
  cv_table_row(a.best_b, a.n_best_b, cur, key, n_linked);
  if (tid == 0) {
    a.conn_n[cur] = nc;
    a.ord_n[cur] = n_linked;
    int parent_set = -1;
    if (a.first_conn[cur] && cur != a.origin_slot) {   // (6)
      parent_set = spfe_cv_key_slot(key[0]);
      a.parent[cur] = parent_set;
      a.first_conn[cur] = 0;
    }
    hdr[SPFE_COVIS_OFF_STATUS / 4] = 0;
    hdr[SPFE_COVIS_OFF_N_COUNTER / 4] = nc;
    hdr[SPFE_COVIS_OFF_N_LINKED / 4] = n_linked;
    hdr[SPFE_COVIS_OFF_N_CHANGED / 4] = 0;
    hdr[SPFE_COVIS_OFF_N_OVERFLOW / 4] = 0;
    hdr[SPFE_COVIS_OFF_MAX_SLOT / 4] = bs;
    hdr[SPFE_COVIS_OFF_MAX_COUNT / 4] = bc;
    hdr[SPFE_COVIS_OFF_PARENT_SET / 4] = parent_set;
  }
}

__global__ __launch_bounds__(CV_WG) void cv_neigh_kernel(CovisArgs a) {
  __shared__ int64_t key[SPFE_COVIS_MAX_CONN];
  __shared__ int sh_found, sh_less;
  const int tid = threadIdx.x, lane = tid & 63, n = a.n_slots, cur = a.cur_slot, cap = a.conn_cap;
  int *hdr = reinterpret_cast<int *>(a.out);
  const int *counter = reinterpret_cast<const int *>(a.out + SPFE_COVIS_OFF_COUNTER);
  const int *linked_slot = reinterpret_cast<const int *>(a.out + SPFE_COVIS_OFF_LINKED_SLOT(n));
  int *linked_code = reinterpret_cast<int *>(a.out + SPFE_COVIS_OFF_LINKED_CODE(n, cap));
  int n_linked = hdr[SPFE_COVIS_OFF_N_LINKED / 4];
  n_linked = n_linked < cap ? n_linked : cap;
  for (int j = blockIdx.x; j < n_linked; j += gridDim.x) {   // uniform over the workgroup
    const int s = linked_slot[j], w = counter[s];
    int *cs = a.conn_slot + (size_t)s * cap, *cw = a.conn_w + (size_t)s * cap;
    int cn = a.conn_n[s];
    cn = cn < 0 ? 0 : (cn > cap ? cap : cn);
    if (tid == 0) {
      sh_found = -1;
      sh_less = 0;
    }
    __syncthreads();
    int less = 0;
    for (int i = tid; i < cn; i += CV_WG) {
      const int t = cs[i];
      key[i] = spfe_cv_key(cw[i], t);
      if (t == cur) sh_found = i;   // the slots of a row are unique: at most one thread
      less += t < cur;
    }
    less = wave_sum(less);
    if (lane == 0 && less) atomicAdd(&sh_less, less);
    __syncthreads();
    const int found = sh_found, pos = sh_less;
    const int code = spfe_cv_add_code(found >= 0, found >= 0 ? spfe_cv_key_w(key[found]) : 0, w, cn, cap);
    int n1 = cn;
    if (code == SPFE_COVIS_CODE_REPLACED) {
      if (tid == 0) {
        key[found] = spfe_cv_key(w, cur);
        cw[found] = w;
      }
    } else if (code == SPFE_COVIS_CODE_INSERTED) {   // cn < cap
      for (int i = pos + tid; i < cn; i += CV_WG) {   // the tail one place up, from the LDS copy
        cs[i + 1] = spfe_cv_key_slot(key[i]);
        cw[i + 1] = spfe_cv_key_w(key[i]);
      }
      if (tid == 0) {
        cs[pos] = cur;
        cw[pos] = w;
        key[cn] = spfe_cv_key(w, cur);
        a.conn_n[s] = cn + 1;
      }
      n1 = cn + 1;
    }
    if (code == SPFE_COVIS_CODE_REPLACED || code == SPFE_COVIS_CODE_INSERTED) {
      const int n2 = cv_pow2(n1);
      for (int i = n1 + tid; i < n2; i += CV_WG) key[i] = SPFE_COVIS_KEY_NONE;
      __syncthreads();
      cv_sort_desc(key, n2);
      int *os = a.ord_slot + (size_t)s * cap, *ow = a.ord_w + (size_t)s * cap;
      for (int i = tid; i < n1; i += CV_WG) {
        os[i] = spfe_cv_key_slot(key[i]);
        ow[i] = spfe_cv_key_w(key[i]);
      }
      cv_table_row(a.best_a, a.n_best_a, s, key, n1);
      cv_table_row(a.best_b, a.n_best_b, s, key, n1);
      if (tid == 0) a.ord_n[s] = n1;
    }
    if (tid == 0) {
      linked_code[j] = code;
      if (code == SPFE_COVIS_CODE_REPLACED || code == SPFE_COVIS_CODE_INSERTED) atomicAdd(&hdr[SPFE_COVIS_OFF_N_CHANGED / 4], 1);
      if (code == SPFE_COVIS_CODE_FULL) {
        atomicAdd(&hdr[SPFE_COVIS_OFF_N_OVERFLOW / 4], 1);
        atomicOr(&hdr[SPFE_COVIS_OFF_STATUS / 4], SPFE_COVIS_NEIGH_OVERFLOW);
      }
    }
    __syncthreads();   // the keys are the next neighbour's from here on
  }
}

size_t covis_scratch_bytes(int n_table, int n_slots) { return pad16(8 * (size_t)n_slots) + localmap_scratch_bytes(n_table); }

hipError_t launch_covis_reset(const CovisArgs &a, int first_slot, int n, hipStream_t s) {
  if (a.conn_cap < 1 || a.conn_cap > SPFE_COVIS_MAX_CONN || first_slot < 0 || n < 1 || first_slot > a.n_slots - n)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(cv_reset_kernel, dim3(groups_for((size_t)n * a.conn_cap, 256, 1024)), dim3(256), 0, s, a, first_slot, n);
  return hipGetLastError();
}

hipError_t launch_covis(const CovisArgs &a, hipStream_t s) {
  if (a.conn_cap < 1 || a.conn_cap > SPFE_COVIS_MAX_CONN || a.cur_slot < 0 || a.cur_slot >= a.n_slots || a.th < 1 || !a.out ||
      (a.best_a && (a.n_best_a < 1 || a.n_best_a > SPFE_LOCALMAP_MAX_BEST)) ||
      (a.best_b && (a.n_best_b < 1 || a.n_best_b > SPFE_LOCALMAP_MAX_BEST)))
    return hipErrorInvalidValue;
  const CvScratch sc = cv_scratch(a.scratch, a.n_slots);
  LocalmapArgs v{};
  v.kf_mp_of_kp = a.kf_mp_of_kp;
  v.kp_stride = a.kp_stride;
  v.n_slots = a.n_slots;
  v.mp_flags = a.mp_flags;
  v.n_table = a.n_table;
  v.mp_of_kp = a.kf_mp_of_kp + (size_t)a.cur_slot * a.kp_stride;   // the frame is the keyframe's own row
  v.n_kp = a.kp_stride;
  v.votes = sc.votes;
  v.total = sc.total;
  v.scratch = sc.lm;
  hipError_t e = launch_localmap_count_row(v, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cv_current_kernel, dim3(1), dim3(CV_WG), 0, s, a);
  hipLaunchKernelGGL(cv_neigh_kernel, dim3(CV_NEIGH_GRID), dim3(CV_WG), 0, s, a);
  return hipGetLastError();
}

}  // namespace spfe
