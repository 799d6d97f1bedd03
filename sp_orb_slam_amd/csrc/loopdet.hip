// loopdet.hip — the loop detection on the device: LoopClosingVLAD::detectLoopCandidates (loop_closer_vlad.cpp:42-118) and the
// minimum score of detectLoopVLAD (:150-165) for one query keyframe, on the caller's resident table of global descriptors.  The
// arithmetic is include/spfe_loopdet_math.h; the host statement the tests hold these kernels to is tests/loopdet_ref/loopdet_ref.c:
// the whole block is equal bit for bit.
//
//   loopdet_mark_kernel     one workgroup: a role byte per slot in LDS (four a word) from d_in_db, then the two lists by LDS
//                           atomics (connected clears the retrieval bit, covisible and not bad sets the other), then role[], the
//                           no-score bits of the slots without a role, n_scored and the status bit of a bad list entry.
//   loopdet_score_kernel    256 threads = the 256 slots of the contract's sum.  A workgroup holds the query in registers (thread t:
//                           elements 1024 p + 4 t .. + 3 of pass p, 16 f32 at dim 4096) and grid-strides over groups of LD_ROWS
//                           = 2 consecutive slots: all 16-byte loads of the group's rows with a role are issued before the first
//                           product (8 a thread in flight, four workgroups a CU), each thread adds its elements of a row to 0.0
//                           in f64 in ascending order, and wavefront r runs the halving tree of row r: two levels out of LDS,
//                           six by shuffles.  A row is read once.  (Measured at 10,000 x 4096: 2 rows a group 40 us, 4 rows —
//                           170 VGPRs, two workgroups a CU — 61 us, 8 rows 100 us, 1 row on four times the grid 38 us.)
//   loopdet_decide_kernel   one workgroup, as many passes over the lists as they need: the covisible minimum, min_score, the
//                           ordered compaction of the slots that pass (four consecutive slots a thread, a scan over the wavefront,
//                           a prefix over the wavefronts' counts), the accumulation with a thread per entry and the neighbours in
//                           row order, best_acc_score as a (value, position) max-reduction that a NaN never wins,
//                           min_score_to_retain, the first occurrence of every best keyframe by atomicMin of the position, and
//                           the ordered compaction into the candidate list.
// Nothing synchronises with the host, and only plain vector stores and vector atomics write.
#include "../../include/spfe.h"
#include "../../include/spfe_loopdet_math.h"
#include "spfe_kernels.h"
#include "wave_ops.h"

#include <limits.h>

static_assert(SPFE_GLOBAL_DESC_DIM == SPFE_LOOPDET_MAX_DIM, "dim");

namespace spfe {

namespace {
constexpr int LD_WG = SPFE_LOOPDET_TREE_SLOTS;                              // score: a thread per slot of the sum
constexpr int LD_ROWS = 2;                                                  // rows a group; wavefront r runs the tree of row r
constexpr int LD_PASSES = SPFE_LOOPDET_MAX_DIM / SPFE_LOOPDET_PASS_ELEMS;   // float4 of a row a thread holds
constexpr int LD_SCORE_GRID = 1024;                                         // four workgroups a CU (106 VGPRs)
constexpr int LD_ONE = 1024;                                                // mark and decide: one workgroup
constexpr int LD_ONE_WAVES = LD_ONE / 64;
constexpr int LD_NONE = INT_MAX;
static_assert(LD_WG == 256 && LD_ROWS * 64 <= LD_WG && SPFE_LOOPDET_MAX_KEYFRAMES % 4 == 0, "shapes");

// role and score of the four slots 4 i .. 4 i + 3 (a role of 0 beyond the table): one 4-byte and one 16-byte load inside it
__device__ __forceinline__ void ld_quad(const uint8_t *role, const float *score, int n, int i, unsigned r[4], float sc[4]) {
  const int s0 = 4 * i;
  if (s0 + 3 < n) {
    const unsigned r4 = *reinterpret_cast<const unsigned *>(role + s0);
    const float4 v = *reinterpret_cast<const float4 *>(score + s0);
    r[0] = r4 & 0xffu; r[1] = (r4 >> 8) & 0xffu; r[2] = (r4 >> 16) & 0xffu; r[3] = r4 >> 24;
    sc[0] = v.x; sc[1] = v.y; sc[2] = v.z; sc[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      r[j] = s0 + j < n ? role[s0 + j] : 0u;
      sc[j] = s0 + j < n ? score[s0 + j] : 0.0f;
    }
  }
}

// (value, index) a before (value, index) b: the greater (MAX) or lesser value, the lower index among equal values; LD_NONE = no value
template <bool MAX>
__device__ __forceinline__ bool ld_beats(float av, int ai, float bv, int bi) {
  if (ai == LD_NONE) return false;
  if (bi == LD_NONE) return true;
  return (MAX ? spfe_ld_raises(av, bv) : spfe_ld_lowers(av, bv)) || (av == bv && ai < bi);
}

// the first of the workgroup's pairs in that order, in every thread; two barriers
template <bool MAX>
__device__ __forceinline__ void ld_reduce(float *v, int *i, float *wv, int *wi) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(*v, off, 64);
    const int oi = __shfl_xor(*i, off, 64);
    if (ld_beats<MAX>(ov, oi, *v, *i)) {
      *v = ov;
      *i = oi;
    }
  }
  if (lane == 0) {
    wv[wave] = *v;
    wi[wave] = *i;
  }
  __syncthreads();
  float rv = wv[0];
  int ri = wi[0];
#pragma unroll
  for (int w = 1; w < LD_ONE_WAVES; ++w)
    if (ld_beats<MAX>(wv[w], wi[w], rv, ri)) {
      rv = wv[w];
      ri = wi[w];
    }
  __syncthreads();
  *v = rv;
  *i = ri;
}
}  // namespace

__global__ __launch_bounds__(LD_ONE) void loopdet_mark_kernel(LoopdetArgs a) {
  __shared__ unsigned role4[SPFE_LOOPDET_MAX_KEYFRAMES / 4];   // a byte per slot
  __shared__ int wcnt[LD_ONE_WAVES];
  const int n = a.n_slots, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int w = threadIdx.x; w < (n + 3) / 4; w += LD_ONE) {
    unsigned v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int s = 4 * w + k;
      if (s < n && s != a.cur_slot && a.in_db[s]) v |= (unsigned)SPFE_LOOPDET_ROLE_DB << (8 * k);
    }
    role4[w] = v;
  }
  __syncthreads();
  int bad = 0;
  for (int i = threadIdx.x; i < a.n_conn; i += LD_ONE) {
    const int s = a.connected[i];
    if (s < 0 || s >= n)
      bad = 1;   // not followed
    else
      atomicAnd(&role4[s >> 2], ~((unsigned)SPFE_LOOPDET_ROLE_DB << (8 * (s & 3))));
  }
  for (int i = threadIdx.x; i < a.n_cov; i += LD_ONE) {
    const int s = a.covisible[i];
    if (s < 0 || s >= n)
      bad = 1;
    else if (!(a.kf_flags[s] & 1))
      atomicOr(&role4[s >> 2], (unsigned)SPFE_LOOPDET_ROLE_COV << (8 * (s & 3)));
  }
  const int any_bad = __syncthreads_or(bad);
  uint8_t *role = a.out + SPFE_LOOPDET_OFF_ROLE(n);
  unsigned *score_bits = reinterpret_cast<unsigned *>(a.out + SPFE_LOOPDET_OFF_SCORE);
  int cnt = 0;
  for (int s = threadIdx.x; s < n; s += LD_ONE) {
    const unsigned r = (role4[s >> 2] >> (8 * (s & 3))) & 0xffu;
    role[s] = (uint8_t)r;
    if (!r) score_bits[s] = SPFE_LOOPDET_NO_SCORE_BITS;
    cnt += r != 0;
  }
  cnt = wave_sum(cnt);
  if (lane == 0) wcnt[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    cnt = 0;
    for (int w = 0; w < LD_ONE_WAVES; ++w) cnt += wcnt[w];
    int *h = reinterpret_cast<int *>(a.out);
    h[0] = any_bad ? SPFE_LOOPDET_BAD_LIST_INDEX : 0;
    h[1] = cnt;
  }
}

__global__ __launch_bounds__(LD_WG) void loopdet_score_kernel(LoopdetArgs a) {
  __shared__ double part[LD_ROWS][LD_WG];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int n = a.n_slots, dim = a.dim;
  const uint8_t *role = a.out + SPFE_LOOPDET_OFF_ROLE(n);
  float *score = reinterpret_cast<float *>(a.out + SPFE_LOOPDET_OFF_SCORE);
  const float *qrow = a.gdesc + (size_t)a.cur_slot * dim;
  float4 q[LD_PASSES];
#pragma unroll
  for (int p = 0; p < LD_PASSES; ++p) {
    const int e = p * SPFE_LOOPDET_PASS_ELEMS + 4 * t;
    q[p] = e < dim ? *reinterpret_cast<const float4 *>(qrow + e) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  const int groups = (n + LD_ROWS - 1) / LD_ROWS;
  for (int g = blockIdx.x; g < groups; g += gridDim.x) {
    float4 v[LD_ROWS][LD_PASSES];
    bool has[LD_ROWS];   // block-uniform
#pragma unroll
    for (int r = 0; r < LD_ROWS; ++r) {
      const int s = g * LD_ROWS + r;
      has[r] = s < n && role[s] != 0;
      const float *row = a.gdesc + (size_t)(has[r] ? s : 0) * dim;
#pragma unroll
      for (int p = 0; p < LD_PASSES; ++p) {
        const int e = p * SPFE_LOOPDET_PASS_ELEMS + 4 * t;
        v[r][p] = has[r] && e < dim ? *reinterpret_cast<const float4 *>(row + e) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      }
    }
#pragma unroll
    for (int r = 0; r < LD_ROWS; ++r) {
      double acc = 0.0;
#pragma unroll
      for (int p = 0; p < LD_PASSES; ++p)
        if (p * SPFE_LOOPDET_PASS_ELEMS + 4 * t < dim) {
          const float qa[4] = {q[p].x, q[p].y, q[p].z, q[p].w}, va[4] = {v[r][p].x, v[r][p].y, v[r][p].z, v[r][p].w};
          acc = spfe_ld_add4(acc, qa, va);
        }
      part[r][t] = acc;
    }
    __syncthreads();
    const int sw = g * LD_ROWS + wave;
    if (wave < LD_ROWS && sw < n && role[sw] != 0) {   // wave-uniform
      const double *sp = part[wave];
      double x = (sp[lane] + sp[lane + 128]) + (sp[lane + 64] + sp[lane + 192]);   // m = 128, then m = 64
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) x = x + __shfl_down(x, m, 64);             // lane l < m holds s[l]
      if (lane == 0) score[sw] = (float)x;
    }
    __syncthreads();   // part is the next group's
  }
}

__global__ __launch_bounds__(LD_ONE) void loopdet_decide_kernel(LoopdetArgs a) {
  __shared__ int wcnt[LD_ONE_WAVES];
  __shared__ float wv[LD_ONE_WAVES];
  __shared__ int wi[LD_ONE_WAVES];
  const int n = a.n_slots, tid = threadIdx.x;
  const uint8_t *role = a.out + SPFE_LOOPDET_OFF_ROLE(n);
  const float *score = reinterpret_cast<const float *>(a.out + SPFE_LOOPDET_OFF_SCORE);
  int *pass_slot = reinterpret_cast<int *>(a.out + SPFE_LOOPDET_OFF_PASS_SLOT(n));
  float *acc_score = reinterpret_cast<float *>(a.out + SPFE_LOOPDET_OFF_ACC_SCORE(n));
  int *best_slot = reinterpret_cast<int *>(a.out + SPFE_LOOPDET_OFF_BEST_SLOT(n));
  int *cand_slot = reinterpret_cast<int *>(a.out + SPFE_LOOPDET_OFF_CAND_SLOT(n));
  float *cand_acc = reinterpret_cast<float *>(a.out + SPFE_LOOPDET_OFF_CAND_ACC(n));
  int *first_pos = reinterpret_cast<int *>(a.out + SPFE_LOOPDET_OFF_FIRST_POS(n));

  // the covisible minimum and min_score
  float cv = spfe_ld_inf();
  int ci = LD_NONE;
  const int quads = (n + 3) / 4;
  for (int i = tid; i < quads; i += LD_ONE) {   // a thread's slots ascend
    unsigned r[4];
    float sc[4];
    ld_quad(role, score, n, i, r, sc);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if ((r[j] & SPFE_LOOPDET_ROLE_COV) && spfe_ld_lowers(sc[j], cv)) {
        cv = sc[j];
        ci = 4 * i + j;
      }
  }
  ld_reduce<false>(&cv, &ci, wv, wi);
  const float cov_min = ci == LD_NONE ? spfe_ld_inf() : cv;
  const float min_score = spfe_ld_min_score(a.min_score_init, cov_min, a.min_score_floor);

  // the slots that pass, ascending
  int n_pass = 0;
  for (int base = 0; base < quads; base += LD_ONE) {   // four consecutive slots a thread, 4096 a pass
    unsigned r[4];
    float sc[4];
    ld_quad(role, score, n, base + tid, r, sc);
    bool f[4];
    int c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f[j] = (r[j] & SPFE_LOOPDET_ROLE_DB) && spfe_ld_passes(sc[j], min_score);
      c += f[j];
    }
    int total;
    int at = n_pass + wg_ordered_offset<LD_ONE>(c, wcnt, &total);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (f[j]) pass_slot[at++] = 4 * (base + tid) + j;
    n_pass += total;
  }
  __syncthreads();

  // accumulation over the best covisibles, a thread per entry
  float bv = 0.0f;
  int bp = LD_NONE, bad_nb = 0;
  for (int p = tid; p < n_pass; p += LD_ONE) {
    const int s = pass_slot[p];
    const float own = score[s];
    float acc = own, best = own;
    int bs = s;
    const int *row = a.best_cov + (size_t)s * SPFE_LOOPDET_NEIGH;
    // the row, then the ten roles and scores, as three rounds of independent loads; the sum itself runs in row order
    int nbs[SPFE_LOOPDET_NEIGH];
    uint8_t nrole[SPFE_LOOPDET_NEIGH];
    float nscore[SPFE_LOOPDET_NEIGH];
#pragma unroll
    for (int k = 0; k < SPFE_LOOPDET_NEIGH; ++k) nbs[k] = row[k];
#pragma unroll
    for (int k = 0; k < SPFE_LOOPDET_NEIGH; ++k) {
      const int safe = nbs[k] >= 0 && nbs[k] < n ? nbs[k] : s;   // an entry outside the table is not followed
      nrole[k] = role[safe];
      nscore[k] = score[safe];
    }
#pragma unroll
    for (int k = 0; k < SPFE_LOOPDET_NEIGH; ++k) {
      const int nb = nbs[k];
      if (nb < 0 || nb >= n) {
        bad_nb |= nb != -1;
        continue;
      }
      if (!(nrole[k] & SPFE_LOOPDET_ROLE_DB)) continue;
      const float sc = nscore[k];
      if (!spfe_ld_passes(sc, min_score)) continue;
      acc = acc + sc;
      if (spfe_ld_raises(sc, best)) {
        best = sc;
        bs = nb;
      }
    }
    acc_score[p] = acc;
    best_slot[p] = bs;
    if (acc == acc && (bp == LD_NONE || spfe_ld_raises(acc, bv))) {
      bv = acc;
      bp = p;
    }
  }
  ld_reduce<true>(&bv, &bp, wv, wi);
  const int any_bad_nb = __syncthreads_or(bad_nb);
  const float best_acc = bp != LD_NONE && spfe_ld_raises(bv, min_score) ? bv : min_score;
  const float retain = spfe_ld_retain(a.retain_ratio, best_acc);

  // the first retained entry of every best keyframe: the preset, the atomicMin and the read behind it are all atomic operations
  // of agent scope on the same word, ordered by the barriers between them
  for (int s = tid; s < n; s += LD_ONE) __hip_atomic_store(&first_pos[s], LD_NONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  for (int p = tid; p < n_pass; p += LD_ONE)
    if (spfe_ld_passes(acc_score[p], retain)) atomicMin(&first_pos[best_slot[p]], p);
  __syncthreads();
  int n_cand = 0;
  for (int base = 0; base < n_pass; base += LD_ONE) {
    const int p = base + tid;
    bool f = p < n_pass && spfe_ld_passes(acc_score[p], retain);
    if (f) f = __hip_atomic_load(&first_pos[best_slot[p]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == p;
    int total;
    const int r = wg_ordered_offset<LD_ONE>(f ? 1 : 0, wcnt, &total);
    if (f) {
      cand_slot[n_cand + r] = best_slot[p];
      cand_acc[n_cand + r] = acc_score[p];
    }
    n_cand += total;
  }
  if (tid == 0) {
    int *h = reinterpret_cast<int *>(a.out);
    float *hf = reinterpret_cast<float *>(a.out + SPFE_LOOPDET_OFF_COV_MIN_SCORE);
    h[0] = h[0] | (any_bad_nb ? SPFE_LOOPDET_BAD_NEIGHBOUR : 0);
    h[2] = n_pass;
    h[3] = n_cand;
    hf[0] = cov_min;
    hf[1] = min_score;
    hf[2] = best_acc;
    hf[3] = retain;
  }
}

hipError_t launch_loopdet(const LoopdetArgs &a, hipStream_t s) {
  if (a.n_slots < 1 || a.n_slots > SPFE_LOOPDET_MAX_KEYFRAMES || a.dim < 4 || a.dim > SPFE_GLOBAL_DESC_DIM || a.dim % 4 ||
      a.cur_slot < 0 || a.cur_slot >= a.n_slots || a.n_conn < 0 || a.n_conn > a.n_slots || a.n_cov < 0 || a.n_cov > a.n_slots)
    return hipErrorInvalidValue;
  const int groups = (a.n_slots + LD_ROWS - 1) / LD_ROWS;
  hipLaunchKernelGGL(loopdet_mark_kernel, dim3(1), dim3(LD_ONE), 0, s, a);
  hipLaunchKernelGGL(loopdet_score_kernel, dim3(groups < LD_SCORE_GRID ? groups : LD_SCORE_GRID), dim3(LD_WG), 0, s, a);
  hipLaunchKernelGGL(loopdet_decide_kernel, dim3(1), dim3(LD_ONE), 0, s, a);
  return hipGetLastError();
}

}  // namespace spfe
