// wave_ops.h — the wavefront and workgroup primitives of the solvers (dust.hip, pose.hip, sim3opt.hip, ba.hip, essgraph.hip), of the
// graph and table kernels (mappoint.hip, loopdet.hip, localmap.hip, covis.hip, cull.hip, mpcull.hip, lba.hip, newkf.hip) and of every ordered compaction
// (wave_search.h's callers, tri.hip, sim3.hip): reductions, the double tree, ordered ranks, barriers, the agent-scope relaxed load
// and store, padding.  (The walk over a keyframe row, the grid of a launcher and the integer clamp of the resident-state kernels are
// resident_rows.h, which a plain C++ compiler includes as well.)  Everything here is
// inlined into its kernel and holds no arithmetic of any contract; the SHAPE of the double tree is part of the exact-math contract
// (SPFE_DUST_SLOTS: slot = thread, halving tree per wavefront, the four wavefronts in order — the host references in tests/*_ref
// follow it), so it stands here once.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace spfe {

// v up to the next multiple of 16 (scratch carving, LDS layouts: host and device agree)
__host__ __device__ inline size_t pad16(size_t v) { return (v + 15) / 16 * 16; }

// ---- integers -------------------------------------------------------------------------------------------------------------------
// the wavefront's sum, the same in every lane
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ uint64_t ck_shfl_xor_u64(uint64_t v, int off) {
  const int lo = __shfl_xor((int)(uint32_t)v, off, 64), hi = __shfl_xor((int)(uint32_t)(v >> 32), off, 64);
  return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}

// ---- the double tree ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double xchg(double v, int m) { return __shfl_xor(v, m, 64); }
// lane L's value (L a constant) as a wavefront-uniform scalar
__device__ __forceinline__ double bcast(double v, int L) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), L), __builtin_amdgcn_readlane(__double2loint(v), L));
}

// the halving tree of one wavefront over one quantity: the same bits in every lane (both operands of every level's sum are swapped)
__device__ __forceinline__ double wave_tree(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = v + xchg(v, m);
  return v;
}

// one reduce-scatter level over CNT live values: keep one half, send the other to lane ^ m, add what arrives
template <int CNT>
__device__ __forceinline__ void rs_level(double (&v)[32], int m, bool hi) {
#pragma unroll
  for (int i = 0; i < CNT / 2; ++i) {
    const double keep = hi ? v[i + CNT / 2] : v[i];
    const double send = hi ? v[i] : v[i + CNT / 2];
    v[i] = keep + xchg(send, m);
  }
}

// The halving tree of one wavefront over up to 32 quantities at once, as a reduce-scatter butterfly: at the level with partner
// lane ^ m a lane keeps one half of its values and sends the other, so the six levels cost 16 + 8 + 4 + 2 + 1 + 1 = 32 exchanges
// instead of 6 x 32.  Lane l ends up with the wavefront's total of quantity l >> 1 in v[0] (the caller stores the even lanes').
// No barrier in here: the caller stores, synchronises, and adds the wavefronts' partials with sum4_ordered.
__device__ __forceinline__ void wave_tree_scatter32(double (&v)[32], int lane) {
  rs_level<32>(v, 32, lane & 32);
  rs_level<16>(v, 16, lane & 16);
  rs_level<8>(v, 8, lane & 8);
  rs_level<4>(v, 4, lane & 4);
  rs_level<2>(v, 2, lane & 2);
  v[0] = v[0] + xchg(v[0], 1);
}

// the four wavefronts' partials of one quantity, `stride` doubles apart, added in wavefront order
__device__ __forceinline__ double sum4_ordered(const double *p, int stride) {
  return ((p[0] + p[stride]) + p[2 * stride]) + p[3 * stride];
}

// ---- barriers and fences --------------------------------------------------------------------------------------------------------
// LDS written by some lanes of a wavefront, read by others of the same one: no other wavefront is waited for
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// global scratch written by some threads of a workgroup, read by others of the same one
__device__ __forceinline__ void block_fence_sync() {
  __threadfence_block();
  __syncthreads();
}

// an int32 that atomics of other workgroups (or of this one, earlier in the kernel) change: read and written past the vector cache
__device__ __forceinline__ int load_agent(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void store_agent(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- ordered ranks of a workgroup of WG threads ---------------------------------------------------------------------------------
// The flag form, ONE barrier.  The number of set votes in the threads below this one — ballot + popcount inside a wavefront, the
// WG / 64 wavefront totals through LDS — and in *total that of the whole chunk (the same in every thread).  A caller that walks
// several chunks carries the totals and puts a barrier behind each chunk's use of the result: wave_total is rewritten by the next
// one.
template <int WG>
__device__ __forceinline__ int wg_ordered_rank(bool vote, int lane, int wave, int *wave_total, int *total) {
  const unsigned long long votes = __ballot(vote);
  const int rank = __popcll(votes & ((1ull << lane) - 1ull));
  if (lane == 0) wave_total[wave] = __popcll(votes);
  __syncthreads();
  int below = 0, sum = 0;
#pragma unroll
  for (int w = 0; w < WG / 64; ++w) {
    const int c = wave_total[w];
    below += w < wave ? c : 0;
    sum += c;
  }
  *total = sum;
  return below + rank;
}

// The count form, TWO barriers: where this thread's c entries go among the workgroup's, in thread order, and the count of all of
// them.  The second barrier is inside, so wcnt may be rewritten at once; a caller may pack two counts into c as long as neither
// field's workgroup total overflows into the next.
template <int WG>
__device__ __forceinline__ int wg_ordered_offset(int c, int *wcnt, int *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = c;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int up = __shfl_up(incl, off, 64);
    if (lane >= off) incl += up;
  }
  if (lane == 63) wcnt[wave] = incl;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < WG / 64; ++w) {
    const int k = wcnt[w];
    before += w < wave ? k : 0;
    all += k;
  }
  __syncthreads();
  *total = all;
  return before + incl - c;
}

}  // namespace spfe
