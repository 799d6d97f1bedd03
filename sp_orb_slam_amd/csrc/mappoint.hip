// mappoint.hip — the map-point table on the device: MapPoint::ComputeDistinctiveDescriptors (mappoint.cpp:237-302) and
// MapPoint::UpdateNormalAndDepth (:322-364) for m listed points, in place, from keyframe records resident in HBM, and the
// gather that turns table rows into the point list of the searches.  The arithmetic is include/spfe_mappoint_math.h; the host
// statement the tests hold these kernels to is tests/mp_ref/mp_ref.c: every output is equal bit for bit.
//
//   mp_refresh_kernel   a workgroup (four wavefronts) serves MP_CHUNK consecutive listed points.  First wavefront w takes points
//                       w, w + 4, ... of the chunk, one at a time: it walks the point's observations 64 per pass (indices are
//                       tested before they are followed), counts the good rows, sums the normal in observation order (the
//                       shares are formed 64 at a time, the f32 sum runs over them in order in every lane) and, where the point
//                       has at most MP_WAVE_OBS good rows, chooses the descriptor itself: row i in registers (16 bytes a lane,
//                       8 for bf16), row j from the record, the double butterfly of wave_search.h, the N distances of row i in
//                       one register per 64 of them, rank selection by counting over shuffles.  Nothing of size N x N exists.
//                       Then the workgroup takes the chunk's larger points one after the other: wavefront 0 compacts the good
//                       rows' addresses into LDS, the rows are staged in LDS once while they fit (bf16 rows as bf16), the four
//                       wavefronts share the rows i, and the per-wavefront bests are merged (least median, lowest row on a tie:
//                       what the ascending strict comparison gives).  Each pair is computed twice, once from either row: the
//                       distance is symmetric bit for bit, and a row's distances never leave the registers of its wavefront.
//   mp_header_kernel    one workgroup: the three sums of the block's header from the codes, and the OR of the records' status.
//   mp_gather_kernel    one wavefront per listed row: a copy.
// No output is read by the refresh, nothing synchronises with the host, and only plain vector stores write.
#include "../../include/spfe.h"
#include "../../include/spfe_mappoint_math.h"
#include "spfe_kernels.h"
#include "wave_search.h"

static_assert(SPFE_MP_R_SKIP_BAD == SPFE_MP_SKIP_BAD && SPFE_MP_R_NO_OBS == SPFE_MP_NO_OBS && SPFE_MP_R_INVALID == SPFE_MP_INVALID &&
              SPFE_MP_R_NO_GOOD_KF == SPFE_MP_NO_GOOD_KF && SPFE_MP_R_TOO_MANY == SPFE_MP_TOO_MANY &&
              SPFE_MP_R_REFRESHED == SPFE_MP_REFRESHED, "codes");

namespace spfe {

namespace {
constexpr int MP_WAVES = 4;
constexpr int MP_WG = MP_WAVES * 64;
constexpr int MP_CHUNK = SPFE_MP_CHUNK;
constexpr int MP_WAVE_OBS = SPFE_MP_WAVE_OBS;
constexpr int MP_MAX = SPFE_MP_MAX_OBS;
constexpr int MP_REGS = MP_MAX / 64;       // registers that hold one row's distances, 64 a register
constexpr int MP_STAGE_BYTES = 40 * 1024;  // rows staged in LDS: 40 f32 rows, 80 bf16 rows; three workgroups a CU
static_assert(MP_CHUNK % MP_WAVES == 0 && MP_WAVE_OBS <= 64 && MP_MAX % 64 == 0, "shapes");

// observation o of the walk: is it in a good keyframe, and where is its row.  Only called with indices the classification passed.
__device__ __forceinline__ bool mp_obs_good(const MpArgs &a, int e, const uint8_t **row) {
  if (!a.records) {
    *row = reinterpret_cast<const uint8_t *>(a.obs_desc + (size_t)e * 256);
    return a.obs_good[e] != 0;
  }
  const int slot = a.obs[2 * e], kp = a.obs[2 * e + 1];
  if (a.kf_flags[slot] & 1) return false;
  *row = a.records[slot] + a.off_desc + (size_t)kp * (a.desc_bf16 ? 512 : 1024);
  return true;
}

// steps 1 - 3 of listed point i and the count of its good rows; 0: the point passes.  Wave-uniform.
__device__ __forceinline__ int mp_classify(const MpArgs &a, int i, int lane, int *row, int *s, int *n_all, int *n_good) {
  *s = *n_all = *n_good = 0;
  const int r = a.point_idx ? a.point_idx[i] : i;
  *row = r;
  if (r < 0 || r >= a.n_table) return SPFE_MP_INVALID;
  if (!(a.flags[r] & SPFE_PROJ_SEARCHABLE)) return SPFE_MP_SKIP_BAD;
  const int s0 = a.obs_start[i], e0 = a.obs_start[i + 1];
  if (s0 < 0 || e0 > a.E || e0 < s0) return SPFE_MP_INVALID;
  if (e0 == s0) return SPFE_MP_NO_OBS;
  const int n = e0 - s0;
  bool bad = false;
  int good = 0;
  if (a.records) {
    const int rs = a.ref_slot[i];
    bad = rs < 0 || rs >= a.n_kf;
  }
  for (int base = 0; base < n; base += 64) {
    const int o = base + lane;
    bool g = false;
    if (o < n) {
      if (!a.records) {
        g = a.obs_good[s0 + o] != 0;
      } else {
        const int slot = a.obs[2 * (s0 + o)], kp = a.obs[2 * (s0 + o) + 1];
        if (slot < 0 || slot >= a.n_kf) {
          bad = true;
        } else {
          g = !(a.kf_flags[slot] & 1);
          const uint8_t *rec = a.records[slot];
          if (!rec) {
            bad |= g;
          } else {
            const int K = min(max(reinterpret_cast<const int *>(rec + a.off_hdr)[0], 0), a.kmax);
            bad |= kp < 0 || kp >= K;
          }
        }
      }
    }
    good += __popcll(__ballot(g));
  }
  if (__ballot(bad)) return SPFE_MP_INVALID;
  *s = s0;
  *n_all = n;
  *n_good = good;
  return 0;
}

// part (b) of one point by one wavefront; lane 0 writes
__device__ __forceinline__ void mp_normal_depth(const MpArgs &a, int i, int row, int s, int n_all, int lane) {
  const float P[3] = {a.xyz[3 * (size_t)row], a.xyz[3 * (size_t)row + 1], a.xyz[3 * (size_t)row + 2]};
  float sum[3] = {0.0f, 0.0f, 0.0f};
  for (int base = 0; base < n_all; base += 64) {
    const int o = base + lane;
    float c[3] = {0.0f, 0.0f, 0.0f};
    if (o < n_all) {
      float Ow[3];
      if (a.records) {
        float T[16];
        const float *src = a.Tcw + 16 * (size_t)a.obs[2 * (s + o)];
#pragma unroll
        for (int k = 0; k < 16; ++k) T[k] = src[k];
        spfe_proj_cam cam;
        spfe_proj_cam_from_f32(T, &cam);
        Ow[0] = cam.Ow[0]; Ow[1] = cam.Ow[1]; Ow[2] = cam.Ow[2];
      } else {
        const float *src = a.obs_Ow + 3 * (size_t)(s + o);
        Ow[0] = src[0]; Ow[1] = src[1]; Ow[2] = src[2];
      }
      spfe_mp_share(P, Ow, c);
    }
    const int cnt = min(64, n_all - base);
    for (int t = 0; t < cnt; ++t) {   // the sum in observation order, the same in every lane
      sum[0] = sum[0] + __shfl(c[0], t, 64);
      sum[1] = sum[1] + __shfl(c[1], t, 64);
      sum[2] = sum[2] + __shfl(c[2], t, 64);
    }
  }
  float Owr[3];
  if (a.records) {
    float T[16];
    const float *src = a.Tcw + 16 * (size_t)a.ref_slot[i];
#pragma unroll
    for (int k = 0; k < 16; ++k) T[k] = src[k];
    spfe_proj_cam cam;
    spfe_proj_cam_from_f32(T, &cam);
    Owr[0] = cam.Ow[0]; Owr[1] = cam.Ow[1]; Owr[2] = cam.Ow[2];
  } else {
    Owr[0] = a.ref_Ow[3 * (size_t)i]; Owr[1] = a.ref_Ow[3 * (size_t)i + 1]; Owr[2] = a.ref_Ow[3 * (size_t)i + 2];
  }
  float nrm[3], range[2];
  spfe_mp_normal_out(sum, n_all, nrm);
  spfe_mp_range(P, Owr, a.level_scale, a.top_scale, range);
  if (lane == 0) {
    a.normal[3 * (size_t)row] = nrm[0]; a.normal[3 * (size_t)row + 1] = nrm[1]; a.normal[3 * (size_t)row + 2] = nrm[2];
    a.dist_range[2 * (size_t)row] = range[0]; a.dist_range[2 * (size_t)row + 1] = range[1];
  }
}

// the good rows of a point, in observation order, into list_p / list_o (LDS) by ONE wavefront: at most cap entries are kept
__device__ __forceinline__ void mp_compact(const MpArgs &a, int s, int n_all, int lane, const uint8_t **list_p, int *list_o, int cap) {
  int cnt = 0;
  for (int base = 0; base < n_all; base += 64) {
    const int o = base + lane;
    const uint8_t *p = nullptr;
    const bool g = o < n_all && mp_obs_good(a, s + o, &p);
    const unsigned long long mask = __ballot(g);
    const int rank = cnt + __popcll(mask & ((1ull << lane) - 1ull));
    if (g && rank < cap) {
      list_p[rank] = p;
      list_o[rank] = o;
    }
    cnt += __popcll(mask);
  }
}

// what this lane holds of row j: elements 4 lane .. 4 lane + 3, from the staged copy (this workgroup's LDS) or from the record
template <bool STAGED>
__device__ __forceinline__ void mp_load4(const uint8_t *stage, const uint8_t *const *list_p, int j, int lane, int bf16, float f[4]) {
  float4 v;
  if (STAGED) {
    if (bf16) {
      const uint2 p = *reinterpret_cast<const uint2 *>(stage + (size_t)j * 512 + lane * 8);
      v = make_float4(__uint_as_float(p.x << 16), __uint_as_float(p.x & 0xffff0000u), __uint_as_float(p.y << 16),
                      __uint_as_float(p.y & 0xffff0000u));
    } else {
      v = *reinterpret_cast<const float4 *>(stage + (size_t)j * 1024 + lane * 16);
    }
  } else {
    v = desc4(reinterpret_cast<const float *>(list_p[j]), (size_t)lane * 4, bf16);
  }
  f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
}

// rows i0, i0 + step, ... of a point with N good rows by one wavefront: the least median and its row (-1: none took over)
template <bool STAGED>
__device__ __forceinline__ void mp_rows(const uint8_t *stage, const uint8_t *const *list_p, int N, int bf16, int lane, int i0, int step,
                                        float *best_out, int *besti_out) {
  float best = spfe_mp_best_init();
  int besti = -1;
  const int k = spfe_mp_median_rank(N);
  for (int i = i0; i < N; i += step) {
    float mf[4];
    mp_load4<STAGED>(stage, list_p, i, lane, bf16, mf);
    float dreg[MP_REGS];   // lane l of register c: D[i][64 c + l]
#pragma unroll
    for (int c = 0; c < MP_REGS; ++c) {
      dreg[c] = 0.0f;
      const int lim = min(64, N - 64 * c);
      for (int jj = 0; jj < lim; ++jj) {
        const int j = 64 * c + jj;
        float d = 0.0f;   // D[i][i] = 0 whatever the row holds
        if (j != i) {
          float kf[4];
          mp_load4<STAGED>(stage, list_p, j, lane, bf16, kf);
          double sum = spfe_proj_lane_sum(mf, kf);
#pragma unroll
          for (int off = 32; off >= 1; off >>= 1) sum = sum + __shfl_xor(sum, off, 64);
          d = spfe_proj_dist(sum);
        }
        if (lane == jj) dreg[c] = d;
      }
    }
    // the element of rank k by counting: lane l of register c is the candidate D[i][64 c + l]
    float median = 0.0f;
    bool found = false;
#pragma unroll
    for (int c = 0; c < MP_REGS; ++c) {
      if (64 * c < N && !found) {   // wave-uniform
        const float v = dreg[c];
        int nb = 0, ns = 0;
#pragma unroll
        for (int c2 = 0; c2 < MP_REGS; ++c2) {
          const int lim = min(64, N - 64 * c2);
          for (int t = 0; t < lim; ++t) {
            const float x = __shfl(dreg[c2], t, 64);
            nb += spfe_mp_before(x, v);
            ns += spfe_mp_same(x, v);
          }
        }
        const unsigned long long hit = __ballot(64 * c + lane < N && spfe_mp_is_rank(nb, ns, k));
        if (hit) {
          median = __shfl(v, __builtin_ctzll(hit), 64);
          found = true;
        }
      }
    }
    if (found && spfe_mp_takes_over(median, best)) {
      best = median;
      besti = i;
    }
  }
  *best_out = best;
  *besti_out = besti;
}

// the chosen row into the table and the block, by one wavefront
__device__ __forceinline__ void mp_write_desc(const MpArgs &a, int i, int row, const uint8_t *const *list_p, const int *list_o, float best,
                                              int besti, int lane) {
  const int b = besti < 0 ? 0 : besti;   // none took over: row 0 stays
  const float4 v = desc4(reinterpret_cast<const float *>(list_p[b]), (size_t)lane * 4, a.desc_bf16);
  *reinterpret_cast<float4 *>(a.desc + (size_t)row * 256 + lane * 4) = v;
  if (lane == 0) {
    reinterpret_cast<int *>(a.out + SPFE_MP_OFF_BEST_OBS)[i] = list_o[b];
    reinterpret_cast<float *>(a.out + SPFE_MP_OFF_BEST_MEDIAN(a.m))[i] = best;
  }
}
}  // namespace

int mp_lds_obs_capacity(int desc_elem_bytes) { return MP_STAGE_BYTES / (256 * desc_elem_bytes); }

__global__ __launch_bounds__(MP_WG) void mp_refresh_kernel(MpArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[MP_STAGE_BYTES];
  __shared__ const uint8_t *big_p[MP_MAX];
  __shared__ int big_o[MP_MAX];
  __shared__ const uint8_t *wave_p[MP_WAVES][MP_WAVE_OBS];
  __shared__ int wave_o[MP_WAVES][MP_WAVE_OBS];
  __shared__ int big_n[MP_CHUNK];   // 0: not a point of the second phase
  __shared__ float wbest[MP_WAVES];
  __shared__ int wbesti[MP_WAVES];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i_base = blockIdx.x * MP_CHUNK;
  const bool want_desc = a.mode & SPFE_MP_DESC, want_nd = a.mode & SPFE_MP_NORMAL_DEPTH;
  const int bf16 = a.desc_bf16;

  // ---- first phase: a wavefront per point ----
  for (int q = wave; q < MP_CHUNK; q += MP_WAVES) {   // wave-uniform
    const int i = i_base + q;
    int big = 0;
    if (i < a.m) {
      int row, s, n_all, n_good;
      int code = mp_classify(a, i, lane, &row, &s, &n_all, &n_good);
      if (!code) {
        code = spfe_mp_code(a.mode, n_good);
        if (want_nd) mp_normal_depth(a, i, row, s, n_all, lane);
      }
      const bool desc_now = want_desc && code == SPFE_MP_REFRESHED;
      if (lane == 0) {
        reinterpret_cast<int *>(a.out + SPFE_MP_OFF_N_GOOD(a.m))[i] = n_good;
        (a.out + SPFE_MP_OFF_CODE(a.m))[i] = (uint8_t)code;
        if (!desc_now) {
          reinterpret_cast<int *>(a.out + SPFE_MP_OFF_BEST_OBS)[i] = -1;
          reinterpret_cast<float *>(a.out + SPFE_MP_OFF_BEST_MEDIAN(a.m))[i] = 0.0f;
        }
      }
      if (desc_now) {
        if (n_good > MP_WAVE_OBS) {
          big = n_good;
        } else {
          wave_sync();   // (the list of this wavefront's last point has been read)
          mp_compact(a, s, n_all, lane, wave_p[wave], wave_o[wave], MP_WAVE_OBS);
          wave_sync();
          float best;
          int besti;
          mp_rows<false>(stage, wave_p[wave], n_good, bf16, lane, 0, 1, &best, &besti);
          mp_write_desc(a, i, row, wave_p[wave], wave_o[wave], best, besti, lane);
        }
      }
    }
    if (lane == 0) big_n[q] = big;
  }
  __syncthreads();

  // ---- second phase: the workgroup per larger point ----
  for (int q = 0; q < MP_CHUNK; ++q) {
    const int N = big_n[q];   // block-uniform
    if (!N) continue;
    const int i = i_base + q;
    const int row = a.point_idx ? a.point_idx[i] : i;
    const int s = a.obs_start[i], n_all = a.obs_start[i + 1] - s;
    if (wave == 0) mp_compact(a, s, n_all, lane, big_p, big_o, MP_MAX);
    __syncthreads();
    const int row_bytes = bf16 ? 512 : 1024;
    const bool staged = N * row_bytes <= MP_STAGE_BYTES;
    if (staged) {
      const int per_row = row_bytes / 16;
      for (int p = threadIdx.x; p < N * per_row; p += MP_WG)
        reinterpret_cast<uint4 *>(stage)[p] = *reinterpret_cast<const uint4 *>(big_p[p / per_row] + (size_t)(p % per_row) * 16);
      __syncthreads();
    }
    float best;
    int besti;
    if (staged)
      mp_rows<true>(stage, big_p, N, bf16, lane, wave, MP_WAVES, &best, &besti);
    else
      mp_rows<false>(stage, big_p, N, bf16, lane, wave, MP_WAVES, &best, &besti);
    if (lane == 0) {
      wbest[wave] = best;
      wbesti[wave] = besti;
    }
    __syncthreads();
    if (wave == 0) {   // the least median; the lowest row on a tie, as the ascending strict comparison leaves it
      best = spfe_mp_best_init();
      besti = -1;
#pragma unroll
      for (int w = 0; w < MP_WAVES; ++w) {
        const float mw = wbest[w];
        const int iw = wbesti[w];
        if (iw >= 0 && (besti < 0 || mw < best || (mw == best && iw < besti))) {
          best = mw;
          besti = iw;
        }
      }
      mp_write_desc(a, i, row, big_p, big_o, best, besti, lane);
    }
    __syncthreads();   // the lists and the stage are the next point's
  }
}

__global__ __launch_bounds__(MP_WG) void mp_header_kernel(MpArgs a) {
  __shared__ int part[3][MP_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint8_t *code = a.out + SPFE_MP_OFF_CODE(a.m);
  int nd = 0, nn = 0, st = 0;
  for (int i = threadIdx.x; i < a.m; i += MP_WG) {
    const int c = code[i];
    nd += (a.mode & SPFE_MP_DESC) && c == SPFE_MP_REFRESHED;
    nn += (a.mode & SPFE_MP_NORMAL_DEPTH) && c >= SPFE_MP_NO_GOOD_KF;
  }
  if (a.records)
    for (int k = threadIdx.x; k < a.n_kf; k += MP_WG) {
      const uint8_t *rec = a.records[k];
      if (rec) st |= reinterpret_cast<const int *>(rec + a.off_hdr)[2];
    }
  nd = wave_sum(nd);
  nn = wave_sum(nn);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) st |= __shfl_xor(st, off, 64);
  if (lane == 0) {
    part[0][wave] = nd;
    part[1][wave] = nn;
    part[2][wave] = st;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    nd = nn = st = 0;
    for (int w = 0; w < MP_WAVES; ++w) {
      nd += part[0][w];
      nn += part[1][w];
      st |= part[2][w];
    }
    int *h = reinterpret_cast<int *>(a.out);
    h[0] = a.m;
    h[1] = nd;
    h[2] = nn;
    h[3] = st;
  }
}

__global__ __launch_bounds__(MP_WG) void mp_gather_kernel(MpGatherArgs a) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * MP_WAVES + (threadIdx.x >> 6);
  if (i >= a.n) return;
  const int r = a.idx[i];
  const bool ok = r >= 0 && r < a.n_table;   // an index outside the table is not followed
  float4 d = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (ok) d = *reinterpret_cast<const float4 *>(a.desc + (size_t)r * 256 + lane * 4);
  *reinterpret_cast<float4 *>(a.o_desc + (size_t)i * 256 + lane * 4) = d;
  if (lane < 3) {
    a.o_xyz[3 * (size_t)i + lane] = ok ? a.xyz[3 * (size_t)r + lane] : 0.0f;
    a.o_normal[3 * (size_t)i + lane] = ok ? a.normal[3 * (size_t)r + lane] : 0.0f;
  }
  if (lane < 2) a.o_dist_range[2 * (size_t)i + lane] = ok ? a.dist_range[2 * (size_t)r + lane] : 0.0f;
  if (lane == 0) {
    a.o_id[i] = r;
    a.o_flags[i] = ok ? a.flags[r] : (uint8_t)0;
  }
}

hipError_t launch_mp_refresh(const MpArgs &a, hipStream_t s) {
  if (a.m < 0 || a.m > SPFE_MP_MAX_POINTS || a.E < 0 || a.E > SPFE_MP_MAX_EDGES || a.n_table < 0 || (a.records && a.n_kf < 1))
    return hipErrorInvalidValue;
  if (a.m > 0) hipLaunchKernelGGL(mp_refresh_kernel, dim3((a.m + MP_CHUNK - 1) / MP_CHUNK), dim3(MP_WG), 0, s, a);
  hipLaunchKernelGGL(mp_header_kernel, dim3(1), dim3(MP_WG), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_mp_gather(const MpGatherArgs &a, hipStream_t s) {
  if (a.n < 0 || a.n > SPFE_MP_MAX_POINTS || a.n_table < 0) return hipErrorInvalidValue;
  if (a.n > 0) hipLaunchKernelGGL(mp_gather_kernel, dim3((a.n + MP_WAVES - 1) / MP_WAVES), dim3(MP_WG), 0, s, a);
  return hipGetLastError();
}

}  // namespace spfe
