// fuse_target.h — what fuse.hip and loopfuse.hip share: target j's view of a FuseArgs and the load of four descriptor elements.
#pragma once
#include "../../include/spfe.h"
#include "spfe_kernels.h"

namespace spfe {

// target j's view of the arguments
struct FuseTarget {
  const float *kp_xy;
  const int16_t *occ;
  const float *kp_desc;
  const int *mp;
  const float *Tcw;
  uint8_t *out;
  int K, status;
};
static __device__ __forceinline__ FuseTarget fuse_target(const FuseArgs &a, int j) {
  const uint8_t *b = a.base[j];
  FuseTarget t;
  t.kp_xy = reinterpret_cast<const float *>(b + a.off_xy);
  t.occ = reinterpret_cast<const int16_t *>(b + a.off_occ);
  t.kp_desc = reinterpret_cast<const float *>(b + a.off_desc);
  t.mp = a.kf_mp_of_kp + (size_t)j * a.kmax;
  t.Tcw = a.Tcw + 16 * (size_t)j;
  t.out = a.out + (size_t)j * SPFE_FUSE_OUT_BYTES(a.cap);
  t.K = a.k_imm;
  t.status = 0;
  if (a.off_hdr >= 0) {
    const int *hdr = reinterpret_cast<const int *>(b + a.off_hdr);
    t.K = min(max(hdr[0], 0), a.kmax);
    t.status = hdr[2];
  }
  return t;
}
// four consecutive descriptor elements from element index e: f32 rows, or bf16 rows widened (exact)
static __device__ __forceinline__ float4 fuse_desc4(const float *rows, size_t e, int bf16) {
  if (!bf16) return *reinterpret_cast<const float4 *>(rows + e);
  const uint2 p = *reinterpret_cast<const uint2 *>(reinterpret_cast<const unsigned short *>(rows) + e);
  return make_float4(__uint_as_float(p.x << 16), __uint_as_float(p.x & 0xffff0000u), __uint_as_float(p.y << 16),
                     __uint_as_float(p.y & 0xffff0000u));
}

}  // namespace spfe
