/*
 * spfe_sim3_math.h — the arithmetic of the front half of loop verification (pair list, random triples, Horn's closed form,
 * the two-way reprojection test, the rule of the returns), shared by the GPU kernels (sp_orb_slam_amd/csrc/sim3.hip) and the
 * host C reference of the test suite (tests/sim3_ref/sim3_ref.c) so that both evaluate the same sequence of IEEE operations
 * (compile with -ffp-contract=off).
 *
 * What it restates, in this project's own words:
 *   LoopClosingVLAD::ComputeSim3         orb_slam2/src/loopclosing/loop_closer_vlad.cpp:345-449
 *   SPMatcher::SearchByBruteForce        orb_slam2/src/cv/sp_matcher_loop.cpp:334-376   (KeyFrame, KeyFrame form)
 *   Sim3Solver                           orb_slam2/src/mapping/sim3_solver.cpp
 * Keyframe 1 is the current keyframe, keyframe 2 the loop candidate.  Tcw = [Rcw | tcw] row-major 4x4, f32.  All arithmetic
 * is f32 with every sum left to right, except where this text says double.
 *
 * Pairs (Sim3Solver::Sim3Solver :64-103).  k1 runs upward over keyframe 1's keypoints; a pair exists iff
 *   match12[k1] = k2 >= 0 (and below the capacity of keyframe 2's arrays), p1 = kf1_mp_of_kp[k1] in [0, n),
 *   p2 = kf2_mp_of_kp[k2] in [0, n), and flags[p1], flags[p2] both carry SPFE_PROJ_SEARCHABLE (!isBad()).
 *   GetIndexInKeyFrame() < 0 (:75-79) cannot occur: p1 and p2 are taken FROM the keyframes' own holder arrays, so the points
 *   are held by k1 and k2.  Pair i (the i-th in ascending k1) keeps k1 (mvnIndices1) and
 *     X1c = Rcw1 X1w + tcw1,  X2c = Rcw2 X2w + tcw2:   Xc_r = ((R_r0 X_0 + R_r1 X_1) + R_r2 X_2) + t_r,
 *     P1im1 = image(K1, X1c), P2im2 = image(K2, X2c):  invz = 1.0f / z, x = X invz, y = Y invz, (fx x + cx, fy y + cy);
 *   no depth test (FromCameraToImage / Project have none): a point behind a camera projects through the centre.
 *   N pairs.  N < max(3, min_inliers): nothing is evaluated, every count is 0 (:149-152 sets bNoMore at once).
 *
 * 1. The random draws are an input.  Sim3Solver::iterate seeds a static mt19937 from random_device, so the reference has no
 *   reproducible output; here hypothesis h reads rand_u32[h][0..2].  Draw j (j = 0, 1, 2) is
 *     r = ((uint64)word * (uint64)(N - j)) >> 32
 *   into a list that starts as 0 .. N-1; the pair taken is list[r], then list[r] = list[N-1-j] and the list shrinks by one —
 *   the reference's swap-with-back.  DEPARTURE: the reference keeps uniform_int_distribution(0, N-1) for all three draws, so
 *   its second and third draw can index a slot it has just popped (the vector's storage behind size()); here a draw is taken
 *   from the live range, so the three pairs are always distinct.
 *
 * 2. The iteration limit stays on the host.  SetRansacParameters computes max(1, min(ceil(log(1 - p) / log(1 - eps^3)),
 *   max_its)) in double libm with eps = (float)min_inliers / N, and N is known only on the device.  The device evaluates
 *   EVERY supplied hypothesis; spfe_sim3_iteration_limit() (include/spfe.h, plain host C) gives the limit and the host ignores
 *   the hypotheses at and beyond it.  Counts, transforms, inlier bits and the list of returns are ordered by hypothesis, so
 *   cutting them at the limit is exact.
 *
 * 3. Thresholds.  mvnMaxError1/2 are std::vector<size_t> (sim3_solver.h:74-75): 9.210 * sigma2 is truncated to the integer 9
 *   when pushed, and `err < 9` is then evaluated in float.  The extractor has one pyramid level, sigma2 = 1, so the
 *   parameters carry max_err1 = max_err2 = 9.0f, not 9.21f.
 *
 * 4. Arithmetic with no OpenCV to match.  For the triple (columns i = 0, 1, 2 of P1, P2 = X1c, X2c of the drawn pairs):
 *   centroid  O_r = ((P_r0 + P_r1) + P_r2) / 3.0f,  Pr_ri = P_ri - O_r;
 *   M = Pr2 Pr1^T:  M_ab = (Pr2_a0 Pr1_b0 + Pr2_a1 Pr1_b1) + Pr2_a2 Pr1_b2;
 *   the N matrix (:235-251): the reference's expressions are sums of floats ASSIGNED to doubles and stored back to f32, so the
 *   entries are f32 sums left to right as written: N11 = (M00 + M11) + M22, N12 = M12 - M21, N13 = M20 - M02, N14 = M01 - M10,
 *   N22 = (M00 - M11) - M22, N23 = M01 + M10, N24 = M20 + M02, N33 = ((-M00) + M11) - M22, N34 = M12 + M21,
 *   N44 = ((-M00) - M11) + M22, symmetric.
 *   The eigenvector of N's largest eigenvalue is DEFINED here (cv::eigen sorts descending and row 0 is taken): a cyclic Jacobi
 *   eigen-iteration in f32, V = I at the start, SPFE_SIM3_JACOBI_SWEEPS sweeps over the pairs (p, q) in the fixed order
 *   (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), no data-dependent exit:  a_pq == 0 leaves the pair alone;
 *     theta = (a_qq - a_pp) / (2 a_pq);  t = sign(theta) / (|theta| + sqrtf(1 + theta theta)), sign(0) = +1;
 *     c = 1 / sqrtf(1 + t t), s = c t;  columns p, q of A and of V become (c p - s q, s p + c q), then rows p, q of A likewise.
 *   The result is the column of V whose diagonal entry of A is largest, the FIRST on ties: q = (w, x, y, z).
 *   The rotation is formed directly from the normalised quaternion: n = sqrtf(((w w + x x) + y y) + z z), each / n, then
 *     R00 = 1 - 2 (yy + zz), R01 = 2 (xy - wz), R02 = 2 (xz + wy), R10 = 2 (xy + wz), R11 = 1 - 2 (xx + zz),
 *     R12 = 2 (yz - wx), R20 = 2 (xz - wy), R21 = 2 (yz + wx), R22 = 1 - 2 (xx + yy).
 *   (The reference's detour through atan2, the angle-axis vector and cv::Rodrigues is the same rotation and would put libm on
 *   the device; the fixtures pin R against float64.)
 *   P3 = R Pr2:  P3_ri = (R_r0 Pr2_0i + R_r1 Pr2_1i) + R_r2 Pr2_2i;
 *   scale (:276-288): nom = sum of (double)Pr1_ri (double)P3_ri, den = sum of (double)(float)(P3_ri P3_ri), both over r outer,
 *     i inner; s = (float)(nom / den); fix_scale: s = 1.0f;
 *   sR_rc = s R_rc;  t12_r = O1_r - ((sR_r0 O2_0 + sR_r1 O2_1) + sR_r2 O2_2);  T12 = [sR | t12];
 *   T21: is = (float)(1.0 / (double)s), iR_rc = is R_cr, t21_r = -((iR_r0 t12_0 + iR_r1 t12_1) + iR_r2 t12_2).
 *   Inlier test of pair i (CheckInliers :318-338): P2im1 = image(K1, T12 X2c), P1im2 = image(K2, T21 X1c) with the transform
 *   applied like a pose above; d1 = P1im1 - P2im1, d2 = P1im2 - P2im2; err = (float)((double)dx dx + (double)dy dy)
 *   (Mat::dot accumulates in double); inlier iff err1 < max_err1 && err2 < max_err2.
 *   A degenerate triple (collinear or coincident points) is evaluated as written: NaN errors compare false, 0 inliers.
 *   IEEE 754 leaves the sign and payload of a NaN result open (a negation folded into an operand flips it on one machine and
 *   not on another), so every NaN among s, R, t is replaced by the quiet NaN 0x7fc00000 before T12 is used or stored.
 *
 * 5. The sequential iterate().  iterate keeps mnBestInliers (0 at the start) and mnIterations across calls.  Hypothesis h
 *   RETURNS a transform iff count_h >= max(0, count_0 .. count_h-1) and count_h > min_inliers; the running best is the last h
 *   that attains the prefix maximum.  Neither depends on how the calls are cut into fives, so the device reports all counts,
 *   the ordered list return_idx[0 .. n_returns) and, over all supplied hypotheses, best_h / best_count; the host replays the
 *   interleaving of the candidates (tests/sim3_ref/sim3_walk.py).
 */
#ifndef SPFE_SIM3_MATH_H
#define SPFE_SIM3_MATH_H

#include <stdint.h>

#if defined(__HIPCC__)
#define SPFE_S3 __host__ __device__ static inline
#else
#define SPFE_S3 static inline
#endif

/* Chosen on the CPU (tests/test_sim3_reference.py::test_one_more_sweep_changes_nothing): the smallest count at which one more
 * sweep changes no bit of any fixture's transform, count or inlier set. */
#define SPFE_SIM3_JACOBI_SWEEPS 5

typedef struct {
  float s, R[9], t[3]; /* T12 = [s R | t], R row-major */
} spfe_sim3_T;

/* Xc = R X + t for a row-major 4x4 pose */
SPFE_S3 void spfe_sim3_to_cam(const float T[16], const float X[3], float Xc[3]) {
  for (int r = 0; r < 3; ++r) Xc[r] = ((T[4 * r] * X[0] + T[4 * r + 1] * X[1]) + T[4 * r + 2] * X[2]) + T[4 * r + 3];
}

SPFE_S3 void spfe_sim3_image(float fx, float fy, float cx, float cy, const float Xc[3], float uv[2]) {
  const float invz = 1.0f / Xc[2];
  const float x = Xc[0] * invz, y = Xc[1] * invz;
  uv[0] = fx * x + cx;
  uv[1] = fy * y + cy;
}

SPFE_S3 int spfe_sim3_draw(uint32_t word, int live) { return (int)(((uint64_t)word * (uint64_t)live) >> 32); }

/* the three distinct pairs of a hypothesis (N >= 3); remove = 0 is the test suite's mutation "draws without removal" */
SPFE_S3 void spfe_sim3_draws(const uint32_t w[3], int N, int remove, int idx[3]) {
  int slot[3], val[3];
  for (int j = 0; j < 3; ++j) {
    const int live = remove ? N - j : N;
    const int r = spfe_sim3_draw(w[j], live);
    int v = r, bv = live - 1;
    if (remove) {
      for (int o = 0; o < j; ++o) {   /* the latest write of a slot wins */
        if (slot[o] == r) v = val[o];
        if (slot[o] == live - 1) bv = val[o];
      }
      slot[j] = r;
      val[j] = bv;
    }
    idx[j] = v;
  }
}

/* the eigenvector (w, x, y, z) of the largest eigenvalue of the symmetric row-major 4x4 A (destroyed) */
SPFE_S3 void spfe_sim3_eig4(float A[16], int sweeps, float q[4]) {
  float V[16];
  for (int i = 0; i < 16; ++i) V[i] = (i % 5 == 0) ? 1.0f : 0.0f;
  for (int sw = 0; sw < sweeps; ++sw)
    for (int p = 0; p < 3; ++p)
      for (int qq = p + 1; qq < 4; ++qq) {
        const float apq = A[4 * p + qq];
        if (apq == 0.0f) continue;
        const float theta = (A[5 * qq] - A[5 * p]) / (2.0f * apq);
        const float h = __builtin_fabsf(theta) + __builtin_sqrtf(1.0f + theta * theta);
        const float t = (theta < 0.0f ? -1.0f : 1.0f) / h;
        const float c = 1.0f / __builtin_sqrtf(1.0f + t * t), s = c * t;
        for (int k = 0; k < 4; ++k) {
          const float ap = A[4 * k + p], aq = A[4 * k + qq];
          A[4 * k + p] = c * ap - s * aq;
          A[4 * k + qq] = s * ap + c * aq;
          const float vp = V[4 * k + p], vq = V[4 * k + qq];
          V[4 * k + p] = c * vp - s * vq;
          V[4 * k + qq] = s * vp + c * vq;
        }
        for (int k = 0; k < 4; ++k) {
          const float ap = A[4 * p + k], aq = A[4 * qq + k];
          A[4 * p + k] = c * ap - s * aq;
          A[4 * qq + k] = s * ap + c * aq;
        }
      }
  int best = 0;
  for (int j = 1; j < 4; ++j)
    if (A[5 * j] > A[5 * best]) best = j;
  for (int i = 0; i < 4; ++i) q[i] = V[4 * i + best];
}

SPFE_S3 void spfe_sim3_rot_from_quat(const float q[4], float R[9]) {
  const float n = __builtin_sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  const float w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
  R[0] = 1.0f - 2.0f * (y * y + z * z);
  R[1] = 2.0f * (x * y - w * z);
  R[2] = 2.0f * (x * z + w * y);
  R[3] = 2.0f * (x * y + w * z);
  R[4] = 1.0f - 2.0f * (x * x + z * z);
  R[5] = 2.0f * (y * z - w * x);
  R[6] = 2.0f * (x * z - w * y);
  R[7] = 2.0f * (y * z + w * x);
  R[8] = 1.0f - 2.0f * (x * x + y * y);
}

SPFE_S3 float spfe_sim3_canon(float x) {
  if (x == x) return x;
  const uint32_t u = 0x7fc00000u;
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}

/* Horn's closed form on the triple: P1, P2 row-major [r][i] (column i = pair i), both destroyed (they become Pr1, Pr2) */
SPFE_S3 void spfe_sim3_horn(float P1[9], float P2[9], int fix_scale, int sweeps, spfe_sim3_T *T) {
  float O1[3], O2[3];
  for (int r = 0; r < 3; ++r) {
    O1[r] = ((P1[3 * r] + P1[3 * r + 1]) + P1[3 * r + 2]) / 3.0f;
    O2[r] = ((P2[3 * r] + P2[3 * r + 1]) + P2[3 * r + 2]) / 3.0f;
    for (int i = 0; i < 3; ++i) {
      P1[3 * r + i] = P1[3 * r + i] - O1[r];
      P2[3 * r + i] = P2[3 * r + i] - O2[r];
    }
  }
  float M[9];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) M[3 * a + b] = (P2[3 * a] * P1[3 * b] + P2[3 * a + 1] * P1[3 * b + 1]) + P2[3 * a + 2] * P1[3 * b + 2];
  float A[16];
  A[0] = (M[0] + M[4]) + M[8];
  A[1] = A[4] = M[5] - M[7];
  A[2] = A[8] = M[6] - M[2];
  A[3] = A[12] = M[1] - M[3];
  A[5] = (M[0] - M[4]) - M[8];
  A[6] = A[9] = M[1] + M[3];
  A[7] = A[13] = M[6] + M[2];
  A[10] = ((-M[0]) + M[4]) - M[8];
  A[11] = A[14] = M[5] + M[7];
  A[15] = ((-M[0]) - M[4]) + M[8];
  float q[4];
  spfe_sim3_eig4(A, sweeps, q);
  spfe_sim3_rot_from_quat(q, T->R);
  float s = 1.0f;
  if (!fix_scale) {
    double nom = 0.0, den = 0.0;
    for (int r = 0; r < 3; ++r)
      for (int i = 0; i < 3; ++i) {
        const float p3 = (T->R[3 * r] * P2[i] + T->R[3 * r + 1] * P2[3 + i]) + T->R[3 * r + 2] * P2[6 + i];
        const float sq = p3 * p3;
        nom = nom + (double)P1[3 * r + i] * (double)p3;
        den = den + (double)sq;
      }
    s = (float)(nom / den);
  }
  T->s = s;
  for (int r = 0; r < 3; ++r) {
    const float a = s * T->R[3 * r], b = s * T->R[3 * r + 1], c = s * T->R[3 * r + 2];
    T->t[r] = O1[r] - ((a * O2[0] + b * O2[1]) + c * O2[2]);
  }
  T->s = spfe_sim3_canon(T->s);
  for (int i = 0; i < 9; ++i) T->R[i] = spfe_sim3_canon(T->R[i]);
  for (int i = 0; i < 3; ++i) T->t[i] = spfe_sim3_canon(T->t[i]);
}

/* T12 and T21 as row-major 3x4 [A | b] for the inlier test */
SPFE_S3 void spfe_sim3_forms(const spfe_sim3_T *T, float T12[12], float T21[12]) {
  const float is = (float)(1.0 / (double)T->s);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) {
      T12[4 * r + c] = T->s * T->R[3 * r + c];
      T21[4 * r + c] = is * T->R[3 * c + r];
    }
    T12[4 * r + 3] = T->t[r];
  }
  for (int r = 0; r < 3; ++r) T21[4 * r + 3] = -((T21[4 * r] * T->t[0] + T21[4 * r + 1] * T->t[1]) + T21[4 * r + 2] * T->t[2]);
}

SPFE_S3 float spfe_sim3_err(const float A[12], const float X[3], float fx, float fy, float cx, float cy, const float obs[2]) {
  float P[3], uv[2];
  for (int r = 0; r < 3; ++r) P[r] = ((A[4 * r] * X[0] + A[4 * r + 1] * X[1]) + A[4 * r + 2] * X[2]) + A[4 * r + 3];
  spfe_sim3_image(fx, fy, cx, cy, P, uv);
  const float dx = obs[0] - uv[0], dy = obs[1] - uv[1];
  return (float)((double)dx * (double)dx + (double)dy * (double)dy);
}

/* hypothesis h returns iff its count equals the inclusive prefix maximum (mnBestInliers starts at 0) and exceeds min_inliers */
SPFE_S3 int spfe_sim3_returns(int count, int prefix_max_inclusive, int min_inliers) {
  return count == prefix_max_inclusive && count > min_inliers;
}

#endif /* SPFE_SIM3_MATH_H */
