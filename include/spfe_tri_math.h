/*
 * spfe_tri_math.h — the arithmetic of the creation of new map points between two keyframes (match gate, triangulation, point
 * gates), shared by the GPU kernels (sp_orb_slam_amd/csrc/tri.hip) and the host C reference of the test suite
 * (tests/tri_ref/tri_ref.c) so that both evaluate the same sequence of IEEE operations (compile with -ffp-contract=off).
 *
 * What it restates, in this project's own words:
 *   LocalMapping::CreateNewMapPointsOverride   orb_slam2/src/mapping/local_mapper.cpp:558-814   (the loop body :592-800)
 *   LocalMapping::ComputeF12                   orb_slam2/src/mapping/local_mapper_raw.cpp:325-342
 *   SPMatcher::SearchForTriByFlann             orb_slam2/src/cv/sp_matcher.cpp:183-262           (matching_method 1)
 *   SPMatcher::CheckDistEpipolarLine           orb_slam2/src/cv/sp_matcher.cpp:441-469
 * Keyframe 1 is the current keyframe, keyframe 2 the neighbour.  Tcw = [Rcw | tcw] row-major 4x4, f32.  All arithmetic is f32
 * with every sum left to right, except where this text says double.
 *
 * Camera:  Ow = -(R^T t) as in spfe_proj_math.h;  invfx = 1.0f / fx,  invfy = 1.0f / fy.
 *
 * Baseline test (:603-611):  baseline = (float)sqrt(sum over k of (double)(Ow2_k - Ow1_k)^2)  (cv::norm accumulates in double);
 *   the neighbour is skipped when (double)(baseline / median_depth) < min_baseline_depth_ratio (0.01, a double literal).
 *
 * Fundamental matrix  F12 = K1^-T [t12]x R12 K2^-1:
 *   R12 = R1 R2^T,  t12_r = -((R12_r0 t2_0 + R12_r1 t2_1) + R12_r2 t2_2) + t1_r,
 *   E = [t12]x R12 with the zero terms left out:  E_0c = t12_1 R12_2c - t12_2 R12_1c,  E_1c = t12_2 R12_0c - t12_0 R12_2c,
 *   E_2c = t12_0 R12_1c - t12_1 R12_0c,
 *   M = K1^-T E:  M_0c = invfx1 E_0c,  M_1c = invfy1 E_1c,  M_2c = ((-(cx1 invfx1)) E_0c + (-(cy1 invfy1)) E_1c) + E_2c,
 *   F = M K2^-1:  F_r0 = M_r0 invfx2,  F_r1 = M_r1 invfy2,  F_r2 = (M_r0 (-(cx2 invfx2)) + M_r1 (-(cy2 invfy2))) + M_r2.
 *   (OpenCV's K.inv() and its 3x3 products are not restated bit for bit: there is no OpenCV to compare with.)
 *
 * Epipole of camera 1 in image 2 (sp_matcher.cpp:187-193):  C2 = R2 Ow1 + t2,  invz = 1.0f / C2.z,
 *   ex = (fx2 C2.x) invz + cx2,  ey = (fy2 C2.y) invz + cy2.  Sideways motion has C2.z == 0: invz is infinite, ex / ey are
 *   +-inf or NaN, the comparison below is false and the pair is NOT rejected — the reference's behaviour, kept.
 *
 * Matching rule (SearchForTriByFlann in exact form).  Keypoint k of a frame is FREE when its mp_of_kp[k] < 0.
 *   Queries: keyframe 2's free keypoints in ascending order.  Train set: keyframe 1's free keypoints.
 *   Each query takes its exact two nearest train rows: dist(a, b) = sqrtf(s_255), s_k = fmaf(a_k - b_k, a_k - b_k, s_k-1),
 *   the lower train index on ties (match.hip).  Rows that hold a point compute distances but never compete, and every row
 *   keeps its own index.
 *   The free set is the one a fresh KeyFrame::buildIndexes() gives; the reference rebuilds it after every pair
 *   (local_mapper.cpp:793-798).  A neighbour with an older index searches a superset and then drops what GetMapPoint rejects.
 *   Pair gate of query k2 with nearest row k1 at d0 and second nearest at d1, in this order:
 *     ratio       d0 < ratio * d1                                        (0.7f)
 *     epipole     rejected when dx dx + dy dy < epipole_r2, dx = ex - x2, dy = ey - y2   (100 * mvScaleFactors[0] = 100)
 *     line        a = (x1 F_00 + y1 F_10) + F_20, b and c likewise with columns 1 and 2; factor = 1.0f / min(cinv2.x, cinv2.y);
 *                 num = (a x2 + b y2) + c; den = a a + b b; den == 0 rejects; dsqr = (num num) / den;
 *                 accepted when (double)dsqr < chi2_line * (double)factor  (3.84, a double literal: a NaN rejects)
 *   An accepted query writes match12[k1] = k2: the last writer wins, so the largest accepted k2 stays; n_matches counts EVERY
 *   acceptance (the reference's nmatches).  vbMatched2 can never fire — the queries are distinct — so they are independent.
 *   The pairs handed on are (k1, match12[k1]) in ascending k1.
 *
 * Triangulation of a pair (local_mapper.cpp:658-768), verdict in the order the reference decides:
 *   xn = ((x - cx) invfx, (y - cy) invfy, 1);  ray_k = (R_0k xn_0 + R_1k xn_1) + R_2k xn_2  (Rwc xn);
 *   cos = (float)(dot(ray1, ray2) / (norm(ray1) norm(ray2))), dot and norm accumulated in double (Mat::dot, cv::norm);
 *   SPFE_TRI_PARALLAX   unless cos > 0 and (double)cos < cos_parallax_max (0.9998); the stereo terms are vacuous (cos < cos + 1)
 *   A_0 = xn1_0 T1_2 - T1_0,  A_1 = xn1_1 T1_2 - T1_1,  A_2 = xn2_0 T2_2 - T2_0,  A_3 = xn2_1 T2_2 - T2_1  (rows of [R | t]);
 *   x = the null vector of A (below);  SPFE_TRI_DEGENERATE when x_3 == 0;  X_k = x_k / x_3;
 *   z1 = (float)(dot(R1 row 2, X) + (double)t1_2), the dot in double;  SPFE_TRI_DEPTH when z1 <= 0, then likewise z2 <= 0;
 *   per image, image 1 first:  xc = (float)(dot(R row 0, X) + (double)t_0), yc likewise, invz = (float)(1.0 / (double)z),
 *   u = (fx xc) invz + cx, v = (fy yc) invz + cy, eu = u - x, ev = v - y,
 *   SPFE_TRI_REPROJ when (double)((eu eu) cinv.x + (ev ev) cinv.y) > chi2_reproj (5.991; a NaN passes, as in the reference);
 *   SPFE_TRI_DEGENERATE when (float)norm(X - Ow1) == 0 or (float)norm(X - Ow2) == 0;  else SPFE_TRI_NEW.
 *
 * The null vector of the 4x4 A.  The reference calls cv::SVD::compute and takes the last row of vt.  OpenCV is not available
 * to compare with and a record carries no OpenCV vectors, so this header DEFINES the computation: a one-sided (Hestenes)
 * Jacobi SVD in f32 on the columns of A, V = I at the start, SPFE_TRI_JACOBI_SWEEPS sweeps over the pairs (p, q) in the fixed
 * order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), no data-dependent exit:
 *   alpha = sum_i A_ip A_ip, beta = sum_i A_iq A_iq, gamma = sum_i A_ip A_iq (i ascending); gamma == 0 leaves the pair alone;
 *   zeta = (beta - alpha) / (2 gamma);  t = sign(zeta) / (|zeta| + sqrtf(1 + zeta zeta)), sign(0) = +1;
 *   c = 1 / sqrtf(1 + t t), s = c t;  columns p, q of A and of V become (c p - s q, s p + c q).
 * The result is the column of V whose column of A has the smallest squared norm (sum i ascending); on ties the LAST column.
 *
 * Undefined in the reference, defined here:
 *   fewer than two free train rows: no query matches (the reference would index matches[i][1]);
 *   NaN or infinite distances never match (they are never "nearest": match.hip).
 */
#ifndef SPFE_TRI_MATH_H
#define SPFE_TRI_MATH_H

#if defined(__HIPCC__)
#define SPFE_TM __host__ __device__ static inline
#else
#define SPFE_TM static inline
#endif

/* per-pair verdict codes (verdict[k1]); SPFE_TRI_NONE: k1 holds no match */
#define SPFE_TRI_NONE 0
#define SPFE_TRI_NEW 1
#define SPFE_TRI_PARALLAX 2
#define SPFE_TRI_DEGENERATE 3
#define SPFE_TRI_DEPTH 4
#define SPFE_TRI_REPROJ 5

/* Chosen on the CPU (tests/test_tri_reference.py::test_one_more_sweep_changes_nothing): with 6 sweeps one more sweep changes
 * no bit of any fixture's null vector, point or verdict. */
#define SPFE_TRI_JACOBI_SWEEPS 6

typedef struct {
  float R[9], t[3]; /* Rcw row-major, tcw */
  float Ow[3];      /* camera centre */
  float fx, fy, cx, cy, invfx, invfy;
} spfe_tri_cam;

typedef struct {
  float F[9];   /* F12 row-major */
  float ex, ey; /* epipole of camera 1 in image 2 */
} spfe_tri_pair;

SPFE_TM void spfe_tri_cam_from_f32(const float Tcw[16], float fx, float fy, float cx, float cy, spfe_tri_cam *c) {
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) c->R[3 * r + k] = Tcw[4 * r + k];
    c->t[r] = Tcw[4 * r + 3];
  }
  for (int k = 0; k < 3; ++k) c->Ow[k] = -((c->R[k] * c->t[0] + c->R[3 + k] * c->t[1]) + c->R[6 + k] * c->t[2]);
  c->fx = fx; c->fy = fy; c->cx = cx; c->cy = cy;
  c->invfx = 1.0f / fx;
  c->invfy = 1.0f / fy;
}

SPFE_TM double spfe_tri_dot3(const float a[3], const float b[3]) {
  double s = (double)a[0] * (double)b[0];
  s = s + (double)a[1] * (double)b[1];
  s = s + (double)a[2] * (double)b[2];
  return s;
}
SPFE_TM double spfe_tri_norm3(const float a[3]) { return __builtin_sqrt(spfe_tri_dot3(a, a)); }

/* 1 when the neighbour is skipped by the baseline test */
SPFE_TM int spfe_tri_baseline_skip(const spfe_tri_cam *c1, const spfe_tri_cam *c2, float median_depth, double min_ratio) {
  const float d[3] = {c2->Ow[0] - c1->Ow[0], c2->Ow[1] - c1->Ow[1], c2->Ow[2] - c1->Ow[2]};
  const float baseline = (float)spfe_tri_norm3(d);
  const float ratio = baseline / median_depth;
  return (double)ratio < min_ratio;
}

SPFE_TM void spfe_tri_pair_from_cams(const spfe_tri_cam *c1, const spfe_tri_cam *c2, spfe_tri_pair *p) {
  float R12[9], t12[3], E[9], M[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      R12[3 * r + c] = (c1->R[3 * r] * c2->R[3 * c] + c1->R[3 * r + 1] * c2->R[3 * c + 1]) + c1->R[3 * r + 2] * c2->R[3 * c + 2];
  for (int r = 0; r < 3; ++r)
    t12[r] = -((R12[3 * r] * c2->t[0] + R12[3 * r + 1] * c2->t[1]) + R12[3 * r + 2] * c2->t[2]) + c1->t[r];
  for (int c = 0; c < 3; ++c) {
    E[c] = t12[1] * R12[6 + c] - t12[2] * R12[3 + c];
    E[3 + c] = t12[2] * R12[c] - t12[0] * R12[6 + c];
    E[6 + c] = t12[0] * R12[3 + c] - t12[1] * R12[c];
  }
  const float kx1 = -(c1->cx * c1->invfx), ky1 = -(c1->cy * c1->invfy);
  const float kx2 = -(c2->cx * c2->invfx), ky2 = -(c2->cy * c2->invfy);
  for (int c = 0; c < 3; ++c) {
    M[c] = c1->invfx * E[c];
    M[3 + c] = c1->invfy * E[3 + c];
    M[6 + c] = (kx1 * E[c] + ky1 * E[3 + c]) + E[6 + c];
  }
  for (int r = 0; r < 3; ++r) {
    p->F[3 * r] = M[3 * r] * c2->invfx;
    p->F[3 * r + 1] = M[3 * r + 1] * c2->invfy;
    p->F[3 * r + 2] = (M[3 * r] * kx2 + M[3 * r + 1] * ky2) + M[3 * r + 2];
  }
  float C2[3];
  for (int r = 0; r < 3; ++r)
    C2[r] = ((c2->R[3 * r] * c1->Ow[0] + c2->R[3 * r + 1] * c1->Ow[1]) + c2->R[3 * r + 2] * c1->Ow[2]) + c2->t[r];
  const float invz = 1.0f / C2[2];
  p->ex = (c2->fx * C2[0]) * invz + c2->cx;
  p->ey = (c2->fy * C2[1]) * invz + c2->cy;
}

SPFE_TM int spfe_tri_ratio_ok(float d0, float d1, float ratio) { return d0 < ratio * d1; }

SPFE_TM int spfe_tri_epipole_reject(const spfe_tri_pair *p, float x2, float y2, float epipole_r2) {
  const float dx = p->ex - x2, dy = p->ey - y2;
  return dx * dx + dy * dy < epipole_r2;
}

SPFE_TM int spfe_tri_line_ok(const spfe_tri_pair *p, float x1, float y1, float x2, float y2, float cinv2x, float cinv2y,
                             double chi2_line) {
  const float *F = p->F;
  const float a = (x1 * F[0] + y1 * F[3]) + F[6];
  const float b = (x1 * F[1] + y1 * F[4]) + F[7];
  const float c = (x1 * F[2] + y1 * F[5]) + F[8];
  const float factor = 1.0f / (cinv2y < cinv2x ? cinv2y : cinv2x);
  const float num = (a * x2 + b * y2) + c;
  const float den = a * a + b * b;
  if (den == 0) return 0;
  const float dsqr = (num * num) / den;
  return (double)dsqr < chi2_line * (double)factor;
}

/* the whole pair gate behind the two nearest distances: 1 = accepted */
SPFE_TM int spfe_tri_gate(const spfe_tri_pair *p, float d0, float d1, float x1, float y1, float x2, float y2, float cinv2x,
                          float cinv2y, float ratio, float epipole_r2, double chi2_line) {
  if (!spfe_tri_ratio_ok(d0, d1, ratio)) return 0;
  if (spfe_tri_epipole_reject(p, x2, y2, epipole_r2)) return 0;
  return spfe_tri_line_ok(p, x1, y1, x2, y2, cinv2x, cinv2y, chi2_line);
}

/* the null vector of the row-major 4x4 A (destroyed), by `sweeps` Jacobi sweeps */
SPFE_TM void spfe_tri_null4(float A[16], int sweeps, float x[4]) {
  float V[16];
  for (int i = 0; i < 16; ++i) V[i] = (i % 5 == 0) ? 1.0f : 0.0f;
  for (int sw = 0; sw < sweeps; ++sw)
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) {
        float alpha = 0.0f, beta = 0.0f, gamma = 0.0f;
        for (int i = 0; i < 4; ++i) {
          alpha = alpha + A[4 * i + p] * A[4 * i + p];
          beta = beta + A[4 * i + q] * A[4 * i + q];
          gamma = gamma + A[4 * i + p] * A[4 * i + q];
        }
        if (gamma == 0.0f) continue;
        const float zeta = (beta - alpha) / (2.0f * gamma);
        const float h = __builtin_fabsf(zeta) + __builtin_sqrtf(1.0f + zeta * zeta);
        const float t = (zeta < 0.0f ? -1.0f : 1.0f) / h;
        const float c = 1.0f / __builtin_sqrtf(1.0f + t * t), s = c * t;
        for (int i = 0; i < 4; ++i) {
          const float ap = A[4 * i + p], aq = A[4 * i + q];
          A[4 * i + p] = c * ap - s * aq;
          A[4 * i + q] = s * ap + c * aq;
          const float vp = V[4 * i + p], vq = V[4 * i + q];
          V[4 * i + p] = c * vp - s * vq;
          V[4 * i + q] = s * vp + c * vq;
        }
      }
  int best = 0;
  float bn = 0.0f;
  for (int j = 0; j < 4; ++j) {
    float n = 0.0f;
    for (int i = 0; i < 4; ++i) n = n + A[4 * i + j] * A[4 * i + j];
    if (j == 0 || n <= bn) { bn = n; best = j; }
  }
  for (int i = 0; i < 4; ++i) x[i] = V[4 * i + best];
}

SPFE_TM void spfe_tri_xn(const spfe_tri_cam *c, float x, float y, float xn[3]) {
  xn[0] = (x - c->cx) * c->invfx;
  xn[1] = (y - c->cy) * c->invfy;
  xn[2] = 1.0f;
}

/* rows 2 i and 2 i + 1 of A from camera c and its normalised keypoint */
SPFE_TM void spfe_tri_rows(const spfe_tri_cam *c, const float xn[3], float *rows) {
  for (int k = 0; k < 4; ++k) {
    const float T0 = k < 3 ? c->R[k] : c->t[0], T1 = k < 3 ? c->R[3 + k] : c->t[1], T2 = k < 3 ? c->R[6 + k] : c->t[2];
    rows[k] = xn[0] * T2 - T0;
    rows[4 + k] = xn[1] * T2 - T1;
  }
}

/* 1 when the reprojection into camera c (depth z) is rejected */
SPFE_TM int spfe_tri_reproj_reject(const spfe_tri_cam *c, const float X[3], float z, float x, float y, float cinvx, float cinvy,
                                   double chi2_reproj) {
  const float xc = (float)(spfe_tri_dot3(&c->R[0], X) + (double)c->t[0]);
  const float yc = (float)(spfe_tri_dot3(&c->R[3], X) + (double)c->t[1]);
  const float invz = (float)(1.0 / (double)z);
  const float u = (c->fx * xc) * invz + c->cx, v = (c->fy * yc) * invz + c->cy;
  const float eu = u - x, ev = v - y;
  const float e = (eu * eu) * cinvx + (ev * ev) * cinvy;
  return (double)e > chi2_reproj;
}

/* the verdict of the pair (keypoint (x1, y1) of camera 1, (x2, y2) of camera 2); X is written for every verdict that reaches
 * the division (NEW, DEPTH, REPROJ, the second DEGENERATE), and is the new point when the verdict is SPFE_TRI_NEW */
SPFE_TM int spfe_tri_triangulate(const spfe_tri_cam *c1, const spfe_tri_cam *c2, float x1, float y1, float cinv1x, float cinv1y,
                                 float x2, float y2, float cinv2x, float cinv2y, double cos_parallax_max, double chi2_reproj,
                                 int sweeps, float X[3]) {
  float xn1[3], xn2[3], ray1[3], ray2[3];
  spfe_tri_xn(c1, x1, y1, xn1);
  spfe_tri_xn(c2, x2, y2, xn2);
  for (int k = 0; k < 3; ++k) {
    ray1[k] = (c1->R[k] * xn1[0] + c1->R[3 + k] * xn1[1]) + c1->R[6 + k] * xn1[2];
    ray2[k] = (c2->R[k] * xn2[0] + c2->R[3 + k] * xn2[1]) + c2->R[6 + k] * xn2[2];
  }
  const float cosr = (float)(spfe_tri_dot3(ray1, ray2) / (spfe_tri_norm3(ray1) * spfe_tri_norm3(ray2)));
  if (!(cosr > 0 && (double)cosr < cos_parallax_max)) return SPFE_TRI_PARALLAX;
  float A[16], x[4];
  spfe_tri_rows(c1, xn1, A);
  spfe_tri_rows(c2, xn2, A + 8);
  spfe_tri_null4(A, sweeps, x);
  if (x[3] == 0) return SPFE_TRI_DEGENERATE;
  for (int k = 0; k < 3; ++k) X[k] = x[k] / x[3];
  const float z1 = (float)(spfe_tri_dot3(&c1->R[6], X) + (double)c1->t[2]);
  if (z1 <= 0) return SPFE_TRI_DEPTH;
  const float z2 = (float)(spfe_tri_dot3(&c2->R[6], X) + (double)c2->t[2]);
  if (z2 <= 0) return SPFE_TRI_DEPTH;
  if (spfe_tri_reproj_reject(c1, X, z1, x1, y1, cinv1x, cinv1y, chi2_reproj)) return SPFE_TRI_REPROJ;
  if (spfe_tri_reproj_reject(c2, X, z2, x2, y2, cinv2x, cinv2y, chi2_reproj)) return SPFE_TRI_REPROJ;
  const float n1[3] = {X[0] - c1->Ow[0], X[1] - c1->Ow[1], X[2] - c1->Ow[2]};
  const float n2[3] = {X[0] - c2->Ow[0], X[1] - c2->Ow[1], X[2] - c2->Ow[2]};
  if ((float)spfe_tri_norm3(n1) == 0 || (float)spfe_tri_norm3(n2) == 0) return SPFE_TRI_DEGENERATE;
  return SPFE_TRI_NEW;
}

#endif /* SPFE_TRI_MATH_H */
