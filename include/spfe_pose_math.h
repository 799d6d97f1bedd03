/*
 * spfe_pose_math.h — the arithmetic of the covariance-weighted pose refinement, shared by the GPU kernel
 * (sp_orb_slam_amd/csrc/pose.hip) and the host C reference of the test suite (tests/pose_ref/pose_ref.c) so that both
 * evaluate the same sequence of IEEE operations (compile with -ffp-contract=off).
 *
 * What it restates:
 *   Optimizer::PoseOptimizationDustPost   orb_slam2/src/mapping/optimizer_dust.cpp:35-167
 *   Optimizer::PoseOptimization           orb_slam2/src/mapping/optimizer.cpp:231-443 (monocular edges only)
 *   and, of g2o (a catkin dependency of the reference, NOT part of the reference snapshot — parity unpinned, published
 *   algorithm restated): EdgeSE3ProjectXYZOnlyPose::computeError / linearizeOplus, BaseEdge::chi2,
 *   BaseUnaryEdge::constructQuadraticForm with and without a robust kernel.  The pose, the exponential map, Huber, the 6x6
 *   solve, the Levenberg bookkeeping and the fixed-shape 256-slot tree are those of spfe_dust_math.h, unchanged.
 *
 * One edge per keypoint i with a map point, in ascending keypoint index (the reference's loop over mvpMapPoints[i]):
 *   obs = kp_xy[i] (floats, widened), Omega = diag(cov2_inv[i].x, cov2_inv[i].y) (optimizer_dust.cpp:86-91),
 *   Xw = the map point's world position (floats, widened).
 *   error   e   = obs - (fx * (x / z) + cx, fy * (y / z) + cy),  (x, y, z) = T.map(Xw)     (g2o project(): x / z first)
 *   chi2        = e0 * (w0 * e0) + e1 * (w1 * e1)                                         (e . (Omega e))
 *   Jacobian A  = d e / d update, 2x6, update = (omega, upsilon)
 *   sums (28 quantities, the tree of spfe_dust_math.h):
 *     q[0]                     rho0 (robust chi2; chi2 without a kernel)
 *     q[1 + i (i + 1) / 2 + j] (A0i * (rho1 w0)) * A0j + (A1i * (rho1 w1)) * A1j            (A^T (rho1 Omega) A)
 *     q[22 + j]                -(rho1 * (A0j * (w0 e0) + A1j * (w1 e1)))                      (b -= rho1 A^T Omega e)
 *   rho = Huber(chi2, delta) with a kernel, (chi2, 1) without.
 */
#ifndef SPFE_POSE_MATH_H
#define SPFE_POSE_MATH_H

#include "spfe_dust_math.h"

#define SPFE_POSE_NSUM 28
/* const float deltaMono = sqrt(5.991): the double square root rounded to float (optimizer_dust.cpp:66, optimizer.cpp:276) */
#define SPFE_POSE_DELTA 2.4476518630981445   /* = (double)(float)sqrt(5.991), exactly */
#define SPFE_POSE_CHI2_MONO 5.991f   /* chi2Mono[it] (float), optimizer.cpp */
#define SPFE_POSE_CHI2_POST 7.378    /* the double literal of optimizer_dust.cpp:140 */

/* T.map(Xw) and the error; returns z through p (the Jacobian's input) */
SPFE_DM void spfe_pose_error(const spfe_se3 *T, const double Xw[3], double fx, double fy, double cx, double cy,
                             double ox, double oy, double p[3], double e[2]) {
  spfe_se3_map(T, Xw, p);
  const double px = p[0] / p[2], py = p[1] / p[2];
  e[0] = ox - (px * fx + cx);
  e[1] = oy - (py * fy + cy);
}

/* e . (Omega e), Omega = diag(w0, w1) */
SPFE_DM double spfe_pose_chi2(const double e[2], double w0, double w1) { return e[0] * (w0 * e[0]) + e[1] * (w1 * e[1]); }

/* linearizeOplus at the mapped point p: rows A0 (u), A1 (v) */
SPFE_DM void spfe_pose_jacobian(const double p[3], double fx, double fy, double A0[6], double A1[6]) {
  const double x = p[0], y = p[1];
  const double invz = 1.0 / p[2];
  const double invz_2 = invz * invz;
  A0[0] = x * y * invz_2 * fx;
  A0[1] = -(1 + (x * x * invz_2)) * fx;
  A0[2] = y * invz * fx;
  A0[3] = -invz * fx;
  A0[4] = 0;
  A0[5] = x * invz_2 * fx;
  A1[0] = (1 + y * y * invz_2) * fy;
  A1[1] = -x * y * invz_2 * fy;
  A1[2] = -x * invz * fy;
  A1[3] = 0;
  A1[4] = -invz * fy;
  A1[5] = y * invz_2 * fy;
}

/* the robust chi2 contribution (activeRobustChi2) of an edge with chi2 `c` */
SPFE_DM double spfe_pose_rho0(double c, int robust) {
  if (!robust) return c;
  double rho[3];
  spfe_huber(c, SPFE_POSE_DELTA, rho);
  return rho[0];
}

/* the 28 quantities of one edge (constructQuadraticForm + activeRobustChi2) */
SPFE_DM void spfe_pose_terms(const double e[2], const double A0[6], const double A1[6], double w0, double w1, int robust,
                             double q[SPFE_POSE_NSUM]) {
  const double c = spfe_pose_chi2(e, w0, w1);
  double rho[3] = {c, 1.0, 0.0};
  if (robust) spfe_huber(c, SPFE_POSE_DELTA, rho);
  const double r0 = rho[1] * w0, r1 = rho[1] * w1;
  const double we0 = w0 * e[0], we1 = w1 * e[1];
  q[0] = rho[0];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j <= i; ++j) q[1 + i * (i + 1) / 2 + j] = (A0[i] * r0) * A0[j] + (A1[i] * r1) * A1[j];
  for (int j = 0; j < 6; ++j) q[22 + j] = -(rho[1] * (A0[j] * we0 + A1[j] * we1));
}

/* the classification chi2: `const float chi2 = e->chi2()` */
SPFE_DM float spfe_pose_chi2f(const double e[2], double w0, double w1) { return (float)spfe_pose_chi2(e, w0, w1); }

#endif /* SPFE_POSE_MATH_H */
