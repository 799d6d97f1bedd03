/*
 * spfe_sim3opt_math.h — the arithmetic of the Sim3 optimisation of a loop hypothesis, shared by the GPU kernel
 * (sp_orb_slam_amd/csrc/sim3opt.hip) and the host C reference of the test suite (tests/sim3opt_ref/sim3opt_ref.c) so that
 * both evaluate the same sequence of IEEE operations (compile with -ffp-contract=off).
 *
 * What it restates:
 *   Optimizer::OptimizeSim3              orb_slam2/src/mapping/optimizer.cpp:1062-1252
 *   and, of g2o (a catkin dependency of the reference, NOT part of the reference snapshot — parity unpinned, published
 *   algorithm restated): Sim3 (the constructor from an update, operator*, inverse, map), VertexSim3Expmap::oplusImpl / cam_map1 /
 *   cam_map2, EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ::computeError, BaseBinaryEdge::linearizeOplus (NUMERIC: the two
 *   edge types do not override it), RobustKernelHuber, constructQuadraticForm, OptimizationAlgorithmLevenberg::solve.  Huber,
 *   the Levenberg constants, the quaternion helpers and the fixed-shape 256-slot tree are those of spfe_dust_math.h, unchanged;
 *   the trial's bookkeeping (spfe_s3o_lm_judge) and the solve (spfe_solve7) are spfe_lm_judge and spfe_solve6 at dimension 7.
 *
 * Correspondences.  matches12[k1] = k2 is what the guided match gives.  k1 runs upward over keyframe 1's K1 keypoints;
 *   matches12[k1] < 0: nothing (verdict NONE).  Otherwise p1 = kf1_mp_of_kp[k1], p2 = kf2_mp_of_kp[k2]; the correspondence is
 *   SERVED when 0 <= k2 < K2, p1 and p2 lie in [0, n) and flags[p1], flags[p2] both carry SPFE_PROJ_SEARCHABLE; else it is
 *   SKIPPED: not counted in nCorrespondences, its matches12 entry left as it is (optimizer.cpp:1128-1149).  Served
 *   correspondence c (the c-th in ascending k1) has
 *     P1c = Rcw1 X_p1 + tcw1, P2c = Rcw2 X_p2 + tcw2      f32, spfe_sim3_to_cam, then widened to double
 *     obs1 = kp_xy1[k1], obs2 = kp_xy2[k2]               widened
 *   information = identity (one pyramid level), th2 = 10.0f, Huber delta = (double)(float)sqrt(10.0).
 *
 * Sim3: a quaternion (x, y, z, w), t and s in double.  map(X) = s (r X) + t;  A B: r = rA rB, t = sA (rA tB) + tA, s = sA sB;
 *   inverse: r' = conj(r), t' = -(1 / s) (r' t), s' = 1 / s.  No product renormalises the quaternion (g2o's does not).
 *   Start value: Sim3(R, t, s) of the f32 T12[13] = (s, R row-major, t), R through spfe_quat_from_rot.
 * Sim3(update), update = (omega[3], upsilon[3], sigma): theta = |omega|, Omega = skew(omega), eps = 1e-5,
 *   s = exp(sigma) — DEFINED as ((1 + sigma) + sigma^2 / 2) + sigma^3 / 6 whenever |sigma| < eps (the correctly rounded value at
 *   that size; no libm call is left in a perturbation) — and R, W = A Omega + B Omega^2 + C I, t = W upsilon in four branches:
 *     0  |sigma| < eps,  theta < eps   C = 1, A = 1/2, B = 1/6, R = I + Omega + Omega^2
 *     1  |sigma| < eps,  else          C = 1, A = (1 - cos) / theta^2, B = (theta - sin) / theta^3,
 *                                      R = I + (sin / theta) Omega + ((1 - cos) / theta^2) Omega^2
 *     2  else,           theta < eps   C = (s - 1) / sigma, A = ((sigma - 1) s + 1) / sigma^2,
 *                                      B = (s sigma^2 / 2 + s - 1 - sigma s) / sigma^3, R = I + Omega + Omega^2
 *     3  else,           else          C = (s - 1) / sigma, R as in 1, a = s sin, b = s cos, c = theta^2 + sigma^2,
 *                                      A = (a sigma + (1 - b) theta) / (theta c), B = (C - ((b - 1) sigma + a theta) / c) / theta^2
 *   (branch 2's B is the form that equals the matrix exponential; ORB-SLAM2's bundled g2o drops the "- 1".)
 *   oplus: sigma = 0 when fix_scale, then estimate = Sim3(update) * estimate.
 * Errors.  e12 = obs1 - cam1(project(S12.map(P2c))), e21 = obs2 - cam2(project(S12^-1.map(P1c))), project = (x / z, y / z),
 *   cam(v) = (v0 fx + cx, v1 fy + cy), chi2 = e0 e0 + e1 e1.  A non-positive depth is evaluated as written.
 * Jacobian, numeric as in g2o: column d = (1 / (2 delta)) (e(Sim3(+delta e_d) * S) - e(Sim3(-delta e_d) * S)), delta = 1e-9,
 *   d = 0 .. 6; with fix_scale column 6 is zero (oplus clears sigma).  The 14 perturbed Sim3 and their inverses do not depend
 *   on the edge: they are formed once per iteration (spfe_s3o_perturb).
 * Sums: SPFE_S3O_NSUM = 36 quantities per edge through the 256-slot tree of spfe_dust_math.h,
 *     q[0]                     rho0
 *     q[1 + i (i + 1) / 2 + j] (J0i rho1) J0j + (J1i rho1) J1j,  0 <= j <= i < 7
 *     q[29 + j]                -(rho1 (J0j e0 + J1j e1))
 *   term index 2 c for e12 and 2 c + 1 for e21 of served correspondence c (slot = term index % 256); a correspondence removed
 *   after round 1 keeps its index and contributes nothing.
 * Schedule.  optimize(iterations); a correspondence is BAD when chi2(e12) > th2 || chi2(e21) > th2 (doubles against the float
 *   th2) on the errors its edges hold when optimize() returns: those of the LAST trial, accepted or not.  Bad ones get
 *   matches12 = -1 and are removed (nBad).  nCorrespondences - nBad < min_kept: return 0 with the INPUT Sim3.  Otherwise
 *   optimize(nBad > 0 ? 2 * iterations : iterations) with lambda initialised afresh, the same test once more nulls entries and
 *   counts nIn.
 * Scw = S12 * Sim3(Rcw2, tcw2, 1) and its f32 4x4 form (s R | t; 0 0 0 1): spfe_s3o_scw, what Converter::toCvMat(g2o::Sim3)
 *   gives.  Every NaN is replaced by the quiet NaN (0x7fc00000 / 0x7ff8000000000000) before it is stored.
 */
#ifndef SPFE_SIM3OPT_MATH_H
#define SPFE_SIM3OPT_MATH_H

#include <stdint.h>

#include "spfe_dust_math.h"

#define SPFE_S3O_NSUM 36
#define SPFE_S3O_DIM 7
#define SPFE_S3O_DELTA 1e-9
#define SPFE_S3O_SCALAR (1.0 / (2 * SPFE_S3O_DELTA))
#define SPFE_S3O_EPS 0.00001
/* const float deltaHuber = sqrt(th2), th2 = 10: the double square root rounded to float (optimizer.cpp:1112) */
#define SPFE_S3O_HUBER_DELTA 3.1622776985168457 /* = (double)(float)sqrt(10.0), exactly */

typedef struct {
  double q[4]; /* x, y, z, w */
  double t[3];
  double s;
} spfe_s3o_sim;

/* Eigen: Quaternion * Vector3 = v + w (2 q x v) + q x (2 q x v) */
SPFE_DM void spfe_s3o_rot(const double q[4], const double p[3], double out[3]) {
  const double ux = 2.0 * (q[1] * p[2] - q[2] * p[1]);
  const double uy = 2.0 * (q[2] * p[0] - q[0] * p[2]);
  const double uz = 2.0 * (q[0] * p[1] - q[1] * p[0]);
  out[0] = p[0] + q[3] * ux + (q[1] * uz - q[2] * uy);
  out[1] = p[1] + q[3] * uy + (q[2] * ux - q[0] * uz);
  out[2] = p[2] + q[3] * uz + (q[0] * uy - q[1] * ux);
}

SPFE_DM void spfe_s3o_map(const spfe_s3o_sim *S, const double p[3], double out[3]) {
  double r[3];
  spfe_s3o_rot(S->q, p, r);
  out[0] = S->s * r[0] + S->t[0];
  out[1] = S->s * r[1] + S->t[1];
  out[2] = S->s * r[2] + S->t[2];
}

/* out = A * B (out may not alias) */
SPFE_DM void spfe_s3o_mul(const spfe_s3o_sim *A, const spfe_s3o_sim *B, spfe_s3o_sim *out) {
  const double *a4 = A->q, *b4 = B->q; /* Eigen quaternion product a * b */
  out->q[3] = a4[3] * b4[3] - a4[0] * b4[0] - a4[1] * b4[1] - a4[2] * b4[2];
  out->q[0] = a4[3] * b4[0] + a4[0] * b4[3] + a4[1] * b4[2] - a4[2] * b4[1];
  out->q[1] = a4[3] * b4[1] + a4[1] * b4[3] + a4[2] * b4[0] - a4[0] * b4[2];
  out->q[2] = a4[3] * b4[2] + a4[2] * b4[3] + a4[0] * b4[1] - a4[1] * b4[0];
  double r[3];
  spfe_s3o_rot(A->q, B->t, r);
  out->t[0] = A->s * r[0] + A->t[0];
  out->t[1] = A->s * r[1] + A->t[1];
  out->t[2] = A->s * r[2] + A->t[2];
  out->s = A->s * B->s;
}

SPFE_DM void spfe_s3o_inv(const spfe_s3o_sim *S, spfe_s3o_sim *out) {
  out->q[0] = -S->q[0]; out->q[1] = -S->q[1]; out->q[2] = -S->q[2]; out->q[3] = S->q[3];
  out->s = 1.0 / S->s;
  double r[3];
  spfe_s3o_rot(out->q, S->t, r);
  const double m = -out->s;
  out->t[0] = m * r[0]; out->t[1] = m * r[1]; out->t[2] = m * r[2];
}

/* exp(sigma) of the contract: the cubic below eps, libm's (the device's) exp elsewhere */
SPFE_DM double spfe_s3o_exp_sigma(double sigma) {
  if (fabs(sigma) < SPFE_S3O_EPS) return ((1.0 + sigma) + sigma * sigma / 2) + sigma * sigma * sigma / 6;
  return exp(sigma);
}

/* Sim3(update); returns the branch 0 .. 3 */
SPFE_DM int spfe_s3o_exp(const double u[SPFE_S3O_DIM], spfe_s3o_sim *E) {
  const double wx = u[0], wy = u[1], wz = u[2], sigma = u[6];
  const double theta = sqrt(wx * wx + wy * wy + wz * wz);
  const double s = spfe_s3o_exp_sigma(sigma);
  const double O[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
  double O2[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) O2[r * 3 + c] = O[r * 3] * O[c] + O[r * 3 + 1] * O[3 + c] + O[r * 3 + 2] * O[6 + c];
  const int small_sigma = fabs(sigma) < SPFE_S3O_EPS, small_theta = theta < SPFE_S3O_EPS;
  double A, B, C, ra = 1.0, rb = 1.0;
  if (small_sigma) {
    C = 1.0;
    if (small_theta) {
      A = 1. / 2.;
      B = 1. / 6.;
    } else {
      const double st = sin(theta), ct = cos(theta), theta2 = theta * theta;
      A = (1.0 - ct) / theta2;
      B = (theta - st) / (theta2 * theta);
      ra = st / theta;
      rb = (1.0 - ct) / theta2;
    }
  } else {
    C = (s - 1.0) / sigma;
    if (small_theta) {
      const double sigma2 = sigma * sigma;
      A = ((sigma - 1.0) * s + 1.0) / sigma2;
      B = (s * sigma2 / 2 + s - 1.0 - sigma * s) / (sigma2 * sigma);
    } else {
      const double st = sin(theta), ct = cos(theta), theta2 = theta * theta;
      ra = st / theta;
      rb = (1.0 - ct) / theta2;
      const double a = s * st, b = s * ct, c = theta2 + sigma * sigma;
      A = (a * sigma + (1.0 - b) * theta) / (theta * c);
      B = (C - ((b - 1.0) * sigma + a * theta) / c) / theta2;
    }
  }
  double R[9], W[9];
  for (int i = 0; i < 9; ++i) {
    const double I = (i % 4 == 0) ? 1.0 : 0.0;
    R[i] = I + ra * O[i] + rb * O2[i];
    W[i] = A * O[i] + B * O2[i] + C * I;
  }
  spfe_quat_from_rot(R, E->q);
  for (int r = 0; r < 3; ++r) E->t[r] = W[r * 3] * u[3] + W[r * 3 + 1] * u[4] + W[r * 3 + 2] * u[5];
  E->s = s;
  return (small_sigma ? 0 : 2) + (small_theta ? 0 : 1);
}

/* VertexSim3Expmap::oplusImpl: S = Sim3(update) * S; returns the branch */
SPFE_DM int spfe_s3o_oplus(spfe_s3o_sim *S, const double upd[SPFE_S3O_DIM], int fix_scale) {
  double u[SPFE_S3O_DIM];
  for (int j = 0; j < SPFE_S3O_DIM; ++j) u[j] = upd[j];
  if (fix_scale) u[6] = 0.0;
  spfe_s3o_sim E, N;
  const int branch = spfe_s3o_exp(u, &E);
  spfe_s3o_mul(&E, S, &N);
  *S = N;
  return branch;
}

/* the perturbed estimate of linearizeOplus and its inverse: p = 2 d + (minus ? 1 : 0), d = 0 .. 6 */
SPFE_DM void spfe_s3o_perturb(const spfe_s3o_sim *S, int p, int fix_scale, spfe_s3o_sim *fwd, spfe_s3o_sim *inv) {
  double u[SPFE_S3O_DIM];
  for (int j = 0; j < SPFE_S3O_DIM; ++j) u[j] = (j == (p >> 1)) ? ((p & 1) ? -SPFE_S3O_DELTA : SPFE_S3O_DELTA) : 0.0;
  *fwd = *S;
  spfe_s3o_oplus(fwd, u, fix_scale);
  spfe_s3o_inv(fwd, inv);
}

/* g2o::Sim3(R, t, s) of the f32 T12 = (s, R[9] row-major, t[3]) */
SPFE_DM void spfe_s3o_from_f32(const float T12[13], spfe_s3o_sim *S) {
  double R[9];
  for (int i = 0; i < 9; ++i) R[i] = (double)T12[1 + i];
  spfe_quat_from_rot(R, S->q);
  S->t[0] = (double)T12[10]; S->t[1] = (double)T12[11]; S->t[2] = (double)T12[12];
  S->s = (double)T12[0];
}

SPFE_DM double spfe_s3o_canon(double x) {
  if (x == x) return x;
  const uint64_t u = 0x7ff8000000000000ull;
  double d;
  __builtin_memcpy(&d, &u, 8);
  return d;
}
SPFE_DM float spfe_s3o_canonf(float x) {
  if (x == x) return x;
  const uint32_t u = 0x7fc00000u;
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}

/* the output forms: S12[13] = (s, R row-major from the quaternion, t) in double and the same cast to float */
SPFE_DM void spfe_s3o_store(const spfe_s3o_sim *S, double S12[13], float T12[13]) {
  double R[9];
  spfe_quat_to_rot(S->q, R);
  S12[0] = spfe_s3o_canon(S->s);
  for (int i = 0; i < 9; ++i) S12[1 + i] = spfe_s3o_canon(R[i]);
  for (int i = 0; i < 3; ++i) S12[10 + i] = spfe_s3o_canon(S->t[i]);
  for (int i = 0; i < 13; ++i) T12[i] = spfe_s3o_canonf((float)S12[i]);
}
/* the echo of the input (nothing optimised, or too few kept): the f32 input and its widening */
SPFE_DM void spfe_s3o_store_echo(const float T12_in[13], double S12[13], float T12[13]) {
  for (int i = 0; i < 13; ++i) {
    T12[i] = T12_in[i];
    S12[i] = (double)T12_in[i];
  }
}

/* mg2oScw = S12 * Sim3(Rcw2, tcw2, 1) from the stored S12[13] and the f32 pose of keyframe 2, as a double similarity */
SPFE_DM void spfe_s3o_scw_sim(const double S12[13], const float Tcw2[16], spfe_s3o_sim *P) {
  spfe_s3o_sim A, B;
  double R[9];
  spfe_quat_from_rot(S12 + 1, A.q);
  A.t[0] = S12[10]; A.t[1] = S12[11]; A.t[2] = S12[12];
  A.s = S12[0];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) R[r * 3 + c] = (double)Tcw2[r * 4 + c];
    B.t[r] = (double)Tcw2[r * 4 + 3];
  }
  spfe_quat_from_rot(R, B.q);
  B.s = 1.0;
  spfe_s3o_mul(&A, &B, P);
}
/* Converter::toCvMat(g2o::Sim3): the row-major 4x4 (s R | t; 0 0 0 1) narrowed to f32, NaNs canonical */
SPFE_DM void spfe_s3o_sim_to_f32(const spfe_s3o_sim *P, float Scw[16]) {
  double R[9];
  spfe_quat_to_rot(P->q, R);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Scw[r * 4 + c] = spfe_s3o_canonf((float)(P->s * R[r * 3 + c]));
    Scw[r * 4 + 3] = spfe_s3o_canonf((float)P->t[r]);
  }
  Scw[12] = Scw[13] = Scw[14] = 0.0f;
  Scw[15] = 1.0f;
}
/* mScw = toCvMat(mg2oScw) */
SPFE_DM void spfe_s3o_scw(const double S12[13], const float Tcw2[16], float Scw[16]) {
  spfe_s3o_sim P;
  spfe_s3o_scw_sim(S12, Tcw2, &P);
  spfe_s3o_sim_to_f32(&P, Scw);
}

/* e = obs - cam(project(M.map(P))): M = S12 with P = P2c for e12, M = S12^-1 with P = P1c for e21 */
SPFE_DM void spfe_s3o_error(const spfe_s3o_sim *M, const double P[3], double fx, double fy, double cx, double cy, double ox,
                            double oy, double e[2]) {
  double p[3];
  spfe_s3o_map(M, P, p);
  const double px = p[0] / p[2], py = p[1] / p[2];
  e[0] = ox - (px * fx + cx);
  e[1] = oy - (py * fy + cy);
}

SPFE_DM double spfe_s3o_chi2(const double e[2]) { return e[0] * e[0] + e[1] * e[1]; }

SPFE_DM double spfe_s3o_rho0(double c) {
  double rho[3];
  spfe_huber(c, SPFE_S3O_HUBER_DELTA, rho);
  return rho[0];
}

/* column d of the numeric Jacobian from the errors at the two perturbed estimates */
SPFE_DM void spfe_s3o_jcol(const double ep[2], const double em[2], double *J0d, double *J1d) {
  *J0d = SPFE_S3O_SCALAR * (ep[0] - em[0]);
  *J1d = SPFE_S3O_SCALAR * (ep[1] - em[1]);
}

/* the 36 quantities of one edge */
SPFE_DM void spfe_s3o_terms(const double e[2], const double J0[SPFE_S3O_DIM], const double J1[SPFE_S3O_DIM],
                            double q[SPFE_S3O_NSUM]) {
  double rho[3];
  spfe_huber(spfe_s3o_chi2(e), SPFE_S3O_HUBER_DELTA, rho);
  q[0] = rho[0];
  for (int i = 0; i < SPFE_S3O_DIM; ++i)
    for (int j = 0; j <= i; ++j) q[1 + i * (i + 1) / 2 + j] = (J0[i] * rho[1]) * J0[j] + (J1[i] * rho[1]) * J1[j];
  for (int j = 0; j < SPFE_S3O_DIM; ++j) q[29 + j] = -(rho[1] * (J0[j] * e[0] + J1[j] * e[1]));
}

SPFE_DM void spfe_s3o_unpack(const double tot[SPFE_S3O_NSUM], double H[49], double b[SPFE_S3O_DIM]) {
  for (int i = 0; i < SPFE_S3O_DIM; ++i)
    for (int j = 0; j <= i; ++j) H[i * 7 + j] = H[j * 7 + i] = tot[1 + i * (i + 1) / 2 + j];
  for (int j = 0; j < SPFE_S3O_DIM; ++j) b[j] = tot[29 + j];
}

/* spfe_solve6 at dimension 7: (H + lambda I) x = b, unpivoted L D L^T, positive = every pivot > 0; x = 0 when not */
SPFE_DM int spfe_solve7(const double H[49], double lambda, const double b[7], double x[7]) {
  double L[49], U[49], rD[7];
  int ok = 1;
  for (int j = 0; j < 7; ++j) {
    for (int i = j; i < 7; ++i) {
      double s = H[i * 7 + j] + (i == j ? lambda : 0.0);
      for (int k = 0; k < j; ++k) s -= L[i * 7 + k] * U[j * 7 + k];
      U[i * 7 + j] = s;
    }
    ok &= U[j * 7 + j] > 0.0;
    rD[j] = 1.0 / U[j * 7 + j];
    for (int i = j + 1; i < 7; ++i) L[i * 7 + j] = U[i * 7 + j] * rD[j];
  }
  double z[7];
  for (int i = 0; i < 7; ++i) {
    double s = b[i];
    for (int k = 0; k < i; ++k) s -= L[i * 7 + k] * z[k];
    z[i] = s;
  }
  for (int i = 6; i >= 0; --i) {
    double s = z[i] * rD[i];
    for (int k = i + 1; k < 7; ++k) s -= L[k * 7 + i] * x[k];
    x[i] = s;
  }
  if (!ok)
    for (int i = 0; i < 7; ++i) x[i] = 0.0;
  return ok;
}

/* spfe_lm_judge at dimension 7 (the same constants and the same order of operations) */
SPFE_DM int spfe_s3o_lm_judge(spfe_lm *lm, double currentChi, double tempChi, const double x[7], const double b[7],
                              double *rho_out) {
  double rho = currentChi - tempChi;
  double scale = 0;
  for (int j = 0; j < 7; ++j) scale += x[j] * (lm->lambda * x[j] + b[j]);
  scale += 1e-3;
  rho /= scale;
  *rho_out = rho;
  if (rho > 0 && isfinite(tempChi)) {
    const double d = 2 * rho - 1;
    double alpha = 1. - d * d * d;
    alpha = alpha < SPFE_LM_GOOD_HI ? alpha : SPFE_LM_GOOD_HI;
    const double sf = SPFE_LM_GOOD_LO > alpha ? SPFE_LM_GOOD_LO : alpha;
    lm->lambda *= sf;
    lm->ni = 2;
    return 1;
  }
  lm->lambda *= lm->ni;
  lm->ni *= 2;
  return 0;
}

#endif /* SPFE_SIM3OPT_MATH_H */
