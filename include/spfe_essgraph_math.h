/*
 * spfe_essgraph_math.h — the arithmetic of the loop closer's pose graph over Sim3 and of its map corrections, shared by the GPU
 * kernels (sp_orb_slam_amd/csrc/essgraph.hip) and the host C reference of the test suite (tests/eg_ref/eg_ref.c) so that both
 * evaluate the same sequence of IEEE operations (compile with -ffp-contract=off).  Everything is computed in doubles.
 *
 * What it restates:
 *   Optimizer::OptimizeEssentialGraph    orb_slam2/src/mapping/optimizer.cpp:776-1060
 *   the map-point corrections of LoopClosingVLAD::CorrectLoop   loop_closer_vlad.cpp:575-606 and optimizer.cpp:1029-1059
 *   and, of g2o (a catkin dependency of the reference, NOT part of the reference snapshot — parity unpinned, published
 *   algorithm restated; THIS HEADER IS THE DEFINITION): Sim3::log, EdgeSim3::computeError, BaseBinaryEdge::linearizeOplus
 *   (numeric), constructQuadraticForm, a sparse Cholesky solve, OptimizationAlgorithmLevenberg::solve.  The Sim3 type, its
 *   product, inverse, map, exponential and oplus are spfe_sim3opt_math.h's, the quaternion helpers, the 256-slot tree and the
 *   Levenberg constants spfe_dust_math.h's, all unchanged.  One thing is NOT reused: an applied update goes through
 *   spfe_eg_oplus, which is spfe_s3o_oplus with the sin, cos and exp of this header.  Measured on an MI355X: with libm's, the
 *   device and glibc differ in a last bit on some of the thousand arguments a large graph meets, the numeric Jacobian of the
 *   next iteration multiplies that by 5e8, and the trial counts at the rounding floor come apart (10 iterations against 4).
 *
 * Vertices.  Slot v of n carries Scw_est[v] (vScw: CorrectedSim3 where it exists, else Sim3(Rcw, tcw, 1); the start value) and
 *   Scw_meas[v] (NonCorrectedSim3 where it exists, else vScw), each f64[8] = q(x, y, z, w), t, s.  flags[v] bit 0: fixed.  The
 *   slot order is the elimination order.
 * Edges.  int32 (i, j, kind): kind 0 measures on Scw_est, kind 1 on Scw_meas: Sji = S_j * inverse(S_i) (spfe_eg_measure),
 *   formed once.  FOLLOWED: 0 <= i, j < n, i != j, kind in {0, 1} (spfe_eg_edge_ok); every other edge is skipped, nothing of it is
 *   read.
 * Error.  e = log(Sji * Si * inverse(Sj)) (spfe_eg_error: two spfe_s3o_mul, left to right), information = identity, no robust
 *   kernel, chi2 = ((((((e0 e0 + e1 e1) + e2 e2) + e3 e3) + e4 e4) + e5 e5) + e6 e6).
 * Sim3::log (spfe_eg_log), with log, acos, sin and cos those of THIS header (spfe_eg_ln, spfe_eg_acos, spfe_eg_sincos: + - * /
 *   sqrt alone, no libm call in an error or a Jacobian): sigma = log(s), R = spfe_quat_to_rot(q), d = 0.5 (((R00 + R11) + R22) - 1), dR = (R21 - R12,
 *   R02 - R20, R10 - R01), eps = 1e-5:
 *     0  |sigma| < eps,  d > 1 - eps   omega = 0.5 dR, C = 1, A = 1/2, B = 1/6
 *     1  |sigma| < eps,  else          theta = acos(d), omega = (theta / (2 sqrt(1 - d d))) dR, C = 1,
 *                                      A = (1 - cos) / theta^2, B = (theta - sin) / theta^3
 *     2  else,           d > 1 - eps   omega = 0.5 dR, C = (s - 1) / sigma, A = ((sigma - 1) s + 1) / sigma^2,
 *                                      B = (s sigma^2 / 2 + s - 1 - sigma s) / sigma^3      (spfe_s3o_exp's branch-2 form)
 *     3  else,           else          theta, omega as in 1, C as in 2, a = s sin, b = s cos, c = theta^2 + sigma^2,
 *                                      A = (a sigma + (1 - b) theta) / (theta c), B = (C - ((b - 1) sigma + a theta) / c) / theta^2
 *   W = A Omega + B Omega^2 + C I, upsilon = W^-1 t by cofactors over the determinant (spfe_eg_solve3), e = (omega, upsilon, sigma).
 * Jacobians, numeric: column d of a non-fixed vertex = (1 / (2 delta)) (e(+) - e(-)), the estimate of that vertex replaced by
 *   spfe_s3o_perturb's (its inverse for vertex j), delta = SPFE_S3O_DELTA.  With fix_scale column 6 comes out zero (oplus clears
 *   sigma, both perturbed estimates are the same).  A fixed vertex has no Jacobian.
 * Unknowns: the non-fixed vertices with at least one followed edge, numbered u = 0 .. U - 1 in slot order.  Every other vertex
 *   keeps its estimate bit for bit.
 *
 * THE ORDER OF EVERY SUM.
 *   (a) H_uu (7x7) and b_u: 0.0, then for the followed edges of the vertex in ascending edge index: H_uu[r][c] += t,
 *       t = spfe_eg_dot7 of columns r and c of the vertex's Jacobian (products added in ascending error row, starting from the
 *       first product); b_u[r] -= spfe_eg_dot7(column r, e).
 *   (b) H_uw (u > w, rows: u's parameters, columns: w's): 0.0, then for the edges of that unordered pair in ascending edge index
 *       += spfe_eg_dot7(column r of J_u, column c of J_w).  Duplicate edges are legal.
 *   (c) chi2 of a state: the 256-slot tree, slot = edge index % 256, followed edges only.
 *   (d) the gain ratio's scale: the tree over x_j (lambda x_j + b_j), j = 7 u + r, slot = j % 256; then + 1e-3.
 *   (e) the solve of (H + lambda I) x = b: block skyline Cholesky in unknown order.  first(u) = the least unknown adjacent to u,
 *       or u; row u stores blocks first(u) .. u (spfe_eg_envelope counts them); ALL entries inside the envelope take part, zero
 *       or not.  With fs(i) = 7 first(i / 7) for scalar row i:
 *         L[i][j] = (A[i][j] - sum_{k = max(fs(i), fs(j))}^{j - 1} L[i][k] L[j][k]) / L[j][j]      j < i, j >= fs(i)
 *         L[j][j] = sqrt(A[j][j] - sum_{k = fs(j)}^{j - 1} L[j][k] L[j][k])
 *       every product subtracted from the running value in ascending k, starting from the matrix entry (left- and right-looking
 *       orders give the same bits); a running diagonal that is not > 0 or not finite: SOLVE FAILED (spfe_eg_pivot_ok).
 *       z[i] = (b[i] - sum_{k = fs(i)}^{i - 1} L[i][k] z[k]) / L[i][i], ascending k;
 *       x[i] = (z[i] - sum_{k > i, fs(k) <= i} L[k][i] x[k]) / L[i][i], DESCENDING k.
 * Schedule: OptimizationAlgorithmLevenberg as spfe_lm_judge restates it (spfe_eg_lm_judge: the scale handed in), lambda =
 *   lambda_init (1e-16: setUserLambdaInit) and ni = 2 before the first iteration; per iteration errors + chi2 at the estimate
 *   (kept from an accepted trial), Jacobians, (a) (b), then at most SPFE_LM_MAX_TRIALS trials: solve, spfe_eg_oplus on every unknown,
 *   chi2 at the candidate, judge; a rejected candidate is restored.  A failed solve applies nothing: scale = 0 + 1e-3, tempChi =
 *   DBL_MAX, counted in n_solve_failed.  The run ends after `iterations` iterations, after a trial with rho == 0 or after the
 *   tenth trial of an iteration.  U == 0: nothing runs (EMPTY).
 * Recovery: Sim3 out = the estimate, NaNs canonical; Tiw = [R(q) | t * (1 / s)] as f32 (spfe_loopfuse_se3_to_f32's form).
 * Point correction: X f32 widened, Y = inverse(S_to[r]).map(S_from[r].map(X)), narrowed entry by entry (spfe_eg_correct_point).
 * Start values of the graph (spfe_eg_from_pose / spfe_eg_corrected): Sim3(quat(R), t, 1) of an f32 pose, and for a connected
 *   keyframe Sic * Scw in double — what spfe_loopfuse_pose forms before it narrows.
 */
#ifndef SPFE_ESSGRAPH_MATH_H
#define SPFE_ESSGRAPH_MATH_H

#include "spfe_sim3opt_math.h"

#define SPFE_EG_DIM 7
#define SPFE_EG_BLOCK 49
#define SPFE_EG_DBL_MAX 1.7976931348623157e308

SPFE_DM void spfe_eg_load(const double *p, spfe_s3o_sim *S) {
  S->q[0] = p[0]; S->q[1] = p[1]; S->q[2] = p[2]; S->q[3] = p[3];
  S->t[0] = p[4]; S->t[1] = p[5]; S->t[2] = p[6];
  S->s = p[7];
}
SPFE_DM void spfe_eg_store(const spfe_s3o_sim *S, double *p) {
  p[0] = S->q[0]; p[1] = S->q[1]; p[2] = S->q[2]; p[3] = S->q[3];
  p[4] = S->t[0]; p[5] = S->t[1]; p[6] = S->t[2];
  p[7] = S->s;
}
SPFE_DM void spfe_eg_store_canon(const spfe_s3o_sim *S, double *p) {
  double v[8];
  spfe_eg_store(S, v);
  for (int i = 0; i < 8; ++i) p[i] = spfe_s3o_canon(v[i]);
}

SPFE_DM int spfe_eg_edge_ok(int i, int j, int kind, int n) {
  return i >= 0 && i < n && j >= 0 && j < n && i != j && (kind == 0 || kind == 1);
}

/* Sji = S_j * inverse(S_i) */
SPFE_DM void spfe_eg_measure(const spfe_s3o_sim *Si, const spfe_s3o_sim *Sj, spfe_s3o_sim *Sji) {
  spfe_s3o_sim inv;
  spfe_s3o_inv(Si, &inv);
  spfe_s3o_mul(Sj, &inv, Sji);
}

/* x = W^-1 t, W row-major 3x3: cofactors over the determinant, no test */
SPFE_DM void spfe_eg_solve3(const double W[9], const double t[3], double x[3]) {
  const double c0 = W[4] * W[8] - W[5] * W[7];
  const double c1 = W[5] * W[6] - W[3] * W[8];
  const double c2 = W[3] * W[7] - W[4] * W[6];
  const double det = (W[0] * c0 + W[1] * c1) + W[2] * c2;
  x[0] = ((c0 * t[0] + (W[2] * W[7] - W[1] * W[8]) * t[1]) + (W[1] * W[5] - W[2] * W[4]) * t[2]) / det;
  x[1] = ((c1 * t[0] + (W[0] * W[8] - W[2] * W[6]) * t[1]) + (W[2] * W[3] - W[0] * W[5]) * t[2]) / det;
  x[2] = ((c2 * t[0] + (W[1] * W[6] - W[0] * W[7]) * t[1]) + (W[0] * W[4] - W[1] * W[3]) * t[2]) / det;
}


/* ---- the four elementary functions of Sim3::log, from + - * / sqrt alone, so that the kernel and the host reference evaluate
 * the same bits whatever libm either side links (the numeric Jacobian multiplies a last-place difference of two errors by
 * 5e8).  Each is a fixed reduction and a fixed Horner chain; they agree with the correctly rounded functions to a few units in
 * the last place (tests/test_essgraph_reference.py measures it). */
#define SPFE_EG_PI 3.141592653589793
#define SPFE_EG_PI_2 1.5707963267948966
#define SPFE_EG_PI_4 0.7853981633974483
#define SPFE_EG_LN2 0.6931471805599453
#define SPFE_EG_LN2_HI 0.6931471803691238    /* 0x3fe62e42fee00000 */
#define SPFE_EG_LN2_LO 1.9082149292705877e-10 /* ln 2 - LN2_HI */
#define SPFE_EG_SQRT2 1.4142135623730951

SPFE_DM double spfe_eg_horner(const double *c, int n, double z) {
  double p = c[n - 1];
  for (int k = n - 2; k >= 0; --k) p = p * z + c[k];
  return p;
}

/* ln(s): s = m 2^k, m in (sqrt(1/2), sqrt(2)], f = (m - 1) / (m + 1), ln m = 2 f (1 + f^2 / 3 + ... + f^24 / 25); not positive
 * or not finite: NaN */
SPFE_DM double spfe_eg_ln(double s) {
  if (!(s > 0.0) || !(s <= SPFE_EG_DBL_MAX)) {
    const double z = s - s;
    return spfe_s3o_canon(z / z);
  }
  const double c[13] = {1.0, 0.3333333333333333, 0.2, 0.14285714285714285, 0.1111111111111111, 0.09090909090909091,
                        0.07692307692307693, 0.06666666666666667, 0.058823529411764705, 0.05263157894736842, 0.047619047619047616,
                        0.043478260869565216, 0.04};
  int k = 0;
  if (s < 2.2250738585072014e-308) {
    s *= 18014398509481984.0; /* 2^54 */
    k = -54;
  }
  uint64_t bits;
  __builtin_memcpy(&bits, &s, 8);
  k += (int)((bits >> 52) & 0x7ff) - 1023;
  bits = (bits & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
  double m;
  __builtin_memcpy(&m, &bits, 8);
  if (m > SPFE_EG_SQRT2) {
    m *= 0.5;
    ++k;
  }
  const double f = (m - 1.0) / (m + 1.0);
  const double r = 2.0 * f * spfe_eg_horner(c, 13, f * f);
  return (double)k * SPFE_EG_LN2 + r;
}

/* asin(x) for |x| <= 1/2: x (1 + x^2 / 6 + 3 x^4 / 40 + ...), 26 terms */
SPFE_DM double spfe_eg_asin_half(double x) {
  const double c[26] = {1.0, 0.16666666666666666, 0.075, 0.044642857142857144, 0.030381944444444444, 0.022372159090909092,
                        0.017352764423076924, 0.01396484375, 0.011551800896139705, 0.009761609529194078, 0.008390335809616815,
                        0.0073125258735988454, 0.006447210311889649, 0.005740037670841924, 0.005153309682319905,
                        0.004660143486915096, 0.004240907093679363, 0.003880964558837669, 0.0035692053938259347,
                        0.003297059503473485, 0.0030578216492580306, 0.002846178401108942, 0.00265787063820729,
                        0.0024894486782468836, 0.002338091892111975, 0.0022014739737101384};
  return x * spfe_eg_horner(c, 26, x * x);
}
/* acos(d): 2 asin(sqrt((1 - d) / 2)) for d >= 1/2, pi / 2 - asin(d) for |d| < 1/2, pi - 2 asin(sqrt((1 + d) / 2)) below; |d| > 1
 * gives the NaN of the square root */
SPFE_DM double spfe_eg_acos(double d) {
  if (d >= 0.5) return 2.0 * spfe_eg_asin_half(sqrt((1.0 - d) * 0.5));
  if (d > -0.5) return SPFE_EG_PI_2 - spfe_eg_asin_half(d);
  return SPFE_EG_PI - 2.0 * spfe_eg_asin_half(sqrt((1.0 + d) * 0.5));
}
/* sin and cos of x in [0, pi] (what spfe_eg_acos gives): x > pi / 2 -> pi - x (the cosine changes sign), then x > pi / 4 ->
 * pi / 2 - x (the two change places), then the Taylor chains to x^19 and x^20 */
SPFE_DM void spfe_eg_sincos(double x, double *sn, double *cs) {
  const double a[10] = {1.0, -0.16666666666666666, 0.008333333333333333, -0.0001984126984126984, 2.7557319223985893e-06,
                        -2.505210838544172e-08, 1.6059043836821613e-10, -7.647163731819816e-13, 2.8114572543455206e-15,
                        -8.22063524662433e-18};
  const double b[11] = {1.0, -0.5, 0.041666666666666664, -0.001388888888888889, 2.48015873015873e-05, -2.755731922398589e-07,
                        2.08767569878681e-09, -1.1470745597729725e-11, 4.779477332387385e-14, -1.5619206968586225e-16,
                        4.110317623312165e-19};
  const int neg = x > SPFE_EG_PI_2;
  if (neg) x = SPFE_EG_PI - x;
  const int swap = x > SPFE_EG_PI_4;
  if (swap) x = SPFE_EG_PI_2 - x;
  const double z = x * x;
  const double ss = x * spfe_eg_horner(a, 10, z), cc = spfe_eg_horner(b, 11, z);
  *sn = swap ? cc : ss;
  const double co = swap ? ss : cc;
  *cs = neg ? -co : co;
}

/* sin and cos of any x >= 0 (the angle of an update): beyond pi, x - floor(x / 2 pi) 2 pi, mirrored about pi (the sine changes
 * sign); what rounding leaves outside [0, pi] is clamped */
SPFE_DM void spfe_eg_sincos_any(double x, double *sn, double *cs) {
  int flip = 0;
  if (x > SPFE_EG_PI) {
    x = x - floor(x / (2.0 * SPFE_EG_PI)) * (2.0 * SPFE_EG_PI);
    if (x > SPFE_EG_PI) {
      x = 2.0 * SPFE_EG_PI - x;
      flip = 1;
    }
    if (x < 0.0) x = 0.0;
    if (x > SPFE_EG_PI) x = SPFE_EG_PI;
  }
  spfe_eg_sincos(x, sn, cs);
  if (flip) *sn = -*sn;
}
/* exp(x): the cubic of spfe_s3o_exp_sigma below eps; else x clamped to [-708, 709], k = the integer nearest x / ln 2, r = x - k ln 2 (ln 2 in two parts),
 * the Taylor chain to r^14 / 14!, times 2^k */
SPFE_DM double spfe_eg_exp(double x) {
  if (fabs(x) < SPFE_S3O_EPS) return ((1.0 + x) + x * x / 2) + x * x * x / 6;
  if (!(x == x)) return spfe_s3o_canon(x);
  const double c[15] = {1.0, 1.0, 0.5, 0.16666666666666666, 0.041666666666666664, 0.008333333333333333, 0.001388888888888889, 0.0001984126984126984, 2.48015873015873e-05, 2.7557319223985893e-06, 2.755731922398589e-07, 2.505210838544172e-08, 2.08767569878681e-09, 1.6059043836821613e-10, 1.1470745597729725e-11};
  if (x > 709.0) x = 709.0;
  if (x < -708.0) x = -708.0;
  const double y = x * 1.4426950408889634; /* x / ln 2 */
  const int k = (int)(y + (y < 0.0 ? -0.5 : 0.5)); /* the nearest integer, by truncation: |y| < 1024 */
  const double kd = (double)k;
  const double r = (x - kd * SPFE_EG_LN2_HI) - kd * SPFE_EG_LN2_LO; /* kd LN2_HI is exact: LN2_HI ends in 21 zero bits */
  const uint64_t bits = (uint64_t)(k + 1023) << 52;
  double p2;
  __builtin_memcpy(&p2, &bits, 8);
  return spfe_eg_horner(c, 15, r) * p2;
}

/* Sim3(update) and oplus of an APPLIED update: spfe_s3o_exp / spfe_s3o_oplus with sin, cos and exp those of this header (the
 * perturbations of the Jacobian stay spfe_s3o_perturb's: below eps neither calls any).  Returns the branch. */
SPFE_DM int spfe_eg_exp_update(const double u[SPFE_EG_DIM], spfe_s3o_sim *E) {
  const double wx = u[0], wy = u[1], wz = u[2], sigma = u[6];
  const double theta = sqrt(wx * wx + wy * wy + wz * wz);
  const double s = spfe_eg_exp(sigma);
  const double O[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
  double O2[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) O2[r * 3 + c] = O[r * 3] * O[c] + O[r * 3 + 1] * O[3 + c] + O[r * 3 + 2] * O[6 + c];
  const int small_sigma = fabs(sigma) < SPFE_S3O_EPS, small_theta = theta < SPFE_S3O_EPS;
  double A, B, C, ra = 1.0, rb = 1.0, st = 0.0, ct = 1.0;
  const double theta2 = theta * theta;
  if (!small_theta) {
    spfe_eg_sincos_any(theta, &st, &ct);
    ra = st / theta;
    rb = (1.0 - ct) / theta2;
  }
  if (small_sigma) {
    C = 1.0;
    if (small_theta) {
      A = 1. / 2.;
      B = 1. / 6.;
    } else {
      A = (1.0 - ct) / theta2;
      B = (theta - st) / (theta2 * theta);
    }
  } else {
    C = (s - 1.0) / sigma;
    if (small_theta) {
      const double sigma2 = sigma * sigma;
      A = ((sigma - 1.0) * s + 1.0) / sigma2;
      B = (s * sigma2 / 2 + s - 1.0 - sigma * s) / (sigma2 * sigma);
    } else {
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
SPFE_DM int spfe_eg_oplus(spfe_s3o_sim *S, const double upd[SPFE_EG_DIM], int fix_scale) {
  double u[SPFE_EG_DIM];
  for (int j = 0; j < SPFE_EG_DIM; ++j) u[j] = upd[j];
  if (fix_scale) u[6] = 0.0;
  spfe_s3o_sim E, N;
  const int branch = spfe_eg_exp_update(u, &E);
  spfe_s3o_mul(&E, S, &N);
  *S = N;
  return branch;
}

/* Sim3::log; returns the branch 0 .. 3 */
SPFE_DM int spfe_eg_log(const spfe_s3o_sim *S, double e[SPFE_EG_DIM]) {
  const double s = S->s;
  const double sigma = spfe_eg_ln(s);
  double R[9];
  spfe_quat_to_rot(S->q, R);
  const double d = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
  const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
  const int small_sigma = fabs(sigma) < SPFE_S3O_EPS, small_theta = d > 1.0 - SPFE_S3O_EPS;
  double A, B, C, k;
  if (small_theta) {
    k = 0.5;
    if (small_sigma) {
      C = 1.0;
      A = 1. / 2.;
      B = 1. / 6.;
    } else {
      const double sigma2 = sigma * sigma;
      C = (s - 1.0) / sigma;
      A = ((sigma - 1.0) * s + 1.0) / sigma2;
      B = (s * sigma2 / 2 + s - 1.0 - sigma * s) / (sigma2 * sigma);
    }
  } else {
    const double theta = spfe_eg_acos(d), theta2 = theta * theta;
    double st, ct;
    spfe_eg_sincos(theta, &st, &ct);
    k = theta / (2.0 * sqrt(1.0 - d * d));
    if (small_sigma) {
      C = 1.0;
      A = (1.0 - ct) / theta2;
      B = (theta - st) / (theta2 * theta);
    } else {
      C = (s - 1.0) / sigma;
      const double a = s * st, b = s * ct, c = theta2 + sigma * sigma;
      A = (a * sigma + (1.0 - b) * theta) / (theta * c);
      B = (C - ((b - 1.0) * sigma + a * theta) / c) / theta2;
    }
  }
  const double wx = k * dR[0], wy = k * dR[1], wz = k * dR[2];
  const double O[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
  double W[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      const double o2 = O[r * 3] * O[c] + O[r * 3 + 1] * O[3 + c] + O[r * 3 + 2] * O[6 + c];
      W[r * 3 + c] = A * O[r * 3 + c] + B * o2 + C * (r == c ? 1.0 : 0.0);
    }
  e[0] = wx; e[1] = wy; e[2] = wz;
  spfe_eg_solve3(W, S->t, e + 3);
  e[6] = sigma;
  return (small_sigma ? 0 : 2) + (small_theta ? 0 : 1);
}

/* e = log(Sji * Si * inverse(Sj)), the inverse handed in */
SPFE_DM void spfe_eg_error(const spfe_s3o_sim *Sji, const spfe_s3o_sim *Si, const spfe_s3o_sim *Sj_inv, double e[SPFE_EG_DIM]) {
  spfe_s3o_sim A, B;
#ifdef SPFE_EG_MUT_SWAP
  spfe_s3o_sim Sj, Si_inv;   /* mutation: the vertices swapped */
  spfe_s3o_inv(Sj_inv, &Sj);
  spfe_s3o_inv(Si, &Si_inv);
  spfe_s3o_mul(Sji, &Sj, &A);
  spfe_s3o_mul(&A, &Si_inv, &B);
#else
  spfe_s3o_mul(Sji, Si, &A);
  spfe_s3o_mul(&A, Sj_inv, &B);
#endif
  spfe_eg_log(&B, e);
}

SPFE_DM double spfe_eg_dot7(const double *a, int sa, const double *b, int sb) {
  double s = a[0] * b[0];
  for (int k = 1; k < SPFE_EG_DIM; ++k) s = s + a[k * sa] * b[k * sb];
  return s;
}
SPFE_DM double spfe_eg_chi2(const double e[SPFE_EG_DIM]) { return spfe_eg_dot7(e, 1, e, 1); }

/* column d of the numeric Jacobian */
SPFE_DM void spfe_eg_jcol(const double ep[SPFE_EG_DIM], const double em[SPFE_EG_DIM], double *J, int d) {
  for (int k = 0; k < SPFE_EG_DIM; ++k) J[k * SPFE_EG_DIM + d] = SPFE_S3O_SCALAR * (ep[k] - em[k]);
}

SPFE_DM int spfe_eg_pivot_ok(double d) { return d > 0.0 && isfinite(d); }
SPFE_DM double spfe_eg_scale_term(double x, double lambda, double b) { return x * (lambda * x + b); }

/* spfe_lm_judge for 7 U parameters: `sum` = the tree of (d) */
SPFE_DM int spfe_eg_lm_judge(spfe_lm *lm, double currentChi, double tempChi, double sum, double *rho_out) {
  double rho = currentChi - tempChi;
  double scale = sum;
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

/* Sim3(quat(R), t, 1) of an f32 pose */
SPFE_DM void spfe_eg_from_pose(const float Tcw[16], spfe_s3o_sim *S) {
  double R[9];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) R[r * 3 + c] = (double)Tcw[r * 4 + c];
    S->t[r] = (double)Tcw[r * 4 + 3];
  }
  spfe_quat_from_rot(R, S->q);
  S->s = 1.0;
}

/* the corrected Sim3 of a connected keyframe in double: steps 1 - 4 of spfe_loopfuse_pose */
SPFE_DM void spfe_eg_corrected(const double S12[13], const float Tcw2[16], const float Twc[16], const float Tiw[16], int is_current,
                               spfe_s3o_sim *P) {
  spfe_s3o_sim Scw;
  spfe_s3o_scw_sim(S12, Tcw2, &Scw);
  if (is_current) {
    *P = Scw;
    return;
  }
  spfe_s3o_sim Sic;
  float Tic[12];
  double Ric[9];
  /* spfe_loopfuse_tic */
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) {
      double s = (double)Tiw[4 * r] * (double)Twc[c];
      s = s + (double)Tiw[4 * r + 1] * (double)Twc[4 + c];
      s = s + (double)Tiw[4 * r + 2] * (double)Twc[8 + c];
      s = s + (double)Tiw[4 * r + 3] * (double)Twc[12 + c];
      Tic[4 * r + c] = (float)s;
    }
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Ric[3 * r + c] = (double)Tic[4 * r + c];
    Sic.t[r] = (double)Tic[4 * r + 3];
  }
  spfe_quat_from_rot(Ric, Sic.q);
  Sic.s = 1.0;
  spfe_s3o_mul(&Sic, &Scw, P);
}

/* [R(q) | t * (1 / s)] as f32: spfe_loopfuse_se3_to_f32's form */
SPFE_DM void spfe_eg_recover(const spfe_s3o_sim *P, float T[16]) {
  double R[9];
  spfe_quat_to_rot(P->q, R);
#ifdef SPFE_EG_MUT_NO_TS
  const double inv = 1.0;
#else
  const double inv = 1.0 / P->s;
#endif
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T[r * 4 + c] = spfe_s3o_canonf((float)R[r * 3 + c]);
    T[r * 4 + 3] = spfe_s3o_canonf((float)(P->t[r] * inv));
  }
  T[12] = T[13] = T[14] = 0.0f;
  T[15] = 1.0f;
}

/* Y = inverse(S_to).map(S_from.map(X)) */
SPFE_DM void spfe_eg_correct_point(const spfe_s3o_sim *S_from, const spfe_s3o_sim *S_to, const float X[3], float Y[3]) {
  const double x[3] = {(double)X[0], (double)X[1], (double)X[2]};
  double w[3], y[3];
  spfe_s3o_map(S_from, x, w);
#ifdef SPFE_EG_MUT_NO_INV
  spfe_s3o_map(S_to, w, y);
#else
  spfe_s3o_sim inv;
  spfe_s3o_inv(S_to, &inv);
  spfe_s3o_map(&inv, w, y);
#endif
  for (int c = 0; c < 3; ++c) Y[c] = spfe_s3o_canonf((float)y[c]); /* every NaN leaves as the quiet NaN */
}

/* The symbolic step on the host: unk[v] = the unknown of slot v or -1 (may be NULL), first[u] (may be NULL; room for n),
 * -> the envelope's block count.  work: n ints. */
static inline long long spfe_eg_envelope(int n, const unsigned char *flags, const int *edges, int E, int *unk_out, int *first_out,
                                         int *n_unknown, int *work) {
  int *unk = work;
  for (int v = 0; v < n; ++v) unk[v] = 0;
  for (int e = 0; e < E; ++e) {
    const int i = edges[3 * e], j = edges[3 * e + 1];
    if (!spfe_eg_edge_ok(i, j, edges[3 * e + 2], n)) continue;
    unk[i] = 1;
    unk[j] = 1;
  }
  int U = 0;
  for (int v = 0; v < n; ++v) unk[v] = (unk[v] && !(flags[v] & 1)) ? U++ : -1;
  long long blocks = 0;
  if (first_out) {
    for (int u = 0; u < U; ++u) first_out[u] = u;
    for (int e = 0; e < E; ++e) {
      const int i = edges[3 * e], j = edges[3 * e + 1];
      if (!spfe_eg_edge_ok(i, j, edges[3 * e + 2], n)) continue;
      const int a = unk[i], b = unk[j];
      if (a < 0 || b < 0) continue;
      const int lo = a < b ? a : b, hi = a < b ? b : a;
      if (lo < first_out[hi]) first_out[hi] = lo;
    }
    for (int u = 0; u < U; ++u) blocks += u - first_out[u] + 1;
  }
  if (unk_out && unk_out != unk)
    for (int v = 0; v < n; ++v) unk_out[v] = unk[v];
  *n_unknown = U;
  return blocks;
}

#endif /* SPFE_ESSGRAPH_MATH_H */
