/*
 * pose_ref.c — host reference of the covariance-weighted pose refinement (sp_orb_slam_amd/csrc/pose.hip), built from
 * include/spfe_pose_math.h with the oracle's flags (gcc -O3 -mavx2 -mfma -ffp-contract=off -fno-fast-math) by the test
 * modules and loaded through ctypes.  It states the two schedules edge by edge and g2o call by call; the kernel must agree
 * with it in flags, counts and iteration counts, and in the pose up to the device's sin / cos.
 *
 *   SPFE_POSE_DUST_POST     Optimizer::PoseOptimizationDustPost   orb_slam2/src/mapping/optimizer_dust.cpp:35-167
 *   SPFE_POSE_OPTIMIZATION  Optimizer::PoseOptimization           orb_slam2/src/mapping/optimizer.cpp:231-443
 *
 * Sums: the 256-slot tree of spfe_dust_math.h; edge j (ascending keypoint order) feeds slot j % 256, edges that are not
 * active in an optimize() call (level 1 at initializeOptimization(0)) feed nothing.
 */
#include <stdint.h>
#include <string.h>

#include "../../include/spfe.h"
#include "../../include/spfe_pose_math.h"

#define API __attribute__((visibility("default")))

typedef struct {
  const float *obs, *w, *pts;
  int n;
  double fx, fy, cx, cy;
  uint8_t *level;   /* 1 = not active in the next optimize() */
  float *chi2f;     /* the chi2 g2o holds for the edge: the error of the last evaluation, rounded to float */
  int robust;
  /* what the coverage claims of the tests rest on: per optimize() call the trials, the longest run of rejected trials
   * inside one iteration's trial loop and the failed solves; over all classification rounds the smallest relative distance
   * of an edge's chi2 from its threshold */
  int call, trials[4], max_run[4], failed[4];
  double margin;
} problem;

static void edge_error(const problem *P, const spfe_se3 *T, int j, double p[3], double e[2]) {
  const double Xw[3] = {(double)P->pts[3 * j], (double)P->pts[3 * j + 1], (double)P->pts[3 * j + 2]};
  spfe_pose_error(T, Xw, P->fx, P->fy, P->cx, P->cy, (double)P->obs[2 * j], (double)P->obs[2 * j + 1], p, e);
}

/* computeActiveErrors + activeRobustChi2 */
static double active_chi2(problem *P, const spfe_se3 *T) {
  double s[SPFE_DUST_SLOTS];
  memset(s, 0, sizeof(s));
  for (int j = 0; j < P->n; ++j) {
    if (P->level[j]) continue;
    double p[3], e[2];
    edge_error(P, T, j, p, e);
    const double w0 = (double)P->w[2 * j], w1 = (double)P->w[2 * j + 1];
    P->chi2f[j] = spfe_pose_chi2f(e, w0, w1);
    s[j % SPFE_DUST_SLOTS] += spfe_pose_rho0(spfe_pose_chi2(e, w0, w1), P->robust);
  }
  return spfe_dust_tree_total(s);
}

/* buildSystem at T */
static void build(const problem *P, const spfe_se3 *T, double H[36], double b[6]) {
  static double s[SPFE_POSE_NSUM][SPFE_DUST_SLOTS];
  memset(s, 0, sizeof(s));
  for (int j = 0; j < P->n; ++j) {
    if (P->level[j]) continue;
    double p[3], e[2], A0[6], A1[6], q[SPFE_POSE_NSUM];
    edge_error(P, T, j, p, e);
    spfe_pose_jacobian(p, P->fx, P->fy, A0, A1);
    spfe_pose_terms(e, A0, A1, (double)P->w[2 * j], (double)P->w[2 * j + 1], P->robust, q);
    for (int k = 0; k < SPFE_POSE_NSUM; ++k) s[k][j % SPFE_DUST_SLOTS] += q[k];
  }
  double tot[SPFE_POSE_NSUM], chi;
  for (int k = 0; k < SPFE_POSE_NSUM; ++k) tot[k] = spfe_dust_tree_total(s[k]);
  spfe_dust_unpack(tot, &chi, H, b);
}

/* initializeOptimization(0); optimize(iterations): returns the iterations run, 0 where g2o returns -1 (no level-0 edge) */
static int optimize(problem *P, spfe_se3 *T, int iterations) {
  int active = 0;
  for (int j = 0; j < P->n; ++j) active += !P->level[j];
  if (!active) return 0;
  spfe_lm lm = {0.0, 2.0};
  int done = 0;
  for (int it = 0; it < iterations; ++it) {
    const double currentChi = active_chi2(P, T);
    double H[36], b[6];
    build(P, T, H, b);
    if (it == 0) {
      double maxDiagonal = 0;
      for (int j = 0; j < 6; ++j) maxDiagonal = fabs(H[j * 6 + j]) > maxDiagonal ? fabs(H[j * 6 + j]) : maxDiagonal;
      lm.lambda = SPFE_LM_TAU * maxDiagonal;
      lm.ni = 2;
    }
    double rho = 0, cur = currentChi;
    int qmax = 0, run = 0;
    do {
      double x[6];
      spfe_se3 Tt = *T;
      const int ok2 = spfe_solve6(H, lm.lambda, b, x);
      P->failed[P->call] += !ok2;
      if (ok2) spfe_se3_oplus(&Tt, x);
      double tempChi = active_chi2(P, &Tt);   /* the edges keep these errors, accepted or not */
      if (!ok2) tempChi = 1.7976931348623157e308;
      if (spfe_lm_judge(&lm, cur, tempChi, x, b, &rho)) { *T = Tt; cur = tempChi; run = 0; }
      else run++;
      if (run > P->max_run[P->call]) P->max_run[P->call] = run;
      P->trials[P->call]++;
      qmax++;
    } while (rho < 0 && qmax < SPFE_LM_MAX_TRIALS);
    done++;
    if (qmax == SPFE_LM_MAX_TRIALS || rho == 0) break;
  }
  return done;
}

/* classify edge j on the chi2 it holds (recomputed at T first when `fresh`) */
static int classify(problem *P, const spfe_se3 *T, int j, int fresh, int post) {
  if (fresh) {
    double p[3], e[2];
    edge_error(P, T, j, p, e);
    P->chi2f[j] = spfe_pose_chi2f(e, (double)P->w[2 * j], (double)P->w[2 * j + 1]);
  }
  const float chi2 = P->chi2f[j];
  const double thr = post ? SPFE_POSE_CHI2_POST : (double)SPFE_POSE_CHI2_MONO;
  const double m = fabs((double)chi2 - thr) / thr;
  if (!(m >= P->margin)) P->margin = m;   /* a NaN chi2 reads as margin NaN */
  const int bad = post ? ((double)chi2 > SPFE_POSE_CHI2_POST) : (chi2 > SPFE_POSE_CHI2_MONO);
  P->level[j] = (uint8_t)bad;
  return bad;
}

/* One solve.  obs / w / pts: [n][2] / [n][2] / [n][3] in edge order.  Tout: the pose (Tcw echoed when n < 3), pose64
 * (optional, [16]): the double pose before the cast; iters[4]: iterations per optimize() call.  level_scratch / chi2_scratch
 * ([n]) hold every edge's final level and float chi2 on return.  Optional: trials[4], max_rejected_run[4], failed_solves[4]
 * per optimize() call, and chi2_margin[1]: min over edges and classification rounds of |chi2 - threshold| / threshold
 * (infinity when nothing was classified).  Returns n_good. */
API int pose_ref_solve(const float *obs, const float *w, const float *pts, int n, const float *Tcw, float fx, float fy,
                       float cx, float cy, int schedule, int iterations, float *Tout, uint8_t *outlier, int *iters,
                       double *pose64, uint8_t *level_scratch, float *chi2_scratch, int *trials, int *max_rejected_run,
                       int *failed_solves, double *chi2_margin) {
  problem P = {obs, w, pts, n, (double)fx, (double)fy, (double)cx, (double)cy, level_scratch, chi2_scratch, 1,
               0, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, INFINITY};
  for (int k = 0; k < 4; ++k) iters[k] = 0;
  for (int k = 0; k < 4; ++k) {
    if (trials) trials[k] = 0;
    if (max_rejected_run) max_rejected_run[k] = 0;
    if (failed_solves) failed_solves[k] = 0;
  }
  if (chi2_margin) *chi2_margin = INFINITY;
  for (int j = 0; j < n; ++j) { outlier[j] = 0; P.level[j] = 0; P.chi2f[j] = 0.0f; }
  if (n < 3) {
    memcpy(Tout, Tcw, 64);
    if (pose64)
      for (int k = 0; k < 16; ++k) pose64[k] = (double)Tcw[k];
    return 0;
  }
  spfe_se3 T;
  int nBad = 0;
  if (schedule == SPFE_POSE_DUST_POST) {
    spfe_se3_from_f32(Tcw, &T);
    iters[0] = optimize(&P, &T, iterations);
    for (int j = 0; j < n; ++j) nBad += outlier[j] = (uint8_t)classify(&P, &T, j, 1, 1);
    P.robust = 0;
    P.call = 1;
    iters[1] = optimize(&P, &T, iterations);
  } else {
    for (int it = 0; it < 4; ++it) {
      P.call = it;
      spfe_se3_from_f32(Tcw, &T);   /* vSE3->setEstimate(toSE3Quat(pFrame->mTcw)): mTcw is written after the loop only */
      iters[it] = optimize(&P, &T, iterations);
      nBad = 0;
      for (int j = 0; j < n; ++j) nBad += outlier[j] = (uint8_t)classify(&P, &T, j, outlier[j], 0);
      if (it == 2) P.robust = 0;
      if (n < 10) break;
    }
  }
  spfe_se3_to_f32(&T, Tout);
  for (int k = 0; k < 4; ++k) {
    if (trials) trials[k] = P.trials[k];
    if (max_rejected_run) max_rejected_run[k] = P.max_run[k];
    if (failed_solves) failed_solves[k] = P.failed[k];
  }
  if (chi2_margin) *chi2_margin = P.margin;
  if (pose64) {
    double R[9];
    spfe_quat_to_rot(T.q, R);
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) pose64[r * 4 + c] = R[r * 3 + c];
      pose64[r * 4 + 3] = T.t[r];
    }
    pose64[12] = pose64[13] = pose64[14] = 0.0;
    pose64[15] = 1.0;
  }
  return n - nBad;
}

/* The header's analytic Jacobian of one edge at Tcw and central differences of its error under spfe_se3_oplus(+-h e_k):
 * A[12], N[12] (row u then row v). */
API void pose_ref_jacobian_check(const float *Tcw, const float *Xw, float fx, float fy, float cx, float cy, double h,
                                 double *A, double *N) {
  spfe_se3 T;
  spfe_se3_from_f32(Tcw, &T);
  const double X[3] = {Xw[0], Xw[1], Xw[2]};
  double p[3], e[2];
  spfe_pose_error(&T, X, fx, fy, cx, cy, 0.0, 0.0, p, e);
  spfe_pose_jacobian(p, fx, fy, A, A + 6);
  for (int k = 0; k < 6; ++k) {
    double d[6] = {0, 0, 0, 0, 0, 0}, ep[2], em[2], pp[3];
    spfe_se3 Tp = T, Tm = T;
    d[k] = h;
    spfe_se3_oplus(&Tp, d);
    d[k] = -h;
    spfe_se3_oplus(&Tm, d);
    spfe_pose_error(&Tp, X, fx, fy, cx, cy, 0.0, 0.0, pp, ep);
    spfe_pose_error(&Tm, X, fx, fy, cx, cy, 0.0, 0.0, pp, em);
    N[k] = (ep[0] - em[0]) / (2 * h);
    N[6 + k] = (ep[1] - em[1]) / (2 * h);
  }
}
