/*
 * sim3opt_ref.c — host reference of the Sim3 optimisation of a loop hypothesis (sp_orb_slam_amd/csrc/sim3opt.hip), built from
 * include/spfe_sim3opt_math.h with the oracle's flags (gcc -O3 -mavx2 -mfma -ffp-contract=off -fno-fast-math) by the test
 * modules and loaded through ctypes.  It states Optimizer::OptimizeSim3 (orb_slam2/src/mapping/optimizer.cpp:1062-1252) edge
 * by edge and g2o call by call; the kernel must agree with it in every integer, verdict and iteration count, and in the
 * transform up to the device's sin / cos / exp in the applied updates.
 *
 * Sums: the 256-slot tree of spfe_dust_math.h; term 2 c (e12) and 2 c + 1 (e21) of served correspondence c feed slot
 * (term % 256), removed correspondences feed nothing.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spfe.h"
#include "../../include/spfe_sim3_math.h"
#include "../../include/spfe_sim3opt_math.h"

#define API __attribute__((visibility("default")))

typedef struct {
  int n;            /* served correspondences */
  const float *dat; /* [n][10]: P1c | P2c | obs1 | obs2 */
  double fx[2], fy[2], cx[2], cy[2];
  int fix_scale;
  uint8_t *alive;
  double *chi;      /* [2 n]: the chi2 each edge holds */
  /* what the coverage claims of the tests rest on */
  int call, trials[2], max_run[2], failed[2], branches[4];
  double margin;
} problem;

/* term i = 2 c + kind: e12 maps P2c with S12 (kind 0), e21 maps P1c with S12^-1 (kind 1) */
static void term_error(const problem *P, const spfe_s3o_sim *fwd, const spfe_s3o_sim *inv, int i, double e[2]) {
  const int c = i >> 1, kind = i & 1;
  const float *d = P->dat + 10 * c;
  const double X[3] = {(double)d[kind ? 0 : 3], (double)d[kind ? 1 : 4], (double)d[kind ? 2 : 5]};
  spfe_s3o_error(kind ? inv : fwd, X, P->fx[kind], P->fy[kind], P->cx[kind], P->cy[kind], (double)d[kind ? 8 : 6],
                 (double)d[kind ? 9 : 7], e);
}

/* computeActiveErrors + activeRobustChi2 */
static double active_chi2(problem *P, const spfe_s3o_sim *S) {
  spfe_s3o_sim inv;
  spfe_s3o_inv(S, &inv);
  double s[SPFE_DUST_SLOTS];
  memset(s, 0, sizeof(s));
  for (int i = 0; i < 2 * P->n; ++i) {
    if (!P->alive[i >> 1]) continue;
    double e[2];
    term_error(P, S, &inv, i, e);
    P->chi[i] = spfe_s3o_chi2(e);
    s[i % SPFE_DUST_SLOTS] += spfe_s3o_rho0(P->chi[i]);
  }
  return spfe_dust_tree_total(s);
}

static void term_jacobian(const problem *P, const spfe_s3o_sim *F, const spfe_s3o_sim *I, int i, double J0[7], double J1[7]) {
  for (int d = 0; d < 7; ++d) {
    double ep[2], em[2];
    term_error(P, &F[2 * d], &I[2 * d], i, ep);
    term_error(P, &F[2 * d + 1], &I[2 * d + 1], i, em);
    spfe_s3o_jcol(ep, em, &J0[d], &J1[d]);
  }
}

/* buildSystem at S */
static void build(const problem *P, const spfe_s3o_sim *S, double H[49], double b[7]) {
  static double s[SPFE_S3O_NSUM][SPFE_DUST_SLOTS];
  memset(s, 0, sizeof(s));
  spfe_s3o_sim inv, F[14], I[14];
  spfe_s3o_inv(S, &inv);
  for (int p = 0; p < 14; ++p) spfe_s3o_perturb(S, p, P->fix_scale, &F[p], &I[p]);
  for (int i = 0; i < 2 * P->n; ++i) {
    if (!P->alive[i >> 1]) continue;
    double e[2], J0[7], J1[7], q[SPFE_S3O_NSUM];
    term_error(P, S, &inv, i, e);
    term_jacobian(P, F, I, i, J0, J1);
    spfe_s3o_terms(e, J0, J1, q);
    for (int k = 0; k < SPFE_S3O_NSUM; ++k) s[k][i % SPFE_DUST_SLOTS] += q[k];
  }
  double tot[SPFE_S3O_NSUM];
  for (int k = 0; k < SPFE_S3O_NSUM; ++k) tot[k] = spfe_dust_tree_total(s[k]);
  spfe_s3o_unpack(tot, H, b);
}

/* initializeOptimization(); optimize(iterations): the iterations run, 0 when no edge is active */
static int optimize(problem *P, spfe_s3o_sim *S, int iterations) {
  int active = 0;
  for (int c = 0; c < P->n; ++c) active += P->alive[c];
  if (!active) return 0;
  spfe_lm lm = {0.0, 2.0};
  int done = 0;
  for (int it = 0; it < iterations; ++it) {
    const double currentChi = active_chi2(P, S);
    double H[49], b[7];
    build(P, S, H, b);
    if (it == 0) {
      double maxDiagonal = 0;
      for (int j = 0; j < 7; ++j) maxDiagonal = fabs(H[j * 7 + j]) > maxDiagonal ? fabs(H[j * 7 + j]) : maxDiagonal;
      lm.lambda = SPFE_LM_TAU * maxDiagonal;
      lm.ni = 2;
    }
    double rho = 0, cur = currentChi;
    int qmax = 0, run = 0;
    do {
      double x[7];
      spfe_s3o_sim St = *S;
      const int ok2 = spfe_solve7(H, lm.lambda, b, x);
      P->failed[P->call] += !ok2;
      if (ok2) P->branches[spfe_s3o_oplus(&St, x, P->fix_scale)]++;
      double tempChi = active_chi2(P, &St);   /* the edges keep these errors, accepted or not */
      if (!ok2) tempChi = 1.7976931348623157e308;
      if (spfe_s3o_lm_judge(&lm, cur, tempChi, x, b, &rho)) { *S = St; cur = tempChi; run = 0; }
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

static int is_bad(problem *P, int c, float th2) {
  for (int k = 0; k < 2; ++k) {
    const double m = fabs(P->chi[2 * c + k] - (double)th2) / (double)th2;
    if (!(m >= P->margin)) P->margin = m;   /* a NaN chi2 reads as margin NaN */
  }
  return P->chi[2 * c] > th2 || P->chi[2 * c + 1] > th2;
}

/* One solve on host arrays (the arguments of spfe_optimize_sim3).  kcap = max(K1, K2, 1) entries of matches12_out, matched and
 * verdict are written.  counts[9]: n_corr, n_bad, n_in, accepted, iterations[2], trials[2], status (0).  Optional stats:
 * max_rejected_run[2], failed_solves[2], branches[4] (how many applied updates took each branch of Sim3(update)),
 * chi2_margin[1] (min over the classified chi2 of both rounds of |chi2 - th2| / th2; infinity when nothing was classified).
 * Returns n_in. */
API int sim3opt_ref_solve(const float *kp_xy1, int K1, const int32_t *mp1, const float *kp_xy2, int K2, const int32_t *mp2,
                          const float *xyz, const uint8_t *flags, int n, const float *Tcw1, const float *Tcw2, const float *T12,
                          const int32_t *matches12, const spfe_sim3opt_params *prm, int32_t *counts, double *S12, float *T12_out,
                          float *Scw, int32_t *matches12_out, int32_t *matched, uint8_t *verdict, int *max_rejected_run,
                          int *failed_solves, int *branches, double *chi2_margin) {
  const int kcap = (K1 > K2 ? K1 : K2) > 1 ? (K1 > K2 ? K1 : K2) : 1;
  float *dat = (float *)malloc(sizeof(float) * 10 * (size_t)(K1 + 1));
  int *k1_of = (int *)malloc(sizeof(int) * (size_t)(K1 + 1));
  uint8_t *alive = (uint8_t *)malloc((size_t)K1 + 1);
  double *chi = (double *)calloc(2 * (size_t)K1 + 2, sizeof(double));
  int nc = 0;
  for (int k1 = 0; k1 < kcap; ++k1) {
    const int k2 = k1 < K1 ? matches12[k1] : -1;
    matches12_out[k1] = k2;
    verdict[k1] = SPFE_SIM3OPT_NONE;
    if (k2 < 0) continue;
    verdict[k1] = SPFE_SIM3OPT_SKIPPED;
    if (k2 >= K2) continue;
    const int p1 = mp1[k1], p2 = mp2[k2];
    if (p1 < 0 || p1 >= n || p2 < 0 || p2 >= n) continue;
    if (!(flags[p1] & SPFE_PROJ_SEARCHABLE) || !(flags[p2] & SPFE_PROJ_SEARCHABLE)) continue;
    float *d = dat + 10 * nc;
    spfe_sim3_to_cam(Tcw1, xyz + 3 * p1, d);
    spfe_sim3_to_cam(Tcw2, xyz + 3 * p2, d + 3);
    d[6] = kp_xy1[2 * k1]; d[7] = kp_xy1[2 * k1 + 1];
    d[8] = kp_xy2[2 * k2]; d[9] = kp_xy2[2 * k2 + 1];
    alive[nc] = 1;
    k1_of[nc++] = k1;
  }
  problem P = {nc, dat, {prm->fx1, prm->fx2}, {prm->fy1, prm->fy2}, {prm->cx1, prm->cx2}, {prm->cy1, prm->cy2},
               prm->fix_scale, alive, chi, 0, {0, 0}, {0, 0}, {0, 0}, {0, 0, 0, 0}, INFINITY};
  spfe_s3o_sim S;
  spfe_s3o_from_f32(T12, &S);
  int iters[2] = {0, 0};
  iters[0] = optimize(&P, &S, prm->iterations);
  int nBad = 0;
  for (int c = 0; c < nc; ++c) {
    const int bad = is_bad(&P, c, prm->th2);
    if (bad) { alive[c] = 0; matches12_out[k1_of[c]] = -1; nBad++; }
    verdict[k1_of[c]] = bad ? SPFE_SIM3OPT_REMOVED : SPFE_SIM3OPT_KEPT;
  }
  const int stop = nc - nBad < prm->min_kept;
  int nIn = 0;
  if (!stop) {
    P.call = 1;
    iters[1] = optimize(&P, &S, nBad > 0 ? 2 * prm->iterations : prm->iterations);
    for (int c = 0; c < nc; ++c) {
      if (!alive[c]) continue;
      const int bad = is_bad(&P, c, prm->th2);
      if (bad) matches12_out[k1_of[c]] = -1;
      else nIn++;
      verdict[k1_of[c]] = bad ? SPFE_SIM3OPT_OUTLIER : SPFE_SIM3OPT_INLIER;
    }
    spfe_s3o_store(&S, S12, T12_out);
  } else {
    spfe_s3o_store_echo(T12, S12, T12_out);
  }
  spfe_s3o_scw(S12, Tcw2, Scw);
  for (int k1 = 0; k1 < kcap; ++k1) {
    const int k2 = matches12_out[k1];
    matched[k1] = (k2 >= 0 && k2 < K2) ? mp2[k2] : -1;
  }
  counts[0] = nc; counts[1] = nBad; counts[2] = nIn; counts[3] = (!stop && nIn >= prm->min_inliers) ? 1 : 0;
  counts[4] = iters[0]; counts[5] = iters[1]; counts[6] = P.trials[0]; counts[7] = P.trials[1]; counts[8] = 0;
  for (int k = 0; k < 2; ++k) {
    if (max_rejected_run) max_rejected_run[k] = P.max_run[k];
    if (failed_solves) failed_solves[k] = P.failed[k];
  }
  if (branches)
    for (int k = 0; k < 4; ++k) branches[k] = P.branches[k];
  if (chi2_margin) *chi2_margin = P.margin;
  free(dat); free(k1_of); free(alive); free(chi);
  return nIn;
}

API void sim3opt_ref_scw(const double *S12, const float *Tcw2, float *Scw) { spfe_s3o_scw(S12, Tcw2, Scw); }

/* The header's numeric Jacobian of one edge at the start value T12: kind 0 = e12 of the point P (P2c), kind 1 = e21 (P1c);
 * e[2], J[14] (row u then row v). */
API void sim3opt_ref_jacobian(const float *T12, const double *P, int kind, double fx, double fy, double cx, double cy, double ox,
                              double oy, int fix_scale, double *e, double *J) {
  spfe_s3o_sim S, inv, F, I;
  spfe_s3o_from_f32(T12, &S);
  spfe_s3o_inv(&S, &inv);
  spfe_s3o_error(kind ? &inv : &S, P, fx, fy, cx, cy, ox, oy, e);
  for (int d = 0; d < 7; ++d) {
    double ep[2], em[2];
    spfe_s3o_perturb(&S, 2 * d, fix_scale, &F, &I);
    spfe_s3o_error(kind ? &I : &F, P, fx, fy, cx, cy, ox, oy, ep);
    spfe_s3o_perturb(&S, 2 * d + 1, fix_scale, &F, &I);
    spfe_s3o_error(kind ? &I : &F, P, fx, fy, cx, cy, ox, oy, em);
    spfe_s3o_jcol(ep, em, &J[d], &J[7 + d]);
  }
}

/* Sim3(update) of the header as a 4x4 (s R | t) and its branch, for the comparison with the matrix exponential */
API int sim3opt_ref_exp(const double *u, double *M) {
  spfe_s3o_sim E;
  const int br = spfe_s3o_exp(u, &E);
  double R[9];
  spfe_quat_to_rot(E.q, R);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) M[4 * r + c] = E.s * R[3 * r + c];
    M[4 * r + 3] = E.t[r];
  }
  M[12] = M[13] = M[14] = 0.0;
  M[15] = 1.0;
  return br;
}
