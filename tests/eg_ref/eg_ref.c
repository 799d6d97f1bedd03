/* eg_ref.c — the host C reference of the essential graph over Sim3 and of the map corrections: the arithmetic of
 * include/spfe_essgraph_math.h run serially, with a LEFT-looking scalar skyline Cholesky (the kernel's is right-looking over
 * block columns: the contract's order of subtraction makes the two bit-equal).  Compiled by eg_ref.py with -ffp-contract=off.
 * The test suite's mutations are single changes of the contract switched on by -DSPFE_EG_MUT_*. */
#include <stdlib.h>
#include <string.h>

#include "spfe.h"
#include "spfe_essgraph_math.h"

#define API __attribute__((visibility("default")))

typedef struct {
  int n, E, U, N;
  const int *edges;
  int *ok, *unk, *vert, *first, *adjs, *adj, *last; /* last[i]: the last scalar row whose envelope holds column i */
  long long *rs; /* rs[i]: where scalar row i starts; it holds columns 7 first(i / 7) .. i */
  spfe_s3o_sim *Sji, *est, *bak;
  double *err, *Ji, *Jj, *H, *L, *b, *x;
  int fix_scale;
} eg;

static int fs(const eg *g, int i) { return 7 * g->first[i / 7]; }
static double *at(const eg *g, double *M, int i, int j) { return M + g->rs[i] + (j - fs(g, i)); }

static double errors_and_chi(eg *g) {
  double s[SPFE_DUST_SLOTS];
  for (int t = 0; t < SPFE_DUST_SLOTS; ++t) s[t] = 0.0;
  for (int e = 0; e < g->E; ++e) {
    if (!g->ok[e]) continue;
    spfe_s3o_sim inv;
    spfe_s3o_inv(&g->est[g->edges[3 * e + 1]], &inv);
    spfe_eg_error(&g->Sji[e], &g->est[g->edges[3 * e]], &inv, g->err + 7 * (size_t)e);
    s[e % SPFE_DUST_SLOTS] += spfe_eg_chi2(g->err + 7 * (size_t)e);
  }
  return spfe_dust_tree_total(s);
}

/* the numeric Jacobians of one edge: pfi / pfj = the 14 perturbed estimates and their 14 inverses of vertex i / j (NULL: that
 * vertex is fixed), e0 = the error at the estimate (the one-sided mutation reads it) */
static void edge_jacobian(const spfe_s3o_sim *Sji, const spfe_s3o_sim *Si, const spfe_s3o_sim *Sj, const spfe_s3o_sim *pfi,
                          const spfe_s3o_sim *pfj, const double *e0, double *Ji, double *Jj) {
  spfe_s3o_sim inv;
  spfe_s3o_inv(Sj, &inv);
  double ep[7], em[7];
  (void)e0;
  if (pfi)
    for (int d = 0; d < 7; ++d) {
      spfe_eg_error(Sji, &pfi[2 * d], &inv, ep);
      spfe_eg_error(Sji, &pfi[2 * d + 1], &inv, em);
#ifdef SPFE_EG_MUT_ONESIDED
      for (int k = 0; k < 7; ++k) em[k] = ep[k] - 2.0 * (ep[k] - e0[k]); /* mutation: (e(+) - e) / delta */
#endif
      spfe_eg_jcol(ep, em, Ji, d);
    }
  if (pfj)
    for (int d = 0; d < 7; ++d) {
      spfe_eg_error(Sji, Si, &pfj[14 + 2 * d], ep);
      spfe_eg_error(Sji, Si, &pfj[14 + 2 * d + 1], em);
#ifdef SPFE_EG_MUT_ONESIDED
      for (int k = 0; k < 7; ++k) em[k] = ep[k] - 2.0 * (ep[k] - e0[k]);
#endif
      spfe_eg_jcol(ep, em, Jj, d);
    }
}

static void jacobians(eg *g) {
  spfe_s3o_sim *pf = (spfe_s3o_sim *)malloc(sizeof(spfe_s3o_sim) * 28 * (size_t)g->n);
  for (int u = 0; u < g->U; ++u) {
    const int v = g->vert[u];
    for (int p = 0; p < 14; ++p) spfe_s3o_perturb(&g->est[v], p, g->fix_scale, &pf[28 * (size_t)v + p], &pf[28 * (size_t)v + 14 + p]);
  }
  for (int e = 0; e < g->E; ++e) {
    if (!g->ok[e]) continue;
    const int vi = g->edges[3 * e], vj = g->edges[3 * e + 1];
    edge_jacobian(&g->Sji[e], &g->est[vi], &g->est[vj], g->unk[vi] >= 0 ? &pf[28 * (size_t)vi] : NULL,
                  g->unk[vj] >= 0 ? &pf[28 * (size_t)vj] : NULL, g->err + 7 * (size_t)e, g->Ji + 49 * (size_t)e, g->Jj + 49 * (size_t)e);
  }
  free(pf);
}

/* (a) (b); returns the largest |diagonal| (the tau mutation reads it) */
static double assemble(eg *g) {
  memset(g->H, 0, sizeof(double) * (size_t)g->rs[g->N]);
  double md = 0.0;
  for (int u = 0; u < g->U; ++u)
    for (int r = 0; r < 7; ++r) {
      const int i = 7 * u + r;
      double bb = 0.0;
      for (int k = g->adjs[u]; k < g->adjs[u + 1]; ++k) {
        const int e = g->adj[k] >> 1, side = g->adj[k] & 1;
        const double *Ju = (side ? g->Jj : g->Ji) + 49 * (size_t)e;
        for (int c = 0; c <= r; ++c) *at(g, g->H, i, 7 * u + c) += spfe_eg_dot7(Ju + r, 7, Ju + c, 7);
        bb -= spfe_eg_dot7(Ju + r, 7, g->err + 7 * (size_t)e, 1);
        const int w = g->unk[g->edges[3 * e + (side ? 0 : 1)]];
        if (w >= 0 && w < u && w >= g->first[u]) {
          const double *Jw = (side ? g->Ji : g->Jj) + 49 * (size_t)e;
          for (int c = 0; c < 7; ++c) *at(g, g->H, i, 7 * w + c) += spfe_eg_dot7(Ju + r, 7, Jw + c, 7);
        }
      }
      g->b[i] = bb;
      const double dd = fabs(*at(g, g->H, i, i));
      if (dd > md) md = dd;
    }
  return md;
}

/* (e): 1 solved, 0 failed */
static int solve(eg *g, double lambda) {
  const int N = g->N;
  for (int i = 0; i < N; ++i) {
    const int fi = fs(g, i);
    for (int j = fi; j <= i; ++j) {
      double s = *at(g, g->H, i, j);
      if (i == j) s += lambda;
      const int fj = fs(g, j);
      for (int k = fi > fj ? fi : fj; k < j; ++k) s -= *at(g, g->L, i, k) * *at(g, g->L, j, k);
      if (j < i) {
        *at(g, g->L, i, j) = s / *at(g, g->L, j, j);
      } else {
        if (!spfe_eg_pivot_ok(s)) return 0;
        *at(g, g->L, i, i) = sqrt(s);
      }
    }
  }
  for (int i = 0; i < N; ++i) {
    double s = g->b[i];
    for (int k = fs(g, i); k < i; ++k) s -= *at(g, g->L, i, k) * g->x[k];
    g->x[i] = s / *at(g, g->L, i, i);
  }
  for (int i = N - 1; i >= 0; --i) {
    double s = g->x[i];
    for (int k = g->last[i]; k > i; --k)
      if (fs(g, k) <= i) s -= *at(g, g->L, k, i) * g->x[k];
    g->x[i] = s / *at(g, g->L, i, i);
  }
  return 1;
}

static void write_poses(const eg *g, unsigned char *out) {
  for (int v = 0; v < g->n; ++v) {
    spfe_eg_store_canon(&g->est[v], (double *)(out + SPFE_ESSGRAPH_OFF_SIM3) + 8 * (size_t)v);
    spfe_eg_recover(&g->est[v], (float *)(out + SPFE_ESSGRAPH_OFF_TIW(g->n)) + 16 * (size_t)v);
  }
}

/* diag (doubles, may be NULL): [0] failed solves, [1] rejected trials, [2] accepted trials, [3] least |rho| of a solved trial */
API int eg_ref_solve(const double *est_in, const double *meas, const unsigned char *flags_in, int n, const int *edges, int E,
                     int env_cap, int iterations, int fix_scale, double lambda_init, unsigned char *out, double *diag) {
  eg G, *g = &G;
  memset(g, 0, sizeof(G));
  g->n = n; g->E = E; g->edges = edges; g->fix_scale = fix_scale;
  const size_t ne = (size_t)(E > 0 ? E : 1), nv = (size_t)n + 1;
  unsigned char *flags = (unsigned char *)malloc(nv);
  for (int v = 0; v < n; ++v) flags[v] = flags_in[v];
#ifdef SPFE_EG_MUT_FIXED_BLOCK
  for (int v = 0; v < n; ++v) flags[v] = 0; /* mutation: the fixed vertex's block is added */
#endif
  g->ok = (int *)calloc(ne, 4); g->unk = (int *)calloc(nv, 4); g->vert = (int *)calloc(nv, 4); g->first = (int *)calloc(nv, 4);
  g->adjs = (int *)calloc(nv + 1, 4); g->adj = (int *)calloc(2 * ne, 4);
  g->Sji = (spfe_s3o_sim *)calloc(ne, sizeof(spfe_s3o_sim));
  g->est = (spfe_s3o_sim *)calloc(nv, sizeof(spfe_s3o_sim)); g->bak = (spfe_s3o_sim *)calloc(nv, sizeof(spfe_s3o_sim));
  g->err = (double *)calloc(ne * 7, 8); g->Ji = (double *)calloc(ne * 49, 8); g->Jj = (double *)calloc(ne * 49, 8);
  int *work = (int *)calloc(nv, 4);
  for (int v = 0; v < n; ++v) spfe_eg_load(est_in + 8 * (size_t)v, &g->est[v]);
  int followed = 0;
  for (int e = 0; e < E; ++e) {
    const int i = edges[3 * e], j = edges[3 * e + 1], kind = edges[3 * e + 2];
    g->ok[e] = spfe_eg_edge_ok(i, j, kind, n);
    if (!g->ok[e]) continue;
    ++followed;
#ifdef SPFE_EG_MUT_KIND
    const double *src = est_in; /* mutation: the kind is ignored */
#else
    const double *src = kind == 0 ? est_in : meas;
#endif
    spfe_s3o_sim Si, Sj;
    spfe_eg_load(src + 8 * (size_t)i, &Si);
    spfe_eg_load(src + 8 * (size_t)j, &Sj);
    spfe_eg_measure(&Si, &Sj, &g->Sji[e]);
  }
  const long long blocks = spfe_eg_envelope(n, flags, edges, E, g->unk, g->first, &g->U, work);
  const int U = g->U;
  g->N = 7 * U;
  for (int v = 0; v < n; ++v)
    if (g->unk[v] >= 0) g->vert[g->unk[v]] = v;
  int *hdr = (int *)out;
  double *dout = (double *)(out + SPFE_ESSGRAPH_OFF_CHI2_INITIAL);
  const int status = U == 0 ? SPFE_ESSGRAPH_EMPTY : blocks > env_cap ? SPFE_ESSGRAPH_ENVELOPE_OVERFLOW : SPFE_ESSGRAPH_OK;
  hdr[0] = status; hdr[1] = U; hdr[2] = followed; hdr[3] = E - followed; hdr[4] = (int)blocks;
  int it_done = 0, n_trials = 0, n_failed = 0, n_rej = 0, n_acc = 0;
  double chi_initial = 0.0, currentChi = 0.0, min_rho = 1e300;
  spfe_lm lm = {lambda_init, 2.0};
  if (status == SPFE_ESSGRAPH_OK && iterations > 0) {
#ifdef SPFE_EG_MUT_ENV_OFF
    for (int u = 0; u < U; ++u) /* mutation: the envelope starts one block late */
      if (g->first[u] < u) g->first[u]++;
#endif
    /* adjacency in ascending edge index */
    for (int e = 0; e < E; ++e) {
      if (!g->ok[e]) continue;
      for (int side = 0; side < 2; ++side) {
        const int u = g->unk[edges[3 * e + side]];
        if (u >= 0) g->adjs[u + 1]++;
      }
    }
    for (int u = 0; u < U; ++u) g->adjs[u + 1] += g->adjs[u];
    for (int u = 0; u < U; ++u) work[u] = g->adjs[u];
    for (int e = 0; e < E; ++e) {
      if (!g->ok[e]) continue;
      for (int side = 0; side < 2; ++side) {
        const int u = g->unk[edges[3 * e + side]];
        if (u >= 0) g->adj[work[u]++] = 2 * e + side;
      }
    }
    g->rs = (long long *)calloc((size_t)g->N + 1, 8);
    for (int i = 0; i < g->N; ++i) g->rs[i + 1] = g->rs[i] + (i - fs(g, i) + 1);
    g->last = (int *)calloc((size_t)g->N + 1, 4);
    for (int k = 0; k < g->N; ++k) g->last[fs(g, k)] = k; /* ascending k: the largest stays */
    for (int i = 1; i < g->N; ++i)
      if (g->last[i - 1] > g->last[i]) g->last[i] = g->last[i - 1];
    g->H = (double *)calloc((size_t)g->rs[g->N] + 1, 8); g->L = (double *)calloc((size_t)g->rs[g->N] + 1, 8);
    g->b = (double *)calloc((size_t)g->N + 1, 8); g->x = (double *)calloc((size_t)g->N + 1, 8);
    int fresh = 0, go = 1;
    for (int it = 0; it < iterations && go; ++it) {
      if (!fresh) currentChi = errors_and_chi(g);
      if (it == 0) chi_initial = currentChi;
      jacobians(g);
      const double md = assemble(g);
      (void)md;
#ifdef SPFE_EG_MUT_TAU
      if (it == 0) lm.lambda = SPFE_LM_TAU * md; /* mutation: lambda started at tau * max diagonal */
#endif
      double rho = 0;
      int qmax = 0;
      do {
        const double lambda = lm.lambda;
        const int ok = solve(g, lambda);
        double sum = 0.0, tempChi = SPFE_EG_DBL_MAX;
        if (ok) {
          double s[SPFE_DUST_SLOTS];
          for (int t = 0; t < SPFE_DUST_SLOTS; ++t) s[t] = 0.0;
          for (int j = 0; j < g->N; ++j) s[j % SPFE_DUST_SLOTS] += spfe_eg_scale_term(g->x[j], lambda, g->b[j]);
          sum = spfe_dust_tree_total(s);
          for (int u = 0; u < U; ++u) {
            const int v = g->vert[u];
            g->bak[v] = g->est[v];
            spfe_eg_oplus(&g->est[v], g->x + 7 * (size_t)u, fix_scale);
          }
          tempChi = errors_and_chi(g);
        } else {
          ++n_failed;
        }
        fresh = spfe_eg_lm_judge(&lm, currentChi, tempChi, sum, &rho);
        if (ok && fabs(rho) < min_rho) min_rho = fabs(rho);
        if (fresh) {
          currentChi = tempChi;
          ++n_acc;
        } else {
          ++n_rej;
          if (ok)
            for (int u = 0; u < U; ++u) g->est[g->vert[u]] = g->bak[g->vert[u]];
        }
        ++qmax;
        ++n_trials;
      } while (rho < 0 && qmax < SPFE_LM_MAX_TRIALS);
      ++it_done;
      if (qmax == SPFE_LM_MAX_TRIALS || rho == 0) go = 0;
    }
    hdr[5] = it_done; hdr[6] = n_trials; hdr[7] = n_failed;
    dout[0] = spfe_s3o_canon(chi_initial); dout[1] = spfe_s3o_canon(currentChi); dout[2] = spfe_s3o_canon(lm.lambda);
  } else {
    hdr[5] = 0; hdr[6] = 0; hdr[7] = 0;
    dout[0] = 0.0; dout[1] = 0.0; dout[2] = lambda_init;
  }
  write_poses(g, out);
  if (diag) { diag[0] = n_failed; diag[1] = n_rej; diag[2] = n_acc; diag[3] = min_rho; }
  free(flags); free(g->ok); free(g->unk); free(g->vert); free(g->first); free(g->adjs); free(g->adj); free(g->Sji); free(g->est);
  free(g->bak); free(g->err); free(g->Ji); free(g->Jj); free(work); free(g->rs); free(g->H); free(g->L); free(g->b); free(g->x); free(g->last);
  return status;
}

API int eg_ref_log(const double S[8], double e[7]) {
  spfe_s3o_sim P;
  spfe_eg_load(S, &P);
  return spfe_eg_log(&P, e);
}
API int eg_ref_exp(const double u[7], double S[8]) {
  spfe_s3o_sim P;
  const int br = spfe_s3o_exp(u, &P);
  spfe_eg_store(&P, S);
  return br;
}
API int eg_ref_exp_update(const double u[7], double S[8]) {
  spfe_s3o_sim P;
  const int br = spfe_eg_exp_update(u, &P);
  spfe_eg_store(&P, S);
  return br;
}
/* the header's elementary functions: out = ln(x), acos(x), sin(x), cos(x) (spfe_eg_sincos_any), exp(x) */
API void eg_ref_elementary(double x, double out[5]) {
  out[0] = spfe_eg_ln(x);
  out[1] = spfe_eg_acos(x);
  spfe_eg_sincos_any(x, &out[2], &out[3]);
  out[4] = spfe_eg_exp(x);
}
API void eg_ref_perturb(const double S[8], int p, int fix_scale, double fwd[8], double inv[8]) {
  spfe_s3o_sim P, F, I;
  spfe_eg_load(S, &P);
  spfe_s3o_perturb(&P, p, fix_scale, &F, &I);
  spfe_eg_store(&F, fwd);
  spfe_eg_store(&I, inv);
}
/* the two 7x7 Jacobians of one edge (row-major [error row][column]) as the solver forms them */
API void eg_ref_jacobian(const double Sji[8], const double Si[8], const double Sj[8], int fix_scale, double Ji[49], double Jj[49]) {
  spfe_s3o_sim A, B, C, inv, pfi[28], pfj[28];
  double e0[7];
  spfe_eg_load(Sji, &A); spfe_eg_load(Si, &B); spfe_eg_load(Sj, &C);
  for (int p = 0; p < 14; ++p) {
    spfe_s3o_perturb(&B, p, fix_scale, &pfi[p], &pfi[14 + p]);
    spfe_s3o_perturb(&C, p, fix_scale, &pfj[p], &pfj[14 + p]);
  }
  spfe_s3o_inv(&C, &inv);
  spfe_eg_error(&A, &B, &inv, e0);
  edge_jacobian(&A, &B, &C, pfi, pfj, e0, Ji, Jj);
}
API void eg_ref_error(const double Sji[8], const double Si[8], const double Sj[8], double e[7]) {
  spfe_s3o_sim A, B, C, inv;
  spfe_eg_load(Sji, &A); spfe_eg_load(Si, &B); spfe_eg_load(Sj, &C);
  spfe_s3o_inv(&C, &inv);
  spfe_eg_error(&A, &B, &inv, e);
}
API int eg_ref_envelope(int n, const unsigned char *flags, const int *edges, int E, int *first_out, int *n_unknown) {
  int *work = (int *)calloc((size_t)n + 1, 4);
  const long long b = spfe_eg_envelope(n, flags, edges, E, NULL, first_out, n_unknown, work);
  free(work);
  return (int)b;
}
API void eg_ref_sim3(const float *Tcw, const double *S12, const float *Tcw2, const float *Twc, const int *conn_slot, int n_conn,
                     int cur_slot, double *est, double *meas, int n) {
  for (int v = 0; v < n; ++v) {
    spfe_s3o_sim S;
    spfe_eg_from_pose(Tcw + 16 * (size_t)v, &S);
    spfe_eg_store_canon(&S, est + 8 * (size_t)v);
    spfe_eg_store_canon(&S, meas + 8 * (size_t)v);
  }
  for (int k = 0; k < n_conn; ++k) {
    const int v = conn_slot[k];
    if (v < 0 || v >= n) continue;
    spfe_s3o_sim P;
    spfe_eg_corrected(S12, Tcw2, Twc, Tcw + 16 * (size_t)v, v == cur_slot, &P);
    spfe_eg_store_canon(&P, est + 8 * (size_t)v);
  }
}
API void eg_ref_correct(const double *S_from, const double *S_to, int n_kf, const int *ref_slot, const int *point_idx, int m, float *xyz,
                        const unsigned char *flags, int n_table, unsigned char *code) {
  for (int i = 0; i < m; ++i) {
    const int row = point_idx ? point_idx[i] : i;
    if (row < 0 || row >= n_table) { code[i] = SPFE_EGC_INVALID; continue; }
    if (!(flags[row] & SPFE_PROJ_SEARCHABLE)) { code[i] = SPFE_EGC_SKIP_BAD; continue; }
    const int r = ref_slot[i];
    if (r < 0 || r >= n_kf) { code[i] = SPFE_EGC_INVALID; continue; }
    spfe_s3o_sim A, B;
    spfe_eg_load(S_from + 8 * (size_t)r, &A);
    spfe_eg_load(S_to + 8 * (size_t)r, &B);
    float Y[3];
    spfe_eg_correct_point(&A, &B, xyz + 3 * (size_t)row, Y);
    xyz[3 * (size_t)row] = Y[0]; xyz[3 * (size_t)row + 1] = Y[1]; xyz[3 * (size_t)row + 2] = Y[2];
    code[i] = SPFE_EGC_CORRECTED;
  }
}
