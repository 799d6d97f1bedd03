// essgraph.hip — the loop closer's pose graph over Sim3 (Optimizer::OptimizeEssentialGraph, optimizer.cpp:776-1060), the start
// values of its vertices, the SE3 recovery and the map-point correction of CorrectLoop (loop_closer_vlad.cpp:575-606,
// optimizer.cpp:1029-1059).  The arithmetic is include/spfe_essgraph_math.h, shared with tests/eg_ref/eg_ref.c.
//
// Launches of one optimisation:
//   eg_prepare_kernel   (multi-workgroup) edge validation, the measurements Sji, the working copy of the estimates, and which
//                       slots have a followed edge
//   eg_solve_kernel     ONE workgroup: the unknowns, first(), the envelope's prefix sums, the adjacency lists (ascending edge
//                       index by ranks inside chunks of edges: no sort), and the whole Levenberg schedule.  __syncthreads() is the only synchronisation: no grid barrier, no spin on memory.
//   eg_recover_kernel   (multi-workgroup) the optimised Sim3 and the f32 SE3 poses into the block
//
// Who computes what in a trial (T = EG_THREADS):
//   errors / chi2       a thread per edge; the 256 slot sums by threads 0 .. 255, the tree by wave butterflies
//   perturbed estimates a thread per (unknown, +-column): 14 estimates and their inverses, once per iteration
//   Jacobians           a thread per edge: 28 perturbed errors (fewer when a vertex is fixed)
//   assembly            BY OWNER, a thread per (unknown, row of its block row): it walks the unknown's adjacency list in
//                       ascending edge index and is the only writer of that row of H_uu, b_u and H_uw (w < u) — no atomics
//   factorisation       right-looking over block columns w: thread 0 factors the 7x7 diagonal block and solves the column's z
//                       (A); a thread per block row below solves its 7x7 block against it, stages it in the LDS panel and
//                       takes its share off b (B); a thread per entry of the trailing blocks (rows of the panel, pairwise)
//                       subtracts the column's 7 products in ascending order (C).  Three barriers a block column; the forward
//                       substitution rides on A and B.  A panel longer than EG_PCAP block rows is read from the envelope.
//   back substitution   per block row u, descending: thread 0 the diagonal block, a thread per (block of the row, scalar)
//   update              a thread per unknown (oplus), the scale's tree as chi2's
// Every entry's running value receives its products in the contract's order whichever thread subtracts them, so the result does
// not depend on the panel path or on the thread count.
#include <hip/hip_runtime.h>

#include "../../include/spfe_essgraph_math.h"
#include "../../include/spfe.h"
#include "spfe_kernels.h"
#include "wave_ops.h"

namespace spfe {

namespace {
constexpr int EG_THREADS = 512;
constexpr int EG_PCAP = 128;   // block rows of a column panel in LDS: 128 * 392 = 50,176 bytes
constexpr int B49 = SPFE_EG_BLOCK;
// LDS map (bytes): panel [EG_PCAP][49] f64 | part [8] f64 | diag [49] f64 | vec [8] f64 | d [8] f64 | scan [EG_THREADS] i32 | i [16] i32
constexpr size_t EG_LDS = ((size_t)EG_PCAP * B49 + 8 + 49 + 8 + 8) * 8 + ((size_t)EG_THREADS + 16) * 4;
static_assert(EG_LDS <= 160 * 1024, "LDS of one workgroup");

struct Scratch {
  double *Sji, *err, *chi, *Ji, *Jj, *est, *bak, *pert, *H, *L, *b, *x;
  int *ok, *mark, *unk, *vert, *first, *rowoff, *deg, *adjs, *adj, *plist;
};
__host__ __device__ inline size_t up128(size_t x) { return (x + 127) & ~(size_t)127; }   // no two arrays share a cache line
// per edge 924 bytes, per keyframe 2,064, per envelope block 2 * 392
__host__ __device__ inline size_t scratch_carve(unsigned char *p, int n, int E, int env_cap, Scratch *s, size_t *mark_off = nullptr) {
  const size_t nv = (size_t)n + 1, ne = (size_t)(E > 0 ? E : 1), nb = (size_t)(env_cap > 0 ? env_cap : 1);
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o = up128(o + bytes); return at; };
  const size_t o_sji = take(ne * 64), o_err = take(ne * 56), o_chi = take(ne * 8), o_ji = take(ne * 392), o_jj = take(ne * 392),
               o_est = take(nv * 64), o_bak = take(nv * 64), o_pert = take(nv * 1792), o_h = take(nb * 392), o_l = take(nb * 392),
               o_b = take(nv * 56), o_x = take(nv * 56), o_ok = take(ne * 4), o_mark = take(nv * 4), o_unk = take(nv * 4),
               o_vert = take(nv * 4), o_first = take(nv * 4), o_row = take(nv * 4), o_deg = take(nv * 4), o_adjs = take(nv * 4),
               o_adj = take(ne * 8), o_pl = take(nv * 4);
  if (mark_off) *mark_off = o_mark;
  if (s) {
    auto d = [&](size_t at) { return reinterpret_cast<double *>(p + at); };
    auto i = [&](size_t at) { return reinterpret_cast<int *>(p + at); };
    s->Sji = d(o_sji); s->err = d(o_err); s->chi = d(o_chi); s->Ji = d(o_ji); s->Jj = d(o_jj);
    s->est = d(o_est); s->bak = d(o_bak); s->pert = d(o_pert); s->H = d(o_h); s->L = d(o_l); s->b = d(o_b); s->x = d(o_x);
    s->ok = i(o_ok); s->mark = i(o_mark); s->unk = i(o_unk); s->vert = i(o_vert); s->first = i(o_first); s->rowoff = i(o_row);
    s->deg = i(o_deg); s->adjs = i(o_adjs); s->adj = i(o_adj); s->plist = i(o_pl);
  }
  return o;
}
// the 256-slot tree: `slot` is the slot sum of threads 0 .. 255 (anything elsewhere); every thread calls, every thread gets it
__device__ __forceinline__ double eg_tree(double slot, double *s_part, int tid) {
  const double w = wave_tree(slot);
  if ((tid & 63) == 0 && tid < SPFE_DUST_SLOTS) s_part[tid >> 6] = w;
  block_fence_sync();
  const double tot = sum4_ordered(s_part, 1);
  block_fence_sync();
  return tot;
}
// exclusive prefix of one int per thread, in thread order; *total: the sum
__device__ __forceinline__ int block_scan(int v, int *s_scan, int tid, int *total) {
  s_scan[tid] = v;
  block_fence_sync();
  if (tid == 0) {
    int run = 0;
    for (int t = 0; t < EG_THREADS; ++t) {
      const int c = s_scan[t];
      s_scan[t] = run;
      run += c;
    }
    s_scan[EG_THREADS] = run;   // the first of the 16 ints behind the scan array
  }
  block_fence_sync();
  const int r = s_scan[tid];
  *total = s_scan[EG_THREADS];
  block_fence_sync();
  return r;
}

// errors and chi2 of every followed edge at the estimates `est`; -> the tree's total
__device__ __forceinline__ double eg_errors(const Scratch &sc, const int *edges, int E, double *s_part, int tid) {
  for (int e = tid; e < E; e += EG_THREADS) {
    if (!sc.ok[e]) continue;
    spfe_s3o_sim Sji, Si, Sj, Sjinv;
    spfe_eg_load(sc.Sji + 8 * (size_t)e, &Sji);
    spfe_eg_load(sc.est + 8 * (size_t)edges[3 * e], &Si);
    spfe_eg_load(sc.est + 8 * (size_t)edges[3 * e + 1], &Sj);
    spfe_s3o_inv(&Sj, &Sjinv);
    double err[SPFE_EG_DIM];
    spfe_eg_error(&Sji, &Si, &Sjinv, err);
    for (int k = 0; k < SPFE_EG_DIM; ++k) sc.err[7 * (size_t)e + k] = err[k];
    sc.chi[e] = spfe_eg_chi2(err);
  }
  block_fence_sync();
  double s = 0.0;
  if (tid < SPFE_DUST_SLOTS)
    for (int e = tid; e < E; e += SPFE_DUST_SLOTS)
      if (sc.ok[e]) s += sc.chi[e];
  return eg_tree(s, s_part, tid);
}
}  // namespace

__global__ __launch_bounds__(256) void eg_prepare_kernel(EgArgs a) {
  Scratch sc;
  scratch_carve(a.scratch, a.n, a.E, a.env_cap, &sc);
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < a.n)
    for (int k = 0; k < 8; ++k) sc.est[8 * (size_t)idx + k] = a.est[8 * (size_t)idx + k];
  if (idx < a.E) {
    const int i = a.edges[3 * idx], j = a.edges[3 * idx + 1], kind = a.edges[3 * idx + 2];
    const int ok = spfe_eg_edge_ok(i, j, kind, a.n);
    sc.ok[idx] = ok;
    if (ok) {
      const double *src = kind == 0 ? a.est : a.meas;
      spfe_s3o_sim Si, Sj, Sji;
      spfe_eg_load(src + 8 * (size_t)i, &Si);
      spfe_eg_load(src + 8 * (size_t)j, &Sj);
      spfe_eg_measure(&Si, &Sj, &Sji);
      spfe_eg_store(&Sji, sc.Sji + 8 * (size_t)idx);
      sc.mark[i] = 1;   // every writer stores the same value
      sc.mark[j] = 1;
    }
  }
}

__global__ __launch_bounds__(EG_THREADS) void eg_solve_kernel(EgArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
  const int tid = threadIdx.x;
  double *s_panel = reinterpret_cast<double *>(smem_b);
  double *s_part = s_panel + (size_t)EG_PCAP * B49;
  double *s_diag = s_part + 8;
  double *s_vec = s_diag + 49;
  double *s_d = s_vec + 8;
  int *s_scan = reinterpret_cast<int *>(s_d + 8);
  int *s_i = s_scan + EG_THREADS;   // [0] is block_scan's total
  enum { I_FOLLOWED = 1, I_FAIL, I_PCNT, I_ACCEPT, I_AGAIN, I_GO };   // s_i[0] is block_scan's total
  enum { D_LAMBDA = 0 };

  const int n = a.n, E = a.E;
  const int *edges = a.edges;
  Scratch sc;
  scratch_carve(a.scratch, n, E, a.env_cap, &sc);
  int *hdr = reinterpret_cast<int *>(a.out);
  double *dout = reinterpret_cast<double *>(a.out + SPFE_ESSGRAPH_OFF_CHI2_INITIAL);

  // ---- the structure: unknowns in slot order
  const int chunk = (n + EG_THREADS - 1) / EG_THREADS;
  const int v_lo = min(n, tid * chunk), v_hi = min(n, v_lo + chunk);
  int cnt = 0, U = 0;
  for (int v = v_lo; v < v_hi; ++v) cnt += sc.mark[v] && !(a.flags[v] & 1);
  int base = block_scan(cnt, s_scan, tid, &U);
  for (int v = v_lo; v < v_hi; ++v) {
    const int is = sc.mark[v] && !(a.flags[v] & 1);
    sc.unk[v] = is ? base : -1;
    if (is) sc.vert[base++] = v;
  }
  for (int u = tid; u < U; u += EG_THREADS) {
    sc.deg[u] = 0;
    sc.first[u] = u;
  }
  if (tid == 0) s_i[I_FOLLOWED] = 0;
  block_fence_sync();
  int mine = 0;
  for (int e = tid; e < E; e += EG_THREADS) {
    if (!sc.ok[e]) continue;
    ++mine;
    const int ui = sc.unk[edges[3 * e]], uj = sc.unk[edges[3 * e + 1]];
    if (ui >= 0) atomicAdd(&sc.deg[ui], 1);
    if (uj >= 0) atomicAdd(&sc.deg[uj], 1);
    if (ui >= 0 && uj >= 0) atomicMin(&sc.first[max(ui, uj)], min(ui, uj));
  }
  if (mine) atomicAdd(&s_i[I_FOLLOWED], mine);
  block_fence_sync();
  const int followed = s_i[I_FOLLOWED];
  const int chunk_u = (U + EG_THREADS - 1) / EG_THREADS;
  const int u_lo = min(U, tid * chunk_u), u_hi = min(U, u_lo + chunk_u);
  int n_adj = 0, blocks = 0;
  cnt = 0;
  for (int u = u_lo; u < u_hi; ++u) cnt += sc.deg[u];
  base = block_scan(cnt, s_scan, tid, &n_adj);
  for (int u = u_lo; u < u_hi; ++u) {
    sc.adjs[u] = base;
    base += sc.deg[u];
  }
  cnt = 0;
  for (int u = u_lo; u < u_hi; ++u) cnt += u - sc.first[u] + 1;
  base = block_scan(cnt, s_scan, tid, &blocks);
  for (int u = u_lo; u < u_hi; ++u) {
    sc.rowoff[u] = base;
    base += u - sc.first[u] + 1;
  }
  const int status = U == 0 ? SPFE_ESSGRAPH_EMPTY : blocks > a.env_cap ? SPFE_ESSGRAPH_ENVELOPE_OVERFLOW : SPFE_ESSGRAPH_OK;
  if (tid == 0) {
    sc.adjs[U] = n_adj;
    sc.rowoff[U] = blocks;
    hdr[0] = status; hdr[1] = U; hdr[2] = followed; hdr[3] = E - followed; hdr[4] = blocks;
    if (status != SPFE_ESSGRAPH_OK || a.iterations == 0) {
      hdr[5] = 0; hdr[6] = 0; hdr[7] = 0;
      dout[0] = 0.0; dout[1] = 0.0; dout[2] = a.lambda_init;
    }
  }
  if (status != SPFE_ESSGRAPH_OK || a.iterations == 0) return;
  block_fence_sync();
  // The adjacency lists in ascending edge index, without a sort and without atomics: the edges go by in chunks of EG_THREADS; an
  // entry's place is its list's cursor plus the number of earlier threads of the chunk that name the same unknown, and the last
  // of them moves the cursor on.  E / EG_THREADS chunks of 2 EG_THREADS LDS compares a thread, whatever the degrees are.
  for (int u = tid; u < U; u += EG_THREADS) sc.deg[u] = 0;   // now the cursor
  int *s_u = reinterpret_cast<int *>(s_panel);               // [2][EG_THREADS]: the panel is not in use yet
  block_fence_sync();
  for (int e0 = 0; e0 < E; e0 += EG_THREADS) {
    const int e = e0 + tid;
    int u2[2] = {-1, -1}, pos[2] = {-1, -1}, last[2] = {0, 0};
    if (e < E && sc.ok[e]) {
      u2[0] = sc.unk[edges[3 * e]];
      u2[1] = sc.unk[edges[3 * e + 1]];
    }
    s_u[tid] = u2[0];
    s_u[EG_THREADS + tid] = u2[1];
    block_fence_sync();
    for (int side = 0; side < 2; ++side) {
      const int u = u2[side];
      if (u < 0) continue;
      int before = 0, after = 0;
      for (int t = 0; t < EG_THREADS; ++t) {   // an edge names an unknown once (i != j): threads order the entries
        const int hit = (s_u[t] == u) + (s_u[EG_THREADS + t] == u);
        before += t < tid ? hit : 0;
        after += t > tid ? hit : 0;
      }
      pos[side] = sc.deg[u] + before;
      last[side] = after == 0;
      sc.adj[sc.adjs[u] + pos[side]] = 2 * e + side;
    }
    block_fence_sync();
    for (int side = 0; side < 2; ++side)
      if (pos[side] >= 0 && last[side]) sc.deg[u2[side]] = pos[side] + 1;
    block_fence_sync();
  }

  // ---- the schedule
  const int nd = SPFE_EG_DIM * U;
  const size_t nh = (size_t)blocks * B49;
  spfe_lm lm = {a.lambda_init, 2.0};   // thread 0's
  if (tid == 0) { s_d[D_LAMBDA] = a.lambda_init; s_i[I_GO] = 1; }
  int it_done = 0, n_trials = 0, n_failed = 0, fresh = 0;
  double currentChi = 0.0, chi_initial = 0.0;
  block_fence_sync();
  for (int it = 0; it < a.iterations; ++it) {
    if (!s_i[I_GO]) break;
    if (!fresh) currentChi = eg_errors(sc, edges, E, s_part, tid);
    if (it == 0) chi_initial = currentChi;
    // the 14 perturbed estimates of every unknown and their inverses
    for (int item = tid; item < 14 * U; item += EG_THREADS) {
      const int v = sc.vert[item / 14], p = item % 14;
      spfe_s3o_sim S, fwd, inv;
      spfe_eg_load(sc.est + 8 * (size_t)v, &S);
      spfe_s3o_perturb(&S, p, a.fix_scale, &fwd, &inv);
      spfe_eg_store(&fwd, sc.pert + ((size_t)v * 28 + p) * 8);
      spfe_eg_store(&inv, sc.pert + ((size_t)v * 28 + 14 + p) * 8);
    }
    for (size_t k = tid; k < nh; k += EG_THREADS) sc.H[k] = 0.0;
    block_fence_sync();
    // Jacobians
    for (int e = tid; e < E; e += EG_THREADS) {
      if (!sc.ok[e]) continue;
      const int vi = edges[3 * e], vj = edges[3 * e + 1];
      const int ui = sc.unk[vi], uj = sc.unk[vj];
      if (ui < 0 && uj < 0) continue;
      spfe_s3o_sim Sji, Si, Sj, Sjinv, P;
      spfe_eg_load(sc.Sji + 8 * (size_t)e, &Sji);
      spfe_eg_load(sc.est + 8 * (size_t)vi, &Si);
      spfe_eg_load(sc.est + 8 * (size_t)vj, &Sj);
      spfe_s3o_inv(&Sj, &Sjinv);
      double ep[SPFE_EG_DIM], em[SPFE_EG_DIM];
      if (ui >= 0) {
#pragma unroll 1
        for (int d = 0; d < SPFE_EG_DIM; ++d) {
          spfe_eg_load(sc.pert + ((size_t)vi * 28 + 2 * d) * 8, &P);
          spfe_eg_error(&Sji, &P, &Sjinv, ep);
          spfe_eg_load(sc.pert + ((size_t)vi * 28 + 2 * d + 1) * 8, &P);
          spfe_eg_error(&Sji, &P, &Sjinv, em);
          spfe_eg_jcol(ep, em, sc.Ji + (size_t)B49 * e, d);
        }
      }
      if (uj >= 0) {
#pragma unroll 1
        for (int d = 0; d < SPFE_EG_DIM; ++d) {
          spfe_eg_load(sc.pert + ((size_t)vj * 28 + 14 + 2 * d) * 8, &P);
          spfe_eg_error(&Sji, &Si, &P, ep);
          spfe_eg_load(sc.pert + ((size_t)vj * 28 + 14 + 2 * d + 1) * 8, &P);
          spfe_eg_error(&Sji, &Si, &P, em);
          spfe_eg_jcol(ep, em, sc.Jj + (size_t)B49 * e, d);
        }
      }
    }
    block_fence_sync();
    // assembly by owner: (unknown u, row r)
    for (int item = tid; item < nd; item += EG_THREADS) {
      const int u = item / SPFE_EG_DIM, r = item % SPFE_EG_DIM;
      const int f = sc.first[u], rowbase = sc.rowoff[u];
      double hd[SPFE_EG_DIM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, bb = 0.0;
      for (int k = sc.adjs[u]; k < sc.adjs[u + 1]; ++k) {
        const int e = sc.adj[k] >> 1, side = sc.adj[k] & 1;
        const double *Ju = (side ? sc.Jj : sc.Ji) + (size_t)B49 * e;
        for (int c = 0; c < SPFE_EG_DIM; ++c) hd[c] += spfe_eg_dot7(Ju + r, 7, Ju + c, 7);
        bb -= spfe_eg_dot7(Ju + r, 7, sc.err + 7 * (size_t)e, 1);
        const int w = sc.unk[edges[3 * e + (side ? 0 : 1)]];
        if (w >= 0 && w < u) {
          const double *Jw = (side ? sc.Ji : sc.Jj) + (size_t)B49 * e;
          double *blk = sc.H + ((size_t)rowbase + (w - f)) * B49 + r * 7;
          for (int c = 0; c < SPFE_EG_DIM; ++c) blk[c] += spfe_eg_dot7(Ju + r, 7, Jw + c, 7);
        }
      }
      double *dg = sc.H + ((size_t)rowbase + (u - f)) * B49 + r * 7;
      for (int c = 0; c < SPFE_EG_DIM; ++c) dg[c] = hd[c];
      sc.b[item] = bb;
    }
    block_fence_sync();

    int qmax = 0, again = 0;
    do {
      const double lambda = s_d[D_LAMBDA];
      for (size_t k = tid; k < nh; k += EG_THREADS) sc.L[k] = sc.H[k];
      for (int j = tid; j < nd; j += EG_THREADS) sc.x[j] = sc.b[j];
      if (tid == 0) s_i[I_FAIL] = 0;
      block_fence_sync();
      for (int j = tid; j < nd; j += EG_THREADS) {
        const int u = j / SPFE_EG_DIM, r = j % SPFE_EG_DIM;
        sc.L[((size_t)sc.rowoff[u] + (u - sc.first[u])) * B49 + r * 8] += lambda;
      }
      block_fence_sync();
      // factorisation and forward substitution, right-looking over block columns
      int failed = 0;
      for (int w = 0; w < U; ++w) {
        if (tid == 0) {
          s_i[I_PCNT] = 0;
          double *D = sc.L + ((size_t)sc.rowoff[w] + (w - sc.first[w])) * B49;
          int okp = 1;
          for (int c = 0; c < 7; ++c) {
            double s = D[c * 7 + c];
            for (int k = 0; k < c; ++k) s -= D[c * 7 + k] * D[c * 7 + k];
            okp &= spfe_eg_pivot_ok(s);
            const double djj = sqrt(s);
            D[c * 7 + c] = djj;
            for (int r = c + 1; r < 7; ++r) {
              double t = D[r * 7 + c];
              for (int k = 0; k < c; ++k) t -= D[r * 7 + k] * D[c * 7 + k];
              D[r * 7 + c] = t / djj;
            }
          }
          for (int k = 0; k < B49; ++k) s_diag[k] = D[k];
          for (int i = 0; i < 7; ++i) {
            double s = sc.x[7 * w + i];
            for (int k = 0; k < i; ++k) s -= D[i * 7 + k] * s_vec[k];
            s = s / D[i * 7 + i];
            s_vec[i] = s;
            sc.x[7 * w + i] = s;
          }
          if (!okp) s_i[I_FAIL] = 1;
        }
        block_fence_sync();
        if (s_i[I_FAIL]) { failed = 1; break; }
        for (int u = w + 1 + tid; u < U; u += EG_THREADS) {
          if (sc.first[u] > w) continue;
          double *B = sc.L + ((size_t)sc.rowoff[u] + (w - sc.first[u])) * B49;
          const int slot = atomicAdd(&s_i[I_PCNT], 1);
          sc.plist[slot] = u;
          for (int r = 0; r < 7; ++r) {
            double row[7];
            for (int c = 0; c < 7; ++c) {
              double s = B[r * 7 + c];
              for (int k = 0; k < c; ++k) s -= row[k] * s_diag[c * 7 + k];
              row[c] = s / s_diag[c * 7 + c];
            }
            double xs = sc.x[7 * u + r];
            for (int c = 0; c < 7; ++c) {
              B[r * 7 + c] = row[c];
              if (slot < EG_PCAP) s_panel[(size_t)slot * B49 + r * 7 + c] = row[c];
              xs -= row[c] * s_vec[c];
            }
            sc.x[7 * u + r] = xs;
          }
        }
        block_fence_sync();
        const long long P = s_i[I_PCNT];
        for (long long item = tid; item < P * P * B49; item += EG_THREADS) {
          const int sa = (int)(item / (P * B49)), rem = (int)(item % (P * B49));
          const int sb = rem / B49, r = (rem % B49) / 7, c = rem % 7;
          const int ua = sc.plist[sa], ub = sc.plist[sb];
          if (ua < ub || (ua == ub && c > r)) continue;
          const int fa = sc.first[ua];
          const double *pa = sa < EG_PCAP ? s_panel + (size_t)sa * B49 + r * 7
                                          : sc.L + ((size_t)sc.rowoff[ua] + (w - fa)) * B49 + r * 7;
          const double *pb = sb < EG_PCAP ? s_panel + (size_t)sb * B49 + c * 7
                                          : sc.L + ((size_t)sc.rowoff[ub] + (w - sc.first[ub])) * B49 + c * 7;
          double *T = sc.L + ((size_t)sc.rowoff[ua] + (ub - fa)) * B49 + r * 7 + c;
          double t = *T;
          for (int j = 0; j < 7; ++j) t -= pa[j] * pb[j];
          *T = t;
        }
        block_fence_sync();
      }
      double sum = 0.0, tempChi = SPFE_EG_DBL_MAX;
      if (!failed) {
        // back substitution, block rows descending
        for (int u = U - 1; u >= 0; --u) {
          const int f = sc.first[u];
          if (tid == 0) {
            const double *D = sc.L + ((size_t)sc.rowoff[u] + (u - f)) * B49;
            for (int i = 6; i >= 0; --i) {
              double s = sc.x[7 * u + i];
              for (int k = 6; k > i; --k) s -= D[k * 7 + i] * s_vec[k];
              s = s / D[i * 7 + i];
              s_vec[i] = s;
              sc.x[7 * u + i] = s;
            }
          }
          block_fence_sync();
          for (int item = tid; item < (u - f) * 7; item += EG_THREADS) {
            const int wb = item / 7, i = item % 7;
            const double *B = sc.L + ((size_t)sc.rowoff[u] + wb) * B49;
            double s = sc.x[7 * (f + wb) + i];
            for (int k = 6; k >= 0; --k) s -= B[k * 7 + i] * s_vec[k];
            sc.x[7 * (f + wb) + i] = s;
          }
          block_fence_sync();
        }
        double sl = 0.0;
        if (tid < SPFE_DUST_SLOTS)
          for (int j = tid; j < nd; j += SPFE_DUST_SLOTS) sl += spfe_eg_scale_term(sc.x[j], lambda, sc.b[j]);
        sum = eg_tree(sl, s_part, tid);
        for (int u = tid; u < U; u += EG_THREADS) {
          const int v = sc.vert[u];
          spfe_s3o_sim S;
          spfe_eg_load(sc.est + 8 * (size_t)v, &S);
          spfe_eg_store(&S, sc.bak + 8 * (size_t)v);
          spfe_eg_oplus(&S, sc.x + 7 * (size_t)u, a.fix_scale);
          spfe_eg_store(&S, sc.est + 8 * (size_t)v);
        }
        block_fence_sync();
        tempChi = eg_errors(sc, edges, E, s_part, tid);
      } else {
        ++n_failed;
      }
      if (tid == 0) {
        double rho = 0.0;
        const int acc = spfe_eg_lm_judge(&lm, currentChi, tempChi, sum, &rho);
        ++qmax;   // thread 0's count is the one that decides
        s_i[I_ACCEPT] = acc;
        s_i[I_AGAIN] = rho < 0 && qmax < SPFE_LM_MAX_TRIALS;
        if (qmax == SPFE_LM_MAX_TRIALS || rho == 0) s_i[I_GO] = 0;
        s_d[D_LAMBDA] = lm.lambda;
      } else {
        ++qmax;
      }
      block_fence_sync();
      fresh = s_i[I_ACCEPT];
      again = s_i[I_AGAIN];
      if (fresh) {
        currentChi = tempChi;
      } else if (!failed) {
        for (int u = tid; u < U; u += EG_THREADS) {
          const int v = sc.vert[u];
          for (int k = 0; k < 8; ++k) sc.est[8 * (size_t)v + k] = sc.bak[8 * (size_t)v + k];
        }
      }
      ++n_trials;
      block_fence_sync();
    } while (again);
    ++it_done;
  }
  if (tid == 0) {
    hdr[5] = it_done; hdr[6] = n_trials; hdr[7] = n_failed;
    dout[0] = spfe_s3o_canon(chi_initial); dout[1] = spfe_s3o_canon(currentChi); dout[2] = spfe_s3o_canon(s_d[D_LAMBDA]);
  }
}

__global__ __launch_bounds__(256) void eg_recover_kernel(EgArgs a) {
  Scratch sc;
  scratch_carve(a.scratch, a.n, a.E, a.env_cap, &sc);
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= a.n) return;
  spfe_s3o_sim S;
  spfe_eg_load(sc.est + 8 * (size_t)v, &S);
  spfe_eg_store_canon(&S, reinterpret_cast<double *>(a.out + SPFE_ESSGRAPH_OFF_SIM3) + 8 * (size_t)v);
  float T[16];
  spfe_eg_recover(&S, T);
  float *o = reinterpret_cast<float *>(a.out + SPFE_ESSGRAPH_OFF_TIW(a.n)) + 16 * (size_t)v;
  for (int k = 0; k < 16; ++k) o[k] = T[k];
}

__global__ __launch_bounds__(256) void eg_sim3_base_kernel(const float *Tcw, double *est, double *meas, int n) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  float T[16];
  for (int k = 0; k < 16; ++k) T[k] = Tcw[16 * (size_t)v + k];
  spfe_s3o_sim S;
  spfe_eg_from_pose(T, &S);
  spfe_eg_store_canon(&S, est + 8 * (size_t)v);
  spfe_eg_store_canon(&S, meas + 8 * (size_t)v);
}

__global__ __launch_bounds__(64) void eg_sim3_conn_kernel(const float *Tcw, const double *S12, const float *Tcw2, const float *Twc,
                                                          const int *conn_slot, int n_conn, int cur_slot, double *est, int n) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= n_conn) return;
  const int v = conn_slot[k];
  if (v < 0 || v >= n) return;
  double s12[13];
  float tcw2[16], twc[16], tiw[16];
  for (int j = 0; j < 13; ++j) s12[j] = S12[j];
  for (int j = 0; j < 16; ++j) {
    tcw2[j] = Tcw2[j];
    twc[j] = Twc[j];
    tiw[j] = Tcw[16 * (size_t)v + j];
  }
  spfe_s3o_sim P;
  spfe_eg_corrected(s12, tcw2, twc, tiw, v == cur_slot, &P);
  spfe_eg_store_canon(&P, est + 8 * (size_t)v);
}

__global__ __launch_bounds__(256) void eg_correct_kernel(const double *S_from, const double *S_to, int n_kf, const int *ref_slot,
                                                         const int *point_idx, int m, float *xyz, const uint8_t *flags, int n_table,
                                                         uint8_t *code) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const int row = point_idx ? point_idx[i] : i;
  if (row < 0 || row >= n_table) { code[i] = SPFE_EGC_INVALID; return; }
  if (!(flags[row] & SPFE_PROJ_SEARCHABLE)) { code[i] = SPFE_EGC_SKIP_BAD; return; }
  const int r = ref_slot[i];
  if (r < 0 || r >= n_kf) { code[i] = SPFE_EGC_INVALID; return; }
  spfe_s3o_sim A, B;
  spfe_eg_load(S_from + 8 * (size_t)r, &A);
  spfe_eg_load(S_to + 8 * (size_t)r, &B);
  const float X[3] = {xyz[3 * (size_t)row], xyz[3 * (size_t)row + 1], xyz[3 * (size_t)row + 2]};
  float Y[3];
  spfe_eg_correct_point(&A, &B, X, Y);
  xyz[3 * (size_t)row] = Y[0]; xyz[3 * (size_t)row + 1] = Y[1]; xyz[3 * (size_t)row + 2] = Y[2];
  code[i] = SPFE_EGC_CORRECTED;
}

size_t eg_scratch_bytes(int n, int E, int env_cap) { return scratch_carve(nullptr, n, E, env_cap, nullptr); }

int eg_lds_panel_capacity() { return EG_PCAP; }

hipError_t launch_eg_optimize(const EgArgs &a, hipStream_t s) {
  if (a.n < 1 || a.n > SPFE_ESSGRAPH_MAX_KEYFRAMES || a.E < 0 || a.E > SPFE_ESSGRAPH_MAX_EDGES || a.env_cap < 0 ||
      a.env_cap > SPFE_ESSGRAPH_MAX_BLOCKS)
    return hipErrorInvalidValue;
  static LdsLimitOnce lds_once;   // (spfe_kernels.h)
  if (hipError_t e = raise_lds_limit(lds_once, reinterpret_cast<const void *>(eg_solve_kernel), (int)EG_LDS); e != hipSuccess) return e;
  size_t mark_off = 0;
  scratch_carve(nullptr, a.n, a.E, a.env_cap, nullptr, &mark_off);
  hipError_t e = launch_fill_u32(a.scratch + mark_off, 0u, (size_t)a.n + 1, s);
  if (e != hipSuccess) return e;
  const int items = a.n > a.E ? a.n : a.E;
  hipLaunchKernelGGL(eg_prepare_kernel, dim3((items + 255) / 256), dim3(256), 0, s, a);
  hipLaunchKernelGGL(eg_solve_kernel, dim3(1), dim3(EG_THREADS), EG_LDS, s, a);
  hipLaunchKernelGGL(eg_recover_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_eg_sim3(const float *Tcw, const double *S12, const float *Tcw2, const float *Twc, const int *conn_slot, int n_conn,
                          int cur_slot, double *est, double *meas, int n, hipStream_t s) {
  if (n < 1 || n > SPFE_ESSGRAPH_MAX_KEYFRAMES || n_conn < 0 || n_conn > n || cur_slot < -1 || cur_slot >= n)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(eg_sim3_base_kernel, dim3((n + 255) / 256), dim3(256), 0, s, Tcw, est, meas, n);
  if (n_conn > 0)
    hipLaunchKernelGGL(eg_sim3_conn_kernel, dim3((n_conn + 63) / 64), dim3(64), 0, s, Tcw, S12, Tcw2, Twc, conn_slot, n_conn, cur_slot,
                       est, n);
  return hipGetLastError();
}

hipError_t launch_eg_correct(const double *S_from, const double *S_to, int n_kf, const int *ref_slot, const int *point_idx, int m,
                             float *xyz, const uint8_t *flags, int n_table, uint8_t *code, hipStream_t s) {
  if (m < 0 || m > SPFE_MP_MAX_POINTS || n_kf < 1 || n_table < 0) return hipErrorInvalidValue;
  if (m > 0)
    hipLaunchKernelGGL(eg_correct_kernel, dim3((m + 255) / 256), dim3(256), 0, s, S_from, S_to, n_kf, ref_slot, point_idx, m, xyz, flags,
                       n_table, code);
  return hipGetLastError();
}

}  // namespace spfe
