// Per-step MPC: condensed QP assembly for the linear / bilinear Koopman model and a dense
// strictly convex QP solve, one workgroup per problem.
//
// Replaces Kmpc.get_mpcInput (Kmpc.m:329-387), get_mpcInput_bilinear(_iter) (:750-904) with
// get_costB/H/G/D_bilinear (:569-622), and the quadprog call (:383,810,883).
//
// Algebra: P_k = proj*A^k, Beta(z) = B*kron(I_m,z), S_k = P_k*Beta(z_k);
// (Chat*Bhat)[i,j] = S_{i-j-1} for i > j;  H = (CB)'Q(CB) + R;  f = 2 (CB)'Q(Chat*Ahat*z - Yr).
// The reference rebuilds the (N(Np+1)) x (m Np) matrix Bhat four times per step with dense
// matrix powers; here P_k is precomputed once and only the nproj x m blocks S_k are formed.
//
// QP: Goldfarb-Idnani dual active set run by one wavefront, with the inverse of the active
// constraints' Schur complement (N'H^-1 N)^-1 updated by bordering / deletion formulas, so an
// iteration is O(n^2) lane-parallel work without triangular solves.
#include <algorithm>
#include <cmath>
#include <vector>

#include <cstring>

#include "kp_internal.h"
#include "koopman_hip_sim.h"
#include "kp_wg_inverse.h"
#include "kp_sim_loop.h"
#include <type_traits>

#include "kp_qp.h"

struct kp_mpc {
  kp_ctx* ctx = nullptr;
  int model_type = 0, N = 0, m = 0, Np = 0, nproj = 0, nvar = 0, nrows = 0, mb = 0;
  double q_run = 0, q_term = 0;
  // device
  double* A = nullptr;     // N x N
  double* B = nullptr;     // N x mb
  double* P = nullptr;     // (Np+1) x [nproj x N]  (P_k column-major nproj x N)
  double* S0 = nullptr;    // linear model: Np x [nproj x m]
  double* PB = nullptr;    // bilinear model: [Np * m * nproj][N]  rows of P_k B_i (S_k = P_k Beta(z) = these rows times z); inside P's allocation
  int stage_doubles = 0;   // size of that allocation
  double* r = nullptr;     // m
  double* Aq = nullptr;    // nrows x nvar column-major (constant: L = F, tack rows)
  double* bq0 = nullptr;   // nrows (c and zeros for the tack rows)
  double* Anorm = nullptr; // nrows
  double* ellv = nullptr;  // K x nrows
  int* ellc = nullptr;     // K x nrows
  int ellK = 1;
  double* work = nullptr;  // per-problem QP export: Hq (nvar^2) | f (nvar)
  size_t work_problems = 0;
  double *d_in = nullptr, *d_out = nullptr;     // d_out: x (nvar) and z (N) per problem, then the status words
  double *h_in = nullptr, *h_out = nullptr;     // pinned staging buffers: one copy in, one copy out per step
  unsigned long long* h_flag = nullptr;         // pinned: [0] sequence number of the last finished single step, [1] start, [2] end stamp
  unsigned long long step_seq = 0;
  int* warm = nullptr;                          // device: [count, rows...] optimal active set of the last single step
  int* d_status = nullptr;                      // points into d_out
  size_t io_problems = 0;
  // state bounds (Kmpc.m:300-318 / :716-730), single-problem steps only
  int sb_n = 0, sb_kmax = 0, sb_rows = 0;       // n bounded outputs, highest power of A needed, 2 n (Np + 1) rows
  double* sb_lohi = nullptr;                    // [lo (n) | hi (n)] scaled down
  double* sb_Apow = nullptr;                    // (kmax + 1) x [N x N]: A^0 .. A^kmax
  double* sb_A = nullptr;                       // dense constraint matrix of a step: (nrows + sb_rows) x nvar, column-major
  double* sb_b = nullptr;                       // | right-hand sides | row norms | solution x
  int* sb_col = nullptr;                        // ELL column table of a dense matrix: col[k * rows + r] = k
  size_t sb_cap = 0;                            // problems sb_A / sb_b are sized for
  double* sb_work = nullptr;                    // [sb_cap][nvar^2 + nvar + nrows]: H, f, b of every problem of a batch
  // loaded steps: page-locked [observation window | estimate (nw) and resnorm] that the kernel reads and writes in place
  double* h_ld = nullptr;
  size_t h_ld_doubles = 0;
};

// ---- generic QP shim kernel -----------------------------------------------------------------
// One wave per problem.  Problem p = blockIdx.x reads H + p sH, f + p sf, the ELL values / row norms + p sA / p sb and
// b + p sb, writes x + p n and status[p] (strides in doubles; 0 for a single problem).  sticky: a problem whose status
// word already carries a failure (an earlier linearisation pass) is left alone.
__global__ __launch_bounds__(64) void kp_qp_kernel(const double* H, const double* f, EllMat A, const double* b, int n, int mr,
                                                   double* x, int* status, size_t sH, size_t sf, size_t sA, size_t sb, int sticky) {
  extern __shared__ double sm[];
  const size_t p = blockIdx.x;
  if (sticky && status[p] != KP_OK) return;
  EllMat Ap = A;
  Ap.val = A.val + p * sA;
  Ap.norm = A.norm + p * sb;
  int st = qp_goldfarb_idnani(H + p * sH, f + p * sf, Ap, b + p * sb, n, mr, sm, x + p * (size_t)n, 1e-10);
  if (threadIdx.x == 0) status[p] = st ? KP_ERR_QP_FAIL : KP_OK;
}

// dense (mr x n, column-major) -> ELL on the host
static void to_ell(const double* A, int mr, int n, std::vector<double>& val, std::vector<int>& col, std::vector<double>& norm, int& K) {
  K = 1;
  for (int r = 0; r < mr; ++r) {
    int c = 0;
    for (int j = 0; j < n; ++j) c += A[r + (size_t)j * mr] != 0.0;
    K = std::max(K, c);
  }
  val.assign((size_t)K * mr, 0.0);
  col.assign((size_t)K * mr, 0);
  norm.assign(mr, 0.0);
  for (int r = 0; r < mr; ++r) {
    int k = 0;
    double s = 0.0;
    for (int j = 0; j < n; ++j) {
      double v = A[r + (size_t)j * mr];
      if (v != 0.0) {
        val[(size_t)k * mr + r] = v;
        col[(size_t)k * mr + r] = j;
        s += v * v;
        ++k;
      }
    }
    norm[r] = std::sqrt(s);
  }
}

extern "C" int kp_qp_solve(kp_ctx* ctx, const double* H, const double* f, const double* A, const double* b, int n, int mr,
                           double* x, int* status) {
  if (!ctx || !H || !f || !x || n < 1 || n > QP_MAXN || mr < 0 || (mr > 0 && (!A || !b)))
    return ctx ? ctx->fail(KP_ERR_ARG, "kp_qp_solve: bad argument (n <= 64)") : KP_ERR_ARG;
  KP_HIP(ctx, hipSetDevice(ctx->device));
  std::vector<double> val, norm;
  std::vector<int> col;
  int K = 1;
  to_ell(A, mr, n, val, col, norm, K);
  size_t bH = (size_t)n * n * 8, bV = val.size() * 8, bCo = col.size() * 4;
  char* ws = (char*)ctx->workspace(7, bH + bV + bCo + (size_t)(2 * n + 2 * mr) * 8 + 64);
  if (!ws) return ctx->fail(KP_ERR_HIP, "kp_qp_solve: out of device memory");
  double* dH = (double*)ws;
  double* dV = (double*)(ws + bH);
  double* df = (double*)(ws + bH + bV);
  double* dx = df + n;
  double* db = dx + n;
  double* dn = db + mr;
  int* dC = (int*)(dn + mr);
  int* dst = dC + col.size();
  hipStream_t s = ctx->stream;
  KP_HIP(ctx, hipMemcpyAsync(dH, H, bH, hipMemcpyHostToDevice, s));
  KP_HIP(ctx, hipMemcpyAsync(df, f, (size_t)n * 8, hipMemcpyHostToDevice, s));
  if (mr) {
    KP_HIP(ctx, hipMemcpyAsync(dV, val.data(), bV, hipMemcpyHostToDevice, s));
    KP_HIP(ctx, hipMemcpyAsync(dC, col.data(), bCo, hipMemcpyHostToDevice, s));
    KP_HIP(ctx, hipMemcpyAsync(db, b, (size_t)mr * 8, hipMemcpyHostToDevice, s));
    KP_HIP(ctx, hipMemcpyAsync(dn, norm.data(), (size_t)mr * 8, hipMemcpyHostToDevice, s));
  }
  EllMat E{dV, dC, dn, K};
  size_t lds = (size_t)qp_lds_doubles(n, mr) * 8;
  if (lds > 160 * 1024) return ctx->fail(KP_ERR_ARG, "kp_qp_solve: problem too large");
  static KpLdsCache qp_lds;
  KP_HIP(ctx, kp_ensure_lds(qp_lds, (const void*)kp_qp_kernel, lds));
  hipLaunchKernelGGL(kp_qp_kernel, dim3(1), dim3(64), lds, s, dH, df, E, db, n, mr, dx, dst, (size_t)0, (size_t)0, (size_t)0, (size_t)0, 0);
  KP_HIP(ctx, hipGetLastError());
  int st = 0;
  KP_HIP(ctx, hipMemcpyAsync(x, dx, (size_t)n * 8, hipMemcpyDeviceToHost, s));
  KP_HIP(ctx, hipMemcpyAsync(&st, dst, sizeof(int), hipMemcpyDeviceToHost, s));
  KP_HIP(ctx, hipStreamSynchronize(s));   // also keeps the host vectors alive until the copies are done
  if (status) *status = st;
  return KP_OK;
}

// ---- MPC setup ---------------------------------------------------------------------------------
// P_0 = proj, P_{k+1} = P_k A   (Ahat rows of Kmpc.m:168-172 / 528-532 projected by Chat :193,540);
// linear model: S_k = P_k B.
__global__ __launch_bounds__(256) void kp_mpc_setup_kernel(const double* __restrict__ A, const double* __restrict__ B,
                                                           const double* __restrict__ proj, int N, int m, int Np, int nproj,
                                                           int linear, double* __restrict__ P, double* __restrict__ S0,
                                                           double* __restrict__ PB) {
  const int tid = threadIdx.x;
  for (int e = tid; e < nproj * N; e += 256) P[e] = proj[e];
  __syncthreads();
  for (int k = 0; k < Np; ++k) {
    const double* Pk = P + (size_t)k * nproj * N;
    double* Pn = P + (size_t)(k + 1) * nproj * N;
    for (int e = tid; e < nproj * N; e += 256) {
      int p = e % nproj, c = e / nproj;
      double s = 0.0;
      for (int j = 0; j < N; ++j) s += Pk[p + j * nproj] * A[j + (size_t)c * N];
      Pn[e] = s;
    }
    __syncthreads();
  }
  if (linear) {
    for (int e = tid; e < Np * nproj * m; e += 256) {
      int k = e / (nproj * m), rem = e % (nproj * m), p = rem % nproj, a = rem / nproj;
      const double* Pk = P + (size_t)k * nproj * N;
      double s = 0.0;
      for (int j = 0; j < N; ++j) s += Pk[p + j * nproj] * B[j + (size_t)a * N];
      S0[e] = s;
    }
  } else {
    // bilinear: S_k = P_k Beta(z) with Beta(z) = [B_1 z ... B_m z] (Kmpc.m:578-585), i.e. entry (p, i) of S_k is row p of
    // P_k B_i times z.  Those rows are constants of the model: Np m nproj N doubles (40 KB for the bench's N = 84) instead of
    // the N x N m of B (169 KB) that a step would otherwise stream through its one CU to form Beta(z) first.
    for (int e = tid; e < Np * nproj * m * N; e += 256) {
      const int j = e % N, row = e / N;
      const int k = row / (nproj * m), rem = row % (nproj * m), p = rem % nproj, i = rem / nproj;
      const double* Pk = P + (size_t)k * nproj * N;
      const double* Bi = B + (size_t)i * N * N + (size_t)j * N;
      double s = 0.0;
      for (int c = 0; c < N; ++c) s += Pk[p + c * nproj] * Bi[c];
      PB[e] = s;
    }
  }
}


struct MpcArgs {
  BasisDev basis;   // used when zeta != nullptr (fused lift)
  int model_type, N, m, Np, nproj, nvar, nrows, iters, has_basis;
  double q_run, q_term;
  const double *A, *B, *P, *S0, *PB, *r, *Aq, *bq0, *Anorm;
  EllMat ell;
  int* warm;            // [1 + nvar] active set of the previous single-problem step (nullptr: cold start)
  int alias;            // batched launches: z | beta | S | e live inside the solver's scratch (dead before it is first written)
  int assemble_only;    // stop after the QP data have been exported (state-bound steps solve with the generic QP kernel)
  const double* U_lin;  // [nb][nvar] or nullptr: re-linearise along the lifted horizon of THESE inputs (pass >= 2 of a
                        // state-bound step, Kmpc.m:890-895) instead of starting from z
  const double* z;      // [nb][N]      (or nullptr with zeta)
  const double* zeta;   // [nb][nzeta]  (fused lift)
  const double* u_prev; // [nb][m]
  const double* Yr;     // [nb][nproj*(Np+1)]
  double* U;            // [nb][nvar]   x = vec(U') : u_0 (m), u_1 (m), ...
  double* z_out;        // [nb][N] or nullptr
  double* qp_export;    // [nb][nvar*nvar + nvar + nrows] or nullptr
  int* status;          // [nb]
  long long* stamps;    // [8] wall_clock64 stamps + [8] counters of problem 0 (diagnostics), or nullptr
  unsigned long long* done_flag;   // pinned host word: the kernel stores done_seq there when its outputs are visible (or nullptr)
  unsigned long long done_seq;
  int qp_wg;            // active-set iteration by the whole workgroup (qp_gi_wg) when the problem qualifies
  int stage_off;        // single-problem launches: P | PB are copied to LDS at this offset (doubles) at kernel start; 0: read from L2
  int stage_doubles;    // multiple of 512 (every wave issues the same number of 1 KB LDS-DMA loads)
};

// LDS (doubles): z N | beta N*m | S Np*nproj*m | e (Np+1)*nproj | Hq nvar^2 | f nvar | b nrows | zh (Np+1)*N (iters>1)
//                | full nfull (fused lift) | qp scratch
__host__ __device__ inline int mpc_lds_doubles(int N, int m, int Np, int nproj, int nvar, int nrows, int iters, int nfull) {
  return N + N * m + Np * nproj * m + (Np + 1) * nproj + nvar * nvar + nvar + nrows + (iters > 1 ? (Np + 1) * N : 0) + nfull + 4 +
         qp_lds_doubles(nvar, nrows);
}

// ---- loaded steps (kp_mpc_step_loaded): the load observer in front of the step ----------------------------------------
// Kmpc.estimate_load_linear / _bilinear (Kmpc.m:1298-1356, :1360-1444) over a window of nobs past samples, then the loaded
// lift z = [psi; w_1 psi; ...; w_nw psi] (Ksysid.m:1606-1612) of the current zeta.  The observer works in its own LDS block
// behind the step's (offsets in doubles, each even):
//   win: the staged window [(nobs + 1) x nzeta zeta rows | nobs x m inputs | nw previous estimate]
//   fullc: dictionary columns of `chunk` window rows | psi: max(nobs, 1) x Nb | R: nobs x nz x (nw + 1) | d: nobs x nz
//   M: (nw + 1)^2 normal matrix, q (nw + 1), d'd | QP: H nw^2, f, b, val, norm (2 nw each), col (2 nw ints), x (nw)
//   xw: [1; w] | the QP solver's scratch
#define KP_LOAD_MAX_NW 8
#define KP_LOAD_MAX_NOBS 64
#define KP_LOAD_FULL_CHUNK 4096   // doubles of dictionary columns evaluated per pass over the window rows
struct LoadLayout {
  int win, fullc, psi, R, d, M, H, f, b, val, norm, col, x, xw, qws, total, chunk;
};
__host__ __device__ inline int even_up(int n) { return (n + 1) & ~1; }
__host__ __device__ inline LoadLayout load_layout(int nw, int nobs, int nzeta, int m, int nfull, int Nb) {
  LoadLayout L;
  const int nw1 = nw + 1, nr = 2 * nw;
  L.chunk = nobs < 1 ? 1 : (KP_LOAD_FULL_CHUNK / nfull < 1 ? 1 : (KP_LOAD_FULL_CHUNK / nfull < nobs ? KP_LOAD_FULL_CHUNK / nfull : nobs));
  int o = 0;
  L.win = o; o += even_up((nobs + 1) * nzeta + nobs * m + nw);
  L.fullc = o; o += even_up(L.chunk * nfull);
  L.psi = o; o += even_up((nobs > 1 ? nobs : 1) * Nb);
  L.R = o; o += even_up(nobs * nzeta * nw1);
  L.d = o; o += even_up(nobs * nzeta);
  L.M = o; o += even_up(nw1 * nw1 + nw1 + 1);
  L.H = o; o += even_up(nw * nw);
  L.f = o; o += even_up(nw);
  L.b = o; o += even_up(nr);
  L.val = o; o += even_up(nr);
  L.norm = o; o += even_up(nr);
  L.col = o; o += even_up((nr + 1) / 2);
  L.x = o; o += even_up(nw);
  L.xw = o; o += even_up(nw1 + 1);
  L.qws = o; o += even_up(qp_lds_doubles(nw, nr));
  L.total = o;
  return L;
}
enum { KP_LOAD_RATE = 1, KP_LOAD_PIN_LAST = 2 };   // (the flags of kp_mpc_step_loaded)
struct MpcLoadArgs {
  int nw, nobs, flags, obs_off;   // obs_off: LDS offset (doubles) of the observer's block
  const double* win;              // the window block in page-locked host memory (layout of `win` above)
  double* out;                    // [nw] estimate | resnorm | 1 when the estimate failed, else 0  (page-locked host memory)
};

// one dictionary column of zeta: the evaluation of the fused lift in mpc_step_body, for the observer's window rows (the
// unloaded instantiations keep their own copy of the loop, so that their code does not change)
__device__ __forceinline__ double mpc_full_col(const BasisDev& b, const ColDesc& cd, const double* zeta) {
  if (cd.kind == COL_MONO && b.nvars <= 8) {
    int ex[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) ex[i] = ((uint32_t)(i < 4 ? cd.aux : cd.pad) >> (8 * (i & 3))) & 0xff;
    double v = 1.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const double x = zeta[i < b.nvars ? i : 0];
      for (int k = 0; k < ex[i]; ++k) v *= x;
    }
    return v;
  }
  return kp_eval_col(b, cd, zeta, 1);
}
// entry c of psi = econ_full(zeta) from its dictionary columns (dim_red: [zeta; pcs' full; 1], Ksysid.m:1521-1565)
__device__ __forceinline__ double mpc_psi_entry(const BasisDev& b, const double* zeta, const double* full, int c) {
  if (b.k_pcs == 0) return full[c];
  if (c < b.nvars) return zeta[c];
  if (c < b.nvars + b.k_pcs) {
    const double* pc = b.pcs + (size_t)(c - b.nvars) * b.nfull;
    double v = 0.0;
    for (int i = 0; i < b.nfull; ++i) v += pc[i] * full[i];
    return v;
  }
  return 1.0;
}

// The end of a loaded step whose estimate failed: the status word and, for a single zero-copy step, the release of the
// spinning host thread (the same sequence as the end of mpc_step_body, which keeps its own copy so that the code of the
// unloaded instantiations does not change).
__device__ __forceinline__ void mpc_step_finish(const MpcArgs& a, int pb, int tid, int status, long long* stamps) {
  if (tid == 0) a.status[pb] = status ? KP_ERR_QP_FAIL : KP_OK;
  if (a.done_flag && pb == 0) {
    __syncthreads();
    if (tid == 0) {
      __threadfence_system();
      if (stamps) { a.done_flag[1] = (unsigned long long)stamps[0]; a.done_flag[2] = (unsigned long long)wall_clock64(); }
      __threadfence_system();
      __hip_atomic_store(&a.done_flag[0], a.done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// The load observer of a loaded step, by the whole workgroup (the window is in LDS at ob + L.win).  For past sample i with
// psi_i = econ_full(zeta_i) the regression rows are R_i = G_i kron(I_{nw+1}, psi_i), G_i = A[:nz,:] (linear) or
// A[:nz,:] + sum_j u_ij B_j[:nz,:] (bilinear): column l of R_i is the nz x Nb block l of G_i times psi_i, so no kron is
// formed.  The right-hand sides are zeta_{i+1}[:nz] - B[:nz,:] u_i (linear) or zeta_{i+1}[:nz] (bilinear).  The normal
// equations M = sum R_i'R_i, q = sum R_i'd_i give the lsqlin of Kmpc.m:1354 / :1442 as a QP in the free loads:
// min ||R [1; w] - d||^2, -1 <= w <= 1 and, with KP_LOAD_RATE, |w - what_prev| <= 0.01; KP_LOAD_PIN_LAST pins the last
// load to zero (the debugging equality Aeq = blkdiag(1, 0, 1) of Kmpc.m:1350).  Solved by wave 0 with the dual active-set
// solver of kp_qp_solve (the host-assembled path's solver).  nobs = 0: no estimate, w = what_prev.
// Writes [1; w] to xw (LDS), the estimate, the residual norm and the failure flag to la.out; returns true (uniform) when the
// QP failed.
__device__ __forceinline__ bool mpc_load_observer(const MpcArgs& a, const MpcLoadArgs& la, double* ob, double*& xw) {
  const int tid = threadIdx.x;
  const BasisDev& b = a.basis;
  const int nw = la.nw, nobs = la.nobs, nz = b.nzeta, Nb = b.N, N = a.N, m = a.m, nw1 = nw + 1;
  const LoadLayout L = load_layout(nw, nobs, nz, m, b.nfull, Nb);
  const double* zw = ob + L.win;
  const double* uw = zw + (nobs + 1) * nz;
  const double* wprev = uw + nobs * m;
  double* fullc = ob + L.fullc;
  double* psi = ob + L.psi;
  double* R = ob + L.R;
  double* dv = ob + L.d;
  double* Mq = ob + L.M;
  xw = ob + L.xw;
  if (nobs == 0) {
    if (tid <= nw) xw[tid] = tid == 0 ? 1.0 : wprev[tid - 1];
    if (tid < nw) la.out[tid] = wprev[tid];
    if (tid == 0) { la.out[nw] = 0.0; la.out[nw + 1] = 0.0; }
    wg_lds_barrier();
    return false;
  }
  // psi of the first nobs window rows, `chunk` rows per pass
  for (int r0 = 0; r0 < nobs; r0 += L.chunk) {
    const int nr = min(L.chunk, nobs - r0);
    for (int e = tid; e < nr * b.nfull; e += 256) {
      const int i = e / b.nfull, c = e - i * b.nfull;
      fullc[e] = mpc_full_col(b, b.cols[c], zw + (size_t)(r0 + i) * nz);
    }
    wg_lds_barrier();
    for (int e = tid; e < nr * Nb; e += 256) {
      const int i = e / Nb, c = e - i * Nb;
      psi[(r0 + i) * Nb + c] = mpc_psi_entry(b, zw + (size_t)(r0 + i) * nz, fullc + i * b.nfull, c);
    }
    wg_lds_barrier();
  }
  // regression rows R[i][r][l] and right-hand sides d[i][r]
  const bool bil = a.model_type == KP_MODEL_BILINEAR;
  for (int e = tid; e < nobs * nz * nw1; e += 256) {
    const int i = e / (nz * nw1), rem = e - i * nz * nw1, r = rem / nw1, l = rem - r * nw1;
    const double* ps = psi + i * Nb;
    const double* Ar = a.A + r + (size_t)l * Nb * N;
    double s = 0.0;
    for (int c = 0; c < Nb; ++c) s += Ar[(size_t)c * N] * ps[c];
    if (bil)
      for (int j = 0; j < m; ++j) {
        const double* Br = a.B + r + ((size_t)j * N + (size_t)l * Nb) * N;
        double t = 0.0;
        for (int c = 0; c < Nb; ++c) t += Br[(size_t)c * N] * ps[c];
        s += t * uw[i * m + j];
      }
    R[e] = s;
  }
  for (int e = tid; e < nobs * nz; e += 256) {
    const int i = e / nz, r = e - i * nz;
    double v = zw[(i + 1) * nz + r];
    if (!bil) {
      double s = 0.0;
      for (int j = 0; j < m; ++j) s += a.B[r + (size_t)j * N] * uw[i * m + j];
      v -= s;
    }
    dv[e] = v;
  }
  wg_lds_barrier();
  // M (nw1 x nw1), q (nw1), d'd: 16 lanes per entry, summed by shuffles
  const int nM = nw1 * nw1 + nw1 + 1, nt = nobs * nz;
  for (int e16 = tid; e16 < nM * 16; e16 += 256) {
    const int e = e16 >> 4, part = e16 & 15;
    int c1, c2;   // columns of [R d] (nw1: d)
    if (e < nw1 * nw1) { c1 = e % nw1; c2 = e / nw1; }
    else if (e < nM - 1) { c1 = e - nw1 * nw1; c2 = nw1; }
    else { c1 = nw1; c2 = nw1; }
    double s = 0.0;
    for (int t = part; t < nt; t += 16) {
      const double x1 = c1 < nw1 ? R[t * nw1 + c1] : dv[t];
      const double x2 = c2 < nw1 ? R[t * nw1 + c2] : dv[t];
      s += x1 * x2;
    }
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    s += __shfl_xor(s, 8, 64);
    if (part == 0) Mq[e] = s;
  }
  wg_lds_barrier();
  // the QP in the free loads (w_0 .. w_{nf-1}; the pinned last one is 0)
  const int nf = (la.flags & KP_LOAD_PIN_LAST) ? nw - 1 : nw;
  double* H = ob + L.H;
  double* f = ob + L.f;
  double* bq = ob + L.b;
  double* val = ob + L.val;
  double* nrm = ob + L.norm;
  int* col = (int*)(ob + L.col);
  double* x = ob + L.x;
  int* st_sh = (int*)(xw + nw1);
  if (tid < 64) {
    const int lane = tid;
    for (int e = lane; e < nf * nf; e += 64) {
      const int k1 = e % nf, k2 = e / nf;
      H[e] = 2.0 * Mq[(k1 + 1) + (k2 + 1) * nw1];
    }
    const double* q = Mq + nw1 * nw1;
    if (lane < nf) {
      f[lane] = -2.0 * (q[lane + 1] - Mq[lane + 1]);     // -2 Rf'(d - R e_0)
      double lo = -1.0, hi = 1.0;
      if (la.flags & KP_LOAD_RATE) { lo = fmax(lo, wprev[lane] - 0.01); hi = fmin(hi, wprev[lane] + 0.01); }
      val[2 * lane] = 1.0; col[2 * lane] = lane; nrm[2 * lane] = 1.0; bq[2 * lane] = hi;
      val[2 * lane + 1] = -1.0; col[2 * lane + 1] = lane; nrm[2 * lane + 1] = 1.0; bq[2 * lane + 1] = -lo;
    }
    WSYNC();
    int st = 0;
    if (nf > 0) st = qp_goldfarb_idnani(H, f, EllMat{val, col, nrm, 1}, bq, nf, 2 * nf, ob + L.qws, x, 1e-10);
    WSYNC();
    if (lane <= nw) xw[lane] = lane == 0 ? 1.0 : (lane <= nf ? x[lane - 1] : 0.0);
    WSYNC();
    // resnorm = ||R [1; w] - d||^2, from the rows (the quadratic form in M, q, d'd would cancel)
    double s = 0.0;
    for (int t = lane; t < nt; t += 64) {
      double r_ = 0.0;
      for (int l = 0; l < nw1; ++l) r_ += R[t * nw1 + l] * xw[l];
      r_ -= dv[t];
      s += r_ * r_;
    }
    s = wave_sum(s);
    if (lane < nw) la.out[lane] = st ? __builtin_nan("") : xw[lane + 1];
    if (lane == 0) {
      la.out[nw] = st ? __builtin_nan("") : s;
      la.out[nw + 1] = st ? 1.0 : 0.0;
      *st_sh = st;
    }
  }
  wg_lds_barrier();
  return *st_sh != 0;
}

// WARM: single-problem instantiation with the active-set warm start; the batched one carries none of that code
// (its registers and branches cost the batch 1.8x when they were a run-time option).
// LOADED: the load observer and the loaded lift in front (kp_mpc_step_loaded, la != nullptr); the other instantiations
// carry none of its code.
// SIM: one step of a device-resident closed loop (kp_mpc_sim_kernel, si != nullptr): zeta, u_prev and the reference window
// are taken from LDS, where the loop keeps them, the solution goes to LDS and the P | PB block was staged by the caller.
// Returns the step's status (0, or nonzero when a QP failed; uniform).
struct MpcSimIn {
  const double *zeta, *up, *yr;   // LDS: nzeta | m | (Np + 1) nproj
  double* x;                      // LDS: the solution [u_0; u_1; ...] (nvar)
  double* z;                      // set by the step: its lifted state (LDS, N), intact until the next step
};
template <bool WARM, bool LOADED = false, bool SIM = false>
__device__ __forceinline__ int mpc_step_body(const MpcArgs& a, const MpcLoadArgs* la = nullptr, MpcSimIn* si = nullptr) {
  extern __shared__ __align__(16) double sm[];
  const int tid = threadIdx.x;
  const int pb = SIM ? 0 : blockIdx.x;     // (SIM: the caller's pointers are the trial's own)
  const int N = a.N, m = a.m, Np = a.Np, nproj = a.nproj, nv = a.nvar, nr = a.nrows;
  // a.alias (batched launches, one linearisation pass): the assembly's inputs z | beta | S | e are dead once Hq and f
  // exist, which is before the solver's scratch is first written - they live in its second n x n block, and a problem
  // takes 40.7 KB instead of 44.6: FOUR workgroups per CU instead of three.
  const int n_asm = N + N * m + Np * nproj * m + (Np + 1) * nproj;
  double* Hq = sm + (a.alias ? 0 : n_asm);   // nv x nv  (= 2H)
  double* f = Hq + nv * nv;
  double* bq = f + nv;
  double* zh = bq + nr;                  // (Np+1) x N   lifted horizon (iters > 1)
  double* full = zh + ((a.iters > 1 || a.U_lin) ? (Np + 1) * N : 0);
  int* st_sh = (int*)(full + (a.has_basis ? a.basis.nfull : 0));   // one slot for the QP status
  double* qpws = (double*)st_sh + 1;
  qpws += (qpws - sm) & 1;                // 16-byte aligned (sm is), by index arithmetic: the pointer stays an LDS pointer
  double* z = a.alias ? qpws + nv * nv : sm;
  double* beta = z + N;                  // N x m  (Beta(z) = B kron(I,z), Ksysid.m:1288-1289)
  double* S = beta + N * m;              // [Np][nproj x m]
  double* ev = S + Np * nproj * m;       // [(Np+1)][nproj]   P_i z - Yr_i
  const double* Yr = a.Yr + (size_t)pb * nproj * (Np + 1);
  const double* up = a.u_prev + (size_t)pb * m;
  long long* stamps = (a.stamps && pb == 0) ? a.stamps : nullptr;
  if (stamps && tid == 0) stamps[0] = wall_clock64();

  // The step's inputs lie in page-locked HOST memory in single-problem launches (zero-copy: no copy command on the latency
  // path of a closed loop), so every access is a PCIe round trip of ~2.3 us.  u_prev, Yr and zeta / z are requested HERE,
  // before anything else that has to be waited for - one round trip instead of three behind each other (dictionary ->
  // right-hand sides -> tracking error) - and go straight to the LDS arrays that are written for good only later: u_prev
  // to f, Yr to e (which becomes P z - Yr in place), zeta (or the lifted state itself) to z, which the dictionary evaluation
  // reads and only the step after it overwrites.  By LDS-DMA (4-byte pieces: any alignment of the caller's block), one array
  // per wave: no register waits for them.  (Measured and undone: everything that consumes them moved into the first pass of
  // the linearisation loop, so that the loop's hoisted address arithmetic - ~2 us of scalar instructions after the tracking
  // error - would run while the words are in flight: the hoisted block grew to ~1 500 instructions, longer than the round
  // trip it was to hide behind, 32.6 against 31.7 us.)
  const double* zin = a.has_basis ? a.zeta + (size_t)pb * a.basis.nzeta : a.z + (size_t)pb * N;
  const int nzin = a.has_basis ? a.basis.nzeta : N, nyr = (Np + 1) * nproj;
  if constexpr (SIM) {
    // the loop's state is in LDS (the previous step's ordinary stores; an LDS-DMA from global memory is not ordered behind
    // those): plain copies to the same three arrays, published by the barrier below
    for (int e = tid; e < nzin; e += 256) z[e] = si->zeta[e];
    for (int e = tid; e < nyr; e += 256) ev[e] = si->yr[e];
    if (tid < m) f[tid] = si->up[tid];
    si->z = z;
  } else {
    typedef __attribute__((address_space(3))) char lds_char;
    typedef __attribute__((address_space(1))) const char glb_char;
    const int w_ = tid >> 6, l4 = (tid & 63) * 4;
    const double* src = w_ == 0 ? zin : w_ == 1 ? Yr : up;
    double* dst = w_ == 0 ? z : w_ == 1 ? ev : f;
    const int bytes = w_ == 0 ? nzin * 8 : w_ == 1 ? nyr * 8 : w_ == 2 ? m * 8 : 0;
    for (int o = 0; o < bytes; o += 256)
      if (o + l4 < bytes) __builtin_amdgcn_global_load_lds((glb_char*)src + o + l4, (lds_char*)dst + o, 4, 0, 0);
    if constexpr (LOADED) {   // the observation window by the fourth wave
      const int wbytes = ((la->nobs + 1) * a.basis.nzeta + la->nobs * m + la->nw) * 8;
      if (w_ == 3)
        for (int o = 0; o < wbytes; o += 256)
          if (o + l4 < wbytes)
            __builtin_amdgcn_global_load_lds((glb_char*)la->win + o + l4, (lds_char*)(sm + la->obs_off) + o, 4, 0, 0);
    }
  }
  const double r_diag = tid < nv ? a.r[tid % m] : 0.0;      // diagonal of R for the Hessian (element tid of its first round)
  const double r_bq0 = tid < nr ? a.bq0[tid] : 0.0;         // constant right-hand sides (first round of the loop below)
  ColDesc cd0 = {};
  const bool pre0 = a.has_basis && tid < a.basis.nfull;
  if (pre0) cd0 = a.basis.cols[tid];
  // warm start: the previous step's active set - its size and row ids are requested here, the rows' (sparse) entries, whose
  // addresses need the ids, behind the barrier that publishes the host words (the ids have arrived by then): both round trips hide behind
  // the host words and the lift, and no wait for an ordinary load stands between the LDS-DMA requests and that barrier (hipcc
  // drains the whole vector-memory counter at such a wait while an LDS-DMA is in flight)
  int warm_q0 = 0, warm_row = 0;
  double warm_val[QP_KLDS];
  int warm_col[QP_KLDS];
#pragma unroll
  for (int k = 0; k < QP_KLDS; ++k) { warm_val[k] = 0.0; warm_col[k] = 0; }
  if (WARM && a.warm && tid < nv) warm_row = a.warm[1 + tid];      // (the set's size is wave-uniform: the compiler would wait for it at once)
  {
    // P | PB (constants of the model that every step reads once, 55 KB at N = 84) go to LDS by LDS-DMA while the host words
    // are on their way: no registers, nothing to wait for before the barrier below (hipcc drains vmcnt there)
    if (!SIM && a.stage_off) {            // (SIM: staged once, before the loop's first step)
      typedef __attribute__((address_space(3))) char lds_char;
      typedef __attribute__((address_space(1))) const char glb_char;
      lds_char* dst = (lds_char*)(sm + a.stage_off);
      glb_char* src = (glb_char*)a.P;
      const int wbase = (tid & ~63) * 16, lane16 = (tid & 63) * 16;
      for (int o = wbase; o < a.stage_doubles * 8; o += 256 * 16)       // wave-uniform LDS base; each lane its own 16 source bytes
        __builtin_amdgcn_global_load_lds(src + o + lane16, dst + o, 16, 0, 0);
    }
  }
  int status = 0;
  // lifted horizon along an input sequence x = [u_0; u_1; ...] (Kmpc.m:891-895)
  auto lifted_horizon = [&](const double* x) {
    if (tid < 64) {
      for (int c = tid; c < N; c += 64) zh[c] = z[c];
    }
    __syncthreads();
    for (int j = 0; j < Np; ++j) {
      const double* zj = zh + (size_t)j * N;
      for (int e = tid; e < N; e += 256) {
        double s = 0.0;
        for (int c = 0; c < N; ++c) s += a.A[e + (size_t)c * N] * zj[c];
        for (int i = 0; i < m; ++i) {
          const double* Bi = a.B + (size_t)i * N * N;
          double t = 0.0;
          for (int c = 0; c < N; ++c) t += Bi[e + (size_t)c * N] * zj[c];
          s += t * x[j * m + i];
        }
        zh[(size_t)(j + 1) * N + e] = s;
      }
      __syncthreads();
    }
  };
    // every LDS-DMA above (global_load ... lds) must have landed before another wave reads those bytes: that is the vector-memory
    // counter, which a workgroup-scope __syncthreads() is NOT obliged to wait for (one hipcc build lowered it to
    // `s_waitcnt lgkmcnt(0); s_barrier`) - so the wait is written out
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (WARM && a.warm) warm_q0 = a.warm[0];
    if (WARM && a.warm && a.ell.K <= QP_KLDS) {
#pragma unroll
      for (int k = 0; k < QP_KLDS; ++k) {
        warm_val[k] = (tid < nv && k < a.ell.K) ? a.ell.val[k * nr + warm_row] : 0.0;
        warm_col[k] = (tid < nv && k < a.ell.K) ? a.ell.col[k * nr + warm_row] : 0;
      }
    }
    if (stamps && tid == 0) stamps[10] = wall_clock64();      // host words and staged constants have landed
  // ---- load estimate of the observation window (Kmpc.m:1298-1356 / :1360-1444) ----
  double* xw = nullptr;   // [1; w]
  bool obs_fail = false;
  if constexpr (LOADED) {
    obs_fail = mpc_load_observer(a, *la, sm + la->obs_off, xw);
    if (obs_fail) {       // (uniform) the estimator's QP failed: NaN everywhere, as a failed step
      for (int e = tid; e < nv; e += 256) a.U[(size_t)pb * nv + e] = __builtin_nan("");
      if (a.z_out)
        for (int c = tid; c < N; c += 256) a.z_out[(size_t)pb * N + c] = __builtin_nan("");
      if (a.qp_export) {  // (state-bound steps: the generic QP kernel that follows sees NaN data, never a stale problem)
        double* ex = a.qp_export + (size_t)pb * (nv * nv + nv + nr);
        for (int e = tid; e < nv * nv + nv + nr; e += 256) ex[e] = __builtin_nan("");
      }
      mpc_step_finish(a, pb, tid, 1, stamps);
      return 1;
    }
  }
  // ---- lifted state (Kmpc.m:842; loaded: Kmpc.m:839-840, Ksysid.m:1606-1612) ----
  if (a.has_basis) {
    const BasisDev& b = a.basis;
    const double* zeta = z;
    for (int c = tid; c < b.nfull; c += 256) {
      const ColDesc cd = c == tid ? cd0 : b.cols[c];
      double v;
      if (cd.kind == COL_MONO && b.nvars <= 8) {
        // the exponent bytes come with the descriptor (kp_eval_col fetches them one by one between branches: a dependent L2
        // round trip per variable, 6.7 us for this phase at 6 variables)
        int ex[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) ex[i] = ((uint32_t)(i < 4 ? cd.aux : cd.pad) >> (8 * (i & 3))) & 0xff;
        v = 1.0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const double x = zeta[i < b.nvars ? i : 0];
          for (int k = 0; k < ex[i]; ++k) v *= x;
        }
      } else {
        v = kp_eval_col(b, cd, zeta, 1);
      }
      full[c] = v;
    }
    wg_lds_barrier();
    if constexpr (LOADED) {
      const LoadLayout L = load_layout(la->nw, la->nobs, b.nzeta, m, b.nfull, b.N);
      double* psi = sm + la->obs_off + L.psi;   // (the window's psi rows are dead)
      for (int c = tid; c < b.N; c += 256) psi[c] = mpc_psi_entry(b, zeta, full, c);
      wg_lds_barrier();
      for (int c = tid; c < N; c += 256) {
        const int l = c / b.N, j = c - l * b.N;
        z[c] = l == 0 ? psi[j] : xw[l] * psi[j];
      }
    } else {
      for (int c = tid; c < N; c += 256) {
        double v;
        if (b.k_pcs == 0)
          v = full[c];
        else if (c < b.nvars)
          v = zeta[c];
        else if (c < b.nvars + b.k_pcs) {
          const double* pc = b.pcs + (size_t)(c - b.nvars) * b.nfull;
          v = 0.0;
          for (int i = 0; i < b.nfull; ++i) v += pc[i] * full[i];
        } else
          v = 1.0;
        z[c] = v;
      }
    }
  }
  wg_lds_barrier();
  if (stamps && tid == 0) stamps[11] = wall_clock64();        // lifted state
  if (a.z_out)
    for (int c = tid; c < N; c += 256) a.z_out[(size_t)pb * N + c] = z[c];

  // constraint right-hand side: b = c (E = 0 without state bounds, Kmpc.m:862) and the
  // "memory" rows +-u_0 <= +-u_prev (Kmpc.m:865-870)
  for (int e = tid; e < nr; e += 256) {
    double v = e == tid ? r_bq0 : a.bq0[e];
    int k = e - (nr - 2 * m);
    if (k >= 0) v = k < m ? f[k] : -f[k - m];
    bq[e] = v;
  }
  // e_i = P_i z - Yr_i
  auto track_err = [&](auto Pp) {          // (Pp: P in global memory or its LDS copy - two instantiations, no generic pointer)
    for (int e4 = tid; e4 < (Np + 1) * nproj * 4; e4 += 256) {   // each dot product split over 4 lanes
      int e = e4 >> 2, part = e4 & 3;
      int i = e / nproj, p = e % nproj;
      auto Pi = Pp + (size_t)i * nproj * N;
      double s = 0.0;
#pragma unroll 4
      for (int j = part; j < N; j += 4) s += Pi[p + j * nproj] * z[j];
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      if (part == 0) ev[e] = s - ev[e];
    }
  };
  if (a.stage_off) track_err(sm + a.stage_off);
  else track_err(a.P);
  if (stamps && tid == 0) stamps[1] = wall_clock64();
  int iter0 = 0;
  if (a.U_lin) {                         // (uniform) a later pass of a state-bound step: linearise along the previous solution
    __syncthreads();
    lifted_horizon(a.U_lin + (size_t)pb * nv);
    iter0 = 1;
  }
  for (int iter = iter0; iter < iter0 + a.iters; ++iter) {
    // ---- S_k = P_k * Beta(z_k)  (get_costB_bilinear, Kmpc.m:578-585: block i uses z(i,:) when a
    // horizon of lifted states is given, else z) ----
    if (stamps && tid == 0) stamps[6] = wall_clock64();        // (what precedes is the loop's hoisted address arithmetic)
    if (a.model_type == KP_MODEL_BILINEAR) {
      for (int k = 0; k < Np; ++k) {
        const double* zk = iter == 0 ? z : zh + (size_t)k * N;
        if (iter == 0 && k > 0) break;   // same z for every block: one pass over all of them
        int k0 = k, k1 = iter == 0 ? Np : k + 1;
        auto s_rows = [&](auto PBp) {
          for (int e4 = tid; e4 < (k1 - k0) * nproj * m * 4; e4 += 256) {
            const int e = k0 * nproj * m + (e4 >> 2), part = e4 & 3;
            auto row = PBp + (size_t)e * N;        // row p of P_k B_i, contiguous: four lanes share a dot product
            double s = 0.0;
#pragma unroll 8
            for (int j = part; j < N; j += 4) s += row[j] * zk[j];
            s += __shfl_xor(s, 1, 64);
            s += __shfl_xor(s, 2, 64);
            if (part == 0) S[e] = s;
          }
        };
        if (a.stage_off) s_rows(sm + a.stage_off + (a.PB - a.P));
        else s_rows(a.PB);
      }
    } else {
      for (int e = tid; e < Np * nproj * m; e += 256) S[e] = a.S0[e];
    }
    wg_lds_barrier();
    if (stamps && tid == 0) stamps[2] = wall_clock64();
    // ---- Hq = 2 (CB'Q CB + R),  f = 2 CB'Q e   (Kmpc.m:604,879,883) ----
    // With Sall = [S_0 S_1 ... S_{Np-1}] (nproj x nv: block k, input a is column k m + a) the blocks of CB_i are columns of Sall,
    // so every term of H is an entry of the Gram matrix T = Sall' Sall, and H(r1, r2) walks down one diagonal of it:
    //   H(j1 m + a1, j2 m + a2) = 2 sum_{t < Np - j2} q_{j2 + 1 + t} T((j2 - j1 + t) m + a1, t m + a2)        (j2 >= j1).
    // Stage 1 forms T once (nv (nv / 2 + 1) short dot products, into the solver's scratch, which is free until H^-1), stage 2
    // is one LDS read and one multiply-add per term - the direct form recomputed every T entry up to Np times inside a
    // doubly nested loop of dependent LDS round trips (4.5 us of a 34 us step).  Same terms in the same order: same bits.
    // Both stages use symmetry: the pairs {r, (r + d) mod nv}, d = 0 .. nv / 2, cover the upper triangle (the last d twice
    // when nv is even: the same value stored twice); small quotients by a float reciprocal with one correction (a 32-bit
    // integer division is ~35 instructions).
    {
      const float rnv = 1.0f / (float)nv, rmf = 1.0f / (float)m;
      auto divmod = [](int x, int d, float rd, int& q, int& r) {
        q = (int)((float)x * rd);
        r = x - q * d;
        if (r < 0) { r += d; --q; }
        if (r >= d) { r -= d; ++q; }
      };
      double* Tm = qpws;
      // The loops below fetch the operands of FOUR terms (and of all nproj products of a term) before they use the first: a
      // loop that reads, waits, adds and branches per term is a chain of LDS round trips (~130 cycles each, ten per element).
      // Indices past the end are clamped (the reads stay inside the arrays), the sums take only the valid terms, in order.
      auto stage1 = [&](auto NPc) {
        constexpr int NP = decltype(NPc)::value;          // nproj (0: any)
        for (int e = tid; e < nv * (nv / 2 + 1); e += 256) {
          int d, i0;
          divmod(e, nv, rnv, d, i0);
          int jx = i0 + d;
          if (jx >= nv) jx -= nv;
          const int c1 = min(i0, jx), c2 = max(i0, jx);
          const double* S1 = S + c1 * nproj;
          const double* S2 = S + c2 * nproj;
          double t = 0.0;
          if constexpr (NP > 0) {
            double x1[NP], x2[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) { x1[p] = S1[p]; x2[p] = S2[p]; }
#pragma unroll
            for (int p = 0; p < NP; ++p) t += x1[p] * x2[p];
          } else {
            for (int p = 0; p < nproj; ++p) t += S1[p] * S2[p];
          }
          Tm[c1 + c2 * nv] = t;
          Tm[c2 + c1 * nv] = t;
        }
        // f = 2 CB'Q e by the LAST threads (they have the fewest elements of the two H rounds)
        for (int e = 255 - tid; e < nv; e += 256) {
          int j, a1;
          divmod(e, m, rmf, j, a1);
          double s = 0.0;
          if constexpr (NP > 0) {
            const int cnt = Np - j, last = cnt - 1;
            const double* S0 = S + a1 * nproj;               // column a1 of S_0; term t uses S_t and e_{j + 1 + t}
            const double* e0 = ev + (j + 1) * nproj;
            for (int t0 = 0; t0 < cnt; t0 += 4) {
              double xs[4][NP], xe[4][NP];
#pragma unroll
              for (int u = 0; u < 4; ++u) {
                const int tt = min(t0 + u, last);
#pragma unroll
                for (int p = 0; p < NP; ++p) { xs[u][p] = S0[tt * nproj * m + p]; xe[u][p] = e0[tt * nproj + p]; }
              }
#pragma unroll
              for (int u = 0; u < 4; ++u) {
                double t = 0.0;
#pragma unroll
                for (int p = 0; p < NP; ++p) t += xs[u][p] * xe[u][p];
                if (t0 + u < last) s += a.q_run * t;
                else if (t0 + u == last) s += a.q_term * t;
              }
            }
          } else {
            for (int i = j + 1; i <= Np; ++i) {
              double qi = i == Np ? a.q_term : a.q_run;
              const double* S1 = S + (i - j - 1) * nproj * m + a1 * nproj;
              double t = 0.0;
              for (int p = 0; p < nproj; ++p) t += S1[p] * ev[i * nproj + p];
              s += qi * t;
            }
          }
          f[e] = 2.0 * s;
        }
      };
      switch (nproj) {
        case 1: stage1(std::integral_constant<int, 1>()); break;
        case 2: stage1(std::integral_constant<int, 2>()); break;
        case 3: stage1(std::integral_constant<int, 3>()); break;
        case 4: stage1(std::integral_constant<int, 4>()); break;
        default: stage1(std::integral_constant<int, 0>()); break;
      }
      wg_lds_barrier();
      const int dstride = m * (nv + 1);
      for (int e = tid; e < nv * (nv / 2 + 1); e += 256) {
        int d, i0;
        divmod(e, nv, rnv, d, i0);
        int jx = i0 + d;
        if (jx >= nv) jx -= nv;
        const int r1 = min(i0, jx), r2 = max(i0, jx);
        int j1, a1, j2, a2;
        divmod(r1, m, rmf, j1, a1);
        divmod(r2, m, rmf, j2, a2);
        const double* tp = Tm + ((j2 - j1) * m + a1) + a2 * nv;      // T(S_{i-j1-1} column a1, S_{i-j2-1} column a2) at i = j2 + 1
        const int cnt = Np - j2, last = cnt - 1;
        double s = 0.0;
        for (int t0 = 0; t0 < cnt; t0 += 4) {
          double v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] = tp[min(t0 + u, last) * dstride];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            if (t0 + u < last) s += a.q_run * v[u];
            else if (t0 + u == last) s += a.q_term * v[u];
          }
        }
        if (r1 == r2) s += (e == tid && tid < nv) ? r_diag : a.r[a1];
        Hq[r1 + r2 * nv] = 2.0 * s;
        Hq[r2 + r1 * nv] = 2.0 * s;
      }
    }
    wg_lds_barrier();
    if (a.qp_export) {
      double* ex = a.qp_export + (size_t)pb * (nv * nv + nv + nr);
      for (int e = tid; e < nv * nv; e += 256) ex[e] = Hq[e];
      for (int e = tid; e < nv; e += 256) ex[nv * nv + e] = f[e];
      for (int e = tid; e < nr; e += 256) ex[nv * nv + nv + e] = bq[e];
    }
    if (a.assemble_only) return 0;               // (uniform) H, f, b are in qp_export, z in z_out
    // ---- QP by wave 0 ----
    if (stamps && tid == 0) stamps[3] = wall_clock64();
    double* xout = SIM ? si->x : a.U + (size_t)pb * nv;
    // H^-1 by the whole workgroup into the solver's scratch (first n*n doubles).  Hq is not needed after this
    // point (the solver works from H^-1; the next linearisation pass rebuilds it), so it is the second buffer of the
    // ping-pong inverse.
    // (the solver's own single-wave inverse, have_hinv = false, measured 63 us against 38 us for the first workgroup
    //  version, 27 us for the two-barrier in-place one and 10 us for this one, nv = 30)
    const int hbad = wg_spd_inverse_pp(qpws, Hq, nv, nv, true);       // (the pair sweep reads Hq where it lies)
    if (stamps && tid == 0) stamps[12] = wall_clock64();      // H^-1
    const bool have_hinv = true;
    // warm start from the previous step's active set (closed loops change it by a few rows per step): the whole
    // workgroup forms HN = H^-1 N' and S = N H^-1 N' and inverts S; wave 0 then only has to release rows whose
    // multiplier is negative and add the newly violated ones
    int wq = 0;
    if (WARM && a.warm && !hbad) {
      if (iter != iter0) {                     // later linearisation passes start from the set the previous pass left
        warm_q0 = a.warm[0];
        if (tid < nv) warm_row = a.warm[1 + tid];
        if (a.ell.K <= QP_KLDS) {
#pragma unroll
          for (int k = 0; k < QP_KLDS; ++k) {
            warm_val[k] = (tid < nv && k < a.ell.K) ? a.ell.val[k * nr + warm_row] : 0.0;
            warm_col[k] = (tid < nv && k < a.ell.K) ? a.ell.col[k * nr + warm_row] : 0;
          }
        }
      }
      wq = min(warm_q0, nv);
      double* HNw = qpws + nv * nv;
      double* Sw = qpws + 2 * nv * nv;
      int* actw = (int*)(qpws + 3 * nv * nv + 9 * nv) + nv + (nv & 1);     // the solver's act[] (behind apv and apc)
      if (wq > 0) {
        const int K = a.ell.K;
        if (K <= QP_KLDS && 3 * QP_KLDS <= 2 * nv) {          // (the staged rows take 1.5 QP_KLDS nv doubles of Hq's nv^2)
          // rows staged in LDS (Hq is free between the two inverses): val [wq][4] | col [wq][4]; no global access and
          // no integer division in the two products (lane = row of the result, waves stride the columns)
          double* sv = Hq;
          int* sc = (int*)(Hq + QP_KLDS * nv);
          if (tid < wq) {
            actw[tid] = warm_row;
#pragma unroll
            for (int k = 0; k < QP_KLDS; ++k) {
              sv[tid * QP_KLDS + k] = warm_val[k];
              sc[tid * QP_KLDS + k] = warm_col[k];
            }
          }
          wg_lds_barrier();
          // lane = row of the result, groups of 32 (nv <= 32) or 64 lanes stride the columns; always QP_KLDS terms (the
          // entries behind a row's last one are 0 * column 0), so the reads of a sum do not wait for each other and
          // two columns are in flight per thread - the loops over a run-time K were chains of dependent LDS round trips
          const int RL = nv <= 32 ? 32 : 64, NG = 256 / RL;
          const int li_ = tid & (RL - 1), cg = tid / RL;
          if (li_ < nv) {
#pragma unroll 2
            for (int c = cg; c < wq; c += NG) {
              double v4[QP_KLDS], h4[QP_KLDS];
#pragma unroll
              for (int k = 0; k < QP_KLDS; ++k) {
                v4[k] = sv[c * QP_KLDS + k];
                h4[k] = qpws[li_ + sc[c * QP_KLDS + k] * nv];
              }
              double sacc = 0.0;
#pragma unroll
              for (int k = 0; k < QP_KLDS; ++k) sacc += v4[k] * h4[k];
              HNw[li_ + c * nv] = sacc;
            }
          }
          wg_lds_barrier();
          if (li_ < wq) {
            double v4[QP_KLDS];
            int c4[QP_KLDS];
#pragma unroll
            for (int k = 0; k < QP_KLDS; ++k) {
              v4[k] = sv[li_ * QP_KLDS + k];
              c4[k] = sc[li_ * QP_KLDS + k];
            }
#pragma unroll 2
            for (int c2 = cg; c2 < wq; c2 += NG) {
              double h4[QP_KLDS];
#pragma unroll
              for (int k = 0; k < QP_KLDS; ++k) h4[k] = HNw[c4[k] + c2 * nv];
              double sacc = 0.0;
#pragma unroll
              for (int k = 0; k < QP_KLDS; ++k) sacc += v4[k] * h4[k];
              Sw[li_ + c2 * nv] = sacc;
            }
          }
          wg_lds_barrier();
        } else {
          for (int c = tid; c < wq; c += 256) actw[c] = a.warm[1 + c];
          __syncthreads();
          for (int e = tid; e < nv * wq; e += 256) {
            const int i = e % nv, c = e / nv, row = actw[c];
            double sacc = 0.0;
            for (int k = 0; k < K; ++k) sacc += a.ell.val[k * nr + row] * qpws[i + a.ell.col[k * nr + row] * nv];
            HNw[i + c * nv] = sacc;
          }
          __syncthreads();
          for (int e = tid; e < wq * wq; e += 256) {
            const int c = e % wq, c2 = e / wq, row = actw[c];
            double sacc = 0.0;
            for (int k = 0; k < K; ++k) sacc += a.ell.val[k * nr + row] * HNw[a.ell.col[k * nr + row] + c2 * nv];
            Sw[c + c2 * nv] = sacc;
          }
          __syncthreads();
        }
        if (stamps && tid == 0) stamps[13] = wall_clock64();  // H^-1 N', N H^-1 N'
        if (wg_spd_inverse_pp(Sw, Hq, wq, nv)) wq = 0;   // dependent rows: cold start
        if (stamps && tid == 0) stamps[14] = wall_clock64();  // its inverse
      }
    }
    // single-problem launches: the iteration by all four waves (12 % faster cold solves; in the batched kernel it would
    // cost the third workgroup per CU and is slower: 1.64 against 1.27 ms per 4096 problems)
    if (WARM && a.qp_wg && nv <= 32 && a.ell.K <= QP_KLDS) {
      const int st = qp_gi_wg(f, a.ell, bq, nv, nr, qpws, qpws + qp_lds_doubles(nv, nr) - 64, xout, 1e-10, stamps, hbad, wq,
                              WARM ? a.warm : nullptr);
      if (tid == 0) *st_sh = st;
    } else if (tid < 64) {
      int st = WARM ? qp_goldfarb_idnani(Hq, f, a.ell, bq, nv, nr, qpws, xout, 1e-10, stamps, have_hinv, hbad, wq, a.warm)
                    : qp_goldfarb_idnani(Hq, f, a.ell, bq, nv, nr, qpws, xout, 1e-10, stamps, have_hinv, hbad);
      if (tid == 0) *st_sh = st;
    }
    // the other waves wait here (the solver itself only uses wave-local synchronisation)
    __syncthreads();
    if (stamps && tid == 0) stamps[5] = wall_clock64();
    status = *st_sh;
    if (status || iter == iter0 + a.iters - 1) break;
    // ---- lifted horizon for the next linearisation (Kmpc.m:891-895) ----
    lifted_horizon(xout);
  }
  if (tid == 0) a.status[pb] = status ? KP_ERR_QP_FAIL : KP_OK;
  if (a.done_flag && pb == 0) {
    // single zero-copy step: tell the spinning host thread that U, z and the status are in its memory.  Every wave has
    // waited for its stores at the barrier; lane 0 then releases at system scope and stores the sequence number.
    __syncthreads();
    if (tid == 0) {
      __threadfence_system();
      if (stamps) { a.done_flag[1] = (unsigned long long)stamps[0]; a.done_flag[2] = (unsigned long long)wall_clock64(); }
      __threadfence_system();
      __hip_atomic_store(&a.done_flag[0], a.done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  return status;
}

// Two entry points over the same body: the single-problem kernel (warm start, workgroup-wide solver) may use every register
// it likes; the batched one is held to 128 so that FOUR workgroups share a CU (with a.alias their LDS fits).
template <bool WARM>
__global__ __launch_bounds__(256) void kp_mpc_step_kernel(MpcArgs a) {
  mpc_step_body<WARM>(a);
}
template <bool WARM>
__global__ __launch_bounds__(256) void kp_mpc_step_loaded_kernel(MpcArgs a, MpcLoadArgs l) {
  mpc_step_body<WARM, true>(a, &l);
}
__global__ __launch_bounds__(256, 4) void kp_mpc_step_batch_kernel(MpcArgs a) {
  mpc_step_body<false>(a);
}

// ---- whole closed loops with the model as the plant (kp_mpc_simulate; the loop's contract: kp_sim_loop.h) ---------------
// The step is the QP step of kp_mpc_step_zeta: lift of Y[k-1], then the solve against the reference window.  The plant step
// is Y[k] = (A z + B u_prev)[0:n] or (A z + sum_i u_prev,i B_i z)[0:n] (C = [I 0], and only those n rows are ever read: the
// next step lifts Y[k] again).  Z rows are the lifted states.
// Everything the loop carries lives in LDS behind the step's own block, at sim_off (offsets in doubles, each even):
//   y n | u m | x nvar | ab (m + 1) n partial products of the model step | the padded reference ((nref + Np) nproj) | warm
//   1 + nvar ints: the trial's own optimal active set of the previous step | the dictionary's column descriptors | then
//   P | PB at stage_off.
// r and bq0 (m + nrows doubles) stay in global memory: a step asks for them with its first instructions and uses them
// after the lift, as a single step does - nothing waits for them.
// The step body takes these by plain LDS reads (its SIM mode): nothing that a step wrote is read through LDS-DMA.
struct SimLayout {
  int y, u, x, ab, ref, warm, cols, total;
};
__host__ __device__ inline SimLayout sim_layout(int n, int m, int nv, int nproj, int Np, int nref, int nfull) {
  SimLayout L;
  int o = 0;
  L.y = o; o += even_up(n);
  L.u = o; o += even_up(m);
  L.x = o; o += even_up(nv);
  L.ab = o; o += even_up((m + 1) * n);
  L.ref = o; o += even_up((nref + Np) * nproj);
  L.warm = o; o += even_up((1 + nv + 1) / 2);
  L.cols = o; o += 2 * nfull;               // ColDesc: 16 bytes
  L.total = o;
  return L;
}
struct MpcSimArgs {
  KpSimLoop loop;                   // (ny = n = the dictionary's nzeta, aux = Z, aux_w = N)
  int sim_off;
};
__global__ __launch_bounds__(256) void kp_mpc_sim_kernel(MpcArgs a, MpcSimArgs sa) {
  extern __shared__ __align__(16) double sm[];
  const int tid = threadIdx.x;
  const KpSimLoop& S = sa.loop;
  const int N = a.N, m = a.m, Np = a.Np, nproj = a.nproj, nv = a.nvar, n = S.ny, nref = S.nref;
  const int nfull = a.basis.nfull;
  const SimLayout L = sim_layout(n, m, nv, nproj, Np, nref, nfull);
  double* sb = sm + sa.sim_off;
  double* y = sb + L.y;
  double* u = sb + L.u;
  double* ab = sb + L.ab;
  double* refl = sb + L.ref;
  int* warm = (int*)(sb + L.warm);
  ColDesc* cols = (ColDesc*)(sb + L.cols);
  // ---- once per trial: what is constant over the run, the staged reference and row 0 ----
  if (a.stage_off) {          // P | PB by LDS-DMA, as a single step stages it
    typedef __attribute__((address_space(3))) char lds_char;
    typedef __attribute__((address_space(1))) const char glb_char;
    lds_char* dst = (lds_char*)(sm + a.stage_off);
    glb_char* src = (glb_char*)a.P;
    const int wbase = (tid & ~63) * 16, lane16 = (tid & 63) * 16;
    for (int o = wbase; o < a.stage_doubles * 8; o += 256 * 16)
      __builtin_amdgcn_global_load_lds(src + o + lane16, dst + o, 16, 0, 0);
  }
  const KpSimRows T = kp_sim_prologue(S, refl, y, u);
  for (int e = tid; e < nfull; e += 256) cols[e] = a.basis.cols[e];
  // cold first step: an empty set - and row ids of 0 behind it: a step asks for the constraint rows of ALL nvar ids before
  // it knows the set's size (mpc_step_body: warm_row, then ell.val[k nrows + warm_row]), and LDS starts out as garbage
  if (tid <= nv) warm[tid] = 0;             // (nvar <= 64)
  // the LDS-DMA above is counted by the vector-memory counter, which a barrier does not wait for by itself
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  MpcArgs s = a;
  s.basis.cols = cols;
  s.warm = warm;
  s.status = S.status + blockIdx.x;
  MpcSimIn si;
  si.zeta = y;
  si.up = u;
  si.x = sb + L.x;
  si.z = sm;
  const bool bil = a.model_type == KP_MODEL_BILINEAR;
  int k = 1, failed = 0;
  for (; k < nref; ++k) {
    si.yr = refl + (size_t)(k - 1) * nproj;
    s.z_out = T.aux ? T.aux + (size_t)(k - 1) * N : nullptr;
    failed = mpc_step_body<true, false, true>(s, nullptr, &si);     // (ends behind a barrier: x, z and the status are visible)
    if (failed) break;                      // (uniform)
    // model step, rows 0 .. n-1: ab[j n + r] = row r of A (j = 0) or of B_j (bilinear, j = 1 .. m) times z, four lanes each
    const double* z = si.z;
    const int nterm = (bil ? m + 1 : 1) * n;
    for (int e4 = tid; e4 < nterm * 4; e4 += 256) {
      const int e = e4 >> 2, part = e4 & 3;
      const int j = e / n, r = e - j * n;
      const double* Mr = (j == 0 ? a.A : a.B + (size_t)(j - 1) * N * N) + r;
      double t = 0.0;
      for (int c = part; c < N; c += 4) t += Mr[(size_t)c * N] * z[c];
      t += __shfl_xor(t, 1, 64);
      t += __shfl_xor(t, 2, 64);
      if (part == 0) ab[e] = t;
    }
    __syncthreads();
    double ynew = 0.0, unew = 0.0;
    if (tid < n) {                          // (n <= 256: kp_mpc_simulate)
      ynew = ab[tid];
      // (two loops where one conditional expression would do: see the compiler hazard in DESIGN 3.3h - with the single
      //  expression the hipcc of ROCm 7.2 places its copy of the LDS aperture register in VCC and stops with "Illegal
      //  instruction detected"; a build failure, never wrong code)
      if (bil)
        for (int i = 0; i < m; ++i) ynew += ab[(i + 1) * n + tid] * u[i];
      else
        for (int i = 0; i < m; ++i) ynew += a.B[tid + (size_t)i * N] * u[i];
    }
    if (tid < m) unew = si.x[m + tid];      // the second row of the solution
    __syncthreads();                        // (every read of the old u is done)
    kp_sim_commit(S, T, k, y, u, [&](int) { return ynew; }, [&](int) { return unew; });
    __syncthreads();                        // y, u and the body's arrays are free for the next step
  }
  // (a failed step wrote its z behind a barrier: the NaN tail of Z starts at its row)
  kp_sim_epilogue(S, T, k, failed, failed ? KP_ERR_QP_FAIL : KP_OK);
}

// ---- host API ------------------------------------------------------------------------------------

extern "C" int kp_mpc_destroy(kp_mpc* M) {
  if (!M) return KP_OK;
  (void)hipSetDevice(M->ctx->device);
  double* ptrs[] = {M->A, M->B, M->P, M->S0, M->r, M->Aq, M->bq0, M->Anorm, M->work, M->d_in, M->d_out};
  for (double* p : ptrs)
    if (p) (void)hipFree(p);
  if (M->h_in) (void)hipHostFree(M->h_in);
  if (M->h_out) (void)hipHostFree(M->h_out);
  if (M->h_ld) (void)hipHostFree(M->h_ld);
  if (M->warm) (void)hipFree(M->warm);
  if (M->ellc) (void)hipFree(M->ellc);
  if (M->ellv) (void)hipFree(M->ellv);
  if (M->sb_lohi) (void)hipFree(M->sb_lohi);
  if (M->sb_Apow) (void)hipFree(M->sb_Apow);
  if (M->sb_A) (void)hipFree(M->sb_A);
  if (M->sb_b) (void)hipFree(M->sb_b);
  if (M->sb_col) (void)hipFree(M->sb_col);
  if (M->sb_work) (void)hipFree(M->sb_work);
  delete M;
  return KP_OK;
}

extern "C" int kp_mpc_create(kp_ctx* ctx, int model_type, const double* A, const double* B, int N, int m, int Np,
                             const double* proj, int nproj, double q_run, double q_term, const double* r, const double* lo,
                             const double* hi, double slope_lim, double smooth_lim, kp_mpc** out) {
  if (!ctx || !out) return KP_ERR_ARG;
  *out = nullptr;
  if (!A || !B || !proj || !r || N < 1 || m < 1 || Np < 1 || nproj < 1)
    return ctx->fail(KP_ERR_ARG, "kp_mpc_create: bad argument");
  if (model_type != KP_MODEL_LINEAR && model_type != KP_MODEL_BILINEAR)
    return ctx->fail(KP_ERR_ARG, "kp_mpc_create: model_type must be linear or bilinear (NMPC is out of scope)");
  if ((lo == nullptr) != (hi == nullptr)) return ctx->fail(KP_ERR_ARG, "kp_mpc_create: lo and hi must both be given or both NULL");
  const int nvar = m * Np;
  if (nvar > QP_MAXN) return ctx->fail(KP_ERR_ARG, "kp_mpc_create: m*horizon must be <= 64");
  KP_HIP(ctx, hipSetDevice(ctx->device));
  const bool has_slope = !std::isnan(slope_lim) && Np >= 2, has_smooth = !std::isnan(smooth_lim) && Np >= 3;
  // constraint rows in the order the reference stacks them (Kmpc.m:641-730, then :865-870)
  int nb = lo ? 2 * m * (Np + 1) : 0, ns = has_slope ? 2 * m * (Np - 1) : 0, nsm = has_smooth ? 2 * m * (Np - 2) : 0;
  const int nrows = nb + ns + nsm + 2 * m;
  std::vector<double> Aq((size_t)nrows * nvar, 0.0), bq(nrows, 0.0);
  auto at = [&](int row, int col) -> double& { return Aq[(size_t)col * nrows + row]; };
  int row0 = 0;
  if (lo) {  // Fbounds: kron(I_Np, [-I; I]) in the first 2m*Np rows, last 2m rows zero (Kmpc.m:646-663)
    for (int j = 0; j < Np; ++j)
      for (int i = 0; i < m; ++i) {
        at(row0 + j * 2 * m + i, j * m + i) = -1.0;
        bq[row0 + j * 2 * m + i] = -lo[i];
        at(row0 + j * 2 * m + m + i, j * m + i) = 1.0;
        bq[row0 + j * 2 * m + m + i] = hi[i];
      }
    row0 += nb;
  }
  if (has_slope) {  // [u_{j+1} - u_j ; -(u_{j+1} - u_j)] <= slope_lim   (Kmpc.m:670-688)
    int h = m * (Np - 1);
    for (int j = 0; j < Np - 1; ++j)
      for (int i = 0; i < m; ++i) {
        int rr = j * m + i;
        at(row0 + rr, j * m + i) = -1.0;
        at(row0 + rr, (j + 1) * m + i) = 1.0;
        at(row0 + h + rr, j * m + i) = 1.0;
        at(row0 + h + rr, (j + 1) * m + i) = -1.0;
        bq[row0 + rr] = slope_lim;
        bq[row0 + h + rr] = slope_lim;
      }
    row0 += ns;
  }
  if (has_smooth) {  // u_j - 2u_{j+1} + u_{j+2}   (Kmpc.m:694-708)
    int h = m * (Np - 2);
    for (int j = 0; j < Np - 2; ++j)
      for (int i = 0; i < m; ++i) {
        int rr = j * m + i;
        at(row0 + rr, j * m + i) = 1.0;
        at(row0 + rr, (j + 1) * m + i) = -2.0;
        at(row0 + rr, (j + 2) * m + i) = 1.0;
        at(row0 + h + rr, j * m + i) = -1.0;
        at(row0 + h + rr, (j + 1) * m + i) = 2.0;
        at(row0 + h + rr, (j + 2) * m + i) = -1.0;
        bq[row0 + rr] = smooth_lim;
        bq[row0 + h + rr] = smooth_lim;
      }
    row0 += nsm;
  }
  for (int i = 0; i < m; ++i) {  // memory rows (Kmpc.m:865): [I; -I] on u_0
    at(row0 + i, i) = 1.0;
    at(row0 + m + i, i) = -1.0;
  }
  kp_mpc* M = new kp_mpc();
  M->ctx = ctx;
  M->model_type = model_type;
  M->N = N; M->m = m; M->Np = Np; M->nproj = nproj; M->nvar = nvar; M->nrows = nrows;
  M->mb = model_type == KP_MODEL_BILINEAR ? N * m : m;
  M->q_run = q_run; M->q_term = q_term;
  int rc = kp_dev_alloc_copy(ctx, &M->A, A, (size_t)N * N);
  if (!rc) rc = kp_dev_alloc_copy(ctx, &M->B, B, (size_t)N * M->mb);
  // P | PB in ONE allocation (PB at an even offset), padded to a multiple of 4 KB: a single-problem step copies the block
  // to LDS with 1 KB loads per wave
  const size_t nP = ((size_t)(Np + 1) * nproj * N + 1) & ~(size_t)1;
  const size_t nPB = model_type == KP_MODEL_BILINEAR ? (size_t)Np * nproj * m * N : 0;
  M->stage_doubles = (int)((nP + nPB + 511) & ~(size_t)511);
  if (!rc) rc = kp_dev_alloc_copy(ctx, &M->P, nullptr, (size_t)M->stage_doubles);
  if (!rc && nPB) M->PB = M->P + nP;
  if (!rc) rc = kp_dev_alloc_copy(ctx, &M->S0, nullptr, (size_t)Np * nproj * m);
  if (!rc) rc = kp_dev_alloc_copy(ctx, &M->r, r, m);
  if (!rc) rc = kp_dev_alloc_copy(ctx, &M->Aq, Aq.data(), Aq.size());
  if (!rc) rc = kp_dev_alloc_copy(ctx, &M->bq0, bq.data(), nrows);
  std::vector<double> ev, en;
  std::vector<int> ec;
  to_ell(Aq.data(), nrows, nvar, ev, ec, en, M->ellK);
  if (!rc) rc = kp_dev_alloc_copy(ctx, &M->Anorm, en.data(), nrows);
  if (!rc) rc = kp_dev_alloc_copy(ctx, &M->ellv, ev.data(), ev.size());
  if (!rc) {
    hipError_t e2 = hipMalloc((void**)&M->ellc, ec.size() * 4);
    if (e2 == hipSuccess) e2 = hipMemcpy(M->ellc, ec.data(), ec.size() * 4, hipMemcpyHostToDevice);
    if (e2 != hipSuccess) rc = ctx->fail(KP_ERR_HIP, std::string("kp_mpc_create: ") + hipGetErrorString(e2));
  }
  double* dproj = nullptr;
  if (!rc) rc = kp_dev_alloc_copy(ctx, &dproj, proj, (size_t)nproj * N);
  if (rc) {
    if (dproj) (void)hipFree(dproj);
    kp_mpc_destroy(M);
    return rc;
  }
  hipLaunchKernelGGL(kp_mpc_setup_kernel, dim3(1), dim3(256), 0, ctx->stream, M->A, M->B, dproj, N, m, Np, nproj,
                     model_type == KP_MODEL_LINEAR ? 1 : 0, M->P, M->S0, M->PB);
  hipError_t e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(dproj);
  if (e != hipSuccess) {
    kp_mpc_destroy(M);
    return ctx->fail(KP_ERR_HIP, std::string("kp_mpc_create: ") + hipGetErrorString(e));
  }
  *out = M;
  return KP_OK;
}

extern "C" int kp_mpc_dims(const kp_mpc* M, int* nvar, int* nrows) {
  if (!M) return KP_ERR_ARG;
  if (nvar) *nvar = M->nvar;
  if (nrows) *nrows = M->nrows;
  return KP_OK;
}

// ---- state bounds (Kmpc.m:300-318, :716-730) -----------------------------------------------------------------------
// The reference bounds the entries s = i n + j (block i = 0..Np, j < n) of the STACKED lifted state [z_0; z_1; ...]
// (the kron block of E is written into its first (Np+1) n columns, :306 - not strided by N; restated literally, as the
// oracle does): entry s belongs to step k = s / N, component c = s % N, so
//   (Ahat z)_s = (A^k z)_c,   (Bhat U)_s = sum_{j < k} (A^(k-1-j) Bz)_c,: u_j,   Bz = Beta(z) (bilinear) or B (linear),
// rows  -(Bhat U)_s <= -lo_j + (Ahat z)_s  and  (Bhat U)_s <= hi_j - (Ahat z)_s.  These rows are dense in U and, for a
// bilinear model, change with z: kp_mpc_sb_kernel writes the whole constraint matrix of the step densely (the constant
// sparse rows expanded, then the state-bound rows) and the generic QP kernel solves with it.
__global__ void kp_matmul_nn_kernel(const double* __restrict__ X, const double* __restrict__ Y, int N, double* __restrict__ Z) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N * N) return;
  const int i = e % N, j = e / N;
  double s = 0.0;
  for (int k = 0; k < N; ++k) s += X[i + (size_t)k * N] * Y[k + (size_t)j * N];
  Z[e] = s;
}

__global__ __launch_bounds__(256) void kp_mpc_sb_kernel(int model_type, int N, int m, int Np, int nvar, int nrows, int n_sb, int kmax,
                                                        const double* __restrict__ Apow, const double* __restrict__ B,
                                                        const double* __restrict__ Aq, const double* __restrict__ b_in,
                                                        const double* __restrict__ z, const double* __restrict__ lohi,
                                                        double* __restrict__ Ad, double* __restrict__ bd, double* __restrict__ nrm,
                                                        size_t b_stride) {
  extern __shared__ double sm[];
  double* Bz = sm;                         // N x m
  double* zs = Bz + N * m;                 // N
  const int tid = threadIdx.x;
  const int mr = nrows + 2 * n_sb * (Np + 1);
  {                                        // problem p = blockIdx.x of a batch
    const size_t p = blockIdx.x;
    b_in += p * b_stride; z += p * N;
    Ad += p * (size_t)mr * nvar; bd += p * mr; nrm += p * mr;
  }
  for (int c = tid; c < N; c += 256) zs[c] = z[c];
  __syncthreads();
  for (int e = tid; e < N * m; e += 256) {
    const int r = e % N, i = e / N;
    double s;
    if (model_type == KP_MODEL_BILINEAR) {
      s = 0.0;
      const double* Bi = B + (size_t)i * N * N;
      for (int c = 0; c < N; ++c) s += Bi[r + (size_t)c * N] * zs[c];
    } else {
      s = B[r + (size_t)i * N];
    }
    Bz[e] = s;
  }
  __syncthreads();
  // constant rows: expanded copy
  for (int e = tid; e < nrows * nvar; e += 256) {
    const int r = e % nrows, v = e / nrows;
    Ad[r + (size_t)v * mr] = Aq[e];
  }
  for (int r = tid; r < nrows; r += 256) bd[r] = b_in[r];
  // state-bound rows: one (stacked entry, variable) pair per thread and pass
  const int nst = n_sb * (Np + 1);
  for (int e = tid; e < nst * nvar; e += 256) {
    const int st = e % nst, v = e / nst;            // stacked entry, variable v = jj * m + ii
    const int blk = st / n_sb, j = st % n_sb;
    const int k = st / N, c = st % N;
    const int jj = v / m, ii = v % m;
    double val = 0.0;
    if (jj < k) {
      const double* Ap = Apow + (size_t)(k - 1 - jj) * N * N;       // row c of A^(k-1-jj)
      for (int r = 0; r < N; ++r) val += Ap[c + (size_t)r * N] * Bz[r + ii * N];
    }
    const int rneg = nrows + blk * 2 * n_sb + j, rpos = rneg + n_sb;
    Ad[rneg + (size_t)v * mr] = -val;
    Ad[rpos + (size_t)v * mr] = val;
  }
  for (int st = tid; st < nst; st += 256) {
    const int blk = st / n_sb, j = st % n_sb;
    const int k = st / N, c = st % N;
    const double* Ap = Apow + (size_t)k * N * N;
    double az = 0.0;
    for (int r = 0; r < N; ++r) az += Ap[c + (size_t)r * N] * zs[r];
    const int rneg = nrows + blk * 2 * n_sb + j, rpos = rneg + n_sb;
    bd[rneg] = -lohi[j] + az;
    bd[rpos] = lohi[n_sb + j] - az;
  }
  __syncthreads();
  __threadfence_block();
  for (int r = tid; r < mr; r += 256) {             // row norms (the solver scales violations by them)
    double s = 0.0;
    for (int v = 0; v < nvar; ++v) {
      const double a = Ad[r + (size_t)v * mr];
      s += a * a;
    }
    nrm[r] = sqrt(s);
  }
}

extern "C" int kp_mpc_set_state_bounds(kp_mpc* M, int n, const double* lo, const double* hi) {
  if (!M) return KP_ERR_ARG;
  kp_ctx* ctx = M->ctx;
  if (n < 0 || n > M->N || (n > 0 && (!lo || !hi))) return ctx->fail(KP_ERR_ARG, "kp_mpc_set_state_bounds: bad argument");
  KP_HIP(ctx, hipSetDevice(ctx->device));
  double** bufs[] = {&M->sb_lohi, &M->sb_Apow, &M->sb_A, &M->sb_b, &M->sb_work};
  for (double** p : bufs)
    if (*p) { (void)hipFree(*p); *p = nullptr; }
  M->sb_cap = 0;
  if (M->sb_col) { (void)hipFree(M->sb_col); M->sb_col = nullptr; }
  M->sb_n = 0; M->sb_rows = 0;
  if (n == 0) return KP_OK;
  const int N = M->N, Np = M->Np, nv = M->nvar;
  const int kmax = ((Np + 1) * n - 1) / N;
  const int mr = M->nrows + 2 * n * (Np + 1);
  std::vector<double> lh(2 * n);
  for (int i = 0; i < n; ++i) { lh[i] = lo[i]; lh[n + i] = hi[i]; }
  int rc = kp_dev_alloc_copy(ctx, &M->sb_lohi, lh.data(), lh.size());
  if (rc) return rc;
  KP_HIP(ctx, hipMalloc((void**)&M->sb_Apow, (size_t)(kmax + 1) * N * N * 8));
  std::vector<double> eye((size_t)N * N, 0.0);
  for (int i = 0; i < N; ++i) eye[(size_t)i * N + i] = 1.0;
  KP_HIP(ctx, hipMemcpy(M->sb_Apow, eye.data(), (size_t)N * N * 8, hipMemcpyHostToDevice));
  for (int p = 1; p <= kmax; ++p) {
    hipLaunchKernelGGL(kp_matmul_nn_kernel, dim3((N * N + 255) / 256), dim3(256), 0, ctx->stream, M->sb_Apow + (size_t)(p - 1) * N * N, M->A, N,
                       M->sb_Apow + (size_t)p * N * N);
    KP_HIP(ctx, hipGetLastError());
  }
  std::vector<int> col((size_t)mr * nv);
  for (int k = 0; k < nv; ++k)
    for (int r = 0; r < mr; ++r) col[(size_t)k * mr + r] = k;
  KP_HIP(ctx, hipMalloc((void**)&M->sb_col, col.size() * sizeof(int)));
  KP_HIP(ctx, hipMemcpy(M->sb_col, col.data(), col.size() * sizeof(int), hipMemcpyHostToDevice));
  KP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  M->sb_n = n; M->sb_kmax = kmax; M->sb_rows = 2 * n * (Np + 1);
  return KP_OK;
}

// the observation window and outputs of a loaded step (kp_mpc_step_loaded)
struct LoadIn {
  int nw, nobs, flags;
  const double *zeta_win, *u_win, *what_prev;
  double *what_out, *resnorm;
};

static int mpc_run(kp_mpc* M, const kp_basis* basis, int nb, const double* z, const double* zeta, const double* u_prev,
                   const double* Yr, int iters, double* U_out, double* z_out, int* status, const LoadIn* ld = nullptr) {
  kp_ctx* ctx = M->ctx;
  if (nb < 1 || !u_prev || !Yr || !U_out || iters < 1 || (!z && !zeta)) return ctx->fail(KP_ERR_ARG, "kp_mpc_step: bad argument");
  if (iters > 1 && M->model_type != KP_MODEL_BILINEAR) iters = 1;
  KP_HIP(ctx, hipSetDevice(ctx->device));
  const int N = M->N, m = M->m, Np = M->Np, nproj = M->nproj, nv = M->nvar, nr = M->nrows;
  int nzeta = 0;
  if (zeta) {
    if (!basis) return ctx->fail(KP_ERR_ARG, "kp_mpc_step_zeta: basis required");
    if (ld) {
      if (basis->dev.model_type == KP_MODEL_NONLINEAR || basis->dev.N * (ld->nw + 1) != N)
        return ctx->fail(KP_ERR_ARG, "kp_mpc_step_loaded: the controller's width must be basis N * (nw + 1) = " +
                                         std::to_string(basis->dev.N * (ld->nw + 1)) + ", it is " + std::to_string(N));
    } else if (basis->dev.N != N || basis->dev.model_type == KP_MODEL_NONLINEAR)
      return ctx->fail(KP_ERR_ARG, "kp_mpc_step_zeta: basis does not match the controller's model");
    nzeta = basis->dev.nzeta;
  }
  const size_t n_out = (size_t)nv + N;
  const size_t n_ex = (size_t)nv * nv + nv + nr;
  const size_t in_per = (size_t)std::max(N, 64) + m + (size_t)nproj * (Np + 1);
  if (M->io_problems < (size_t)nb) {
    if (M->d_in) (void)hipFree(M->d_in);
    if (M->d_out) (void)hipFree(M->d_out);
    if (M->work) (void)hipFree(M->work);
    if (M->h_in) (void)hipHostFree(M->h_in);
    if (M->h_out) (void)hipHostFree(M->h_out);
    M->d_in = M->d_out = M->work = M->h_in = M->h_out = nullptr;
    M->d_status = nullptr;
    M->io_problems = 0;
    size_t cap = (size_t)nb;
    KP_HIP(ctx, hipMalloc((void**)&M->d_in, cap * in_per * 8));
    KP_HIP(ctx, hipMalloc((void**)&M->d_out, cap * n_out * 8 + cap * sizeof(int) + 8));
    KP_HIP(ctx, hipMalloc((void**)&M->work, (n_ex + 16) * 8));
    KP_HIP(ctx, hipMemset(M->work, 0, (n_ex + 16) * 8));      // (stamps a step does not reach read as zero, not as stale memory)
    KP_HIP(ctx, hipHostMalloc((void**)&M->h_in, cap * in_per * 8, hipHostMallocDefault));
    KP_HIP(ctx, hipHostMalloc((void**)&M->h_out, cap * n_out * 8 + cap * sizeof(int) + 8, hipHostMallocDefault));
    M->io_problems = cap;
  }
  M->d_status = (int*)(M->d_out + M->io_problems * n_out);
  const size_t nz = zeta ? nzeta : N;
  double* d_z = M->d_in;
  double* d_up = d_z + (size_t)nb * nz;
  double* d_yr = d_up + (size_t)nb * m;
  // inputs packed in the pinned buffer in device order: one host-to-device copy
  const size_t n_in = (size_t)nb * (nz + m + (size_t)nproj * (Np + 1));
  memcpy(M->h_in, zeta ? zeta : z, (size_t)nb * nz * 8);
  memcpy(M->h_in + (size_t)nb * nz, u_prev, (size_t)nb * m * 8);
  memcpy(M->h_in + (size_t)nb * (nz + m), Yr, (size_t)nb * nproj * (Np + 1) * 8);
  // single problem: the kernel reads the (few hundred bytes of) inputs straight from the pinned, device-mapped
  // staging buffer and writes its outputs there - no copy commands at all on the latency path of a closed loop
  static const bool no_zc = getenv("KP_MPC_NO_ZEROCOPY") != nullptr;
  const bool zc = nb == 1 && !no_zc;
  if (zc) {
    d_z = M->h_in;
    d_up = d_z + (size_t)nb * nz;
    d_yr = d_up + (size_t)nb * m;
  } else {
    KP_HIP(ctx, hipMemcpyAsync(d_z, M->h_in, n_in * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  MpcArgs a{};
  if (zeta) a.basis = basis->dev;
  a.has_basis = zeta ? 1 : 0;
  a.model_type = M->model_type; a.N = N; a.m = m; a.Np = Np; a.nproj = nproj; a.nvar = nv; a.nrows = nr; a.iters = iters;
  a.q_run = M->q_run; a.q_term = M->q_term;
  a.A = M->A; a.B = M->B; a.P = M->P; a.S0 = M->S0; a.PB = M->PB; a.r = M->r; a.Aq = M->Aq; a.bq0 = M->bq0; a.Anorm = M->Anorm;
  a.ell = EllMat{M->ellv, M->ellc, M->Anorm, M->ellK};
  a.z = zeta ? nullptr : d_z;
  a.zeta = zeta ? d_z : nullptr;
  a.u_prev = d_up; a.Yr = d_yr;
  a.U = zc ? M->h_out : M->d_out;
  a.z_out = a.U + (size_t)nb * nv;
  a.qp_export = nb == 1 ? M->work : nullptr;
  a.assemble_only = M->sb_n > 0 ? 1 : 0;
  a.U_lin = nullptr;
  const bool sb = M->sb_n > 0;
  const int mr_sb = nr + M->sb_rows;
  if (sb) {
    // state-bound steps: per problem the exported H, f, b, the dense constraint matrix of the step, right-hand sides,
    // row norms and the solution of the generic QP kernel
    if (M->sb_cap < (size_t)nb) {
      if (M->sb_A) (void)hipFree(M->sb_A);
      if (M->sb_b) (void)hipFree(M->sb_b);
      if (M->sb_work) (void)hipFree(M->sb_work);
      M->sb_A = M->sb_b = M->sb_work = nullptr;
      M->sb_cap = 0;
      KP_HIP(ctx, hipMalloc((void**)&M->sb_A, (size_t)nb * mr_sb * nv * 8));
      KP_HIP(ctx, hipMalloc((void**)&M->sb_b, (size_t)nb * (2 * mr_sb + nv + 1) * 8 + 64));
      KP_HIP(ctx, hipMalloc((void**)&M->sb_work, (size_t)nb * n_ex * 8));
      M->sb_cap = (size_t)nb;
    }
    a.qp_export = M->sb_work;
    a.iters = 1;                       // the linearisation passes are driven from the host (the QP runs in its own kernel)
  }
  static const bool no_warm = getenv("KP_MPC_NO_WARM") != nullptr;
  static const int qp_wg = [] { const char* e = getenv("KP_QP_WG"); return e ? atoi(e) : 1; }();
  a.qp_wg = qp_wg;
  if (!M->warm) {
    KP_HIP(ctx, hipMalloc((void**)&M->warm, (size_t)(1 + nv) * sizeof(int)));
    KP_HIP(ctx, hipMemsetAsync(M->warm, 0, (size_t)(1 + nv) * sizeof(int), ctx->stream));
  }
  a.warm = (nb == 1 && !no_warm) ? M->warm : nullptr;
  a.status = zc ? (int*)(M->h_out + M->io_problems * n_out) : M->d_status;
  a.stamps = nb == 1 ? (long long*)(M->work + n_ex) : nullptr;
  // single zero-copy step without state bounds: the host does not go through hipStreamSynchronize (a 15-20 us wake-up) or
  // event records - the kernel stores a sequence number into pinned memory behind its outputs and the host spins on it
  static const bool no_spin = getenv("KP_MPC_NO_SPIN") != nullptr;
  const bool spin = zc && !sb && !no_spin;
  a.done_flag = nullptr;
  a.done_seq = 0;
  if (spin) {
    if (!M->h_flag) {
      KP_HIP(ctx, hipHostMalloc((void**)&M->h_flag, 64, hipHostMallocDefault));
      memset(M->h_flag, 0, 64);
    }
    a.done_flag = M->h_flag;
    a.done_seq = ++M->step_seq;
  }
  size_t lds = (size_t)mpc_lds_doubles(N, m, Np, nproj, nv, nr, (sb && iters > 1) ? 2 : iters, zeta ? basis->dev.nfull : 0) * 8 + 32;
  MpcLoadArgs la{};
  if (ld) {
    // the observer's block behind the step's; the window goes to page-locked memory the kernel reads in place
    const BasisDev& b = basis->dev;
    const LoadLayout L = load_layout(ld->nw, ld->nobs, nzeta, m, b.nfull, b.N);
    la.nw = ld->nw; la.nobs = ld->nobs; la.flags = ld->flags;
    la.obs_off = (int)((lds / 8 + 1) & ~(size_t)1);
    lds = (size_t)(la.obs_off + L.total) * 8;
    if (lds > 160 * 1024)
      return ctx->fail(KP_ERR_ARG, "kp_mpc_step_loaded: the observation window of " + std::to_string(ld->nobs) +
                                       " samples exceeds the LDS budget (" + std::to_string(lds) + " bytes of 163840)");
    const size_t nwin = (size_t)(ld->nobs + 1) * nzeta + (size_t)ld->nobs * m + ld->nw;
    if (M->h_ld_doubles < nwin + ld->nw + 2) {
      if (M->h_ld) (void)hipHostFree(M->h_ld);
      M->h_ld = nullptr;
      M->h_ld_doubles = 0;
      KP_HIP(ctx, hipHostMalloc((void**)&M->h_ld, (nwin + ld->nw + 2) * 8, hipHostMallocDefault));
      M->h_ld_doubles = nwin + ld->nw + 2;
    }
    double* w = M->h_ld;
    if (ld->nobs > 0) {
      memcpy(w, ld->zeta_win, (size_t)(ld->nobs + 1) * nzeta * 8);
      memcpy(w + (size_t)(ld->nobs + 1) * nzeta, ld->u_win, (size_t)ld->nobs * m * 8);
    }
    double* wp = w + (size_t)(ld->nobs + 1) * nzeta + (size_t)ld->nobs * m;
    for (int i = 0; i < ld->nw; ++i) wp[i] = ld->what_prev ? ld->what_prev[i] : 0.0;
    la.win = w;
    la.out = w + nwin;
  }
  {
    // batched launches: the assembly's inputs inside the solver's scratch, no exchange words of the workgroup-wide solver
    const int n_asm = N + N * m + Np * nproj * m + (Np + 1) * nproj;
    a.alias = (nb > 1 && !a.warm && !sb && iters == 1 && n_asm <= 2 * nv * nv) ? 1 : 0;
    if (a.alias) lds -= (size_t)(n_asm + 64) * 8;
  }
  if (lds > 160 * 1024) return ctx->fail(KP_ERR_ARG, "kp_mpc_step: problem too large for LDS");
  // single-problem launches: the model's P | PB block behind everything else in LDS when it fits (a batch reads it from L2,
  // shared by its workgroups, and needs its LDS for occupancy)
  static const bool no_stage = getenv("KP_MPC_NO_STAGE") != nullptr;
  a.stage_off = 0;
  a.stage_doubles = M->stage_doubles;
  if (nb == 1 && !no_stage && lds + 16 + (size_t)M->stage_doubles * 8 <= 160 * 1024) {
    a.stage_off = (int)((lds / 8 + 1) & ~(size_t)1);
    lds = (size_t)(a.stage_off + M->stage_doubles) * 8;
  }
  static KpLdsCache step_lds[2], loaded_lds[2];
  const int wk = a.warm != nullptr;
  static KpLdsCache batch_lds;
  const bool bk = a.alias != 0;                       // the batched entry point
  if (bk) KP_HIP(ctx, kp_ensure_lds(batch_lds, (const void*)kp_mpc_step_batch_kernel, lds));
  else if (ld)
    KP_HIP(ctx, kp_ensure_lds(loaded_lds[wk], wk ? (const void*)kp_mpc_step_loaded_kernel<true> : (const void*)kp_mpc_step_loaded_kernel<false>, lds));
  else KP_HIP(ctx, kp_ensure_lds(step_lds[wk], wk ? (const void*)kp_mpc_step_kernel<true> : (const void*)kp_mpc_step_kernel<false>, lds));
  // one launch of the single-problem step kernel (loaded steps: with the observer in front)
  auto launch_step = [&]() {
    if (ld) {
      if (wk) hipLaunchKernelGGL(kp_mpc_step_loaded_kernel<true>, dim3(nb), dim3(256), lds, ctx->stream, a, la);
      else hipLaunchKernelGGL(kp_mpc_step_loaded_kernel<false>, dim3(nb), dim3(256), lds, ctx->stream, a, la);
    } else if (wk) hipLaunchKernelGGL(kp_mpc_step_kernel<true>, dim3(nb), dim3(256), lds, ctx->stream, a);
    else hipLaunchKernelGGL(kp_mpc_step_kernel<false>, dim3(nb), dim3(256), lds, ctx->stream, a);
  };
  if (!spin) KP_HIP(ctx, hipEventRecord(ctx->evp[4], ctx->stream));
  if (!sb) {
    if (bk) hipLaunchKernelGGL(kp_mpc_step_batch_kernel, dim3(nb), dim3(256), lds, ctx->stream, a);
    else launch_step();
    KP_HIP(ctx, hipGetLastError());
  } else {
    // Every pass: the step kernel assembles H, f (along the lifted horizon of the previous pass's inputs from pass 2 on,
    // Kmpc.m:874-895) and the right-hand sides of the constant rows and stops; the dense constraint matrix of the step
    // is formed ONCE from z (the reference computes A = get_constraintL_bilinear(zrow) before its iteration loop,
    // Kmpc.m:861); the generic QP kernel solves, one wave per problem.
    double* bd = M->sb_b;                                   // [nb][mr]
    double* nrm = bd + (size_t)nb * mr_sb;                  // [nb][mr]
    double* dx = nrm + (size_t)nb * mr_sb;                  // [nb][nv]
    int* dst = (int*)(dx + (size_t)nb * nv);                // [nb]
    const size_t lq = (size_t)qp_lds_doubles(nv, mr_sb) * 8 + 64;
    static KpLdsCache sbqp_lds;
    KP_HIP(ctx, kp_ensure_lds(sbqp_lds, (const void*)kp_qp_kernel, lq));
    EllMat E{M->sb_A, M->sb_col, nrm, nv};
    for (int pass = 0; pass < iters; ++pass) {
      a.U_lin = pass > 0 ? dx : nullptr;
      launch_step();
      KP_HIP(ctx, hipGetLastError());
      if (pass == 0) {
        hipLaunchKernelGGL(kp_mpc_sb_kernel, dim3(nb), dim3(256), (size_t)(N * m + N) * 8, ctx->stream, M->model_type, N, m, Np, nv, nr, M->sb_n,
                           M->sb_kmax, M->sb_Apow, M->B, M->Aq, M->sb_work + (size_t)nv * nv + nv, a.z_out, M->sb_lohi, M->sb_A, bd, nrm, n_ex);
        KP_HIP(ctx, hipGetLastError());
      }
      hipLaunchKernelGGL(kp_qp_kernel, dim3(nb), dim3(64), lq, ctx->stream, M->sb_work, M->sb_work + (size_t)nv * nv, E, bd, nv, mr_sb, dx, dst,
                         n_ex, n_ex, (size_t)mr_sb * nv, (size_t)mr_sb, pass > 0 ? 1 : 0);
      KP_HIP(ctx, hipGetLastError());
    }
    // x and the status words into the output block the host reads below
    KP_HIP(ctx, hipMemcpyAsync(a.U, dx, (size_t)nb * nv * 8, zc ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ctx->stream));
    KP_HIP(ctx, hipMemcpyAsync(a.status, dst, (size_t)nb * sizeof(int), zc ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ctx->stream));
    if (nb == 1)   // kp_mpc_last_qp reads the single-problem export
      KP_HIP(ctx, hipMemcpyAsync(M->work, M->sb_work, n_ex * 8, hipMemcpyDeviceToDevice, ctx->stream));
  }
  if (!spin) KP_HIP(ctx, hipEventRecord(ctx->evp[5], ctx->stream));
  // one device-to-host copy: x and z of every problem, then the status words
  const size_t out_bytes = M->io_problems * n_out * 8 + (size_t)nb * sizeof(int);
  if (!zc) KP_HIP(ctx, hipMemcpyAsync(M->h_out, M->d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
  bool spun = false;
  if (spin) {
    volatile unsigned long long* fl = M->h_flag;
    for (long it = 0; it < 20000000L; ++it) {          // a few ms at most; a slower kernel falls through to the stream wait
      if (__atomic_load_n(&fl[0], __ATOMIC_ACQUIRE) == a.done_seq) { spun = true; break; }
      __builtin_ia32_pause();
    }
  }
  if (!spun) KP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  // x = [u_0; u_1; ...] (m each)  ->  U (Np x m column-major) = reshape(x,[m,Np])'  (Kmpc.m:884)
  const double* x = M->h_out;
  const int* st = (const int*)(M->h_out + M->io_problems * n_out);
  if (z_out) memcpy(z_out, M->h_out + (size_t)nb * nv, (size_t)nb * N * 8);
  for (int p = 0; p < nb; ++p) {
    for (int j = 0; j < Np; ++j)
      for (int i = 0; i < m; ++i) U_out[(size_t)p * nv + (size_t)i * Np + j] = x[(size_t)p * nv + j * m + i];
    if (status) status[p] = st[p];
  }
  if (ld) {
    if (ld->what_out) memcpy(ld->what_out, la.out, (size_t)ld->nw * 8);
    if (ld->resnorm) *ld->resnorm = la.out[ld->nw];
    // a failed estimate fails the step whatever path solved it (the state-bound passes run on the NaN state the kernel
    // exported and would report their own status)
    if (la.out[ld->nw + 1] != 0.0) {
      for (int i = 0; i < nv; ++i) U_out[i] = std::nan("");
      if (status) status[0] = KP_ERR_QP_FAIL;
    }
  }
  float ms = 0;
  if (spin) ctx->timers[2] = (double)(M->h_flag[2] - M->h_flag[1]) * 1e-5;        // wall_clock64 ticks of 10 ns -> ms
  else if (hipEventElapsedTime(&ms, ctx->evp[4], ctx->evp[5]) == hipSuccess) ctx->timers[2] = ms;
  return KP_OK;
}

extern "C" int kp_mpc_step(kp_mpc* M, const double* z, const double* u_prev, const double* Yr, int iters, double* U_out,
                           int* status) {
  if (!M) return KP_ERR_ARG;
  return mpc_run(M, nullptr, 1, z, nullptr, u_prev, Yr, iters, U_out, nullptr, status);
}

extern "C" int kp_mpc_step_zeta(kp_mpc* M, const kp_basis* basis, const double* zeta, const double* u_prev, const double* Yr,
                                int iters, double* U_out, double* z_out, int* status) {
  if (!M) return KP_ERR_ARG;
  return mpc_run(M, basis, 1, nullptr, zeta, u_prev, Yr, iters, U_out, z_out, status);
}

extern "C" int kp_mpc_step_loaded(kp_mpc* M, const kp_basis* basis, int nw, int nobs, const double* zeta_win, const double* u_win,
                                  const double* what_prev, int flags, const double* zeta, const double* u_prev, const double* Yr,
                                  int iters, double* U_out, double* z_out, double* what_out, double* resnorm, int* status) {
  if (!M) return KP_ERR_ARG;
  kp_ctx* ctx = M->ctx;
  if (!basis || !zeta) return ctx->fail(KP_ERR_ARG, "kp_mpc_step_loaded: basis and zeta are required");
  if (nw < 1 || nw > KP_LOAD_MAX_NW)
    return ctx->fail(KP_ERR_ARG, "kp_mpc_step_loaded: nw = " + std::to_string(nw) + " outside 1 .. " + std::to_string(KP_LOAD_MAX_NW));
  if (nobs < 0 || nobs > KP_LOAD_MAX_NOBS)
    return ctx->fail(KP_ERR_ARG, "kp_mpc_step_loaded: nobs = " + std::to_string(nobs) + " outside 0 .. " + std::to_string(KP_LOAD_MAX_NOBS));
  if (flags & ~(KP_LOAD_RATE | KP_LOAD_PIN_LAST)) return ctx->fail(KP_ERR_ARG, "kp_mpc_step_loaded: unknown flags");
  if (nobs > 0 && (!zeta_win || !u_win)) return ctx->fail(KP_ERR_ARG, "kp_mpc_step_loaded: nobs > 0 needs zeta_win and u_win");
  if ((nobs == 0 || (flags & KP_LOAD_RATE)) && !what_prev)
    return ctx->fail(KP_ERR_ARG, "kp_mpc_step_loaded: what_prev is required with nobs = 0 or KP_LOAD_RATE");
  const LoadIn ld{nw, nobs, flags, zeta_win, u_win, what_prev, what_out, resnorm};
  return mpc_run(M, basis, 1, nullptr, zeta, u_prev, Yr, iters, U_out, z_out, status, &ld);
}

extern "C" int kp_mpc_step_batch(kp_mpc* M, int nb, const double* z, const double* u_prev, const double* Yr, double* U_out,
                                 int* status) {
  if (!M) return KP_ERR_ARG;
  return mpc_run(M, nullptr, nb, z, nullptr, u_prev, Yr, 1, U_out, nullptr, status);
}

// Whole closed loops, one workgroup per trial (kp_mpc_sim_kernel); the host transfers are kp_sim_loop.h's.
extern "C" int kp_mpc_simulate(kp_mpc* M, const kp_basis* basis, int nb, int nref, const double* ref, int ref_shared,
                               const double* y0, const double* u0, int iters, double* U, double* Y, double* Z, int* steps_done,
                               int* status) {
  if (!M) return KP_ERR_ARG;
  kp_ctx* ctx = M->ctx;
  if (nb < 1 || nref < 1 || iters < 1)
    return ctx->fail(KP_ERR_ARG, "kp_mpc_simulate: nb, nref and iters must be at least 1 (nb = " + std::to_string(nb) + ", nref = " +
                                     std::to_string(nref) + ", iters = " + std::to_string(iters) + ")");
  if (!basis || !ref || !y0 || !u0 || !U || !Y || !steps_done || !status)
    return ctx->fail(KP_ERR_ARG, "kp_mpc_simulate: NULL argument (only Z may be NULL)");
  const BasisDev& b = basis->dev;
  if (b.model_type == KP_MODEL_NONLINEAR) return ctx->fail(KP_ERR_ARG, "kp_mpc_simulate: the dictionary of a nonlinear model");
  if (b.N != M->N)
    return ctx->fail(KP_ERR_ARG, "kp_mpc_simulate: the dictionary lifts to N = " + std::to_string(b.N) + ", the controller's model has N = " +
                                     std::to_string(M->N) + " (a loaded controller, N (nw + 1), has no such loop)");
  if (M->sb_n > 0)
    return ctx->fail(KP_ERR_ARG, "kp_mpc_simulate: the controller has state bounds (those steps go through the generic QP kernel)");
  const int N = M->N, m = M->m, Np = M->Np, nproj = M->nproj, nv = M->nvar, nr = M->nrows, n = b.nzeta;
  if (Np < 2) return ctx->fail(KP_ERR_ARG, "kp_mpc_simulate: the loop applies the second row of the solution: horizon >= 2");
  if (n > N || n > 256) return ctx->fail(KP_ERR_ARG, "kp_mpc_simulate: nzeta = " + std::to_string(n) + " exceeds N or 256");
  if (iters > 1 && M->model_type != KP_MODEL_BILINEAR) iters = 1;
  KP_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->async_pending) {
    int rc0 = kp_synchronize(ctx);
    if (rc0) return rc0;
  }
  // LDS: the step's block | the loop's block | P | PB when it still fits
  size_t lds = (size_t)mpc_lds_doubles(N, m, Np, nproj, nv, nr, iters, b.nfull) * 8 + 32;
  const SimLayout L = sim_layout(n, m, nv, nproj, Np, nref, b.nfull);
  MpcSimArgs sa{};
  sa.sim_off = (int)((lds / 8 + 1) & ~(size_t)1);
  const size_t lds_need = ((size_t)sa.sim_off + (size_t)L.total) * 8;
  if (lds_need > 160 * 1024)
    return ctx->fail(KP_ERR_ARG, "kp_mpc_simulate: the step and a reference of " + std::to_string(nref) + " rows need " +
                                     std::to_string(lds_need) + " bytes of LDS (163840 at most)");
  lds = lds_need;
  MpcArgs a{};
  a.basis = b;
  a.has_basis = 1;
  a.model_type = M->model_type; a.N = N; a.m = m; a.Np = Np; a.nproj = nproj; a.nvar = nv; a.nrows = nr; a.iters = iters;
  a.q_run = M->q_run; a.q_term = M->q_term;
  a.A = M->A; a.B = M->B; a.P = M->P; a.S0 = M->S0; a.PB = M->PB; a.r = M->r; a.Aq = M->Aq; a.bq0 = M->bq0; a.Anorm = M->Anorm;
  a.ell = EllMat{M->ellv, M->ellc, M->Anorm, M->ellK};
  a.qp_wg = 1;
  a.stage_off = 0;
  a.stage_doubles = M->stage_doubles;
  if (lds + 16 + (size_t)M->stage_doubles * 8 <= 160 * 1024) {
    a.stage_off = (int)((lds / 8 + 1) & ~(size_t)1);
    lds = (size_t)(a.stage_off + M->stage_doubles) * 8;
  }
  KpSimLoop& S = sa.loop;
  S.nref = nref; S.ny = n; S.m = m; S.nproj = nproj; S.Np = Np; S.ref_shared = ref_shared ? 1 : 0; S.aux_w = Z ? N : 0;
  KpSimIo io;
  if (int rcu = kp_sim_upload(ctx, "kp_mpc_simulate", nb, ref, y0, u0, S, io)) return rcu;
  hipStream_t s = ctx->stream;
  static KpLdsCache sim_lds;
  KP_HIP(ctx, kp_ensure_lds(sim_lds, (const void*)kp_mpc_sim_kernel, lds));
  KP_HIP(ctx, hipEventRecord(ctx->evp[4], s));
  hipLaunchKernelGGL(kp_mpc_sim_kernel, dim3(nb), dim3(256), lds, s, a, sa);
  KP_HIP(ctx, hipGetLastError());
  KP_HIP(ctx, hipEventRecord(ctx->evp[5], s));
  if (int rcd = kp_sim_download(ctx, io, S, U, Y, Z, steps_done, status)) return rcd;
  float ms = 0;
  if (hipEventElapsedTime(&ms, ctx->evp[4], ctx->evp[5]) == hipSuccess) ctx->timers[19] = ms;
  return KP_OK;
}

extern "C" int kp_mpc_last_qp(kp_mpc* M, double* Hq, double* f, double* Aq, double* bq) {
  if (!M || !M->work) return M ? M->ctx->fail(KP_ERR_ARG, "kp_mpc_last_qp: no single-problem step has run") : KP_ERR_ARG;
  kp_ctx* ctx = M->ctx;
  KP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t nv = M->nvar, nr = M->nrows;
  if (Hq) KP_HIP(ctx, hipMemcpy(Hq, M->work, nv * nv * 8, hipMemcpyDeviceToHost));
  if (f) KP_HIP(ctx, hipMemcpy(f, M->work + nv * nv, nv * 8, hipMemcpyDeviceToHost));
  if (bq) KP_HIP(ctx, hipMemcpy(bq, M->work + nv * nv + nv, nr * 8, hipMemcpyDeviceToHost));
  if (Aq) KP_HIP(ctx, hipMemcpy(Aq, M->Aq, nr * nv * 8, hipMemcpyDeviceToHost));
  return KP_OK;
}

// Diagnostics: phase times (microseconds) of the most recent single-problem step:
// [0] lift + e, [1] Beta/S, [2] H/f, [3] Hinv (Gauss-Jordan), [4] active-set iterations,
// [5] total kernel; counts[0] = solver iterations, counts[1] = active constraints at the optimum.
// every stamp of the most recent single step relative to its first, in microseconds (slots the step did not reach hold the value
// of an earlier step, or minus the first stamp if no step reached them yet): [1] tracking error, [2] S_k, [3] H and f, [4] solver entered, [5] solved, [10] inputs landed, [11] lifted
// state, [6] iteration loop entered, [12] H^-1, [13] warm-start products, [14] inverse of the warm set's Schur complement
extern "C" int kp_mpc_last_stamps(kp_mpc* M, double* us16) {
  if (!M || !M->work || !us16) return KP_ERR_ARG;
  kp_ctx* ctx = M->ctx;
  KP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t n_ex = (size_t)M->nvar * M->nvar + M->nvar + M->nrows;
  long long st[16];
  KP_HIP(ctx, hipMemcpy(st, M->work + n_ex, sizeof(st), hipMemcpyDeviceToHost));
  for (int i = 0; i < 16; ++i) us16[i] = (i == 8 || i == 9) ? (double)st[i] : (st[i] - st[0]) * 0.01;
  return KP_OK;
}

extern "C" int kp_mpc_last_profile(kp_mpc* M, double* us, int* counts) {
  if (!M || !M->work || !us) return KP_ERR_ARG;
  kp_ctx* ctx = M->ctx;
  KP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t n_ex = (size_t)M->nvar * M->nvar + M->nvar + M->nrows;
  long long st[16];
  KP_HIP(ctx, hipMemcpy(st, M->work + n_ex, sizeof(st), hipMemcpyDeviceToHost));
  const double tick = 0.01;  // wall_clock64: 100 MHz
  us[0] = (st[1] - st[0]) * tick;
  us[1] = (st[2] - st[1]) * tick;
  us[2] = (st[3] - st[2]) * tick;
  us[3] = (st[4] - st[3]) * tick;
  us[4] = (st[5] - st[4]) * tick;
  us[5] = (st[5] - st[0]) * tick;
  if (counts) {
    counts[0] = (int)st[8];
    counts[1] = (int)st[9];
  }
  return KP_OK;
}
