// Nonlinear MPC: the SQP of one get_mpcInput_nonlinear call (Kmpc.m:906-1181) in one launch, one workgroup per problem.
//
// The reference hands fmincon (SQP, exact gradients) the decision variable X = [z_0; ...; z_Np; u_1; ...; u_Np] with the
// dynamics z_k = F(z_{k-1}, u_k) as equality constraints (nonlcon_nmpc, :1074-1111), z_0 = zeta and u_1 = u_prev pinned
// (Aeq, :1149-1152).  Here the states are eliminated (single shooting): the decision variable is U = [u_1; ...; u_Np]
// (x layout: u_1 (m), u_2 (m), ...), z_k(U) is a rollout of the model and the problem is
//   min J(U) = sum_{k=0..Np} q_k |C z_k - r_k|^2 + sum_k u_k' R u_k     (get_costMatrices_nonlinear, :909-943)
//   s.t. the linear rows of get_constraintMatrices_nonlinear (:946-1059) on U and lo <= z_k <= hi (k = 0..Np)
// with q_k = cost_running (k < Np), cost_terminal (k = Np).  Its optimum is the reference's (same KKT points).
//
// F(v) = Kf econ_full(v), v = [zeta; u], is folded at create time into F(v) = Kv v + Kfull full(v) + c: without dim_red
// Kfull = Kf (Kv = 0, c = 0); with dim_red econ_full = [v; pcs' full(v); 1] (Ksysid.m:1615-1618), so Kv = Kf(:, 1:nv),
// Kfull = Kf(:, pcs block) pcs', c = Kf(:, N).  One Jacobian dF/dv is then nzeta * nfull * nvars FMAs.
//
// One SQP iteration, all in LDS: the Jacobians A_k = dF/dz, B_k = dF/du at the Np rollout points, the sensitivities
// S_k = dz_k/dU by the forward recursion S_k = A_k S_{k-1} + [0 .. B_k .. 0], the Gauss-Newton QP in the step d
//   min 1/2 d' Hq d + g' d,  Hq = 2 (sum_k q_k S_k'C'C S_k + R) (1 + nu on the diagonal),  g = grad J(U) (exact)
//   s.t. the linear rows on U + d, the state rows linearised as z_k + S_k d, d_1 = 0 (two "tack" rows, as kp_mpc.hip pins u_0)
// solved by the dual active-set solver of kp_qp.h, then a backtracking line search on the l1 merit J + mu * (sum of the
// constraint violations) - Armijo on J alone while the iterates are feasible, which they stay without state bounds.
// The Hessian carries a Levenberg-Marquardt damping nu diag(Hq): nu starts at `damping` (default 10), shrinks by 0.3 after
// every full step and stays after a shortened one, so the last iterations are undamped Gauss-Newton.  Undamped from
// the reference's start X0, the first Gauss-Newton step of a start from rest (u_prev = 0, the arm's stored step 0) jumps into
// the basin of a worse local minimum (cost 0.0919 against fmincon's 0.0838); the damped first steps follow the descent path
// into fmincon's.  The stopping test does not depend on nu: the KKT residual uses the exact gradient.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "kp_internal.h"
#include "koopman_hip_nmpc.h"
#include "kp_wg_inverse.h"
#include "kp_qp.h"
#include "kp_sim_loop.h"

#define NMPC_CHUNK 16           // dictionary columns whose gradients are staged per pass of the Jacobian
#define NMPC_LDS_MAX (160 * 1024)
#define NMPC_LS_MAX 30          // halvings of the line search

// ---- value and gradient of one dictionary column ----------------------------------------------------------------------
// Factor of variable i in a product column (MONO, HERMITE, FOURIER, FSPARSE): f and df/dv_i.
__device__ __forceinline__ void kp_col_factor(const BasisDev& b, const ColDesc& c, const double* v, int i, double& f, double& df) {
  const double x = v[i];
  const double twopi = 2.0 * 3.14159265358979323846;
  f = 1.0;
  df = 0.0;
  switch (c.kind) {
    case COL_MONO: {
      const int e = b.exps[(size_t)c.arg * b.nvars + i];
      if (e) {
        double p = 1.0;
        for (int k = 0; k < e - 1; ++k) p *= x;
        df = (double)e * p;
        f = p * x;
      }
      break;
    }
    case COL_HERMITE: {      // H_n' = 2 n H_{n-1}
      const int n = b.exps[(size_t)c.arg * b.nvars + i];
      if (n) {
        double h0 = 1.0, h1 = 2.0 * x;
        for (int k = 1; k < n; ++k) {
          const double h2 = 2.0 * x * h1 - 2.0 * (double)k * h0;
          h0 = h1;
          h1 = h2;
        }
        f = h1;
        df = 2.0 * (double)n * h0;
      }
      break;
    }
    case COL_FOURIER: {      // digit of variable i in the mixed-radix index (kp_eval_col)
      const int radix = 2 * c.aux + 1;
      int idx = c.arg;
      for (int j = b.nvars - 1; j > i; --j) idx /= radix;
      const int d = idx % radix;
      if (d) {
        const double w = twopi * (double)((d + 1) >> 1);
        double s, co;
        sincos(w * x, &s, &co);
        if (d & 1) { f = co; df = -w * s; }
        else { f = s; df = w * co; }
      }
      break;
    }
    case COL_FSPARSE: {
      const uint8_t* sm_ = b.exps + (size_t)c.arg * b.nvars;
      const int ms = sm_[i], mc = sm_[b.nvars + i];
      double fs = 1.0, dfs = 0.0, fc = 1.0, dfc = 0.0;
      if (ms) {
        double s, co;
        sincos(twopi * (double)ms * x, &s, &co);
        fs = s; dfs = twopi * (double)ms * co;
      }
      if (mc) {
        double s, co;
        sincos(twopi * (double)mc * x, &s, &co);
        fc = co; dfc = -twopi * (double)mc * s;
      }
      f = fs * fc;
      df = dfs * fc + fs * dfc;
      break;
    }
    default:
      break;
  }
}

// Value of full-basis column c at v (as kp_eval_col) and its gradient g[i * gs] = d col / d v_i, i < nvars.  Product
// columns take prefix and suffix products of their factors (no division: a factor may be zero).
__device__ __forceinline__ double kp_eval_col_grad(const BasisDev& b, const ColDesc c, const double* v, double* g, int gs) {
  const int nv = b.nvars;
  switch (c.kind) {
    case COL_VAR:
      for (int i = 0; i < nv; ++i) g[i * gs] = i == c.arg ? 1.0 : 0.0;
      return v[c.arg];
    case COL_GAUSS: {
      const double* ctr = b.centres + (size_t)c.arg * nv;
      double r2 = 0.0;
      for (int i = 0; i < nv; ++i) {
        const double d = v[i] - ctr[i];
        r2 += d * d;
      }
      const double e = exp(-r2);
      for (int i = 0; i < nv; ++i) g[i * gs] = -2.0 * (v[i] - ctr[i]) * e;
      return e;
    }
    case COL_MONO:
    case COL_HERMITE:
    case COL_FOURIER:
    case COL_FSPARSE: {
      double pre = 1.0, f, df;
      for (int i = 0; i < nv; ++i) {
        g[i * gs] = pre;
        kp_col_factor(b, c, v, i, f, df);
        pre *= f;
      }
      double suf = 1.0;
      for (int i = nv - 1; i >= 0; --i) {
        kp_col_factor(b, c, v, i, f, df);
        g[i * gs] = df == 0.0 ? 0.0 : g[i * gs] * df * suf;
        suf *= f;
      }
      return kp_eval_col(b, c, v, 1);
    }
    default:
      for (int i = 0; i < nv; ++i) g[i * gs] = 0.0;
      return 1.0;
  }
}

// ---- kp_lift_jacobian: d econ_full / dv at given rows ------------------------------------------------------------------
// One workgroup per row: the column gradients go to LDS (nfull x nvars), then the rows of econ_full: without dim_red the
// full basis itself, with dim_red [I; pcs' dfull; 0].  J: per row an N x nvars column-major block.
__global__ __launch_bounds__(256) void kp_lift_jacobian_kernel(BasisDev b, const double* __restrict__ V, int nrows, double* __restrict__ J) {
  extern __shared__ double sm[];
  const int tid = threadIdx.x, row = blockIdx.x, nv = b.nvars, N = b.N;
  double* v = sm;
  double* dfull = sm + ((nv + 1) & ~1);    // [c][i]
  for (int i = tid; i < nv; i += 256) v[i] = V[(size_t)i * nrows + row];
  __syncthreads();
  for (int c = tid; c < b.nfull; c += 256) kp_eval_col_grad(b, b.cols[c], v, dfull + (size_t)c * nv, 1);
  __syncthreads();
  double* Jr = J + (size_t)row * N * nv;
  for (int e = tid; e < N * nv; e += 256) {
    const int c = e % N, i = e / N;
    double s;
    if (b.k_pcs == 0)
      s = dfull[(size_t)c * nv + i];
    else if (c < nv)
      s = c == i ? 1.0 : 0.0;
    else if (c < nv + b.k_pcs) {
      const double* pc = b.pcs + (size_t)(c - nv) * b.nfull;
      s = 0.0;
      for (int j = 0; j < b.nfull; ++j) s += pc[j] * dfull[(size_t)j * nv + i];
    } else
      s = 0.0;
    Jr[e] = s;
  }
}

extern "C" int kp_lift_jacobian(kp_ctx* ctx, const kp_basis* basis, int nrows, const double* V, double* J) {
  if (!ctx) return KP_ERR_ARG;
  if (!basis || !V || !J || nrows < 0) return ctx->fail(KP_ERR_ARG, "kp_lift_jacobian: bad argument");
  if (nrows == 0) return KP_OK;
  const BasisDev& b = basis->dev;
  const size_t lds = (size_t)(((b.nvars + 1) & ~1) + (size_t)b.nfull * b.nvars) * 8;
  if (lds > 64 * 1024)
    return ctx->fail(KP_ERR_ARG, "kp_lift_jacobian: nfull * nvars + nvars (rounded up to even) = " +
                                     std::to_string(lds / 8) + " exceeds the 8192 doubles of the kernel's LDS");
  KP_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->async_pending) {
    int rc0 = kp_synchronize(ctx);
    if (rc0) return rc0;
  }
  const size_t nV = (size_t)nrows * b.nvars, nJ = (size_t)nrows * b.N * b.nvars;
  double* ws = (double*)ctx->workspace(6, (nV + nJ) * 8);
  if (!ws) return ctx->fail(KP_ERR_HIP, "kp_lift_jacobian: out of device memory");
  hipStream_t s = ctx->stream;
  KP_HIP(ctx, hipMemcpyAsync(ws, V, nV * 8, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(kp_lift_jacobian_kernel, dim3(nrows), dim3(256), lds, s, b, ws, nrows, ws + nV);
  KP_HIP(ctx, hipGetLastError());
  KP_HIP(ctx, hipMemcpyAsync(J, ws + nV, nJ * 8, hipMemcpyDeviceToHost, s));
  KP_HIP(ctx, hipStreamSynchronize(s));
  return KP_OK;
}

// ---- the SQP step kernel ---------------------------------------------------------------------------------------------
struct NmpcLayout {   // LDS offsets (doubles, each even)
  int Kfull, zeta0, up, Yr, U, dU, Ut, V, Vt, Z, Zt, full, dfull, Jac, S, P, ev, f, Hq, bq, act, red, sc, qws, total;
};
__host__ __device__ inline int nm_even(int n) { return (n + 1) & ~1; }
__host__ __device__ inline NmpcLayout nmpc_layout(int nz, int m, int Np, int nproj, int nfull, int mr) {
  NmpcLayout L;
  const int nv = nz + m, nU = m * Np;
  int o = 0;
  L.Kfull = o; o += nm_even(nz * nfull);
  L.zeta0 = o; o += nm_even(nz);
  L.up = o; o += nm_even(m);
  L.Yr = o; o += nm_even((Np + 1) * nproj);
  L.U = o; o += nm_even(nU);
  L.dU = o; o += nm_even(nU);
  L.Ut = o; o += nm_even(nU);
  L.V = o; o += nm_even(Np * nv);
  L.Vt = o; o += nm_even(Np * nv);
  L.Z = o; o += nm_even((Np + 1) * nz);
  L.Zt = o; o += nm_even((Np + 1) * nz);
  L.full = o; o += nm_even(nfull);
  L.dfull = o; o += nm_even(Np * NMPC_CHUNK * nv);
  L.Jac = o; o += nm_even(Np * nz * nv);
  L.S = o; o += nm_even((Np + 1) * nz * nU);
  L.P = o; o += nm_even((Np + 1) * nproj * nU);
  L.ev = o; o += nm_even((Np + 1) * nproj);
  L.f = o; o += nm_even(nU);
  L.Hq = o; o += nm_even(nU * nU);
  L.bq = o; o += nm_even(mr);
  L.act = o; o += nm_even((nU + 2) / 2);
  L.red = o; o += 16;
  L.sc = o; o += 16;
  L.qws = o; o += nm_even(qp_lds_doubles(nU, mr));
  L.total = o;
  return L;
}

struct NmpcArgs {
  BasisDev b;
  int nz, m, nv, Np, nproj, nU, nlin, mr, sb, max_iter;
  double q_run, q_term, tol_kkt, tol_step, damping;
  const double *Kv, *Kfull, *cvec, *proj, *r, *sb_lohi;
  EllMat lin;             // linear rows over U (box, slope, smooth, then the two tack rows of u_1), constant
  const double* lin_b;    // their right-hand sides (the tack rows' parts come from u_prev)
  double* dval;           // state bounds: per problem the dense rows [mr x nU] (linear rows, then the state rows) ...
  int* dcol;              //   ... their column table (col[k mr + r] = k, shared) and row norms [mr] per problem
  double* dnorm;
  const double* in;       // per problem: zeta (nz) | u_prev (m) | Yr (nproj (Np+1)) | has_init (1) | U_init (nU, x layout)
  int in_per;
  double* out;            // per problem: U (nU, x layout) | Z ((Np+1) nz) | info: iterations, KKT residual
  int out_per;
  int* status;
  double* jac_out;        // problem 0: the Jacobians [Np][nz x nv] of the last linearisation (or nullptr)
  unsigned long long* done_flag;
  unsigned long long done_seq;
  NmpcLayout L;
};

__device__ __forceinline__ double nm_wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double nm_wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
// workgroup sums / maxima of two values, the same in every thread (fixed order: deterministic)
__device__ __forceinline__ void nm_block2(double& a, double& b, double* red, bool amax, bool bmax) {
  a = amax ? nm_wave_max(a) : nm_wave_sum(a);
  b = bmax ? nm_wave_max(b) : nm_wave_sum(b);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[w] = a; red[4 + w] = b; }
  __syncthreads();
  a = amax ? fmax(fmax(red[0], red[1]), fmax(red[2], red[3])) : (red[0] + red[1]) + (red[2] + red[3]);
  b = bmax ? fmax(fmax(red[4], red[5]), fmax(red[6], red[7])) : (red[4] + red[5]) + (red[6] + red[7]);
  __syncthreads();
}

// The dense constraint matrix of a controller with state bounds (global memory, [mr x nU] per problem): its linear rows.
// They are constant; the state rows behind them are rewritten at every linearisation.
__device__ __forceinline__ void nmpc_dense_lin_rows(const NmpcArgs& a, double* dval, double* dnorm) {
  const int nlin = a.nlin, nU = a.nU, mr = a.mr;
  for (int row = threadIdx.x; row < nlin; row += 256) {
    for (int k = 0; k < nU; ++k) dval[(size_t)k * mr + row] = 0.0;
    for (int k = 0; k < a.lin.K; ++k) {
      const double v = a.lin.val[k * nlin + row];
      if (v != 0.0) dval[(size_t)a.lin.col[k * nlin + row] * mr + row] = v;
    }
    dnorm[row] = a.lin.norm[row];
  }
}

// One SQP step of problem pb; returns its status, the iteration count and the KKT residual, and leaves the returned inputs in
// the U block and their rollout z_0 .. z_Np in the Z block of LDS.
// SIM = false (kp_nmpc_kernel): the problem's inputs come from a.in, Kfull and the dense linear rows are staged here, the
//   results go to a.out / a.status.
// SIM = true (kp_nmpc_sim_kernel): Kfull, zeta0, up and the dense linear rows are in place, the reference window is yr_sim
//   (LDS), and the start is X0 (up repeated) or, with warm, the U block's previous content shifted by one row, last row
//   repeated, row 1 = up.  Nothing is written to global memory but the state rows of the dense matrix.
template <bool SIM>
__device__ __forceinline__ int nmpc_step_body(const NmpcArgs& a, double* sm, const int pb, const double* yr_sim, const bool warm,
                                              int& it_out, double& kkt_out) {
  const int tid = threadIdx.x;
  const NmpcLayout& L = a.L;
  const BasisDev& b = a.b;
  const int nz = a.nz, m = a.m, nv = a.nv, Np = a.Np, nproj = a.nproj, nU = a.nU, mr = a.mr, nlin = a.nlin, nfull = b.nfull;
  const double* Yr = SIM ? yr_sim : sm + L.Yr;
  double *Kfull = sm + L.Kfull, *zeta0 = sm + L.zeta0, *up = sm + L.up, *U = sm + L.U, *dU = sm + L.dU,
         *Ut = sm + L.Ut, *V = sm + L.V, *Vt = sm + L.Vt, *Z = sm + L.Z, *Zt = sm + L.Zt, *full = sm + L.full,
         *dfull = sm + L.dfull, *Jac = sm + L.Jac, *S = sm + L.S, *P = sm + L.P, *ev = sm + L.ev, *f = sm + L.f,
         *Hq = sm + L.Hq, *bq = sm + L.bq, *red = sm + L.red, *sc = sm + L.sc, *qws = sm + L.qws;
  int* act = (int*)(sm + L.act);
  const double* in = a.in + (size_t)pb * a.in_per;
  double* dval = a.sb ? a.dval + (size_t)pb * mr * nU : nullptr;
  double* dnorm = a.sb ? a.dnorm + (size_t)pb * mr : nullptr;
  const double* sb_lo = a.sb_lohi;
  const double* sb_hi = a.sb_lohi + nz;
  const int tack0 = nlin - 2 * m;

  if constexpr (!SIM) {
    double* Yrs = sm + L.Yr;
    for (int e = tid; e < nz * nfull; e += 256) Kfull[e] = a.Kfull[e];
    for (int e = tid; e < nz; e += 256) zeta0[e] = in[e];
    for (int e = tid; e < m; e += 256) up[e] = in[nz + e];
    for (int e = tid; e < (Np + 1) * nproj; e += 256) Yrs[e] = in[nz + m + e];
    const int o_init = nz + m + (Np + 1) * nproj;
    const bool has_init = in[o_init] != 0.0;
    __syncthreads();
    for (int j = tid; j < nU; j += 256) U[j] = j < m ? up[j] : (has_init ? in[o_init + 1 + j] : up[j % m]);   // u_1 = u_prev (:1152, X0 :1155)
  } else {
    double u_start = 0.0;                       // (nU <= 64: one entry per thread)
    if (tid < nU) {
      const int row = tid / m, i = tid - row * m;
      u_start = row == 0 ? up[i] : (warm ? U[min(row + 1, Np - 1) * m + i] : up[i]);
    }
    __syncthreads();                            // (every read of the previous solution is done)
    if (tid < nU) U[tid] = u_start;
  }
  // right-hand side of linear row `row` (the tack rows pin u_1 to u_prev)
  auto lin_rhs = [&](int row) -> double {
    const int t = row - tack0;
    return t < 0 ? a.lin_b[row] : (t < m ? up[t] : -up[t - m]);
  };
  if constexpr (!SIM)
    if (a.sb) nmpc_dense_lin_rows(a, dval, dnorm);   // the linear rows of the dense constraint matrix, once per step
  __syncthreads();

  // ---- rollout of Ub: points Vb [k][nv] = [z_k; u_{k+1}], states Zb [k][nz]; returns (J, sum of constraint violations) ----
  auto rollout = [&](const double* Ub, double* Vb, double* Zb, double& Jc, double& viol) {
    for (int e = tid; e < nz; e += 256) Zb[e] = zeta0[e];
    __syncthreads();
    for (int k = 0; k < Np; ++k) {
      double* v = Vb + k * nv;
      for (int e = tid; e < nv; e += 256) v[e] = e < nz ? Zb[k * nz + e] : Ub[k * m + e - nz];
      __syncthreads();
      for (int c = tid; c < nfull; c += 256) full[c] = kp_eval_col(b, b.cols[c], v, 1);
      __syncthreads();
      const int g = tid >> 5, l = tid & 31;      // 8 groups of 32 lanes; a group sums one output row
      for (int r0 = 0; r0 < nz; r0 += 8) {
        const int r = r0 + g;
        double s = 0.0;
        if (r < nz) {
          for (int i = l; i < nv; i += 32) s += a.Kv[r + (size_t)i * nz] * v[i];
          for (int c = l; c < nfull; c += 32) s += Kfull[r + (size_t)c * nz] * full[c];
        }
        for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (r < nz && l == 0) Zb[(k + 1) * nz + r] = s + a.cvec[r];
      }
      __syncthreads();
    }
    double jp = 0.0, vp = 0.0;
    for (int e = tid; e < (Np + 1) * nproj; e += 256) {
      const int k = e / nproj, p = e % nproj;
      double s = -Yr[e];
      for (int t = 0; t < nz; ++t) s += a.proj[p + t * nproj] * Zb[k * nz + t];
      jp += (k == Np ? a.q_term : a.q_run) * s * s;
    }
    for (int j = tid; j < nU; j += 256) jp += a.r[j % m] * Ub[j] * Ub[j];
    for (int row = tid; row < nlin; row += 256) {
      double s = -lin_rhs(row);
      for (int k = 0; k < a.lin.K; ++k) s += a.lin.val[k * nlin + row] * Ub[a.lin.col[k * nlin + row]];
      vp += fmax(s, 0.0);
    }
    if (a.sb)
      for (int e = tid; e < (Np + 1) * nz; e += 256) {
        const int i = e % nz;
        vp += fmax(sb_lo[i] - Zb[e], 0.0) + fmax(Zb[e] - sb_hi[i], 0.0);
      }
    nm_block2(jp, vp, red, false, false);
    Jc = jp;
    viol = vp;
  };

  double J, viol;
  rollout(U, V, Z, J, viol);
  int status = KP_ERR_NOT_CONVERGED, it = 0;
  double kkt = __builtin_inf(), mu = 0.0, nu = a.damping;
  while (it < a.max_iter) {
    // ---- Jacobians [A_k B_k] = dF/dv at v_k = [z_{k-1}; u_k], column-major nz x nv each ----
    for (int e = tid; e < Np * nz * nv; e += 256) Jac[e] = 0.0;
    for (int c0 = 0; c0 < nfull; c0 += NMPC_CHUNK) {
      for (int e = tid; e < Np * NMPC_CHUNK; e += 256) {
        const int k = e / NMPC_CHUNK, cc = e % NMPC_CHUNK, c = c0 + cc;
        double* g = dfull + (size_t)e * nv;
        if (c < nfull) kp_eval_col_grad(b, b.cols[c], V + k * nv, g, 1);
        else
          for (int i = 0; i < nv; ++i) g[i] = 0.0;
      }
      __syncthreads();
      for (int e = tid; e < Np * nz * nv; e += 256) {
        const int k = e / (nz * nv), rem = e % (nz * nv), i = rem / nz, r = rem % nz;
        const double* g = dfull + (size_t)k * NMPC_CHUNK * nv + i;
        double s = Jac[e];
        for (int cc = 0; cc < NMPC_CHUNK; ++cc) s += Kfull[r + (size_t)(c0 + cc < nfull ? c0 + cc : 0) * nz] * g[cc * nv];
        Jac[e] = s;
      }
      __syncthreads();
    }
    for (int e = tid; e < Np * nz * nv; e += 256) {
      const int rem = e % (nz * nv), i = rem / nz, r = rem % nz;
      Jac[e] += a.Kv[r + (size_t)i * nz];
    }
    __syncthreads();
    // ---- sensitivities S_k = dz_k / dU (nz x nU column-major), S_0 = 0 ----
    for (int e = tid; e < nz * nU; e += 256) S[e] = 0.0;
    for (int k = 1; k <= Np; ++k) {
      const double* Jk = Jac + (size_t)(k - 1) * nz * nv;
      const double* Sp = S + (size_t)(k - 1) * nz * nU;
      double* Sk = S + (size_t)k * nz * nU;
      for (int e = tid; e < nz * nU; e += 256) {
        const int r = e % nz, j = e / nz, blk = j / m;
        double s = 0.0;
        if (blk < k - 1)
          for (int t = 0; t < nz; ++t) s += Jk[r + t * nz] * Sp[t + j * nz];
        else if (blk == k - 1)
          s = Jk[r + (nz + j - blk * m) * nz];
        Sk[e] = s;
      }
      __syncthreads();
    }
    // ---- P_k = C S_k, e_k = C z_k - r_k ----
    for (int e = tid; e < (Np + 1) * nproj * nU; e += 256) {
      const int k = e / (nproj * nU), rem = e % (nproj * nU), j = rem / nproj, p = rem % nproj;
      const double* Sk = S + (size_t)k * nz * nU + (size_t)j * nz;
      double s = 0.0;
      for (int t = 0; t < nz; ++t) s += a.proj[p + t * nproj] * Sk[t];
      P[e] = s;
    }
    for (int e = tid; e < (Np + 1) * nproj; e += 256) {
      const int k = e / nproj, p = e % nproj;
      double s = -Yr[e];
      for (int t = 0; t < nz; ++t) s += a.proj[p + t * nproj] * Z[k * nz + t];
      ev[e] = s;
    }
    __syncthreads();
    // ---- Hq = 2 (sum_k q_k P_k'P_k + R), gradient f = 2 (sum_k q_k P_k' e_k + R U) ----
    for (int e = tid; e < nU * nU; e += 256) {
      const int j1 = e % nU, j2 = e / nU;
      double s = 0.0;
      for (int k = 1; k <= Np; ++k) {
        const double* Pk = P + (size_t)k * nproj * nU;
        double t = 0.0;
        for (int p = 0; p < nproj; ++p) t += Pk[p + j1 * nproj] * Pk[p + j2 * nproj];
        s += (k == Np ? a.q_term : a.q_run) * t;
      }
      if (j1 == j2) s = (s + a.r[j1 % m]) * (1.0 + nu);      // (Levenberg-Marquardt damping of the diagonal)
      Hq[e] = 2.0 * s;
    }
    for (int j = tid; j < nU; j += 256) {
      double s = 0.0;
      for (int k = 1; k <= Np; ++k) {
        const double* Pk = P + (size_t)k * nproj * nU;
        double t = 0.0;
        for (int p = 0; p < nproj; ++p) t += Pk[p + j * nproj] * ev[k * nproj + p];
        s += (k == Np ? a.q_term : a.q_run) * t;
      }
      f[j] = 2.0 * (s + a.r[j % m] * U[j]);
    }
    // ---- constraint rows on the step: A d <= b - A U (linear), -+S_k d <= z_k - lo / hi - z_k (states) ----
    for (int row = tid; row < nlin; row += 256) {
      double s = lin_rhs(row);
      for (int k = 0; k < a.lin.K; ++k) s -= a.lin.val[k * nlin + row] * U[a.lin.col[k * nlin + row]];
      bq[row] = s;
    }
    if (a.sb) {
      for (int e = tid; e < 2 * (Np + 1) * nz; e += 256) {     // row nlin + e: state k, lower (i < nz) or upper bound of i
        const int k = e / (2 * nz), rem = e % (2 * nz), hi = rem >= nz, i = hi ? rem - nz : rem, row = nlin + e;
        const double* Sk = S + (size_t)k * nz * nU;
        const double sg = hi ? 1.0 : -1.0;
        double nrm = 0.0;
        for (int j = 0; j < nU; ++j) {
          const double v = sg * Sk[i + j * nz];
          dval[(size_t)j * mr + row] = v;
          nrm += v * v;
        }
        dnorm[row] = sqrt(nrm);
        bq[row] = hi ? sb_hi[i] - Z[k * nz + i] : Z[k * nz + i] - sb_lo[i];
      }
      __threadfence_block();   // the dense rows live in global memory: visible to every wave of the workgroup
    }
    __syncthreads();
    // ---- QP ----
    const EllMat E = a.sb ? EllMat{dval, a.dcol, dnorm, nU} : a.lin;
    const int hbad = wg_spd_inverse_pp(qws, Hq, nU, nU, true);
    if (nU <= 32 && E.K <= QP_KLDS) {
      const int st = qp_gi_wg(f, E, bq, nU, mr, qws, qws + qp_lds_doubles(nU, mr) - 64, dU, 1e-10, nullptr, hbad, 0, act);
      if (tid == 0) sc[0] = st;
    } else if (tid < 64) {
      const int st = qp_goldfarb_idnani(Hq, f, E, bq, nU, mr, qws, dU, 1e-10, nullptr, true, hbad, 0, act);
      if (tid == 0) sc[0] = st;
    }
    __syncthreads();
    ++it;
    if (sc[0] != 0.0) {
      status = KP_ERR_QP_FAIL;
      break;
    }
    for (int j = tid; j < m; j += 256) dU[j] = 0.0;   // (the tack rows hold d_1 at 0 to the solver's tolerance: keep u_1 = u_prev exact)
    // ---- KKT residual of the NLP at U from the QP multipliers: stationarity |grad J + A'lam| (= -Hq d at the QP's
    //      optimum), primal infeasibility max(g(U), 0) = max(-b, 0), complementarity lam_i |g_i(U)|; step |d| ----
    const int q = act[0];
    const double* lam = qws + 3 * nU * nU + 3 * nU;
    double kp = 0.0, sp = 0.0;
    for (int j = tid; j < nU; j += 256) {
      double s = f[j];
      for (int c = 0; c < q; ++c) {
        const int row = act[1 + c];
        double arj = 0.0;
        if (a.sb) arj = dval[(size_t)j * mr + row];
        else
          for (int k = 0; k < E.K; ++k) arj += E.col[k * mr + row] == j ? E.val[k * mr + row] : 0.0;
        s += lam[c] * arj;
      }
      kp = fmax(kp, fabs(s));
      sp = fmax(sp, fabs(dU[j]));
    }
    for (int row = tid; row < mr; row += 256) kp = fmax(kp, fmax(-bq[row], 0.0));
    double lmax = 0.0;
    for (int c = tid; c < q; c += 256) {
      kp = fmax(kp, lam[c] * fabs(bq[act[1 + c]]));
      lmax = fmax(lmax, lam[c]);
    }
    nm_block2(kp, sp, red, true, true);
    double dd = 0.0;
    for (int j = tid; j < nU; j += 256) dd += f[j] * dU[j];
    nm_block2(lmax, dd, red, true, false);
    kkt = kp;
    if (kkt <= a.tol_kkt && sp <= a.tol_step) {
      status = KP_OK;
      break;
    }
    if (it >= a.max_iter) break;
    // ---- backtracking line search on the l1 merit ----
    mu = fmax(mu, 2.0 * lmax);
    const double phi = J + mu * viol, D = dd - mu * viol;
    double alpha = 1.0;
    bool ok = false;
    for (int ls = 0; ls < NMPC_LS_MAX; ++ls) {
      for (int j = tid; j < nU; j += 256) Ut[j] = U[j] + alpha * dU[j];
      __syncthreads();
      double Jt, vt;
      rollout(Ut, Vt, Zt, Jt, vt);
      // Armijo, with a slack of the merit's rounding (near the optimum the predicted decrease falls below it)
      if (Jt + mu * vt <= phi + 1e-4 * alpha * fmin(D, 0.0) + 1e-13 * fabs(phi)) {
        J = Jt;
        viol = vt;
        ok = true;
        break;
      }
      alpha *= 0.5;
    }
    if (!ok) break;   // no decrease along the step: the last iterate, KP_ERR_NOT_CONVERGED
    if (alpha == 1.0) nu = nu * 0.3 < 1e-12 ? 0.0 : nu * 0.3;   // (a shortened step keeps nu: doubling it made steps near a
                                                              // degenerate optimum creep)
    for (int j = tid; j < nU; j += 256) U[j] = Ut[j];
    for (int e = tid; e < Np * nv; e += 256) V[e] = Vt[e];
    for (int e = tid; e < (Np + 1) * nz; e += 256) Z[e] = Zt[e];
    __syncthreads();
  }

  it_out = it;
  kkt_out = kkt;
  if constexpr (!SIM) {
    double* out = a.out + (size_t)pb * a.out_per;
    for (int j = tid; j < nU; j += 256) out[j] = status == KP_ERR_QP_FAIL ? __builtin_nan("") : U[j];
    for (int e = tid; e < (Np + 1) * nz; e += 256) out[nU + e] = Z[e];
    if (tid == 0) {
      out[nU + (Np + 1) * nz] = (double)it;
      out[nU + (Np + 1) * nz + 1] = kkt;
      a.status[pb] = status;
    }
    if (a.jac_out && pb == 0)
      for (int e = tid; e < Np * nz * nv; e += 256) a.jac_out[e] = Jac[e];
  }
  return status;
}

__global__ __launch_bounds__(256) void kp_nmpc_kernel(NmpcArgs a) {
  extern __shared__ __align__(16) double sm[];
  int it;
  double kkt;
  nmpc_step_body<false>(a, sm, blockIdx.x, nullptr, false, it, kkt);
  if (a.done_flag && blockIdx.x == 0) {
    __syncthreads();
    if (threadIdx.x == 0) {
      __threadfence_system();
      __hip_atomic_store(&a.done_flag[0], a.done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// ---- whole closed loops with the model as the plant (kp_nmpc_simulate; the loop's contract: kp_sim_loop.h) ---------------
// The step is the SQP of kp_nmpc_step; the plant step is Y[k] = z_1 of the solution's rollout = F(zeta, u_prev), because
// u_1 is pinned to u_prev.  mu and the damping restart at every step, as in separate launches.
// Staged once per trial besides the padded reference (behind the step's block, at sim_off): Kfull and, with state bounds,
// the constant linear rows of the trial's dense constraint matrix.  zeta, u_prev and the previous solution U stay in the
// step's own LDS blocks from one step to the next.  Only a failed QP subproblem ends the trial; an unconverged step returns
// its last iterate, the trial goes on and its status becomes KP_ERR_NOT_CONVERGED.  The aux rows are info: SQP iterations,
// KKT residual and status of every step.  Every loop is bounded by nref, max_iter and NMPC_LS_MAX.
struct NmpcSimArgs {
  KpSimLoop loop;                   // (ny = nz, aux = info, aux_w = 3)
  int warm, sim_off;
};
__global__ __launch_bounds__(256) void kp_nmpc_sim_kernel(NmpcArgs a, NmpcSimArgs sa) {
  extern __shared__ __align__(16) double sm[];
  const int tid = threadIdx.x, pb = blockIdx.x;
  const size_t trial = blockIdx.x;
  const KpSimLoop& S = sa.loop;
  const NmpcLayout& L = a.L;
  const int nz = a.nz, m = a.m, nproj = a.nproj, nref = S.nref, nfull = a.b.nfull;
  double *Kfull = sm + L.Kfull, *zeta0 = sm + L.zeta0, *up = sm + L.up, *U = sm + L.U, *Z = sm + L.Z, *refl = sm + sa.sim_off;
  // ---- once per trial ----
  for (int e = tid; e < nz * nfull; e += 256) Kfull[e] = a.Kfull[e];
  const KpSimRows T = kp_sim_prologue(S, refl, zeta0, up);
  if (a.sb) nmpc_dense_lin_rows(a, a.dval + trial * (size_t)a.mr * a.nU, a.dnorm + trial * (size_t)a.mr);
  __syncthreads();
  int k = 1, failed = 0, unconverged = 0;
  for (; k < nref; ++k) {
    int it;
    double kkt;
    const int st = nmpc_step_body<true>(a, sm, pb, refl + (size_t)(k - 1) * nproj, sa.warm != 0 && k > 1, it, kkt);
    if (st == KP_ERR_QP_FAIL) {             // (uniform)
      failed = 1;
      break;
    }
    unconverged |= st != KP_OK;
    __syncthreads();                        // (every read of zeta0 and up is done; U and Z are the step's results)
    kp_sim_commit(S, T, k, zeta0, up, [&](int e) { return Z[nz + e]; },      // z_1 = F(zeta, u_prev)
                  [&](int e) { return U[m + e]; });                            // the second row of the solution
    if (T.aux && tid == 0) {
      T.aux[(size_t)(k - 1) * 3] = (double)it;
      T.aux[(size_t)(k - 1) * 3 + 1] = kkt;
      T.aux[(size_t)(k - 1) * 3 + 2] = (double)st;
    }
    __syncthreads();
  }
  kp_sim_epilogue(S, T, k, failed, failed ? KP_ERR_QP_FAIL : (unconverged ? KP_ERR_NOT_CONVERGED : KP_OK));
}

// ---- host side ---------------------------------------------------------------------------------------------------------
struct kp_nmpc {
  kp_ctx* ctx = nullptr;
  const kp_basis* basis = nullptr;
  int nz = 0, m = 0, nv = 0, Np = 0, nproj = 0, nU = 0, nlin = 0, linK = 1, sb = 0, max_iter = 60;
  double q_run = 0, q_term = 0, tol_kkt = 1e-8, tol_step = 1e-8, damping = 10.0;
  double *Kv = nullptr, *Kfull = nullptr, *cvec = nullptr, *proj = nullptr, *r = nullptr;
  double *lin_val = nullptr, *lin_b = nullptr, *lin_norm = nullptr;
  int* lin_col = nullptr;
  double* sb_lohi = nullptr;
  double *dval = nullptr, *dnorm = nullptr;    // state-bound rows of every problem of a launch
  int* dcol = nullptr;
  size_t dense_problems = 0;
  double *h_in = nullptr, *h_out = nullptr;    // page-locked: the kernel reads the inputs and writes the outputs in place
  int* h_status = nullptr;
  size_t io_problems = 0;
  unsigned long long* h_flag = nullptr;
  unsigned long long step_seq = 0;
  double* jac = nullptr;                        // device: the Jacobians of the last single step
};

static int nmpc_rows(const kp_nmpc* M) { return M->nlin + (M->sb ? 2 * (M->Np + 1) * M->nz : 0); }

extern "C" int kp_nmpc_destroy(kp_nmpc* M) {
  if (!M) return KP_OK;
  (void)hipSetDevice(M->ctx->device);
  double* ptrs[] = {M->Kv, M->Kfull, M->cvec, M->proj, M->r, M->lin_val, M->lin_b, M->lin_norm, M->sb_lohi, M->dval, M->dnorm, M->jac};
  for (double* p : ptrs)
    if (p) (void)hipFree(p);
  if (M->lin_col) (void)hipFree(M->lin_col);
  if (M->dcol) (void)hipFree(M->dcol);
  if (M->h_in) (void)hipHostFree(M->h_in);
  if (M->h_out) (void)hipHostFree(M->h_out);
  if (M->h_flag) (void)hipHostFree(M->h_flag);
  delete M;
  return KP_OK;
}

static size_t nmpc_lds_bytes(const kp_nmpc* M) {
  return (size_t)nmpc_layout(M->nz, M->m, M->Np, M->nproj, M->basis->dev.nfull, nmpc_rows(M)).total * 8;
}

extern "C" int kp_nmpc_create(kp_ctx* ctx, const kp_basis* basis, const double* Kf, int Np, const double* proj, int nproj,
                              double q_run, double q_term, const double* r, const double* lo, const double* hi, double slope_lim,
                              double smooth_lim, kp_nmpc** out) {
  if (!ctx || !out) return KP_ERR_ARG;
  *out = nullptr;
  if (!basis || !Kf || !proj || !r || Np < 1 || nproj < 1) return ctx->fail(KP_ERR_ARG, "kp_nmpc_create: bad argument");
  const BasisDev& bd = basis->dev;
  if (bd.model_type != KP_MODEL_NONLINEAR)
    return ctx->fail(KP_ERR_ARG, "kp_nmpc_create: the dictionary must be of the nonlinear model type (F(zeta, u) = Kf econ_full([zeta; u]))");
  if ((lo == nullptr) != (hi == nullptr)) return ctx->fail(KP_ERR_ARG, "kp_nmpc_create: lo and hi must both be given or both NULL");
  const int nz = bd.nzeta, m = bd.m, nv = bd.nvars, N = bd.N, nfull = bd.nfull, nU = m * Np;
  if (nU > QP_MAXN) return ctx->fail(KP_ERR_ARG, "kp_nmpc_create: m*horizon = " + std::to_string(nU) + " must be <= 64 (the QP limit)");
  KP_HIP(ctx, hipSetDevice(ctx->device));
  // fold econ_full into F(v) = Kv v + Kfull full(v) + c
  std::vector<double> Kv((size_t)nz * nv, 0.0), Kfu((size_t)nz * nfull, 0.0), cv(nz, 0.0);
  if (bd.k_pcs == 0) {
    std::copy(Kf, Kf + (size_t)nz * nfull, Kfu.begin());
  } else {
    const int kp = bd.k_pcs;
    std::vector<double> pcs((size_t)nfull * kp);
    KP_HIP(ctx, hipMemcpy(pcs.data(), bd.pcs, pcs.size() * 8, hipMemcpyDeviceToHost));
    for (int r_ = 0; r_ < nz; ++r_) {
      for (int i = 0; i < nv; ++i) Kv[r_ + (size_t)i * nz] = Kf[r_ + (size_t)i * nz];
      cv[r_] = Kf[r_ + (size_t)(N - 1) * nz];
      for (int c = 0; c < nfull; ++c) {
        double s = 0.0;
        for (int p = 0; p < kp; ++p) s += Kf[r_ + (size_t)(nv + p) * nz] * pcs[c + (size_t)p * nfull];
        Kfu[r_ + (size_t)c * nz] = s;
      }
    }
  }
  // linear rows over U = [u_1; ...; u_Np] in the order of get_constraintMatrices_nonlinear (Kmpc.m:960-1030), then the tack rows
  const bool has_slope = !std::isnan(slope_lim) && Np >= 2, has_smooth = !std::isnan(smooth_lim) && Np >= 3;
  const int nb = lo ? 2 * m * Np : 0, ns = has_slope ? 2 * m * (Np - 1) : 0, nsm = has_smooth ? 2 * m * (Np - 2) : 0;
  const int nlin = nb + ns + nsm + 2 * m;
  std::vector<double> A((size_t)nlin * nU, 0.0), bl(nlin, 0.0);
  auto at = [&](int row, int col) -> double& { return A[(size_t)col * nlin + row]; };
  int row0 = 0;
  if (lo) {     // kron(I_Np, [-I; I]) (:964-981): every input, the pinned u_1 included
    for (int j = 0; j < Np; ++j)
      for (int i = 0; i < m; ++i) {
        at(row0 + j * 2 * m + i, j * m + i) = -1.0;
        bl[row0 + j * 2 * m + i] = -lo[i];
        at(row0 + j * 2 * m + m + i, j * m + i) = 1.0;
        bl[row0 + j * 2 * m + m + i] = hi[i];
      }
    row0 += nb;
  }
  if (has_slope) {   // [u_{j+1} - u_j; -(u_{j+1} - u_j)] <= slope_lim (:984-1000)
    const int h = m * (Np - 1);
    for (int j = 0; j < Np - 1; ++j)
      for (int i = 0; i < m; ++i) {
        const int rr = j * m + i;
        at(row0 + rr, j * m + i) = -1.0;
        at(row0 + rr, (j + 1) * m + i) = 1.0;
        at(row0 + h + rr, j * m + i) = 1.0;
        at(row0 + h + rr, (j + 1) * m + i) = -1.0;
        bl[row0 + rr] = slope_lim;
        bl[row0 + h + rr] = slope_lim;
      }
    row0 += ns;
  }
  if (has_smooth) {  // u_j - 2 u_{j+1} + u_{j+2} (:1003-1018).  The reference writes the middle block as -2*Fslope_i, which
                     // exists only when a slope constraint is set too; -2 I is its evident intent and is used here
    const int h = m * (Np - 2);
    for (int j = 0; j < Np - 2; ++j)
      for (int i = 0; i < m; ++i) {
        const int rr = j * m + i;
        at(row0 + rr, j * m + i) = 1.0;
        at(row0 + rr, (j + 1) * m + i) = -2.0;
        at(row0 + rr, (j + 2) * m + i) = 1.0;
        at(row0 + h + rr, j * m + i) = -1.0;
        at(row0 + h + rr, (j + 1) * m + i) = 2.0;
        at(row0 + h + rr, (j + 2) * m + i) = -1.0;
        bl[row0 + rr] = smooth_lim;
        bl[row0 + h + rr] = smooth_lim;
      }
    row0 += nsm;
  }
  for (int i = 0; i < m; ++i) {   // u_1 = u_prev (Aeq, :1149-1152) as u_1 <= u_prev, -u_1 <= -u_prev
    at(row0 + i, i) = 1.0;
    at(row0 + m + i, i) = -1.0;
  }
  std::vector<double> ev, en;
  std::vector<int> ec;
  int K = 1;
  for (int rr = 0; rr < nlin; ++rr) {
    int c = 0;
    for (int j = 0; j < nU; ++j) c += at(rr, j) != 0.0;
    K = std::max(K, c);
  }
  ev.assign((size_t)K * nlin, 0.0);
  ec.assign((size_t)K * nlin, 0);
  en.assign(nlin, 0.0);
  for (int rr = 0; rr < nlin; ++rr) {
    int k = 0;
    double s = 0.0;
    for (int j = 0; j < nU; ++j)
      if (at(rr, j) != 0.0) {
        ev[(size_t)k * nlin + rr] = at(rr, j);
        ec[(size_t)k * nlin + rr] = j;
        s += at(rr, j) * at(rr, j);
        ++k;
      }
    en[rr] = std::sqrt(s);
  }
  kp_nmpc* M = new kp_nmpc();
  M->ctx = ctx; M->basis = basis;
  M->nz = nz; M->m = m; M->nv = nv; M->Np = Np; M->nproj = nproj; M->nU = nU; M->nlin = nlin; M->linK = K;
  M->q_run = q_run; M->q_term = q_term;
  const size_t lds = nmpc_lds_bytes(M);
  if (lds > NMPC_LDS_MAX) {
    delete M;
    return ctx->fail(KP_ERR_ARG, "kp_nmpc_create: the step's workspace (" + std::to_string(lds) + " bytes) exceeds the " +
                                     std::to_string(NMPC_LDS_MAX) + " bytes of LDS");
  }
  int rc = kp_dev_alloc_copy(ctx, &M->Kv, Kv.data(), Kv.size());
  if (!rc) rc = kp_dev_alloc_copy(ctx, &M->Kfull, Kfu.data(), Kfu.size());
  if (!rc) rc = kp_dev_alloc_copy(ctx, &M->cvec, cv.data(), cv.size());
  if (!rc) rc = kp_dev_alloc_copy(ctx, &M->proj, proj, (size_t)nproj * nz);
  if (!rc) rc = kp_dev_alloc_copy(ctx, &M->r, r, m);
  if (!rc) rc = kp_dev_alloc_copy(ctx, &M->lin_val, ev.data(), ev.size());
  if (!rc) rc = kp_dev_alloc_copy(ctx, &M->lin_b, bl.data(), bl.size());
  if (!rc) rc = kp_dev_alloc_copy(ctx, &M->lin_norm, en.data(), en.size());
  if (!rc) rc = kp_dev_alloc_copy(ctx, &M->jac, nullptr, (size_t)Np * nz * nv);
  if (!rc) {
    hipError_t e = hipMalloc((void**)&M->lin_col, ec.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(M->lin_col, ec.data(), ec.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = ctx->fail(KP_ERR_HIP, std::string("kp_nmpc_create: ") + hipGetErrorString(e));
  }
  if (rc) {
    kp_nmpc_destroy(M);
    return rc;
  }
  *out = M;
  return KP_OK;
}

extern "C" int kp_nmpc_set_state_bounds(kp_nmpc* M, int n, const double* lo, const double* hi) {
  if (!M) return KP_ERR_ARG;
  kp_ctx* ctx = M->ctx;
  if (n == 0) {
    M->sb = 0;
    return KP_OK;
  }
  if (n != M->nz || !lo || !hi) return ctx->fail(KP_ERR_ARG, "kp_nmpc_set_state_bounds: n must be nzeta = " + std::to_string(M->nz) + " (or 0)");
  const int sb_old = M->sb;
  M->sb = 1;
  const size_t lds = nmpc_lds_bytes(M);
  if (lds > NMPC_LDS_MAX) {
    M->sb = sb_old;
    return ctx->fail(KP_ERR_ARG, "kp_nmpc_set_state_bounds: with the state rows the step's workspace (" + std::to_string(lds) +
                                     " bytes) exceeds the " + std::to_string(NMPC_LDS_MAX) + " bytes of LDS");
  }
  KP_HIP(ctx, hipSetDevice(ctx->device));
  std::vector<double> lh(2 * (size_t)n);
  std::copy(lo, lo + n, lh.begin());
  std::copy(hi, hi + n, lh.begin() + n);
  if (!M->sb_lohi) KP_HIP(ctx, hipMalloc((void**)&M->sb_lohi, 2 * (size_t)M->nz * 8));
  KP_HIP(ctx, hipMemcpy(M->sb_lohi, lh.data(), lh.size() * 8, hipMemcpyHostToDevice));
  return KP_OK;
}

extern "C" int kp_nmpc_set_options(kp_nmpc* M, int max_iter, double tol_kkt, double tol_step, double damping) {
  if (!M) return KP_ERR_ARG;
  if (max_iter < 1 || !(tol_kkt > 0.0) || !(tol_step > 0.0) || !(damping >= 0.0))
    return M->ctx->fail(KP_ERR_ARG, "kp_nmpc_set_options: max_iter >= 1, positive tolerances and damping >= 0 required");
  M->damping = damping;
  M->max_iter = max_iter;
  M->tol_kkt = tol_kkt;
  M->tol_step = tol_step;
  return KP_OK;
}

// State bounds: the dense constraint rows of every problem (or trial) of a launch.
static int nmpc_ensure_dense(kp_nmpc* M, int nb) {
  kp_ctx* ctx = M->ctx;
  const int nU = M->nU, mr = nmpc_rows(M);
  if (M->sb && M->dense_problems < (size_t)nb) {
    if (M->dval) (void)hipFree(M->dval);
    if (M->dnorm) (void)hipFree(M->dnorm);
    if (M->dcol) (void)hipFree(M->dcol);
    M->dval = M->dnorm = nullptr;
    M->dcol = nullptr;
    M->dense_problems = 0;
    // (the column table is sized for the largest row count: with state bounds mr is fixed by the controller)
    KP_HIP(ctx, hipMalloc((void**)&M->dval, (size_t)nb * mr * nU * 8));
    KP_HIP(ctx, hipMalloc((void**)&M->dnorm, (size_t)nb * mr * 8));
    KP_HIP(ctx, hipMalloc((void**)&M->dcol, (size_t)mr * nU * 4));
    std::vector<int> col((size_t)mr * nU);
    for (int k = 0; k < nU; ++k)
      for (int row = 0; row < mr; ++row) col[(size_t)k * mr + row] = k;
    KP_HIP(ctx, hipMemcpy(M->dcol, col.data(), col.size() * 4, hipMemcpyHostToDevice));
    M->dense_problems = nb;
  }
  return KP_OK;
}

extern "C" int kp_nmpc_step_batch(kp_nmpc* M, int nb, const double* zeta, const double* u_prev, const double* Yr, const double* U_init,
                                  double* U_out, double* Z_out, double* info, int* status) {
  if (!M) return KP_ERR_ARG;
  kp_ctx* ctx = M->ctx;
  if (nb < 1 || !zeta || !u_prev || !Yr || !U_out) return ctx->fail(KP_ERR_ARG, "kp_nmpc_step: bad argument");
  KP_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->async_pending) {
    int rc0 = kp_synchronize(ctx);
    if (rc0) return rc0;
  }
  const int nz = M->nz, m = M->m, Np = M->Np, nproj = M->nproj, nU = M->nU, mr = nmpc_rows(M);
  const int nyr = nproj * (Np + 1);
  const int in_per = nm_even(nz + m + nyr + 1 + nU), out_per = nm_even(nU + (Np + 1) * nz + 2);
  if (M->io_problems < (size_t)nb) {
    if (M->h_in) (void)hipHostFree(M->h_in);
    if (M->h_out) (void)hipHostFree(M->h_out);
    M->h_in = M->h_out = nullptr;
    M->io_problems = 0;
    KP_HIP(ctx, hipHostMalloc((void**)&M->h_in, (size_t)nb * in_per * 8, hipHostMallocDefault));
    KP_HIP(ctx, hipHostMalloc((void**)&M->h_out, (size_t)nb * out_per * 8 + (size_t)nb * sizeof(int) + 8, hipHostMallocDefault));
    M->io_problems = nb;
  }
  M->h_status = (int*)(M->h_out + M->io_problems * out_per);
  if (int rcd = nmpc_ensure_dense(M, nb)) return rcd;
  for (int p = 0; p < nb; ++p) {
    double* in = M->h_in + (size_t)p * in_per;
    memcpy(in, zeta + (size_t)p * nz, (size_t)nz * 8);
    memcpy(in + nz, u_prev + (size_t)p * m, (size_t)m * 8);
    memcpy(in + nz + m, Yr + (size_t)p * nyr, (size_t)nyr * 8);
    in[nz + m + nyr] = U_init ? 1.0 : 0.0;
    if (U_init)   // Np x m column-major -> x = [u_1; u_2; ...]
      for (int j = 0; j < Np; ++j)
        for (int i = 0; i < m; ++i) in[nz + m + nyr + 1 + j * m + i] = U_init[(size_t)p * nU + (size_t)i * Np + j];
  }
  NmpcArgs a{};
  a.b = M->basis->dev;
  a.nz = nz; a.m = m; a.nv = M->nv; a.Np = Np; a.nproj = nproj; a.nU = nU; a.nlin = M->nlin; a.mr = mr; a.sb = M->sb;
  a.max_iter = M->max_iter;
  a.q_run = M->q_run; a.q_term = M->q_term; a.tol_kkt = M->tol_kkt; a.tol_step = M->tol_step;
  a.damping = M->damping;
  a.Kv = M->Kv; a.Kfull = M->Kfull; a.cvec = M->cvec; a.proj = M->proj; a.r = M->r; a.sb_lohi = M->sb_lohi;
  a.lin = EllMat{M->lin_val, M->lin_col, M->lin_norm, M->linK};
  a.lin_b = M->lin_b;
  a.dval = M->dval; a.dcol = M->dcol; a.dnorm = M->dnorm;
  a.in = M->h_in; a.in_per = in_per; a.out = M->h_out; a.out_per = out_per; a.status = M->h_status;
  a.jac_out = nb == 1 ? M->jac : nullptr;
  a.L = nmpc_layout(nz, m, Np, nproj, a.b.nfull, mr);
  const size_t lds = (size_t)a.L.total * 8;
  if (lds > NMPC_LDS_MAX) return ctx->fail(KP_ERR_ARG, "kp_nmpc_step: the step's workspace exceeds the LDS budget");
  // a single step: the kernel stores a sequence number behind its outputs and the host spins on it (as kp_mpc_step)
  const bool spin = nb == 1;
  if (spin) {
    if (!M->h_flag) {
      KP_HIP(ctx, hipHostMalloc((void**)&M->h_flag, 64, hipHostMallocDefault));
      memset(M->h_flag, 0, 64);
    }
    a.done_flag = M->h_flag;
    a.done_seq = ++M->step_seq;
  }
  static KpLdsCache lds_c;
  KP_HIP(ctx, kp_ensure_lds(lds_c, (const void*)kp_nmpc_kernel, lds));
  hipLaunchKernelGGL(kp_nmpc_kernel, dim3(nb), dim3(256), lds, ctx->stream, a);
  KP_HIP(ctx, hipGetLastError());
  bool spun = false;
  if (spin) {
    volatile unsigned long long* fl = M->h_flag;
    for (long it = 0; it < 20000000L; ++it) {       // a slower step falls through to the stream wait
      if (__atomic_load_n(&fl[0], __ATOMIC_ACQUIRE) == a.done_seq) { spun = true; break; }
      __builtin_ia32_pause();
    }
  }
  if (!spun) KP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int p = 0; p < nb; ++p) {
    const double* o = M->h_out + (size_t)p * out_per;
    for (int j = 0; j < Np; ++j)
      for (int i = 0; i < m; ++i) U_out[(size_t)p * nU + (size_t)i * Np + j] = o[j * m + i];
    if (Z_out) memcpy(Z_out + (size_t)p * (Np + 1) * nz, o + nU, (size_t)(Np + 1) * nz * 8);
    if (info) { info[2 * (size_t)p] = o[nU + (Np + 1) * nz]; info[2 * (size_t)p + 1] = o[nU + (Np + 1) * nz + 1]; }
    if (status) status[p] = M->h_status[p];
  }
  return KP_OK;
}

extern "C" int kp_nmpc_step(kp_nmpc* M, const double* zeta, const double* u_prev, const double* Yr, const double* U_init,
                            double* U_out, double* Z_out, double* info, int* status) {
  return kp_nmpc_step_batch(M, 1, zeta, u_prev, Yr, U_init, U_out, Z_out, info, status);
}

// Whole closed loops, one workgroup per trial (kp_nmpc_sim_kernel); the host transfers are kp_sim_loop.h's.
extern "C" int kp_nmpc_simulate(kp_nmpc* M, int nb, int nref, const double* ref, int ref_shared, const double* y0, const double* u0,
                                int warm, double* U, double* Y, double* info, int* steps_done, int* status) {
  if (!M) return KP_ERR_ARG;
  kp_ctx* ctx = M->ctx;
  if (nb < 1 || nref < 1)
    return ctx->fail(KP_ERR_ARG, "kp_nmpc_simulate: nb and nref must be at least 1 (nb = " + std::to_string(nb) + ", nref = " +
                                     std::to_string(nref) + ")");
  if (!ref || !y0 || !u0 || !U || !Y || !steps_done || !status)
    return ctx->fail(KP_ERR_ARG, "kp_nmpc_simulate: NULL argument (only info may be NULL)");
  const int nz = M->nz, m = M->m, Np = M->Np, nproj = M->nproj, nUv = M->nU, mr = nmpc_rows(M);
  if (Np < 2) return ctx->fail(KP_ERR_ARG, "kp_nmpc_simulate: the loop applies the second row of the solution: horizon >= 2");
  NmpcSimArgs sa{};
  NmpcArgs a{};
  a.L = nmpc_layout(nz, m, Np, nproj, M->basis->dev.nfull, mr);
  sa.sim_off = a.L.total;
  const size_t ref_doubles = (((size_t)nref + Np) * nproj + 1) & ~(size_t)1;
  const size_t lds = ((size_t)a.L.total + ref_doubles) * 8;
  if (lds > NMPC_LDS_MAX)
    return ctx->fail(KP_ERR_ARG, "kp_nmpc_simulate: the step's workspace and a reference of " + std::to_string(nref) + " rows need " +
                                     std::to_string(lds) + " bytes of LDS (" + std::to_string(NMPC_LDS_MAX) + " at most)");
  KP_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->async_pending) {
    int rc0 = kp_synchronize(ctx);
    if (rc0) return rc0;
  }
  if (int rcd = nmpc_ensure_dense(M, nb)) return rcd;
  a.b = M->basis->dev;
  a.nz = nz; a.m = m; a.nv = M->nv; a.Np = Np; a.nproj = nproj; a.nU = nUv; a.nlin = M->nlin; a.mr = mr; a.sb = M->sb;
  a.max_iter = M->max_iter;
  a.q_run = M->q_run; a.q_term = M->q_term; a.tol_kkt = M->tol_kkt; a.tol_step = M->tol_step;
  a.damping = M->damping;
  a.Kv = M->Kv; a.Kfull = M->Kfull; a.cvec = M->cvec; a.proj = M->proj; a.r = M->r; a.sb_lohi = M->sb_lohi;
  a.lin = EllMat{M->lin_val, M->lin_col, M->lin_norm, M->linK};
  a.lin_b = M->lin_b;
  a.dval = M->dval; a.dcol = M->dcol; a.dnorm = M->dnorm;
  sa.warm = warm ? 1 : 0;
  KpSimLoop& S = sa.loop;
  S.nref = nref; S.ny = nz; S.m = m; S.nproj = nproj; S.Np = Np; S.ref_shared = ref_shared ? 1 : 0; S.aux_w = info ? 3 : 0;
  KpSimIo io;
  if (int rcu = kp_sim_upload(ctx, "kp_nmpc_simulate", nb, ref, y0, u0, S, io)) return rcu;
  hipStream_t s = ctx->stream;
  static KpLdsCache sim_lds;
  KP_HIP(ctx, kp_ensure_lds(sim_lds, (const void*)kp_nmpc_sim_kernel, lds));
  KP_HIP(ctx, hipEventRecord(ctx->evp[4], s));
  hipLaunchKernelGGL(kp_nmpc_sim_kernel, dim3(nb), dim3(256), lds, s, a, sa);
  KP_HIP(ctx, hipGetLastError());
  KP_HIP(ctx, hipEventRecord(ctx->evp[5], s));
  if (int rcd = kp_sim_download(ctx, io, S, U, Y, info, steps_done, status)) return rcd;
  float ms = 0;
  if (hipEventElapsedTime(&ms, ctx->evp[4], ctx->evp[5]) == hipSuccess) ctx->timers[21] = ms;
  return KP_OK;
}

extern "C" int kp_nmpc_last_jacobians(kp_nmpc* M, double* J) {
  if (!M || !J) return KP_ERR_ARG;
  KP_HIP(M->ctx, hipSetDevice(M->ctx->device));
  KP_HIP(M->ctx, hipMemcpy(J, M->jac, (size_t)M->Np * M->nz * M->nv * 8, hipMemcpyDeviceToHost));
  return KP_OK;
}

extern "C" int kp_nmpc_dims(const kp_nmpc* M, int* nvar, int* nrows) {
  if (!M) return KP_ERR_ARG;
  if (nvar) *nvar = M->nU;
  if (nrows) *nrows = nmpc_rows(M);
  return KP_OK;
}
