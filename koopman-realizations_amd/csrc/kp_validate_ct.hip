// The validation table of continuous-time models: every candidate rolled out over every validation trial in one launch, each
// sample interval ode45 over [0, Ts] with the input held (val_model / val_BLmodel / val_NLmodel, Ksysid.m:1679-1683,
// 1777-1781, 1849-1856), the metrics of get_error (:1886-1897) reduced in the kernel.  It joins the workgroup-wide
// Dormand-Prince integrator of kp_ct_rollout.hip with the (model x trial) grid, the chunked staging and the serial-in-time
// reduction of kp_validate.hip, and replaces nmod x ntr calls of kp_rollout_ct / kp_rollout_nl_ct of one workgroup each.
//
// One workgroup per (model, trial) pair, nothing shared between pairs but the read-only models: the numbers of a pair are the
// same bits alone or in a batch.  The right-hand side, the per-sample model and the integration of a sample interval are
// kp_ct_step.h's, the code kp_ct_rollout_kernel runs, and the argument checks are kp_validate_args.h's, shared with
// kp_validate.hip.  This file keeps the grid, the LDS layout, the staging of the model and of a chunk, and the error reduction.
//   - A linear A or a nonlinear Kf of at most KP_VALIDATE_CT_STAGE doubles is staged in LDS, a larger one is read from memory
//     (L2; the models are uploaded once per call, nmod of them).  The bilinear matrix of a sample, A + sum_i u_i B_i, is private
//     to the pair: in LDS under the same limit, else in the pair's slice of a scratch buffer.
//   - Time runs in chunks of KP_VALIDATE_CT_CHUNK samples: inputs and real outputs of a chunk are staged in LDS and the
//     simulated outputs collected there, so the integration loop loads nothing of them from memory.
//
// LDS layout (doubles): y | yn | yt0 | yt1 (NS each) | k [7][NS] | red (16) | acc (4 n + 4) | yfactor (n) | Uc [m][TC] |
// Yr [n][TC + 1] | Ys [n][TC + 1] | Ec [TC] | Euc [TC] | model part.  Model part, linear and bilinear: B u (N) | staged matrix
// (N x N); nonlinear: v = [zeta; u] (nvars) | full (nfull) | lifted (N) | staged Kf (nzeta x N).
//
// Order of the reductions: that of kp_validate_kernel - behind the rollout of a chunk, thread tt forms the two Euclidean norms
// of sample tt, then thread c < n adds |d|, d^2 and min / max of yreal of column c over the chunk in ascending time, thread n
// and n + 1 the two norms likewise.  No atomics, no tree.  The statements are restated from kp_validate.hip on purpose: the
// two kernels differ in their barrier and chunk length, and a change to one reduction must be made in the other.
#include <algorithm>
#include <cmath>

#include "koopman_hip_validate.h"
#include "kp_ct_step.h"
#include "kp_internal.h"
#include "kp_validate_args.h"

namespace {

constexpr int VCT_TC = KP_VALIDATE_CT_CHUNK;
constexpr int VCT_TCP = VCT_TC + 1;   // row stride of Yr / Ys: thread c walks row c in the column reduction
constexpr size_t VCT_LDS = 160 * 1024;

struct VctArgs {
  int kind;            // 0 linear, 1 bilinear, 2 nonlinear
  int N, m, n, NS;     // model width, inputs, outputs, state length (N, or nzeta for the nonlinear model)
  int ntr, stage, want_sim;
  int64_t rows;        // all trials' rows
  double Ts, rtol, atol;
  const double* A;     // nmod x [N x N], or Kf nmod x [nzeta x N]
  const double* B;     // nmod x [N x m] or nmod x [N x N m]
  double* Ag;          // bilinear beyond the LDS staging: one N x N slice per pair
  const int64_t* off;
  const double* Z0;    // ntr x NS column-major
  const double* U;     // rows x m
  const double* Yreal; // rows x n
  const double* yfac;
  double* err;
  double* Ysim;
  int* status; int* nacc; int* nrej;
};

template <bool NL>
__global__ __launch_bounds__(256) void kp_validate_ct_kernel(VctArgs g, BasisDev bd) {
  extern __shared__ double sm[];
  const int tid = threadIdx.x, nth = blockDim.x;
  const int mod = blockIdx.x / g.ntr, tr = blockIdx.x - mod * g.ntr;
  const int NS = g.NS, N = g.N, m = g.m, n = g.n;
  const int64_t r0 = g.off[tr];
  const int T = (int)(g.off[tr + 1] - r0);
  CtStep w;
  w.N = N; w.m = m; w.NS = NS; w.kind = g.kind;
  w.y = sm;
  w.yn = w.y + NS;
  w.yt0 = w.yn + NS;                          // matrix models: two stage-input buffers
  w.yt1 = w.yt0 + NS;
  w.kk = w.yt1 + NS;                          // 7 x NS
  w.red = w.kk + 7 * NS;                      // 16
  double* acc = w.red + 16;                   // [c][sum |d|, sum d^2, min, max] | euclid | unscaled euclid | not finite
  double* fs = acc + 4 * n + 4;
  double* Uc = fs + n;
  double* Yr = Uc + m * VCT_TC;
  double* Ys = Yr + n * VCT_TCP;
  double* Ec = Ys + n * VCT_TCP;
  double* Euc = Ec + VCT_TC;
  double* extra = Euc + VCT_TC;
  w.bu = extra;
  double* Ash = w.bu + N;
  w.v = extra;
  w.full = NL ? w.v + bd.nvars : nullptr;
  w.zl = NL ? w.full + bd.nfull : nullptr;
  double* Ksh = NL ? w.zl + N : nullptr;
  const double* Ab = g.A + (size_t)mod * (NL ? (size_t)NS * N : (size_t)N * N);
  w.Ab = Ab;
  w.Bb = NL ? nullptr : g.B + (size_t)mod * N * (g.kind == 1 ? (size_t)N * m : (size_t)m);
  w.Am = Ab;
  if (!NL) {
    if (g.kind == 1) w.Am = g.stage ? Ash : g.Ag + (size_t)blockIdx.x * N * N;
    else if (g.stage) {
      for (int e = tid; e < N * N; e += nth) Ash[e] = Ab[e];
      w.Am = Ash;
    }
  } else if (g.stage) {
    for (int e = tid; e < NS * N; e += nth) Ksh[e] = Ab[e];
    w.Am = Ksh;
  }
  for (int c = tid; c < n; c += nth) {
    acc[4 * c] = 0.0;
    acc[4 * c + 1] = 0.0;
    acc[4 * c + 2] = INFINITY;
    acc[4 * c + 3] = -INFINITY;
    fs[c] = g.yfac[c];
  }
  if (tid < 3) acc[4 * n + tid] = 0.0;
  for (int r = tid; r < NS; r += nth) w.y[r] = g.Z0[tr + (size_t)r * g.ntr];
  w.rtol = g.rtol; w.thr = g.atol / g.rtol; w.Ts = g.Ts; w.hmax = 0.1 * fabs(g.Ts);

  double* Yo = g.want_sim ? g.Ysim + (size_t)mod * g.rows * n : nullptr;
  for (int t0 = 0; t0 < T; t0 += VCT_TC) {
    const int tc = min(VCT_TC, T - t0);
    // stage the inputs and the real outputs of the chunk (the previous chunk's last reader passed a barrier)
    for (int e = tid; e < m * tc; e += nth) {
      const int i = e / tc, tt = e - i * tc;
      Uc[i * VCT_TC + tt] = g.U[(size_t)i * g.rows + r0 + t0 + tt];
    }
    for (int e = tid; e < n * tc; e += nth) {
      const int i = e / tc, tt = e - i * tc;
      Yr[i * VCT_TCP + tt] = g.Yreal[(size_t)i * g.rows + r0 + t0 + tt];
    }
    __syncthreads();
    for (int tt = 0; tt < tc; ++tt) {
      const int j = t0 + tt;
      for (int r = tid; r < n; r += nth) Ys[r * VCT_TCP + tt] = j == 0 ? Yr[r * VCT_TCP] : w.y[r];   // row 0: :1654
      if (j == T - 1) break;
      if (w.failed) {
        for (int r = tid; r < NS; r += nth) w.y[r] = NAN;
        continue;
      }
      ct_sample_model<NL>(w, Uc + tt, VCT_TC);     // inputs of the sample: Uc[tt + i * VCT_TC]
      __syncthreads();
      ct_integrate<NL>(w, bd);
    }
    __syncthreads();       // the last sample leaves the loop before its barrier
    // ---- the errors of the chunk (kp_validate_kernel) ----
    for (int tt = tid; tt < tc; tt += nth) {
      double e2 = 0.0, eu2 = 0.0;
      bool bad = false;
      for (int c = 0; c < n; ++c) {
        const double ys = Ys[c * VCT_TCP + tt];
        const double dd = ys - Yr[c * VCT_TCP + tt];
        const double du = dd * fs[c];
        e2 += dd * dd;
        eu2 += du * du;
        bad = bad || !isfinite(ys);
      }
      Ec[tt] = sqrt(e2);
      Euc[tt] = sqrt(eu2);
      if (bad) acc[4 * n + 2] = 1.0;
    }
    if (g.want_sim)
      for (int e = tid; e < n * tc; e += nth) {
        const int c = e / tc, tt = e - c * tc;
        Yo[(size_t)c * g.rows + r0 + t0 + tt] = Ys[c * VCT_TCP + tt];
      }
    __syncthreads();
    for (int c = tid; c < n + 2; c += nth) {
      if (c < n) {
        double sa = acc[4 * c], sq = acc[4 * c + 1], mn = acc[4 * c + 2], mx = acc[4 * c + 3];
        for (int tt = 0; tt < tc; ++tt) {
          const double yr = Yr[c * VCT_TCP + tt];
          const double dd = Ys[c * VCT_TCP + tt] - yr;
          sa += fabs(dd);
          sq += dd * dd;
          mn = fmin(mn, yr);
          mx = fmax(mx, yr);
        }
        acc[4 * c] = sa; acc[4 * c + 1] = sq; acc[4 * c + 2] = mn; acc[4 * c + 3] = mx;
      } else {
        const double* E = c == n ? Ec : Euc;
        double s = acc[4 * n + (c - n)];
        for (int tt = 0; tt < tc; ++tt) s += E[tt];
        acc[4 * n + (c - n)] = s;
      }
    }
    __syncthreads();
  }
  double* eo = g.err + (size_t)blockIdx.x * (3 * n + 2);
  const double Td = (double)T;
  for (int c = tid; c < n; c += nth) {
    const double rmse = sqrt(acc[4 * c + 1] / Td);
    eo[c] = acc[4 * c] / Td;
    eo[n + c] = rmse;
    eo[2 * n + c] = rmse / fabs(acc[4 * c + 3] - acc[4 * c + 2]);
  }
  if (tid == 0) {
    eo[3 * n] = acc[4 * n] / Td;
    eo[3 * n + 1] = acc[4 * n + 1] / Td;
    g.status[blockIdx.x] = (w.failed || acc[4 * n + 2] != 0.0) ? 1 : 0;
    g.nacc[blockIdx.x] = w.nacc;
    g.nrej[blockIdx.x] = w.nrej;
  }
}

}  // namespace

extern "C" int kp_validate_ct(kp_ctx* ctx, const kp_basis* basis, int model_type, int N, int m, int n, int nzeta, int nw, int nmod,
                              const double* A, const double* B, int ntr, const int64_t* trial_off, const double* zeta0, const double* U,
                              const double* Yreal, const double* Wl, const double* yfactor, int want_sim, double Ts, double rtol,
                              double atol, double* err_out, int* status_out, double* Ysim, int* naccept, int* nreject) {
  if (!ctx) return KP_ERR_ARG;
  const int rc_arg = val_check_args(ctx, "kp_validate_ct", basis, model_type, N, m, n, nzeta, nw, nmod, A, B, ntr, trial_off, zeta0, U,
                                    Yreal, yfactor, want_sim, err_out, status_out, Ysim);
  if (rc_arg) return rc_arg;
  if (nw != 0) return ctx->fail(KP_ERR_ARG, "kp_validate_ct: loaded continuous-time models are not supported (nw must be 0)");
  if (!ct_tol_ok(Ts, rtol, atol)) return ctx->fail(KP_ERR_ARG, "kp_validate_ct: Ts, rtol and atol must be positive and finite");
  if (N > 512) return ctx->fail(KP_ERR_ARG, "kp_validate_ct: N must be at most 512");
  const bool nl = model_type == KP_MODEL_NONLINEAR, bil = model_type == KP_MODEL_BILINEAR;
  const BasisDev& b = basis->dev;
  const int64_t rows = trial_off[ntr];
  const size_t NS = nl ? nzeta : N;

  // LDS: what every pair needs - 11 state vectors, the error sums, one chunk, the model part's vectors - then the matrix
  const size_t vecs = nl ? (size_t)b.nvars + b.nfull + N : (size_t)N;
  const size_t fixed = 11 * NS + 16 + 4 * (size_t)n + 4 + n + (size_t)m * VCT_TC + 2 * (size_t)n * VCT_TCP + 2 * VCT_TC + vecs;
  if (fixed * 8 > VCT_LDS)
    return ctx->fail(KP_ERR_ARG, "kp_validate_ct: the state vectors, the stages and one chunk of " + std::to_string(VCT_TC) +
                                     " samples need " + std::to_string(fixed * 8) + " bytes of LDS, the limit is " + std::to_string(VCT_LDS));
  const size_t model_lds = nl ? NS * N : (size_t)N * N;
  const int stage = model_lds <= (size_t)KP_VALIDATE_CT_STAGE && (fixed + model_lds) * 8 <= VCT_LDS;
  const size_t lds = (fixed + (stage ? model_lds : 0)) * 8;

  KP_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->async_pending) {
    int rc0 = kp_synchronize(ctx);
    if (rc0) return rc0;
  }
  const size_t npairs = (size_t)nmod * ntr;
  const size_t mbc = nl ? 0 : (bil ? (size_t)m * N : (size_t)m);
  const size_t nA = (size_t)nmod * (nl ? (size_t)nzeta * N : (size_t)N * N), nB = (size_t)nmod * N * mbc;
  const size_t nz0 = (size_t)ntr * nzeta, nU = (size_t)rows * m, nY = (size_t)rows * n;
  const size_t nZ0 = nl ? 0 : (size_t)ntr * N, nE = npairs * (3 * (size_t)n + 2), nS = want_sim ? (size_t)nmod * rows * n : 0;
  const size_t nAg = (bil && !stage) ? npairs * N * N : 0;
  const size_t bytes = (nA + nB + nz0 + nU + nY + n + nZ0 + nE + nS + nAg) * 8 + (size_t)(ntr + 1) * 8 + 3 * npairs * 4 + 64;
  double* ws = (double*)ctx->workspace(6, bytes);
  if (!ws) return ctx->fail(KP_ERR_HIP, "kp_validate_ct: out of device memory (" + std::to_string(bytes) + " bytes)");
  double *dA = ws, *dB = dA + nA, *dz0 = dB + nB, *dU = dz0 + nz0, *dY = dU + nU, *df = dY + nY, *dZ0 = df + n, *dE = dZ0 + nZ0,
         *dS = dE + nE, *dAg = dS + nS;
  int64_t* dOff = (int64_t*)(dAg + nAg);
  int* dSt = (int*)(dOff + ntr + 1);
  hipStream_t s = ctx->stream;
  KP_HIP(ctx, hipMemcpyAsync(dA, A, nA * 8, hipMemcpyHostToDevice, s));
  if (nB) KP_HIP(ctx, hipMemcpyAsync(dB, B, nB * 8, hipMemcpyHostToDevice, s));
  KP_HIP(ctx, hipMemcpyAsync(dz0, zeta0, nz0 * 8, hipMemcpyHostToDevice, s));
  if (nU) KP_HIP(ctx, hipMemcpyAsync(dU, U, nU * 8, hipMemcpyHostToDevice, s));
  KP_HIP(ctx, hipMemcpyAsync(dY, Yreal, nY * 8, hipMemcpyHostToDevice, s));
  KP_HIP(ctx, hipMemcpyAsync(df, yfactor, (size_t)n * 8, hipMemcpyHostToDevice, s));
  KP_HIP(ctx, hipMemcpyAsync(dOff, trial_off, (size_t)(ntr + 1) * 8, hipMemcpyHostToDevice, s));
  KP_HIP(ctx, hipEventRecord(ctx->ev0, s));
  if (!nl) {                                                       // z_0 = econ_full(zeta0) of every trial, by the lift kernel
    int rc = kp_lift_dev(ctx, basis, KP_LIFT_ECON, dz0, nullptr, ntr, dZ0);
    if (rc) return rc;
  }
  VctArgs g{};
  g.kind = nl ? 2 : (bil ? 1 : 0);
  g.N = N; g.m = m; g.n = n; g.NS = (int)NS; g.ntr = ntr; g.stage = stage; g.want_sim = want_sim; g.rows = rows;
  g.Ts = Ts; g.rtol = rtol; g.atol = atol;
  g.A = dA; g.B = dB; g.Ag = dAg; g.off = dOff; g.Z0 = nl ? dz0 : dZ0; g.U = dU; g.Yreal = dY; g.yfac = df;
  g.err = dE; g.Ysim = dS; g.status = dSt; g.nacc = dSt + npairs; g.nrej = dSt + 2 * npairs;
  // 64 or 256 threads by the widest per-stage loop, as kp_rollout_ct / kp_rollout_nl_ct choose
  const int nth = (N <= 64 && (!nl || b.nfull <= 64)) ? 64 : 256;
  static KpLdsCache c0, c1;
  if (nl) {
    KP_HIP(ctx, kp_ensure_lds(c1, (const void*)kp_validate_ct_kernel<true>, VCT_LDS));
    hipLaunchKernelGGL(kp_validate_ct_kernel<true>, dim3((unsigned)npairs), dim3(nth), lds, s, g, b);
  } else {
    BasisDev b0{};
    KP_HIP(ctx, kp_ensure_lds(c0, (const void*)kp_validate_ct_kernel<false>, VCT_LDS));
    hipLaunchKernelGGL(kp_validate_ct_kernel<false>, dim3((unsigned)npairs), dim3(nth), lds, s, g, b0);
  }
  KP_HIP(ctx, hipGetLastError());
  KP_HIP(ctx, hipEventRecord(ctx->ev1, s));
  KP_HIP(ctx, hipMemcpyAsync(err_out, dE, nE * 8, hipMemcpyDeviceToHost, s));
  KP_HIP(ctx, hipMemcpyAsync(status_out, g.status, npairs * 4, hipMemcpyDeviceToHost, s));
  if (naccept) KP_HIP(ctx, hipMemcpyAsync(naccept, g.nacc, npairs * 4, hipMemcpyDeviceToHost, s));
  if (nreject) KP_HIP(ctx, hipMemcpyAsync(nreject, g.nrej, npairs * 4, hipMemcpyDeviceToHost, s));
  if (nS) KP_HIP(ctx, hipMemcpyAsync(Ysim, dS, nS * 8, hipMemcpyDeviceToHost, s));
  KP_HIP(ctx, hipStreamSynchronize(s));
  float ms = 0;
  (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
  ctx->timers[5] = ms;
  return KP_OK;
}
