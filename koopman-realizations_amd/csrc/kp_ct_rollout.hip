// Continuous-time validation rollouts (koopman_hip_ct.h): every sample interval of val_model / val_BLmodel / val_NLmodel
// (Ksysid.m:1679-1683, 1777-1781, 1849-1856) is ode45 over [0, Ts] with the input held, from the end point of the previous one.
// The integrator is kp_ct_step.h's workgroup-wide ode45 (right-hand side, per-sample model, step control), which
// kp_validate_ct.hip runs as well; this file keeps the LDS layout, the staging of the model and the inputs, and the outputs.
//
// One workgroup per rollout.  The steps are serial, so everything a stage touches lives in LDS: the state, the seven stages,
// the inputs of a chunk of samples and, when it fits, the model (for a bilinear model the matrix A + sum_i u_i B_i of the
// sample, formed once per sample; in global memory beyond 90 states, where B streams from L2).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "koopman_hip_ct.h"
#include "kp_ct_step.h"
#include "kp_internal.h"

namespace {

constexpr int CT_TC = 256;            // samples of input staged per chunk
constexpr int CT_STAGE = 8192;        // doubles of model staged in LDS (N <= 90)

struct CtArgs {
  int kind;            // 0 linear, 1 bilinear, 2 nonlinear
  int N, m, NS;        // model width, inputs, state length (N, or nzeta for the nonlinear model)
  int T, n_out;
  double Ts, rtol, atol;
  const double* A;     // linear / bilinear: batch x N x N; nonlinear: Kf batch x [nzeta x N]
  const double* B;     // batch x N x mb
  double* Ag;          // bilinear beyond the LDS staging: batch x N x N scratch of A + sum u_i B_i
  const double* z0;    // batch x NS
  const double* U;     // batch x [T x m]
  double* Y;           // batch x [T x n_out]
  int* nacc; int* nrej; int* status;
  int stageA, tc;
};

template <bool NL>
__global__ __launch_bounds__(256) void kp_ct_rollout_kernel(CtArgs g, BasisDev bd) {
  extern __shared__ double sm[];
  const int tid = threadIdx.x, nth = blockDim.x, bi = blockIdx.x;
  const int NS = g.NS, N = g.N, m = g.m, T = g.T;
  CtStep w;
  w.N = N; w.m = m; w.NS = NS; w.kind = g.kind;
  w.y = sm;
  w.yn = w.y + NS;
  w.yt0 = w.yn + NS;                          // matrix models: two stage-input buffers
  w.yt1 = w.yt0 + NS;
  w.kk = w.yt1 + NS;                          // 7 x NS
  w.red = w.kk + 7 * NS;                      // 16
  double* Uc = w.red + 16;                    // m x tc
  double* extra = Uc + (size_t)m * g.tc;
  // matrix models: bu (N) then the staged matrix; nonlinear: v (nvars), full (nfull), zl (N), staged Kf
  w.bu = extra;
  double* Ash = w.bu + N;
  w.v = extra;
  w.full = NL ? w.v + bd.nvars : nullptr;
  w.zl = NL ? w.full + bd.nfull : nullptr;
  double* Ksh = NL ? w.zl + N : nullptr;
  const double* Ab = g.A + (size_t)bi * (NL ? (size_t)NS * N : (size_t)N * N);
  w.Ab = Ab;
  w.Bb = NL ? nullptr : g.B + (size_t)bi * N * (g.kind == 1 ? (size_t)N * m : (size_t)m);
  const double* Ub = g.U + (size_t)bi * T * m;
  double* Yb = g.Y + (size_t)bi * T * g.n_out;
  w.Am = Ab;
  if (!NL) {
    if (g.kind == 1) w.Am = g.stageA ? Ash : g.Ag + (size_t)bi * N * N;
    else if (g.stageA) {
      for (int e = tid; e < N * N; e += nth) Ash[e] = Ab[e];
      w.Am = Ash;
    }
  } else if (g.stageA) {
    for (int e = tid; e < NS * N; e += nth) Ksh[e] = Ab[e];
    w.Am = Ksh;
  }
  for (int r = tid; r < NS; r += nth) w.y[r] = g.z0[(size_t)bi * NS + r];
  w.rtol = g.rtol; w.thr = g.atol / g.rtol; w.Ts = g.Ts; w.hmax = 0.1 * fabs(g.Ts);

  for (int j = 0; j < T; ++j) {
    for (int r = tid; r < g.n_out; r += nth) Yb[(size_t)r * T + j] = w.y[r];
    if (j == T - 1) break;
    if (w.failed) {
      for (int r = tid; r < NS; r += nth) w.y[r] = NAN;
      continue;
    }
    const int jc = j % g.tc;
    if (jc == 0) {      // stage the inputs of the next chunk of samples (the previous chunk's last reader passed a barrier)
      const int tc = min(g.tc, T - 1 - j);
      for (int e = tid; e < m * tc; e += nth) {
        const int i = e / tc, tt = e - i * tc;
        Uc[i * g.tc + tt] = Ub[(size_t)i * T + j + tt];
      }
      __syncthreads();
    }
    ct_sample_model<NL>(w, Uc + jc, g.tc);     // inputs of the sample: Uc[jc + i * tc]
    __syncthreads();
    ct_integrate<NL>(w, bd);
  }
  if (tid == 0) {
    if (g.nacc) g.nacc[bi] = w.nacc;
    if (g.nrej) g.nrej[bi] = w.nrej;
    g.status[bi] = w.failed ? KP_ERR_NOT_CONVERGED : KP_OK;
  }
}

int ct_launch(kp_ctx* ctx, const char* fn, bool nl, CtArgs g, const BasisDev* bd, int batch, const double* A, size_t nA,
              const double* B, size_t nB, const double* z0, const double* U, double* Y, int* naccept, int* nreject, int* status) {
  const size_t nz = (size_t)batch * g.NS, nU = (size_t)batch * g.T * g.m, nY = (size_t)batch * g.T * g.n_out;
  const size_t nAg = (!nl && g.kind == 1 && !g.stageA) ? (size_t)batch * g.N * g.N : 0;
  const size_t ints = ((size_t)3 * batch * 4 + 7) / 8;
  double* ws = (double*)ctx->workspace(6, (nA + nB + nz + nU + nY + nAg + ints) * 8);
  if (!ws) return ctx->fail(KP_ERR_HIP, std::string(fn) + ": out of device memory");
  double *dA = ws, *dB = dA + nA, *dz = dB + nB, *dU = dz + nz, *dY = dU + nU, *dAg = dY + nY;
  int* di = (int*)(dAg + nAg);
  hipStream_t s = ctx->stream;
  KP_HIP(ctx, hipMemcpyAsync(dA, A, nA * 8, hipMemcpyHostToDevice, s));
  if (nB) KP_HIP(ctx, hipMemcpyAsync(dB, B, nB * 8, hipMemcpyHostToDevice, s));
  KP_HIP(ctx, hipMemcpyAsync(dz, z0, nz * 8, hipMemcpyHostToDevice, s));
  if (nU) KP_HIP(ctx, hipMemcpyAsync(dU, U, nU * 8, hipMemcpyHostToDevice, s));
  g.A = dA; g.B = dB; g.Ag = dAg; g.z0 = dz; g.U = dU; g.Y = dY;
  g.nacc = di; g.nrej = di + batch; g.status = di + 2 * batch;
  // LDS: 11 state vectors, reduction slots, the input chunk, then the model part
  const size_t base = (size_t)(11 * g.NS + 16) * 8;
  size_t modl;
  int nth;
  if (!nl) {
    modl = (size_t)g.N * 8 + (g.stageA ? (size_t)g.N * g.N * 8 : 0);
    nth = g.N <= 64 ? 64 : 256;
  } else {
    modl = (size_t)(bd->nvars + bd->nfull + g.N) * 8 + (g.stageA ? (size_t)g.NS * g.N * 8 : 0);
    nth = bd->nfull <= 64 && g.N <= 64 ? 64 : 256;
  }
  const size_t budget = 128 * 1024;
  if (base + modl + (size_t)g.m * 8 > budget) return ctx->fail(KP_ERR_ARG, std::string(fn) + ": model too large for the LDS staging");
  g.tc = g.m ? (int)std::min<size_t>(CT_TC, (budget - base - modl) / ((size_t)g.m * 8)) : CT_TC;
  g.tc = std::max(1, g.tc);
  const size_t lds = base + modl + (size_t)g.m * g.tc * 8;
  static KpLdsCache c0, c1;
  BasisDev b0{};
  KP_HIP(ctx, hipEventRecord(ctx->ev0, s));
  if (nl) {
    KP_HIP(ctx, kp_ensure_lds(c1, (const void*)kp_ct_rollout_kernel<true>, budget));
    hipLaunchKernelGGL(kp_ct_rollout_kernel<true>, dim3(batch), dim3(nth), lds, s, g, *bd);
  } else {
    KP_HIP(ctx, kp_ensure_lds(c0, (const void*)kp_ct_rollout_kernel<false>, budget));
    hipLaunchKernelGGL(kp_ct_rollout_kernel<false>, dim3(batch), dim3(nth), lds, s, g, b0);
  }
  KP_HIP(ctx, hipGetLastError());
  KP_HIP(ctx, hipEventRecord(ctx->ev1, s));
  KP_HIP(ctx, hipMemcpyAsync(Y, dY, nY * 8, hipMemcpyDeviceToHost, s));
  KP_HIP(ctx, hipMemcpyAsync(status, g.status, (size_t)batch * 4, hipMemcpyDeviceToHost, s));
  if (naccept) KP_HIP(ctx, hipMemcpyAsync(naccept, g.nacc, (size_t)batch * 4, hipMemcpyDeviceToHost, s));
  if (nreject) KP_HIP(ctx, hipMemcpyAsync(nreject, g.nrej, (size_t)batch * 4, hipMemcpyDeviceToHost, s));
  KP_HIP(ctx, hipStreamSynchronize(s));
  float ms = 0;
  (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
  ctx->timers[5] = ms;
  return KP_OK;
}

}  // namespace

extern "C" int kp_rollout_ct(kp_ctx* ctx, int model_type, int batch, const double* A, const double* B, int N, int m, const double* z0,
                             const double* U, int T, int n_out, double Ts, double rtol, double atol, double* Y, int* naccept,
                             int* nreject, int* status) {
  if (!ctx || !A || !B || !z0 || !U || !Y || !status || batch < 1 || N < 1 || m < 0 || T < 1 || n_out < 1 || n_out > N)
    return ctx ? ctx->fail(KP_ERR_ARG, "kp_rollout_ct: bad argument") : KP_ERR_ARG;
  if (model_type != KP_MODEL_LINEAR && model_type != KP_MODEL_BILINEAR)
    return ctx->fail(KP_ERR_ARG, "kp_rollout_ct: linear or bilinear models only");
  if (N > 512) return ctx->fail(KP_ERR_ARG, "kp_rollout_ct: N must be at most 512");
  if (!ct_tol_ok(Ts, rtol, atol)) return ctx->fail(KP_ERR_ARG, "kp_rollout_ct: Ts, rtol and atol must be positive and finite");
  KP_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->async_pending) {
    int rc0 = kp_synchronize(ctx);
    if (rc0) return rc0;
  }
  const int bil = model_type == KP_MODEL_BILINEAR;
  CtArgs g{};
  g.kind = bil; g.N = N; g.m = m; g.NS = N; g.T = T; g.n_out = n_out; g.Ts = Ts; g.rtol = rtol; g.atol = atol;
  g.stageA = (size_t)N * N <= CT_STAGE;
  const size_t mb = bil ? (size_t)N * m : (size_t)m;
  return ct_launch(ctx, "kp_rollout_ct", false, g, nullptr, batch, A, (size_t)batch * N * N, B, (size_t)batch * N * mb, z0, U, Y,
                   naccept, nreject, status);
}

extern "C" int kp_rollout_nl_ct(kp_ctx* ctx, const kp_basis* basis, int batch, const double* Kf, const double* zeta0, const double* U,
                                int T, double Ts, double rtol, double atol, double* Z, int* naccept, int* nreject, int* status) {
  if (!ctx || !basis || !Kf || !zeta0 || !U || !Z || !status || batch < 1 || T < 1)
    return ctx ? ctx->fail(KP_ERR_ARG, "kp_rollout_nl_ct: bad argument") : KP_ERR_ARG;
  const BasisDev& b = basis->dev;
  if (b.model_type != KP_MODEL_NONLINEAR) return ctx->fail(KP_ERR_ARG, "kp_rollout_nl_ct: the dictionary must be of the nonlinear model type");
  if ((size_t)(b.nvars + b.nfull + b.N) * 8 > 64 * 1024) return ctx->fail(KP_ERR_ARG, "kp_rollout_nl_ct: dictionary too large");
  if (!ct_tol_ok(Ts, rtol, atol)) return ctx->fail(KP_ERR_ARG, "kp_rollout_nl_ct: Ts, rtol and atol must be positive and finite");
  KP_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->async_pending) {
    int rc0 = kp_synchronize(ctx);
    if (rc0) return rc0;
  }
  CtArgs g{};
  g.kind = 2; g.N = b.N; g.m = b.m; g.NS = b.nzeta; g.T = T; g.n_out = b.nzeta; g.Ts = Ts; g.rtol = rtol; g.atol = atol;
  g.stageA = (size_t)b.nzeta * b.N <= CT_STAGE;
  return ct_launch(ctx, "kp_rollout_nl_ct", true, g, &b, batch, Kf, (size_t)batch * b.nzeta * b.N, nullptr, 0, zeta0, U, Z,
                   naccept, nreject, status);
}
