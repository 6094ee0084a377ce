// Continuous-time validation rollouts (koopman_hip_ct.h): every sample interval of val_model / val_BLmodel / val_NLmodel
// (Ksysid.m:1679-1683, 1777-1781, 1849-1856) is ode45 over [0, Ts] with the input held, from the end point of the previous one.
// The integrator restates ode45's Dormand-Prince 5(4) pair and step control exactly as arm.dopri45 does (initial step, MaxStep
// Ts / 10, the 1.1 h stretch to the end point, first-failure shrink then halving, growth of at most 5x).
//
// One workgroup per rollout.  The steps are serial, so everything a stage touches lives in LDS: the state, the seven stages,
// the inputs of a chunk of samples and, when it fits, the model (for a bilinear model the matrix A + sum_i u_i B_i of the
// sample, formed once per sample; in global memory beyond 90 states, where B streams from L2).  Thread r owns rows r, r + nth,
// ... of every vector, so a stage needs one barrier (its input complete) before the right-hand side; stage inputs alternate
// between two buffers.  The error norm is one workgroup max per step.  Every thread runs the same step control on the same
// LDS values, so control flow stays uniform.
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
  double* y = sm;
  double* yn = y + NS;
  double* yt0 = yn + NS;                      // matrix models: two stage-input buffers
  double* yt1 = yt0 + NS;
  double* kk = yt1 + NS;                      // 7 x NS
  double* red = kk + 7 * NS;                  // 16
  double* Uc = red + 16;                      // m x tc
  double* extra = Uc + (size_t)m * g.tc;
  // matrix models: bu (N) then the staged matrix; nonlinear: v (nvars), full (nfull), zl (N), staged Kf
  double* bu = extra;
  double* Ash = bu + N;
  double* v = extra;
  double* full = NL ? v + bd.nvars : nullptr;
  double* zl = NL ? full + bd.nfull : nullptr;
  double* Ksh = NL ? zl + N : nullptr;
  const double* Ab = g.A + (size_t)bi * (NL ? (size_t)NS * N : (size_t)N * N);
  const double* Bb = NL ? nullptr : g.B + (size_t)bi * N * (g.kind == 1 ? (size_t)N * m : (size_t)m);
  const double* Ub = g.U + (size_t)bi * T * m;
  double* Yb = g.Y + (size_t)bi * T * g.n_out;
  const double* Am = Ab;                      // the matrix of the right-hand side (linear: A, bilinear: A + sum u_i B_i)
  if (!NL) {
    if (g.kind == 1) Am = g.stageA ? Ash : g.Ag + (size_t)bi * N * N;
    else if (g.stageA) {
      for (int e = tid; e < N * N; e += nth) Ash[e] = Ab[e];
      Am = Ash;
    }
  } else if (g.stageA) {
    for (int e = tid; e < NS * N; e += nth) Ksh[e] = Ab[e];
    Am = Ksh;
  }
  for (int r = tid; r < NS; r += nth) y[r] = g.z0[(size_t)bi * NS + r];
  int flip = 0, failed = 0, nacc = 0, nrej = 0;
  const double rtol = g.rtol, thr = g.atol / g.rtol, Ts = g.Ts, hmax = 0.1 * fabs(Ts);
  const double* uc = Uc;     // inputs of the current sample: uc[i * tc]

  // right-hand side f(x) -> out (own rows).  Matrix models: x complete (the caller's barrier).  Nonlinear: x is v[0..nz)
  // (own rows written by the caller), the lift runs inside behind its own barriers.
  auto rhs = [&](const double* x, double* out) {
    if (!NL) {
      for (int r = tid; r < N; r += nth) {
        double s = 0.0;
#pragma unroll 4
        for (int c = 0; c < N; ++c) s += Am[r + (size_t)c * N] * x[c];
        out[r] = g.kind == 0 ? s + bu[r] : s;
      }
    } else {
      __syncthreads();
      for (int c = tid; c < bd.nfull; c += nth) full[c] = kp_eval_col(bd, bd.cols[c], v, 1);
      __syncthreads();
      const double* z = full;
      if (bd.k_pcs) {
        for (int c = tid; c < N; c += nth) {
          double val;
          if (c < bd.nvars) val = v[c];
          else if (c < bd.nvars + bd.k_pcs) {
            const double* pc = bd.pcs + (size_t)(c - bd.nvars) * bd.nfull;
            val = 0.0;
            for (int i = 0; i < bd.nfull; ++i) val += pc[i] * full[i];
          } else val = 1.0;
          zl[c] = val;
        }
        __syncthreads();
        z = zl;
      }
      for (int r = tid; r < NS; r += nth) {
        double s = 0.0;
        for (int c = 0; c < N; ++c) s += Am[r + (size_t)c * NS] * z[c];
        out[r] = s;
      }
    }
  };

  for (int j = 0; j < T; ++j) {
    for (int r = tid; r < g.n_out; r += nth) Yb[(size_t)r * T + j] = y[r];
    if (j == T - 1) break;
    if (failed) {
      for (int r = tid; r < NS; r += nth) y[r] = NAN;
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
    uc = Uc + jc;
    // per-sample model: linear B u, bilinear A + sum_i u_i B_i, nonlinear [zeta; u]
    if (!NL) {
      if (g.kind == 0) {
        for (int r = tid; r < N; r += nth) {
          double s = 0.0;
          for (int i = 0; i < m; ++i) s += Bb[r + (size_t)i * N] * uc[i * g.tc];
          bu[r] = s;
        }
      } else {
        double* Aw = const_cast<double*>(Am);
        for (int e = tid; e < N * N; e += nth) {
          double s = Ab[e];
          for (int i = 0; i < m; ++i) s += uc[i * g.tc] * Bb[(size_t)i * N * N + e];
          Aw[e] = s;
        }
      }
    } else {
      for (int i = tid; i < m; i += nth) v[NS + i] = uc[i * g.tc];
      for (int r = tid; r < NS; r += nth) v[r] = y[r];
    }
    __syncthreads();
    // ---- dopri45 over [0, Ts] from y ----
    double* k0 = kk;
    double* k6 = kk + 6 * NS;
    rhs(y, k0);
    double loc = 0.0;
    for (int r = tid; r < NS; r += nth) loc = ct_max(loc, fabs(k0[r] / fmax(fabs(y[r]), thr)));
    double rh = ct_block_max(loc, red, flip) / (0.8 * pow(rtol, 0.2));
    double t = 0.0;
    double h = fmin(hmax, fabs(Ts));
    if (h * rh > 1.0) h = 1.0 / rh;
    h = fmax(h, 16.0 * CT_EPS * 1e-300);
    int attempts = 0;
    while (t < Ts && !failed) {
      const double hmin = 16.0 * CT_EPS * fmax(fabs(t), 1e-300);
      h = fmin(hmax, fmax(hmin, h));
      if (1.1 * h >= Ts - t) h = Ts - t;
      bool nofail = true;
      double err, tnew;
      for (;;) {
        for (int s = 1; s < 6; ++s) {
          double* xin = NL ? v : ((s & 1) ? yt1 : yt0);
          for (int r = tid; r < NS; r += nth) {
            double acc = 0.0;
            for (int q = 0; q < s; ++q) acc += dp_a(s, q) * kk[q * NS + r];
            xin[r] = y[r] + h * acc;
          }
          if (!NL) __syncthreads();
          rhs(xin, kk + s * NS);
        }
        for (int r = tid; r < NS; r += nth) {
          double acc = 0.0;
          for (int q = 0; q < 6; ++q) acc += dp_a(6, q) * kk[q * NS + r];
          yn[r] = y[r] + h * acc;
          if (NL) v[r] = yn[r];
        }
        tnew = t + h;
        if (!NL) __syncthreads();
        rhs(yn, k6);
        double le = 0.0;
        for (int r = tid; r < NS; r += nth) {
          double e = 0.0;
          for (int q = 0; q < 7; ++q) e += dp_e(q) * kk[q * NS + r];
          le = ct_max(le, fabs(e) / fmax(fmax(fabs(y[r]), fabs(yn[r])), thr));
          if (!(fabs(yn[r]) < INFINITY)) le = NAN;
        }
        err = h * ct_block_max(le, red, flip);
        ++attempts;
        if (!(err < INFINITY) || attempts > CT_MAX_ATTEMPTS) { failed = 1; break; }
        if (err > rtol) {
          if (h <= hmin) { failed = 1; break; }     // step-size underflow
          ++nrej;
          if (nofail) {
            nofail = false;
            h = fmax(hmin, h * fmax(0.1, 0.8 * pow(rtol / err, 0.2)));
          } else {
            h = fmax(hmin, 0.5 * h);
          }
          continue;
        }
        break;
      }
      if (failed) break;
      double hnext;
      if (nofail) {
        const double temp = 1.25 * pow(err / rtol, 0.2);
        hnext = temp > 0.2 ? h / temp : 5.0 * h;
      } else {
        hnext = h;
      }
      t = tnew;
      ++nacc;
      { double* tmp = y; y = yn; yn = tmp; }
      // FSAL: the last stage of the accepted step is the first of the next
      double* kl = kk + 6 * NS;
      for (int r = tid; r < NS; r += nth) kk[r] = kl[r];
      if (NL) for (int r = tid; r < NS; r += nth) v[r] = y[r];
      h = hnext;
    }
    if (failed)
      for (int r = tid; r < NS; r += nth) y[r] = NAN;
    __syncthreads();     // y complete before the next sample's model and right-hand side read it
  }
  if (tid == 0) {
    if (g.nacc) g.nacc[bi] = nacc;
    if (g.nrej) g.nrej[bi] = nrej;
    g.status[bi] = failed ? KP_ERR_NOT_CONVERGED : KP_OK;
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

bool ct_tol_ok(double Ts, double rtol, double atol) {
  return std::isfinite(Ts) && Ts > 0 && std::isfinite(rtol) && rtol > 0 && std::isfinite(atol) && atol > 0;
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
