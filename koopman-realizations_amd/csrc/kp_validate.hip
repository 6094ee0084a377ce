// The validation table: every candidate model rolled out over every validation trial in one launch, the metrics of get_error
// (Ksysid.m:1886-1897) reduced in the kernel.  Replaces nmod x ntr calls of val_model / val_BLmodel / val_NLmodel, each a host
// lift, four uploads, a launch, a trajectory copied back and get_error on the host.
//
// One workgroup per (model, trial) pair, nothing shared between pairs: the numbers of a pair are the same bits alone or in a
// batch.  The rollout is a serial chain of small matrix-vector products (kp_rollout_kernel, kp_more.hip), so:
//   - the rows 1:N of the model that feed forward are staged in LDS when they fit beside the rest, else read from memory (L2);
//   - the state is double buffered, one barrier per step - a wave-level fence when the workgroup is one wave (widest per-step
//     loop <= 64);
//   - time runs in chunks of KP_VALIDATE_CHUNK steps: inputs, loads and real outputs of a chunk are staged in LDS and the
//     simulated outputs collected there, so no global load of them sits inside the recurrence.
// A loaded model (nw > 0) is given at its full width; step j weights the nw + 1 column blocks of A(1:N, :), B_i(1:N, :) or Kf
// by [1; w_j] (Ksysid.m:1667-1668: znow = kron(I, z(1:N)) [1; w_j], only rows 1:N of the result are used again).
//
// LDS layout (doubles): state | acc (4 n + 4) | yfactor (n) | Uc [m][TC] | Wc [nw][TC] | Yr [n][TC + 1] | Ys [n][TC + 1] |
// Ec [TC] | Euc [TC] | staged model.  state: z [2][N] (linear, bilinear) or v [nvars] | full [nfull] | psi [N] (nonlinear).
//
// Order of the reductions, fixed in time: behind the recurrence of a chunk, thread tt forms the two Euclidean norms of step tt
// (sum over the outputs in ascending order); then thread c < n adds |d|, d^2 and min / max of yreal of column c over the steps
// of the chunk in ascending order, thread n and n + 1 the two norms likewise, each into its accumulator, which runs on from
// chunk to chunk.  No atomics, no tree: the sums are those of a serial loop over t.  kp_validate_ct.hip restates these
// statements with its own barrier and chunk length, on purpose: a change to one reduction must be made in the other.  The
// argument checks are kp_validate_args.h's, shared with kp_validate_ct.
#include <algorithm>
#include <cmath>

#include "kp_internal.h"
#include "koopman_hip_validate.h"
#include "kp_validate_args.h"

#define VAL_TC KP_VALIDATE_CHUNK
#define VAL_TCP (VAL_TC + 1)   // row stride of Yr / Ys: thread c walks row c in the column reduction
#define VAL_LDS (160 * 1024)

struct ValDims {
  int mt, N, m, n, nz, nw, ntr;
  int stage;          // the model rows are in LDS
  int64_t rows;       // all trials' rows
};

template <bool ONE_WAVE>
__global__ __launch_bounds__(256) void kp_validate_kernel(BasisDev b, ValDims d, const double* __restrict__ A, const double* __restrict__ B,
                                                          const int64_t* __restrict__ off, const double* __restrict__ Z0,
                                                          const double* __restrict__ U, const double* __restrict__ Yreal,
                                                          const double* __restrict__ Wl, const double* __restrict__ yfac, int want_sim,
                                                          double* __restrict__ err, int* __restrict__ status, double* __restrict__ Ysim) {
  extern __shared__ double sm[];
  const int tid = threadIdx.x, nth = blockDim.x;
  const int mod = blockIdx.x / d.ntr, tr = blockIdx.x - mod * d.ntr;
  const int N = d.N, m = d.m, n = d.n, nz = d.nz, nw = d.nw, nw1 = d.nw + 1;
  const int NL = N * nw1;
  const bool nl = d.mt == KP_MODEL_NONLINEAR, bil = d.mt == KP_MODEL_BILINEAR;
  const int64_t r0 = off[tr];
  const int T = (int)(off[tr + 1] - r0);
  const int R = nl ? nz : N;                                     // rows of the model that feed forward
  const int nstate = nl ? b.nvars + b.nfull + N : 2 * N;
  double* st = sm;
  double* acc = st + nstate;                                     // [c][sum |d|, sum d^2, min, max] | euclid | unscaled euclid | not finite
  double* fs = acc + 4 * n + 4;
  double* Uc = fs + n;
  double* Wc = Uc + m * VAL_TC;
  double* Yr = Wc + nw * VAL_TC;
  double* Ys = Yr + n * VAL_TCP;
  double* Ec = Ys + n * VAL_TCP;
  double* Euc = Ec + VAL_TC;
  double* Msh = Euc + VAL_TC;

  // the model: Am is R x NL (leading dimension lda), Bm R x m (linear) or m blocks of R x NL (bilinear)
  const int mbc = nl ? 0 : (bil ? m * NL : m);                    // columns of B
  const double* Am = A + (size_t)mod * (nl ? (size_t)nz * NL : (size_t)NL * NL);
  const double* Bm = nl ? nullptr : B + (size_t)mod * NL * mbc;
  int lda = nl ? nz : NL;
  if (d.stage) {
    for (int e = tid; e < R * NL; e += nth) {
      const int c = e / R, r = e - c * R;
      Msh[e] = Am[r + (size_t)c * lda];
    }
    double* Bsh = Msh + R * NL;
    for (int e = tid; e < R * mbc; e += nth) {
      const int c = e / R, r = e - c * R;
      Bsh[e] = Bm[r + (size_t)c * lda];
    }
    Am = Msh;
    Bm = Bsh;
    lda = R;
  }
  for (int c = tid; c < n; c += nth) {
    acc[4 * c] = 0.0;
    acc[4 * c + 1] = 0.0;
    acc[4 * c + 2] = INFINITY;
    acc[4 * c + 3] = -INFINITY;
    fs[c] = yfac[c];
  }
  if (tid < 3) acc[4 * n + tid] = 0.0;
  if (nl) {
    for (int i = tid; i < nz; i += nth) st[i] = Z0[tr + (size_t)i * d.ntr];       // zeta0: ntr x nzeta column-major
  } else {
    for (int r = tid; r < N; r += nth) st[r] = Z0[tr + (size_t)r * d.ntr];        // econ_full(zeta0): ntr x N column-major
  }
  auto sync = [&]() {
    if (ONE_WAVE) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
      __syncthreads();
    }
  };
  sync();
  double* v = st;                   // nonlinear: [zeta; u]
  double* full = st + b.nvars;
  double* psi = full + b.nfull;
  double* Yo = want_sim ? Ysim + (size_t)mod * d.rows * n : nullptr;
  for (int t0 = 0; t0 < T; t0 += VAL_TC) {
    const int tc = min(VAL_TC, T - t0);
    for (int e = tid; e < m * tc; e += nth) {
      const int i = e / tc, tt = e - i * tc;
      Uc[i * VAL_TC + tt] = U[(size_t)i * d.rows + r0 + t0 + tt];
    }
    for (int e = tid; e < nw * tc; e += nth) {
      const int i = e / tc, tt = e - i * tc;
      Wc[i * VAL_TC + tt] = Wl[(size_t)i * d.rows + r0 + t0 + tt];
    }
    for (int e = tid; e < n * tc; e += nth) {
      const int i = e / tc, tt = e - i * tc;
      Yr[i * VAL_TCP + tt] = Yreal[(size_t)i * d.rows + r0 + t0 + tt];
    }
    sync();
    for (int tt = 0; tt < tc; ++tt) {
      const int t = t0 + tt;
      if (nl) {
        for (int r = tid; r < n; r += nth) Ys[r * VAL_TCP + tt] = t == 0 ? Yr[r * VAL_TCP] : v[r];
        if (t == T - 1) break;
        for (int i = tid; i < m; i += nth) v[nz + i] = Uc[i * VAL_TC + tt];
        sync();
        for (int c = tid; c < b.nfull; c += nth) full[c] = kp_eval_col(b, b.cols[c], v, 1);
        sync();
        for (int c = tid; c < N; c += nth) {                     // econ_full (Ksysid.m:1615-1618), as kp_rollout_nl_kernel
          double val;
          if (b.k_pcs == 0)
            val = full[c];
          else if (c < b.nvars)
            val = v[c];
          else if (c < b.nvars + b.k_pcs) {
            const double* pc = b.pcs + (size_t)(c - b.nvars) * b.nfull;
            val = 0.0;
            for (int i = 0; i < b.nfull; ++i) val += pc[i] * full[i];
          } else
            val = 1.0;
          psi[c] = val;
        }
        sync();
        for (int r = tid; r < nz; r += nth) {
          double s = 0.0;
          for (int l = 0; l < nw1; ++l) {
            const double* Al = Am + (size_t)l * N * lda;
            double q = 0.0;
#pragma unroll 4
            for (int c = 0; c < N; ++c) q += Al[r + (size_t)c * lda] * psi[c];
            s += l == 0 ? q : Wc[(l - 1) * VAL_TC + tt] * q;
          }
          v[r] = s;
        }
        sync();
      } else {
        const double* z = st + (t & 1) * N;
        double* zn = st + ((t + 1) & 1) * N;
        for (int r = tid; r < n; r += nth) Ys[r * VAL_TCP + tt] = t == 0 ? Yr[r * VAL_TCP] : z[r];   // y = C z, C = [I 0]; row 0: :1654
        if (t == T - 1) break;
        for (int r = tid; r < N; r += nth) {
          double s = 0.0;
          for (int l = 0; l < nw1; ++l) {
            const double* Al = Am + (size_t)l * N * lda;
            double q = 0.0;
#pragma unroll 4
            for (int c = 0; c < N; ++c) q += Al[r + (size_t)c * lda] * z[c];
            s += l == 0 ? q : Wc[(l - 1) * VAL_TC + tt] * q;
          }
          if (bil) {
            for (int i = 0; i < m; ++i) {
              double qi = 0.0;
              for (int l = 0; l < nw1; ++l) {
                const double* Bl = Bm + ((size_t)i * NL + (size_t)l * N) * lda;
                double q = 0.0;
#pragma unroll 4
                for (int c = 0; c < N; ++c) q += Bl[r + (size_t)c * lda] * z[c];
                qi += l == 0 ? q : Wc[(l - 1) * VAL_TC + tt] * q;
              }
              s += qi * Uc[i * VAL_TC + tt];
            }
          } else {
            for (int i = 0; i < m; ++i) s += Bm[r + (size_t)i * lda] * Uc[i * VAL_TC + tt];
          }
          zn[r] = s;
        }
        sync();
      }
    }
    sync();   // the last step leaves the loop before its barrier
    for (int tt = tid; tt < tc; tt += nth) {
      double e2 = 0.0, eu2 = 0.0;
      bool bad = false;
      for (int c = 0; c < n; ++c) {
        const double ys = Ys[c * VAL_TCP + tt];
        const double dd = ys - Yr[c * VAL_TCP + tt];
        const double du = dd * fs[c];
        e2 += dd * dd;
        eu2 += du * du;
        bad = bad || !isfinite(ys);
      }
      Ec[tt] = sqrt(e2);
      Euc[tt] = sqrt(eu2);
      if (bad) acc[4 * n + 2] = 1.0;
    }
    if (want_sim)
      for (int e = tid; e < n * tc; e += nth) {
        const int c = e / tc, tt = e - c * tc;
        Yo[(size_t)c * d.rows + r0 + t0 + tt] = Ys[c * VAL_TCP + tt];
      }
    sync();
    for (int c = tid; c < n + 2; c += nth) {
      if (c < n) {
        double sa = acc[4 * c], sq = acc[4 * c + 1], mn = acc[4 * c + 2], mx = acc[4 * c + 3];
        for (int tt = 0; tt < tc; ++tt) {
          const double yr = Yr[c * VAL_TCP + tt];
          const double dd = Ys[c * VAL_TCP + tt] - yr;
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
    sync();
  }
  double* eo = err + (size_t)blockIdx.x * (3 * n + 2);
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
    status[blockIdx.x] = acc[4 * n + 2] != 0.0 ? 1 : 0;
  }
}

extern "C" int kp_validate(kp_ctx* ctx, const kp_basis* basis, int model_type, int N, int m, int n, int nzeta, int nw, int nmod,
                           const double* A, const double* B, int ntr, const int64_t* trial_off, const double* zeta0, const double* U,
                           const double* Yreal, const double* Wl, const double* yfactor, int want_sim, double* err_out,
                           int* status_out, double* Ysim) {
  if (!ctx) return KP_ERR_ARG;
  const int rc_arg = val_check_args(ctx, "kp_validate", basis, model_type, N, m, n, nzeta, nw, nmod, A, B, ntr, trial_off, zeta0, U,
                                    Yreal, yfactor, want_sim, err_out, status_out, Ysim);
  if (rc_arg) return rc_arg;
  if (nw > 0 && !Wl) return ctx->fail(KP_ERR_ARG, "kp_validate: Wl required for a loaded model");
  const bool nl = model_type == KP_MODEL_NONLINEAR, bil = model_type == KP_MODEL_BILINEAR;
  const BasisDev& b = basis->dev;
  const int64_t rows = trial_off[ntr];
  const size_t NL = (size_t)N * (nw + 1);
  if (NL > (size_t)INT32_MAX / (size_t)std::max(1, m + 1)) return ctx->fail(KP_ERR_ARG, "kp_validate: model too wide");

  // LDS: what every pair needs, then the model when it fits as well
  const size_t nstate = nl ? (size_t)b.nvars + b.nfull + N : (size_t)2 * N;
  const size_t fixed = nstate + 4 * (size_t)n + 4 + n + (size_t)(m + nw) * VAL_TC + 2 * (size_t)n * VAL_TCP + 2 * VAL_TC;
  if (fixed * 8 > VAL_LDS)
    return ctx->fail(KP_ERR_ARG, "kp_validate: the state vectors and one chunk of " + std::to_string(VAL_TC) + " steps need " +
                                     std::to_string(fixed * 8) + " bytes of LDS, the limit is " + std::to_string(VAL_LDS));
  const size_t R = nl ? nzeta : N;
  const size_t mbc = nl ? 0 : (bil ? (size_t)m * NL : (size_t)m);
  const size_t model_lds = R * NL + R * mbc;
  const int stage = (fixed + model_lds) * 8 <= VAL_LDS;
  const size_t lds = (fixed + (stage ? model_lds : 0)) * 8;

  KP_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->async_pending) {
    int rc0 = kp_synchronize(ctx);
    if (rc0) return rc0;
  }
  const size_t nA = (size_t)nmod * (nl ? (size_t)nzeta * NL : NL * NL), nB = (size_t)nmod * NL * mbc;
  const size_t nz0 = (size_t)ntr * nzeta, nU = (size_t)rows * m, nY = (size_t)rows * n, nW = (size_t)rows * nw;
  const size_t nZ0 = nl ? 0 : (size_t)ntr * N, nE = (size_t)nmod * ntr * (3 * n + 2), nS = want_sim ? (size_t)nmod * rows * n : 0;
  const size_t npairs = (size_t)nmod * ntr;
  const size_t bytes = (nA + nB + nz0 + nU + nY + nW + n + nZ0 + nE + nS) * 8 + (size_t)(ntr + 1) * 8 + npairs * 4 + 64;
  double* ws = (double*)ctx->workspace(6, bytes);
  if (!ws) return ctx->fail(KP_ERR_HIP, "kp_validate: out of device memory (" + std::to_string(bytes) + " bytes)");
  double *dA = ws, *dB = dA + nA, *dz0 = dB + nB, *dU = dz0 + nz0, *dY = dU + nU, *dW = dY + nY, *df = dW + nW, *dZ0 = df + n,
         *dE = dZ0 + nZ0, *dS = dE + nE;
  int64_t* dOff = (int64_t*)(dS + nS);
  int* dSt = (int*)(dOff + ntr + 1);
  hipStream_t s = ctx->stream;
  KP_HIP(ctx, hipMemcpyAsync(dA, A, nA * 8, hipMemcpyHostToDevice, s));
  if (nB) KP_HIP(ctx, hipMemcpyAsync(dB, B, nB * 8, hipMemcpyHostToDevice, s));
  KP_HIP(ctx, hipMemcpyAsync(dz0, zeta0, nz0 * 8, hipMemcpyHostToDevice, s));
  if (nU) KP_HIP(ctx, hipMemcpyAsync(dU, U, nU * 8, hipMemcpyHostToDevice, s));
  KP_HIP(ctx, hipMemcpyAsync(dY, Yreal, nY * 8, hipMemcpyHostToDevice, s));
  if (nW) KP_HIP(ctx, hipMemcpyAsync(dW, Wl, nW * 8, hipMemcpyHostToDevice, s));
  KP_HIP(ctx, hipMemcpyAsync(df, yfactor, (size_t)n * 8, hipMemcpyHostToDevice, s));
  KP_HIP(ctx, hipMemcpyAsync(dOff, trial_off, (size_t)(ntr + 1) * 8, hipMemcpyHostToDevice, s));
  KP_HIP(ctx, hipEventRecord(ctx->ev0, s));
  if (!nl) {                                                       // z_0 = econ_full(zeta0) of every trial, by the lift kernel
    int rc = kp_lift_dev(ctx, basis, KP_LIFT_ECON, dz0, nullptr, ntr, dZ0);
    if (rc) return rc;
  }
  ValDims d{model_type, N, m, n, nzeta, nw, ntr, stage, rows};
  static KpLdsCache lds_c0, lds_c1;
  // one wave when no per-step loop is wider than a wave: the rows of the state, and the columns of a nonlinear dictionary
  const bool one_wave = N <= 64 && (!nl || b.nfull <= 64);
  const double* z0dev = nl ? dz0 : dZ0;
  if (one_wave) {
    KP_HIP(ctx, kp_ensure_lds(lds_c1, (const void*)kp_validate_kernel<true>, VAL_LDS));
    hipLaunchKernelGGL(kp_validate_kernel<true>, dim3((unsigned)npairs), dim3(64), lds, s, b, d, dA, dB, dOff, z0dev, dU, dY, dW, df,
                       want_sim, dE, dSt, dS);
  } else {
    KP_HIP(ctx, kp_ensure_lds(lds_c0, (const void*)kp_validate_kernel<false>, VAL_LDS));
    hipLaunchKernelGGL(kp_validate_kernel<false>, dim3((unsigned)npairs), dim3(256), lds, s, b, d, dA, dB, dOff, z0dev, dU, dY, dW, df,
                       want_sim, dE, dSt, dS);
  }
  KP_HIP(ctx, hipGetLastError());
  KP_HIP(ctx, hipEventRecord(ctx->ev1, s));
  KP_HIP(ctx, hipMemcpyAsync(err_out, dE, nE * 8, hipMemcpyDeviceToHost, s));
  KP_HIP(ctx, hipMemcpyAsync(status_out, dSt, npairs * 4, hipMemcpyDeviceToHost, s));
  if (nS) KP_HIP(ctx, hipMemcpyAsync(Ysim, dS, nS * 8, hipMemcpyDeviceToHost, s));
  KP_HIP(ctx, hipStreamSynchronize(s));
  float ms = 0;
  (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
  ctx->timers[5] = ms;
  return KP_OK;
}
