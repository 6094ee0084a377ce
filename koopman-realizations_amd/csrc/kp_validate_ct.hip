// The validation table of continuous-time models: every candidate rolled out over every validation trial in one launch, each
// sample interval ode45 over [0, Ts] with the input held (val_model / val_BLmodel / val_NLmodel, Ksysid.m:1679-1683,
// 1777-1781, 1849-1856), the metrics of get_error (:1886-1897) reduced in the kernel.  It joins the workgroup-wide
// Dormand-Prince integrator of kp_ct_rollout.hip with the (model x trial) grid, the chunked staging and the serial-in-time
// reduction of kp_validate.hip, and replaces nmod x ntr calls of kp_rollout_ct / kp_rollout_nl_ct of one workgroup each.
//
// One workgroup per (model, trial) pair, nothing shared between pairs but the read-only models: the numbers of a pair are the
// same bits alone or in a batch.  Thread r owns rows r, r + nth, ... of every vector, so a stage needs one barrier (its input
// complete) before the right-hand side; every thread runs the same step control on the same LDS values.  The step control is
// that of kp_ct_rollout_kernel, statement for statement.
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
// and n + 1 the two norms likewise.  No atomics, no tree.
#include <algorithm>
#include <cmath>

#include "koopman_hip_validate.h"
#include "kp_ct_step.h"
#include "kp_internal.h"

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
  double* y = sm;
  double* yn = y + NS;
  double* yt0 = yn + NS;                      // matrix models: two stage-input buffers
  double* yt1 = yt0 + NS;
  double* kk = yt1 + NS;                      // 7 x NS
  double* red = kk + 7 * NS;                  // 16
  double* acc = red + 16;                     // [c][sum |d|, sum d^2, min, max] | euclid | unscaled euclid | not finite
  double* fs = acc + 4 * n + 4;
  double* Uc = fs + n;
  double* Yr = Uc + m * VCT_TC;
  double* Ys = Yr + n * VCT_TCP;
  double* Ec = Ys + n * VCT_TCP;
  double* Euc = Ec + VCT_TC;
  double* extra = Euc + VCT_TC;
  double* bu = extra;
  double* Ash = bu + N;
  double* v = extra;
  double* full = NL ? v + bd.nvars : nullptr;
  double* zl = NL ? full + bd.nfull : nullptr;
  double* Ksh = NL ? zl + N : nullptr;
  const double* Ab = g.A + (size_t)mod * (NL ? (size_t)NS * N : (size_t)N * N);
  const double* Bb = NL ? nullptr : g.B + (size_t)mod * N * (g.kind == 1 ? (size_t)N * m : (size_t)m);
  const double* Am = Ab;                      // the matrix of the right-hand side (linear: A, bilinear: A + sum u_i B_i)
  if (!NL) {
    if (g.kind == 1) Am = g.stage ? Ash : g.Ag + (size_t)blockIdx.x * N * N;
    else if (g.stage) {
      for (int e = tid; e < N * N; e += nth) Ash[e] = Ab[e];
      Am = Ash;
    }
  } else if (g.stage) {
    for (int e = tid; e < NS * N; e += nth) Ksh[e] = Ab[e];
    Am = Ksh;
  }
  for (int c = tid; c < n; c += nth) {
    acc[4 * c] = 0.0;
    acc[4 * c + 1] = 0.0;
    acc[4 * c + 2] = INFINITY;
    acc[4 * c + 3] = -INFINITY;
    fs[c] = g.yfac[c];
  }
  if (tid < 3) acc[4 * n + tid] = 0.0;
  for (int r = tid; r < NS; r += nth) y[r] = g.Z0[tr + (size_t)r * g.ntr];
  int flip = 0, failed = 0, nacc = 0, nrej = 0;
  const double rtol = g.rtol, thr = g.atol / g.rtol, Ts = g.Ts, hmax = 0.1 * fabs(Ts);

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
      for (int r = tid; r < n; r += nth) Ys[r * VCT_TCP + tt] = j == 0 ? Yr[r * VCT_TCP] : y[r];   // row 0: :1654
      if (j == T - 1) break;
      if (failed) {
        for (int r = tid; r < NS; r += nth) y[r] = NAN;
        continue;
      }
      const double* uc = Uc + tt;     // inputs of the sample: uc[i * VCT_TC]
      // per-sample model: linear B u, bilinear A + sum_i u_i B_i, nonlinear [zeta; u]
      if (!NL) {
        if (g.kind == 0) {
          for (int r = tid; r < N; r += nth) {
            double s = 0.0;
            for (int i = 0; i < m; ++i) s += Bb[r + (size_t)i * N] * uc[i * VCT_TC];
            bu[r] = s;
          }
        } else {
          double* Aw = const_cast<double*>(Am);
          for (int e = tid; e < N * N; e += nth) {
            double s = Ab[e];
            for (int i = 0; i < m; ++i) s += uc[i * VCT_TC] * Bb[(size_t)i * N * N + e];
            Aw[e] = s;
          }
        }
      } else {
        for (int i = tid; i < m; i += nth) v[NS + i] = uc[i * VCT_TC];
        for (int r = tid; r < NS; r += nth) v[r] = y[r];
      }
      __syncthreads();
      // ---- dopri45 over [0, Ts] from y (kp_ct_rollout_kernel) ----
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
              double a = 0.0;
              for (int q = 0; q < s; ++q) a += dp_a(s, q) * kk[q * NS + r];
              xin[r] = y[r] + h * a;
            }
            if (!NL) __syncthreads();
            rhs(xin, kk + s * NS);
          }
          for (int r = tid; r < NS; r += nth) {
            double a = 0.0;
            for (int q = 0; q < 6; ++q) a += dp_a(6, q) * kk[q * NS + r];
            yn[r] = y[r] + h * a;
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
    g.status[blockIdx.x] = (failed || acc[4 * n + 2] != 0.0) ? 1 : 0;
    g.nacc[blockIdx.x] = nacc;
    g.nrej[blockIdx.x] = nrej;
  }
}

}  // namespace

extern "C" int kp_validate_ct(kp_ctx* ctx, const kp_basis* basis, int model_type, int N, int m, int n, int nzeta, int nw, int nmod,
                              const double* A, const double* B, int ntr, const int64_t* trial_off, const double* zeta0, const double* U,
                              const double* Yreal, const double* Wl, const double* yfactor, int want_sim, double Ts, double rtol,
                              double atol, double* err_out, int* status_out, double* Ysim, int* naccept, int* nreject) {
  if (!ctx) return KP_ERR_ARG;
  if (!basis || !A || !trial_off || !zeta0 || !Yreal || !yfactor || !err_out || !status_out || nmod < 1 || ntr < 1 || N < 1 || m < 0 ||
      n < 1 || nzeta < 1 || nw < 0)
    return ctx->fail(KP_ERR_ARG, "kp_validate_ct: bad argument");
  if (model_type != KP_MODEL_LINEAR && model_type != KP_MODEL_BILINEAR && model_type != KP_MODEL_NONLINEAR)
    return ctx->fail(KP_ERR_ARG, "kp_validate_ct: unknown model type");
  if (nw != 0) return ctx->fail(KP_ERR_ARG, "kp_validate_ct: loaded continuous-time models are not supported (nw must be 0)");
  if (!(std::isfinite(Ts) && Ts > 0 && std::isfinite(rtol) && rtol > 0 && std::isfinite(atol) && atol > 0))
    return ctx->fail(KP_ERR_ARG, "kp_validate_ct: Ts, rtol and atol must be positive and finite");
  const bool nl = model_type == KP_MODEL_NONLINEAR, bil = model_type == KP_MODEL_BILINEAR;
  const BasisDev& b = basis->dev;
  if (b.model_type != model_type)
    return ctx->fail(KP_ERR_ARG, "kp_validate_ct: the dictionary is of model type " + std::to_string(b.model_type) +
                                     ", the models of type " + std::to_string(model_type));
  if (b.N != N || b.m != m || b.nzeta != nzeta)
    return ctx->fail(KP_ERR_ARG, "kp_validate_ct: N, m and nzeta must be those of the dictionary (" + std::to_string(b.N) + ", " +
                                     std::to_string(b.m) + ", " + std::to_string(b.nzeta) + ")");
  if (N > 512) return ctx->fail(KP_ERR_ARG, "kp_validate_ct: N must be at most 512");
  if (n > N || (nl && n > nzeta))
    return ctx->fail(KP_ERR_ARG, "kp_validate_ct: n = " + std::to_string(n) + " outputs, but the state has " +
                                     std::to_string(nl ? nzeta : N) + " entries");
  if (!nl && !B) return ctx->fail(KP_ERR_ARG, "kp_validate_ct: B required");
  if (m > 0 && !U) return ctx->fail(KP_ERR_ARG, "kp_validate_ct: U required");
  if (want_sim && !Ysim) return ctx->fail(KP_ERR_ARG, "kp_validate_ct: Ysim required with want_sim");
  if (trial_off[0] != 0) return ctx->fail(KP_ERR_ARG, "kp_validate_ct: trial_off must start at 0");
  for (int q = 0; q < ntr; ++q) {
    const int64_t Tq = trial_off[q + 1] - trial_off[q];
    if (Tq < 1) return ctx->fail(KP_ERR_ARG, "kp_validate_ct: trial " + std::to_string(q) + " is empty");
    if (Tq > INT32_MAX) return ctx->fail(KP_ERR_ARG, "kp_validate_ct: trial " + std::to_string(q) + " is too long");
  }
  if ((int64_t)nmod * ntr > INT32_MAX) return ctx->fail(KP_ERR_ARG, "kp_validate_ct: too many (model, trial) pairs");
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
