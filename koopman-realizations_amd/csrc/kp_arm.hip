// The planar arm plant (koopman_hip_arm.h): Arm.m's equations of motion integrated by ode45's Dormand-Prince 5(4) pair,
// one GPU lane per trial.  Modes and their row rules are in the header.
//
// Equations of motion (Arm.m:111-222, 256-300), in the closed form of arm.py with theta_j = alpha_0 + ... + alpha_j,
// e_j = (-sin theta_j, cos theta_j) and d_j = d e_j / d theta_j = (-cos theta_j, -sin theta_j):
//   Jacobian column k of the end effector  E(k)    = sum_{j >= k} l d_j
//   Jacobian column k of the centre of mass of link i (k <= i)  Jc_i(k) = sum_{k <= j < i} l d_j + l/2 d_i
//   Dq_ab = I (n - max(a, b)) + w_0 E(a).E(b) + m sum_{i >= max(a, b)} Jc_i(a).Jc_i(b)
//   Coriolis: Dq_dt alphadot - dKE/dalpha.  arm.py sums the derivatives dDq/dalpha_p; contracted twice with alphadot
//   they reduce to sum_i m Jc_i(k).a_i + w_0 E(k).a_end, where a_i = -sum_j w_ij e_j thetadot_j^2 is the acceleration of
//   the point at zero alphaddot (w_ij = l, or l/2 for j = i), so no dDq/dalpha_p is formed.
//   dPE/dalpha_k = k alpha_k - w_0 g grav.E(k) - m g grav.sum_{i >= k} Jc_i(k), grav = (-sin w_1, cos w_1) (Arm.m:164-166)
//   damping d alphadot, input torque -ku (repeat(u, nlinks) - alpha) (Arm.m:204-209)
//   alphaddot = Dq \ -(Coriolis + dPE + damping + input): Dq is SPD, solved by an unpivoted Cholesky in registers.
//
// Layout.  A trial's steps are serial, so the parallelism is the batch: lane b integrates trial b, in 64-lane workgroups
// so that a wave that finishes early frees its slot.  Nlinks is a template parameter (1..8): the state, the seven stages
// and Dq are register arrays indexed by constants only.  Lanes diverge in step counts; nothing is shared, no barrier.
// The input / load row of a stage is cached per lane and reloaded only when the row changes (every ~60 steps).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "koopman_hip_arm.h"
#include "kp_dopri45.h"
#include "kp_internal.h"

namespace {

using namespace kp_dopri;

constexpr int ARM_MAX_LINKS = 8;
constexpr int ARM_MAX_ATTEMPTS = 100000;   // attempted steps between two outputs
constexpr double ARM_EPS = EPS;

struct ArmArgs {
  int mode, batch, T, Tout, Nmods, nlinks;
  double l, k, d, m, inertia, g, ku;
  double Ts, rtol, atol;
  const double* t;     // T
  const double* x0;    // batch x 2N, or null (rest)
  const double* U;     // batch x T x Nmods
  const double* W;     // batch x T x 2, or null (no load)
  double* X;           // batch x Tout x 2N
  int* nacc; int* nrej; int* status;
};

// the input / load row of one lane: per-link inputs (repeat(u, nlinks)) of row r and, for 'interp', of row r + 1
template <int N>
struct Row {
  int r = -1;
  double u[N], u2[N];
  double w0, w1, tr, tr1;
};

template <int N>
__device__ void load_row(const ArmArgs& g, int b, int r, Row<N>& c) {
  c.r = r;
  const double* Ub = g.U + (size_t)b * g.T * g.Nmods;
#pragma unroll
  for (int j = 0; j < N; ++j) c.u[j] = Ub[(size_t)r * g.Nmods + j / g.nlinks];
  if (g.mode == KP_ARM_SPAN_INTERP) {
    const int r1 = min(r + 1, g.T - 1);
#pragma unroll
    for (int j = 0; j < N; ++j) c.u2[j] = Ub[(size_t)r1 * g.Nmods + j / g.nlinks];
    c.tr = g.t[r]; c.tr1 = g.t[r1];
  }
  if (g.W) {
    c.w0 = g.W[((size_t)b * g.T + r) * 2];
    c.w1 = g.W[((size_t)b * g.T + r) * 2 + 1];
  } else {
    c.w0 = 0.0; c.w1 = 0.0;
  }
}

// the row of stage time s (header rules); `cur` is the lane's cursor: the number of t entries below s
__device__ __forceinline__ int row_of(const ArmArgs& g, double s, int& cur) {
  if (g.mode == KP_ARM_SPAN_FLOOR) {
    const double q = floor(s / g.Ts);
    return !(q > 0.0) ? 0 : (q >= (double)(g.T - 1) ? g.T - 1 : (int)q);
  }
  while (cur < g.T && g.t[cur] < s) ++cur;
  while (cur > 0 && g.t[cur - 1] >= s) --cur;
  return s == 0.0 ? 1 : min(cur, g.T - 1);
}

// f = [alphadot; alphaddot] at state x under input row c (u interpolated at s in 'interp' mode)
template <int N>
__device__ void arm_rhs(const ArmArgs& g, const Row<N>& c, double s, const double* x, double* f) {
  double sn[N], cs[N], thd[N];
  {
    double th = 0.0, td = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      th += x[j]; td += x[N + j];
      sincos(th, &sn[j], &cs[j]);
      thd[j] = td;
    }
  }
  const double l = g.l, m = g.m, w0 = c.w0;
  const double gx = -sin(c.w1), gy = cos(c.w1);
  // end effector: E(k) and its zero-alphaddot acceleration
  double Ex[N], Ey[N];
  double ax = 0.0, ay = 0.0;
  {
    double sx = 0.0, sy = 0.0;
#pragma unroll
    for (int j = N - 1; j >= 0; --j) {
      sx += l * -cs[j]; sy += l * -sn[j];
      Ex[j] = sx; Ey[j] = sy;
      ax -= l * -sn[j] * thd[j] * thd[j];
      ay -= l * cs[j] * thd[j] * thd[j];
    }
  }
  double D[N][N], h[N];
#pragma unroll
  for (int a = 0; a < N; ++a) {
#pragma unroll
    for (int b = a; b < N; ++b) D[a][b] = g.inertia * (double)(N - b) + w0 * (Ex[a] * Ex[b] + Ey[a] * Ey[b]);
    h[a] = w0 * (Ex[a] * ax + Ey[a] * ay) - w0 * g.g * (gx * Ex[a] + gy * Ey[a]);
  }
  // centres of mass
  double cax = 0.0, cay = 0.0;         // sum_{j < i} l (-e_j) thetadot_j^2
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double q = thd[i] * thd[i];
    const double aix = cax - 0.5 * l * -sn[i] * q, aiy = cay - 0.5 * l * cs[i] * q;
    cax -= l * -sn[i] * q; cay -= l * cs[i] * q;
    double Jx[N], Jy[N];
    double sx = 0.5 * l * -cs[i], sy = 0.5 * l * -sn[i];
#pragma unroll
    for (int k = N - 1; k >= 0; --k) {
      if (k <= i) {
        if (k < i) { sx += l * -cs[k]; sy += l * -sn[k]; }
        Jx[k] = sx; Jy[k] = sy;
      }
    }
#pragma unroll
    for (int a = 0; a <= i && a < N; ++a) {
#pragma unroll
      for (int b = a; b <= i && b < N; ++b) D[a][b] += m * (Jx[a] * Jx[b] + Jy[a] * Jy[b]);
      h[a] += m * (Jx[a] * aix + Jy[a] * aiy) - m * g.g * (gx * Jx[a] + gy * Jy[a]);
    }
  }
  double uj[N];
#pragma unroll
  for (int j = 0; j < N; ++j) uj[j] = c.u[j];
  if (g.mode == KP_ARM_SPAN_INTERP) {
#pragma unroll
    for (int j = 0; j < N; ++j) uj[j] = c.u[j] + (c.u2[j] - c.u[j]) / (c.tr1 - c.tr) * (s - c.tr);   // Arm.m:1007
  }
  double rhs[N];
#pragma unroll
  for (int a = 0; a < N; ++a)
    rhs[a] = -(h[a] + g.k * x[a] + g.d * x[N + a] - g.ku * (uj[a] - x[a]));
  // unpivoted Cholesky D = L L' (L over D's upper triangle, transposed), then the two triangular solves
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double dj = D[j][j];
#pragma unroll
    for (int q = 0; q < j; ++q) dj -= D[q][j] * D[q][j];
    dj = sqrt(dj);
    D[j][j] = dj;
    const double inv = 1.0 / dj;
#pragma unroll
    for (int i = j + 1; i < N; ++i) {
      double v = D[j][i];
#pragma unroll
      for (int q = 0; q < j; ++q) v -= D[q][i] * D[q][j];
      D[j][i] = v * inv;
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double v = rhs[i];
#pragma unroll
    for (int q = 0; q < i; ++q) v -= D[q][i] * rhs[q];
    rhs[i] = v / D[i][i];
  }
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    double v = rhs[i];
#pragma unroll
    for (int q = i + 1; q < N; ++q) v -= D[i][q] * rhs[q];
    rhs[i] = v / D[i][i];
  }
#pragma unroll
  for (int j = 0; j < N; ++j) { f[j] = x[N + j]; f[N + j] = rhs[j]; }
}

template <int N>
__global__ __launch_bounds__(64) void kp_arm_kernel(ArmArgs g) {
  constexpr int S = 2 * N;
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= g.batch) return;
  double* Xb = g.X + (size_t)b * g.Tout * S;
  double y[S], yn[S], kk[7][S], xs[S];
#pragma unroll
  for (int r = 0; r < S; ++r) y[r] = g.x0 ? g.x0[(size_t)b * S + r] : 0.0;
#pragma unroll
  for (int r = 0; r < S; ++r) Xb[r] = y[r];
  Row<N> row;
  int cur = 0, nacc = 0, nrej = 0, failed = 0;
  const bool restart = g.mode == KP_ARM_RESTART;
  const double rtol = g.rtol, thr = g.atol / g.rtol;
  const int nint = restart ? g.T - 1 : 1;     // integrations
  int nxt = 1;                                // next output row
  for (int iv = 0; iv < nint && !failed; ++iv) {
    // span of this integration and its first interval (ode45's htspan)
    double tf, htspan;
    if (restart) {
      tf = g.t[iv + 1] - g.t[iv];
      htspan = tf;
      load_row<N>(g, b, iv, row);
    } else {
      tf = g.t[g.Tout - 1];
      htspan = g.t[1] - g.t[0];
    }
    const double hmax = 0.1 * tf;
    auto stage = [&](double s, const double* x, double* f) {
      if (!restart) {
        const int r = row_of(g, s, cur);
        if (r != row.r) load_row<N>(g, b, r, row);
      }
      arm_rhs<N>(g, row, s, x, f);
    };
    double t = 0.0;
    stage(t, y, kk[0]);
    double rh = 0.0;
#pragma unroll
    for (int r = 0; r < S; ++r) rh = fmax(rh, fabs(kk[0][r] / fmax(fabs(y[r]), thr)));
    rh /= 0.8 * pow(rtol, 0.2);
    double h = fmin(hmax, htspan);
    if (h * rh > 1.0) h = 1.0 / rh;
    h = fmax(h, 16.0 * ARM_EPS * 1e-300);
    int attempts = 0;
    while (t < tf) {
      const double hmin = 16.0 * ARM_EPS * fmax(fabs(t), 1e-300);
      h = fmin(hmax, fmax(hmin, h));
      if (1.1 * h >= tf - t) h = tf - t;
      bool nofail = true;
      double err, tnew;
      for (;;) {
#pragma unroll
        for (int s = 1; s < 6; ++s) {
#pragma unroll
          for (int r = 0; r < S; ++r) {
            double acc = 0.0;
#pragma unroll
            for (int q = 0; q < s; ++q) acc += dp_a(s, q) * kk[q][r];
            xs[r] = y[r] + h * acc;
          }
          stage(t + dp_c(s) * h, xs, kk[s]);
        }
#pragma unroll
        for (int r = 0; r < S; ++r) {
          double acc = 0.0;
#pragma unroll
          for (int q = 0; q < 6; ++q) acc += dp_a(6, q) * kk[q][r];
          yn[r] = y[r] + h * acc;
        }
        tnew = t + h;
        stage(tnew, yn, kk[6]);
        double le = 0.0;
#pragma unroll
        for (int r = 0; r < S; ++r) {
          double e = 0.0;
#pragma unroll
          for (int q = 0; q < 7; ++q) e += dp_e(q) * kk[q][r];
          const double v = fabs(e) / fmax(fmax(fabs(y[r]), fabs(yn[r])), thr);
          le = (v > le || v != v) ? v : le;
          if (!(fabs(yn[r]) < INFINITY)) le = NAN;
        }
        err = h * le;
        ++attempts;
        if (!(err < INFINITY) || attempts > ARM_MAX_ATTEMPTS) { failed = 1; break; }
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
      ++nacc;
      if (!restart) {     // outputs in (t, tnew]: the step end, or ntrp45
        while (nxt < g.Tout && g.t[nxt] <= tnew) {
          double* o = Xb + (size_t)nxt * S;
          if (g.t[nxt] == tnew) {
#pragma unroll
            for (int r = 0; r < S; ++r) o[r] = yn[r];
          } else {
            const double sg = (g.t[nxt] - t) / h;
            const double p[4] = {sg, sg * sg, sg * sg * sg, sg * sg * sg * sg};
#pragma unroll
            for (int r = 0; r < S; ++r) {
              double acc = 0.0;
#pragma unroll
              for (int q = 0; q < 7; ++q) {
                if (q == 1) continue;
                double cq = 0.0;
#pragma unroll
                for (int c = 0; c < 4; ++c) cq += bi(q, c) * p[c];
                acc += kk[q][r] * cq;
              }
              o[r] = y[r] + h * acc;
            }
          }
          ++nxt;
          attempts = 0;
        }
      }
      double hnext;
      if (nofail) {
        const double temp = 1.25 * pow(err / rtol, 0.2);
        hnext = temp > 0.2 ? h / temp : 5.0 * h;
      } else {
        hnext = h;
      }
      t = tnew;
#pragma unroll
      for (int r = 0; r < S; ++r) { y[r] = yn[r]; kk[0][r] = kk[6][r]; }     // FSAL
      h = hnext;
    }
    if (restart && !failed) {
      double* o = Xb + (size_t)(iv + 1) * S;
#pragma unroll
      for (int r = 0; r < S; ++r) o[r] = y[r];
      nxt = iv + 2;
    }
  }
  if (failed)
    for (int j = nxt; j < g.Tout; ++j)
#pragma unroll
      for (int r = 0; r < S; ++r) Xb[(size_t)j * S + r] = NAN;
  if (g.nacc) g.nacc[b] = nacc;
  if (g.nrej) g.nrej[b] = nrej;
  g.status[b] = failed ? KP_ERR_NOT_CONVERGED : KP_OK;
}

template <int N>
void arm_launch(const ArmArgs& g, hipStream_t s) {
  hipLaunchKernelGGL(kp_arm_kernel<N>, dim3((g.batch + 63) / 64), dim3(64), 0, s, g);
}

bool finite_pos(double v) { return std::isfinite(v) && v > 0; }

}  // namespace

extern "C" int kp_arm_simulate(kp_ctx* ctx, const kp_arm_params* p, int mode, int batch, int T, const double* t, double Ts,
                               const double* x0, const double* U, const double* W, double rtol, double atol, double* X,
                               int* naccept, int* nreject, int* status) {
  if (!ctx) return KP_ERR_ARG;
  if (!p || !t || !U || !X || !status || batch < 1)
    return ctx->fail(KP_ERR_ARG, "kp_arm_simulate: null argument or batch < 1");
  if (mode < KP_ARM_SPAN_ZOH || mode > KP_ARM_RESTART) return ctx->fail(KP_ERR_ARG, "kp_arm_simulate: unknown mode");
  if (p->Nmods < 1 || p->nlinks < 1 || (long)p->Nmods * p->nlinks > ARM_MAX_LINKS)
    return ctx->fail(KP_ERR_ARG, "kp_arm_simulate: Nmods and nlinks must be >= 1 and Nlinks = Nmods nlinks at most 8");
  const double pv[7] = {p->l, p->k, p->d, p->m, p->i, p->g, p->ku};
  for (double v : pv)
    if (!std::isfinite(v)) return ctx->fail(KP_ERR_ARG, "kp_arm_simulate: params must be finite");
  if (T < 2 || (mode == KP_ARM_SPAN_INTERP && T < 3))
    return ctx->fail(KP_ERR_ARG, "kp_arm_simulate: T must be at least 2 (3 for the interp mode)");
  if (t[0] != 0.0) return ctx->fail(KP_ERR_ARG, "kp_arm_simulate: t must start at 0");
  for (int j = 1; j < T; ++j)
    if (!(t[j] > t[j - 1]) || !std::isfinite(t[j])) return ctx->fail(KP_ERR_ARG, "kp_arm_simulate: t must be strictly increasing and finite");
  if (!finite_pos(rtol) || !finite_pos(atol)) return ctx->fail(KP_ERR_ARG, "kp_arm_simulate: rtol and atol must be positive and finite");
  if (mode == KP_ARM_SPAN_FLOOR && !finite_pos(Ts)) return ctx->fail(KP_ERR_ARG, "kp_arm_simulate: Ts must be positive and finite");
  KP_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->async_pending) {
    int rc0 = kp_synchronize(ctx);
    if (rc0) return rc0;
  }
  const int N = p->Nmods * p->nlinks, S = 2 * N;
  const int Tout = mode == KP_ARM_SPAN_INTERP ? T - 1 : T;
  const size_t nt = T, nx0 = x0 ? (size_t)batch * S : 0, nU = (size_t)batch * T * p->Nmods, nW = W ? (size_t)batch * T * 2 : 0;
  const size_t nX = (size_t)batch * Tout * S, ints = ((size_t)3 * batch * 4 + 7) / 8;
  double* ws = (double*)ctx->workspace(6, (nt + nx0 + nU + nW + nX + ints) * 8);
  if (!ws) return ctx->fail(KP_ERR_HIP, "kp_arm_simulate: out of device memory");
  double *dt = ws, *dx0 = dt + nt, *dU = dx0 + nx0, *dW = dU + nU, *dX = dW + nW;
  int* di = (int*)(dX + nX);
  hipStream_t s = ctx->stream;
  KP_HIP(ctx, hipMemcpyAsync(dt, t, nt * 8, hipMemcpyHostToDevice, s));
  if (nx0) KP_HIP(ctx, hipMemcpyAsync(dx0, x0, nx0 * 8, hipMemcpyHostToDevice, s));
  KP_HIP(ctx, hipMemcpyAsync(dU, U, nU * 8, hipMemcpyHostToDevice, s));
  if (nW) KP_HIP(ctx, hipMemcpyAsync(dW, W, nW * 8, hipMemcpyHostToDevice, s));
  ArmArgs g{};
  g.mode = mode; g.batch = batch; g.T = T; g.Tout = Tout; g.Nmods = p->Nmods; g.nlinks = p->nlinks;
  g.l = p->l; g.k = p->k; g.d = p->d; g.m = p->m; g.inertia = p->i; g.g = p->g; g.ku = p->ku;
  g.Ts = Ts; g.rtol = rtol; g.atol = atol;
  g.t = dt; g.x0 = nx0 ? dx0 : nullptr; g.U = dU; g.W = nW ? dW : nullptr; g.X = dX;
  g.nacc = di; g.nrej = di + batch; g.status = di + 2 * batch;
  KP_HIP(ctx, hipEventRecord(ctx->ev0, s));
  switch (N) {
    case 1: arm_launch<1>(g, s); break;
    case 2: arm_launch<2>(g, s); break;
    case 3: arm_launch<3>(g, s); break;
    case 4: arm_launch<4>(g, s); break;
    case 5: arm_launch<5>(g, s); break;
    case 6: arm_launch<6>(g, s); break;
    case 7: arm_launch<7>(g, s); break;
    default: arm_launch<8>(g, s); break;
  }
  KP_HIP(ctx, hipGetLastError());
  KP_HIP(ctx, hipEventRecord(ctx->ev1, s));
  KP_HIP(ctx, hipMemcpyAsync(X, dX, nX * 8, hipMemcpyDeviceToHost, s));
  KP_HIP(ctx, hipMemcpyAsync(status, g.status, (size_t)batch * 4, hipMemcpyDeviceToHost, s));
  if (naccept) KP_HIP(ctx, hipMemcpyAsync(naccept, g.nacc, (size_t)batch * 4, hipMemcpyDeviceToHost, s));
  if (nreject) KP_HIP(ctx, hipMemcpyAsync(nreject, g.nrej, (size_t)batch * 4, hipMemcpyDeviceToHost, s));
  KP_HIP(ctx, hipStreamSynchronize(s));
  float ms = 0;
  (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
  ctx->timers[5] = ms;
  return KP_OK;
}
