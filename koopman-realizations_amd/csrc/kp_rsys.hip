// The random-system generator (koopman_hip_rsys.h): Rsys.m's random 1-D systems integrated by ode45's Dormand-Prince
// 5(4) pair, one GPU lane per (system, trial).  Modes, row rules and input forms are in the header.
//
// Right-hand side (Rsys.m:60-90, rsys.py): xdot = exp(-x^4) (sum_j c_j x^(a_j) u^(b_j) + c_u u) - atan(x).  While an
// input row is held, sum_j c_j u^(b_j) [a_j = p] (+ c_u u at p = 0) is a polynomial w_p in x: it is collected once per
// row change, per lane, and evaluated by Horner - the arithmetic of rsys.py's simulate_systems_fast, term by term
// (u^b by repeated products, the terms of one power summed in order), so that the two agree to the last bits.
//
// Layout.  A trial's steps are serial, so the parallelism is the batch: lane b = i ntrials + j integrates trial j of
// system i (the draw order of Rsys), in 64-lane workgroups so that a wave that finishes early frees its slot.  The
// polynomial is a register array of KP_RSYS_MAX_DEG + 1 entries indexed by constants only; degree_x is uniform.  Lanes
// diverge in step counts; nothing is shared, no LDS, no barrier.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "koopman_hip_rsys.h"
#include "kp_dopri45.h"
#include "kp_internal.h"

// host and device evaluate the same products and sums: no contraction into fused multiply-adds
#pragma clang fp contract(off)

namespace {

using namespace kp_dopri;

constexpr int RSYS_MAX_DEG = 15;
constexpr int RSYS_MAX_ATTEMPTS = 100000;   // attempted steps between two outputs

struct RsysArgs {
  int mode, L, ntrials, T, nterms, dx, du, hold, nlev;
  double rtol, atol;
  const double* t;        // T
  const double* coeffs;   // nsys x nterms
  const int* px;          // nsys x nterms
  const int* pu;          // nsys x nterms
  const double* cu;       // nsys
  const double* x0;       // ntrials
  const double* U;        // L x T (hold 0) or L x nlev
  double* Y;              // L x T
  int* nacc; int* nrej; int* status;
};

// input of row r of lane b (header: the two input forms)
__device__ __forceinline__ double input_row(const RsysArgs& g, int b, int r) {
  if (g.hold == 0) return g.U[(size_t)b * g.T + r];
  return r < g.hold * (g.nlev - 1) ? g.U[(size_t)b * g.nlev + r / g.hold] : 0.0;
}

// the polynomial in x of system `sys` under input u (rsys.py: cub = c u^b, wp[p] = sum over a_j = p, wp[0] += c_u u)
__device__ void collect(const RsysArgs& g, int sys, double u, double* w) {
#pragma unroll
  for (int p = 0; p <= RSYS_MAX_DEG; ++p) w[p] = 0.0;
  const double* c = g.coeffs + (size_t)sys * g.nterms;
  const int* ax = g.px + (size_t)sys * g.nterms;
  const int* bu = g.pu + (size_t)sys * g.nterms;
  for (int j = 0; j < g.nterms; ++j) {
    double ub = 1.0;
    for (int q = 0; q < bu[j]; ++q) ub = ub * u;
    const double v = c[j] * ub;
    const int a = ax[j];
#pragma unroll
    for (int p = 0; p <= RSYS_MAX_DEG; ++p)
      if (p == a) w[p] = w[p] + v;
  }
  w[0] = w[0] + g.cu[sys] * u;
}

__device__ __forceinline__ double rsys_rhs(const double* w, int dx, double x) {
  double acc = 0.0;
#pragma unroll
  for (int p = RSYS_MAX_DEG; p >= 0; --p) {
    if (p == dx) acc = w[p];
    else if (p < dx) acc = acc * x + w[p];
  }
  const double x2 = x * x;
  return exp(-(x2 * x2)) * acc - atan(x);
}

__global__ __launch_bounds__(64) void kp_rsys_kernel(RsysArgs g) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= g.L) return;
  const int sys = b / g.ntrials;
  double* Yb = g.Y + (size_t)b * g.T;
  double w[RSYS_MAX_DEG + 1];
  double kk[7];
  double y = g.x0[b - sys * g.ntrials];
  Yb[0] = y;
  const bool restart = g.mode == KP_RSYS_RESTART;
  int cur = 0, nacc = 0, nrej = 0, failed = 0;
  double ucur = 0.0;
  bool have_u = false;
  auto use_row = [&](int r) {
    const double u = input_row(g, b, r);
    if (!have_u || !(u == ucur)) {      // value-keyed, as the host mirror: a held level is collected once
      collect(g, sys, u, w);
      ucur = u;
      have_u = true;
    }
  };
  const double rtol = g.rtol, thr = g.atol / g.rtol;
  const int nint = restart ? g.T - 1 : 1;     // integrations
  int nxt = 1;                                // next output row
  for (int iv = 0; iv < nint && !failed; ++iv) {
    double t, tf, htspan;
    if (restart) {
      t = g.t[iv];
      tf = g.t[iv + 1];
      htspan = tf - t;
      use_row(iv);
    } else {
      t = g.t[0];
      tf = g.t[g.T - 1];
      htspan = g.t[1] - g.t[0];
    }
    const double hmax = 0.1 * (tf - t);
    // f at stage time s; span mode: the row of get_u (the last t_j <= s), found from the lane's cursor
    auto stage = [&](double s, double x) {
      if (!restart) {
        while (cur + 1 < g.T && g.t[cur + 1] <= s) ++cur;
        while (cur > 0 && g.t[cur] > s) --cur;
        use_row(cur);
      }
      return rsys_rhs(w, g.dx, x);
    };
    kk[0] = stage(t, y);
    const double rh = fabs(kk[0] / fmax(fabs(y), thr)) / (0.8 * pow(rtol, 0.2));
    double h = fmin(hmax, htspan);
    if (h * rh > 1.0) h = 1.0 / rh;
    h = fmax(h, 16.0 * EPS * fmax(fabs(t), 1e-300));
    int attempts = 0;
    while (t < tf) {
      const double hmin = 16.0 * EPS * fmax(fabs(t), 1e-300);
      h = fmin(hmax, fmax(hmin, h));
      if (1.1 * h >= tf - t) h = tf - t;
      bool nofail = true;
      double err, tnew, yn;
      for (;;) {
        // stages 1..6 in a rolled loop: ONE inlined right-hand side (exp, atan, the row lookup) instead of six.  Stage 6
        // is the new point itself (A's row 6 is B5, c_6 = 1); kk is indexed by constants through selects.
        for (int s = 1; s <= 6; ++s) {
          double acc = 0.0;
#pragma unroll
          for (int q = 0; q < 6; ++q)
            if (q < s) acc += dp_a(s, q) * kk[q];
          const double xs = y + h * acc;
          const double f = stage(t + dp_c(s) * h, xs);
#pragma unroll
          for (int q = 1; q < 7; ++q)
            if (q == s) kk[q] = f;
          yn = xs;
        }
        tnew = t + h;
        if (restart && h >= tf - t) tnew = tf;      // the closing step lands exactly on the sample
        double e = 0.0;
#pragma unroll
        for (int q = 0; q < 7; ++q) e += dp_e(q) * kk[q];
        double le = fabs(e) / fmax(fmax(fabs(y), fabs(yn)), thr);
        if (!(fabs(yn) < INFINITY)) le = NAN;
        err = h * le;
        ++attempts;
        if (!(err < INFINITY) || attempts > RSYS_MAX_ATTEMPTS) { failed = 1; break; }
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
        while (nxt < g.T && g.t[nxt] <= tnew) {
          if (g.t[nxt] == tnew) {
            Yb[nxt] = yn;
          } else {
            const double sg = (g.t[nxt] - t) / h;
            const double p[4] = {sg, sg * sg, sg * sg * sg, sg * sg * sg * sg};
            double acc = 0.0;
#pragma unroll
            for (int q = 0; q < 7; ++q) {
              if (q == 1) continue;
              double cq = 0.0;
#pragma unroll
              for (int c = 0; c < 4; ++c) cq += bi(q, c) * p[c];
              acc += kk[q] * cq;
            }
            Yb[nxt] = y + h * acc;
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
      y = yn;
      kk[0] = kk[6];     // FSAL
      h = hnext;
    }
    if (restart && !failed) {
      Yb[iv + 1] = y;
      nxt = iv + 2;
    }
  }
  if (failed)
    for (int j = nxt; j < g.T; ++j) Yb[j] = NAN;
  if (g.nacc) g.nacc[b] = nacc;
  if (g.nrej) g.nrej[b] = nrej;
  g.status[b] = failed ? KP_ERR_NOT_CONVERGED : KP_OK;
}

// Rsys.save_data's layout of one kp_traj (n = m = 1): trial j < ntrials - 1 of system i is rows j T .. j T + T - 1 of
// system i's training block, the last trial its validation block; one thread per (lane, row), inputs expanded from U
__global__ __launch_bounds__(256) void kp_rsys_to_traj_kernel(RsysArgs g, double* __restrict__ Ytr, double* __restrict__ Utr,
                                                              double* __restrict__ Yv, double* __restrict__ Uv) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)g.L * g.T) return;
  const int b = (int)(e / g.T), r = (int)(e - (size_t)b * g.T);
  const int sys = b / g.ntrials, j = b - sys * g.ntrials;
  const double y = g.Y[e], u = input_row(g, b, r);
  if (j < g.ntrials - 1) {
    const size_t o = ((size_t)sys * (g.ntrials - 1) + j) * g.T + r;
    Ytr[o] = y; Utr[o] = u;
  } else {
    const size_t o = (size_t)sys * g.T + r;
    Yv[o] = y; Uv[o] = u;
  }
}

bool finite_pos(double v) { return std::isfinite(v) && v > 0; }

}  // namespace

extern "C" int kp_rsys_simulate(kp_ctx* ctx, const kp_rsys_dims* dims, int mode, int nsys, int ntrials, int T, const double* t,
                                const double* coeffs, const int* pow_x, const int* pow_u, const double* input_gain,
                                const double* x0, const double* U, int hold, double rtol, double atol, double* Y, int* naccept,
                                int* nreject, int* status, kp_traj** traj) {
  if (!ctx) return KP_ERR_ARG;
  if (traj) *traj = nullptr;
  if (!dims || !t || !coeffs || !pow_x || !pow_u || !input_gain || !x0 || !U || !status)
    return ctx->fail(KP_ERR_ARG, "kp_rsys_simulate: null argument");
  if (mode != KP_RSYS_SPAN && mode != KP_RSYS_RESTART) return ctx->fail(KP_ERR_ARG, "kp_rsys_simulate: unknown mode");
  if (nsys < 1 || dims->num_terms < 1) return ctx->fail(KP_ERR_ARG, "kp_rsys_simulate: nsys and num_terms must be >= 1");
  if (ntrials < (traj ? 2 : 1))
    return ctx->fail(KP_ERR_ARG, "kp_rsys_simulate: ntrials must be >= 1 (>= 2 with traj: the last trial validates)");
  if (T < 3) return ctx->fail(KP_ERR_ARG, "kp_rsys_simulate: T must be at least 3");
  if ((int64_t)nsys * ntrials > (int64_t)1 << 30) return ctx->fail(KP_ERR_ARG, "kp_rsys_simulate: nsys * ntrials too large");
  if (hold < 0) return ctx->fail(KP_ERR_ARG, "kp_rsys_simulate: hold must be >= 0");
  const int dx = dims->degree_x, du = dims->degree_u, nterms = dims->num_terms;
  if (dx < 0 || dx > RSYS_MAX_DEG || du < 0 || du > RSYS_MAX_DEG)
    return ctx->fail(KP_ERR_ARG, "kp_rsys_simulate: degree_x and degree_u must lie in 0..15");
  for (size_t e = 0; e < (size_t)nsys * nterms; ++e)
    if (pow_x[e] < 0 || pow_x[e] > dx || pow_u[e] < 0 || pow_u[e] > du)
      return ctx->fail(KP_ERR_ARG, "kp_rsys_simulate: pow_x / pow_u must lie in 0..degree_x / 0..degree_u");
  if (t[0] != 0.0) return ctx->fail(KP_ERR_ARG, "kp_rsys_simulate: t must start at 0");
  for (int j = 1; j < T; ++j)
    if (!(t[j] > t[j - 1]) || !std::isfinite(t[j]))
      return ctx->fail(KP_ERR_ARG, "kp_rsys_simulate: t must be strictly increasing and finite");
  if (!finite_pos(rtol) || !finite_pos(atol))
    return ctx->fail(KP_ERR_ARG, "kp_rsys_simulate: rtol and atol must be positive and finite");
  KP_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->async_pending) {
    int rc0 = kp_synchronize(ctx);
    if (rc0) return rc0;
  }
  const int L = nsys * ntrials;
  const int nlev = hold ? (T + hold - 1) / hold : 0;
  const size_t nt = T, nc = (size_t)nsys * nterms, nU = (size_t)L * (hold ? nlev : T), nY = (size_t)L * T;
  const size_t ints = ((size_t)2 * nc + (size_t)3 * L) * 4;
  double* ws = (double*)ctx->workspace(6, (nt + nc + nsys + ntrials + nU + nY) * 8 + ints);
  if (!ws) return ctx->fail(KP_ERR_HIP, "kp_rsys_simulate: out of device memory");
  double *dt = ws, *dc = dt + nt, *dcu = dc + nc, *dx0 = dcu + nsys, *dU = dx0 + ntrials, *dY = dU + nU;
  int* di = (int*)(dY + nY);
  hipStream_t s = ctx->stream;
  KP_HIP(ctx, hipMemcpyAsync(dt, t, nt * 8, hipMemcpyHostToDevice, s));
  KP_HIP(ctx, hipMemcpyAsync(dc, coeffs, nc * 8, hipMemcpyHostToDevice, s));
  KP_HIP(ctx, hipMemcpyAsync(dcu, input_gain, (size_t)nsys * 8, hipMemcpyHostToDevice, s));
  KP_HIP(ctx, hipMemcpyAsync(dx0, x0, (size_t)ntrials * 8, hipMemcpyHostToDevice, s));
  KP_HIP(ctx, hipMemcpyAsync(dU, U, nU * 8, hipMemcpyHostToDevice, s));
  KP_HIP(ctx, hipMemcpyAsync(di, pow_x, nc * 4, hipMemcpyHostToDevice, s));
  KP_HIP(ctx, hipMemcpyAsync(di + nc, pow_u, nc * 4, hipMemcpyHostToDevice, s));
  RsysArgs g{};
  g.mode = mode; g.L = L; g.ntrials = ntrials; g.T = T; g.nterms = nterms; g.dx = dx; g.du = du; g.hold = hold; g.nlev = nlev;
  g.rtol = rtol; g.atol = atol;
  g.t = dt; g.coeffs = dc; g.px = di; g.pu = di + nc; g.cu = dcu; g.x0 = dx0; g.U = dU; g.Y = dY;
  g.nacc = di + 2 * nc; g.nrej = g.nacc + L; g.status = g.nrej + L;
  KP_HIP(ctx, hipEventRecord(ctx->ev0, s));
  hipLaunchKernelGGL(kp_rsys_kernel, dim3((L + 63) / 64), dim3(64), 0, s, g);
  KP_HIP(ctx, hipGetLastError());
  KP_HIP(ctx, hipEventRecord(ctx->ev1, s));
  if (Y) KP_HIP(ctx, hipMemcpyAsync(Y, dY, nY * 8, hipMemcpyDeviceToHost, s));
  KP_HIP(ctx, hipMemcpyAsync(status, g.status, (size_t)L * 4, hipMemcpyDeviceToHost, s));
  if (naccept) KP_HIP(ctx, hipMemcpyAsync(naccept, g.nacc, (size_t)L * 4, hipMemcpyDeviceToHost, s));
  if (nreject) KP_HIP(ctx, hipMemcpyAsync(nreject, g.nrej, (size_t)L * 4, hipMemcpyDeviceToHost, s));
  KP_HIP(ctx, hipStreamSynchronize(s));
  float ms = 0;
  (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
  ctx->timers[5] = ms;
  if (!traj) return KP_OK;
  int nfail = 0;
  for (int b = 0; b < L; ++b) nfail += status[b] != KP_OK;
  if (nfail)
    return ctx->fail(KP_ERR_NOT_CONVERGED, "kp_rsys_simulate: " + std::to_string(nfail) +
                                               " trial(s) did not converge; no trajectory object was created");
  // the trajectories go straight into a new object's device blocks, then the object is finished (scaled) as usual
  kp_traj* tr = nullptr;
  int rc = kp_traj_create(ctx, nsys, ntrials - 1, T, 1, 1, T, &tr);
  if (rc) return rc;
  double* blk[4];
  kp_traj_device_blocks(tr, blk);
  hipLaunchKernelGGL(kp_rsys_to_traj_kernel, dim3((unsigned)((nY + 255) / 256)), dim3(256), 0, s, g, blk[0], blk[1], blk[2], blk[3]);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    kp_traj_destroy(tr);
    return ctx->fail(KP_ERR_HIP, std::string("kp_rsys_simulate: ") + hipGetErrorString(e));
  }
  rc = kp_traj_finish(tr);
  if (rc) {
    kp_traj_destroy(tr);
    return rc;
  }
  *traj = tr;
  return KP_OK;
}
