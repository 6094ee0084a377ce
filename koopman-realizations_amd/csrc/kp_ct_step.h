// The workgroup-wide ode45 of kp_ct_rollout.hip and kp_validate_ct.hip: one workgroup integrates one state over a sample
// interval [0, Ts] with the input held.  It restates ode45's Dormand-Prince 5(4) pair and step control exactly as arm.dopri45
// does (initial step, MaxStep Ts / 10, the 1.1 h stretch to the end point, first-failure shrink then halving, growth of at
// most 5x); accepted and rejected step counts equal the host's.  The tableau and EPS are those of kp_dopri45.h, whose other
// users (kp_arm.hip, kp_rsys.hip) integrate one lane per trajectory with a step control of their own.
//
// Thread r owns rows r, r + nth, ... of every vector, so a stage needs one barrier (its input complete) before the right-hand
// side; stage inputs alternate between two buffers.  The error norm is one workgroup max per step.  Every thread runs the same
// step control on the same LDS values, so control flow stays uniform.  A kernel carves the LDS, stages the model and the
// inputs, fills a CtStep and calls, per sample, ct_sample_model, a barrier, and ct_integrate.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "kp_dopri45.h"
#include "kp_internal.h"

namespace {

using kp_dopri::dp_a;
using kp_dopri::dp_e;

constexpr int CT_MAX_ATTEMPTS = 100000;   // steps (accepted + rejected) per sample interval
constexpr double CT_EPS = kp_dopri::EPS;

inline bool ct_tol_ok(double Ts, double rtol, double atol) {
  return std::isfinite(Ts) && Ts > 0 && std::isfinite(rtol) && rtol > 0 && std::isfinite(atol) && atol > 0;
}

__device__ __forceinline__ double ct_max(double a, double b) { return (b > a || b != b) ? b : a; }

// workgroup max (NaN wins); red: two alternating slots of 8 doubles, `flip` toggled by the caller
__device__ __forceinline__ double ct_block_max(double v, double* red, int& flip) {
  for (int off = 32; off > 0; off >>= 1) v = ct_max(v, __shfl_xor(v, off));
  const int nw = blockDim.x >> 6;
  double* r = red + 8 * flip;
  flip ^= 1;
  if (nw == 1) return v;
  if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = v;
  __syncthreads();
  double m = r[0];
  for (int w = 1; w < nw; ++w) m = ct_max(m, r[w]);
  return m;
}

// What a workgroup's integration works on.  kind: 0 linear, 1 bilinear, 2 nonlinear; NS: state length (N, or nzeta for the
// nonlinear model).
struct CtStep {
  double *y, *yn;          // LDS, NS each: the state at the start of a step and its candidate (swapped at every accepted step)
  double *yt0, *yt1;       // LDS, NS each: the two stage-input buffers of the matrix models
  double *kk, *red;        // LDS: the stages 7 x NS, the reduction slots 16
  double* bu;              // LDS, matrix models: B u of the sample (N)
  double *v, *full, *zl;   // LDS, nonlinear: [zeta; u] (nvars), the dictionary (nfull), the lifted state (N)
  const double* Am;        // the matrix of the right-hand side (linear: A, bilinear: A + sum u_i B_i, nonlinear: Kf), LDS or memory
  const double *Ab, *Bb;   // the model in memory
  int N, m, NS, kind;
  double rtol, thr, Ts, hmax;
  int flip = 0, failed = 0, nacc = 0, nrej = 0;
};

// right-hand side f(x) -> out (own rows).  Matrix models: x complete (the caller's barrier).  Nonlinear: x is v[0..nz)
// (own rows written by the caller), the lift runs inside behind its own barriers.
template <bool NL>
__device__ __forceinline__ void ct_rhs(const CtStep& w, const BasisDev& bd, const double* x, double* out) {
  const int tid = threadIdx.x, nth = blockDim.x, N = w.N, NS = w.NS;
  const double* Am = w.Am;
  if (!NL) {
    for (int r = tid; r < N; r += nth) {
      double s = 0.0;
#pragma unroll 4
      for (int c = 0; c < N; ++c) s += Am[r + (size_t)c * N] * x[c];
      out[r] = w.kind == 0 ? s + w.bu[r] : s;
    }
  } else {
    const double* v = w.v;
    double* full = w.full;
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
        w.zl[c] = val;
      }
      __syncthreads();
      z = w.zl;
    }
    for (int r = tid; r < NS; r += nth) {
      double s = 0.0;
      for (int c = 0; c < N; ++c) s += Am[r + (size_t)c * NS] * z[c];
      out[r] = s;
    }
  }
}

// per-sample model from the inputs uc[i * us]: linear B u, bilinear A + sum_i u_i B_i, nonlinear [zeta; u].  The caller's
// barrier follows.
template <bool NL>
__device__ __forceinline__ void ct_sample_model(const CtStep& w, const double* uc, int us) {
  const int tid = threadIdx.x, nth = blockDim.x, N = w.N, m = w.m, NS = w.NS;
  if (!NL) {
    if (w.kind == 0) {
      for (int r = tid; r < N; r += nth) {
        double s = 0.0;
        for (int i = 0; i < m; ++i) s += w.Bb[r + (size_t)i * N] * uc[i * us];
        w.bu[r] = s;
      }
    } else {
      double* Aw = const_cast<double*>(w.Am);
      for (int e = tid; e < N * N; e += nth) {
        double s = w.Ab[e];
        for (int i = 0; i < m; ++i) s += uc[i * us] * w.Bb[(size_t)i * N * N + e];
        Aw[e] = s;
      }
    }
  } else {
    for (int i = tid; i < m; i += nth) w.v[NS + i] = uc[i * us];
    for (int r = tid; r < NS; r += nth) w.v[r] = w.y[r];
  }
}

// dopri45 over [0, Ts] from w.y, behind the barrier that completes y and the sample's model.  Leaves the end point in w.y
// (NaN after a failure), behind a barrier: y is complete before the next sample's model and right-hand side read it.
template <bool NL>
__device__ __forceinline__ void ct_integrate(CtStep& w, const BasisDev& bd) {
  const int tid = threadIdx.x, nth = blockDim.x, NS = w.NS;
  const double rtol = w.rtol, thr = w.thr, Ts = w.Ts, hmax = w.hmax;
  double* const kk = w.kk;
  double* const v = w.v;
  double* k0 = kk;
  double* k6 = kk + 6 * NS;
  ct_rhs<NL>(w, bd, w.y, k0);
  double loc = 0.0;
  for (int r = tid; r < NS; r += nth) loc = ct_max(loc, fabs(k0[r] / fmax(fabs(w.y[r]), thr)));
  double rh = ct_block_max(loc, w.red, w.flip) / (0.8 * pow(rtol, 0.2));
  double t = 0.0;
  double h = fmin(hmax, fabs(Ts));
  if (h * rh > 1.0) h = 1.0 / rh;
  h = fmax(h, 16.0 * CT_EPS * 1e-300);
  int attempts = 0;
  while (t < Ts && !w.failed) {
    const double hmin = 16.0 * CT_EPS * fmax(fabs(t), 1e-300);
    h = fmin(hmax, fmax(hmin, h));
    if (1.1 * h >= Ts - t) h = Ts - t;
    bool nofail = true;
    double err, tnew;
    const double* y = w.y;
    double* yn = w.yn;
    for (;;) {
      for (int s = 1; s < 6; ++s) {
        double* xin = NL ? v : ((s & 1) ? w.yt1 : w.yt0);
        for (int r = tid; r < NS; r += nth) {
          double acc = 0.0;
          for (int q = 0; q < s; ++q) acc += dp_a(s, q) * kk[q * NS + r];
          xin[r] = y[r] + h * acc;
        }
        if (!NL) __syncthreads();
        ct_rhs<NL>(w, bd, xin, kk + s * NS);
      }
      for (int r = tid; r < NS; r += nth) {
        double acc = 0.0;
        for (int q = 0; q < 6; ++q) acc += dp_a(6, q) * kk[q * NS + r];
        yn[r] = y[r] + h * acc;
        if (NL) v[r] = yn[r];
      }
      tnew = t + h;
      if (!NL) __syncthreads();
      ct_rhs<NL>(w, bd, yn, k6);
      double le = 0.0;
      for (int r = tid; r < NS; r += nth) {
        double e = 0.0;
        for (int q = 0; q < 7; ++q) e += dp_e(q) * kk[q * NS + r];
        le = ct_max(le, fabs(e) / fmax(fmax(fabs(y[r]), fabs(yn[r])), thr));
        if (!(fabs(yn[r]) < INFINITY)) le = NAN;
      }
      err = h * ct_block_max(le, w.red, w.flip);
      ++attempts;
      if (!(err < INFINITY) || attempts > CT_MAX_ATTEMPTS) { w.failed = 1; break; }
      if (err > rtol) {
        if (h <= hmin) { w.failed = 1; break; }     // step-size underflow
        ++w.nrej;
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
    if (w.failed) break;
    double hnext;
    if (nofail) {
      const double temp = 1.25 * pow(err / rtol, 0.2);
      hnext = temp > 0.2 ? h / temp : 5.0 * h;
    } else {
      hnext = h;
    }
    t = tnew;
    ++w.nacc;
    { double* tmp = w.y; w.y = w.yn; w.yn = tmp; }
    // FSAL: the last stage of the accepted step is the first of the next
    double* kl = kk + 6 * NS;
    for (int r = tid; r < NS; r += nth) kk[r] = kl[r];
    if (NL) for (int r = tid; r < NS; r += nth) v[r] = w.y[r];
    h = hnext;
  }
  if (w.failed)
    for (int r = tid; r < NS; r += nth) w.y[r] = NAN;
  __syncthreads();     // y complete before the next sample's model and right-hand side read it
}

}  // namespace
