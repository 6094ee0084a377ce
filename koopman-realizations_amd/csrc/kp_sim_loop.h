// The closed-loop scaffold shared by kp_mpc_simulate (kp_mpc.hip) and kp_nmpc_simulate (kp_nmpc.hip): what a whole run with
// the model as the plant (Kmpc.run_simulation, Kmpc.m:403-512) does around its controller step and its plant step.
//
// The contract of a run, stated here once:
//   * One workgroup of 256 threads per trial runs steps k = 1 .. nref - 1 in scaled units.  Step k sees y = Y[k-1],
//     u_prev = U[k-1] and rows k-1 .. k-1+Np of the reference, whose last row is repeated behind its end (:354-365,
//     :473-477); it yields U[k] (the second row of the solution) and Y[k] (the plant step with u_prev: the one-step input
//     delay of :495-496).  Row 0 of U and Y is u0 and y0.
//   * The reference is staged in LDS with Np trailing copies of its last row, so that every step's window is one contiguous
//     block; y and u_prev stay in LDS from one step to the next.  No state passes through global memory: U, Y and aux rows
//     are only ever written.
//   * A failed step ends the trial (the break of :483-485): rows k .. nref-1 of U and Y and aux rows k-1 .. nref-2 are NaN,
//     steps_done = k - 1.  A trial that ran to the end has steps_done = nref - 1.
//   * A trial touches nothing that depends on blockIdx.x except its own rows, so its result does not depend on nb or on its
//     index.
//   * The reference is one block for every trial (ref_shared) or one per trial.
// What is a kernel's own - its LDS layout, what else it stages, its step and its plant step - is described with that kernel.
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "kp_internal.h"

// Passed by value inside each kernel's own argument block.  aux: one row per step, Z (width N) or info (width 3), or nullptr.
struct KpSimLoop {
  int nref, ny, m, nproj, Np, ref_shared, aux_w;
  const double *ref, *y0, *u0;      // [nb or 1][nref][nproj], [nb][ny], [nb][m]
  double *U, *Y, *aux;              // [nb][nref][m], [nb][nref][ny], [nb][nref - 1][aux_w] or nullptr
  int *steps_done, *status;         // [nb]
};

// ---- device part: no helper contains a barrier; the callers' barriers stand where the contract above needs them ---------
struct KpSimRows {
  double *U, *Y, *aux;              // the trial's own output rows
};

// Once per trial: the padded reference to refl ((nref + Np) nproj doubles of LDS), y0 / u0 to y / u (LDS) and to row 0 of
// Y / U.  The caller's barrier follows before anything reads them.
__device__ __forceinline__ KpSimRows kp_sim_prologue(const KpSimLoop& S, double* refl, double* y, double* u) {
  const int tid = threadIdx.x, nref = S.nref, ny = S.ny, m = S.m, nproj = S.nproj;
  const size_t trial = blockIdx.x;
  KpSimRows T;
  T.U = S.U + trial * (size_t)nref * m;
  T.Y = S.Y + trial * (size_t)nref * ny;
  T.aux = S.aux ? S.aux + trial * (size_t)(nref - 1) * S.aux_w : nullptr;
  const double* rt = S.ref + (S.ref_shared ? 0 : trial * (size_t)nref * nproj);
  for (int e = tid; e < (nref + S.Np) * nproj; e += 256) {
    const int row = e / nproj, p = e - row * nproj;
    refl[e] = rt[(size_t)min(row, nref - 1) * nproj + p];
  }
  for (int e = tid; e < ny; e += 256) {
    const double v = S.y0[trial * ny + e];
    y[e] = v;
    T.Y[e] = v;
  }
  for (int e = tid; e < m; e += 256) {
    const double v = S.u0[trial * m + e];
    u[e] = v;
    T.U[e] = v;
  }
  return T;
}

// End of step k: ynew(e) and unew(e) give elements e of the new y and u; both go to LDS and to row k.  The caller has a
// barrier in front (every read of the old y and u is done) and one behind.
template <class FY, class FU>
__device__ __forceinline__ void kp_sim_commit(const KpSimLoop& S, const KpSimRows& T, int k, double* y, double* u, FY ynew, FU unew) {
  const int tid = threadIdx.x, ny = S.ny, m = S.m;
  for (int e = tid; e < ny; e += 256) {
    const double v = ynew(e);
    y[e] = v;
    T.Y[(size_t)k * ny + e] = v;
  }
  for (int e = tid; e < m; e += 256) {
    const double v = unew(e);
    u[e] = v;
    T.U[(size_t)k * m + e] = v;
  }
}

// End of the trial: k is the step that failed (NaN tail) or nref; `status` is the trial's status word.
__device__ __forceinline__ void kp_sim_epilogue(const KpSimLoop& S, const KpSimRows& T, int k, int failed, int status) {
  const int tid = threadIdx.x, nref = S.nref;
  if (failed) {
    const double qnan = __builtin_nan("");
    for (size_t e = (size_t)k * S.m + tid; e < (size_t)nref * S.m; e += 256) T.U[e] = qnan;
    for (size_t e = (size_t)k * S.ny + tid; e < (size_t)nref * S.ny; e += 256) T.Y[e] = qnan;
    if (T.aux)
      for (size_t e = (size_t)(k - 1) * S.aux_w + tid; e < (size_t)(nref - 1) * S.aux_w; e += 256) T.aux[e] = qnan;
  }
  if (tid == 0) {
    S.steps_done[blockIdx.x] = k - 1;
    S.status[blockIdx.x] = status;
  }
}

// ---- host part --------------------------------------------------------------------------------------------------------
// Device block of a call (workspace slot 6), in doubles: [ref | y0 | u0] | U | Y | aux | steps_done, status (2 nb ints).
// Small calls (a single trial of a few hundred steps) are latency bound: inputs and outputs each cross in ONE copy through
// the page-locked scratch.  Large batches are bandwidth bound: their outputs go straight to the caller's arrays instead of
// through a second host copy.
#define KP_SIM_PINNED_BYTES ((size_t)4 << 20)
struct KpSimPlan {
  int nb;
  size_t nR, nY0, nU0, n_in, nU, nY, nA, n_out;
  bool pinned;
};
inline KpSimPlan kp_sim_plan(int nb, int nref, int nproj, int ny, int m, int aux_w, int ref_shared) {
  KpSimPlan P;
  P.nb = nb;
  P.nR = (size_t)(ref_shared ? 1 : nb) * nref * nproj; P.nY0 = (size_t)nb * ny; P.nU0 = (size_t)nb * m;
  P.n_in = P.nR + P.nY0 + P.nU0;
  P.nU = (size_t)nb * nref * m; P.nY = (size_t)nb * nref * ny; P.nA = (size_t)nb * (nref - 1) * aux_w;
  P.n_out = P.nU + P.nY + P.nA + ((size_t)2 * nb + 1) / 2;
  P.pinned = (P.n_in + P.n_out) * 8 <= KP_SIM_PINNED_BYTES;
  return P;
}
struct KpSimIo {
  KpSimPlan P;
  double* h = nullptr;              // host staging: the page-locked scratch (inputs and outputs) or h_vec (inputs)
  std::vector<double> h_vec;
};
// S holds the call's sizes (aux_w = 0: no aux rows); the inputs cross in one copy on the context's stream and S gets its
// device pointers.  `who` is the entry point's name in the error texts.
inline int kp_sim_upload(kp_ctx* ctx, const char* who, int nb, const double* ref, const double* y0, const double* u0, KpSimLoop& S,
                         KpSimIo& io) {
  const KpSimPlan P = io.P = kp_sim_plan(nb, S.nref, S.nproj, S.ny, S.m, S.aux_w, S.ref_shared);
  double* ws = (double*)ctx->workspace(6, (P.n_in + P.n_out) * 8);
  if (!ws) return ctx->fail(KP_ERR_HIP, std::string(who) + ": out of device memory");
  if (P.pinned) {
    io.h = (double*)kp_pinned_scratch(ctx, (P.n_in + P.n_out) * 8);
    if (!io.h) return ctx->fail(KP_ERR_HIP, std::string(who) + ": out of page-locked memory");
  } else {
    io.h_vec.resize(P.n_in);
    io.h = io.h_vec.data();
  }
  memcpy(io.h, ref, P.nR * 8);
  memcpy(io.h + P.nR, y0, P.nY0 * 8);
  memcpy(io.h + P.nR + P.nY0, u0, P.nU0 * 8);
  KP_HIP(ctx, hipMemcpyAsync(ws, io.h, P.n_in * 8, hipMemcpyHostToDevice, ctx->stream));
  double* d_out = ws + P.n_in;
  S.ref = ws; S.y0 = ws + P.nR; S.u0 = ws + P.nR + P.nY0;
  S.U = d_out; S.Y = d_out + P.nU; S.aux = P.nA ? d_out + P.nU + P.nY : nullptr;
  S.steps_done = (int*)(d_out + P.nU + P.nY + P.nA);
  S.status = S.steps_done + nb;
  return KP_OK;
}
// The outputs of the launch that followed kp_sim_upload, and the wait for them.
inline int kp_sim_download(kp_ctx* ctx, const KpSimIo& io, const KpSimLoop& S, double* U, double* Y, double* aux, int* steps_done,
                           int* status) {
  const KpSimPlan& P = io.P;
  const size_t int_bytes = (size_t)P.nb * sizeof(int);
  hipStream_t s = ctx->stream;
  if (P.pinned) {
    double* h_out = io.h + P.n_in;
    KP_HIP(ctx, hipMemcpyAsync(h_out, S.U, P.n_out * 8, hipMemcpyDeviceToHost, s));
    KP_HIP(ctx, hipStreamSynchronize(s));
    memcpy(U, h_out, P.nU * 8);
    memcpy(Y, h_out + P.nU, P.nY * 8);
    if (P.nA) memcpy(aux, h_out + P.nU + P.nY, P.nA * 8);
    memcpy(steps_done, h_out + P.nU + P.nY + P.nA, int_bytes);
    memcpy(status, (const int*)(h_out + P.nU + P.nY + P.nA) + P.nb, int_bytes);
  } else {
    KP_HIP(ctx, hipMemcpyAsync(U, S.U, P.nU * 8, hipMemcpyDeviceToHost, s));
    KP_HIP(ctx, hipMemcpyAsync(Y, S.Y, P.nY * 8, hipMemcpyDeviceToHost, s));
    if (P.nA) KP_HIP(ctx, hipMemcpyAsync(aux, S.aux, P.nA * 8, hipMemcpyDeviceToHost, s));
    KP_HIP(ctx, hipMemcpyAsync(steps_done, S.steps_done, int_bytes, hipMemcpyDeviceToHost, s));
    KP_HIP(ctx, hipMemcpyAsync(status, S.status, int_bytes, hipMemcpyDeviceToHost, s));
    KP_HIP(ctx, hipStreamSynchronize(s));
  }
  return KP_OK;
}
