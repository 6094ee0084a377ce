// Batched load observer: the estimates of Ksysid.observer_load (Ksysid.m:1978-2030) over many windows of many trials, the
// work of val_observer_load / val_observer_load_sparse (:2033-2139), in three launches.
//
// A window of hor rows regresses its hor - 1 pairs (zeta_k, zeta_{k+1}, u_k).  Pair k contributes nz rows
//   R_k = G_k kron(I_{nw+1}, psi_k),  psi_k = econ_full(zeta_k),  G_k = A[:nz, :] (linear) or A[:nz, :] + sum_j u_kj B_j[:nz, :]
// (bilinear), and the right-hand side d_k = zeta_{k+1}[:nz] - B[:nz, :] u_k (linear) or zeta_{k+1}[:nz] (bilinear).  Column l
// of R_k is the nz x N block l of G_k times psi_k, so R_k is one product of the stacked row blocks of A (and of the B_j) with
// psi_k.  Neighbouring windows share hor - 2 of their pairs, so:
//   1. kp_lift_dev: psi of every row the windows touch, once per row;
//   2. kp_obs_blocks_kernel: [R_k | d_k] (nz x (nw + 2)) once per row, from psi_k and the stacked blocks Gs;
//   3. kp_obs_window_kernel<nw + 1>: one wave per window sums its hor - 1 blocks into [R d]'[R d] (each lane a fixed set
//      of rows, then a fixed reduction tree: no atomics, the same bits every call), forms the QP in the free loads as the
//      fused observer of kp_mpc_step_loaded does (kp_mpc.hip mpc_load_observer), checks that its Hessian is positive
//      definite, solves it with the dual active-set solver of kp_qp.h at the same 1e-10 threshold and takes the residual
//      norm from the rows (the quadratic form in [R d]'[R d] cancels).
// The launch count does not depend on the number of trials, rows or windows; only when the rows spanned by the windows
// need more than OBS_WS_BUDGET of psi and blocks are the windows taken in chunks (three launches per chunk).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "kp_internal.h"
#include "koopman_hip_observer.h"
#include "kp_wg_inverse.h"
#include "kp_qp.h"

#define OBS_MAX_NW 8
#define OBS_MAX_HOR 1025
#define OBS_WAVES 4                              // windows per 256-thread workgroup (one per wave)
#define OBS_WS_BUDGET ((size_t)256 << 20)        // bytes of psi + blocks per chunk
#define OBS_PIVOT_TOL 1e-8                       // Cholesky pivot of the free loads' Hessian relative to its diagonal entry

// LDS of one wave (doubles, each offset even): H 64 | f 8 | b 16 | val 16 | norm 16 | col 16 ints | x 8 | xw 10 | M 56 |
// flag 2 | the QP solver's scratch for 8 variables and 16 rows
struct ObsLayout {
  enum { H = 0, F = 64, B = 72, VAL = 88, NORM = 104, COL = 120, X = 128, XW = 136, M = 146, FLAG = 202, QWS = 204 };
};
__host__ __device__ inline int obs_wave_doubles() { return ObsLayout::QWS + ((qp_lds_doubles(OBS_MAX_NW, 2 * OBS_MAX_NW) + 1) & ~1); }

// [R_k | d_k] of rows r0 .. r0 + nr - 1: Rd[(k nz + r)(nw1 + 1) + l], l < nw1 column l of R_k, l = nw1 the right-hand side.
// Gs: [(j nz + r) nw1 + l][c] = (j == 0 ? A : B_{j-1})[r, l Nb + c] (j = 0 only for a linear model), CB: nz x m (linear).
// Psi: nr x Nb column-major (the rows of this chunk); zeta, u: S x nz, S x m column-major (every row of the call).
__global__ __launch_bounds__(256) void kp_obs_blocks_kernel(const double* __restrict__ Psi, int64_t nr, int64_t r0,
                                                             const double* __restrict__ zeta, const double* __restrict__ u,
                                                             int64_t S, const double* __restrict__ Gs,
                                                             const double* __restrict__ CB, int nz, int nw1, int Nb, int m,
                                                             int bil, double* __restrict__ Rd) {
  const int ne = nz * (nw1 + 1);
  const int64_t total = nr * ne;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t k = e / ne;
    const int rem = (int)(e - k * ne), r = rem / (nw1 + 1), l = rem - r * (nw1 + 1);
    const int64_t g = r0 + k;
    double s;
    if (l < nw1) {
      const double* gs = Gs + (size_t)(r * nw1 + l) * Nb;
      const double* ps = Psi + k;
      s = 0.0;
      for (int c = 0; c < Nb; ++c) s += gs[c] * ps[(size_t)c * nr];
      if (bil)
        for (int j = 0; j < m; ++j) {
          const double* gj = Gs + ((size_t)((j + 1) * nz + r) * nw1 + l) * Nb;
          double t = 0.0;
          for (int c = 0; c < Nb; ++c) t += gj[c] * ps[(size_t)c * nr];
          s += t * u[g + (size_t)j * S];
        }
    } else {
      s = g + 1 < S ? zeta[g + 1 + (size_t)r * S] : 0.0;   // (the last row of a trial starts no pair of any window)
      if (!bil) {
        double t = 0.0;
        for (int j = 0; j < m; ++j) t += CB[r + j * nz] * u[g + (size_t)j * S];
        s -= t;
      }
    }
    Rd[e] = s;
  }
}

// index of entry (i, j), i <= j, of the upper triangle of a V x V matrix stored row by row
__host__ __device__ constexpr int obs_tri(int V, int i, int j) { return i * V - i * (i - 1) / 2 + (j - i); }

// One wave per window.  wrow[w]: the chunk-relative row of the window's first pair; out: what (nw per window), resnorm,
// status.
template <int NW1>
__global__ __launch_bounds__(256) void kp_obs_window_kernel(const double* __restrict__ Rd, int nz, int npairs,
                                                             const int64_t* __restrict__ wrow, int64_t w0, int64_t nwin,
                                                             const double* __restrict__ wprev, int flags,
                                                             double* __restrict__ what, double* __restrict__ resnorm,
                                                             int* __restrict__ status) {
  constexpr int NW = NW1 - 1, V = NW1 + 1, NA = V * (V + 1) / 2;
  extern __shared__ __align__(16) double sm[];
  const int lane = threadIdx.x & 63;
  const int64_t wl = (int64_t)blockIdx.x * OBS_WAVES + (threadIdx.x >> 6);
  if (wl >= nwin) return;                      // (no workgroup barrier below: the waves are independent)
  const int64_t w = w0 + wl;
  double* ws = sm + (threadIdx.x >> 6) * obs_wave_doubles();
  double* H = ws + ObsLayout::H;
  double* f = ws + ObsLayout::F;
  double* bq = ws + ObsLayout::B;
  double* val = ws + ObsLayout::VAL;
  double* nrm = ws + ObsLayout::NORM;
  int* col = (int*)(ws + ObsLayout::COL);
  double* x = ws + ObsLayout::X;
  double* xw = ws + ObsLayout::XW;
  double* Mq = ws + ObsLayout::M;
  int* flag = (int*)(ws + ObsLayout::FLAG);
  const double* R = Rd + (size_t)wrow[wl] * nz * V;
  const int nt = npairs * nz;

  // [R d]'[R d], upper triangle: every lane its rows t = lane, lane + 64, ..., then the wave's reduction tree
  double acc[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) acc[a] = 0.0;
  for (int t = lane; t < nt; t += 64) {
    double v[V];
#pragma unroll
    for (int l = 0; l < V; ++l) v[l] = R[(size_t)t * V + l];
#pragma unroll
    for (int i = 0; i < V; ++i)
#pragma unroll
      for (int j = i; j < V; ++j) acc[obs_tri(V, i, j)] += v[i] * v[j];
  }
  bool finite = true;
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    acc[a] = wave_sum(acc[a]);
    finite = finite && isfinite(acc[a]);
  }
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < NA; ++a) Mq[a] = acc[a];
  }
  WSYNC();

  // the QP in the free loads w_0 .. w_{nf-1} (PIN_LAST: the last one is 0), x = [1; w]:
  // 1/2 w'(2 Rf'Rf) w - 2 (Rf'(d - R e_0))' w,  -1 <= w <= 1 and, with RATE, |w - wprev| <= 0.01
  const int nf = (flags & KP_OBS_PIN_LAST) ? NW - 1 : NW;
  for (int e = lane; e < nf * nf; e += 64) {
    const int k1 = e % nf, k2 = e / nf;
    H[e] = 2.0 * Mq[obs_tri(V, min(k1, k2) + 1, max(k1, k2) + 1)];
  }
  if (lane < nf) {
    f[lane] = -2.0 * (Mq[obs_tri(V, lane + 1, V - 1)] - Mq[obs_tri(V, 0, lane + 1)]);
    double lo = -1.0, hi = 1.0;
    if (flags & KP_OBS_RATE) {
      const double wp = wprev[(size_t)w * NW + lane];
      lo = fmax(lo, wp - 0.01);
      hi = fmin(hi, wp + 0.01);
    }
    val[2 * lane] = 1.0; col[2 * lane] = lane; nrm[2 * lane] = 1.0; bq[2 * lane] = hi;
    val[2 * lane + 1] = -1.0; col[2 * lane + 1] = lane; nrm[2 * lane + 1] = 1.0; bq[2 * lane + 1] = -lo;
  }
  WSYNC();
  // positive definite Hessian of the free loads: Cholesky pivots above OBS_PIVOT_TOL of their diagonal entries (a window
  // whose rows do not determine the loads - e.g. one of zero-padded rows only with nw > nz - has no unique estimate)
  if (lane == 0) {
    int bad = !finite || nt < nf;              // fewer rows than free loads: singular whatever the rounding says
    double* L = ws + ObsLayout::QWS;           // (the solver's scratch, free until the solve)
    for (int k = 0; k < nf && !bad; ++k) {
      for (int i = k; i < nf; ++i) {
        double s = H[i + k * nf];
        for (int p = 0; p < k; ++p) s -= L[i + p * nf] * L[k + p * nf];
        if (i == k) {
          if (!(s > OBS_PIVOT_TOL * H[k + k * nf])) { bad = 1; break; }
          L[k + k * nf] = sqrt(s);
        } else {
          L[i + k * nf] = s / L[k + k * nf];
        }
      }
    }
    *flag = bad;
  }
  WSYNC();
  int st = *flag;
  if (!st && nf > 0) st = qp_goldfarb_idnani(H, f, EllMat{val, col, nrm, 1}, bq, nf, 2 * nf, ws + ObsLayout::QWS, x, 1e-10);
  WSYNC();
  if (lane <= NW) xw[lane] = lane == 0 ? 1.0 : (lane <= nf ? x[lane - 1] : 0.0);
  WSYNC();
  // resnorm = ||R [1; w] - d||^2 from the rows
  double xr[NW1];
#pragma unroll
  for (int l = 0; l < NW1; ++l) xr[l] = xw[l];
  double s = 0.0;
  for (int t = lane; t < nt; t += 64) {
    double r_ = -R[(size_t)t * V + NW1];
#pragma unroll
    for (int l = 0; l < NW1; ++l) r_ += R[(size_t)t * V + l] * xr[l];
    s += r_ * r_;
  }
  s = wave_sum(s);
  if (lane < NW) what[(size_t)w * NW + lane] = st ? __builtin_nan("") : xr[lane + 1];
  if (lane == 0) {
    resnorm[w] = st ? __builtin_nan("") : s;
    status[w] = st ? KP_ERR_QP_FAIL : KP_OK;
  }
}

typedef void (*obs_window_fn)(const double*, int, int, const int64_t*, int64_t, int64_t, const double*, int, double*, double*, int*);
static obs_window_fn obs_window_kernel(int nw) {
  switch (nw) {
    case 1: return kp_obs_window_kernel<2>;
    case 2: return kp_obs_window_kernel<3>;
    case 3: return kp_obs_window_kernel<4>;
    case 4: return kp_obs_window_kernel<5>;
    case 5: return kp_obs_window_kernel<6>;
    case 6: return kp_obs_window_kernel<7>;
    case 7: return kp_obs_window_kernel<8>;
    default: return kp_obs_window_kernel<9>;
  }
}

extern "C" int kp_load_observe(kp_ctx* ctx, const kp_basis* basis, int model_type, const double* A, const double* B, int nw,
                               int64_t rows, const double* zeta, const double* u, int ntrials, const int64_t* trial_off,
                               int64_t nwin, const int32_t* win_trial, const int64_t* win_start, int hor,
                               const double* whatpast, int flags, double* what, double* resnorm, int* status) {
  if (!ctx) return KP_ERR_ARG;
  if (!basis || !A || !B) return ctx->fail(KP_ERR_ARG, "kp_load_observe: NULL basis or model");
  if (model_type != KP_MODEL_LINEAR && model_type != KP_MODEL_BILINEAR)
    return ctx->fail(KP_ERR_ARG, "kp_load_observe: model_type must be linear or bilinear (there is no observer of a nonlinear loaded model)");
  if (nw < 1 || nw > OBS_MAX_NW) return ctx->fail(KP_ERR_ARG, "kp_load_observe: nw = " + std::to_string(nw) + " outside 1..8");
  if (hor < 2 || hor > OBS_MAX_HOR)
    return ctx->fail(KP_ERR_ARG, "kp_load_observe: hor = " + std::to_string(hor) + " outside 2..1025 (1 to 1024 pairs per window)");
  if (flags & ~(KP_OBS_RATE | KP_OBS_PIN_LAST)) return ctx->fail(KP_ERR_ARG, "kp_load_observe: unknown flags");
  if ((flags & KP_OBS_RATE) && nwin > 0 && !whatpast) return ctx->fail(KP_ERR_ARG, "kp_load_observe: KP_OBS_RATE needs whatpast");
  const BasisDev& bd = basis->dev;
  if (bd.model_type == KP_MODEL_NONLINEAR) return ctx->fail(KP_ERR_ARG, "kp_load_observe: basis must be a linear or bilinear dictionary");
  const int nz = bd.nzeta, m = bd.m, Nb = bd.N, nw1 = nw + 1;
  const int64_t NL = (int64_t)Nb * nw1;
  if (m < 1) return ctx->fail(KP_ERR_ARG, "kp_load_observe: the dictionary has no inputs");
  if (ntrials < 1 || rows < 0 || nwin < 0 || !trial_off)
    return ctx->fail(KP_ERR_ARG, "kp_load_observe: bad trial table");
  if (trial_off[0] != 0 || trial_off[ntrials] != rows) return ctx->fail(KP_ERR_ARG, "kp_load_observe: trial_off must run from 0 to rows");
  for (int t = 0; t < ntrials; ++t)
    if (trial_off[t + 1] < trial_off[t]) return ctx->fail(KP_ERR_ARG, "kp_load_observe: trial_off must not decrease");
  if (nwin == 0) return KP_OK;
  if (!zeta || !u || !win_trial || !win_start || !what || !resnorm || !status)
    return ctx->fail(KP_ERR_ARG, "kp_load_observe: NULL pointer");
  // first pair row of every window (global row)
  std::vector<int64_t> grow((size_t)nwin);
  for (int64_t w = 0; w < nwin; ++w) {
    const int32_t t = win_trial[w];
    const int64_t s = win_start[w];
    if (t < 0 || t >= ntrials || s < 0 || s + hor > trial_off[t + 1] - trial_off[t])
      return ctx->fail(KP_ERR_ARG, "kp_load_observe: window " + std::to_string(w) + " lies outside its trial");
    grow[w] = trial_off[t] + s;
  }
  // stacked row blocks: Gs[(j nz + r) nw1 + l][c] = (j == 0 ? A : B_{j-1})[r, l Nb + c]; CB = B[:nz, :] (linear)
  const bool bil = model_type == KP_MODEL_BILINEAR;
  const int nG = bil ? m + 1 : 1;
  std::vector<double> Gs((size_t)nG * nz * nw1 * Nb), CB((size_t)nz * m, 0.0);
  for (int j = 0; j < nG; ++j)
    for (int r = 0; r < nz; ++r)
      for (int l = 0; l < nw1; ++l)
        for (int c = 0; c < Nb; ++c) {
          const int64_t colA = (int64_t)l * Nb + c;
          Gs[(((size_t)j * nz + r) * nw1 + l) * Nb + c] = j == 0 ? A[r + colA * NL] : B[r + ((int64_t)(j - 1) * NL + colA) * NL];
        }
  if (!bil)
    for (int j = 0; j < m; ++j)
      for (int r = 0; r < nz; ++r) CB[r + (size_t)j * nz] = B[r + (int64_t)j * NL];

  // chunks: consecutive windows whose pair rows span at most cap rows (psi + blocks within OBS_WS_BUDGET)
  const size_t row_bytes = (size_t)(Nb + nz * (nw1 + 1)) * 8;
  const int64_t cap = std::max<int64_t>((int64_t)(OBS_WS_BUDGET / row_bytes), hor);
  struct Chunk { int64_t w0, nw, lo, hi; };
  std::vector<Chunk> chunks;
  int64_t max_span = 0;
  for (int64_t w = 0; w < nwin;) {
    int64_t lo = grow[w], hi = grow[w] + hor - 1, e = w + 1;
    while (e < nwin) {
      const int64_t lo2 = std::min(lo, grow[e]), hi2 = std::max(hi, grow[e] + hor - 1);
      if (hi2 - lo2 > cap) break;
      lo = lo2; hi = hi2; ++e;
    }
    chunks.push_back({w, e - w, lo, hi});
    max_span = std::max(max_span, hi - lo);
    w = e;
  }

  KP_HIP(ctx, hipSetDevice(ctx->device));
  // workspace: zeta | u | Gs | CB | whatpast | wrow (chunk-relative) | what | resnorm | Psi | Rd | status
  const size_t nZ = (size_t)rows * nz, nU = (size_t)rows * m, nWp = (flags & KP_OBS_RATE) ? (size_t)nwin * nw : 0;
  const size_t nPsi = (size_t)max_span * Nb, nRd = (size_t)max_span * nz * (nw1 + 1);
  const size_t doubles = nZ + nU + Gs.size() + CB.size() + nWp + (size_t)nwin /*wrow*/ + (size_t)nwin * nw + nwin + nPsi + nRd;
  const size_t bytes = doubles * 8 + (size_t)nwin * 4 + 64;
  double* d = (double*)ctx->workspace(20, bytes);
  if (!d) return ctx->fail(KP_ERR_HIP, "kp_load_observe: out of device memory (" + std::to_string(bytes) + " bytes)");
  double* dZ = d;
  double* dU = dZ + nZ;
  double* dGs = dU + nU;
  double* dCB = dGs + Gs.size();
  double* dWp = dCB + CB.size();
  int64_t* dWrow = (int64_t*)(dWp + nWp);
  double* dWhat = (double*)(dWrow + nwin);
  double* dRes = dWhat + (size_t)nwin * nw;
  double* dPsi = dRes + nwin;
  double* dRd = dPsi + nPsi;
  int* dSt = (int*)(dRd + nRd);
  std::vector<int64_t> wrow((size_t)nwin);
  for (const Chunk& c : chunks)
    for (int64_t w = c.w0; w < c.w0 + c.nw; ++w) wrow[w] = grow[w] - c.lo;
  hipStream_t st = ctx->stream;
  KP_HIP(ctx, hipMemcpyAsync(dZ, zeta, nZ * 8, hipMemcpyHostToDevice, st));
  KP_HIP(ctx, hipMemcpyAsync(dU, u, nU * 8, hipMemcpyHostToDevice, st));
  KP_HIP(ctx, hipMemcpyAsync(dGs, Gs.data(), Gs.size() * 8, hipMemcpyHostToDevice, st));
  if (!bil) KP_HIP(ctx, hipMemcpyAsync(dCB, CB.data(), CB.size() * 8, hipMemcpyHostToDevice, st));
  if (nWp) KP_HIP(ctx, hipMemcpyAsync(dWp, whatpast, nWp * 8, hipMemcpyHostToDevice, st));
  KP_HIP(ctx, hipMemcpyAsync(dWrow, wrow.data(), (size_t)nwin * 8, hipMemcpyHostToDevice, st));
  KP_HIP(ctx, hipEventRecord(ctx->ev0, st));
  const size_t lds = (size_t)OBS_WAVES * obs_wave_doubles() * 8;
  const obs_window_fn wk = obs_window_kernel(nw);
  for (const Chunk& c : chunks) {
    const int64_t nr = c.hi - c.lo;   // rows that start a pair of some window of the chunk
    int rc = kp_lift_dev_ld(ctx, basis, KP_LIFT_ECON, dZ + c.lo, nullptr, nr, rows, dPsi, nr);
    if (rc) return rc;
    const int64_t total = nr * nz * (nw1 + 1);
    const unsigned gb = (unsigned)std::min<int64_t>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(kp_obs_blocks_kernel, dim3(gb), dim3(256), 0, st, dPsi, nr, c.lo, dZ, dU, rows, dGs, dCB, nz, nw1, Nb,
                       m, bil ? 1 : 0, dRd);
    KP_HIP(ctx, hipGetLastError());
    const unsigned gw = (unsigned)((c.nw + OBS_WAVES - 1) / OBS_WAVES);
    hipLaunchKernelGGL(wk, dim3(gw), dim3(256), lds, st, dRd, nz, hor - 1, dWrow + c.w0, c.w0, c.nw, dWp, flags, dWhat, dRes, dSt);
    KP_HIP(ctx, hipGetLastError());
  }
  KP_HIP(ctx, hipEventRecord(ctx->ev1, st));
  KP_HIP(ctx, hipMemcpyAsync(what, dWhat, (size_t)nwin * nw * 8, hipMemcpyDeviceToHost, st));
  KP_HIP(ctx, hipMemcpyAsync(resnorm, dRes, (size_t)nwin * 8, hipMemcpyDeviceToHost, st));
  KP_HIP(ctx, hipMemcpyAsync(status, dSt, (size_t)nwin * 4, hipMemcpyDeviceToHost, st));
  KP_HIP(ctx, hipStreamSynchronize(st));
  float ms = 0;
  (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
  ctx->timers[4] = ms;
  return KP_OK;
}
