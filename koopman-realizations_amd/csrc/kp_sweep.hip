// =====================================================================================================================
// evaluate_rand_models.m:45-144 with the data resident on the device: trajectories uploaded once (kp_traj), then per
// (model type, degree) ONE call does scaling + snapshot pairs + fit (kp_small_fit_kernel) + model extraction (M-projection
// of get_model for linear models) + the validation rollout + the normalised mean error (:69-72), and only the error
// table entries come back.
// =====================================================================================================================
#include "kp_small_tile.h"
#include "kp_sweep_plan.h"
#include <vector>

// Validation rollout + error of one fitted model per system, one wave per system (N <= 16): val_model / val_BLmodel /
// val_NLmodel (Ksysid.m:1623-1879) on the scaled validation trial, then evaluate_rand_models.m:70-72:
// err_j = mean_t |y_sim - y_real|_j / (sum_t |y_real|_j / T).  Lane r owns component r of the lifted state.
// Ks: this system's K (column-major, leading dimension W); Aps / Bps: its projected A (N x N), B (N x m) for linear models
__device__ __forceinline__ void sweep_rollout_body(const BasisDev& b, const double* __restrict__ Ks, const double* __restrict__ Aps,
                                                   const double* __restrict__ Bps, const double* __restrict__ yv,
                                                   const double* __restrict__ uv, int Tv, int bad_fit, double* __restrict__ err_sys,
                                                   double* vsh) {
  const int lane = threadIdx.x;
  const int N = b.N, W = b.W, n = b.nzeta, m = b.m, mt = b.model_type;
  const int r = lane < N ? lane : 0;
  double arow[16], brow[3][16];
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    arow[c] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) brow[i][c] = 0.0;
  }
  if (mt == KP_MODEL_LINEAR) {          // projected model M A, M B (get_model, Ksysid.m:1224-1225)
#pragma unroll
    for (int c = 0; c < 16; ++c) if (c < N) arow[c] = Aps[(size_t)c * N + r];
#pragma unroll
    for (int i = 0; i < 3; ++i) if (i < m) brow[i][0] = Bps[(size_t)i * N + r];
  } else if (mt == KP_MODEL_BILINEAR) { // A = UT(1:N,1:N), B = UT(1:N,N+1:end), UT = K' (get_BLmodel, Ksysid.m:1250-1259)
#pragma unroll
    for (int c = 0; c < 16; ++c)
      if (c < N) {
        arow[c] = Ks[c + (size_t)r * W];
#pragma unroll
        for (int i = 0; i < 3; ++i) if (i < m) brow[i][c] = Ks[N + N * i + c + (size_t)r * W];
      }
  } else {                              // F = K(:,1:nzeta)' basis (get_NLmodel, Ksysid.m:1325-1329): lane c keeps column c of Kf
#pragma unroll
    for (int q = 0; q < 16; ++q) if (q < n) arow[q] = Ks[r + (size_t)q * W];
  }
  // scaled first validation row -> lifted state
  if (lane < n) vsh[lane] = yv[(size_t)lane * Tv];
  if (mt == KP_MODEL_NONLINEAR && lane < m) vsh[n + lane] = uv[(size_t)lane * Tv];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  double z = 0.0;
  if (mt != KP_MODEL_NONLINEAR) { if (lane < N) z = kp_eval_col(b, b.cols[lane], vsh, 1); }
  else if (lane < n) z = vsh[lane];
  double acc_e = 0.0, acc_a = 0.0;
  for (int t = 0; t < Tv; ++t) {
    if (lane < n) {
      const double yr = yv[(size_t)lane * Tv + t];
      if (t > 0) acc_e += fabs(z - yr);               // the first simulated row is the measured one (Ksysid.m:1654)
      acc_a += fabs(yr);
    }
    if (t == Tv - 1) break;
    double ut[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 3; ++i) if (i < m) ut[i] = uv[(size_t)i * Tv + t];
    double zn = 0.0;
    if (mt == KP_MODEL_LINEAR) {
#pragma unroll
      for (int c = 0; c < 16; ++c) if (c < N) zn += arow[c] * sb_bcast(z, c);
#pragma unroll
      for (int i = 0; i < 3; ++i) if (i < m) zn += brow[i][0] * ut[i];
    } else if (mt == KP_MODEL_BILINEAR) {              // z+ = A z + sum_i u_i B_i z (val_BLmodel, Ksysid.m:1772-1787)
#pragma unroll
      for (int c = 0; c < 16; ++c)
        if (c < N) {
          double w = arow[c];
#pragma unroll
          for (int i = 0; i < 3; ++i) if (i < m) w += ut[i] * brow[i][c];
          zn += w * sb_bcast(z, c);
        }
    } else {                                           // zeta+ = Kf psi([zeta; u]) (val_NLmodel, Ksysid.m:1848-1863)
      if (lane < n) vsh[lane] = z;
      if (lane < m) vsh[n + lane] = ut[lane];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      const double psi = lane < N ? kp_eval_col(b, b.cols[lane], vsh, 1) : 0.0;
#pragma unroll
      for (int q = 0; q < 16; ++q)
        if (q < n) {
          double sacc = lane < N ? arow[q] * psi : 0.0;
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) sacc += __shfl_xor(sacc, o, 64);
          if (lane == q) zn = sacc;
        }
      __builtin_amdgcn_wave_barrier();
    }
    z = zn;
  }
  if (lane < n) {
    const double bad = bad_fit ? __builtin_nan("") : 0.0;
    err_sys[lane] = (acc_e / Tv) / (acc_a / Tv) + bad;
  }
}


__global__ __launch_bounds__(64) void kp_sweep_rollout_kernel(BasisDev b, const double* __restrict__ K, const double* __restrict__ Ap,
                                                              const double* __restrict__ Bp, const double* __restrict__ Yv,
                                                              const double* __restrict__ Uv, const double* __restrict__ scv, int Tv,
                                                              const int* __restrict__ fit_status, double* __restrict__ err) {
  __shared__ double vsh[KP_MAX_VARS];
  const int sys = blockIdx.x, n = b.nzeta, m = b.m;
  sweep_rollout_body(b, K + (size_t)sys * b.W * b.W, Ap ? Ap + (size_t)sys * b.N * b.N : nullptr, Bp ? Bp + (size_t)sys * b.N * m : nullptr,
                     Yv + (size_t)sys * Tv * n, Uv + (size_t)sys * Tv * m, Tv, fit_status && fit_status[sys], err + (size_t)sys * n, vsh);
}

__global__ void kp_l1_flag_kernel(const double* __restrict__ K, int W, double t, int* __restrict__ flags) {
  const int sys = blockIdx.x;
  double s = 0.0;
  for (int e = threadIdx.x; e < W * W; e += 64) s += fabs(K[(size_t)sys * W * W + e]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (threadIdx.x == 0) flags[sys] = s > t ? 1 : 0;
}

// Lasso rows of the sweep (nonlinear models, lasso = 4, evaluate_rand_models.m:122): the L1 row is active only when
// ||K_LS||_1 > t = lasso N, which the generated and shipped systems never reach.  The caller has launched its flag kernel into
// dF; the systems it flagged are re-solved here with kp_lasso_dev on (G, C).  System e lies at e * stride in dK, dG, dC, and
// width_t(e, &W, &t) tells its width and its t.
template <class WidthT>
static int sweep_l1_resolve(kp_ctx* ctx, const int* dF, size_t count, size_t stride, double* dK, double* dG, double* dC, WidthT width_t) {
  hipStream_t s = ctx->stream;
  KP_HIP(ctx, hipGetLastError());
  std::vector<int> flags(count);
  KP_HIP(ctx, hipMemcpyAsync(flags.data(), dF, count * 4, hipMemcpyDeviceToHost, s));
  KP_HIP(ctx, hipStreamSynchronize(s));
  for (size_t e = 0; e < count; ++e)
    if (flags[e]) {
      int W = 0;
      double t = 0.0;
      width_t(e, &W, &t);
      int rc = kp_lasso_dev(ctx, dG + e * stride, dC + e * stride, W, W, t, 20000, 1e-10, dK + e * stride, nullptr);
      if (rc && rc != KP_ERR_NOT_CONVERGED) return rc;
    }
  return KP_OK;
}

extern "C" int kp_sweep_eval(kp_ctx* ctx, const kp_traj* traj, const kp_basis* basis, double lasso, double* err_out, double* K_out,
                             int* status_out) {
  if (!ctx || !traj || !basis || !err_out) return ctx ? ctx->fail(KP_ERR_ARG, "kp_sweep_eval: bad argument") : KP_ERR_ARG;
  if (traj->have != 31) return ctx->fail(KP_ERR_ARG, "kp_sweep_eval: trajectory object not finished (kp_traj_finish)");
  const BasisDev& b = basis->dev;
  if (b.nzeta != traj->n || b.m != traj->m) return ctx->fail(KP_ERR_ARG, "kp_sweep_eval: trajectory / dictionary dimension mismatch");
  if (b.W > SB_W || b.k_pcs != 0 || b.N != b.nfull || b.m > 3) return ctx->fail(KP_ERR_ARG, "kp_sweep_eval: needs W <= 16, m <= 3 and no dimension reduction");
  KP_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->async_pending) {
    int rc0 = kp_synchronize(ctx);
    if (rc0) return rc0;
  }
  const int nb = traj->nb, W = b.W, N = b.N, n = traj->n, m = traj->m;
  const int Ns = traj->ntrials * (traj->T - 1) - 1;            // get_snapshotPairs: #good - 1 (Ksysid.m:960)
  const size_t bW = (size_t)nb * W * W * 8, bA = (size_t)nb * N * N * 8, bB = (size_t)nb * N * m * 8;
  char* ws = (char*)ctx->workspace(6, 3 * bW + bA + bB + (size_t)nb * (n * 8 + 12) + 256);
  if (!ws) return ctx->fail(KP_ERR_HIP, "kp_sweep_eval: out of device memory");
  double *dK = (double*)ws, *dG = (double*)(ws + bW), *dC = (double*)(ws + 2 * bW);
  double *dA = (double*)(ws + 3 * bW), *dB = (double*)(ws + 3 * bW + bA), *dE = (double*)(ws + 3 * bW + bA + bB);
  int* dS = (int*)(dE + (size_t)nb * n);
  int* dF = dS + nb;
  hipStream_t s = ctx->stream;
  KP_HIP(ctx, hipEventRecord(ctx->ev0, s));
  const bool use_rec = kp_small_fit_launch(ctx, basis, nb, nullptr, nullptr, nullptr, 0, Ns, traj_view(traj), dK, dG, dC, dS);
  KP_HIP(ctx, hipGetLastError());
  KP_HIP(ctx, hipEventRecord(ctx->ev1, s));
  if (lasso < 1e6) {
    const double t = lasso * N;
    hipLaunchKernelGGL(kp_l1_flag_kernel, dim3(nb), dim3(64), 0, s, dK, W, t, dF);
    int rc = sweep_l1_resolve(ctx, dF, nb, (size_t)W * W, dK, dG, dC, [&](size_t, int* We, double* te) { *We = W; *te = t; });
    if (rc) return rc;
  }
  if (b.model_type == KP_MODEL_LINEAR) {
    kp_small_project_launch(ctx, nb, dK, dG, dC, N, m, dA, dB, nullptr, nullptr);
    KP_HIP(ctx, hipGetLastError());
  }
  hipLaunchKernelGGL(kp_sweep_rollout_kernel, dim3(nb), dim3(64), 0, s, b, dK, dA, dB, traj->Yv, traj->Uv, traj->sc, traj->Tv, dS, dE);
  KP_HIP(ctx, hipGetLastError());
  ctx->timers[14] = (use_rec ? 5000.0 : 6000.0) + 3.0;   // kp_small_fit_kernel with / without recipes, kp_sweep_rollout_kernel
  KP_HIP(ctx, hipMemcpyAsync(err_out, dE, (size_t)nb * n * 8, hipMemcpyDeviceToHost, s));
  if (K_out) KP_HIP(ctx, hipMemcpyAsync(K_out, dK, bW, hipMemcpyDeviceToHost, s));
  if (status_out) KP_HIP(ctx, hipMemcpyAsync(status_out, dS, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
  return kp_sync_timer0(ctx);
}

// ---- the nested sweep: all degrees of one model type from ONE pass over the data (how, and the host plan: kp_sweep_plan.h) ----

__global__ __launch_bounds__(256) void kp_sweep_sub_kernel(const double* __restrict__ Gc, const double* __restrict__ Cc, int Wmax, int nb,
                                                           const SweepDeg* __restrict__ degs, const int* __restrict__ fit_status,
                                                           double* __restrict__ Kall, double* __restrict__ Gall,
                                                           double* __restrict__ Call, int* __restrict__ stat) {
  __shared__ double Gs[16 * SB_LD], Cs[16 * SB_LD], Xs[16 * SB_LD], Ls[16 * SB_LD], Dd[16], T1[16 * SB_LD], T2[16 * SB_LD], Sf[16 * SB_LD],
      Ti[16 * SB_LD];
  __shared__ int bad;
  const int tid = threadIdx.x, i = tid >> 4, j = tid & 15, sys = blockIdx.x, dj = blockIdx.y;
  const SweepDeg& d = degs[dj];
  const int W = d.W;
  const double* G0 = Gc + (size_t)sys * Wmax * Wmax;
  const double* C0 = Cc + (size_t)sys * Wmax * Wmax;
  const bool in = i < W && j < W;
  Gs[i * SB_LD + j] = in ? G0[d.idx[i] + (size_t)d.idx[j] * Wmax] : (i == j ? 1.0 : 0.0);
  Cs[i * SB_LD + j] = in ? C0[d.idx[i] + (size_t)d.idx[j] * Wmax] : 0.0;
  Sf[i * SB_LD + j] = d.Sf[i * 16 + j];
  Ti[i * SB_LD + j] = d.Tinv[i * 16 + j];
  if (tid == 0) bad = 0;
  __syncthreads();
  sb_spd_solve16(Gs, Cs, Xs, Ls, Dd, &bad);                       // Xs = K_c
  double a = 0.0, g = 0.0, c = 0.0;                                // X T, G S', C S'  (T[k][j] = Sf[j][k])
  for (int k = 0; k < 16; ++k) {
    const double sjk = Sf[j * SB_LD + k];
    a += Xs[i * SB_LD + k] * sjk;
    g += Gs[i * SB_LD + k] * sjk;
    c += Cs[i * SB_LD + k] * sjk;
  }
  __syncthreads();
  T1[i * SB_LD + j] = a; T2[i * SB_LD + j] = g; Ls[i * SB_LD + j] = c;
  __syncthreads();
  double km = 0.0, gm = 0.0, cm = 0.0;
  for (int k = 0; k < 16; ++k) {
    km += Ti[i * SB_LD + k] * T1[k * SB_LD + j];
    gm += Sf[i * SB_LD + k] * T2[k * SB_LD + j];
    cm += Sf[i * SB_LD + k] * Ls[k * SB_LD + j];
  }
  const size_t o = ((size_t)dj * nb + sys) * 256;
  const int isbad = bad || (fit_status && fit_status[sys]);
  if (in) {
    Kall[o + (size_t)j * W + i] = isbad ? __builtin_nan("") : km;
    Gall[o + (size_t)j * W + i] = gm;
    Call[o + (size_t)j * W + i] = cm;
  }
  if (tid == 0) stat[(size_t)dj * nb + sys] = isbad;
}

// kp_small_project_kernel for every (system, degree) of a nested linear sweep
__global__ __launch_bounds__(256) void kp_sweep_project_kernel(const double* __restrict__ Kall, const double* __restrict__ Gall,
                                                               const double* __restrict__ Call, int nb, int m, const SweepDeg* __restrict__ degs,
                                                               double* __restrict__ Aall, double* __restrict__ Ball) {
  __shared__ double Ks[16 * SB_LD], Gs[16 * SB_LD], Cs[16 * SB_LD], Ts[16 * SB_LD], LL[16 * SB_LD], LR[16 * SB_LD], Ms[16 * SB_LD], Ls[16 * SB_LD], Dd[16];
  __shared__ int bad;
  const int tid = threadIdx.x, i = tid >> 4, j = tid & 15, sys = blockIdx.x, dj = blockIdx.y;
  const int N = degs[dj].N, W = N + m;
  const size_t off = ((size_t)dj * nb + sys) * 256;
  const bool in = i < W && j < W;
  Ks[i * SB_LD + j] = in ? Kall[off + (size_t)j * W + i] : 0.0;
  Gs[i * SB_LD + j] = in ? Gall[off + (size_t)j * W + i] : 0.0;
  Cs[i * SB_LD + j] = in ? Call[off + (size_t)j * W + i] : 0.0;
  if (tid == 0) bad = 0;
  __syncthreads();
  double t = 0.0;
  if (j < N)
    for (int w = 0; w < W; ++w) t += Gs[i * SB_LD + w] * Ks[w * SB_LD + j];
  Ts[i * SB_LD + j] = t;
  __syncthreads();
  double ll = 0.0, lr = 0.0;
  if (i < N && j < N)
    for (int w = 0; w < W; ++w) {
      ll += Ks[w * SB_LD + i] * Ts[w * SB_LD + j];
      lr += Ks[w * SB_LD + i] * Cs[w * SB_LD + j];
    }
  LL[i * SB_LD + j] = (i < N && j < N) ? ll : (i == j ? 1.0 : 0.0);
  LR[i * SB_LD + j] = (i < N && j < N) ? lr : 0.0;
  __syncthreads();
  sb_spd_solve16(LL, LR, Ms, Ls, Dd, &bad);
  const double nanv = __builtin_nan("");
  double a = 0.0, b = 0.0;
  if (i < N)
    for (int k = 0; k < N; ++k) {
      const double mik = Ms[k * SB_LD + i];
      if (j < N) a += mik * Ks[j * SB_LD + k];
      if (j < m) b += mik * Ks[(N + j) * SB_LD + k];
    }
  if (i < N && j < N) Aall[off + (size_t)j * N + i] = bad ? nanv : a;
  if (i < N && j < m) Ball[off + (size_t)j * N + i] = bad ? nanv : b;
}

__global__ __launch_bounds__(64) void kp_sweep_rollout_nested_kernel(BasisDev b, const SweepDeg* __restrict__ degs, const ColDesc* __restrict__ cols_all,
                                                                     int nb, const double* __restrict__ Kall, const double* __restrict__ Aall,
                                                                     const double* __restrict__ Ball, const double* __restrict__ Yv,
                                                                     const double* __restrict__ Uv, int Tv, const int* __restrict__ stat,
                                                                     double* __restrict__ err) {
  __shared__ double vsh[KP_MAX_VARS];
  const int sys = blockIdx.x, dj = blockIdx.y, n = b.nzeta, m = b.m;
  BasisDev bj = b;
  bj.N = degs[dj].N; bj.W = degs[dj].W; bj.nfull = bj.N; bj.cols = cols_all + (size_t)dj * 16;
  const size_t off = ((size_t)dj * nb + sys) * 256;
  sweep_rollout_body(bj, Kall + off, Aall ? Aall + off : nullptr, Ball ? Ball + off : nullptr, Yv + (size_t)sys * Tv * n, Uv + (size_t)sys * Tv * m,
                     Tv, stat[(size_t)dj * nb + sys], err + ((size_t)dj * nb + sys) * n, vsh);
}

// Validation rollouts of the nested sweep, FOUR (system, degree) jobs per wave: a job lives in one 16-lane row (N <= 16),
// lane r of the row owns component r of the lifted state.  z+ = A z column by column: z[c] is broadcast inside every row by
// a DPP row_newbcast move and lane r adds A[r][c] z[c] - N moves + N FMAs per step for all four jobs, instead of sixteen
// v_readlane broadcasts per job.
// MT: the model type at compile time - the row of B_i (96 registers) exists only in the bilinear instantiation; with the type
// a run-time value every instantiation carried it, 2 waves per SIMD fitted and the 3328 waves of the linear pass (13 degrees
// x 1024 systems) ran in two rounds.
template <int MT>
__global__ __launch_bounds__(64) void kp_sweep_rollout4_kernel(BasisDev b, const SweepDeg* __restrict__ degs, const ColDesc* __restrict__ cols_all,
                                                               int nb, int n_deg, const double* __restrict__ Kall, const double* __restrict__ Aall,
                                                               const double* __restrict__ Ball, const double* __restrict__ Yv,
                                                               const double* __restrict__ Uv, int Tv, const int* __restrict__ stat,
                                                               double* __restrict__ err) {
  __shared__ double vsh[4][KP_MAX_VARS];
  const int lane = threadIdx.x, q = lane >> 4, r = lane & 15;
  const int njobs = nb * n_deg;
  int job = blockIdx.x * 4 + q;
  const bool live = job < njobs;
  if (!live) job = njobs - 1;
  const int dj = job / nb, sys = job - dj * nb;
  const int n = b.nzeta, m = b.m;
  constexpr int mt = MT;
  const int N = degs[dj].N, W = degs[dj].W;
  BasisDev bj = b;
  bj.N = N; bj.W = W; bj.nfull = N; bj.cols = cols_all + (size_t)dj * 16;
  const size_t off = ((size_t)dj * nb + sys) * 256;
  const double* Ks = Kall + off;
  const double* yv = Yv + (size_t)sys * Tv * n;
  const double* uv = Uv + (size_t)sys * Tv * m;
  const bool rin = r < N;
  // row r of the model matrices: ak[c] = A[r][c], bk[i][c] = B_i[r][c]
  constexpr int NBK = MT == KP_MODEL_BILINEAR ? 3 : 1;      // (a zero-length array is not allowed)
  double ak[16], bk[NBK][16], bl[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    const bool in = rin && c < N;
    double a = 0.0;
    if (mt == KP_MODEL_LINEAR) a = in ? Aall[off + (size_t)c * N + r] : 0.0;
    else if (mt == KP_MODEL_BILINEAR) a = in ? Ks[c + (size_t)r * W] : 0.0;
    ak[c] = a;
    if constexpr (MT == KP_MODEL_BILINEAR) {
#pragma unroll
      for (int i = 0; i < 3; ++i) bk[i][c] = (i < m && in) ? Ks[N + N * i + c + (size_t)r * W] : 0.0;
    } else {
      bk[0][c] = 0.0;
    }
  }
  // columns to visit: the widest of the wave's four jobs (consecutive jobs share their degree except at a boundary)
  int Nw = N;
  Nw = max(Nw, __builtin_amdgcn_readlane(N, 16));
  Nw = max(Nw, __builtin_amdgcn_readlane(N, 32));
  Nw = max(Nw, __builtin_amdgcn_readlane(N, 48));
  Nw = __builtin_amdgcn_readfirstlane(max(Nw, __builtin_amdgcn_readlane(N, 0)));
  if (mt == KP_MODEL_LINEAR)
#pragma unroll
    for (int i = 0; i < 3; ++i) bl[i] = (i < m && rin) ? Ball[off + (size_t)i * N + r] : 0.0;
  double kf[4] = {0.0, 0.0, 0.0, 0.0};             // nonlinear: lane c keeps column c of Kf = K(:, 1:n)' (n <= 4 outputs)
  if (mt == KP_MODEL_NONLINEAR)
#pragma unroll
    for (int o = 0; o < 4; ++o) kf[o] = (o < n && rin) ? Ks[r + (size_t)o * W] : 0.0;
  // nonlinear: column r of the dictionary over [zeta; u] as packed exponents (4 bits per variable, <= 8 variables), so that a
  // step evaluates psi from registers - zeta_i by a DPP broadcast from lane i of the row, u_i from the lane's own copy -
  // instead of kp_eval_col's exponent bytes from global memory and the trip through LDS (two wave barriers per step)
  unsigned epack = 0;
  bool nl_fast = false;
  if constexpr (MT == KP_MODEL_NONLINEAR) {
    bool ok = n <= 4 && m <= 3;
    if (rin && ok) {
      const ColDesc c = bj.cols[r];
      if (c.kind == COL_VAR) epack = 1u << (4 * c.arg);
      else if (c.kind == COL_MONO) {
        for (int i = 0; i < bj.nvars; ++i) {
          const unsigned e = bj.exps[(size_t)c.arg * bj.nvars + i];
          ok = ok && e < 16;
          epack |= (e & 15u) << (4 * i);
        }
      } else if (c.kind != COL_CONST) ok = false;
    }
    nl_fast = __all(ok);
  }
  // first validation row -> lifted state
  if (r < n) vsh[q][r] = yv[(size_t)r * Tv];
  if (mt == KP_MODEL_NONLINEAR && r < m) vsh[q][n + r] = uv[(size_t)r * Tv];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  double z = 0.0;
  if (mt != KP_MODEL_NONLINEAR) { if (rin) z = kp_eval_col(bj, bj.cols[r], vsh[q], 1); }
  else if (r < n) z = vsh[q][r];
  double acc_e = 0.0, acc_a = 0.0;
  double yr = r < n ? yv[(size_t)r * Tv] : 0.0;
  double ut[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) ut[i] = i < m ? uv[(size_t)i * Tv] : 0.0;
  // The time loop with the column count of the wave's widest job as a compile-time constant: with `if (c < Nw)` around every
  // column the 16 scalar compare-and-branch pairs of a step cost a lone wave more than its arithmetic (0.4 us per step at
  // degree 13).  (Also measured: the trial fetched in 4-step register chunks a chunk ahead, or staged in LDS in 16-step
  // chunks, instead of the one-step-ahead loads below - no faster: the step time is the dependent chain, not the loads.)
  auto run = [&](auto nwc) {
    constexpr int NW = decltype(nwc)::value;
    for (int t = 0; t < Tv; ++t) {
      if (r < n) {
        if (t > 0) acc_e += fabs(z - yr);               // the first simulated row is the measured one (Ksysid.m:1654)
        acc_a += fabs(yr);
      }
      if (t == Tv - 1) break;
      const double yr_n = r < n ? yv[(size_t)r * Tv + t + 1] : 0.0;      // values of the next step: in flight during this one
      double ut_n[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) ut_n[i] = i < m ? uv[(size_t)i * Tv + t + 1] : 0.0;
      double zn = 0.0;
      if constexpr (MT != KP_MODEL_NONLINEAR) {
        // z+ = (A + sum_i u_i B_i) z  (val_model :1685 / val_BLmodel :1783); linear: B u added below.  z[c] reaches every
        // lane of its 16-lane row by ONE DP-ALU DPP move (v_mov_b64_dpp row_newbcast:c).  (Round 2 broadcast it with two
        // ds_swizzle per column: with 13 waves per CU the LDS crossbar was the bound.)  Two partial sums: half the chain.
        double zn1 = 0.0;
#define KP_COL_STEP(CC, ACC)                                                                                   \
        if constexpr (CC < NW) {                                                                                 \
          double w = ak[CC];                                                                                     \
          if constexpr (MT == KP_MODEL_BILINEAR) { w += ut[0] * bk[0][CC]; if (m > 1) w += ut[1] * bk[1][CC]; if (m > 2) w += ut[2] * bk[2][CC]; } \
          ACC += w * __builtin_amdgcn_update_dpp(0.0, z, 0x150 + (CC), 0xf, 0xf, true);                         \
        }
        KP_COL_STEP(0, zn) KP_COL_STEP(1, zn1) KP_COL_STEP(2, zn) KP_COL_STEP(3, zn1) KP_COL_STEP(4, zn) KP_COL_STEP(5, zn1)
        KP_COL_STEP(6, zn) KP_COL_STEP(7, zn1) KP_COL_STEP(8, zn) KP_COL_STEP(9, zn1) KP_COL_STEP(10, zn) KP_COL_STEP(11, zn1)
        KP_COL_STEP(12, zn) KP_COL_STEP(13, zn1) KP_COL_STEP(14, zn) KP_COL_STEP(15, zn1)
#undef KP_COL_STEP
        zn += zn1;
        if constexpr (MT == KP_MODEL_LINEAR) zn += bl[0] * ut[0] + bl[1] * ut[1] + bl[2] * ut[2];
      } else {                                           // zeta+ = Kf psi([zeta; u]) (val_NLmodel, Ksysid.m:1848-1863)
        double psi;
        if (nl_fast) {
          psi = rin ? 1.0 : 0.0;
#define KP_NL_VAR(I, X)                                                                  \
          {                                                                               \
            const double x_ = X;                                                          \
            const int e_ = (int)((epack >> (4 * (I))) & 15u);                             \
            for (int k_ = 0; k_ < e_; ++k_) psi *= x_;                                    \
          }
          KP_NL_VAR(0, __builtin_amdgcn_update_dpp(0.0, z, 0x150, 0xf, 0xf, true))
          if (n > 1) KP_NL_VAR(1, __builtin_amdgcn_update_dpp(0.0, z, 0x151, 0xf, 0xf, true))
          if (n > 2) KP_NL_VAR(2, __builtin_amdgcn_update_dpp(0.0, z, 0x152, 0xf, 0xf, true))
          if (n > 3) KP_NL_VAR(3, __builtin_amdgcn_update_dpp(0.0, z, 0x153, 0xf, 0xf, true))
          KP_NL_VAR(n, ut[0])
          if (m > 1) KP_NL_VAR(n + 1, ut[1])
          if (m > 2) KP_NL_VAR(n + 2, ut[2])
#undef KP_NL_VAR
        } else {
          if (r < n) vsh[q][r] = z;
          if (r < m) vsh[q][n + r] = ut[r];
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
          psi = rin ? kp_eval_col(bj, bj.cols[r], vsh[q], 1) : 0.0;
          __builtin_amdgcn_wave_barrier();
        }
#pragma unroll
        for (int o = 0; o < 4; ++o)
          if (o < n) {
            const double sacc = sb_row_sum(kf[o] * psi);
            if (r == o) zn = sacc;
          }
      }
      z = zn;
      yr = yr_n;
#pragma unroll
      for (int i = 0; i < 3; ++i) ut[i] = ut_n[i];
    }
  };
  if constexpr (MT == KP_MODEL_NONLINEAR) {
    run(std::integral_constant<int, 0>{});
  } else {
    switch (Nw) {
#define KP_NW_CASE(V) case V: run(std::integral_constant<int, V>{}); break;
      KP_NW_CASE(1) KP_NW_CASE(2) KP_NW_CASE(3) KP_NW_CASE(4) KP_NW_CASE(5) KP_NW_CASE(6) KP_NW_CASE(7) KP_NW_CASE(8)
      KP_NW_CASE(9) KP_NW_CASE(10) KP_NW_CASE(11) KP_NW_CASE(12) KP_NW_CASE(13) KP_NW_CASE(14) KP_NW_CASE(15)
#undef KP_NW_CASE
      default: run(std::integral_constant<int, 16>{}); break;
    }
  }
  if (live && r < n) {
    const double bad = stat[(size_t)dj * nb + sys] ? __builtin_nan("") : 0.0;
    err[((size_t)dj * nb + sys) * n + r] = (acc_e / Tv) / (acc_a / Tv) + bad;
  }
}

__global__ void kp_l1_flag_all_kernel(const double* __restrict__ Kall, const SweepDeg* __restrict__ degs, int nb, double lasso, int* __restrict__ flags) {
  const int sys = blockIdx.x, dj = blockIdx.y, W = degs[dj].W;
  const double* K = Kall + ((size_t)dj * nb + sys) * 256;
  double s = 0.0;
  for (int e = threadIdx.x; e < W * W; e += 64) s += fabs(K[e]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (threadIdx.x == 0) flags[(size_t)dj * nb + sys] = s > lasso * degs[dj].N ? 1 : 0;
}

// Byte offsets of the blocks of workspace 6 for a nested call (the layout is drawn in kp_internal.h): the one place that
// kp_sweep_eval_nested and kp_sweep_nested_get_K take them from.  Only the blocks behind B depend on n.
struct SweepWs {
  size_t Gc, Cc, K, G, C, A, B, E, S0, S, F, tab, cols, bytes;
  SweepWs(int nb, int Wmax, int n_deg, int n) {
    const size_t bW = (size_t)nb * Wmax * Wmax * 8, bAll = (size_t)n_deg * nb * 256 * 8, bI = (size_t)n_deg * nb * 4;
    Gc = 0; Cc = Gc + bW;
    K = Cc + bW; G = K + bAll; C = G + bAll; A = C + bAll; B = A + bAll;
    E = B + bAll;
    S0 = E + (size_t)n_deg * nb * n * 8; S = S0 + (size_t)nb * 4; F = S + bI;
    tab = (F + bI + 63) & ~(size_t)63;
    cols = (tab + (size_t)n_deg * sizeof(SweepDeg) + 63) & ~(size_t)63;
    bytes = cols + (size_t)n_deg * 16 * sizeof(ColDesc);
  }
};

extern "C" int kp_sweep_eval_nested(kp_ctx* ctx, const kp_traj* traj, const kp_basis* basis, double lasso, int n_deg, double* err_out,
                                    int* status_out) {
  if (!ctx || !traj || !basis || !err_out || n_deg < 1) return ctx ? ctx->fail(KP_ERR_ARG, "kp_sweep_eval_nested: bad argument") : KP_ERR_ARG;
  if (traj->have != 31) return ctx->fail(KP_ERR_ARG, "kp_sweep_eval_nested: trajectory object not finished (kp_traj_finish)");
  const BasisDev& b = basis->dev;
  if (b.nzeta != traj->n || b.m != traj->m) return ctx->fail(KP_ERR_ARG, "kp_sweep_eval_nested: trajectory / dictionary dimension mismatch");
  if (b.W > SB_W || b.k_pcs != 0 || b.N != b.nfull || b.m > 3 || !basis->fast || basis->h_recipes.size() != (size_t)b.nfull)
    return ctx->fail(KP_ERR_ARG, "kp_sweep_eval_nested: needs a polynomial dictionary with W <= 16, m <= 3 and no dimension reduction");
  KP_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->async_pending) {
    int rc0 = kp_synchronize(ctx);
    if (rc0) return rc0;
  }
  const int nb = traj->nb, n = traj->n, m = traj->m;
  // plan: per degree the columns, the basis change and the rollout's column descriptors (host arithmetic, kp_sweep_plan.h)
  SweepPlan plan;
  if (const char* refusal = sweep_plan_build(basis->h_recipes.data(), b.N, b.nvars, basis->pow_depth, b.model_type, m, n_deg, &plan))
    return ctx->fail(KP_ERR_ARG, refusal);
  // workspace
  const SweepWs L(nb, b.W, n_deg, n);
  char* ws = (char*)ctx->workspace(6, L.bytes);
  if (!ws) return ctx->fail(KP_ERR_HIP, "kp_sweep_eval_nested: out of device memory");
  double *dGc = (double*)(ws + L.Gc), *dCc = (double*)(ws + L.Cc), *dK = (double*)(ws + L.K), *dG = (double*)(ws + L.G), *dC = (double*)(ws + L.C);
  double *dA = (double*)(ws + L.A), *dB = (double*)(ws + L.B), *dE = (double*)(ws + L.E);
  int *dS0 = (int*)(ws + L.S0), *dS = (int*)(ws + L.S), *dF = (int*)(ws + L.F);
  SweepDeg* dT = (SweepDeg*)(ws + L.tab);
  ColDesc* dCols = (ColDesc*)(ws + L.cols);
  hipStream_t s = ctx->stream;
  KP_HIP(ctx, hipMemcpyAsync(dT, plan.degs.data(), plan.degs.size() * sizeof(SweepDeg), hipMemcpyHostToDevice, s));
  KP_HIP(ctx, hipMemcpyAsync(dCols, plan.cols.data(), plan.cols.size() * sizeof(ColDesc), hipMemcpyHostToDevice, s));
  KP_HIP(ctx, hipMemsetAsync(dS0, 0, (size_t)nb * 4, s));
  // Gram (degree D, internal basis), between the event pair
  const int Ns = traj->ntrials * (traj->T - 1) - 1;
  double code = 0.0;
  int rc = kp_sweep_gram_launch(ctx, traj, basis, Ns, plan.cheb, dGc, dCc, &code);
  if (rc) return rc;
  KP_HIP(ctx, hipEventRecord(ctx->ev1, s));
  // sub-block solve of every degree, back in the monomial basis
  const dim3 grid(nb, n_deg);
  hipLaunchKernelGGL(kp_sweep_sub_kernel, grid, dim3(256), 0, s, dGc, dCc, b.W, nb, dT, (const int*)nullptr, dK, dG, dC, dS);
  KP_HIP(ctx, hipGetLastError());
  if (lasso < 1e6) {                                  // L1 row active (never for the shipped / generated systems): lasso solve on (G_m, C_m)
    hipLaunchKernelGGL(kp_l1_flag_all_kernel, grid, dim3(64), 0, s, dK, dT, nb, lasso, dF);
    rc = sweep_l1_resolve(ctx, dF, (size_t)n_deg * nb, 256, dK, dG, dC,
                          [&](size_t e, int* We, double* te) { *We = plan.degs[e / nb].W; *te = lasso * plan.degs[e / nb].N; });
    if (rc) return rc;
  }
  const bool lin = b.model_type == KP_MODEL_LINEAR;
  if (lin) {
    hipLaunchKernelGGL(kp_sweep_project_kernel, grid, dim3(256), 0, s, dK, dG, dC, nb, m, dT, dA, dB);
    KP_HIP(ctx, hipGetLastError());
  }
  // validation rollouts
  static const bool rollout4 = getenv("KP_SWEEP_NO_ROLLOUT4") == nullptr;
  if (rollout4 && n <= 4) {
#define KP_ROLL4(MT_) hipLaunchKernelGGL(kp_sweep_rollout4_kernel<MT_>, dim3((nb * n_deg + 3) / 4), dim3(64), 0, s, b, dT, dCols, nb, n_deg, dK, \
                                         MT_ == KP_MODEL_LINEAR ? dA : nullptr, MT_ == KP_MODEL_LINEAR ? dB : nullptr, traj->Yv, traj->Uv, traj->Tv, dS, dE)
    if (lin) KP_ROLL4(KP_MODEL_LINEAR);
    else if (b.model_type == KP_MODEL_BILINEAR) KP_ROLL4(KP_MODEL_BILINEAR);
    else KP_ROLL4(KP_MODEL_NONLINEAR);
#undef KP_ROLL4
  } else
    hipLaunchKernelGGL(kp_sweep_rollout_nested_kernel, grid, dim3(64), 0, s, b, dT, dCols, nb, dK, lin ? dA : nullptr, lin ? dB : nullptr, traj->Yv,
                       traj->Uv, traj->Tv, dS, dE);
  KP_HIP(ctx, hipGetLastError());
  ctx->timers[14] = code + (rollout4 && n <= 4 ? 1.0 : 2.0);
  KP_HIP(ctx, hipMemcpyAsync(err_out, dE, (size_t)n_deg * nb * n * 8, hipMemcpyDeviceToHost, s));
  if (status_out) KP_HIP(ctx, hipMemcpyAsync(status_out, dS, (size_t)n_deg * nb * 4, hipMemcpyDeviceToHost, s));
  return kp_sync_timer0(ctx);
}

// K (degree j, monomial basis) of one nested evaluation, for parity checks: call right after kp_sweep_eval_nested
extern "C" int kp_sweep_nested_get_K(kp_ctx* ctx, int nb, int Wmax, int n_deg, int deg_index, int W, double* K_out) {
  if (!ctx || !K_out || deg_index < 0 || deg_index >= n_deg || !ctx->ws[6]) return ctx ? ctx->fail(KP_ERR_ARG, "kp_sweep_nested_get_K: bad argument") : KP_ERR_ARG;
  const double* dK = (const double*)((char*)ctx->ws[6] + SweepWs(nb, Wmax, n_deg, 0).K) + (size_t)deg_index * nb * 256;
  std::vector<double> tmp((size_t)nb * 256);
  KP_HIP(ctx, hipMemcpy(tmp.data(), dK, tmp.size() * 8, hipMemcpyDeviceToHost));
  for (int q = 0; q < nb; ++q)
    for (int e = 0; e < W * W; ++e) K_out[(size_t)q * W * W + e] = tmp[(size_t)q * 256 + e];
  return KP_OK;
}
