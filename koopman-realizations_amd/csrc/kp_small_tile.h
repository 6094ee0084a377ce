// What the files of the W <= 16 kernels share (kp_small_fit.hip, kp_traj.hip, kp_sweep_gram.hip, kp_sweep.hip): the 16 x 16 LDS
// tile convention with its solve and row helpers, and the device-resident trajectory object with the view kernels take.
#pragma once
#include "kp_internal.h"

#define SB_TS 64      // snapshots per tile
#define SB_W 16       // maximum Px width
#define SB_LD 18      // row stride of the tiles (even: 16-byte aligned rows for the 4-wide operand reads)

__device__ __forceinline__ double sb_bcast(double v, int lane) {
  int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// Solves G X = C for the 16 x 16 SPD matrix Gs (identity on the padding) and 16 right-hand sides Cs, all in LDS with
// row stride SB_LD; X -> Xs.  Cholesky in registers: lane r (< 16) of wave 0 owns row r, pivots by v_readlane (as
// kp_chol_kernel's diagonal block), then forward / backward substitution, one thread per right-hand side.
// All 256 threads call; *bad is set when a pivot is not positive.
__device__ __forceinline__ void sb_spd_solve16(const double* Gs, const double* Cs, double* Xs, double* Ls, double* Dd, int* bad) {
  const int tid = threadIdx.x;
  if (tid < 64) {
    const int r = tid & 15;
    double row[16];
#pragma unroll
    for (int cc = 0; cc < 16; ++cc) row[cc] = Gs[r * SB_LD + cc];
#pragma unroll
    for (int cc = 0; cc < 16; ++cc) {
      double d = sb_bcast(row[cc], cc);
      if (!(d > 0.0)) {
        if (tid == 0) *bad = 1;
        d = 1.0;
      }
      double id = __builtin_amdgcn_rsq(d);
      id = id * (1.5 - 0.5 * d * id * id);
      id = id * (1.5 - 0.5 * d * id * id);
      if (tid == cc) Dd[cc] = id;
      const double l = row[cc] * id;
      row[cc] = l;
#pragma unroll
      for (int c2 = cc + 1; c2 < 16; ++c2) row[c2] -= l * sb_bcast(l, c2);
    }
    if (tid < 16) {
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) Ls[r * SB_LD + cc] = cc <= r ? row[cc] : 0.0;
    }
  }
  __syncthreads();
  // L Y = C, L' X = Y: one thread per right-hand side
  if (tid < 16) {
    const int j = tid;
    double y[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      double s = Cs[i * SB_LD + j];
#pragma unroll
      for (int q = 0; q < i; ++q) s -= Ls[i * SB_LD + q] * y[q];
      y[i] = s * Dd[i];
    }
#pragma unroll
    for (int i = 15; i >= 0; --i) {
      double s = y[i];
#pragma unroll
      for (int q = i + 1; q < 16; ++q) s -= Ls[q * SB_LD + i] * y[q];
      y[i] = s * Dd[i];
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) Xs[i * SB_LD + j] = y[i];
  }
  __syncthreads();
}

template <int CTRL>
__device__ __forceinline__ double sb_row_ror(double v) {       // lane l of a 16-lane row receives from lane (l - n) mod 16
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double sb_row_sum(double v) {        // sum over the 16 lanes of a row, in every lane
  v += sb_row_ror<0x128>(v);
  v += sb_row_ror<0x124>(v);
  v += sb_row_ror<0x122>(v);
  v += sb_row_ror<0x121>(v);
  return v;
}

// Device-resident trajectories of nb systems with one layout (kp_traj.hip): per system the merged training trials
// (rows = ntrials * T, column-major rows x n / rows x m) and the per-system scaling sc = [y offset (n) | y factor (n) |
// u offset (m) | u factor (m)] (get_scale, Ksysid.m:180-229), plus one validation trial of Tv rows.
struct kp_traj {
  kp_ctx* ctx = nullptr;
  int nb = 0, ntrials = 0, T = 0, n = 0, m = 0, Tv = 0;
  double *Y = nullptr, *U = nullptr, *Yv = nullptr, *Uv = nullptr, *sc = nullptr;
  size_t cap[5] = {0, 0, 0, 0, 0};      // real sizes of the five blocks (they may come from the context's pool)
  int have = 0;                         // bit w: block w has been put; 31: scaled (ready)
};

// What a kernel takes of it.  With Y != nullptr the fit kernels form the scaled snapshot pairs themselves (get_snapshotPairs,
// Ksysid.m:941-978, delays = 0, all pairs in time order): pair p of a system is row (p / (T-1)) T + p % (T-1) and its
// successor - no pair across a trial seam - and the last good pair is dropped (:960), so a system has ntrials (T - 1) - 1 pairs.
struct TrajView {
  const double* Y;      // SCALED in place at upload (kp_traj_apply_scale_kernel): the fit passes only index
  const double* U;
  const double* sc;
  int ntrials, T, rows, n, m;
  unsigned long long div_magic;   // ceil(2^40 / (T - 1)): pair / (T - 1) = (pair * magic) >> 40 for pair < 2^24
};

inline TrajView traj_view(const kp_traj* t) {
  const unsigned long long d = (unsigned long long)(t->T - 1);
  return TrajView{t->Y, t->U, t->sc, t->ntrials, t->T, t->ntrials * t->T, t->n, t->m, ((1ull << 40) + d - 1) / d};
}

// The tail of the entry points that time their first kernel with the context's event pair: wait for the stream, ev0 -> ev1
// into timers[0]
inline int kp_sync_timer0(kp_ctx* ctx) {
  hipStream_t s = ctx->stream;
  KP_HIP(ctx, hipStreamSynchronize(s));
  float ms = 0;
  (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
  ctx->timers[0] = ms;
  return KP_OK;
}
