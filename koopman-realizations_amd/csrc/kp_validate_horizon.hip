// Prediction-horizon validation: the h-step-ahead errors, h = 1 .. H, of every candidate model from EVERY start sample of every
// validation trial (kp_validate rolls each pair once, from row 0, over the whole trial).  The structure is the opposite of
// kp_validate's serial chain: all starts of a trial advance together, so one horizon step is a matrix product - the model's
// rows times a tile of start states - on the f64 matrix pipe.
//
// One workgroup (4 waves) = one model x one tile of S_T = 64, 32 or 16 consecutive starts of one trial, all H steps.  Column j
// of the tile is start s_j = (j0 + j) stride; a tile's unused columns (the last tile of a trial) repeat its last start and are
// left out of every sum.  Per step:
//   linear     Zn = [A | B] [Z; U_h]                             K = N + m
//   bilinear   Zn = [A | B_1 .. B_m] [Z; u_h1 o Z; ..; u_hm o Z]  K = N (1 + m); the weighted copies are formed in LDS by the
//              pass that moves Zn into the operand tile (the operand layout wants the contraction index contiguous per column)
//   nonlinear  Full = dictionary of [zeta; u_h] per column (kp_eval_col), Psi = [v; pcs' Full; 1] (only with dim_red: the
//              first product), Zn = Kf Psi (the second)
// All products go through hz_tile_product: v_mfma_f64_4x4x4_4b as kp_tn_gemm.h uses it - lane (lc = lane & 3, blk = (lane >> 2)
// & 3, lk = lane >> 4) holds A[row lc][k lk] (the same in all four blocks), B[k lk][column 4 blk + lc] and D[row lk][column
// 4 blk + lc] - one instruction is a 4-row x 16-column x 4-deep product.  Wave w owns the row groups w, w + 4, ..; a lane keeps
// S_T / 16 accumulators.  The B operand is a tile in LDS, [column][k], row stride = 2 mod 4 (the bank rule of TNG_RS), zero in
// k = K .. Kp - 1; the A operand is the model: staged in LDS as Rp x Kp with zero padding when it fits beside the tiles, else
// read from memory (L2) with clamped addresses and the padding selected to zero.  pcs is always read from memory.
//
// LDS (doubles): yfactor (n, even) | V [S_T][VS] start states / [zeta; u] | Full [S_T][FS] (dim_red only) | X [S_T][XS] the
// operand tile | Zn [S_T][ZS] the product | Uc [HC][m][S_T] | Yc [HC][n][S_T] | Ec, Euc [HC][S_T] | Bad [HC] | staged model.
// Inputs and real outputs are staged HC = KP_HORIZON_CHUNK steps at a time per (step, column): what is staged does not depend
// on the stride.  Behind step h the thread of column j replaces the real outputs in Yc by d = yhat - y and forms the two
// Euclidean norms (outputs in ascending order); at the end of a chunk thread (step, figure) adds its figure over the columns in
// ascending order and writes the tile's partial: H x (2 n + 3) per tile - sum |d| (n), sum d^2 (n), the two norm sums, and a
// not-finite flag.  kp_validate_horizon_finish_kernel adds a pair's tiles in ascending order.  No atomics anywhere; the tile
// width depends on the shape alone: a (model, trial) pair has the same bits alone or in any batch.
#include <algorithm>
#include <cmath>
#include <vector>

#include "kp_internal.h"
#include "koopman_hip_horizon.h"
#include "kp_validate_args.h"

#define HZ_HC KP_HORIZON_CHUNK
#define HZ_LDS (160 * 1024)
#define HZ_NT 256

struct HzDims {
  int mt, N, m, n, nz, ntr, H, stride;
  int stage;           // the model rows are in LDS
  int K, R;            // contraction length of the step product; rows that feed forward (N, or nzeta for a nonlinear model)
  int VS, FS, XS, ZS;  // row strides of the tiles
  int ntiles;          // tiles of all trials
  int64_t rows;        // all trials' rows
};

static inline int hz_pad4(int x) { return (x + 3) & ~3; }

// the A operand of a tile product: element (i, k) at p0[i si + k sk], or from k = ksplit on at p1[i si + (k - ksplit) sk]
struct HzOp {
  const double *p0, *p1;
  int ksplit, si, sk, M, K;
  int padded;          // p0 holds hz_pad4(M) x hz_pad4(K) with zeros beyond M x K: no clamps
};

__device__ __forceinline__ double hz_a(const HzOp& a, int i, int k) {
  if (a.padded) return a.p0[i * a.si + k * a.sk];
  const int ic = min(i, a.M - 1), kc = min(k, a.K - 1);
  const double* p = kc < a.ksplit ? a.p0 + (size_t)kc * a.sk : a.p1 + (size_t)(kc - a.ksplit) * a.sk;
  const double v = p[(size_t)ic * a.si];
  return (i < a.M && k < a.K) ? v : 0.0;
}

// Out[column][row] (row stride os) = A (M x K) X, X[column][k] (row stride xs) a tile of 16 RB columns, zero in k >= K
template <int RB>
__device__ __forceinline__ void hz_tile_product(const HzOp& a, const double* X, int xs, double* Out, int os, int tid) {
  const int lane = tid & 63, wave = tid >> 6, lc = lane & 3, blk = (lane >> 2) & 3, lk = lane >> 4;
  const int nrg = (a.M + 3) >> 2, Kp = (a.K + 3) & ~3;
  const double* xb = X + (4 * blk + lc) * xs + lk;
  for (int rg = wave; rg < nrg; rg += HZ_NT / 64) {
    double acc[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) acc[rb] = 0.0;
    const int i = 4 * rg + lc;
    double av = hz_a(a, i, lk);
    for (int k0 = 0; k0 < Kp; k0 += 4) {
      const double an = k0 + 4 < Kp ? hz_a(a, i, k0 + 4 + lk) : 0.0;
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) acc[rb] = __builtin_amdgcn_mfma_f64_4x4x4f64(av, xb[16 * rb * xs + k0], acc[rb], 0, 0, 0);
      av = an;
    }
    const int r = 4 * rg + lk;
    if (r < a.M) {
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) Out[(16 * rb + 4 * blk + lc) * os + r] = acc[rb];
    }
  }
}

// Dst[column] = econ_full(V[column]) (Ksysid.m:1615-1618): the dictionary itself, or [v; pcs' full; 1] with dim_red.  Ends
// behind a barrier.
template <int RB>
__device__ __forceinline__ void hz_lift(const BasisDev& b, const double* V, int VS, double* Full, int FS, double* Dst, int DS, int tid) {
  constexpr int S = 16 * RB;
  if (b.k_pcs == 0) {
    for (int e = tid; e < S * b.nfull; e += HZ_NT) {
      const int c = e / S, j = e - c * S;
      Dst[j * DS + c] = kp_eval_col(b, b.cols[c], V + j * VS, 1);
    }
    __syncthreads();
    return;
  }
  for (int e = tid; e < S * b.nfull; e += HZ_NT) {
    const int c = e / S, j = e - c * S;
    Full[j * FS + c] = kp_eval_col(b, b.cols[c], V + j * VS, 1);
  }
  for (int e = tid; e < S * (b.nvars + 1); e += HZ_NT) {
    const int c = e / S, j = e - c * S;
    if (c < b.nvars) Dst[j * DS + c] = V[j * VS + c];
    else Dst[j * DS + b.nvars + b.k_pcs] = 1.0;
  }
  __syncthreads();
  const HzOp pc{b.pcs, nullptr, b.nfull, b.nfull, 1, b.k_pcs, b.nfull, 0};     // pcs' (k_pcs x nfull): element (i, k) = pcs[k + i nfull]
  hz_tile_product<RB>(pc, Full, FS, Dst + b.nvars, DS, tid);
  __syncthreads();
}

template <int RB>
__global__ __launch_bounds__(HZ_NT) void kp_validate_horizon_kernel(BasisDev b, HzDims d, const double* __restrict__ A, const double* __restrict__ B,
                                                                   const int64_t* __restrict__ off, const int* __restrict__ tile_tr,
                                                                   const int* __restrict__ tile_j0, const double* __restrict__ Zeta,
                                                                   const double* __restrict__ U, const double* __restrict__ yfac,
                                                                   double* __restrict__ part) {
  constexpr int S = 16 * RB;
  extern __shared__ __align__(16) double sm[];
  const int tid = threadIdx.x;
  const int mod = blockIdx.x / d.ntiles, tile = blockIdx.x - mod * d.ntiles;
  const int tr = tile_tr[tile], j0 = tile_j0[tile];
  const int N = d.N, m = d.m, n = d.n, nz = d.nz, H = d.H, K = d.K, R = d.R;
  const int VS = d.VS, FS = d.FS, XS = d.XS, ZS = d.ZS;
  const bool nl = d.mt == KP_MODEL_NONLINEAR, bil = d.mt == KP_MODEL_BILINEAR;
  const int64_t r0 = off[tr];
  const int T = (int)(off[tr + 1] - r0);
  const int nst = (T - 1 - H) / d.stride + 1;                    // starts of the trial (a tile exists only where T - 1 >= H)
  const int jv = min(S, nst - j0);                               // columns of this tile that are starts
  double* fs = sm;
  double* V = fs + ((n + 1) & ~1);
  double* Full = V + S * VS;
  double* X = Full + S * FS;
  double* Zn = X + S * XS;
  double* Uc = Zn + S * ZS;
  double* Yc = Uc + HZ_HC * m * S;
  double* Ec = Yc + HZ_HC * n * S;
  double* Euc = Ec + HZ_HC * S;
  double* Bad = Euc + HZ_HC * S;
  double* Msh = Bad + HZ_HC;
  // first row of column j in the trial-stacked arrays; the unused columns repeat the tile's last start
  auto row_of = [&](int j) { return r0 + (int64_t)(j0 + min(j, jv - 1)) * d.stride; };

  // the model: R x K, rows 1:N of [A | B] or Kf
  const int ksplit = nl ? K : N, lda = nl ? nz : N;
  const double* Am = A + (size_t)mod * (nl ? (size_t)nz * N : (size_t)N * N);
  const double* Bm = nl ? nullptr : B + (size_t)mod * N * (size_t)(K - N);
  HzOp mop{Am, Bm, ksplit, 1, lda, R, K, 0};
  if (d.stage) {
    const int Rp = (R + 3) & ~3, Kp = (K + 3) & ~3;
    for (int e = tid; e < Rp * Kp; e += HZ_NT) {
      const int k = e / Rp, i = e - k * Rp;
      Msh[e] = hz_a(mop, i, k);
    }
    mop = HzOp{Msh, nullptr, Kp, 1, Rp, R, K, 1};
  }
  for (int c = tid; c < n; c += HZ_NT) fs[c] = yfac[c];
  for (int e = tid; e < S * XS; e += HZ_NT) X[e] = 0.0;
  for (int e = tid; e < S * FS; e += HZ_NT) Full[e] = 0.0;
  for (int e = tid; e < S * b.nvars; e += HZ_NT) {
    const int c = e / S, j = e - c * S;
    V[j * VS + c] = c < nz ? Zeta[(size_t)c * d.rows + row_of(j)] : U[(size_t)(c - nz) * d.rows + row_of(j)];
  }
  __syncthreads();
  if (!nl) {                                                       // z_0 = econ_full(zeta_s), then the input part of the operand
    hz_lift<RB>(b, V, VS, Full, FS, X, XS, tid);
    for (int e = tid; e < S * (K - N); e += HZ_NT) {
      const int c = e / S, j = e - c * S;
      const int i = bil ? c / N : c;
      const double u = U[(size_t)i * d.rows + row_of(j)];
      X[j * XS + N + c] = bil ? u * X[j * XS + (c - i * N)] : u;
    }
    __syncthreads();
  }
  double* pt = part + ((size_t)mod * d.ntiles + tile) * (size_t)H * (2 * n + 3);
  for (int h = 0; h < H; ++h) {
    const int hh = h % HZ_HC;
    if (hh == 0) {                                                 // rows s + h + 1 .. of the chunk: read behind the product's barrier
      const int qn = min(HZ_HC, H - h);
      for (int e = tid; e < qn * m * S; e += HZ_NT) {
        const int qi = e / S, j = e - qi * S, q = qi / m, i = qi - q * m;
        Uc[e] = U[(size_t)i * d.rows + row_of(j) + h + 1 + q];
      }
      for (int e = tid; e < qn * n * S; e += HZ_NT) {
        const int qc = e / S, j = e - qc * S, q = qc / n, c = qc - q * n;
        Yc[e] = Zeta[(size_t)c * d.rows + row_of(j) + h + 1 + q];
      }
      if (tid < HZ_HC) Bad[tid] = 0.0;
    }
    if (nl) hz_lift<RB>(b, V, VS, Full, FS, X, XS, tid);
    hz_tile_product<RB>(mop, X, XS, Zn, ZS, tid);
    __syncthreads();
    if (tid < jv) {                                                // the errors of step h + 1 of column tid
      double e2 = 0.0, eu2 = 0.0;
      bool bad = false;
      for (int c = 0; c < n; ++c) {
        const double ys = Zn[tid * ZS + c];
        const double dd = ys - Yc[(hh * n + c) * S + tid];
        const double du = dd * fs[c];
        Yc[(hh * n + c) * S + tid] = dd;
        e2 += dd * dd;
        eu2 += du * du;
        bad = bad || !isfinite(ys);
      }
      Ec[hh * S + tid] = sqrt(e2);
      Euc[hh * S + tid] = sqrt(eu2);
      if (bad) Bad[hh] = 1.0;
    }
    if (h + 1 < H) {                                               // the operand of the next step
      if (nl) {
        for (int e = tid; e < S * b.nvars; e += HZ_NT) {
          const int c = e / S, j = e - c * S;
          V[j * VS + c] = c < nz ? Zn[j * ZS + c] : Uc[(hh * m + (c - nz)) * S + j];
        }
      } else {
        for (int e = tid; e < S * K; e += HZ_NT) {
          const int c = e / S, j = e - c * S;
          double v;
          if (c < N) v = Zn[j * ZS + c];
          else if (bil) {
            const int i = (c - N) / N;
            v = Uc[(hh * m + i) * S + j] * Zn[j * ZS + (c - N - i * N)];
          } else v = Uc[(hh * m + (c - N)) * S + j];
          X[j * XS + c] = v;
        }
      }
    }
    __syncthreads();
    if (hh == HZ_HC - 1 || h == H - 1) {                           // the chunk's sums over the columns, ascending
      const int nf = 2 * n + 3;
      for (int e = tid; e < (hh + 1) * (n + 3); e += HZ_NT) {
        const int q = e / (n + 3), c = e - q * (n + 3);
        double* po = pt + (size_t)(h - hh + q) * nf;
        if (c < n) {
          double sa = 0.0, sq = 0.0;
          for (int j = 0; j < jv; ++j) {
            const double dd = Yc[(q * n + c) * S + j];
            sa += fabs(dd);
            sq += dd * dd;
          }
          po[c] = sa;
          po[n + c] = sq;
        } else if (c < n + 2) {
          const double* E = (c == n ? Ec : Euc) + q * S;
          double s = 0.0;
          for (int j = 0; j < jv; ++j) s += E[j];
          po[2 * n + (c - n)] = s;
        } else {
          po[2 * n + 2] = Bad[q];
        }
      }
      if (h + 1 < H) __syncthreads();                              // before the next chunk is staged over this one
    }
  }
}

// err (nmod x ntr x H x (2 n + 2)) and status (nmod x ntr) from the tiles' partials: one workgroup per pair, the tiles of the pair
// added in ascending order
__global__ __launch_bounds__(256) void kp_validate_horizon_finish_kernel(int ntr, int n, int H, int stride, int ntiles,
                                                                          const int64_t* __restrict__ off, const int* __restrict__ toff,
                                                                          const double* __restrict__ part, double* __restrict__ err,
                                                                          int* __restrict__ status) {
  __shared__ int flag;
  const int mod = blockIdx.x / ntr, tr = blockIdx.x - mod * ntr;
  const int T = (int)(off[tr + 1] - off[tr]);
  const int nst = T - 1 < H ? 0 : (T - 1 - H) / stride + 1;
  const int t0 = toff[tr], t1 = toff[tr + 1];
  const int nf = 2 * n + 3, no = 2 * n + 2;
  if (threadIdx.x == 0) flag = 0;
  __syncthreads();
  double* eo = err + (size_t)blockIdx.x * H * no;
  for (int e = threadIdx.x; e < H * no; e += 256) {
    const int h = e / no, k = e - h * no;
    double v = NAN;
    if (nst > 0) {
      double s = 0.0;
      bool bad = false;
      for (int t = t0; t < t1; ++t) {
        const double* p = part + (((size_t)mod * ntiles + t) * H + h) * nf;
        s += p[k];
        if (k == 0) bad = bad || p[nf - 1] != 0.0;
      }
      if (bad) flag = 1;
      const double q = s / (double)nst;
      v = (k >= n && k < 2 * n) ? sqrt(q) : q;
    }
    eo[e] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) status[blockIdx.x] = flag;
}

// LDS of one workgroup with tiles of S columns, in doubles: the tiles and chunks, and the staged model
static void hz_lds_doubles(const BasisDev& b, int model_type, int N, int m, int n, int nzeta, int S, HzDims* d, size_t* fixed, size_t* model) {
  const bool nl = model_type == KP_MODEL_NONLINEAR, bil = model_type == KP_MODEL_BILINEAR;
  d->K = nl ? N : (bil ? N * (1 + m) : N + m);
  d->R = nl ? nzeta : N;
  d->VS = hz_pad4(b.nvars) + 2;
  d->FS = b.k_pcs > 0 ? hz_pad4(b.nfull) + 2 : 0;
  d->XS = hz_pad4(d->K) + 2;
  d->ZS = hz_pad4(d->R) + 2;
  *fixed = (size_t)((n + 1) & ~1) + (size_t)S * ((size_t)d->VS + d->FS + d->XS + d->ZS) + (size_t)HZ_HC * (m + n + 2) * S + HZ_HC;
  *model = (size_t)hz_pad4(d->R) * hz_pad4(d->K);
}

extern "C" int kp_validate_horizon(kp_ctx* ctx, const kp_basis* basis, int model_type, int N, int m, int n, int nzeta, int nmod,
                                   const double* A, const double* B, int ntr, const int64_t* trial_off, const double* Zeta,
                                   const double* U, const double* yfactor, int H, int stride, double* err_out, int64_t* nstart_out,
                                   int* status_out) {
  if (!ctx) return KP_ERR_ARG;
  const std::string fn = "kp_validate_horizon";
  const int rc_arg = val_check_args(ctx, fn, basis, model_type, N, m, n, nzeta, 0, nmod, A, B, ntr, trial_off, Zeta, U, Zeta, yfactor, 0,
                                    err_out, status_out, nullptr);
  if (rc_arg) return rc_arg;
  const int rc_h = val_check_horizon_args(ctx, fn, n, nzeta, H, stride, nstart_out);
  if (rc_h) return rc_h;
  const bool nl = model_type == KP_MODEL_NONLINEAR;
  const BasisDev& b = basis->dev;
  const int64_t rows = trial_off[ntr];
  if ((size_t)N * (size_t)(m + 1) > (size_t)INT32_MAX / 512) return ctx->fail(KP_ERR_ARG, fn + ": model too wide");
  if (b.nvars != nzeta + (nl ? m : 0) || (b.k_pcs == 0 ? b.nfull != N : b.nvars + b.k_pcs + 1 != N))      // econ_full's layout
    return ctx->fail(KP_ERR_ARG, fn + ": the dictionary's columns do not add up to N");

  // the tile width: the widest of 64, 32, 16 whose tiles fit the LDS; from the shape alone
  HzDims d{};
  size_t fixed = 0, model = 0;
  int S = 0;
  for (int s : {64, 32, 16}) {
    hz_lds_doubles(b, model_type, N, m, n, nzeta, s, &d, &fixed, &model);
    if (fixed * 8 <= HZ_LDS) { S = s; break; }
  }
  if (!S)
    return ctx->fail(KP_ERR_ARG, fn + ": a tile of 16 starts needs " + std::to_string(fixed * 8) + " bytes of LDS, the limit is " +
                                     std::to_string(HZ_LDS));
  const int stage = (fixed + model) * 8 <= HZ_LDS;
  const size_t lds = (fixed + (stage ? model : 0)) * 8;

  // starts and tiles of every trial
  std::vector<int> tile_tr, tile_j0, toff(ntr + 1, 0);
  for (int q = 0; q < ntr; ++q) {
    const int64_t Tq = trial_off[q + 1] - trial_off[q];
    const int64_t ns = Tq - 1 < H ? 0 : (Tq - 1 - H) / stride + 1;
    nstart_out[q] = ns;
    for (int64_t j0 = 0; j0 < ns; j0 += S) {
      tile_tr.push_back(q);
      tile_j0.push_back((int)j0);
    }
    if (tile_tr.size() > (size_t)INT32_MAX / 2) return ctx->fail(KP_ERR_ARG, fn + ": too many tiles");
    toff[q + 1] = (int)tile_tr.size();
  }
  const int ntiles = (int)tile_tr.size();
  if ((int64_t)nmod * ntiles > INT32_MAX) return ctx->fail(KP_ERR_ARG, fn + ": too many (model, tile) pairs");

  KP_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->async_pending) {
    int rc0 = kp_synchronize(ctx);
    if (rc0) return rc0;
  }
  const size_t mbc = (size_t)d.K - (nl ? (size_t)d.K : (size_t)N);                     // columns of B
  const size_t nA = (size_t)nmod * (nl ? (size_t)nzeta * N : (size_t)N * N), nB = (size_t)nmod * N * mbc;
  const size_t nZ = (size_t)rows * nzeta, nU = (size_t)rows * m, npairs = (size_t)nmod * ntr;
  const size_t nE = npairs * H * (2 * (size_t)n + 2), nP = (size_t)nmod * ntiles * H * (2 * (size_t)n + 3);
  const size_t nI = (size_t)(ntr + 1) + 2 * (size_t)ntiles + npairs + 4;               // ints: toff, tile_tr, tile_j0, status
  const size_t bytes = (nA + nB + nZ + nU + n + nE + nP) * 8 + (size_t)(ntr + 1) * 8 + nI * 4 + 64;
  double* ws = (double*)ctx->workspace(6, bytes);
  if (!ws) return ctx->fail(KP_ERR_HIP, fn + ": out of device memory (" + std::to_string(bytes) + " bytes)");
  double *dA = ws, *dB = dA + nA, *dZ = dB + nB, *dU = dZ + nZ, *df = dU + nU, *dE = df + n, *dP = dE + nE;
  int64_t* dOff = (int64_t*)(dP + nP);
  int* dToff = (int*)(dOff + ntr + 1);
  int *dTtr = dToff + ntr + 1, *dTj0 = dTtr + ntiles, *dSt = dTj0 + ntiles;
  hipStream_t s = ctx->stream;
  KP_HIP(ctx, hipMemcpyAsync(dA, A, nA * 8, hipMemcpyHostToDevice, s));
  if (nB) KP_HIP(ctx, hipMemcpyAsync(dB, B, nB * 8, hipMemcpyHostToDevice, s));
  KP_HIP(ctx, hipMemcpyAsync(dZ, Zeta, nZ * 8, hipMemcpyHostToDevice, s));
  if (nU) KP_HIP(ctx, hipMemcpyAsync(dU, U, nU * 8, hipMemcpyHostToDevice, s));
  KP_HIP(ctx, hipMemcpyAsync(df, yfactor, (size_t)n * 8, hipMemcpyHostToDevice, s));
  KP_HIP(ctx, hipMemcpyAsync(dOff, trial_off, (size_t)(ntr + 1) * 8, hipMemcpyHostToDevice, s));
  KP_HIP(ctx, hipMemcpyAsync(dToff, toff.data(), (size_t)(ntr + 1) * 4, hipMemcpyHostToDevice, s));
  if (ntiles) {
    KP_HIP(ctx, hipMemcpyAsync(dTtr, tile_tr.data(), (size_t)ntiles * 4, hipMemcpyHostToDevice, s));
    KP_HIP(ctx, hipMemcpyAsync(dTj0, tile_j0.data(), (size_t)ntiles * 4, hipMemcpyHostToDevice, s));
  }
  KP_HIP(ctx, hipEventRecord(ctx->ev0, s));
  d.mt = model_type; d.N = N; d.m = m; d.n = n; d.nz = nzeta; d.ntr = ntr; d.H = H; d.stride = stride;
  d.stage = stage; d.ntiles = ntiles; d.rows = rows;
  if (ntiles) {
    static KpLdsCache lds_c[3];
    const unsigned grid = (unsigned)((size_t)nmod * ntiles);
    if (S == 64) {
      KP_HIP(ctx, kp_ensure_lds(lds_c[0], (const void*)kp_validate_horizon_kernel<4>, HZ_LDS));
      hipLaunchKernelGGL(kp_validate_horizon_kernel<4>, dim3(grid), dim3(HZ_NT), lds, s, b, d, dA, dB, dOff, dTtr, dTj0, dZ, dU, df, dP);
    } else if (S == 32) {
      KP_HIP(ctx, kp_ensure_lds(lds_c[1], (const void*)kp_validate_horizon_kernel<2>, HZ_LDS));
      hipLaunchKernelGGL(kp_validate_horizon_kernel<2>, dim3(grid), dim3(HZ_NT), lds, s, b, d, dA, dB, dOff, dTtr, dTj0, dZ, dU, df, dP);
    } else {
      KP_HIP(ctx, kp_ensure_lds(lds_c[2], (const void*)kp_validate_horizon_kernel<1>, HZ_LDS));
      hipLaunchKernelGGL(kp_validate_horizon_kernel<1>, dim3(grid), dim3(HZ_NT), lds, s, b, d, dA, dB, dOff, dTtr, dTj0, dZ, dU, df, dP);
    }
    KP_HIP(ctx, hipGetLastError());
  }
  hipLaunchKernelGGL(kp_validate_horizon_finish_kernel, dim3((unsigned)npairs), dim3(256), 0, s, ntr, n, H, stride, ntiles, dOff, dToff, dP,
                     dE, dSt);
  KP_HIP(ctx, hipGetLastError());
  KP_HIP(ctx, hipEventRecord(ctx->ev1, s));
  KP_HIP(ctx, hipMemcpyAsync(err_out, dE, nE * 8, hipMemcpyDeviceToHost, s));
  KP_HIP(ctx, hipMemcpyAsync(status_out, dSt, npairs * 4, hipMemcpyDeviceToHost, s));
  KP_HIP(ctx, hipStreamSynchronize(s));
  float ms = 0;
  (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
  ctx->timers[24] = ms;
  ctx->timers[25] = 1000.0 * stage + S;
  return KP_OK;
}
