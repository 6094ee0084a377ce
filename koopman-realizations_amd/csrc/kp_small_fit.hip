// Batched small fits: many independent systems with the SAME dictionary and W <= 16, one workgroup per system.
// This is the shape of evaluate_rand_models.m (one Ksysid fit per random system, model type and degree;
// 1-D state, W <= 16): the per-system work (lift of ~1e4 snapshot pairs, Px'Px, Px'Py, the least-squares
// solve) is far too small for a launch sequence of its own, so one launch does all systems.
//   lift            generic column evaluation (any dictionary without dimension reduction), 64 snapshots per tile in LDS
//   Px'Px, Px'Py    register-blocked: a lane owns one 4 x 4 block of G and of C for 4 of the 64 snapshots of a tile
//                   (16 blocks x 16 snapshot groups = 256 threads): three 4-wide LDS reads per 32 FMAs.  (One output
//                   element per thread needed 3 LDS reads per 2 FMAs and was LDS-bound: 0.78 ms per 1024 systems.)
//                   The 16 groups are summed in a fixed order at the end (deterministic).
//   G K = C         sb_spd_solve16: Cholesky of the 16 x 16 block in registers (one wave, pivots by v_readlane, as
//                   kp_chol_kernel's diagonal block), then forward / backward substitution, one thread per right-hand side
// Replaces, for each system: Ksysid.get_Koopman (Ksysid.m:987-1092) with lasso = Inf.
#include "kp_small_tile.h"
#include <algorithm>

// recipes != nullptr (monomial dictionaries): column c is the product of <= nfmax entries of a per-snapshot power table
// x_v^e (recipe byte = v * D + e - 1, 0xff = unused; the table kp_basis_create builds for the fused Gram kernels), so a
// lift entry costs <= nfmax LDS reads and multiplies instead of the generic evaluation (exponent rows from global
// memory, up to 13 multiplies per column for the degree-13 dictionaries of the sweep).
//
// refine > 0: iterative refinement of the normal-equations solution with the residual formed FROM THE DATA,
//   R = Px' (Py - Px K),  G dK = R,  K += dK,
// in further sweeps over the snapshots (the tile E = Py - Px K replaces Py in the same accumulation).  The reference
// solves Px \ Py by QR (Ksysid.m:1069); the degree-13 dictionaries of the sweep have cond(Px) ~ 1e5, where the plain
// normal equations are only good to cond^2 eps ~ 1e-6 - one refinement step brings K to the accuracy of the QR solution.
__global__ __launch_bounds__(256) void kp_small_fit_kernel(BasisDev b, const double* __restrict__ alpha, const double* __restrict__ beta,
                                                           const double* __restrict__ u, int64_t Ns_total, int Ns, double* __restrict__ Kout,
                                                           double* __restrict__ Gout, double* __restrict__ Cout, int* __restrict__ status,
                                                           const uint32_t* __restrict__ recipes, int D, int nfmax, int refine, TrajView tv, int cheb) {
  extern __shared__ __align__(16) double sm[];
  // LDS: vx[nvars][TS] | vy[nvars][TS] | um[m][TS] | Px[TS][LD] | Py[TS][LD] | Gs[16][LD] | Cs[16][LD] | Ls[16][LD] | Dd[16] | Ks[16][LD] | Xs[16][LD] | pw
  const int nv = b.nvars, m = b.m, N = b.N, W = b.W;
  double* vx = sm;
  double* vy = vx + nv * SB_TS;
  double* um = vy + nv * SB_TS;
  double* Px = um + (m > 0 ? m : 1) * SB_TS;
  double* Py = Px + SB_TS * SB_LD;
  double* Gs = Py + SB_TS * SB_LD;
  double* Cs = Gs + 16 * SB_LD;
  double* Ls = Cs + 16 * SB_LD;
  double* Dd = Ls + 16 * SB_LD;
  double* Ks = Dd + 16;                             // current K, [row][col]
  double* Xs = Ks + 16 * SB_LD;                     // solution of the last solve
  double* pw = Xs + 16 * SB_LD;                     // [side][v * D + e - 1][snapshot]  (only with recipes)
  __shared__ int bad;
  __shared__ uint32_t recs[SB_W];
  if (recipes && threadIdx.x < N) recs[threadIdx.x] = recipes[threadIdx.x];
  const int tid = threadIdx.x;
  const int sys = blockIdx.x;
  const int64_t base = (int64_t)sys * Ns;           // first row of this system inside the merged arrays
  if (tid == 0) bad = 0;
  for (int e = tid; e < 2 * SB_TS * SB_LD; e += 256) Px[e] = 0.0;      // Px and Py (contiguous): unused columns stay zero
  const int gi = tid >> 4, gj = tid & 15;
  const int blk = tid & 15, grp = tid >> 4;          // 4 x 4 output block, snapshot group (4 consecutive snapshots of a tile)
  const int bi = (blk >> 2) * 4, bj = (blk & 3) * 4;
  Ks[gi * SB_LD + gj] = 0.0;
  for (int pass = 0; pass <= refine; ++pass) {
    double g[4][4], c[4][4];
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
      for (int y = 0; y < 4; ++y) g[x][y] = c[x][y] = 0.0;
    __syncthreads();
    for (int r0 = 0; r0 < Ns; r0 += SB_TS) {
      const int nl = min(SB_TS, Ns - r0);
      // raw variables of the tile: x side (alpha [, u]), y side (beta [, u]), inputs
      for (int e = tid; e < (2 * nv + m) * SB_TS; e += 256) {
        const int v = e / SB_TS, p = e % SB_TS;
        double x = 0.0;
        if (p < nl && tv.Y) {                          // pair straight from the (already scaled) trajectories
          const int pair = r0 + p, Tm1 = tv.T - 1;
          const int tr = (int)(((unsigned long long)pair * tv.div_magic) >> 40);
          const int row = tr * tv.T + (pair - tr * Tm1);
          int var = v < nv ? v : v < 2 * nv ? v - nv : b.nzeta + (v - 2 * nv);        // index into [y (n) ; u (m)]
          const int shift = (v >= nv && v < 2 * nv && var < b.nzeta) ? 1 : 0;         // beta = the next row of y
          if (var < b.nzeta) x = tv.Y[((size_t)sys * tv.n + var) * tv.rows + row + shift];
          else x = tv.U[((size_t)sys * tv.m + (var - b.nzeta)) * tv.rows + row];
        } else if (p < nl) {
          const int64_t row = base + r0 + p;
          if (v < nv) x = v < b.nzeta ? alpha[(int64_t)v * Ns_total + row] : u[(int64_t)(v - b.nzeta) * Ns_total + row];
          else if (v < 2 * nv) x = (v - nv) < b.nzeta ? beta[(int64_t)(v - nv) * Ns_total + row] : u[(int64_t)(v - nv - b.nzeta) * Ns_total + row];
          else x = u[(int64_t)(v - 2 * nv) * Ns_total + row];
        }
        sm[e] = x;                                     // vx | vy | um are contiguous in this order
      }
      __syncthreads();
      if (recipes) {                                   // power table of both sides
        for (int e = tid; e < 2 * nv * SB_TS; e += 256) {
          const int p = e % SB_TS, sv = e / SB_TS;     // sv = side * nv + v; vx | vy are contiguous
          const double x = sm[sv * SB_TS + p];
          double q = x, qm = 1.0;
          for (int k = 0; k < D; ++k) {
            pw[(sv * D + k) * SB_TS + p] = q;
            const double qn = cheb ? 2.0 * x * q - qm : q * x;      // cheb: T_(k+2) = 2 x T_(k+1) - T_k instead of x^(k+2)
            qm = q;
            q = qn;
          }
        }
        __syncthreads();
      }
      // rows of Px / Py (Ksysid.m:1034-1064): [psi, u] / psi (x) [1; u] / psi([zeta; u])
      for (int e = tid; e < 2 * N * SB_TS; e += 256) {
        const int p = e % SB_TS, sc = e / SB_TS, side = sc / N, col = sc - side * N;
        double val;
        if (recipes) {
          const uint32_t rc = recs[col];
          val = p < nl ? 1.0 : 0.0;
          for (int f = 0; f < nfmax; ++f) {
            const uint32_t id = (rc >> (8 * f)) & 255u;
            const double t = pw[((side * nv) * D + (id == 255u ? 0u : id)) * SB_TS + p];       // unconditional read, then select
            val *= id == 255u ? 1.0 : t;
          }
        } else {
          val = p < nl ? kp_eval_col(b, b.cols[col], (side ? vy : vx) + p, SB_TS) : 0.0;
        }
        double* P = (side ? Py : Px) + p * SB_LD;
        P[col] = val;
        if (b.model_type == KP_MODEL_BILINEAR)
          for (int i = 0; i < m; ++i) P[(i + 1) * N + col] = val * um[i * SB_TS + p];
      }
      if (b.model_type == KP_MODEL_LINEAR)
        for (int e = tid; e < 2 * m * SB_TS; e += 256) {
          const int p = e % SB_TS, si = e / SB_TS, side = si / m, i = si - side * m;
          ((side ? Py : Px) + p * SB_LD)[N + i] = um[i * SB_TS + p];       // zero past the tail (um is)
        }
      __syncthreads();
      if (pass > 0) {                                  // E = Py - Px K in place of Py: thread = (snapshot, 4 columns)
        const int p = tid >> 2, j4 = (tid & 3) * 4;
        double2 e0 = *reinterpret_cast<const double2*>(Py + p * SB_LD + j4), e1 = *reinterpret_cast<const double2*>(Py + p * SB_LD + j4 + 2);
        for (int i = 0; i < W; ++i) {
          const double xi = Px[p * SB_LD + i];
          const double2 k0 = *reinterpret_cast<const double2*>(Ks + i * SB_LD + j4), k1 = *reinterpret_cast<const double2*>(Ks + i * SB_LD + j4 + 2);
          e0.x -= xi * k0.x; e0.y -= xi * k0.y; e1.x -= xi * k1.x; e1.y -= xi * k1.y;
        }
        *reinterpret_cast<double2*>(Py + p * SB_LD + j4) = e0;
        *reinterpret_cast<double2*>(Py + p * SB_LD + j4 + 2) = e1;
        __syncthreads();
      }
#pragma unroll
      for (int s_ = 0; s_ < 4; ++s_) {
        const double* xr = Px + (grp * 4 + s_) * SB_LD;
        const double* yr = Py + (grp * 4 + s_) * SB_LD;
        const double2 xa = *reinterpret_cast<const double2*>(xr + bi), xb = *reinterpret_cast<const double2*>(xr + bi + 2);
        const double2 ja = *reinterpret_cast<const double2*>(xr + bj), jb = *reinterpret_cast<const double2*>(xr + bj + 2);
        const double2 ya = *reinterpret_cast<const double2*>(yr + bj), yb = *reinterpret_cast<const double2*>(yr + bj + 2);
        const double xi[4] = {xa.x, xa.y, xb.x, xb.y}, xj[4] = {ja.x, ja.y, jb.x, jb.y}, yj[4] = {ya.x, ya.y, yb.x, yb.y};
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
          for (int y = 0; y < 4; ++y) {
            if (pass == 0) g[x][y] += xi[x] * xj[y];
            c[x][y] += xi[x] * yj[y];
          }
      }
      __syncthreads();
    }
    // sum of the 16 snapshot groups in a fixed order (pass 0: G and C; later passes: the residual R in Cs)
    if (pass == 0) Gs[gi * SB_LD + gj] = 0.0;
    Cs[gi * SB_LD + gj] = 0.0;
    for (int t = 0; t < 16; ++t) {
      __syncthreads();
      if (grp == t) {
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
          for (int y = 0; y < 4; ++y) {
            if (pass == 0) Gs[(bi + x) * SB_LD + bj + y] += g[x][y];
            Cs[(bi + x) * SB_LD + bj + y] += c[x][y];
          }
      }
    }
    __syncthreads();
    if (pass == 0) {
      // G (identity on the padding so that the 16 x 16 factorisation is well defined) and C
      const double gv = Gs[gi * SB_LD + gj], cv = Cs[gi * SB_LD + gj];
      if (gi < W && gj < W) {
        if (Gout) Gout[(size_t)sys * W * W + (size_t)gj * W + gi] = gv;
        if (Cout) Cout[(size_t)sys * W * W + (size_t)gj * W + gi] = cv;
      } else {
        Gs[gi * SB_LD + gj] = gi == gj ? 1.0 : 0.0;
        Cs[gi * SB_LD + gj] = 0.0;
      }
      __syncthreads();
    }
    // G X = C (pass 0) or G dK = R: 16 x 16 Cholesky in registers + substitution
    sb_spd_solve16(Gs, Cs, Xs, Ls, Dd, &bad);
    Ks[gi * SB_LD + gj] += Xs[gi * SB_LD + gj];
    if (bad) break;                                  // (uniform: `bad` is shared and the solve ends with a barrier)
  }
  __syncthreads();
  if (gi < W && gj < W) Kout[(size_t)sys * W * W + (size_t)gj * W + gi] = bad ? __builtin_nan("") : Ks[gi * SB_LD + gj];
  if (tid == 0 && status) status[sys] = bad;
}

bool kp_small_fit_launch(kp_ctx* ctx, const kp_basis* basis, int nb, const double* alpha, const double* beta, const double* u, int64_t Ns_total,
                         int Ns, const TrajView& tv, double* dK, double* dG, double* dC, int* dS) {
  const BasisDev& b = basis->dev;
  size_t lds = ((size_t)(2 * b.nvars + (b.m > 0 ? b.m : 1)) * SB_TS + 2 * SB_TS * SB_LD + 5 * 16 * SB_LD + 16) * sizeof(double);
  // power-table lift for monomial dictionaries whose table fits (2 sides x nvars x depth x 64 snapshots)
  // refinement steps with the residual taken from the data (default 1; KP_BATCH_REFINE=0 gives the plain normal equations)
  static const int refine = [] { const char* e = getenv("KP_BATCH_REFINE"); return e ? std::max(0, std::min(4, atoi(e))) : 1; }();
  const size_t pw_bytes = (size_t)2 * b.nvars * basis->pow_depth * SB_TS * sizeof(double);
  const bool use_rec = basis->fast && basis->d_recipes && basis->pow_depth >= 1 && lds + pw_bytes <= 64 * 1024;
  if (use_rec) lds += pw_bytes;
  hipLaunchKernelGGL(kp_small_fit_kernel, dim3(nb), dim3(256), lds, ctx->stream, b, alpha, beta, u, Ns_total, Ns, dK, dG, dC, dS,
                     use_rec ? (const uint32_t*)basis->d_recipes : nullptr, basis->pow_depth, basis->max_factors > 0 ? basis->max_factors : 1,
                     refine, tv, 0);
  return use_rec;
}

extern "C" int kp_fit_batch(kp_ctx* ctx, const kp_basis* basis, const kp_snapshots* snaps, int nb, int64_t Ns_each, double* K_out,
                            double* G_out, double* C_out, int* status_out) {
  if (!ctx || !basis || !snaps || !K_out || nb < 1 || Ns_each < 1) return ctx ? ctx->fail(KP_ERR_ARG, "kp_fit_batch: bad argument") : KP_ERR_ARG;
  const BasisDev& b = basis->dev;
  if (snaps->nzeta != b.nzeta || snaps->m != b.m) return ctx->fail(KP_ERR_ARG, "kp_fit_batch: snapshot/basis dimension mismatch");
  if (snaps->Ns != (int64_t)nb * Ns_each) return ctx->fail(KP_ERR_ARG, "kp_fit_batch: snapshots must hold nb x Ns_each rows");
  if (b.W > SB_W || b.k_pcs != 0 || b.N != b.nfull) return ctx->fail(KP_ERR_ARG, "kp_fit_batch: needs W <= 16 and no dimension reduction");
  if (Ns_each > 0x7fffffff) return ctx->fail(KP_ERR_ARG, "kp_fit_batch: too many snapshots per system");
  KP_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->async_pending) {
    int rc0 = kp_synchronize(ctx);
    if (rc0) return rc0;
  }
  const int W = b.W;
  const size_t bW = (size_t)nb * W * W * 8;
  char* ws = (char*)ctx->workspace(6, 3 * bW + (size_t)nb * 4 + 64);
  if (!ws) return ctx->fail(KP_ERR_HIP, "kp_fit_batch: out of device memory");
  double* dK = (double*)ws;
  double* dG = (double*)(ws + bW);
  double* dC = (double*)(ws + 2 * bW);
  int* dS = (int*)(ws + 3 * bW);
  hipStream_t s = ctx->stream;
  KP_HIP(ctx, kp_snaps_acquire(snaps, s));
  KP_HIP(ctx, hipEventRecord(ctx->ev0, s));
  kp_small_fit_launch(ctx, basis, nb, snaps->alpha, snaps->beta, snaps->u, snaps->Ns, (int)Ns_each, TrajView{}, dK, dG, dC, dS);
  KP_HIP(ctx, hipGetLastError());
  KP_HIP(ctx, kp_snaps_release(snaps, s));
  KP_HIP(ctx, hipEventRecord(ctx->ev1, s));
  KP_HIP(ctx, hipMemcpyAsync(K_out, dK, bW, hipMemcpyDeviceToHost, s));
  if (G_out) KP_HIP(ctx, hipMemcpyAsync(G_out, dG, bW, hipMemcpyDeviceToHost, s));
  if (C_out) KP_HIP(ctx, hipMemcpyAsync(C_out, dC, bW, hipMemcpyDeviceToHost, s));
  if (status_out) KP_HIP(ctx, hipMemcpyAsync(status_out, dS, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
  return kp_sync_timer0(ctx);
}

// ---- batched M-projection of get_model (Ksysid.m:1206-1225) for the small linear models of the sweep ---------------
// Per model, with K1 = K(:, 1:N) (W x N), A0 = K1(1:N, :)', B0 = K1(N+1:W, :)':
//   L'L = K1' G K1,   L'R = K1' C(:, 1:N),   M' = (L'L) \ (L'R),   A = M A0,  B = M B0.
// Thread (i, j) of the 16 x 16 grid owns one element of every product; matrices live in LDS with row stride SB_LD.
__global__ __launch_bounds__(256) void kp_small_project_kernel(const double* __restrict__ K, const double* __restrict__ G,
                                                               const double* __restrict__ C, int N, int m, double* __restrict__ Aout,
                                                               double* __restrict__ Bout, double* __restrict__ Mout, int* __restrict__ status) {
  __shared__ double Ks[16 * SB_LD], Gs[16 * SB_LD], Cs[16 * SB_LD], Ts[16 * SB_LD], LL[16 * SB_LD], LR[16 * SB_LD], Ms[16 * SB_LD], Ls[16 * SB_LD], Dd[16];
  __shared__ int bad;
  const int tid = threadIdx.x, i = tid >> 4, j = tid & 15, sys = blockIdx.x, W = N + m;
  const size_t off = (size_t)sys * W * W;
  const bool in = i < W && j < W;
  Ks[i * SB_LD + j] = in ? K[off + (size_t)j * W + i] : 0.0;            // [row][col]
  Gs[i * SB_LD + j] = in ? G[off + (size_t)j * W + i] : 0.0;
  Cs[i * SB_LD + j] = in ? C[off + (size_t)j * W + i] : 0.0;
  if (tid == 0) bad = 0;
  __syncthreads();
  double t = 0.0;                                                        // T = G K1  (W x N)
  if (j < N)
    for (int w = 0; w < W; ++w) t += Gs[i * SB_LD + w] * Ks[w * SB_LD + j];
  Ts[i * SB_LD + j] = t;
  __syncthreads();
  double ll = 0.0, lr = 0.0;                                             // L'L = K1' T, L'R = K1' C(:, 1:N)  (N x N)
  if (i < N && j < N)
    for (int w = 0; w < W; ++w) {
      ll += Ks[w * SB_LD + i] * Ts[w * SB_LD + j];
      lr += Ks[w * SB_LD + i] * Cs[w * SB_LD + j];
    }
  LL[i * SB_LD + j] = (i < N && j < N) ? ll : (i == j ? 1.0 : 0.0);      // identity on the padding
  LR[i * SB_LD + j] = (i < N && j < N) ? lr : 0.0;
  __syncthreads();
  sb_spd_solve16(LL, LR, Ms, Ls, Dd, &bad);                               // Ms = M' (N x N)
  const double nanv = __builtin_nan("");
  double a = 0.0, b = 0.0;                                               // A = M A0: A[i][j] = sum_k M[i][k] K[j][k]; B[i][j] = sum_k M[i][k] K[N + j][k]
  if (i < N)
    for (int k = 0; k < N; ++k) {
      const double mik = Ms[k * SB_LD + i];                              // M[i][k] = M'[k][i]
      if (j < N) a += mik * Ks[j * SB_LD + k];
      if (j < m) b += mik * Ks[(N + j) * SB_LD + k];
    }
  if (i < N && j < N) {
    Aout[(size_t)sys * N * N + (size_t)j * N + i] = bad ? nanv : a;
    if (Mout) Mout[(size_t)sys * N * N + (size_t)j * N + i] = bad ? nanv : Ms[j * SB_LD + i];
  }
  if (i < N && j < m) Bout[(size_t)sys * N * m + (size_t)j * N + i] = bad ? nanv : b;
  if (tid == 0 && status) status[sys] = bad;
}

void kp_small_project_launch(kp_ctx* ctx, int nb, const double* dK, const double* dG, const double* dC, int N, int m, double* dA, double* dB,
                             double* dM, int* dS) {
  hipLaunchKernelGGL(kp_small_project_kernel, dim3(nb), dim3(256), 0, ctx->stream, dK, dG, dC, N, m, dA, dB, dM, dS);
}

extern "C" int kp_model_project_batch(kp_ctx* ctx, const double* K, const double* G, const double* C, int nb, int N, int m, double* A_out,
                                      double* B_out, double* M_out, int* status_out) {
  if (!ctx || !K || !G || !C || !A_out || !B_out || nb < 1 || N < 1 || m < 0 || N + m > SB_W)
    return ctx ? ctx->fail(KP_ERR_ARG, "kp_model_project_batch: bad argument (needs N + m <= 16)") : KP_ERR_ARG;
  KP_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->async_pending) {
    int rc0 = kp_synchronize(ctx);
    if (rc0) return rc0;
  }
  const int W = N + m;
  const size_t bW = (size_t)nb * W * W * 8, bA = (size_t)nb * N * N * 8, bB = (size_t)nb * N * (m > 0 ? m : 1) * 8;
  char* ws = (char*)ctx->workspace(6, 3 * bW + 2 * bA + bB + (size_t)nb * 4 + 64);
  if (!ws) return ctx->fail(KP_ERR_HIP, "kp_model_project_batch: out of device memory");
  double *dK = (double*)ws, *dG = (double*)(ws + bW), *dC = (double*)(ws + 2 * bW);
  double *dA = (double*)(ws + 3 * bW), *dM = (double*)(ws + 3 * bW + bA), *dB = (double*)(ws + 3 * bW + 2 * bA);
  int* dS = (int*)(ws + 3 * bW + 2 * bA + bB);
  hipStream_t s = ctx->stream;
  KP_HIP(ctx, hipMemcpyAsync(dK, K, bW, hipMemcpyHostToDevice, s));
  KP_HIP(ctx, hipMemcpyAsync(dG, G, bW, hipMemcpyHostToDevice, s));
  KP_HIP(ctx, hipMemcpyAsync(dC, C, bW, hipMemcpyHostToDevice, s));
  kp_small_project_launch(ctx, nb, dK, dG, dC, N, m, dA, dB, M_out ? dM : nullptr, dS);
  KP_HIP(ctx, hipGetLastError());
  KP_HIP(ctx, hipMemcpyAsync(A_out, dA, bA, hipMemcpyDeviceToHost, s));
  if (m > 0) KP_HIP(ctx, hipMemcpyAsync(B_out, dB, (size_t)nb * N * m * 8, hipMemcpyDeviceToHost, s));
  if (M_out) KP_HIP(ctx, hipMemcpyAsync(M_out, dM, bA, hipMemcpyDeviceToHost, s));
  if (status_out) KP_HIP(ctx, hipMemcpyAsync(status_out, dS, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
  KP_HIP(ctx, hipStreamSynchronize(s));
  return KP_OK;
}
