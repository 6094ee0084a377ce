// Batched real matrix logarithm (koopman_hip_ct.h): logm(K' + 1e-12 I) of the continuous-time models (Ksysid.m:1186-1187,
// 1245-1246, 1307-1310).  Inverse scaling and squaring without a Schur form:
//   * square roots A <- A^(1/2) until ||A - I||_1 <= 0.25, each by the determinant-scaled product-form Denman-Beavers
//     iteration  M_0 = Y_0 = A,  mu = |det M|^(-1/(2n)),  M+ = (I + (mu^2 M + mu^-2 M^-1) / 2) / 2,  Y+ = mu Y (I + mu^-2 M^-1) / 2;
//   * log(I + X) = sum_j w_j (I + x_j X)^-1 X over the 7 Gauss-Legendre nodes of [0, 1] (the [7/7] Pade approximant, accurate to
//     double precision for ||X||_1 <= 0.264), the 7 solves of every matrix as one batch;
//   * L = scale 2^s log(I + X).
// Every inverse / solve is a Gauss-Jordan elimination with partial pivoting over the augmented [M | R], one launch per pivot
// column for the whole batch (ping-pong buffers, so no workgroup reads what another writes in the same launch); the determinant
// comes from the pivots.  Products run on the f64 matrix pipe (kp_tn_gemm: every iterate is a function of A, so Y is carried
// transposed and Y+ = (W' Y')' with W = mu (I + mu^-2 M^-1) / 2).  Norms, convergence and failure flags stay on the device; the
// host reads one count per square root and per Denman-Beavers step after the third.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "koopman_hip_ct.h"
#include "kp_internal.h"
#include "kp_tn_gemm.h"

namespace {

constexpr int LG_NT = 256;
constexpr int LG_EPT = 4;            // output elements per thread of a Gauss-Jordan step
constexpr double LG_THETA = 0.25;    // ||A - I||_1 at which the quadrature takes over
constexpr int LG_MAX_SQRT = 64;
constexpr int LG_DB_CAP = 50;

// per-matrix state (device)
struct LgState {
  int status, nsqrt, sq, active, it, neg;
  double dprev;
};

__device__ __forceinline__ void lg_block_max(double& v, int& idx, double* sv, int* si) {
  // max |.| with the lowest index on ties (deterministic); v < 0 marks "none"
  const int t = threadIdx.x;
  sv[t] = v; si[t] = idx;
  __syncthreads();
  for (int s = LG_NT / 2; s > 0; s >>= 1) {
    if (t < s) {
      const double a = sv[t], b = sv[t + s];
      const int ia = si[t], ib = si[t + s];
      if (b > a || (b == a && ib < ia)) { sv[t] = b; si[t] = ib; }
    }
    __syncthreads();
  }
  v = sv[0]; idx = si[0];
}

__device__ __forceinline__ double lg_block_sum_max(double v, double* sv) {
  // max over the workgroup (NaN wins)
  const int t = threadIdx.x;
  sv[t] = v;
  __syncthreads();
  for (int s = LG_NT / 2; s > 0; s >>= 1) {
    if (t < s) {
      const double a = sv[t], b = sv[t + s];
      sv[t] = (b > a || b != b) ? b : a;
    }
    __syncthreads();
  }
  const double r = sv[0];
  __syncthreads();
  return r;
}

// ||A - I||_1 of one n x n column-major matrix, one workgroup
__device__ double lg_norm1_minus_I(const double* A, int n, double* sv) {
  double best = 0.0;
  for (int c = threadIdx.x; c < n; c += LG_NT) {
    double s = 0.0;
    const double* col = A + (size_t)c * n;
    for (int r = 0; r < n; ++r) s += fabs(col[r] - (r == c ? 1.0 : 0.0));
    best = (s > best || s != s) ? s : best;
  }
  return lg_block_sum_max(best, sv);
}

// one Gauss-Jordan step (pivot column k) of the augmented n x ncol systems sys = blockIdx.y: reads X, writes Y (columns k+1..)
__global__ __launch_bounds__(LG_NT) void kp_gj_step_kernel(const double* __restrict__ Xb, double* __restrict__ Yb, int64_t stride, int n,
                                                           int ncol, int k, const int* __restrict__ act, int* __restrict__ bad,
                                                           double* __restrict__ logdet, int* __restrict__ neg) {
  const int sys = blockIdx.y;
  if (!act[sys]) return;
  __shared__ double sv[LG_NT];
  __shared__ int si[LG_NT];
  const double* X = Xb + (size_t)sys * stride;
  double* Y = Yb + (size_t)sys * stride;
  double best = -1.0;
  int bi = n;
  for (int i = k + (int)threadIdx.x; i < n; i += LG_NT) {
    const double a = fabs(X[i + (size_t)k * n]);
    if (a > best) { best = a; bi = i; }     // a NaN entry is never chosen
  }
  lg_block_max(best, bi, sv, si);
  const int p = bi;
  if (p >= n || !(best > 0.0) || !(best < INFINITY)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) bad[sys] = 1;
    return;
  }
  const double piv = X[p + (size_t)k * n];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    logdet[sys] += log(fabs(piv));
    neg[sys] ^= (p != k) ^ (piv < 0.0);
  }
  const int64_t tot = (int64_t)n * (ncol - k - 1);
  const int64_t e0 = (int64_t)blockIdx.x * LG_NT * LG_EPT + threadIdx.x;
  for (int q = 0; q < LG_EPT; ++q) {
    const int64_t e = e0 + (int64_t)q * LG_NT;
    if (e >= tot) break;
    const int i = (int)(e % n);
    const int j = k + 1 + (int)(e / n);
    const double f = X[p + (size_t)j * n] / piv;
    if (i == k) {
      Y[k + (size_t)j * n] = f;
    } else {
      const int src = (i == p) ? k : i;
      Y[i + (size_t)j * n] = X[src + (size_t)j * n] - X[src + (size_t)k * n] * f;
    }
  }
}

// ---- phase kernels (one workgroup per matrix unless noted) ----
__global__ __launch_bounds__(LG_NT) void kp_logm_start_kernel(double* __restrict__ A, int n, double shift, LgState* __restrict__ st) {
  const int b = blockIdx.x;
  double* Ab = A + (size_t)b * n * n;
  for (int i = threadIdx.x; i < n; i += LG_NT) Ab[i + (size_t)i * n] += shift;
  if (threadIdx.x == 0) {
    st[b].status = KP_OK; st[b].nsqrt = 0; st[b].sq = 0; st[b].active = 0; st[b].it = 0; st[b].neg = 0; st[b].dprev = INFINITY;
  }
}

// decides per matrix whether another square root is needed; counts them into *cnt
__global__ __launch_bounds__(LG_NT) void kp_logm_check_kernel(const double* __restrict__ A, int n, LgState* __restrict__ st, int* __restrict__ cnt,
                                                              int* __restrict__ other) {
  __shared__ double sv[LG_NT];
  const int b = blockIdx.x;
  if (b == 0 && threadIdx.x == 0) *other = 0;      // the counter of the next counting launch
  if (st[b].status != KP_OK) {
    if (threadIdx.x == 0) st[b].sq = 0;
    return;
  }
  const double d = lg_norm1_minus_I(A + (size_t)b * n * n, n, sv);
  if (threadIdx.x == 0) {
    int sq = 0;
    if (!(d < INFINITY)) st[b].status = KP_ERR_NOT_CONVERGED;          // non-finite input
    else if (d > LG_THETA) {
      if (st[b].nsqrt >= LG_MAX_SQRT) st[b].status = KP_ERR_NOT_CONVERGED;
      else sq = 1;
    }
    st[b].sq = sq;
    st[b].active = sq; st[b].it = 0; st[b].dprev = INFINITY;
    if (sq) atomicAdd(cnt, 1);
  }
}

// M = A, Yt = A' for the matrices taking a square root (grid: tiles x matrices)
__global__ __launch_bounds__(LG_NT) void kp_logm_db_init_kernel(const double* __restrict__ A, double* __restrict__ M, double* __restrict__ Yt, int n,
                                                                const LgState* __restrict__ st, int* __restrict__ act) {
  const int b = blockIdx.y;
  if (blockIdx.x == 0 && threadIdx.x == 0) act[b] = st[b].sq;
  if (!st[b].sq) return;
  const int64_t nn = (int64_t)n * n, o = (int64_t)b * nn;
  for (int64_t e = (int64_t)blockIdx.x * LG_NT + threadIdx.x; e < nn; e += (int64_t)gridDim.x * LG_NT) {
    const int i = (int)(e % n), j = (int)(e / n);
    const double v = A[o + e];
    M[o + e] = v;
    Yt[o + j + (int64_t)i * n] = v;
  }
}

// augmented [M | I] of the active matrices; clears the pivot bookkeeping
__global__ __launch_bounds__(LG_NT) void kp_logm_aug_inv_kernel(const double* __restrict__ M, double* __restrict__ X, int n, const int* __restrict__ act,
                                                                int* __restrict__ bad, double* __restrict__ logdet, int* __restrict__ neg) {
  const int b = blockIdx.y;
  if (!act[b]) return;
  const int64_t nn = (int64_t)n * n;
  double* Xb = X + (size_t)b * 2 * nn;
  const double* Mb = M + (size_t)b * nn;
  for (int64_t e = (int64_t)blockIdx.x * LG_NT + threadIdx.x; e < 2 * nn; e += (int64_t)gridDim.x * LG_NT) {
    if (e < nn) Xb[e] = Mb[e];
    else {
      const int64_t f = e - nn;
      Xb[e] = ((f % n) == (f / n)) ? 1.0 : 0.0;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { bad[b] = 0; logdet[b] = 0.0; neg[b] = 0; }
}

// M <- (I + (mu^2 M + mu^-2 Mi) / 2) / 2,  W <- mu (I + mu^-2 Mi) / 2   (grid: tiles x matrices; Mi = right half of X)
__global__ __launch_bounds__(LG_NT) void kp_logm_db_update_kernel(double* __restrict__ M, double* __restrict__ W, const double* __restrict__ X, int n,
                                                                  const int* __restrict__ act, const int* __restrict__ bad,
                                                                  const double* __restrict__ logdet) {
  const int b = blockIdx.y;
  if (!act[b] || bad[b]) return;
  const int64_t nn = (int64_t)n * n, o = (int64_t)b * nn;
  const double mu = exp(-logdet[b] / (2.0 * n));
  const double mu2 = mu * mu, imu2 = 1.0 / mu2;
  const double* Mi = X + (size_t)b * 2 * nn + nn;
  for (int64_t e = (int64_t)blockIdx.x * LG_NT + threadIdx.x; e < nn; e += (int64_t)gridDim.x * LG_NT) {
    const double id = ((e % n) == (e / n)) ? 1.0 : 0.0;
    const double mi = Mi[e];
    M[o + e] = 0.5 * (id + 0.5 * (mu2 * M[o + e] + imu2 * mi));
    W[o + e] = 0.5 * mu * (id + imu2 * mi);
  }
}

// commits Y+ (transposed), tests convergence; counts the matrices still iterating into *cnt
__global__ __launch_bounds__(LG_NT) void kp_logm_db_finish_kernel(const double* __restrict__ M, double* __restrict__ Yt, const double* __restrict__ Ytmp,
                                                                  int n, int* __restrict__ act, const int* __restrict__ bad,
                                                                  const int* __restrict__ neg, LgState* __restrict__ st, int* __restrict__ cnt,
                                                                  int* __restrict__ other) {
  __shared__ double sv[LG_NT];
  __shared__ int fail;
  const int b = blockIdx.x;
  if (b == 0 && threadIdx.x == 0) *other = 0;
  if (!act[b]) return;
  const int64_t nn = (int64_t)n * n, o = (int64_t)b * nn;
  if (threadIdx.x == 0) fail = bad[b] || (st[b].it == 0 && neg[b]);    // singular pivot; det(A) < 0: no real logarithm
  __syncthreads();
  if (fail) {
    if (threadIdx.x == 0) { st[b].status = KP_ERR_NOT_CONVERGED; act[b] = 0; st[b].active = 0; }
    return;
  }
  for (int64_t e = threadIdx.x; e < nn; e += LG_NT) Yt[o + e] = Ytmp[o + e];
  const double d = lg_norm1_minus_I(M + o, n, sv);
  if (threadIdx.x == 0) {
    const int it = st[b].it + 1;
    int a = 1;
    if (!(d < INFINITY)) { st[b].status = KP_ERR_NOT_CONVERGED; a = 0; }
    else if (d <= 1e-13 || st[b].dprev <= 1e-7) a = 0;             // quadratic convergence: the step after 1e-7 is at round-off
    else if (it >= LG_DB_CAP) { st[b].status = KP_ERR_NOT_CONVERGED; a = 0; }
    st[b].it = it; st[b].dprev = d; st[b].active = a; act[b] = a;
    if (a) atomicAdd(cnt, 1);
  }
}

// Aold <- A, A <- Y = Yt' for the matrices that took a square root (grid: tiles x matrices)
__global__ __launch_bounds__(LG_NT) void kp_logm_sqrt_commit_kernel(double* __restrict__ A, double* __restrict__ Aold, const double* __restrict__ Yt, int n,
                                                                    LgState* __restrict__ st) {
  const int b = blockIdx.y;
  if (!st[b].sq || st[b].status != KP_OK) return;
  const int64_t nn = (int64_t)n * n, o = (int64_t)b * nn;
  for (int64_t e = (int64_t)blockIdx.x * LG_NT + threadIdx.x; e < nn; e += (int64_t)gridDim.x * LG_NT) {
    const int i = (int)(e % n), j = (int)(e / n);
    Aold[o + e] = A[o + e];
    A[o + e] = Yt[o + j + (int64_t)i * n];
  }
}

// the square root must square back: ||Y^2 - Aold||_1 <= 1e-8 ||Aold||_1, else the matrix is refused (an inverse of an
// ill-conditioned iterate can send the iteration to a wrong fixed point without any non-finite value)
__global__ __launch_bounds__(LG_NT) void kp_logm_sqrt_check_kernel(const double* __restrict__ Y2, const double* __restrict__ Aold, int n,
                                                                   LgState* __restrict__ st) {
  __shared__ double sv[LG_NT];
  const int b = blockIdx.x;
  if (!st[b].sq || st[b].status != KP_OK) return;
  const int64_t nn = (int64_t)n * n, o = (int64_t)b * nn;
  double rmax = 0.0, amax = 0.0;
  for (int c = threadIdx.x; c < n; c += LG_NT) {
    double r = 0.0, a = 0.0;
    for (int i = 0; i < n; ++i) {
      r += fabs(Y2[o + i + (int64_t)c * n] - Aold[o + i + (int64_t)c * n]);
      a += fabs(Aold[o + i + (int64_t)c * n]);
    }
    rmax = (r > rmax || r != r) ? r : rmax;
    amax = a > amax ? a : amax;
  }
  rmax = lg_block_sum_max(rmax, sv);
  amax = lg_block_sum_max(amax, sv);
  if (threadIdx.x == 0) {
    if (!(rmax <= 1e-8 * amax)) st[b].status = KP_ERR_NOT_CONVERGED;
    else st[b].nsqrt += 1;
  }
}

// 7-point Gauss-Legendre rule on [-1, 1]
__constant__ double lg_xi[7] = {-0.9491079123427585, -0.7415311855993945, -0.4058451513773972, 0.0,
                                0.4058451513773972, 0.7415311855993945, 0.9491079123427585};
__constant__ double lg_wi[7] = {0.1294849661688697, 0.2797053914892766, 0.3818300505051189, 0.4179591836734694,
                                0.3818300505051189, 0.2797053914892766, 0.1294849661688697};

// systems s = j nb + b: [I + x_j X | X], X = A - I (grid: tiles x 7 nb)
__global__ __launch_bounds__(LG_NT) void kp_logm_pade_prep_kernel(const double* __restrict__ A, double* __restrict__ Xs, int n, int nb,
                                                                  const LgState* __restrict__ st, int* __restrict__ act, int* __restrict__ bad,
                                                                  double* __restrict__ logdet, int* __restrict__ neg) {
  const int s = blockIdx.y, j = s / nb, b = s - j * nb;
  const int ok = st[b].status == KP_OK;
  if (blockIdx.x == 0 && threadIdx.x == 0) { act[s] = ok; bad[s] = 0; logdet[s] = 0.0; neg[s] = 0; }
  if (!ok) return;
  const double x = 0.5 * (1.0 + lg_xi[j]);
  const int64_t nn = (int64_t)n * n;
  const double* Ab = A + (size_t)b * nn;
  double* Xb = Xs + (size_t)s * 2 * nn;
  for (int64_t e = (int64_t)blockIdx.x * LG_NT + threadIdx.x; e < nn; e += (int64_t)gridDim.x * LG_NT) {
    const double id = ((e % n) == (e / n)) ? 1.0 : 0.0;
    const double xe = Ab[e] - id;
    Xb[e] = id + x * xe;
    Xb[nn + e] = xe;
  }
}

// L = scale 2^s sum_j w_j T_j, NaN for a failed matrix (grid: tiles x matrices)
__global__ __launch_bounds__(LG_NT) void kp_logm_pade_sum_kernel(const double* __restrict__ Xs, double* __restrict__ L, int n, int nb, double scale,
                                                                 LgState* __restrict__ st, const int* __restrict__ bad) {
  const int b = blockIdx.y;
  int ok = st[b].status == KP_OK;
  for (int j = 0; j < 7; ++j) ok = ok && !bad[j * nb + b];
  const int64_t nn = (int64_t)n * n;
  const double f = scale * ldexp(1.0, st[b].nsqrt);
  for (int64_t e = (int64_t)blockIdx.x * LG_NT + threadIdx.x; e < nn; e += (int64_t)gridDim.x * LG_NT) {
    double v = NAN;
    if (ok) {
      v = 0.0;
      for (int j = 0; j < 7; ++j) v += 0.5 * lg_wi[j] * Xs[(size_t)(j * nb + b) * 2 * nn + nn + e];
      v *= f;
      if (!(fabs(v) < INFINITY)) ok = 0;
    }
    L[(size_t)b * nn + e] = v;
  }
  // a non-finite entry anywhere marks the whole matrix (the host turns it into NaN)
  if (!ok && st[b].status == KP_OK) st[b].status = KP_ERR_NOT_CONVERGED;
}

__global__ __launch_bounds__(LG_NT) void kp_logm_nan_kernel(double* __restrict__ L, int n, const LgState* __restrict__ st) {
  const int b = blockIdx.y;
  if (st[b].status == KP_OK) return;
  const int64_t nn = (int64_t)n * n;
  for (int64_t e = (int64_t)blockIdx.x * LG_NT + threadIdx.x; e < nn; e += (int64_t)gridDim.x * LG_NT) L[(size_t)b * nn + e] = NAN;
}

inline unsigned lg_tiles(int64_t elems) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((elems + LG_NT - 1) / LG_NT, 1024)); }

// n Gauss-Jordan steps over nsys systems of n x ncol held in buf0; returns the buffer holding [I | M^-1 R]
double* lg_gauss_jordan(hipStream_t s, double* buf0, double* buf1, int nsys, int n, int ncol, const int* act, int* bad, double* logdet, int* neg) {
  const int64_t stride = (int64_t)n * ncol;
  for (int k = 0; k < n; ++k) {
    const double* X = (k & 1) ? buf1 : buf0;
    double* Y = (k & 1) ? buf0 : buf1;
    const int64_t tot = (int64_t)n * (ncol - k - 1);
    const unsigned gx = (unsigned)std::max<int64_t>(1, (tot + LG_NT * LG_EPT - 1) / (LG_NT * LG_EPT));
    hipLaunchKernelGGL(kp_gj_step_kernel, dim3(gx, nsys), dim3(LG_NT), 0, s, X, Y, stride, n, ncol, k, act, bad, logdet, neg);
  }
  return (n & 1) ? buf1 : buf0;
}

int lg_read_count(kp_ctx* ctx, int* cnt_dev, int* out) {
  KP_HIP(ctx, hipMemcpyAsync(out, cnt_dev, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  KP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return KP_OK;
}

// one chunk of matrices, all on the device; A is overwritten; *st_out: the per-matrix state
int lg_chunk(kp_ctx* ctx, int nb, int n, double* A, double shift, double scale, double* L, char* ws, LgState** st_out) {
  hipStream_t s = ctx->stream;
  const int64_t nn = (int64_t)n * n;
  auto take = [&](size_t bytes) { char* p = ws; ws += (bytes + 255) / 256 * 256; return p; };
  double* M = (double*)take(nb * nn * 8);
  double* Yt = (double*)take(nb * nn * 8);
  double* Ytmp = (double*)take(nb * nn * 8);
  double* W = (double*)take(nb * nn * 8);
  double* buf0 = (double*)take((size_t)7 * nb * 2 * nn * 8);
  double* buf1 = (double*)take((size_t)7 * nb * 2 * nn * 8);
  LgState* st = (LgState*)take(nb * sizeof(LgState));
  int* act = (int*)take(nb * 4);
  int* pact = (int*)take(7 * nb * 4);
  int* bad = (int*)take(7 * nb * 4);
  int* neg = (int*)take(7 * nb * 4);
  double* logdet = (double*)take(7 * nb * 8);
  int* cnt = (int*)take(2 * 4);      // two counters: each counting launch adds to one and clears the other
  int ci = 0;
  *st_out = st;
  const unsigned tiles = lg_tiles(nn);
  KP_HIP(ctx, hipMemsetAsync(cnt, 0, 2 * 4, s));
  hipLaunchKernelGGL(kp_logm_start_kernel, dim3(nb), dim3(LG_NT), 0, s, A, n, shift, st);
  for (int sq = 0; sq <= LG_MAX_SQRT; ++sq) {
    int* c0 = cnt + ci;
    hipLaunchKernelGGL(kp_logm_check_kernel, dim3(nb), dim3(LG_NT), 0, s, A, n, st, c0, cnt + (ci ^ 1));
    ci ^= 1;
    KP_HIP(ctx, hipGetLastError());
    int need = 0;
    if (int rc = lg_read_count(ctx, c0, &need)) return rc;
    if (!need) break;
    hipLaunchKernelGGL(kp_logm_db_init_kernel, dim3(tiles, nb), dim3(LG_NT), 0, s, A, M, Yt, n, st, act);
    for (int it = 0; it < LG_DB_CAP; ++it) {
      hipLaunchKernelGGL(kp_logm_aug_inv_kernel, dim3(lg_tiles(2 * nn), nb), dim3(LG_NT), 0, s, M, buf0, n, act, bad, logdet, neg);
      double* R = lg_gauss_jordan(s, buf0, buf1, nb, n, 2 * n, act, bad, logdet, neg);
      hipLaunchKernelGGL(kp_logm_db_update_kernel, dim3(tiles, nb), dim3(LG_NT), 0, s, M, W, R, n, act, bad, logdet);
      KP_HIP(ctx, hipGetLastError());
      for (int b = 0; b < nb; ++b)       // Ytmp_b = W_b' Yt_b  (= (Y W)')
        KP_HIP(ctx, kp_tn_gemm(s, W + b * nn, n, Yt + b * nn, n, n, n, n, Ytmp + b * nn, n, 1.0, 0.0, 0, 1, nullptr));
      int* c1 = cnt + ci;
      hipLaunchKernelGGL(kp_logm_db_finish_kernel, dim3(nb), dim3(LG_NT), 0, s, M, Yt, Ytmp, n, act, bad, neg, st, c1, cnt + (ci ^ 1));
      ci ^= 1;
      KP_HIP(ctx, hipGetLastError());
      if (it >= 2) {     // a scaled iteration takes 3-4 steps: no host round trip before the third
        int left = 0;
        if (int rc = lg_read_count(ctx, c1, &left)) return rc;
        if (!left) break;
      }
    }
    hipLaunchKernelGGL(kp_logm_sqrt_commit_kernel, dim3(tiles, nb), dim3(LG_NT), 0, s, A, M, Yt, n, st);
    KP_HIP(ctx, hipGetLastError());
    for (int b = 0; b < nb; ++b)         // Ytmp_b = Yt_b' A_b = Y_b^2
      KP_HIP(ctx, kp_tn_gemm(s, Yt + b * nn, n, A + b * nn, n, n, n, n, Ytmp + b * nn, n, 1.0, 0.0, 0, 1, nullptr));
    hipLaunchKernelGGL(kp_logm_sqrt_check_kernel, dim3(nb), dim3(LG_NT), 0, s, Ytmp, M, n, st);
    KP_HIP(ctx, hipGetLastError());
  }
  // quadrature: the 7 solves of every matrix in one Gauss-Jordan batch
  hipLaunchKernelGGL(kp_logm_pade_prep_kernel, dim3(tiles, 7 * nb), dim3(LG_NT), 0, s, A, buf0, n, nb, st, pact, bad, logdet, neg);
  double* R = lg_gauss_jordan(s, buf0, buf1, 7 * nb, n, 2 * n, pact, bad, logdet, neg);
  hipLaunchKernelGGL(kp_logm_pade_sum_kernel, dim3(tiles, nb), dim3(LG_NT), 0, s, R, L, n, nb, scale, st, bad);
  hipLaunchKernelGGL(kp_logm_nan_kernel, dim3(tiles, nb), dim3(LG_NT), 0, s, L, n, st);
  KP_HIP(ctx, hipGetLastError());
  return KP_OK;
}

}  // namespace

extern "C" int kp_logm(kp_ctx* ctx, int nb, int n, const double* A, double shift, double scale, double* L, int* nsqrt, int* status) {
  if (!ctx || !A || !L || !status || nb < 1) return ctx ? ctx->fail(KP_ERR_ARG, "kp_logm: bad argument") : KP_ERR_ARG;
  if (n < 1 || n > 512) return ctx->fail(KP_ERR_ARG, "kp_logm: n must be in 1..512");
  if (!std::isfinite(shift) || !std::isfinite(scale)) return ctx->fail(KP_ERR_ARG, "kp_logm: shift and scale must be finite");
  KP_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->async_pending) {
    int rc0 = kp_synchronize(ctx);
    if (rc0) return rc0;
  }
  const size_t nn = (size_t)n * n;
  // per matrix: A, L, M, Yt, Ytmp, W and the 2 x 7 augmented systems (34 n^2 doubles); chunks of at most ~1 GB
  const size_t per = (34 * nn) * 8 + 1024;
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)nb, ((size_t)1 << 30) / per));
  // + the 256-byte-aligned pieces of lg_chunk: state, flags, pivot bookkeeping, counters
  const size_t small = (size_t)chunk * (sizeof(LgState) + 4 + 3 * 7 * 4 + 7 * 8) + 16 * 256;
  char* ws = (char*)ctx->workspace(6, (size_t)chunk * per + small);
  if (!ws) return ctx->fail(KP_ERR_HIP, "kp_logm: out of device memory");
  hipStream_t s = ctx->stream;
  double* dA = (double*)ws;
  double* dL = dA + (size_t)chunk * nn;
  char* rest = (char*)(dL + (size_t)chunk * nn);
  rest = (char*)(((uintptr_t)rest + 255) / 256 * 256);
  std::vector<LgState> hst(chunk);
  KP_HIP(ctx, hipEventRecord(ctx->ev0, s));
  for (int b0 = 0; b0 < nb; b0 += chunk) {
    const int cb = std::min(chunk, nb - b0);
    KP_HIP(ctx, hipMemcpyAsync(dA, A + b0 * nn, cb * nn * 8, hipMemcpyHostToDevice, s));
    LgState* dst = nullptr;
    if (int rc = lg_chunk(ctx, cb, n, dA, shift, scale, dL, rest, &dst)) return rc;
    KP_HIP(ctx, hipMemcpyAsync(L + b0 * nn, dL, cb * nn * 8, hipMemcpyDeviceToHost, s));
    KP_HIP(ctx, hipMemcpyAsync(hst.data(), dst, cb * sizeof(LgState), hipMemcpyDeviceToHost, s));
    KP_HIP(ctx, hipStreamSynchronize(s));
    for (int b = 0; b < cb; ++b) {
      status[b0 + b] = hst[b].status;
      if (nsqrt) nsqrt[b0 + b] = hst[b].nsqrt;
    }
  }
  KP_HIP(ctx, hipEventRecord(ctx->ev1, s));
  KP_HIP(ctx, hipStreamSynchronize(s));
  return KP_OK;
}
