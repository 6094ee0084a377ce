// kp_eig (include/koopman_hip_spectrum.h): eigenvalues and right eigenvectors of a batch of real general matrices, one matrix
// per workgroup, the batch in the grid.  The classical real algorithm, restated from the textbook (tests/_eig_reference.py is
// the same restatement in numpy, step for step):
//   1. balancing by powers of two, no permutation (exact arithmetic)
//   2. Householder reduction to Hessenberg form H; with vectors the reflectors are accumulated forwards into Z
//   3. Francis double-shift QR with deflation; exceptional shifts at iterations 10 and 20 of an eigenvalue, at most
//      KP_EIG_MAX_ITER.  With vectors the reflectors go to the whole of H and to Z (H ends quasi-triangular, A = Z T Z');
//      with values only to the active window
//   4. back-substitution on T, one lane per eigenvalue (a pair in real arithmetic) into X; V = Z X over the workgroup; the
//      balancing undone; unit 2-norm
// All control flow is uniform: every thread reads the same pivots and shifts from the shared matrix and computes the same
// scalars.  The discipline that makes that safe: a phase that reads pivots ends with a barrier before any thread overwrites
// them.  One bulge step is [pivots, row update | barrier | column update, Z update, the new pivot | barrier]: two barriers.
// Searches (the small subdiagonal, two consecutive small subdiagonals) are maximum reductions, sums go through __shfl_xor
// within a wave and then through LDS slots; the butterfly leaves the same bits in every lane, and every wave adds the slots in
// the same order.  Every loop has a bound from its arguments; a matrix that reaches a cap writes NaN and its status and ends.
//
// Regimes (kp_timer_get 23): 1 - n <= KP_EIG_WAVE_MAX, 64 threads, H and Z in LDS: the barrier of a one-wave workgroup is
// lowered to wave-level synchronisation by the compiler, and the few KB of LDS let many workgroups share a CU; 2 - 256 threads,
// LDS-resident; 3 - 256 threads, H and Z in a workspace slot, L2-resident, visibility by the workgroup's barriers.  2 and 3
// are one body with two storage accessors and no contraction of multiply-adds, so they return the same bits.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>

#include "kp_internal.h"
#include "koopman_hip_spectrum.h"

#pragma clang fp contract(off)

namespace {

constexpr int EIG_BAL_SWEEPS = 64;      // balancing sweeps (a sweep that changes nothing ends them)
constexpr int EIG_SCRATCH_PAD = 64;     // reduction slots behind the four n-vectors of the scratch

static_assert(2 * KP_EIG_LDS_MAXN_VEC * (KP_EIG_LDS_MAXN_VEC + 1) + 4 * KP_EIG_LDS_MAXN_VEC + EIG_SCRATCH_PAD <= 20480 &&
              2 * (KP_EIG_LDS_MAXN_VEC + 1) * (KP_EIG_LDS_MAXN_VEC + 2) + 4 * (KP_EIG_LDS_MAXN_VEC + 1) + EIG_SCRATCH_PAD > 20480,
              "KP_EIG_LDS_MAXN_VEC is not the largest n of the header's formula");
static_assert(KP_EIG_LDS_MAXN_VAL * (KP_EIG_LDS_MAXN_VAL + 1) + 4 * KP_EIG_LDS_MAXN_VAL + EIG_SCRATCH_PAD <= 20480 &&
              (KP_EIG_LDS_MAXN_VAL + 1) * (KP_EIG_LDS_MAXN_VAL + 2) + 4 * (KP_EIG_LDS_MAXN_VAL + 1) + EIG_SCRATCH_PAD > 20480,
              "KP_EIG_LDS_MAXN_VAL is not the largest n of the header's formula");

struct EigArgs {
  int n, ld, vec;
  const double* A;   // nb x [n x n]
  double* wr;        // nb x n
  double* wi;
  double* V;         // nb x [n x n] (vec)
  double* X;         // nb x [n x n] (vec): the back-substituted vectors of T
  double* G;         // regime 3: nb x [nmat x n x ld]
  int* iters;
  int* status;
};

// the two storage accessors: column-major with leading dimension ld (odd: a column walk and a row walk both spread over the banks)
struct LdsMat {
  double* p;
  int ld;
  __device__ __forceinline__ double& operator()(int i, int j) const { return p[i + j * ld]; }
};
struct GlobalMat {
  double* p;
  int ld;
  __device__ __forceinline__ double& operator()(int i, int j) const { return p[(size_t)i + (size_t)j * ld]; }
};

// Sum (OP 0) or maximum (OP 1) over the workgroup, the same bits in every thread; ends behind a barrier.  `red` holds two
// banks of slots used in turn: the barrier of one reduction separates the reads of the previous from the writes of the next.
template <int NT, int OP>
__device__ __forceinline__ double eig_reduce(double v, double* red, int& par) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double w = __shfl_xor(v, o, 64);
    v = OP == 0 ? v + w : fmax(v, w);
  }
  if (NT > 64) {
    constexpr int NW = NT / 64;
    double* slot = red + par * NW;
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    v = slot[0];
#pragma unroll
    for (int k = 1; k < NW; ++k) v = OP == 0 ? v + slot[k] : fmax(v, slot[k]);
    par ^= 1;
  } else {
    __syncthreads();
  }
  return v;
}

__device__ __forceinline__ void eig_cdiv(double ar, double ai, double br, double bi, double& cr, double& ci) {
  double s = fabs(br) + fabs(bi);
  const double ars = ar / s, ais = ai / s, brs = br / s, bis = bi / s;
  s = brs * brs + bis * bis;
  cr = (ars * brs + ais * bis) / s;
  ci = (ais * brs - ars * bis) / s;
}

// v scaled down by 0.01 until tst1 + v == tst1 (the perturbation of a zero pivot in the back-substitution)
__device__ __forceinline__ double eig_perturb(double tst1, double v) {
  for (int k = 0; k < 40; ++k) {
    v *= 0.01;
    if (!(tst1 + v > tst1)) break;
  }
  return v;
}

template <int NT>
__device__ void eig_fail(const EigArgs& a, int b, int total) {
  const int n = a.n, tid = threadIdx.x;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int i = tid; i < n; i += NT) {
    a.wr[(size_t)b * n + i] = nan;
    a.wi[(size_t)b * n + i] = nan;
  }
  if (a.vec)
    for (int i = tid; i < n * n; i += NT) a.V[(size_t)b * n * n + i] = nan;
  if (tid == 0) {
    a.iters[b] = total;
    a.status[b] = KP_ERR_NOT_CONVERGED;
  }
}

// the start of a double-shift step at row m: the first column of (H - s1)(H - s2), scaled
template <class Mat>
__device__ __forceinline__ void eig_start(const Mat& H, int m, double x, double y, double w, double& p, double& q, double& r) {
  const double zz = H(m, m);
  const double rr = x - zz, ss = y - zz;
  p = (rr * ss - w) / H(m + 1, m) + H(m, m + 1);
  q = H(m + 1, m + 1) - zz - rr - ss;
  r = H(m + 2, m + 1);
  const double s = fabs(p) + fabs(q) + fabs(r);
  p /= s;
  q /= s;
  r /= s;
}

template <int NT, class Mat>
__device__ void eig_body(const EigArgs& a, const Mat H, const Mat Z, double* sc, const int b) {
  const int n = a.n, tid = threadIdx.x;
  const bool vec = a.vec != 0;
  double* ort = sc;
  double* wr = sc + n;
  double* wi = sc + 2 * n;
  double* scl = sc + 3 * n;
  double* red = sc + 4 * n;
  int par = 0;
  const double* A = a.A + (size_t)b * n * n;

  // ---- load; a non-finite entry makes v - v NaN ----
  double bad = 0.0;
  for (int idx = tid; idx < n * n; idx += NT) {
    const int i = idx % n, j = idx / n;
    const double v = A[idx];
    H(i, j) = v;
    bad += v - v;
    if (vec) Z(i, j) = i == j ? 1.0 : 0.0;
  }
  for (int i = tid; i < n; i += NT) scl[i] = 1.0;
  bad = eig_reduce<NT, 0>(bad, red, par);
  if (!(bad == 0.0)) {
    eig_fail<NT>(a, b, 0);
    return;
  }

  // ---- 1. balancing: D^-1 H D with D = diag(scl) of powers of two ----
  for (int sweep = 0; sweep < EIG_BAL_SWEEPS; ++sweep) {
    bool changed = false;
    for (int i = 0; i < n; ++i) {
      double c = 0.0, r = 0.0;
      for (int j = tid; j < n; j += NT) {   // the diagonal entry counts in both norms: a row of rounding noise beside a
        c += fabs(H(j, i));                 // diagonal of order one (the constant observable of a fitted model) is left
        r += fabs(H(i, j));                 // alone - scaling it up would cost the vectors their residual after the way back
      }
      c = eig_reduce<NT, 0>(c, red, par);
      r = eig_reduce<NT, 0>(r, red, par);
      if (c == 0.0 || r == 0.0) continue;
      double g = r / 2.0, f = 1.0;
      const double s = c + r;
      for (int k = 0; k < 1100 && c < g; ++k) {
        f *= 2.0;
        c *= 4.0;
      }
      g = r * 2.0;
      for (int k = 0; k < 1100 && c >= g; ++k) {
        f /= 2.0;
        c /= 4.0;
      }
      if ((c + r) / f < 0.95 * s) {
        changed = true;
        const double fi = 1.0 / f;
        if (tid == 0) scl[i] *= f;
        for (int j = tid; j < n; j += NT) {   // (i, i) is scaled down and up by the one thread j == i
          H(i, j) *= fi;
          H(j, i) *= f;
        }
        __syncthreads();
      }
    }
    if (!changed) break;
  }

  // ---- 2. Householder reduction to Hessenberg form ----
  for (int m = 1; m < n - 1; ++m) {
    double s = 0.0;
    for (int i = m + tid; i < n; i += NT) s += fabs(H(i, m - 1));
    const double scale = eig_reduce<NT, 0>(s, red, par);
    if (scale == 0.0) continue;
    double hh = 0.0;
    for (int i = m + tid; i < n; i += NT) {
      const double v = H(i, m - 1) / scale;
      ort[i] = v;
      hh += v * v;
    }
    double h = eig_reduce<NT, 0>(hh, red, par);
    const double om0 = ort[m];
    const double g = -copysign(sqrt(h), om0);
    h -= om0 * g;
    const double om = om0 - g;   // the reflector's entry m, kept in a register: ort[m] itself stays as it is
    // (I - u u' / h) H: one column per thread
    for (int j = m + tid; j < n; j += NT) {
      double f = om * H(m, j);
      for (int i = m + 1; i < n; ++i) f += ort[i] * H(i, j);
      f /= h;
      H(m, j) -= f * om;
      for (int i = m + 1; i < n; ++i) H(i, j) -= f * ort[i];
    }
    __syncthreads();
    // H (I - u u' / h) and Z (I - u u' / h): one row per thread
    for (int i = tid; i < n; i += NT) {
      double f = H(i, m) * om;
      for (int j = m + 1; j < n; ++j) f += H(i, j) * ort[j];
      f /= h;
      H(i, m) -= f * om;
      for (int j = m + 1; j < n; ++j) H(i, j) -= f * ort[j];
      if (vec) {
        f = Z(i, m) * om;
        for (int j = m + 1; j < n; ++j) f += Z(i, j) * ort[j];
        f /= h;
        Z(i, m) -= f * om;
        for (int j = m + 1; j < n; ++j) Z(i, j) -= f * ort[j];
      }
    }
    if (tid == 0) H(m, m - 1) = scale * g;
    for (int i = m + 1 + tid; i < n; i += NT) H(i, m - 1) = 0.0;
    __syncthreads();
  }

  // ---- 3. Francis double-shift QR ----
  double norm = 0.0;
  {
    double s = 0.0;
    for (int j = tid; j < n; j += NT) {
      const int i1 = min(j + 2, n);
      for (int i = 0; i < i1; ++i) s += fabs(H(i, j));
    }
    norm = eig_reduce<NT, 0>(s, red, par);
  }
  int en = n - 1, its = 0, total = 0;
  double t = 0.0;
  bool ok = true;
  const int maxpass = (KP_EIG_MAX_ITER + 1) * n + 1;
  for (int pass = 0; pass < maxpass && en >= 0; ++pass) {
    // the largest l <= en whose subdiagonal entry H(l, l - 1) is negligible (0: none)
    double lm = 0.0;
    for (int i = 1 + tid; i <= en; i += NT) {
      double s = fabs(H(i - 1, i - 1)) + fabs(H(i, i));
      if (s == 0.0) s = norm;
      if (s + fabs(H(i, i - 1)) == s) lm = (double)i;
    }
    const int l = (int)eig_reduce<NT, 1>(lm, red, par);
    double x = H(en, en), y = 0.0, w = 0.0, hl = 0.0, hl2 = 0.0;
    if (en >= 1) {
      y = H(en - 1, en - 1);
      hl = H(en, en - 1);
      w = hl * H(en - 1, en);
    }
    if (en >= 2) hl2 = H(en - 1, en - 2);
    __syncthreads();   // every thread holds the pivots before any of them is overwritten
    if (l == en) {     // one root
      if (tid == 0) {
        wr[en] = x + t;
        wi[en] = 0.0;
        H(en, en) = x + t;
      }
      --en;
      its = 0;
      continue;
    }
    if (l == en - 1) {   // two roots
      double p = (y - x) / 2.0;
      double q = p * p + w;
      double zz = sqrt(fabs(q));
      const double xx = x + t;
      if (tid == 0) {
        H(en, en) = xx;
        H(en - 1, en - 1) = y + t;
      }
      if (q >= 0.0) {   // a real pair
        zz = p + copysign(zz, p);
        if (tid == 0) {
          wr[en - 1] = xx + zz;
          wr[en] = zz != 0.0 ? xx - w / zz : xx + zz;
          wi[en - 1] = 0.0;
          wi[en] = 0.0;
        }
        if (vec) {   // the rotation that makes the block upper triangular
          __syncthreads();
          const double s = fabs(hl) + fabs(zz);
          p = hl / s;
          q = zz / s;
          const double r = sqrt(p * p + q * q);
          p /= r;
          q /= r;
          for (int j = en - 1 + tid; j < n; j += NT) {
            const double u = H(en - 1, j), v = H(en, j);
            H(en - 1, j) = q * u + p * v;
            H(en, j) = q * v - p * u;
          }
          __syncthreads();
          for (int i = tid; i <= en; i += NT) {
            const double u = H(i, en - 1), v = H(i, en);
            H(i, en - 1) = q * u + p * v;
            H(i, en) = q * v - p * u;
          }
          for (int i = tid; i < n; i += NT) {
            const double u = Z(i, en - 1), v = Z(i, en);
            Z(i, en - 1) = q * u + p * v;
            Z(i, en) = q * v - p * u;
          }
          __syncthreads();
        }
      } else if (tid == 0) {   // a complex pair, the positive imaginary part first
        wr[en - 1] = xx + p;
        wr[en] = xx + p;
        wi[en - 1] = zz;
        wi[en] = -zz;
      }
      en -= 2;
      its = 0;
      continue;
    }
    if (its == KP_EIG_MAX_ITER) {
      ok = false;
      break;
    }
    if (its == 10 || its == 20) {   // exceptional shift
      t += x;
      for (int i = tid; i <= en; i += NT) H(i, i) -= x;
      const double s = fabs(hl) + fabs(hl2);
      x = y = 0.75 * s;
      w = -0.4375 * s * s;
      __syncthreads();
    }
    ++its;
    ++total;
    // the largest m in (l, en - 2] with two consecutive small subdiagonal entries (l: none)
    double mm = (double)l;
    for (int c = l + 1 + tid; c <= en - 2; c += NT) {
      double p, q, r;
      eig_start(H, c, x, y, w, p, q, r);
      const double tst1 = fabs(p) * (fabs(H(c - 1, c - 1)) + fabs(H(c, c)) + fabs(H(c + 1, c + 1)));
      const double tst2 = fabs(H(c, c - 1)) * (fabs(q) + fabs(r));
      if (tst1 + tst2 == tst1) mm = (double)c;
    }
    const int m = (int)eig_reduce<NT, 1>(mm, red, par);
    double p, q, r;
    eig_start(H, m, x, y, w, p, q, r);
    const double hm = m > l ? H(m, m - 1) : 0.0;
    for (int i = m + 2 + tid; i <= en; i += NT) {
      H(i, i - 2) = 0.0;
      if (i != m + 2) H(i, i - 3) = 0.0;
    }
    __syncthreads();   // the start vector is read, the stale bulge entries are cleared
    const int j1 = vec ? n : en + 1;
    const int i0 = vec ? 0 : l;
    for (int k = m; k < en; ++k) {   // the bulge chase: two barriers a step
      const bool notlast = k != en - 1;
      if (k != m) {
        p = H(k, k - 1);
        q = H(k + 1, k - 1);
        r = notlast ? H(k + 2, k - 1) : 0.0;
        x = fabs(p) + fabs(q) + fabs(r);
        if (x == 0.0) continue;
        p /= x;
        q /= x;
        r /= x;
      }
      const double s = copysign(sqrt(p * p + q * q + r * r), p);
      bool setpiv = false;
      double piv = 0.0;
      if (k != m) {
        piv = -s * x;
        setpiv = true;
      } else if (l != m) {
        piv = -hm;
        setpiv = true;
      }
      p += s;
      x = p / s;
      y = q / s;
      const double zz = r / s;
      q /= p;
      r /= p;
      const int i1 = min(en, k + 3);
      if (notlast) {
        for (int j = k + tid; j < j1; j += NT) {
          const double pp = H(k, j) + q * H(k + 1, j) + r * H(k + 2, j);
          H(k, j) -= pp * x;
          H(k + 1, j) -= pp * y;
          H(k + 2, j) -= pp * zz;
        }
        __syncthreads();
        for (int i = i0 + tid; i <= i1; i += NT) {
          const double pp = x * H(i, k) + y * H(i, k + 1) + zz * H(i, k + 2);
          H(i, k) -= pp;
          H(i, k + 1) -= pp * q;
          H(i, k + 2) -= pp * r;
        }
        if (vec)
          for (int i = tid; i < n; i += NT) {
            const double pp = x * Z(i, k) + y * Z(i, k + 1) + zz * Z(i, k + 2);
            Z(i, k) -= pp;
            Z(i, k + 1) -= pp * q;
            Z(i, k + 2) -= pp * r;
          }
      } else {
        for (int j = k + tid; j < j1; j += NT) {
          const double pp = H(k, j) + q * H(k + 1, j);
          H(k, j) -= pp * x;
          H(k + 1, j) -= pp * y;
        }
        __syncthreads();
        for (int i = i0 + tid; i <= i1; i += NT) {
          const double pp = x * H(i, k) + y * H(i, k + 1);
          H(i, k) -= pp;
          H(i, k + 1) -= pp * q;
        }
        if (vec)
          for (int i = tid; i < n; i += NT) {
            const double pp = x * Z(i, k) + y * Z(i, k + 1);
            Z(i, k) -= pp;
            Z(i, k + 1) -= pp * q;
          }
      }
      if (setpiv && tid == 0) H(k, k - 1) = piv;
      __syncthreads();
    }
  }
  if (!ok || en >= 0) {
    eig_fail<NT>(a, b, total);
    return;
  }
  __syncthreads();   // wr, wi of thread 0
  for (int i = tid; i < n; i += NT) {
    a.wr[(size_t)b * n + i] = wr[i];
    a.wi[(size_t)b * n + i] = wi[i];
  }
  if (tid == 0) {
    a.iters[b] = total;
    a.status[b] = KP_OK;
  }
  if (!vec) return;

  // ---- 4. vectors: back-substitution on T, one lane per eigenvalue; the columns are independent ----
  double* X = a.X + (size_t)b * n * n;
  for (int e = tid; e < n; e += NT) {
    double* xe = X + (size_t)e * n;   // column e
    const double p = wr[e], q = wi[e];
    if (norm == 0.0) {
      for (int i = 0; i <= e; ++i) xe[i] = i == e ? 1.0 : 0.0;
    } else if (q == 0.0) {   // a real vector
      int m = e;
      xe[e] = 1.0;
      double zz = 0.0, s = 0.0;
      for (int i = e - 1; i >= 0; --i) {
        const double w = H(i, i) - p;
        double r = 0.0;
        for (int j = m; j <= e; ++j) r += H(i, j) * xe[j];
        if (wi[i] < 0.0) {
          zz = w;
          s = r;
          continue;
        }
        m = i;
        if (wi[i] == 0.0) {
          double tt = w;
          if (tt == 0.0) tt = eig_perturb(norm, norm);
          xe[i] = -r / tt;
        } else {
          const double x = H(i, i + 1), y = H(i + 1, i);
          const double qq = (wr[i] - p) * (wr[i] - p) + wi[i] * wi[i];
          const double tt = (x * s - zz * r) / qq;
          xe[i] = tt;
          xe[i + 1] = fabs(x) > fabs(zz) ? (-r - w * tt) / x : (-s - y * tt) / zz;
        }
        const double tt = fabs(xe[i]);
        if (tt != 0.0 && tt + 1.0 / tt <= tt)
          for (int j = i; j <= e; ++j) xe[j] /= tt;
      }
    } else if (q < 0.0) {   // the pair (e - 1, e): real part in column e - 1, imaginary part in column e
      const int na = e - 1;
      double* xa = X + (size_t)na * n;
      int m = na;
      if (fabs(H(e, na)) > fabs(H(na, e))) {
        xa[na] = q / H(e, na);
        xe[na] = -(H(e, e) - p) / H(e, na);
      } else {
        eig_cdiv(0.0, -H(na, e), H(na, na) - p, q, xa[na], xe[na]);
      }
      xa[e] = 0.0;
      xe[e] = 1.0;
      double zz = 0.0, r = 0.0, s = 0.0;
      for (int i = e - 2; i >= 0; --i) {
        const double w = H(i, i) - p;
        double ra = 0.0, sa = 0.0;
        for (int j = m; j <= e; ++j) {
          const double hij = H(i, j);
          ra += hij * xa[j];
          sa += hij * xe[j];
        }
        if (wi[i] < 0.0) {
          zz = w;
          r = ra;
          s = sa;
          continue;
        }
        m = i;
        if (wi[i] == 0.0) {
          eig_cdiv(-ra, -sa, w, q, xa[i], xe[i]);
        } else {
          const double x = H(i, i + 1), y = H(i + 1, i);
          double vr = (wr[i] - p) * (wr[i] - p) + wi[i] * wi[i] - q * q;
          const double vi = (wr[i] - p) * 2.0 * q;
          if (vr == 0.0 && vi == 0.0) {
            const double tst1 = norm * (fabs(w) + fabs(q) + fabs(x) + fabs(y) + fabs(zz));
            vr = eig_perturb(tst1, tst1);
          }
          eig_cdiv(x * r - zz * ra + q * sa, x * s - zz * sa - q * ra, vr, vi, xa[i], xe[i]);
          if (fabs(x) > fabs(zz) + fabs(q)) {
            xa[i + 1] = (-ra - w * xa[i] + q * xe[i]) / x;
            xe[i + 1] = (-sa - w * xe[i] - q * xa[i]) / x;
          } else {
            eig_cdiv(-r - y * xa[i], -s - y * xe[i], zz, q, xa[i + 1], xe[i + 1]);
          }
        }
        const double tt = fmax(fabs(xa[i]), fabs(xe[i]));
        if (tt != 0.0 && tt + 1.0 / tt <= tt)
          for (int j = i; j <= e; ++j) {
            xa[j] /= tt;
            xe[j] /= tt;
          }
      }
    }
  }
  __syncthreads();
  // V = D Z X over the workgroup (X is upper triangular in the packed form)
  double* V = a.V + (size_t)b * n * n;
  for (int idx = tid; idx < n * n; idx += NT) {
    const int i = idx % n, j = idx / n;
    const double* xj = X + (size_t)j * n;
    double s = 0.0;
    for (int k = 0; k <= j; ++k) s += Z(i, k) * xj[k];
    V[idx] = s * scl[i];
  }
  __syncthreads();
  // unit 2-norm: one lane per real column or pair
  for (int j = tid; j < n; j += NT) {
    if (wi[j] < 0.0) continue;
    double* v0 = V + (size_t)j * n;
    if (wi[j] > 0.0) {
      double* v1 = v0 + n;
      double s = 0.0;
      for (int i = 0; i < n; ++i) s += v0[i] * v0[i] + v1[i] * v1[i];
      s = sqrt(s);
      for (int i = 0; i < n; ++i) {
        v0[i] /= s;
        v1[i] /= s;
      }
    } else {
      double s = 0.0;
      for (int i = 0; i < n; ++i) s += v0[i] * v0[i];
      s = sqrt(s);
      for (int i = 0; i < n; ++i) v0[i] /= s;
    }
  }
}

extern __shared__ __attribute__((aligned(16))) char kp_eig_smem[];

template <int NT, bool LDS>
__global__ void __launch_bounds__(NT) kp_eig_kernel(const EigArgs a) {
  double* sc = (double*)kp_eig_smem;
  const int b = blockIdx.x;
  const int n = a.n, ld = a.ld;
  if (LDS) {
    double* base = sc + 4 * n + EIG_SCRATCH_PAD;
    const LdsMat H{base, ld}, Z{base + n * ld, ld};   // Z is touched only with vectors
    eig_body<NT>(a, H, Z, sc, b);
  } else {
    double* base = a.G + (size_t)b * (a.vec ? 2 : 1) * n * ld;
    const GlobalMat H{base, ld}, Z{base + (size_t)n * ld, ld};
    eig_body<NT>(a, H, Z, sc, b);
  }
}

}  // namespace

extern "C" int kp_eig(kp_ctx* ctx, int nb, int n, const double* A, int want_vectors, double* wr, double* wi, double* V, int* iters,
                      int* status) {
  if (!ctx) return KP_ERR_ARG;
  if (nb < 1) return ctx->fail(KP_ERR_ARG, "kp_eig: nb must be at least 1");
  if (n < 1 || n > KP_EIG_MAXN) return ctx->fail(KP_ERR_ARG, "kp_eig: n must be in 1..512");
  if (!A || !wr || !wi || !status) return ctx->fail(KP_ERR_ARG, "kp_eig: A, wr, wi and status must not be NULL");
  if (want_vectors && !V) return ctx->fail(KP_ERR_ARG, "kp_eig: V must not be NULL when vectors are wanted");
  KP_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->async_pending) {
    int rc0 = kp_synchronize(ctx);
    if (rc0) return rc0;
  }
  const int vec = want_vectors ? 1 : 0;
  const int nmat = vec ? 2 : 1;
  const int lds_max = vec ? KP_EIG_LDS_MAXN_VEC : KP_EIG_LDS_MAXN_VAL;
  int regime = n <= KP_EIG_WAVE_MAX ? 1 : n <= lds_max ? 2 : 3;
  if (const char* e = getenv("KP_EIG_REGIME")) {   // read per call: tests and A/B runs
    const int want = atoi(e);
    if (want == 3 || (want == 2 && n <= lds_max)) regime = want;
  }
  const int ld = n | 1;
  const size_t nn = (size_t)n * n;
  const size_t scratch = (size_t)(4 * n + EIG_SCRATCH_PAD) * 8;
  const size_t lds = regime == 3 ? scratch : scratch + (size_t)nmat * n * ld * 8;
  if (lds > 160 * 1024) return ctx->fail(KP_ERR_ARG, "kp_eig: the matrix does not fit the LDS of its regime");
  // per matrix: A, wr, wi, iters, status, with vectors V and X, in regime 3 H (and Z); chunks of at most ~1 GB
  const size_t gmat = regime == 3 ? (size_t)nmat * n * ld : 0;
  const size_t per = (nn * (vec ? 3 : 1) + 2 * (size_t)n + gmat) * 8 + 2 * sizeof(int);
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)nb, ((size_t)1 << 30) / per));
  char* ws = (char*)ctx->workspace(6, (size_t)chunk * per + 8 * 256);
  if (!ws) return ctx->fail(KP_ERR_HIP, "kp_eig: out of device memory");
  auto carve = [&](size_t bytes) {
    char* p = ws;
    ws += (bytes + 255) / 256 * 256;
    return p;
  };
  EigArgs a{};
  a.n = n;
  a.ld = ld;
  a.vec = vec;
  double* dA = (double*)carve((size_t)chunk * nn * 8);
  a.A = dA;
  a.wr = (double*)carve((size_t)chunk * n * 8);
  a.wi = (double*)carve((size_t)chunk * n * 8);
  a.V = vec ? (double*)carve((size_t)chunk * nn * 8) : nullptr;
  a.X = vec ? (double*)carve((size_t)chunk * nn * 8) : nullptr;
  a.G = gmat ? (double*)carve((size_t)chunk * gmat * 8) : nullptr;
  a.iters = (int*)carve((size_t)chunk * sizeof(int));
  a.status = (int*)carve((size_t)chunk * sizeof(int));
  hipStream_t s = ctx->stream;
  static KpLdsCache lds1, lds2, lds3;
  if (regime == 1) KP_HIP(ctx, kp_ensure_lds(lds1, (const void*)kp_eig_kernel<64, true>, lds));
  else if (regime == 2) KP_HIP(ctx, kp_ensure_lds(lds2, (const void*)kp_eig_kernel<256, true>, lds));
  else KP_HIP(ctx, kp_ensure_lds(lds3, (const void*)kp_eig_kernel<256, false>, lds));
  std::vector<int> hint(2 * (size_t)chunk);
  double kernel_ms = 0.0;
  for (int b0 = 0; b0 < nb; b0 += chunk) {
    const int cb = std::min(chunk, nb - b0);
    KP_HIP(ctx, hipMemcpyAsync(dA, A + (size_t)b0 * nn, (size_t)cb * nn * 8, hipMemcpyHostToDevice, s));
    KP_HIP(ctx, hipEventRecord(ctx->evp[4], s));
    if (regime == 1) hipLaunchKernelGGL((kp_eig_kernel<64, true>), dim3(cb), dim3(64), lds, s, a);
    else if (regime == 2) hipLaunchKernelGGL((kp_eig_kernel<256, true>), dim3(cb), dim3(256), lds, s, a);
    else hipLaunchKernelGGL((kp_eig_kernel<256, false>), dim3(cb), dim3(256), lds, s, a);
    KP_HIP(ctx, hipGetLastError());
    KP_HIP(ctx, hipEventRecord(ctx->evp[5], s));
    KP_HIP(ctx, hipMemcpyAsync(wr + (size_t)b0 * n, a.wr, (size_t)cb * n * 8, hipMemcpyDeviceToHost, s));
    KP_HIP(ctx, hipMemcpyAsync(wi + (size_t)b0 * n, a.wi, (size_t)cb * n * 8, hipMemcpyDeviceToHost, s));
    if (vec) KP_HIP(ctx, hipMemcpyAsync(V + (size_t)b0 * nn, a.V, (size_t)cb * nn * 8, hipMemcpyDeviceToHost, s));
    KP_HIP(ctx, hipMemcpyAsync(hint.data(), a.iters, (size_t)cb * sizeof(int), hipMemcpyDeviceToHost, s));
    KP_HIP(ctx, hipMemcpyAsync(hint.data() + chunk, a.status, (size_t)cb * sizeof(int), hipMemcpyDeviceToHost, s));
    KP_HIP(ctx, hipStreamSynchronize(s));
    for (int b = 0; b < cb; ++b) {
      if (iters) iters[b0 + b] = hint[b];
      status[b0 + b] = hint[chunk + b];
    }
    float ms = 0;
    if (hipEventElapsedTime(&ms, ctx->evp[4], ctx->evp[5]) == hipSuccess) kernel_ms += ms;
  }
  ctx->timers[22] = kernel_ms;
  ctx->timers[23] = (double)regime;
  return KP_OK;
}
