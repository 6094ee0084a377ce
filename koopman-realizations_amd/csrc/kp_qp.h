// Dense strictly convex QP solvers shared by the MPC step kernels (kp_mpc.hip) and the NMPC SQP kernel (kp_nmpc.hip):
// the dual active-set iteration of Goldfarb and Idnani by one wave (qp_goldfarb_idnani) or by a whole 256-thread
// workgroup (qp_gi_wg), with the wave-level reductions they use.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "koopman_hip.h"

#define QP_MAXN 64       // variables (one wave handles <= 64)
#define QP_MAXIT 2000
#define QP_MAX_RELEASE 6   // rows a warm start may release before it is abandoned for the cold start

// ---- wave-level helpers (64 lanes): DPP inside 16-lane rows, v_readlane across the 4 rows ----
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v) {
  int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
  int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
template <int CTRL>
__device__ __forceinline__ int dpp_movi(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true);
}
__device__ __forceinline__ double lane_get(double v, int lane) {
  int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}
// quad_perm [1,0,3,2] = 0xB1, [2,3,0,1] = 0x4E, row_half_mirror = 0x141, row_mirror = 0x140
__device__ __forceinline__ double wave_sum(double v) {
  v += dpp_mov<0xB1>(v);
  v += dpp_mov<0x4E>(v);
  v += dpp_mov<0x141>(v);
  v += dpp_mov<0x140>(v);                 // every lane: sum of its 16-lane row
  return (lane_get(v, 0) + lane_get(v, 16)) + (lane_get(v, 32) + lane_get(v, 48));
}
// arg max / arg min over the wave: the extreme VALUE by a DPP reduction (2 moves + 1 v_max per step), then the first lane
// that holds it (ballot + s_ff1) hands over its index.  (Carrying (value, index) pairs through the reduction took ~12
// dependent VALU instructions per step, ~600 cycles per call; this is ~220.)  Ties go to the lowest lane.
__device__ __forceinline__ void wave_argmax(double& v, int& idx) {
  double m = v;
  m = fmax(m, dpp_mov<0xB1>(m));
  m = fmax(m, dpp_mov<0x4E>(m));
  m = fmax(m, dpp_mov<0x141>(m));
  m = fmax(m, dpp_mov<0x140>(m));
  const double w = fmax(fmax(lane_get(m, 0), lane_get(m, 16)), fmax(lane_get(m, 32), lane_get(m, 48)));
  const unsigned long long mask = __ballot(v == w);
  idx = mask ? __builtin_amdgcn_readlane(idx, __ffsll((long long)mask) - 1) : 0x7fffffff;
  v = w;
}
__device__ __forceinline__ void wave_argmin(double& v, int& idx) {
  double m = v;
  m = fmin(m, dpp_mov<0xB1>(m));
  m = fmin(m, dpp_mov<0x4E>(m));
  m = fmin(m, dpp_mov<0x141>(m));
  m = fmin(m, dpp_mov<0x140>(m));
  const double w = fmin(fmin(lane_get(m, 0), lane_get(m, 16)), fmin(lane_get(m, 32), lane_get(m, 48)));
  const unsigned long long mask = __ballot(v == w);
  idx = mask ? __builtin_amdgcn_readlane(idx, __ffsll((long long)mask) - 1) : 0x7fffffff;
  v = w;
}

// Constraint matrix in ELL form: row r has K slots (val[k*mr + r], col[k*mr + r]); unused slots
// carry val = 0, col = 0.  The MPC rows have <= 3 non-zeros, so A x, H^-1 a_p and N'H^-1 a_p cost
// K operations instead of n.
struct EllMat {
  const double* val;
  const int* col;
  const double* norm;  // row 2-norms
  int K;
};

// LDS scratch of the QP solver (doubles): Hinv n*n | HN n*n | Sinv n*n | x,hp,r,lam,d,zd,ap,f: 8n |
// act: n ints | isact: mr bytes | LDS copy of the constraint rows when K <= QP_KLDS: val mr*K, col mr*K ints, norm mr, b mr
#define QP_KLDS 4
__host__ __device__ inline int qp_lds_doubles(int n, int mr) {
  return 3 * n * n + 9 * n + 2 * ((n + 1) / 2) + (mr + 7) / 8 + 8 + mr * QP_KLDS + (mr * QP_KLDS + 1) / 2 + 2 * mr + 2 +
         64;   // (the last 64: scalar exchanges of the workgroup-wide solver)
}

// Wave-local synchronisation: LDS operations of one wave complete in issue order, so lanes only
// need the compiler not to reorder across this point (usable inside multi-wave workgroups).
#define WSYNC()                                              \
  do {                                                       \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   \
    __builtin_amdgcn_wave_barrier();                         \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   \
  } while (0)

// min 1/2 x'Hq x + f'x  s.t.  A x <= b.   Hq: n x n column-major (LDS or global).
// Executed by ONE wave (all 64 lanes must call).  Returns 0 on success, 1 on infeasible /
// iteration cap / non-SPD Hessian (x_out = NaN then).
// Warm start (warm_q > 0): the caller has put warm_q active rows into act[], the columns H^-1 a_c into HN and the
// inverse of S = N'H^-1 N into Sinv (layout below).  The multipliers of the equality-constrained minimiser are
// formed; constraints with negative multipliers are released one by one (rank-1 downdates); what remains is a
// valid dual-feasible state from which the usual iteration continues.  The optimum is unique, so the result does
// not depend on the start.  warm_out (global, 1 + n ints): the optimal active set for the next call.
__device__ __forceinline__ int qp_goldfarb_idnani(const double* Hq, const double* f, const EllMat A, const double* bvec, int n, int mr,
                                  double* ws, double* x_out, double tol, long long* stamps = nullptr, bool have_hinv = false,
                                  int hinv_bad = 0, int warm_q = 0, int* warm_out = nullptr) {
  const int lane = threadIdx.x & 63;
  double* Hinv = ws;
  double* HN = Hinv + n * n;
  double* Sinv = HN + n * n;
  double* x = Sinv + n * n;
  double* hp = x + n;
  double* r = hp + n;
  double* lam = r + n;
  double* d = lam + n;
  double* zd = d + n;
  double* ap = zd + n;
  double* fl = ap + n;
  double* apv = fl + n;                      // sparse a_p values (K <= n)
  int* apc = (int*)(apv + n);                // and columns
  int* act = apc + n + (n & 1);
  unsigned char* isact = (unsigned char*)(act + n + (n & 1));
  // constraint rows in LDS (the violation scan of every iteration reads all of them; from global memory a scan costs
  // ~3000 cycles of L2 latency)
  // (isact is 8-byte aligned.  No pointer -> integer -> pointer round trips here: they hide the LDS address space from
  // the compiler, which then emits FLAT loads and stores for the whole workspace instead of ds_read / ds_write)
  double* lval = (double*)isact + ((mr + 7) >> 3);
  double* lnorm = lval + mr * QP_KLDS;
  double* lb = lnorm + mr;
  int* lcol = (int*)(lb + mr);
  const bool ell_lds = A.K <= QP_KLDS;
  const double* Aval = A.val;
  const int* Acol = A.col;
  const double* Anorm = A.norm;
  const double* bv_ = bvec;
  if (ell_lds) {
    for (int e = lane; e < mr * A.K; e += 64) { lval[e] = A.val[e]; lcol[e] = A.col[e]; }
    for (int e = lane; e < mr; e += 64) {          // the LDS copy holds 1 / norm (0 for a null row): no division in the scan
      const double nr_ = A.norm[e];
      lnorm[e] = nr_ == 0.0 ? 0.0 : 1.0 / nr_;
      lb[e] = bvec[e];
    }
    Aval = lval; Acol = lcol; Anorm = lnorm; bv_ = lb;
  }

  // ---- Hinv by in-place Gauss-Jordan (SPD: no pivoting) ----
  if (!have_hinv)
    for (int e = lane; e < n * n; e += 64) Hinv[e] = Hq[e];
  for (int e = lane; e < n; e += 64) {
    fl[e] = f[e];
    ap[e] = 0.0;
  }
  for (int e = lane; e < mr; e += 64) isact[e] = 0;
  WSYNC();
  for (int c = lane; c < warm_q; c += 64) isact[act[c]] = 1;
  WSYNC();
  int bad = hinv_bad;
  for (int k = 0; k < (have_hinv ? 0 : n); ++k) {
    const double piv = Hinv[k + k * n];
    if (!(piv > 0.0)) bad = 1;
    const double ip = 1.0 / piv;
    // each lane owns rows i = lane (n <= 64): read its column-k entry once, then update the row
    const int i = lane;
    double cik = 0.0;
    if (i < n) cik = Hinv[i + k * n];
    WSYNC();
    if (i < n && i != k) {
      const double fct = cik * ip;
#pragma unroll 4
      for (int j = 0; j < n; ++j) {
        if (j != k) Hinv[i + j * n] -= fct * Hinv[k + j * n];
      }
      Hinv[i + k * n] = -fct;
    }
    WSYNC();
    if (i < n && i != k) Hinv[k + i * n] *= ip;   // row k (read by everyone above, scaled after)
    if (lane == 0) Hinv[k + k * n] = ip;
    WSYNC();
  }
  for (int i = lane; i < n; i += 64) {
    double s = 0.0;
#pragma unroll 4
    for (int j = 0; j < n; ++j) s += Hinv[i + j * n] * fl[j];
    x[i] = -s;
  }
  WSYNC();

  if (stamps && lane == 0) stamps[4] = wall_clock64();
#ifdef KP_QP_PROF
  long long qpt[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, qlast = clock64();
#define QP_TICK(i) do { long long tn_ = clock64(); qpt[i] += tn_ - qlast; qlast = tn_; } while (0)
#else
#define QP_TICK(i) do { } while (0)
#endif
  int q = 0;
  int status = 1;
  int it = bad ? QP_MAXIT : 0;   // non-SPD Hessian: report failure
  // remove active constraint l: swap with the last entry (symmetric permutation of Sinv, column swap of HN), then one
  // rank-1 downdate of the leading block deletes the LAST index of the inverse Schur complement
  auto drop_active = [&](int l) {
    const int last = q - 1;
    if (l != last) {
      if (lane < q) {                       // columns l <-> last (lane = row)
        const double a_ = Sinv[lane + l * n], b_ = Sinv[lane + last * n];
        Sinv[lane + l * n] = b_;
        Sinv[lane + last * n] = a_;
      }
      WSYNC();
      if (lane < q) {                       // rows l <-> last (lane = column)
        const double a_ = Sinv[l + lane * n], b_ = Sinv[last + lane * n];
        Sinv[l + lane * n] = b_;
        Sinv[last + lane * n] = a_;
      }
      for (int i = lane; i < n; i += 64) {
        const double a_ = HN[i + l * n];
        HN[i + l * n] = HN[i + last * n];
        HN[i + last * n] = a_;
      }
      if (lane == 0) {
        const int ta = act[l]; act[l] = act[last]; act[last] = ta;
        const double tl = lam[l]; lam[l] = lam[last]; lam[last] = tl;
      }
      WSYNC();
    }
    const double isl = 1.0 / Sinv[last + last * n];
    if (lane < last) {
      const double ri = Sinv[lane + last * n] * isl;
      // four columns at a time, every read before the first write: the compiler cannot tell the read-modify-write of
      // column j from the reads of column j + 1 (same LDS array) and would otherwise pay one LDS round trip per column
      int j = 0;
      for (; j + 4 <= last; j += 4) {
        const double a0 = Sinv[lane + j * n], a1 = Sinv[lane + (j + 1) * n], a2 = Sinv[lane + (j + 2) * n], a3 = Sinv[lane + (j + 3) * n];
        const double r0 = Sinv[last + j * n], r1 = Sinv[last + (j + 1) * n], r2 = Sinv[last + (j + 2) * n], r3 = Sinv[last + (j + 3) * n];
        Sinv[lane + j * n] = a0 - ri * r0;
        Sinv[lane + (j + 1) * n] = a1 - ri * r1;
        Sinv[lane + (j + 2) * n] = a2 - ri * r2;
        Sinv[lane + (j + 3) * n] = a3 - ri * r3;
      }
      for (; j < last; ++j) Sinv[lane + j * n] -= ri * Sinv[last + j * n];
    }
    if (lane == 0) isact[act[last]] = 0;
    --q;
    WSYNC();
  };
  if (warm_q > 0 && !bad) {
    q = warm_q;
    int n_rel = 0;
    while (q > 0) {
      // lam = Sinv (N x0 - b)
      for (int c = lane; c < q; c += 64) {
        const int row = act[c];
        double v = -bv_[row];
        for (int k = 0; k < A.K; ++k) v += Aval[k * mr + row] * x[Acol[k * mr + row]];
        d[c] = v;
      }
      WSYNC();
      double lmin = 1e300;
      int l = 0x7fffffff;
      for (int c = lane; c < q; c += 64) {
        double s_ = 0.0;
#pragma unroll 4
        for (int k = 0; k < q; ++k) s_ += Sinv[c + k * n] * d[k];
        lam[c] = s_;
        lmin = s_;
        l = c;
      }
      wave_argmin(lmin, l);
      WSYNC();
      if (!(lmin < 0.0)) break;             // dual feasible
      // Every release is a rank-1 downdate of the inverse Schur complement, and their errors accumulate.  A set that
      // needs more than a few is not the neighbourhood a warm start is for (another reference, another state): give
      // it up - the cold start is exact - instead of iterating on a degraded inverse.
      if (++n_rel > QP_MAX_RELEASE) {
        for (int c = lane; c < q; c += 64) isact[act[c]] = 0;
        q = 0;
        break;
      }
      drop_active(l);
    }
    // x = x0 - H^-1 N lam
    for (int i = lane; i < n; i += 64) {
      double s_ = x[i];
#pragma unroll 4
      for (int c = 0; c < q; ++c) s_ -= HN[i + c * n] * lam[c];
      x[i] = s_;
    }
    WSYNC();
  }
  while (it < QP_MAXIT) {
    ++it;
    // most violated inactive constraint (scaled by the row norm)
    double best = -1e300;
    int bestp = 0x7fffffff;
    int infeas = 0;
    // branch-free, two rows per lane at a time: every LDS read of both rows is issued unconditionally and before any
    // arithmetic (a `continue` or a guarded isact read makes the compiler wait for each read in turn; one row after the
    // other doubles the col -> x[col] dependent chain), the rows are then taken or not by selects
    for (int row0 = lane; row0 < mr; row0 += 128) {
      const int rowA = row0, rowB = row0 + 64;
      const bool inB = rowB < mr;
      const int rB = inB ? rowB : rowA;
      double vA = -bv_[rowA], vB = -bv_[rB];
      const double nA = Anorm[rowA], nB = Anorm[rB];
      const int actA = isact[rowA], actB = isact[rB];
      for (int k = 0; k < A.K; ++k) {
        const int cA = Acol[k * mr + rowA], cB = Acol[k * mr + rB];
        const double aA = Aval[k * mr + rowA], aB = Aval[k * mr + rB];
        vA += aA * x[cA];
        vB += aB * x[cB];
      }
      const double iA = ell_lds ? nA : (nA == 0.0 ? 0.0 : 1.0 / nA);
      const double iB = ell_lds ? nB : (nB == 0.0 ? 0.0 : 1.0 / nB);
      const double sA = vA * iA, sB = vB * iB;
      infeas |= ((iA == 0.0 && vA > tol) || (inB && iB == 0.0 && vB > tol)) ? 1 : 0;
      const bool takeA = iA != 0.0 && !actA && sA > best;
      best = takeA ? sA : best;
      bestp = takeA ? rowA : bestp;
      const bool takeB = inB && iB != 0.0 && !actB && sB > best;
      best = takeB ? sB : best;
      bestp = takeB ? rowB : bestp;
    }
    wave_argmax(best, bestp);
    QP_TICK(0);
    infeas = __any(infeas);
    if (infeas) break;
    if (best <= tol) {
      status = 0;
      break;
    }
    const int p = bestp;
    const double bp = bv_[p];
    // sparse a_p: (col_k, val_k), k < K, staged in LDS (apv/apc) for the loops below; dense copy in ap
    if (lane < A.K) {
      double v = Aval[lane * mr + p];
      int cidx = Acol[lane * mr + p];
      apv[lane] = v;
      apc[lane] = cidx;
      if (v != 0.0) ap[cidx] = v;
    }
    WSYNC();
    double app_l = 0.0;
    for (int i = lane; i < n; i += 64) {
      double s = 0.0;
      for (int k = 0; k < A.K; ++k) s += apv[k] * Hinv[i + apc[k] * n];
      hp[i] = s;
      app_l += s * ap[i];
    }
    const double app = wave_sum(app_l);
    WSYNC();
    QP_TICK(1);
    double lam_p = 0.0;
    bool fail = false;
    while (it < QP_MAXIT) {
      ++it;
      // d = N' Hinv a_p ; r = Sinv d ; zd = hp - HN r
      for (int c = lane; c < q; c += 64) {
        double s = 0.0;
        for (int k = 0; k < A.K; ++k) s += apv[k] * HN[apc[k] + c * n];
        d[c] = s;
      }
      WSYNC();
      QP_TICK(6);
      for (int c = lane; c < q; c += 64) {
        double s = 0.0;
#pragma unroll 8
        for (int k = 0; k < q; ++k) s += Sinv[c + k * n] * d[k];
        r[c] = s;
      }
      WSYNC();
      QP_TICK(7);
      double apz_l = 0.0, apx_l = 0.0;
      for (int i = lane; i < n; i += 64) {
        double s = hp[i];
#pragma unroll 8
        for (int c = 0; c < q; ++c) s -= HN[i + c * n] * r[c];
        zd[i] = s;
        apz_l += ap[i] * s;
        apx_l += ap[i] * x[i];
      }
      QP_TICK(8);
      const double apz = wave_sum(apz_l);
      const double apx = wave_sum(apx_l);
      QP_TICK(9);
      double t1 = 1e300;
      int l = 0x7fffffff;
      for (int c = lane; c < q; c += 64) {
        if (r[c] > 1e-13) {
          double ratio = lam[c] / r[c];
          if (ratio < t1) {
            t1 = ratio;
            l = c;
          }
        }
      }
      wave_argmin(t1, l);
      QP_TICK(2);
      const bool t2fin = apz > 1e-13 * app;
      const double t2 = t2fin ? (apx - bp) / apz : 1e300;
      const double t = fmin(t1, t2);
      if (!(t < 1e299)) {
        fail = true;
        break;
      }
      WSYNC();
      for (int c = lane; c < q; c += 64) lam[c] -= t * r[c];
      lam_p += t;
      if (t2fin)
        for (int i = lane; i < n; i += 64) x[i] -= t * zd[i];
      WSYNC();
      QP_TICK(3);
      if (t2 <= t1) {
        // add p: Sinv <- bordered inverse with w = r, beta = apz (Schur complement)
        if (q >= n) {
          fail = true;
          break;
        }
        const double ib = 1.0 / apz;
        if (lane < q) {                         // lane i owns row i (q <= n <= 64): no index arithmetic
          const double ri = r[lane] * ib;
          int j = 0;
          for (; j + 4 <= q; j += 4) {           // reads before writes, as in drop_active
            const double a0 = Sinv[lane + j * n], a1 = Sinv[lane + (j + 1) * n], a2 = Sinv[lane + (j + 2) * n], a3 = Sinv[lane + (j + 3) * n];
            const double r0 = r[j], r1 = r[j + 1], r2 = r[j + 2], r3 = r[j + 3];
            Sinv[lane + j * n] = a0 + ri * r0;
            Sinv[lane + (j + 1) * n] = a1 + ri * r1;
            Sinv[lane + (j + 2) * n] = a2 + ri * r2;
            Sinv[lane + (j + 3) * n] = a3 + ri * r3;
          }
          for (; j < q; ++j) Sinv[lane + j * n] += ri * r[j];
        }
        for (int c = lane; c < q; c += 64) {
          Sinv[c + q * n] = -r[c] * ib;
          Sinv[q + c * n] = -r[c] * ib;
        }
        for (int i = lane; i < n; i += 64) HN[i + q * n] = hp[i];
        if (lane == 0) {
          Sinv[q + q * n] = ib;
          act[q] = p;
          lam[q] = lam_p;
          isact[p] = 1;
        }
        ++q;
        WSYNC();
        QP_TICK(4);
        break;
      }
      // partial step: drop active constraint l (swap-with-last rank-1 downdate, no compaction sweeps)
      {
        drop_active(l);
        QP_TICK(5);
      }
    }
    // clear the dense copy of a_p
    if (lane < A.K) ap[apc[lane]] = 0.0;
    WSYNC();
    if (fail) break;
  }
  WSYNC();
  if (stamps && lane == 0) {
    stamps[8] = it;
    stamps[9] = q;
  }
#ifdef KP_QP_PROF
  if (stamps && lane == 0)
    printf("qp prof (cycles): scan+argmax %lld  a_p/hp %lld  ratios %lld  step %lld  add(border) %lld  drop %lld | d %lld r %lld zd %lld sums %lld  it %d q %d\n",
           qpt[0], qpt[1], qpt[2], qpt[3], qpt[4], qpt[5], qpt[6], qpt[7], qpt[8], qpt[9], it, q);
#endif
  for (int i = lane; i < n; i += 64) x_out[i] = status == 0 ? x[i] : __builtin_nan("");
  if (warm_out) {                            // optimal active set: the start of the next call
    if (lane == 0) warm_out[0] = status == 0 ? q : 0;
    for (int c = lane; c < q; c += 64) warm_out[1 + c] = act[c];
  }
  return status;
}

// ---- the same dual active-set iteration by the WHOLE workgroup (256 threads) ----------------------------------------------
// For n <= 32 variables with the constraint rows in LDS (K <= QP_KLDS) and H^-1 already formed by the caller.  One wave
// spends an iteration in dependent chains: a 30-term dot product per lane (r = S^-1 d, z = hp - HN r), 30 columns of the
// bordering update per lane, two rows of the violation scan per lane.  Here every such loop is two-dimensional:
//   * matrix-vector products: 8 adjacent lanes share a row and split the columns (4 terms each), summed by DPP
//     (quad_perm x2 + row_half_mirror);
//   * bordering / removal updates of S^-1: thread (i = tid & 31, j = tid >> 5, +8, ..) owns elements, no chains at all;
//   * violation scan: one row per thread;
// and the few scalars that steer the iteration (most violated row, step lengths) go through LDS: each wave reduces, lane 0
// stores, barrier, every thread combines the four entries in the same order - the control flow is uniform.
// Same algorithm, thresholds and data layout as qp_goldfarb_idnani (the products are summed in another order: results
// agree to rounding).  ~10 barriers per iteration.  red: 64 doubles of LDS for the exchanges.
struct WgX {
  double* v;
  int* i;
};
__device__ __forceinline__ void wgx_argmax(double& v, int& idx, WgX x) {
  wave_argmax(v, idx);
  if ((threadIdx.x & 63) == 0) { x.v[threadIdx.x >> 6] = v; x.i[threadIdx.x >> 6] = idx; }
  __syncthreads();
  double b = x.v[0];
  int bi = x.i[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) {
    const double c = x.v[w];
    const int ci = x.i[w];
    if (c > b) { b = c; bi = ci; }
  }
  v = b; idx = bi;
}
__device__ __forceinline__ void wgx_argmin(double& v, int& idx, WgX x) {
  wave_argmin(v, idx);
  if ((threadIdx.x & 63) == 0) { x.v[threadIdx.x >> 6] = v; x.i[threadIdx.x >> 6] = idx; }
  __syncthreads();
  double b = x.v[0];
  int bi = x.i[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) {
    const double c = x.v[w];
    const int ci = x.i[w];
    if (c < b) { b = c; bi = ci; }
  }
  v = b; idx = bi;
}
// two sums at once (a over x.v[0..4), b over x.v[4..8))
__device__ __forceinline__ void wgx_sum2(double& a, double& b, WgX x) {
  a = wave_sum(a);
  b = wave_sum(b);
  if ((threadIdx.x & 63) == 0) { x.v[threadIdx.x >> 6] = a; x.v[4 + (threadIdx.x >> 6)] = b; }
  __syncthreads();
  a = (x.v[0] + x.v[1]) + (x.v[2] + x.v[3]);
  b = (x.v[4] + x.v[5]) + (x.v[6] + x.v[7]);
}
__device__ __forceinline__ double sum8(double v) {      // over the 8 adjacent lanes of an aligned group, in every lane
  v += dpp_mov<0xB1>(v);
  v += dpp_mov<0x4E>(v);
  v += dpp_mov<0x141>(v);
  return v;
}

__device__ __forceinline__ int qp_gi_wg(const double* f, const EllMat A, const double* bvec, int n, int mr, double* ws, double* red,
                                        double* x_out, double tol, long long* stamps, int hinv_bad, int warm_q, int* warm_out) {
  const int tid = threadIdx.x;
  double* Hinv = ws;
  double* HN = Hinv + n * n;
  double* Sinv = HN + n * n;
  double* x = Sinv + n * n;
  double* hp = x + n;
  double* r = hp + n;
  double* lam = r + n;
  double* d = lam + n;
  double* zd = d + n;
  double* ap = zd + n;
  double* fl = ap + n;
  double* apv = fl + n;
  int* apc = (int*)(apv + n);
  int* act = apc + n + (n & 1);
  unsigned char* isact = (unsigned char*)(act + n + (n & 1));
  double* lval = (double*)isact + ((mr + 7) >> 3);
  double* lnorm = lval + mr * QP_KLDS;
  double* lb = lnorm + mr;
  int* lcol = (int*)(lb + mr);
  // exchange areas (distinct per reduction site: a site is not reached again before every thread has read it)
  WgX xs{red, (int*)(red + 4)}, xr{red + 8, (int*)(red + 12)}, xq{red + 16, (int*)(red + 28)}, xw{red + 32, (int*)(red + 36)};
  const int K = A.K;
  for (int e = tid; e < mr * K; e += 256) { lval[e] = A.val[e]; lcol[e] = A.col[e]; }
  for (int e = tid; e < mr; e += 256) {
    const double nr_ = A.norm[e];
    lnorm[e] = nr_ == 0.0 ? 0.0 : 1.0 / nr_;
    lb[e] = bvec[e];
    isact[e] = 0;
  }
  for (int e = tid; e < n; e += 256) {
    fl[e] = f[e];
    ap[e] = 0.0;
  }
  __syncthreads();
  for (int c = tid; c < warm_q; c += 256) isact[act[c]] = 1;
  // x = -Hinv f : row i = tid >> 3, the 8 lanes of a group split the columns
  const int gi = tid >> 3, gp = tid & 7;
  {
    double s_ = 0.0;
    if (gi < n)
      for (int j = gp; j < n; j += 8) s_ += Hinv[gi + j * n] * fl[j];
    s_ = sum8(s_);
    if (gi < n && gp == 0) x[gi] = -s_;
  }
  __syncthreads();
  if (stamps && tid == 0) stamps[4] = wall_clock64();
  int q = 0;
  int status = 1;
  int it = hinv_bad ? QP_MAXIT : 0;
  // r_out[c] = sum_k M[c + k n] v[k], c < rows, k < cols   (all threads; caller places the barrier)
  auto matvec = [&](const double* M, const double* v, int rows, int cols, double* out) {
    double s_ = 0.0;
    if (gi < rows)
      for (int k = gp; k < cols; k += 8) s_ += M[gi + k * n] * v[k];
    s_ = sum8(s_);
    if (gi < rows && gp == 0) out[gi] = s_;
  };
  // removal of active constraint l: swap with the last one, then the rank-1 downdate that deletes the last index
  auto drop_active = [&](int l) {
    const int last = q - 1;
    if (l != last) {
      if (tid < q) {                                  // columns l <-> last
        const double a_ = Sinv[tid + l * n], b_ = Sinv[tid + last * n];
        Sinv[tid + l * n] = b_;
        Sinv[tid + last * n] = a_;
      }
      if (tid >= 64 && tid < 64 + n) {                // (another wave) columns of HN
        const int i = tid - 64;
        const double a_ = HN[i + l * n];
        HN[i + l * n] = HN[i + last * n];
        HN[i + last * n] = a_;
      }
      if (tid == 128) {
        const int ta = act[l]; act[l] = act[last]; act[last] = ta;
        const double tl = lam[l]; lam[l] = lam[last]; lam[last] = tl;
      }
      __syncthreads();
      if (tid < q) {                                  // rows l <-> last
        const double a_ = Sinv[l + tid * n], b_ = Sinv[last + tid * n];
        Sinv[l + tid * n] = b_;
        Sinv[last + tid * n] = a_;
      }
      __syncthreads();
    }
    const double isl = wg_recip(Sinv[last + last * n]);
    {
      const int i = tid & 31;
      if (i < last) {
        const double ri = Sinv[i + last * n] * isl;
        for (int j = tid >> 5; j < last; j += 8) Sinv[i + j * n] -= ri * Sinv[last + j * n];
      }
    }
    if (tid == 0) isact[act[last]] = 0;
    --q;
    __syncthreads();
  };
  if (warm_q > 0 && !hinv_bad) {
    q = warm_q;
    int n_rel = 0;
    while (q > 0) {
      if (tid < q) {
        const int row = act[tid];
        double v = -lb[row];
        for (int k = 0; k < K; ++k) v += lval[k * mr + row] * x[lcol[k * mr + row]];
        d[tid] = v;
      }
      __syncthreads();
      matvec(Sinv, d, q, q, lam);
      __syncthreads();
      double lmin = tid < q ? lam[tid] : 1e300;
      int l = tid < q ? tid : 0x7fffffff;
      wgx_argmin(lmin, l, xw);
      if (!(lmin < 0.0)) break;
      if (++n_rel > QP_MAX_RELEASE) {
        if (tid < q) isact[act[tid]] = 0;
        q = 0;
        break;
      }
      drop_active(l);
    }
    // x = x0 - HN lam
    {
      double s_ = 0.0;
      if (gi < n)
        for (int c = gp; c < q; c += 8) s_ += HN[gi + c * n] * lam[c];
      s_ = sum8(s_);
      __syncthreads();
      if (gi < n && gp == 0) x[gi] -= s_;
    }
    __syncthreads();
  }
  while (it < QP_MAXIT) {
    ++it;
    // ---- most violated inactive constraint ----
    double best = -1e300;
    int bestp = 0x7fffffff;
    int infeas = 0;
    for (int row = tid; row < mr; row += 256) {
      double v = -lb[row];
      for (int k = 0; k < K; ++k) v += lval[k * mr + row] * x[lcol[k * mr + row]];
      const double in_ = lnorm[row];
      const double sv_ = v * in_;
      infeas |= (in_ == 0.0 && v > tol) ? 1 : 0;
      if (in_ != 0.0 && !isact[row] && sv_ > best) { best = sv_; bestp = row; }
    }
    infeas = __any(infeas);
    if ((tid & 63) == 0) xs.i[4 + (tid >> 6)] = infeas;     // rides on the barrier of the arg max
    wgx_argmax(best, bestp, xs);
    infeas = xs.i[4] | xs.i[5] | xs.i[6] | xs.i[7];
    if (infeas) break;
    if (best <= tol) {
      status = 0;
      break;
    }
    const int p = bestp;
    const double bp = lb[p];
    if (tid < K) {
      const double v = lval[tid * mr + p];
      const int cidx = lcol[tid * mr + p];
      apv[tid] = v;
      apc[tid] = cidx;
      if (v != 0.0) ap[cidx] = v;
    }
    __syncthreads();
    double app = 0.0;
    if (tid < n) {                                   // (n <= 32: wave 0 alone holds the terms of a_p'H^-1 a_p)
      double s_ = 0.0;
      for (int k = 0; k < K; ++k) s_ += apv[k] * Hinv[tid + apc[k] * n];
      hp[tid] = s_;
      app = s_ * ap[tid];
    }
    if (tid < 64) {
      app = wave_sum(app);
      if (tid == 0) xq.v[0] = app;
    }
    __syncthreads();                                 // (also publishes hp)
    app = xq.v[0];
    double lam_p = 0.0;
    bool fail = false;
    while (it < QP_MAXIT) {
      ++it;
      if (tid < q) {
        double s_ = 0.0;
        for (int k = 0; k < K; ++k) s_ += apv[k] * HN[apc[k] + tid * n];
        d[tid] = s_;
      }
      __syncthreads();
      matvec(Sinv, d, q, q, r);
      __syncthreads();
      // zd = hp - HN r ; a_p'zd ; a_p'x
      double apz = 0.0, apx = 0.0;
      {
        double s_ = 0.0;
        if (gi < n)
          for (int c = gp; c < q; c += 8) s_ += HN[gi + c * n] * r[c];
        s_ = sum8(s_);
        if (gi < n && gp == 0) {
          const double z_ = hp[gi] - s_;
          zd[gi] = z_;
          apz = ap[gi] * z_;
          apx = ap[gi] * x[gi];
        }
      }
      wgx_sum2(apz, apx, xr);                       // (publishes zd)
      double t1 = 1e300;
      int l = 0x7fffffff;
      if (tid < q && r[tid] > 1e-13) {
        t1 = lam[tid] * wg_recip(r[tid]);
        l = tid;
      }
      wgx_argmin(t1, l, xw);
      const bool t2fin = apz > 1e-13 * app;
      const double t2 = t2fin ? (apx - bp) * wg_recip(apz) : 1e300;
      const double t = fmin(t1, t2);
      if (!(t < 1e299)) {
        fail = true;
        break;
      }
      if (tid < q) lam[tid] -= t * r[tid];
      lam_p += t;
      if (t2fin && tid >= 64 && tid < 64 + n) x[tid - 64] -= t * zd[tid - 64];
      __syncthreads();
      if (t2 <= t1) {
        if (q >= n) {
          fail = true;
          break;
        }
        const double ib = wg_recip(apz);
        {
          const int i = tid & 31;
          if (i < q) {
            const double ri = r[i] * ib;
            for (int j = tid >> 5; j < q; j += 8) Sinv[i + j * n] += ri * r[j];
          }
        }
        if (tid < q) {
          Sinv[tid + q * n] = -r[tid] * ib;
          Sinv[q + tid * n] = -r[tid] * ib;
        }
        if (tid >= 64 && tid < 64 + n) HN[tid - 64 + q * n] = hp[tid - 64];
        if (tid == 128) {
          Sinv[q + q * n] = ib;
          act[q] = p;
          lam[q] = lam_p;
          isact[p] = 1;
        }
        ++q;
        __syncthreads();
        break;
      }
      drop_active(l);
    }
    if (tid < K) ap[apc[tid]] = 0.0;
    __syncthreads();
    if (fail) break;
  }
  if (stamps && tid == 0) {
    stamps[8] = it;
    stamps[9] = q;
  }
  for (int i = tid; i < n; i += 256) x_out[i] = status == 0 ? x[i] : __builtin_nan("");
  if (warm_out) {
    if (tid == 0) warm_out[0] = status == 0 ? q : 0;
    for (int c = tid; c < q; c += 256) warm_out[1 + c] = act[c];
  }
  return status;
}
