// Host plan of the nested sweep (kp_sweep_eval_nested, kp_sweep.hip).  No HIP here: tools/sweep_plan_check.cpp prints a plan on
// the host and tests/test_sweep_plan.py checks it without a device.
//
// All degrees of one model type from ONE pass over the data (evaluate_rand_models.m loops degree by degree, :47-143).
//  * The degree-j polynomial dictionary is a column subset of the degree-D one: def_polyLift orders the monomials by
//    total degree (Ksysid.m:645-648), so fullBasis_j = the first N_j - 1 columns of fullBasis_D plus the constant, and
//    Px_j'Px_j, Px_j'Py_j are sub-blocks of the degree-D Grams.
//  * The Grams are accumulated in a CHEBYSHEV internal basis (the data are scaled to [-1, 1], get_scale): psi_c has
//    T_e(x_v) where the monomial has x_v^e.  psi_m = S psi_c with an exactly known S (x^a = sum_b s1[a][b] T_b(x), all
//    coefficients positive: no cancellation), hence  K_m = T^-1 K_c T (T = S'),  G_m = S G_c S',  C_m = S C_c S'.
//    cond(Px_c) ~ 20-40 where cond(Px_m) ~ 1e5 for the degree-13 dictionaries, so the normal equations in the internal
//    basis give K_m to ~5e-12 of the QR solution that MATLAB's `\` (Ksysid.m:1069) returns - without the second sweep
//    over the snapshots that iterative refinement needs.
#pragma once
#include <stdint.h>
#include <cmath>
#include <utility>
#include <vector>

#include "koopman_hip.h"   // KP_MODEL_*
#include "kp_col_desc.h"

struct SweepDeg {       // one degree of the sweep, as the device reads it
  int N, W, pad0, pad1;
  int idx[16];          // column of the degree-D Px for each column of the degree-j Px
  double Sf[256];       // [r * 16 + c]: psi_m = Sf psi_c (identity on the padding)
  double Tinv[256];     // (Sf')^-1
};

struct SweepPlan {
  std::vector<std::vector<int>> ex;   // [column][variable]: exponent multi-index (the constant is all zeros)
  std::vector<int> deg;               // total degree of every column
  int dmax = 0;
  bool cheb = true;                   // the Chebyshev internal basis spans every nested dictionary (else S = I)
  std::vector<SweepDeg> degs;         // n_deg
  std::vector<ColDesc> cols;          // 16 per degree: psi_j for the rollout's lift
};

// 1-D monomial -> Chebyshev coefficients: x^a = sum_b s1[a][b] T_b(x)   (x T_b = (T_(b+1) + T_|b-1|) / 2, x T_0 = T_1)
inline void cheb_table(int dmax, std::vector<std::vector<double>>& s1) {
  s1.assign(dmax + 1, std::vector<double>(dmax + 1, 0.0));
  s1[0][0] = 1.0;
  for (int a = 0; a < dmax; ++a)
    for (int bq = 0; bq <= a; ++bq) {
      const double c = s1[a][bq];
      if (c == 0.0) continue;
      if (bq == 0) s1[a + 1][1] += c;
      else { s1[a + 1][bq + 1] += 0.5 * c; s1[a + 1][bq - 1] += 0.5 * c; }
    }
}

// The plan of degrees 1 .. n_deg of the dictionary whose Nmax power-table recipes (4 x 8-bit ids v * Dp + e - 1, 255 = none) are
// given; the widest Px must fit the 16 x 16 tile.  Returns nullptr, or the text of the refusal.
inline const char* sweep_plan_build(const uint32_t* recipes, int Nmax, int nv, int Dp, int model_type, int m, int n_deg, SweepPlan* P) {
  // exponent multi-index and total degree of every column (from the power-table recipes; the constant is all zeros)
  std::vector<std::vector<int>>& ex = P->ex;
  std::vector<int>& deg = P->deg;
  ex.assign(Nmax, std::vector<int>(nv, 0));
  deg.assign(Nmax, 0);
  for (int c = 0; c < Nmax; ++c) {
    const uint32_t r = recipes[c];
    for (int f = 0; f < 4; ++f) {
      const uint32_t id = (r >> (8 * f)) & 255u;
      if (id == 255u) continue;
      ex[c][id / Dp] += (int)(id % Dp) + 1;
    }
    for (int v = 0; v < nv; ++v) deg[c] += ex[c][v];
  }
  if (deg[Nmax - 1] != 0) return "kp_sweep_eval_nested: the last dictionary column must be the constant";
  for (int c = 0; c + 2 < Nmax; ++c)
    if (deg[c] > deg[c + 1] || deg[c] < 1) return "kp_sweep_eval_nested: monomials must be ordered by total degree";
  const int dmax = P->dmax = Nmax >= 2 ? deg[Nmax - 2] : 0;
  if (n_deg > dmax) return "kp_sweep_eval_nested: n_deg exceeds the degree of the dictionary";
  std::vector<std::vector<double>> s1;
  cheb_table(dmax, s1);
  std::vector<SweepDeg>& degs = P->degs;
  degs.assign(n_deg, SweepDeg{});
  P->cols.assign((size_t)n_deg * 16, ColDesc{COL_CONST, 0, 0, 0});
  auto cols_of_degree = [&](int j) {                 // columns of psi_D that make psi_j: degree <= j, then the constant
    std::vector<int> psi;
    for (int c = 0; c + 1 < Nmax; ++c)
      if (deg[c] <= j) psi.push_back(c);
    psi.push_back(Nmax - 1);
    return psi;
  };
  // The Chebyshev internal basis spans psi_j only if, with a monomial, every product of T_b(x_v) in its expansion (b = a, a - 2,
  // ...) is a column of psi_j too - true of the full tables of def_polyLift, not of a sparse one: [x, x^9, 1] against [T_1, T_9, 1]
  // is another dictionary and gave another K.  Such tables keep the monomials as the internal basis (S = I).
  bool cheb = true;
  for (int dj = 0; dj < n_deg && cheb; ++dj) {
    const std::vector<int> psi = cols_of_degree(dj + 1);
    for (int r : psi) {
      int terms = 1, hits = 0;
      for (int v = 0; v < nv; ++v) terms *= ex[r][v] / 2 + 1;
      for (int c : psi) {
        bool hit = true;
        for (int v = 0; v < nv; ++v) hit = hit && ex[c][v] <= ex[r][v] && ((ex[r][v] - ex[c][v]) & 1) == 0;
        hits += hit ? 1 : 0;
      }
      if (hits != terms) cheb = false;
    }
  }
  P->cheb = cheb;
  for (int dj = 0; dj < n_deg; ++dj) {
    const int j = dj + 1;
    SweepDeg& d = degs[dj];
    const std::vector<int> psi = cols_of_degree(j);
    const int Nj = (int)psi.size();
    d.N = Nj;
    d.W = model_type == KP_MODEL_LINEAR ? Nj + m : model_type == KP_MODEL_BILINEAR ? Nj * (m + 1) : Nj;
    d.pad0 = d.pad1 = 0;
    // S_psi (Nj x Nj) and its layout inside Sf
    std::vector<long double> Sp((size_t)Nj * Nj, 0.0L);
    for (int r = 0; r < Nj; ++r)
      for (int c = 0; c < Nj; ++c) {
        long double p = 1.0L;
        for (int v = 0; v < nv; ++v) {
          const int a = ex[psi[r]][v], bq = ex[psi[c]][v];
          p *= bq <= a ? (long double)s1[a][bq] : 0.0L;
        }
        Sp[(size_t)r * Nj + c] = cheb ? p : (r == c ? 1.0L : 0.0L);
      }
    std::vector<long double> Sf((size_t)256, 0.0L);
    for (int q = 0; q < 16; ++q) Sf[q * 16 + q] = 1.0L;
    for (int q = 0; q < 16; ++q) d.idx[q] = 0;
    const int nblk = model_type == KP_MODEL_BILINEAR ? m + 1 : 1;
    for (int blk = 0; blk < nblk; ++blk)
      for (int r = 0; r < Nj; ++r) {
        d.idx[blk * Nj + r] = blk * Nmax + psi[r];
        for (int c = 0; c < Nj; ++c) Sf[(size_t)(blk * Nj + r) * 16 + blk * Nj + c] = Sp[(size_t)r * Nj + c];
      }
    if (model_type == KP_MODEL_LINEAR)
      for (int i = 0; i < m; ++i) d.idx[Nj + i] = Nmax + i;
    // Tinv = (Sf')^-1 by Gauss-Jordan in extended precision (Sf is triangular up to the column order, diagonal 2^(1-deg))
    std::vector<long double> A((size_t)256), I((size_t)256, 0.0L);
    for (int r = 0; r < 16; ++r)
      for (int c = 0; c < 16; ++c) A[r * 16 + c] = Sf[c * 16 + r];
    for (int q = 0; q < 16; ++q) I[q * 16 + q] = 1.0L;
    for (int k = 0; k < 16; ++k) {
      int piv = k;
      for (int r = k + 1; r < 16; ++r)
        if (fabsl(A[r * 16 + k]) > fabsl(A[piv * 16 + k])) piv = r;
      if (A[piv * 16 + k] == 0.0L) return "kp_sweep_eval_nested: singular basis change";
      for (int c = 0; c < 16; ++c) { std::swap(A[k * 16 + c], A[piv * 16 + c]); std::swap(I[k * 16 + c], I[piv * 16 + c]); }
      const long double inv = 1.0L / A[k * 16 + k];
      for (int c = 0; c < 16; ++c) { A[k * 16 + c] *= inv; I[k * 16 + c] *= inv; }
      for (int r = 0; r < 16; ++r)
        if (r != k && A[r * 16 + k] != 0.0L) {
          const long double f = A[r * 16 + k];
          for (int c = 0; c < 16; ++c) { A[r * 16 + c] -= f * A[k * 16 + c]; I[r * 16 + c] -= f * I[k * 16 + c]; }
        }
    }
    for (int q = 0; q < 256; ++q) { d.Sf[q] = (double)Sf[q]; d.Tinv[q] = (double)I[q]; }
    // column descriptors of psi_j for the rollout's lift
    for (int r = 0; r < Nj; ++r) {
      const int c = psi[r];
      ColDesc cd{COL_CONST, 0, 0, 0};
      if (c < nv) cd = ColDesc{COL_VAR, c, 0, 0};
      else if (c + 1 < Nmax) cd = ColDesc{COL_MONO, c - nv, 0, 0};
      P->cols[(size_t)dj * 16 + r] = cd;
    }
  }
  return nullptr;
}
