// Host plan of the dictionary lift (kp_lift_kernel, kp_context.hip) and the digit packing of fourier columns (kp_basis_create).
// No HIP here: tools/lift_plan_check.cpp prints both on the host and tests/test_lift_plan.py checks them without a device.
//
//  * The launch plan: points per workgroup (64 when the batch gives every CU several workgroups and 64 points' staging fits the
//    LDS, else 16), the dynamic LDS bytes, whether the column descriptors are staged beside the points (stage_cols bit 0) and
//    whether the kernel's fourier-only loop serves the dictionary (bit 1); or the refusal.
//  * The packing: the mixed-radix digits of a fourier function's index (def_fourierLift, Ksysid.m:694-731: digit of variable v =
//    harmonic of x_v, 0 none, 2j - 1 cos, 2j sin; last variable fastest), four bits per variable in ColDesc::pad when they fit.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "kp_col_desc.h"

constexpr size_t KP_LIFT_LDS_BYTES = 160 * 1024;

struct LiftPlan {
  int lt = 0;                     // points per workgroup: 64 or 16
  size_t lds = 0;                 // dynamic LDS bytes of the launch
  int stage_cols = 0;             // bit 0: descriptors staged in LDS; bit 1: the fourier-only loop of the kernel
  const char* refusal = nullptr;  // nullptr, or the text of the refusal (lt and lds are then what was refused)
};

// LDS layout of the kernel per point: vars[nvars] | um[max(m, 1)] | trig[nvars][1 + 2 fourier_degree] | full[nfull] (only with a pcs projection)
inline LiftPlan lift_plan_build(int nvars, int m, int nfull, int k_pcs, int fourier_degree, bool pure_fourier, int64_t rows, int num_cu) {
  LiftPlan P;
  const int fdeg = fourier_degree;
  const size_t per_point = (size_t)(nvars + (m > 0 ? m : 1) + nvars * (fdeg > 0 ? 2 * fdeg + 1 : 0) + (k_pcs ? nfull : 0)) * 8;
  // 64 points per workgroup when that still gives every CU several workgroups (the kernel is bound by instruction issue: one
  // workgroup per CU is one wave per SIMD, a quarter of what a SIMD can issue), else 16
  const int ncu_ = num_cu > 0 ? num_cu : 256;
  P.lt = (per_point * 64 <= KP_LIFT_LDS_BYTES && rows >= (int64_t)64 * 4 * ncu_) ? 64 : 16;
  P.lds = per_point * P.lt;
  if (P.lds > KP_LIFT_LDS_BYTES) {
    P.refusal = "kp_lift: dictionary too large for the LDS staging of the pcs projection";
    return P;
  }
  P.stage_cols = P.lds + (size_t)nfull * sizeof(ColDesc) <= KP_LIFT_LDS_BYTES ? 1 : 0;
  if (P.stage_cols) P.lds += (size_t)nfull * sizeof(ColDesc);
  if (P.stage_cols && pure_fourier && fdeg > 0 && nvars <= 8) P.stage_cols |= 2;
  return P;
}

// ColDesc::pad of fourier function `index` (>= 1) of a block of `degree` on nvars variables: the digits of the mixed-radix index
// four bits each (variable v in bits 4 v .. 4 v + 3), or 0 when they do not fit (more than 8 variables, radix above 16).  The lift
// kernel then shifts instead of dividing - twelve 32-bit integer divisions per function and point were ~200 of the ~300
// instructions of a fourier value.
inline uint32_t lift_fourier_pad(int index, int degree, int nvars) {
  uint32_t pk = 0;
  if (nvars <= 8 && 2 * degree + 1 <= 16) {
    int idx = index;
    for (int v = nvars - 1; v >= 0; --v) {
      pk |= (uint32_t)(idx % (2 * degree + 1)) << (4 * v);
      idx /= 2 * degree + 1;
    }
  }
  return pk;
}

// The columns of one fourier block: functions 1 .. total - 1 of the (2 degree + 1)^nvars products (function 0 is the constant)
inline void lift_fourier_append(std::vector<ColDesc>& cols, int degree, int nvars, int total) {
  for (int i = 1; i < total; ++i) cols.push_back({COL_FOURIER, i, degree, (int32_t)lift_fourier_pad(i, degree, nvars)});
}

// What the lift kernel is told about the fourier columns of a dictionary (its first nvars columns are the variables):
//  * fourier_degree: the degree of its fourier blocks when they share one of at most 8 - the kernel then forms the harmonics
//    once per (point, variable); 0: none, or blocks of different degrees, or a degree above 8 (generic evaluation);
//  * pure_fourier: every column behind the variables is the constant or a fourier function of that degree with packed digits.
inline void lift_fourier_flags(const std::vector<ColDesc>& cols, int nvars, int* fourier_degree, bool* pure_fourier) {
  int fourier_deg = 0;
  for (const ColDesc& c : cols)
    if (c.kind == COL_FOURIER) fourier_deg = fourier_deg == 0 ? c.aux : (fourier_deg == c.aux ? c.aux : -1);
  const int fdeg = (fourier_deg > 0 && fourier_deg <= 8) ? fourier_deg : 0;
  bool pure = fdeg > 0 && (int)cols.size() > nvars;
  for (size_t c = (size_t)nvars; c < cols.size() && pure; ++c)
    pure = cols[c].kind == COL_CONST || (cols[c].kind == COL_FOURIER && cols[c].pad != 0 && cols[c].aux == fdeg);
  *fourier_degree = fdeg;
  *pure_fourier = pure;
}
