// What the workgroup-wide ode45 kernels share (kp_ct_rollout.hip, kp_validate_ct.hip): the Dormand-Prince 5(4) tableau, the
// workgroup max of the error norm and the constants of the step control.  The per-lane integrator of the arm and the random
// systems is kp_dopri45.h.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int CT_MAX_ATTEMPTS = 100000;   // steps (accepted + rejected) per sample interval
constexpr double CT_EPS = 2.220446049250313e-16;

// Dormand-Prince 5(4) tableau (arm.py)
__device__ __forceinline__ double dp_a(int s, int j) {
  switch (s * 8 + j) {
    case 8: return 1.0 / 5;
    case 16: return 3.0 / 40;   case 17: return 9.0 / 40;
    case 24: return 44.0 / 45;  case 25: return -56.0 / 15;  case 26: return 32.0 / 9;
    case 32: return 19372.0 / 6561; case 33: return -25360.0 / 2187; case 34: return 64448.0 / 6561; case 35: return -212.0 / 729;
    case 40: return 9017.0 / 3168;  case 41: return -355.0 / 33;     case 42: return 46732.0 / 5247; case 43: return 49.0 / 176;
    case 44: return -5103.0 / 18656;
    case 48: return 35.0 / 384; case 49: return 0.0; case 50: return 500.0 / 1113; case 51: return 125.0 / 192;
    case 52: return -2187.0 / 6784; case 53: return 11.0 / 84;
    default: return 0.0;
  }
}
__device__ __forceinline__ double dp_e(int j) {
  switch (j) {
    case 0: return 71.0 / 57600; case 1: return 0.0; case 2: return -71.0 / 16695; case 3: return 71.0 / 1920;
    case 4: return -17253.0 / 339200; case 5: return 22.0 / 525; default: return -1.0 / 40;
  }
}

__device__ __forceinline__ double ct_max(double a, double b) { return (b > a || b != b) ? b : a; }

// workgroup max (NaN wins); red: two alternating slots of 8 doubles, `flip` toggled by the caller
__device__ __forceinline__ double ct_block_max(double v, double* red, int& flip) {
  for (int off = 32; off > 0; off >>= 1) v = ct_max(v, __shfl_xor(v, off));
  const int nw = blockDim.x >> 6;
  double* r = red + 8 * flip;
  flip ^= 1;
  if (nw == 1) return v;
  if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = v;
  __syncthreads();
  double m = r[0];
  for (int w = 1; w < nw; ++w) m = ct_max(m, r[w]);
  return m;
}

}  // namespace
