// Dormand-Prince 5(4) coefficients of ode45 (arm.py _A, _B5, _E, _C) and ntrp45's BI, shared by the device integrators
// that restate arm.dopri45 / arm.ode45_span one lane per trajectory (kp_arm.hip, kp_rsys.hip).  Every index is a
// compile-time constant in the unrolled stage loops, so each call folds to a literal.
#pragma once
#include <hip/hip_runtime.h>

namespace kp_dopri {

constexpr double EPS = 2.220446049250313e-16;

// A(s, j); row 6 is B5
__device__ __forceinline__ double dp_a(int s, int j) {
  switch (s * 8 + j) {
    case 8: return 1.0 / 5;
    case 16: return 3.0 / 40;   case 17: return 9.0 / 40;
    case 24: return 44.0 / 45;  case 25: return -56.0 / 15;  case 26: return 32.0 / 9;
    case 32: return 19372.0 / 6561; case 33: return -25360.0 / 2187; case 34: return 64448.0 / 6561; case 35: return -212.0 / 729;
    case 40: return 9017.0 / 3168;  case 41: return -355.0 / 33;     case 42: return 46732.0 / 5247; case 43: return 49.0 / 176;
    case 44: return -5103.0 / 18656;
    case 48: return 35.0 / 384; case 50: return 500.0 / 1113; case 51: return 125.0 / 192;
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
__device__ __forceinline__ double dp_c(int s) {
  switch (s) {
    case 0: return 0.0; case 1: return 1.0 / 5; case 2: return 3.0 / 10; case 3: return 4.0 / 5; case 4: return 8.0 / 9;
    default: return 1.0;
  }
}
__device__ __forceinline__ double bi(int q, int c) {
  switch (q * 4 + c) {
    case 0: return 1.0; case 1: return -183.0 / 64; case 2: return 37.0 / 12; case 3: return -145.0 / 128;
    case 9: return 1500.0 / 371; case 10: return -1000.0 / 159; case 11: return 1000.0 / 371;
    case 13: return -125.0 / 32; case 14: return 125.0 / 12; case 15: return -375.0 / 64;
    case 17: return 9477.0 / 3392; case 18: return -729.0 / 106; case 19: return 25515.0 / 6784;
    case 21: return -11.0 / 7; case 22: return 11.0 / 3; case 23: return -55.0 / 28;
    case 25: return 3.0 / 2; case 26: return -4.0; case 27: return 5.0 / 2;
    default: return 0.0;
  }
}

}  // namespace kp_dopri
