// Column descriptors of a dictionary's full basis.  No HIP here: host-only plan code (kp_sweep_plan.h) fills them too.
#pragma once
#include <stdint.h>

// Column kinds of the full basis (device table, one entry per full-basis column)
enum : int { COL_VAR = 0, COL_MONO = 1, COL_FOURIER = 2, COL_GAUSS = 3, COL_CONST = 4, COL_HERMITE = 5, COL_FSPARSE = 6 };

struct ColDesc {
  int32_t kind;
  int32_t arg;  // VAR: variable index; MONO/HERMITE: row in exps; FSPARSE: first of two rows in exps (sin, cos
                // multipliers); FOURIER: mixed-radix index (>=1); GAUSS: centre
  int32_t aux;  // FOURIER: degree; MONO with <= 8 variables (kp_basis_create): exponent bytes of variables 0-3
  int32_t pad;  // MONO with <= 8 variables: exponent bytes of variables 4-7; FOURIER (<= 8 variables, degree <= 7): the digits of the
                // mixed-radix index, four bits per variable (0: not packed)
};
