// Prints the host plan of the nested sweep (csrc/kp_sweep_plan.h) for a dictionary given by its power-table recipes, host only:
//   g++ -std=c++17 -O1 -I koopman-realizations_amd/csrc -I include tools/sweep_plan_check.cpp -o sweep_plan_check
//   sweep_plan_check <model type 0|1|2> <inputs m> <variables nv> <table depth Dp> <n_deg> <recipe word> ...
// One recipe word per dictionary column (the constant last), as kp_basis_create packs them: byte f = v * Dp + e - 1 for the f-th
// variable with a non-zero exponent, 255 for none.  One line of JSON: {"error": text} for a refusal, else the plan - doubles
// with 17 digits, so that they read back bit for bit.  tests/test_sweep_plan.py runs it.
#include <cstdio>
#include <cstdlib>

#include "kp_sweep_plan.h"

int main(int argc, char** argv) {
  if (argc < 8) {
    fprintf(stderr, "usage: %s <model type 0|1|2> <m> <nv> <Dp> <n_deg> <recipe word> <recipe word> ...\n", argv[0]);
    return 2;
  }
  const int mt = atoi(argv[1]), m = atoi(argv[2]), nv = atoi(argv[3]), Dp = atoi(argv[4]), n_deg = atoi(argv[5]), Nmax = argc - 6;
  std::vector<uint32_t> rec;
  for (int c = 0; c < Nmax; ++c) rec.push_back((uint32_t)strtoul(argv[6 + c], nullptr, 0));
  // what kp_sweep_eval_nested has checked before it plans: one 16-wide tile, ids inside the power table
  const int W = mt == KP_MODEL_LINEAR ? Nmax + m : mt == KP_MODEL_BILINEAR ? Nmax * (m + 1) : Nmax;
  bool ok = mt >= 0 && mt <= 2 && m >= 0 && m <= 3 && nv >= 1 && Dp >= 1 && n_deg >= 1 && W <= 16;
  for (uint32_t r : rec)
    for (int f = 0; f < 4; ++f) {
      const uint32_t id = (r >> (8 * f)) & 255u;
      ok = ok && (id == 255u || id < (uint32_t)(nv * Dp));
    }
  if (!ok) {
    fprintf(stderr, "%s: not a dictionary the nested sweep takes (W <= 16, m <= 3, recipe ids below nv * Dp)\n", argv[0]);
    return 2;
  }
  SweepPlan P;
  if (const char* refusal = sweep_plan_build(rec.data(), Nmax, nv, Dp, mt, m, n_deg, &P)) {
    printf("{\"error\": \"%s\"}\n", refusal);
    return 0;
  }
  printf("{\"error\": null, \"dmax\": %d, \"cheb\": %s, \"deg\": [", P.dmax, P.cheb ? "true" : "false");
  for (int c = 0; c < Nmax; ++c) printf("%s%d", c ? ", " : "", P.deg[c]);
  printf("], \"ex\": [");
  for (int c = 0; c < Nmax; ++c) {
    printf("%s[", c ? ", " : "");
    for (int v = 0; v < nv; ++v) printf("%s%d", v ? ", " : "", P.ex[c][v]);
    printf("]");
  }
  printf("], \"degs\": [");
  for (int dj = 0; dj < n_deg; ++dj) {
    const SweepDeg& d = P.degs[dj];
    printf("%s{\"N\": %d, \"W\": %d, \"idx\": [", dj ? ", " : "", d.N, d.W);
    for (int q = 0; q < 16; ++q) printf("%s%d", q ? ", " : "", d.idx[q]);
    printf("], \"Sf\": [");
    for (int q = 0; q < 256; ++q) printf("%s%.17g", q ? ", " : "", d.Sf[q]);
    printf("], \"Tinv\": [");
    for (int q = 0; q < 256; ++q) printf("%s%.17g", q ? ", " : "", d.Tinv[q]);
    printf("], \"cols\": [");
    for (int q = 0; q < 16; ++q) printf("%s[%d, %d]", q ? ", " : "", P.cols[(size_t)dj * 16 + q].kind, P.cols[(size_t)dj * 16 + q].arg);
    printf("]}");
  }
  printf("]}\n");
  return 0;
}
