// Prints the host plan of the dictionary lift (csrc/kp_lift_plan.h) for a dictionary and a batch given by their sizes, host only:
//   g++ -std=c++17 -O1 -I koopman-realizations_amd/csrc -I include tools/lift_plan_check.cpp -o lift_plan_check
//   lift_plan_check <model type 0|1|2> <nzeta> <m> <k_pcs> <rows> <num_cu> [pads] <block> ...
// One word per block of the dictionary, in order: poly:<functions>, fourier:<degree>, gaussian:<centres>, hermite:<functions>,
// fourier_sparser:<functions>.  The columns are laid out as kp_basis_create lays them out (variables, blocks, constant).
// One line of JSON: nvars, nfull, fourier_degree, pure_fourier, then lt, lds, stage_cols and error (the text of the refusal, or
// null) of the launch plan; with `pads`, also ColDesc::pad of every fourier column.  tests/test_lift_plan.py runs it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "koopman_hip.h"   // KP_MODEL_*
#include "kp_lift_plan.h"

static const int KP_MAX_VARS = 32;   // (kp_internal.h, which needs HIP)

int main(int argc, char** argv) {
  if (argc < 7) {
    fprintf(stderr, "usage: %s <model type 0|1|2> <nzeta> <m> <k_pcs> <rows> <num_cu> [pads] <kind>:<count> ...\n", argv[0]);
    return 2;
  }
  const int mt = atoi(argv[1]), nzeta = atoi(argv[2]), m = atoi(argv[3]), k_pcs = atoi(argv[4]), num_cu = atoi(argv[6]);
  const long long rows = atoll(argv[5]);
  int first = 7;
  const bool pads = argc > 7 && !strcmp(argv[7], "pads");
  if (pads) ++first;
  const int nvars = nzeta + (mt == KP_MODEL_NONLINEAR ? m : 0);
  // what kp_basis_create has checked before it lays out the columns
  if (mt < 0 || mt > 2 || nzeta < 1 || m < 0 || nvars > KP_MAX_VARS || k_pcs < 0 || rows < 0) {
    fprintf(stderr, "%s: not a dictionary kp_basis_create takes (model type 0..2, 1 <= variables <= %d, m >= 0)\n", argv[0], KP_MAX_VARS);
    return 2;
  }
  std::vector<ColDesc> cols;
  for (int i = 0; i < nvars; ++i) cols.push_back({COL_VAR, i, 0, 0});
  for (int a = first; a < argc; ++a) {
    const char* colon = strchr(argv[a], ':');
    const int cnt = colon ? atoi(colon + 1) : -1;
    const size_t len = colon ? (size_t)(colon - argv[a]) : 0;
    auto is = [&](const char* kind) { return len == strlen(kind) && !strncmp(argv[a], kind, len); };
    int kind = -1;
    if (is("poly")) kind = COL_MONO;
    else if (is("gaussian")) kind = COL_GAUSS;
    else if (is("hermite")) kind = COL_HERMITE;
    else if (is("fourier_sparser")) kind = COL_FSPARSE;
    if (is("fourier")) {
      const double nf = cnt >= 1 ? std::pow((double)(2 * cnt + 1), (double)nvars) : 0.0;
      if (cnt < 1 || nf > 1e6) {
        fprintf(stderr, "%s: %s: not a fourier block kp_basis_create takes (degree >= 1, at most 1e6 functions)\n", argv[0], argv[a]);
        return 2;
      }
      lift_fourier_append(cols, cnt, nvars, (int)std::llround(nf));
    } else if (kind >= 0 && cnt >= 0) {
      for (int i = 0; i < cnt; ++i) cols.push_back({kind, i, 0, 0});
    } else {
      fprintf(stderr, "%s: %s: not a block (poly, fourier, gaussian, hermite or fourier_sparser, then :count)\n", argv[0], argv[a]);
      return 2;
    }
  }
  cols.push_back({COL_CONST, 0, 0, 0});
  int fdeg = 0;
  bool pure = false;
  lift_fourier_flags(cols, nvars, &fdeg, &pure);
  const int nfull = (int)cols.size();
  const LiftPlan P = lift_plan_build(nvars, m, nfull, k_pcs, fdeg, pure, (int64_t)rows, num_cu);
  printf("{\"nvars\": %d, \"nfull\": %d, \"fourier_degree\": %d, \"pure_fourier\": %s, \"lt\": %d, \"lds\": %zu, \"stage_cols\": %d, \"error\": ",
         nvars, nfull, fdeg, pure ? "true" : "false", P.lt, P.lds, P.stage_cols);
  if (P.refusal) printf("\"%s\"", P.refusal);
  else printf("null");
  if (pads) {
    printf(", \"pads\": [");
    bool any = false;
    for (const ColDesc& c : cols)
      if (c.kind == COL_FOURIER) {
        printf("%s%u", any ? ", " : "", (unsigned)(uint32_t)c.pad);
        any = true;
      }
    printf("]");
  }
  printf("}\n");
  return 0;
}
