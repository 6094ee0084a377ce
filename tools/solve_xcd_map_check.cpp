// Checks the workgroup order of the batched block substitution (csrc/kp_solve_xcd_map.h), host only:
//   g++ -std=c++17 -O2 -I koopman-realizations_amd/csrc tools/solve_xcd_map_check.cpp -o solve_xcd_map_check
//   solve_xcd_map_check [max_nb [max_ncb]]                                    (defaults 130 and 32)
// For every nb in 1..max_nb and ncb in 1..max_ncb it walks the ids 0 .. kp_solve_xcd_grid(ncb, nb) - 1 and counts
//   "not_bijective": (nb, ncb) where the mapped ids do not hit every (system, column block) exactly once, or one is out of range;
//   "split_systems": (nb, ncb) where two column blocks of a system have different id % 8;
//   "unordered":     (nb, ncb) where a system's column blocks are not consecutive, ascending, in its die's sequence id / 8;
//   "max_padding":   the most ids of a grid that map to no system (bound: 7 ncb).
// One line of JSON; tests/test_solve_xcd_map.py runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kp_solve_xcd_map.h"

int main(int argc, char** argv) {
  const int max_nb = argc > 1 ? atoi(argv[1]) : 130, max_ncb = argc > 2 ? atoi(argv[2]) : 32;
  long cases = 0, not_bijective = 0, split_systems = 0, unordered = 0, max_padding = 0, padding_over_bound = 0;
  for (int nb = 1; nb <= max_nb; ++nb)
    for (int ncb = 1; ncb <= max_ncb; ++ncb) {
      ++cases;
      const unsigned grid = kp_solve_xcd_grid(ncb, nb);
      std::vector<int> hits((size_t)nb * ncb, 0), die((size_t)nb, -1);
      std::vector<long> first((size_t)nb, -1);
      bool bij = grid >= (unsigned)(nb * ncb), whole = true, ordered = true;
      long padding = 0;
      for (unsigned id = 0; id < grid; ++id) {
        int sys = -1, cb = -1;
        if (!kp_solve_xcd_map(id, ncb, nb, &sys, &cb)) {
          ++padding;
          continue;
        }
        if (sys < 0 || sys >= nb || cb < 0 || cb >= ncb) {
          bij = false;
          continue;
        }
        ++hits[(size_t)sys * ncb + cb];
        const int x = (int)(id % KP_SOLVE_XCDS);
        const long k = (long)(id / KP_SOLVE_XCDS);
        if (die[sys] < 0) {
          die[sys] = x;
          first[sys] = k - cb;
        }
        if (die[sys] != x) whole = false;
        if (k - cb != first[sys]) ordered = false;
      }
      for (int h : hits)
        if (h != 1) bij = false;
      if (!bij) ++not_bijective;
      if (!whole) ++split_systems;
      if (!ordered) ++unordered;
      if (padding > max_padding) max_padding = padding;
      if (padding > 7L * ncb || padding != (long)grid - (long)nb * ncb) ++padding_over_bound;
    }
  printf("{\"cases\": %ld, \"not_bijective\": %ld, \"split_systems\": %ld, \"unordered\": %ld, \"max_padding\": %ld, \"padding_over_bound\": %ld, "
         "\"grid_128_21\": %u, \"grid_9_21\": %u}\n",
         cases, not_bijective, split_systems, unordered, max_padding, padding_over_bound, kp_solve_xcd_grid(21, 128), kp_solve_xcd_grid(21, 9));
  return 0;
}
