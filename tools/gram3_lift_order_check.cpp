// Builds and checks the lift slot table of the Kronecker Gram kernel for a polynomial dictionary, host only:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I koopman-realizations_amd/csrc
//       tools/gram3_lift_order_check.cpp -o gram3_lift_order_check
//   gram3_lift_order_check <states> <inputs> <degree> [columns [maxfactors [minfactors]]]
// The first arguments are those of tools/gram3_cover_check.cpp; minfactors keeps, of the monomials behind the variables, those
// of at least that many variables (a dictionary of many three-factor columns).  One line of JSON: the job counts by real
// factors, and one flag per property of kp_gram3_lift.h, each checked here against the recipes themselves and not against the
// builder's own bookkeeping; "slots": the table as 768 words.  tests/test_gram3_lift_order.py runs it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "kp_gram3_lift.h"

static void compositions(int total, int n, std::vector<int>& head, std::vector<std::vector<int>>& rows) {
  // exponent rows of n variables summing to total, the last variable the slowest (ksysid.poly_exponent_table)
  if (n == 1) {
    std::vector<int> r{total};
    r.insert(r.end(), head.rbegin(), head.rend());
    rows.push_back(r);
    return;
  }
  for (int last = 0; last <= total; ++last) {
    head.push_back(last);
    compositions(total - last, n - 1, head, rows);
    head.pop_back();
  }
}

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s <states> <inputs> <degree> [columns [maxfactors [minfactors]]]\n", argv[0]);
    return 2;
  }
  const int nz = atoi(argv[1]), m = atoi(argv[2]), deg = atoi(argv[3]);
  const int maxf = argc > 5 && atoi(argv[5]) > 0 ? atoi(argv[5]) : 1 << 30, minf = argc > 6 ? atoi(argv[6]) : 0;
  std::vector<std::vector<int>> rows;
  for (int d = 1; d <= deg; ++d) {
    std::vector<int> head;
    compositions(d, nz, head, rows);
  }
  {
    std::vector<std::vector<int>> kept;
    for (size_t i = 0; i < rows.size(); ++i) {
      const int nf = (int)std::count_if(rows[i].begin(), rows[i].end(), [](int e) { return e > 0; });
      if ((int)i < nz || (nf <= maxf && nf >= minf)) kept.push_back(rows[i]);
    }
    rows.swap(kept);
  }
  if (argc > 4 && atoi(argv[4]) >= 1 && (size_t)atoi(argv[4]) - 1 < rows.size()) rows.resize(atoi(argv[4]) - 1);
  rows.push_back(std::vector<int>(nz, 0));
  const int N = (int)rows.size(), D = deg, nwt = (m + 1) * (m + 2) / 2, nitems = 2 * N + nwt - 1;
  std::vector<uint32_t> rec(N, 0xffffffffu);
  for (int c = 0; c < N; ++c) {
    int nf = 0;
    for (int v = 0; v < nz; ++v)
      if (rows[c][v]) {
        if (nf == 4) return 3;
        rec[c] = (rec[c] & ~(0xffu << (8 * nf))) | ((uint32_t)(v * D + rows[c][v] - 1) << (8 * nf));
        ++nf;
      }
  }
  // the real factors of every item, from the dictionary itself: a column's variables; weight (x, y), x <= y, pair index >= 1
  std::vector<int> nreal(nitems, 0);
  for (int it = 0; it < 2 * N; ++it)
    nreal[it] = (int)std::count_if(rows[it % N].begin(), rows[it % N].end(), [](int e) { return e > 0; });
  {
    int cnt = 0;
    for (int x = 0; x <= m; ++x)
      for (int y = x; y <= m; ++y) {
        if (cnt > 0) nreal[2 * N + cnt - 1] = (x > 0) + (y > 0);
        ++cnt;
      }
  }
  int heavy = 0, two = 0, light = 0;
  for (int it = 0; it < nitems; ++it) (nreal[it] == 3 ? heavy : nreal[it] == 2 ? two : light) += 4;

  Gram3LiftOrderHost lo;
  const bool ordered = gram3_lift_order_build(rec.data(), N, m, &lo);
  bool once = true, idle_behind = true, light_steps = true, real_lead = true, recipe_order = true, counts = true;
  if (ordered) {
    if ((int)lo.slot.size() != GRAM3_LIFT_SLOTS) return 4;
    std::vector<int> seen(4 * nitems, 0);
    int njobs = 0;
    for (int sidx = 0; sidx < GRAM3_LIFT_SLOTS; ++sidx) {
      const uint32_t w = lo.slot[sidx];
      if (w == GRAM3_LIFT_IDLE) continue;
      const int item = (int)(w & 255u), pair = (int)((w >> 8) & 3u), nr = (int)((w >> 16) & 3u);
      if (item >= nitems) { once = false; continue; }
      ++seen[pair * nitems + item];
      ++njobs;
      if (sidx >= 4 * nitems) idle_behind = false;       // the jobs fill the leading slots, the idle ones follow
      if (nr != nreal[item]) counts = false;
      if (sidx >= 256 && nreal[item] > 2) light_steps = false;
      // the factor sources: the real ones first, ascending (= recipe order), then the constant; each real factor once
      int p[3];
      for (int f = 0; f < 3; ++f) p[f] = (int)((w >> (10 + 2 * f)) & 3u);
      for (int f = 0; f < 3; ++f) {
        const bool is_real = p[f] != 3;
        if (is_real != (f < nreal[item])) real_lead = false;
        if (is_real) {
          // source p[f] of the item must be one of its real factors
          const bool src_real = item < 2 * N ? ((rec[item % N] >> (8 * p[f])) & 255u) != 255u : (p[f] == 0 ? nreal[item] == 2 : p[f] == 1);
          if (!src_real) real_lead = false;
          if (f > 0 && p[f - 1] != 3 && p[f - 1] >= p[f]) recipe_order = false;
        }
      }
      if (nreal[item] == 3 && !(p[0] == 0 && p[1] == 1 && p[2] == 2)) recipe_order = false;
    }
    for (int e = 0; e < 4 * nitems; ++e)
      if (seen[e] != 1) once = false;
    if (njobs != 4 * nitems) once = false;
    if (lo.heavy != heavy || lo.two != two || lo.light != light) counts = false;
  }
  printf("{\"N\": %d, \"nitems\": %d, \"njobs\": %d, \"heavy\": %d, \"two\": %d, \"light\": %d, \"ordered\": %s, \"order\": \"%s\", "
         "\"once\": %s, \"idle_behind\": %s, \"light_steps\": %s, \"real_lead\": %s, \"recipe_order\": %s, \"counts\": %s, \"slots\": [",
         N, nitems, 4 * nitems, heavy, two, light, ordered ? "true" : "false", ordered ? "ordered" : "old", once ? "true" : "false",
         idle_behind ? "true" : "false", light_steps ? "true" : "false", real_lead ? "true" : "false", recipe_order ? "true" : "false",
         counts ? "true" : "false");
  for (size_t i = 0; i < lo.slot.size(); ++i) printf("%s%u", i ? ", " : "", lo.slot[i]);
  printf("]}\n");
  return 0;
}
