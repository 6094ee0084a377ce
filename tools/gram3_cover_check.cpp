// Prints the circulant and the cover plan of the Kronecker Gram kernel for a polynomial dictionary, host only:
//   g++ -std=c++17 -O1 -I koopman-realizations_amd/csrc tools/gram3_cover_check.cpp -o gram3_cover_check
//   gram3_cover_check <states> <inputs> <degree> [columns [factors]]
// (columns: the first `columns - 1` monomials of def_polyLift's order plus the constant, as the library's dictionaries end; 0: all.
// factors: only monomials of at most so many variables - the Kronecker kernel takes three.)
// One line of JSON; "cover_ok" is gram3_cover_build's own coverage check, "kept" the rule of kp_gram3.hip (fewer jobs than the
// circulant plan).  tests/test_gram3_cover_plan.py runs it.
#include <cstdio>
#include <cstdlib>

#include "kp_gram3_cover.h"

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
    fprintf(stderr, "usage: %s <states> <inputs> <degree> [columns [factors]]\n", argv[0]);
    return 2;
  }
  const int nz = atoi(argv[1]), m = atoi(argv[2]), deg = atoi(argv[3]);
  std::vector<std::vector<int>> rows;
  for (int d = 1; d <= deg; ++d) {
    std::vector<int> head;
    compositions(d, nz, head, rows);
  }
  if (argc > 5) {
    const int maxf = atoi(argv[5]);
    std::vector<std::vector<int>> kept;
    for (auto& r : rows)
      if (std::count_if(r.begin(), r.end(), [](int e) { return e > 0; }) <= maxf) kept.push_back(r);
    rows.swap(kept);
  }
  if (argc > 4 && atoi(argv[4]) >= 1 && (size_t)atoi(argv[4]) - 1 < rows.size()) rows.resize(atoi(argv[4]) - 1);
  rows.push_back(std::vector<int>(nz, 0));
  const int N = (int)rows.size(), D = deg, nwt = (m + 1) * (m + 2) / 2, G4 = (N + 3) / 4;
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
  size_t maxq = 0;
  const std::vector<std::vector<int>> crow = gram3_circulant_rows(G4, &maxq);     // (make_plan3's)
  Gram3JobsHost circ;
  gram3_pack_rows(crow, G4, nwt, 6, maxq, &circ);
  Gram3CoverHost cov;
  const bool ok = gram3_cover_build(rec.data(), N, D, nwt, 6, &cov);
  printf("{\"N\": %d, \"G4\": %d, \"nwt\": %d, \"circ\": {\"quads\": %d, \"nq\": %d, \"njobs\": %d, \"nsuper\": %d}, "
         "\"cover_ok\": %s, \"cover\": {\"monomials\": %d, \"pairs\": %d, \"quads\": %d, \"nq\": %d, \"njobs\": %d, \"nsuper\": %d, \"dst\": %zu}, \"kept\": %s}\n",
         N, G4, nwt, circ.nquads, circ.nq, circ.njobs, circ.njobs / 4, ok ? "true" : "false", cov.nmonos, cov.npairs, cov.jobs.nquads, cov.jobs.nq,
         cov.jobs.njobs, cov.jobs.njobs / 4, cov.dst.size(), ok && cov.jobs.njobs < circ.njobs ? "true" : "false");
  return 0;
}
