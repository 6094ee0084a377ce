// Prints the one-A-group cover plan of the Kronecker Gram kernel for a polynomial dictionary, host only:
//   g++ -std=c++17 -O2 -I koopman-realizations_amd/csrc tools/gram3_onea_check.cpp -o gram3_onea_check
//   gram3_onea_check <states> <inputs> <degree> [columns [factors]]          (arguments: tools/gram3_cover_check.cpp)
// One line of JSON.  "cover": the cover plan the search starts from (gram3_cover_build); "found": gram3_onea_build's result, its
// own coverage check included; "straddling": jobs with qs < nq; "hash": FNV-1a of desc; "s_hash": FNV-1a of the S groups of
// every row in plan order (the T groups and the weights left out: dictionaries that differ only in the inputs share it);
// "build_ms": the best of 5 builds, the cover plan's own build not counted ("cover_ms").  tests/test_gram3_onea_plan.py runs it.
#include <chrono>
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

static uint64_t fnv(uint64_t h, uint32_t v) {
  for (int k = 0; k < 4; ++k) h = (h ^ ((v >> (8 * k)) & 255u)) * 1099511628211ull;
  return h;
}

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

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
  Gram3CoverHost cov;
  double t0 = now_ms();
  const bool cover_ok = gram3_cover_build(rec.data(), N, D, nwt, 6, &cov);
  const double cover_ms = now_ms() - t0;
  Gram3CoverHost one;
  std::vector<int> hubs;
  bool found = false;
  double build_ms = 1e300;
  for (int rep = 0; cover_ok && rep < 5; ++rep) {
    one = Gram3CoverHost();
    hubs.clear();
    t0 = now_ms();
    found = gram3_onea_build(rec.data(), N, D, cov, &one, &hubs);
    build_ms = std::min(build_ms, now_ms() - t0);
  }
  if (!cover_ok) build_ms = 0.0;
  uint64_t hash = 14695981039346656037ull, s_hash = hash;
  int straddling = 0;
  if (found) {
    for (uint32_t v : one.jobs.desc) hash = fnv(hash, v);
    straddling = gram3_two_group_jobs(one.jobs);
    for (int job = 0; job < one.jobs.njobs; ++job) {
      const uint32_t* jd = &one.jobs.desc[(size_t)job * (1 + one.jobs.nq)];
      s_hash = fnv(s_hash, jd[0] & 255u);
      for (int q = 0; q < one.jobs.nq; ++q)
        for (int k = 0; k < 4; ++k) {
          const uint32_t gb = (jd[1 + q] >> (8 * k)) & 255u;
          if ((int)gb < G4) s_hash = fnv(s_hash, gb);
        }
    }
  }
  printf("{\"N\": %d, \"G4\": %d, \"nwt\": %d, \"cover_ok\": %s, \"cover\": {\"nq\": %d, \"njobs\": %d, \"quads\": %d, \"straddling\": %d}, \"found\": %s, \"hubs\": [",
         N, G4, nwt, cover_ok ? "true" : "false", cov.jobs.nq, cov.jobs.njobs, cov.jobs.nquads, cover_ok ? gram3_two_group_jobs(cov.jobs) : 0, found ? "true" : "false");
  for (size_t h = 0; found && h < hubs.size(); ++h) printf("%s%d", h ? ", " : "", hubs[h]);
  printf("], \"nq\": %d, \"njobs\": %d, \"quads\": %d, \"straddling\": %d, \"monomials\": %d, \"pairs\": %d, \"dst\": %zu, \"cover_ms\": %.3f, \"build_ms\": %.3f, "
         "\"hash\": \"%016llx\", \"s_hash\": \"%016llx\"}\n",
         found ? one.jobs.nq : 0, found ? one.jobs.njobs : 0, found ? one.jobs.nquads : 0, straddling, found ? one.nmonos : cov.nmonos, found ? one.npairs : 0,
         found ? one.dst.size() : (size_t)0, cover_ms, build_ms, (unsigned long long)hash, (unsigned long long)s_hash);
  return 0;
}
