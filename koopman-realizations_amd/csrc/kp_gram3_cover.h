// Host-side plans of the Kronecker Gram kernel (kp_gram3.hip): rows of B groups -> quads -> jobs, and the COVER plan of a
// monomial dictionary.  Plain C++, no device code: tools/gram3_cover_check.cpp builds it on its own.
//
// psi_x psi_x' of a monomial dictionary is a moment matrix: entry (i, j) depends only on the exponent sum e_i + e_j.  The
// circulant plan forms every 4 x 4 block of the symmetric half (231 group pairs for the 84 columns of poly-3 on 6 states:
// 3 570 entries), but those entries are only 924 distinct monomials.  The cover plan keeps a subset of the group pairs that
// still produces every distinct monomial at least once (108 pairs), the reduction writes each entry of G from the ONE block
// element that is its monomial's designated source (gram3_cover_build: dst_off / dst).  Columns keep the dictionary's order.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

struct Gram3JobsHost {
  int nq = 0, njobs = 0, nquads = 0;
  std::vector<uint32_t> desc;        // [njobs][1 + nq], the layout of Gram3Args::desc
};

// The circulant plan's rows: A group g against its circulant half of the psi_x groups (g, g + 1, ..., g + floor(G4 / 2) mod G4;
// antipodal pairs once) and all G4 groups of psi_y.  *maxq: the most quads a row has.
inline std::vector<std::vector<int>> gram3_circulant_rows(int G4, size_t* maxq) {
  std::vector<std::vector<int>> rows(G4);
  *maxq = 0;
  for (int g = 0; g < G4; ++g) {
    for (int d = 0; d <= G4 / 2; ++d) {
      if (d > 0 && 2 * d == G4 && g >= G4 / 2) continue;
      rows[g].push_back((g + d) % G4);
    }
    for (int h = 0; h < G4; ++h) rows[g].push_back(G4 + h);
    *maxq = std::max(*maxq, (rows[g].size() + 3) / 4);
  }
  return rows;
}

// rows[g]: the B groups (psi_x groups < G4, psi_y groups G4 + h) that A group g is multiplied with.  All quads (A group, 4 B
// groups) of all rows form one list; a job (one wave) is nq CONSECUTIVE quads, so it spans at most two A groups when nq <= the
// quads of every row (nq_rows: the bound the caller's rows give), and whole workgroups (wpw jobs) fill evenly.
inline void gram3_pack_rows(const std::vector<std::vector<int>>& rows, int G4, int nwt, int nq_cap, size_t nq_rows, int wpw, int nq_force, Gram3JobsHost* out) {
  const int ZG = 2 * G4;
  std::vector<std::pair<int, uint32_t>> quads;
  for (int g = 0; g < G4; ++g) {
    const size_t nquads = (rows[g].size() + 3) / 4;
    for (size_t q = 0; q < nquads; ++q) {
      uint32_t packed = 0;
      for (int k = 0; k < 4; ++k) {
        size_t idx = q * 4 + k;
        int gb = idx < rows[g].size() ? rows[g][idx] : ZG;
        packed |= (uint32_t)gb << (8 * k);
      }
      quads.push_back({g, packed});
    }
  }
  const int TQ = (int)quads.size();
  // cost ~ waves x (MFMA cycles of nq quads over the two k-steps of a tile + the per-tile VALU share)
  int nq = 1;
  double best = 1e300;
  constexpr int NQMAX = 6;   // 7 or 8 quads (140/160 accumulator registers) spill with the 256-register budget of 2 waves per SIMD
  for (int c = 1; c <= std::min(NQMAX, nq_cap) && (size_t)c <= nq_rows; ++c) {
    int waves = ((TQ + c - 1) / c + 3) / 4 * 4;
    double cost = (double)waves * (c * nwt * 33.0 + 400.0);
    if (cost < best) { best = cost; nq = c; }
  }
  if (nq_force > 0) nq = nq_force;
  else if (const char* ov = getenv("KP_GRAM3_NQ")) {   // tuning override
    int v = atoi(ov);
    if (v >= 1 && v <= std::min(NQMAX, nq_cap) && (size_t)v <= nq_rows) nq = v;
  }
  out->nq = nq;
  out->nquads = TQ;
  out->desc.clear();
  int njobs = 0;
  const uint32_t zq = (uint32_t)ZG * 0x01010101u;
  for (int q0 = 0; q0 < TQ || njobs % wpw; q0 += nq) {
    int a0 = q0 < TQ ? quads[q0].first : 0, a1 = a0, qs = nq;
    for (int q = 0; q < nq; ++q)
      if (q0 + q < TQ && quads[q0 + q].first != a0) { a1 = quads[q0 + q].first; qs = q; break; }
    out->desc.push_back((uint32_t)a0 | ((uint32_t)a1 << 8) | ((uint32_t)qs << 16));
    for (int q = 0; q < nq; ++q) out->desc.push_back(q0 + q < TQ ? quads[q0 + q].second : zq);
    ++njobs;
  }
  out->njobs = njobs;
}

struct Gram3CoverHost {
  Gram3JobsHost jobs;
  int npairs = 0, nmonos = 0;        // S group pairs kept / distinct exponent sums
  // CSR over the block elements of the plan, element e = ((job nq + quad) 4 + B slot) 16 + 4 row + column: the entries
  // (i <= j) of psi_x psi_x' whose designated source it is, as i | j << 16
  std::vector<uint32_t> dst_off, dst;
};

// The cover plan of a dictionary of N monomial columns (recipes: <= 4 power-table ids v D + e - 1 per column, 255 = none).
// False when the plan cannot be built or fails its own coverage check: the caller stays on the circulant plan.
inline bool gram3_cover_build(const uint32_t* recipes, int N, int D, int nwt, int nq_cap, int wpw, Gram3CoverHost* out) {
  if (N < 1 || D < 1 || N > 4 * 127) return false;
  const int G4 = (N + 3) / 4;
  int nv = 1;
  for (int c = 0; c < N; ++c)
    for (int f = 0; f < 4; ++f) {
      const int id = (int)((recipes[c] >> (8 * f)) & 255u);
      if (id != 255) nv = std::max(nv, id / D + 1);
    }
  std::vector<std::vector<uint8_t>> ex(N, std::vector<uint8_t>(nv, 0));
  for (int c = 0; c < N; ++c)
    for (int f = 0; f < 4; ++f) {
      const int id = (int)((recipes[c] >> (8 * f)) & 255u);
      if (id != 255) ex[c][id / D] += (uint8_t)(id % D + 1);
    }
  // mono[i N + j]: id of the exponent sum e_i + e_j
  std::map<std::vector<uint8_t>, int> ids;
  std::vector<int> mono((size_t)N * N);
  std::vector<uint8_t> sum(nv);
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) {
      for (int v = 0; v < nv; ++v) sum[v] = (uint8_t)(ex[i][v] + ex[j][v]);
      mono[(size_t)i * N + j] = ids.emplace(sum, (int)ids.size()).first->second;
    }
  const int nm = (int)ids.size();

  // ---- the pairs: greedy set cover over the group pairs {ga <= gb}, ties to the lowest (ga, gb) ----
  // (padding columns of the last group take part in nothing)
  auto products = [&](int ga, int gb, auto&& f) {
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c)
        if (4 * ga + r < N && 4 * gb + c < N) f(mono[(size_t)(4 * ga + r) * N + 4 * gb + c]);
  };
  std::vector<char> have(nm, 0);
  std::vector<std::pair<int, int>> chosen;
  for (int left = nm; left > 0;) {
    int bn = 0, ba = -1, bb = -1;
    std::vector<char> seen(nm, 0);
    for (int ga = 0; ga < G4; ++ga)
      for (int gb = ga; gb < G4; ++gb) {
        int n = 0;
        std::vector<int> mine;
        products(ga, gb, [&](int mo) {
          if (!have[mo] && !seen[mo]) { seen[mo] = 1; mine.push_back(mo); ++n; }
        });
        for (int mo : mine) seen[mo] = 0;
        if (n > bn) { bn = n; ba = ga; bb = gb; }
      }
    if (bn == 0) return false;
    products(ba, bb, [&](int mo) {
      if (!have[mo]) { have[mo] = 1; --left; }
    });
    chosen.push_back({ba, bb});
  }

  // ---- the rows: a pair goes to the row of either of its groups - where it opens no new quad, else the lighter one ----
  std::vector<std::vector<int>> rows(G4);
  for (auto& p : chosen)
    if (p.first == p.second) rows[p.first].push_back(p.second);
  std::vector<std::pair<int, int>> off;
  for (auto& p : chosen)
    if (p.first != p.second) off.push_back(p);
  std::sort(off.begin(), off.end());
  auto quads_of = [&](size_t s) { return (s + G4 + 3) / 4; };
  for (auto& p : off) {
    const size_t la = rows[p.first].size(), lb = rows[p.second].size();
    const size_t ca = quads_of(la + 1) - quads_of(la), cb = quads_of(lb + 1) - quads_of(lb);
    const bool to_b = cb < ca || (cb == ca && lb < la);
    rows[to_b ? p.second : p.first].push_back(to_b ? p.first : p.second);
  }
  size_t minq = ~(size_t)0;
  for (int g = 0; g < G4; ++g) {
    for (int h = 0; h < G4; ++h) rows[g].push_back(G4 + h);     // T groups follow the S groups of a row
    minq = std::min(minq, (rows[g].size() + 3) / 4);
  }
  gram3_pack_rows(rows, G4, nwt, nq_cap, minq, wpw, 0, &out->jobs);
  out->npairs = (int)chosen.size();
  out->nmonos = nm;

  // ---- designated sources, in plan order, and the coverage check ----
  const Gram3JobsHost& J = out->jobs;
  const int nq = J.nq;
  std::vector<int> src(nm, -1);
  std::vector<int> tgroups((size_t)G4 * G4, 0);                // times T block (ga, h) is formed: exactly once
  for (int job = 0; job < J.njobs; ++job) {
    const uint32_t* jd = &J.desc[(size_t)job * (1 + nq)];
    const int a0 = (int)(jd[0] & 255u), a1 = (int)((jd[0] >> 8) & 255u), qs = (int)((jd[0] >> 16) & 255u);
    if (a0 >= G4 || a1 >= G4) return false;
    for (int q = 0; q < nq; ++q) {
      const int ga = q < qs ? a0 : a1;
      for (int k = 0; k < 4; ++k) {
        const int gb = (int)((jd[1 + q] >> (8 * k)) & 255u);
        if (gb > 2 * G4) return false;
        if (gb >= G4) {
          if (gb < 2 * G4) ++tgroups[(size_t)ga * G4 + gb - G4];
          continue;
        }
        for (int r = 0; r < 4; ++r)
          for (int c = 0; c < 4; ++c) {
            const int i = 4 * ga + r, j = 4 * gb + c;
            if (i >= N || j >= N) continue;
            int& s = src[mono[(size_t)i * N + j]];
            if (s < 0) s = ((job * nq + q) * 4 + k) * 16 + 4 * r + c;
          }
      }
    }
  }
  for (int t : tgroups)
    if (t != 1) return false;                                  // (a job of more than two A groups shows here: its later quads land on a1)
  const int nel = J.njobs * nq * 64;
  std::vector<uint32_t> cnt(nel + 1, 0);
  for (int i = 0; i < N; ++i)
    for (int j = i; j < N; ++j) {
      const int s = src[mono[(size_t)i * N + j]];
      if (s < 0) return false;                                 // an entry without a source
      ++cnt[s + 1];
    }
  for (int e = 0; e < nel; ++e) cnt[e + 1] += cnt[e];
  out->dst_off = cnt;
  out->dst.assign(cnt[nel], 0);
  std::vector<uint32_t> fill(cnt.begin(), cnt.end() - 1);
  for (int i = 0; i < N; ++i)
    for (int j = i; j < N; ++j) out->dst[fill[src[mono[(size_t)i * N + j]]]++] = (uint32_t)i | ((uint32_t)j << 16);
  if ((size_t)cnt[nel] != (size_t)N * (N + 1) / 2) return false;
  // every destination's monomial is its source element's: decode the element back to its columns through desc alone
  for (int e = 0; e < nel; ++e) {
    if (cnt[e] == cnt[e + 1]) continue;
    const int c = e & 3, r = (e >> 2) & 3, k = (e >> 4) & 3, jq = e >> 6, q = jq % nq, job = jq / nq;
    const uint32_t* jd = &J.desc[(size_t)job * (1 + nq)];
    const int ga = q < (int)((jd[0] >> 16) & 255u) ? (int)(jd[0] & 255u) : (int)((jd[0] >> 8) & 255u);
    const int gb = (int)((jd[1 + q] >> (8 * k)) & 255u);
    const int i = 4 * ga + r, j = 4 * gb + c;
    if (gb >= G4 || i >= N || j >= N) return false;
    for (uint32_t d = cnt[e]; d < cnt[e + 1]; ++d) {
      const int di = (int)(out->dst[d] & 0xffffu), dj = (int)(out->dst[d] >> 16);
      if (di > dj || dj >= N || mono[(size_t)di * N + dj] != mono[(size_t)i * N + j]) return false;
    }
  }
  return true;
}
