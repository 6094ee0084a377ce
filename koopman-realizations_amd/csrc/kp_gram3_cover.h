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

constexpr int GRAM3_WAVES = 4;       // waves (jobs) of a workgroup of kp_gram3_kernel

// rows[g]: the B groups (psi_x groups < G4, psi_y groups G4 + h) that A group g is multiplied with.  All quads (A group, 4 B
// groups) of all rows form one list; a job (one wave) is nq CONSECUTIVE quads, so it spans at most two A groups when nq <= the
// quads of every row (nq_rows: the bound the caller's rows give), and whole workgroups (GRAM3_WAVES jobs) fill evenly.
inline void gram3_pack_rows(const std::vector<std::vector<int>>& rows, int G4, int nwt, int nq_cap, size_t nq_rows, Gram3JobsHost* out) {
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
  if (const char* ov = getenv("KP_GRAM3_NQ")) {   // tuning override
    int v = atoi(ov);
    if (v >= 1 && v <= std::min(NQMAX, nq_cap) && (size_t)v <= nq_rows) nq = v;
  }
  out->nq = nq;
  out->nquads = TQ;
  out->desc.clear();
  int njobs = 0;
  const uint32_t zq = (uint32_t)ZG * 0x01010101u;
  for (int q0 = 0; q0 < TQ || njobs % GRAM3_WAVES; q0 += nq) {
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
inline bool gram3_cover_build(const uint32_t* recipes, int N, int D, int nwt, int nq_cap, Gram3CoverHost* out) {
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
  gram3_pack_rows(rows, G4, nwt, nq_cap, minq, &out->jobs);
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

// ---------------------------------------------------------------------------------------------------------------------
// The ONE-A-GROUP cover plan: the cover plan's quads per job and job count, but no job spans two A groups - a wave weighs
// its A fragment once per k-step, not twice (kp_gram3_kernel's tile variant QS == NQ).  gram3_pack_rows cuts jobs out of the
// consecutive quads of all rows, so most of them straddle two rows (headline: 17 of 24); here a row IS one job (a "light" row:
// its G4 T groups and at most 4 nq - G4 S groups) or two (a "hub" row: at most 8 nq - G4 S groups), njobs - G4 hubs in all.
// Which pairs are kept and which row of its two a pair goes to is searched: per candidate hub set (lexicographic) a greedy
// set cover under the rows' capacities - first the pairs that still add products and that a hub with room can take, then the
// most new products, ties to the lowest (ga, gb) - until one covers every product.  Deterministic, bounded work.

// mono[i N + j]: id of the exponent sum e_i + e_j of a dictionary's columns (gram3_cover_build's ids); returns their count, 0: bad arguments
inline int gram3_monomial_ids(const uint32_t* recipes, int N, int D, std::vector<int>* mono) {
  if (N < 1 || D < 1 || N > 4 * 127) return 0;
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
  std::map<std::vector<uint8_t>, int> ids;
  mono->assign((size_t)N * N, 0);
  std::vector<uint8_t> sum(nv);
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) {
      for (int v = 0; v < nv; ++v) sum[v] = (uint8_t)(ex[i][v] + ex[j][v]);
      (*mono)[(size_t)i * N + j] = ids.emplace(sum, (int)ids.size()).first->second;
    }
  return (int)ids.size();
}

// Designated sources in plan order, the coverage check and the reduction's CSR lists of a job list J: what gram3_cover_build
// does with its own jobs, for any plan (every entry (i <= j) of real columns has exactly one source of its own monomial,
// decoded back through desc alone; every T block is formed once; all ids in range).  one_group: every job has qs == nq as well.
inline bool gram3_cover_sources(const std::vector<int>& mono, int nm, int N, bool one_group, Gram3CoverHost* out) {
  const int G4 = (N + 3) / 4;
  const Gram3JobsHost& J = out->jobs;
  const int nq = J.nq;
  if (nq < 1 || J.njobs < 1 || J.desc.size() != (size_t)J.njobs * (1 + nq)) return false;
  std::vector<int> src(nm, -1);
  std::vector<int> tgroups((size_t)G4 * G4, 0);
  for (int job = 0; job < J.njobs; ++job) {
    const uint32_t* jd = &J.desc[(size_t)job * (1 + nq)];
    const int a0 = (int)(jd[0] & 255u), a1 = (int)((jd[0] >> 8) & 255u), qs = (int)((jd[0] >> 16) & 255u);
    if (a0 >= G4 || a1 >= G4) return false;
    if (one_group && (qs != nq || a1 != a0)) return false;
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
    if (t != 1) return false;
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

// jobs of a plan that span two A groups (kp_timer_get(15) reports it for the plan of the last Gram launch)
inline int gram3_two_group_jobs(const Gram3JobsHost& J) {
  int n = 0;
  for (int job = 0; job < J.njobs; ++job) n += (int)((J.desc[(size_t)job * (1 + J.nq)] >> 16) & 255u) < J.nq;
  return n;
}

constexpr int GRAM3_ONEA_MAX_SETS = 2048;   // candidate hub sets tried at most (all 1 330 triples of the headline: it finds its plan at the 878th)

// The one-A-group plan of the dictionary whose cover plan is `cover` (gram3_cover_build's, same arguments): same nq, same
// njobs.  False (*out is then not a plan) when there is nothing to gain (no job of `cover` spans two A groups),
// the capacities cannot hold the rows, no candidate hub set covers every product, or the plan fails its own check: the caller
// keeps the cover plan.  hubs: the hub rows of the plan found.
inline bool gram3_onea_build(const uint32_t* recipes, int N, int D, const Gram3CoverHost& cover, Gram3CoverHost* out, std::vector<int>* hubs = nullptr) {
  std::vector<int> mono;
  const int nm = gram3_monomial_ids(recipes, N, D, &mono);
  if (nm < 1 || nm != cover.nmonos) return false;
  const int G4 = (N + 3) / 4, ZG = 2 * G4, nq = cover.jobs.nq, njobs = cover.jobs.njobs;
  const int H = njobs - G4, cap_light = 4 * nq - G4, cap_hub = 8 * nq - G4;
  if (gram3_two_group_jobs(cover.jobs) == 0) return false;
  if (H < 0 || H > G4 || cap_light < 0) return false;

  // ---- each pair's distinct products, once; which pairs hold a product ----
  const int NP = G4 * (G4 + 1) / 2;
  std::vector<int> pa(NP), pb(NP), pcnt(NP, 0), pmono((size_t)NP * 16);
  {
    int p = 0;
    for (int ga = 0; ga < G4; ++ga)
      for (int gb = ga; gb < G4; ++gb, ++p) {
        pa[p] = ga;
        pb[p] = gb;
        int* mine = &pmono[(size_t)p * 16];
        for (int r = 0; r < 4; ++r)
          for (int c = 0; c < 4; ++c) {
            if (4 * ga + r >= N || 4 * gb + c >= N) continue;
            const int mo = mono[(size_t)(4 * ga + r) * N + 4 * gb + c];
            if (std::find(mine, mine + pcnt[p], mo) == mine + pcnt[p]) mine[pcnt[p]++] = mo;
          }
      }
  }
  std::vector<int> moff(nm + 1, 0), mpair;
  for (int p = 0; p < NP; ++p)
    for (int k = 0; k < pcnt[p]; ++k) ++moff[pmono[(size_t)p * 16 + k] + 1];
  for (int mo = 0; mo < nm; ++mo) moff[mo + 1] += moff[mo];
  mpair.resize(moff[nm]);
  {
    std::vector<int> fill(moff.begin(), moff.end() - 1);
    for (int p = 0; p < NP; ++p)
      for (int k = 0; k < pcnt[p]; ++k) mpair[fill[pmono[(size_t)p * 16 + k]]++] = p;
  }

  // ---- candidate hub sets in lexicographic order; per set the capacity-aware greedy cover ----
  std::vector<int> hub(H);
  for (int h = 0; h < H; ++h) hub[h] = h;
  std::vector<int> gain(NP), cap(G4), act(NP), hact(NP);
  std::vector<char> have(nm), is_hub(G4);
  std::vector<std::vector<int>> srow(G4);
  bool found = false;
  for (int tried = 0; tried < GRAM3_ONEA_MAX_SETS && !found; ++tried) {
    std::fill(is_hub.begin(), is_hub.end(), 0);
    for (int h : hub) is_hub[h] = 1;
    for (int g = 0; g < G4; ++g) {
      cap[g] = is_hub[g] ? cap_hub : cap_light;
      srow[g].clear();
    }
    gain = pcnt;
    std::fill(have.begin(), have.end(), 0);
    int left = nm;
    int nact = NP, nhact = 0;
    for (int p = 0; p < NP; ++p) {
      act[p] = p;
      if (is_hub[pa[p]] || is_hub[pb[p]]) hact[nhact++] = p;
    }
    while (left > 0) {
      // the pairs a hub with room can take come first, and only the pairs of the hubs need a look for them; pairs without new
      // products or without a row with room never come back: either scan drops them, order kept
      int best = -1, bgain = 0, keep = 0;
      for (int x = 0; x < nhact; ++x) {
        const int p = hact[x], ga = pa[p], gb = pb[p];
        if (gain[p] == 0 || !((is_hub[ga] && cap[ga] > 0) || (is_hub[gb] && cap[gb] > 0))) continue;
        hact[keep++] = p;
        if (gain[p] > bgain) { bgain = gain[p]; best = p; }
      }
      nhact = keep;
      if (best < 0) {
        keep = 0;
        for (int x = 0; x < nact; ++x) {
          const int p = act[x], ga = pa[p], gb = pb[p];
          if (gain[p] == 0 || (cap[ga] <= 0 && cap[gb] <= 0)) continue;
          act[keep++] = p;
          if (gain[p] > bgain) { bgain = gain[p]; best = p; }
        }
        nact = keep;
      }
      if (best < 0) break;
      const int ga = pa[best], gb = pb[best];
      // the row: a hub with room before a light row, then the one with more room, ties to ga
      const int ka = cap[ga] > 0 ? (is_hub[ga] ? 1024 : 0) + cap[ga] : -1, kb = cap[gb] > 0 ? (is_hub[gb] ? 1024 : 0) + cap[gb] : -1;
      const bool to_b = kb > ka;
      const int row = to_b ? gb : ga;
      srow[row].push_back(to_b ? ga : gb);
      --cap[row];
      for (int k = 0; k < pcnt[best]; ++k) {
        const int mo = pmono[(size_t)best * 16 + k];
        if (have[mo]) continue;
        have[mo] = 1;
        --left;
        for (int x = moff[mo]; x < moff[mo + 1]; ++x) --gain[mpair[x]];
      }
      // a row that is full now takes its pairs with the other full rows out of play: a product that only such pairs hold can
      // no longer be covered, and this hub set is given up at once (most sets end here, long before the capacities run out)
      bool dead = false;
      for (int g = 0; cap[row] == 0 && g < G4 && !dead; ++g) {
        if (cap[g] > 0) continue;
        const int lo = std::min(g, row), hi = std::max(g, row), p = lo * G4 - lo * (lo - 1) / 2 + hi - lo;
        for (int k = 0; k < pcnt[p] && !dead; ++k) {
          const int mo = pmono[(size_t)p * 16 + k];
          if (have[mo]) continue;
          dead = true;
          for (int x = moff[mo]; x < moff[mo + 1] && dead; ++x) dead = cap[pa[mpair[x]]] <= 0 && cap[pb[mpair[x]]] <= 0;
        }
      }
      if (dead) break;
    }
    if (left == 0) { found = true; break; }
    // the next H-subset of the G4 groups
    int h = H - 1;
    while (h >= 0 && hub[h] == G4 - H + h) --h;
    if (h < 0) break;
    ++hub[h];
    for (int k = h + 1; k < H; ++k) hub[k] = hub[k - 1] + 1;
  }
  if (!found) return false;

  // ---- the jobs: a row's T groups, then its S groups; a hub row's overflow is its second job ----
  Gram3JobsHost& J = out->jobs;
  J.nq = nq;
  J.njobs = 0;
  J.nquads = 0;
  J.desc.clear();
  int npairs = 0;
  for (int g = 0; g < G4; ++g) {
    std::vector<int> slots;
    for (int h = 0; h < G4; ++h) slots.push_back(G4 + h);
    slots.insert(slots.end(), srow[g].begin(), srow[g].end());
    npairs += (int)srow[g].size();
    const int jobs_g = is_hub[g] ? 2 : 1;
    if ((int)slots.size() > jobs_g * 4 * nq) return false;
    J.nquads += ((int)slots.size() + 3) / 4;
    for (int jb = 0; jb < jobs_g; ++jb) {
      J.desc.push_back((uint32_t)g | ((uint32_t)g << 8) | ((uint32_t)nq << 16));
      for (int q = 0; q < nq; ++q) {
        uint32_t packed = 0;
        for (int k = 0; k < 4; ++k) {
          const size_t idx = (size_t)(jb * nq + q) * 4 + k;
          packed |= (uint32_t)(idx < slots.size() ? slots[idx] : ZG) << (8 * k);
        }
        J.desc.push_back(packed);
      }
      ++J.njobs;
    }
  }
  if (J.njobs != njobs) return false;
  out->npairs = npairs;
  out->nmonos = nm;
  if (!gram3_cover_sources(mono, nm, N, true, out)) return false;
  if (hubs) *hubs = hub;
  return true;
}
