// Lift slot table of the Kronecker Gram kernel (kp_gram3.hip, the in-kernel-lift monomial form), host only - a stand-alone
// program can include it (tools/gram3_lift_order_check.cpp), like kp_gram3_cover.h.
//
// A tile's lift is 4 (2 nfull + NWT - 1) jobs - (item, snapshot pair): an item is a column of psi_x, a column of psi_y or one of
// the NWT - 1 Kronecker weights u_x u_y - dealt over 3 lift steps of 256 slots (thread tid serves slots tid, tid + 256, tid + 512).
// A job multiplies up to three power-table entries; most have fewer REAL factors (entries other than the constant 1.0), and a
// multiply by 1.0 on the vector pipe costs what any other costs (nothing there overlaps the f64 MFMA stream).  The ordered table
// puts every job of three real factors into step 0 and gives each job its real factors first, so that steps 1 and 2 read two
// entries and multiply once:
//   step 0:     (f0 * f1) * f2        three-factor jobs keep the recipe's order: the same bits
//   steps 1, 2:  fa * fb              the surviving factors in recipe order; a dropped factor is exactly 1.0: the same bits
// (past Ns every power and the constant entry are 0.0: a product of zeros either way).
// Today's order is job e = tid + 256 j in slot e, job e = (item e % nitems, pair e / nitems).
#pragma once
#include <cstdint>
#include <vector>

#define GRAM3_LIFT_STEPS 3
#define GRAM3_LIFT_SLOTS (GRAM3_LIFT_STEPS * 256)
#define GRAM3_LIFT_IDLE 0xffffffffu

// Slot word: item | pair << 8 | p0 << 10 | p1 << 12 | p2 << 14 | nreal << 16.  p_f = which of the job's three factors in
// RECIPE order (a column: byte p of its recipe; a weight u_x u_y: 0 = u_x, 1 = u_y, 2 = none) is multiplied in as factor f,
// 3 = the constant 1.0; nreal = the job's real factors (the kernel does not read it).  GRAM3_LIFT_IDLE: no job.
static inline uint32_t gram3_lift_word(int item, int pair, const int p[3], int nreal) {
  return (uint32_t)item | (uint32_t)pair << 8 | (uint32_t)p[0] << 10 | (uint32_t)p[1] << 12 | (uint32_t)p[2] << 14 | (uint32_t)nreal << 16;
}

// which factors of an item are real, in recipe order.  Weight w + 1 in the (x <= y) order of kp_gram3_kernel is u_x u_y, u_0 = 1.
static inline void gram3_lift_factors(const uint32_t* recipes, int nfull, int bm, int item, bool real[3]) {
  if (item < 2 * nfull) {
    const uint32_t r = recipes[item < nfull ? item : item - nfull];
    for (int f = 0; f < 3; ++f) real[f] = ((r >> (8 * f)) & 255u) != 255u;
    return;
  }
  const int lw = item - 2 * nfull;
  int cnt = 0;
  real[0] = real[1] = real[2] = false;
  for (int x = 0; x <= bm; ++x)
    for (int y = x; y <= bm; ++y) {
      if (cnt == lw + 1) {
        real[0] = x > 0;
        real[1] = y > 0;
      }
      ++cnt;
    }
}

struct Gram3LiftOrderHost {
  bool ordered = false;              // false: the dictionary keeps today's order, slot is empty
  int njobs = 0, heavy = 0, two = 0, light = 0;   // jobs; of three, of two, of one or no real factors
  std::vector<uint32_t> slot;        // GRAM3_LIFT_SLOTS words
};

// recipes[nfull]: three 8-bit table ids per column in the low bytes (255 = the constant); bm inputs.  Returns out->ordered.
// Refused (today's order stays): more than 192 items (the kernel is not applicable), a column with a fourth factor, or more jobs
// of three real factors than step 0 has slots.
static inline bool gram3_lift_order_build(const uint32_t* recipes, int nfull, int bm, Gram3LiftOrderHost* out) {
  *out = Gram3LiftOrderHost();
  if (nfull < 1 || bm < 1 || bm > 3) return false;
  const int nwt = (bm + 1) * (bm + 2) / 2, nitems = 2 * nfull + nwt - 1;
  out->njobs = 4 * nitems;
  if (out->njobs > GRAM3_LIFT_SLOTS) return false;
  for (int c = 0; c < nfull; ++c)
    if ((recipes[c] >> 24) != 255u) return false;
  // jobs in today's order e = pair * nitems + item; a stable split keeps neighbouring lanes on neighbouring columns
  std::vector<uint32_t> heavy, rest;
  for (int e = 0; e < out->njobs; ++e) {
    const int pair = e / nitems, item = e - pair * nitems;
    bool real[3];
    gram3_lift_factors(recipes, nfull, bm, item, real);
    int p[3] = {3, 3, 3}, n = 0;
    for (int f = 0; f < 3; ++f)
      if (real[f]) p[n++] = f;
    const uint32_t w = gram3_lift_word(item, pair, p, n);
    if (n == 3) {
      heavy.push_back(w);
      ++out->heavy;
    } else {
      rest.push_back(w);
      ++(n == 2 ? out->two : out->light);
    }
  }
  if (heavy.size() > 256) return false;
  out->slot = heavy;
  out->slot.insert(out->slot.end(), rest.begin(), rest.end());
  out->slot.resize(GRAM3_LIFT_SLOTS, GRAM3_LIFT_IDLE);
  out->ordered = true;
  return true;
}
