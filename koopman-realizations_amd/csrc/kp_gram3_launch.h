// Host decisions of a launch of the Kronecker Gram kernel (kp_gram3_kernel, kp_gram3.hip): which FORM of the kernel runs, with
// what GEOMETRY, and what the "what ran" timer slots say about it.  Plain C++, no HIP: tools/gram3_launch_check.cpp prints all
// three on the host and tests/test_gram3_launch_plan.py pins them without a device.  gram3_launch_n (kp_gram3.hip) fills the
// facts and the switches, asks here, and launches what it is told; kp_gram3_groupable asks the same geometry.
//
// Also here, because kernel and launcher share them: the kernel's LDS layout constants and the tile timing of its early barrier.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>

#define KT3 8     // snapshots per LDS tile (two k-steps)
#define NF3 3     // single-variable powers per column (recipes with 4 factors use the general monomial kernel)
// LDS row (doubles): psi_x [0,96) | psi_y [96,192) | zero group [192,196) | weights [196,208) | scratch [208,240)
#define RS3 240   // = 16 mod 32: the four k-rows of an MFMA operand read hit disjoint banks
#define YOFF3 96
#define ZOFF3 192
#define WOFF3 196
#define SOFF3 208
#define NIDMAX3 144                 // power-table entries per snapshot (2 x 16 rows x 4 powers + the constant row's 4 fit)
#define PST3 10                     // doubles per power-table entry: KT3 snapshots + 2 of padding, so that the 16-byte reads of
                                    // 64 lanes with arbitrary ids spread over all banks (a stride of 8 puts them on 4 groups)
#define POWBUF3 (PST3 * NIDMAX3)    // doubles per power-table buffer
#define PSIBUF3 (KT3 * RS3)         // doubles per Psi buffer
#define PSI03 (2 * POWBUF3)         // LDS: pow[2] | psi[2]
#define LDS3_DOUBLES (PSI03 + 2 * PSIBUF3)
// dim_red dictionaries: the projection matrix lives behind the Psi buffers as [column tile of 16 PCs][full column][16]
// (row stride 16 doubles: the two full columns a 32-lane group reads sit on disjoint banks), at most 32 PCs
#define PCS03 LDS3_DOUBLES
#define PCSMAX3 32
#define LDS3_PCS_DOUBLES (2 * YOFF3 * 16)
// fourier / gaussian dictionaries (EXT): the per-variable table also holds cos / sin(2 pi j x) behind the powers, and one
// entry per (side, gaussian centre) behind the constant; the centres live in LDS where the projection matrix would
#define GC03 LDS3_DOUBLES
#define GAUSSMAX3 32                // centres (2 sides x 32 x KT3 values per tile = two items per thread)
#define GNZMAX3 8                   // state variables of a gaussian dictionary
#define LDS3_GAUSS_DOUBLES (GAUSSMAX3 * GNZMAX3)

// EB (the early tile barrier of kp_gram3_kernel): where a tile of NQ quads per wave places its barrier and how it
// times the lift's three chunks.  One function for the kernel and for the launcher, so that the timer slot tells what ran.
#ifndef KP_GRAM3_EB_BEHIND
#define KP_GRAM3_EB_BEHIND 0        // quad steps of a tile that run behind its barrier; 0: as many as B operands are requested ahead
#endif
struct Gram3TileTiming {
  int pf;        // B operands are requested this many quad steps ahead
  int sp, lag;   // lift chunk i: table reads at step i sp, multiplies and stores at step i sp + lag
  int bs;        // step whose end holds the tile's barrier; -1: the barrier stays behind the last step (today's placement)
};
constexpr Gram3TileTiming gram3_tile_timing(int nq, bool lo, bool eb) {
  const int nstep = (KT3 / 4) * nq, nch = 3;
  const int pf_ahead = lo ? 2 : 3;                      // (2 and 4 steps ahead measured the same; LO: four registers for the lift's addresses)
  const int pf = nstep < pf_ahead ? nstep : pf_ahead;
  const int sp = nstep / nch > 0 ? nstep / nch : 1;
  const int lag = sp / 2 > 0 ? sp / 2 : 1;
  // (with the ordered lift only: the order e = tid + 256 j requests B operands three steps ahead and does not pin its twelve
  // lift addresses - with operands carried across the tile boundary its NQ = 6 loops hold 14 to 16 scratch accesses each)
  if (eb && lo) {
    // the barrier step: every operand read of the tile is issued at or before it (B operands run pf steps ahead) unless fewer
    // steps are asked to stay behind it; it must lie in the tile's last k-step (the A fragments and weights of every k-step are
    // requested by then) and at or behind the last lift store.  The chunks move together - the largest spacing of at least
    // two steps that fits, the lag kept - and where none fits the placement is today's: a compile-time matter, never a hazard.
    const int behind = KP_GRAM3_EB_BEHIND > 0 && KP_GRAM3_EB_BEHIND < pf ? KP_GRAM3_EB_BEHIND : pf;
    const int bs = nstep - 1 - behind;
    for (int s = sp; s >= 2; --s) {
      const int l = lag < s ? lag : s;
      if (bs >= (KT3 / 4 - 1) * nq && (nch - 1) * s + l <= bs) return {pf, s, l, bs};
    }
  }
  return {pf, sp, lag, -1};
}

// What a launch's decisions read, as plain values (gram3_facts in kp_gram3.hip fills them from kp_basis, the plan and the context).
struct Gram3Facts {
  // the dictionary (BasisDev / kp_basis)
  int N = 0, m = 0, nfull = 0, nzeta = 0, k_pcs = 0, pow_depth = 0;
  bool fast = false, fast_ext = false;
  int ext_Dp = 0, ext_df = 0, ext_ng = 0;
  bool lift_table = false;      // it has a lift slot table (kp_gram3_lift.h); asked only where gram3_mono says the form can use one
  // the plan this launch runs, and the dictionary's other plan (circulant / cover; all 0: it has one plan)
  int nq = 0, nsuper = 0, njobs = 0, two_group_jobs = 0;
  int other_nq = 0, other_nsuper = 0, other_njobs = 0;
  // the launch: snapshots per fit, fits; the chip
  int64_t Ns = 0;
  int n = 1;
  int num_cu = 0, wg_per_cu = 2;       // (num_cu as the context reports it, 0: unknown)
  int64_t hbm_bytes = 0;
};

// The switches (environment variables; kp_gram3.hip: gram3_switches reads each where and as often as its comment there says)
struct Gram3Switches {
  bool ext = true;                 // KP_NO_GRAM3_EXT unset
  bool prelift = true;             // KP_GRAM3_NO_PRELIFT unset
  int64_t pre_min_ns = 6000;       // KP_GRAM3_PRELIFT_MIN_NS
  bool pow3 = true;                // KP_GRAM3_POW3 != 0
  bool lift_order = true;          // KP_GRAM3_LIFT_ORDER != 0
  bool early_barrier = true;       // KP_GRAM3_EARLY_BARRIER != 0
};

// The switches from the texts of their variables (get(name): the text, or nullptr where it is unset)
template <class Get>
inline Gram3Switches gram3_switches_read(Get get) {
  auto on = [&](const char* name) { const char* e = get(name); return !e || atoi(e) != 0; };
  Gram3Switches s;
  s.ext = get("KP_NO_GRAM3_EXT") == nullptr;
  s.prelift = get("KP_GRAM3_NO_PRELIFT") == nullptr;
  if (const char* e = get("KP_GRAM3_PRELIFT_MIN_NS")) s.pre_min_ns = (int64_t)atoll(e);
  s.pow3 = on("KP_GRAM3_POW3");
  s.lift_order = on("KP_GRAM3_LIFT_ORDER");
  s.early_barrier = on("KP_GRAM3_EARLY_BARRIER");
  return s;
}

// fourier / gaussian blocks as table entries (EXT kernel): not with a projection, <= GAUSSMAX3 centres, <= GNZMAX3 variables
inline bool gram3_ext(const Gram3Facts& f, const Gram3Switches& sw) {
  return f.fast_ext && (f.ext_df > 0 || f.ext_ng > 0) && f.k_pcs == 0 && f.ext_ng <= GAUSSMAX3 && (f.ext_ng == 0 || f.nzeta <= GNZMAX3) && sw.ext;
}

// dim_red dictionaries: econ lift by kp_gram3_prelift_kernel (its power table: 2 x nzeta * depth entries x 256 threads of LDS);
// fourier / gaussian dictionaries: their table entries once per snapshot by kp_gram3_prelift_ext_kernel (kp_gram3_prelift.hip)
inline bool gram3_prelift(const Gram3Facts& f, const Gram3Switches& sw) {
  if (!sw.prelift) return false;
  if ((f.N + 3) / 4 > 14) return false;               // the tile loader of the PRE kernel moves two 16-byte pieces per thread: 4 (8 G4 + 12) <= 512
  if (f.k_pcs > 0) return f.k_pcs <= 32 && f.fast && f.nzeta * f.pow_depth <= 24;      // (2 x 24 entries x 256 threads: 96 KB of LDS)
  return gram3_ext(f, sw) && f.nzeta <= 16 && f.nzeta * (f.ext_Dp + 2 * f.ext_df) + f.ext_ng + 1 <= 64;
}

// The in-kernel-lift monomial form (the kernel's GRP): the tile loop builds the power table (the kernel's INL: no fourier /
// gaussian table entries, no prelift buffer) and there is no projection.  P3, LO, EB, the fits that share a launch and the cover
// plan exist in this form only.  gram3_prelift serves projections and fourier / gaussian tables, so no launch of such a
// dictionary has a prelift buffer: this is a property of the dictionary.
inline bool gram3_mono(const Gram3Facts& f, const Gram3Switches& sw) { return !gram3_ext(f, sw) && f.k_pcs == 0; }

enum Gram3Kind {
  GRAM3_MONO = 0,   // in-kernel lift, monomial columns
  GRAM3_PCS = 1,    // in-kernel lift and projection (dim_red dictionaries)
  GRAM3_EXT = 2,    // fourier / gaussian entries in the in-kernel table
  GRAM3_PRE = 3     // tiles lifted by a prelift kernel (`ext`: kp_gram3_prelift_ext_kernel, else kp_gram3_prelift_kernel)
};

struct Gram3Form {
  Gram3Kind kind = GRAM3_MONO;
  bool ext = false;                // the dictionary's table holds fourier / gaussian entries (EXT recipes; with GRAM3_PRE: its prelift kernel)
  int nq = 0, bm = 0;              // the kernel's NQ and BM
  bool p3 = false, lo = false, eb = false;
  bool want_buffer = false;        // a prelift buffer of pre_bytes is wanted: without one (buffer_ok = false) the form is an in-kernel one
  size_t pre_bytes = 0;
  int pre_rl = 0;                  // entries per snapshot of the prelift buffer
  const char* refusal = nullptr;   // nullptr, or why this launch cannot be made
};

inline int64_t gram3_ktiles(int64_t Ns) { return (Ns + KT3 - 1) / KT3; }

// The form of a launch.  The launcher asks once (buffer_ok = true), tries the workspace where want_buffer says so, and asks again
// with what it got.
inline Gram3Form gram3_form(const Gram3Facts& f, const Gram3Switches& sw, bool buffer_ok) {
  Gram3Form F;
  F.ext = gram3_ext(f, sw);
  F.nq = f.nq;
  F.bm = f.m;
  const bool mono = gram3_mono(f, sw);
  if (f.n > 1 && !mono) {
    F.refusal = "kp_fit_gram: these fits cannot share a launch";
    return F;
  }
  // dim_red dictionaries: the econ lift once per snapshot into a row buffer (kp_gram3_prelift.hip), the Gram kernel loads tiles of it.
  // Round 4's prelift kernel walked its 84 columns in ~40 us however few threads ran, so the in-kernel projection won below
  // ~45 000 pairs; round 5's works tile by tile: at the arm data's 11 999 pairs 0.040 against 0.053 ms of kernels
  // (tools/arm_shape_latency.py with KP_GRAM3_PRELIFT_MIN_NS=0).  Below a few thousand pairs the second launch is not worth it.
  bool pre = gram3_prelift(f, sw) && f.Ns >= sw.pre_min_ns;
  F.pre_rl = 8 * ((f.N + 3) / 4) + 12;
  if (pre) {
    // the row buffer is ~0.7 - 1 KB per snapshot (7 - 10 GB at 1e7 pairs), in one piece: when it is more than a quarter of the
    // device's memory, or cannot be had (a busy device, several contexts of a kp_multi on one GPU), the fit runs with the
    // in-kernel lift instead of failing - same Grams, no buffer
    F.pre_bytes = (size_t)gram3_ktiles(f.Ns) * KT3 * F.pre_rl * 8;
    if (f.hbm_bytes > 0 && F.pre_bytes > (size_t)f.hbm_bytes / 4) pre = false;
    F.want_buffer = pre;
    if (!buffer_ok) pre = false;
  }
  F.kind = pre ? GRAM3_PRE : f.k_pcs > 0 ? GRAM3_PCS : F.ext ? GRAM3_EXT : GRAM3_MONO;
  // the in-kernel-lift monomial form: three table entries where no recipe reads a fourth
  F.p3 = mono && f.pow_depth <= 3 && sw.pow3;
  // ... and, in the same form, the lift's jobs in the slots of the dictionary's table (LO) where it has one
  F.lo = mono && sw.lift_order && f.lift_table;
  // ... and, with the ordered lift, the tile's barrier in front of its last quad steps (EB) where the tile has the room.  Not for
  // a plan with jobs of two A groups at NQ = 6, m = 3: those waves carry a second A fragment across the tile boundary, and two
  // of their five tile loops then reload registers from scratch (the register table; one-A-group plans, fewer
  // quads and fewer weights have none)
  F.eb = mono && sw.early_barrier && gram3_tile_timing(f.nq, F.lo, true).bs >= 0 && (f.two_group_jobs == 0 || f.nq < 6 || f.m < 3);
  return F;
}

struct Gram3Geometry {
  int64_t ktiles = 0;              // tiles of KT3 snapshots per fit
  int nsplit = 1, kps = 1;         // snapshot splits per fit, tiles per split
  int grid = 0;                    // nsuper workgroups per split, n fits
  size_t part_bytes = 0;           // the split partials this launch writes
  size_t ws4_bytes = 0;            // workspace 4: the partials of the largest split count of either plan of the dictionary
  int reduce_block = 256;          // threads per workgroup of kp_gram3_reduce_kernel
};

// workgroup slots of the chip for kp_gram3_kernel (__launch_bounds__(256, 2): two workgroups share a CU)
inline int64_t gram3_slots(const Gram3Facts& f) { return (int64_t)std::max(8, f.num_cu > 0 ? f.num_cu : 256) * f.wg_per_cu; }

// The launch is dealt over the fits: nsplit = max(1, (slots / nsuper) / n) splits each, then as many as ceil(ktiles / kps) needs.
inline Gram3Geometry gram3_geometry(const Gram3Facts& f) {
  Gram3Geometry g;
  const int nwt = (f.m + 1) * (f.m + 2) / 2;
  const int ncu = f.num_cu > 0 ? f.num_cu : 256;
  const int64_t slots = gram3_slots(f);
  g.ktiles = gram3_ktiles(f.Ns);
  // (per fit: the fits of a group launch share the chip)
  g.nsplit = (int)std::max<int64_t>(1, std::min<int64_t>(g.ktiles, slots / f.nsuper / f.n > 0 ? slots / f.nsuper / f.n : 1));
  g.kps = (int)((g.ktiles + g.nsplit - 1) / g.nsplit);
  if (g.kps < 1) g.kps = 1;
  g.nsplit = (int)std::max<int64_t>(1, (g.ktiles + g.kps - 1) / g.kps);
  g.grid = f.nsuper * g.nsplit * f.n;
  const size_t per_split = (size_t)f.njobs * f.nq * nwt * 64;
  g.part_bytes = (size_t)f.n * g.nsplit * per_split * 8;
  // the split partials (workspace 4), sized for the largest split count of this dictionary at once: a workspace that grows
  // with the snapshot count would put a hipFree + hipMalloc of ~80 MB (17 ms, and a device synchronisation) into the first large fit of a running pipeline
  // (... and for both plans of the dictionary: synchronous and pipelined fits of it may alternate, whichever comes first)
  g.ws4_bytes = ((size_t)std::max<int64_t>((int64_t)f.n * g.nsplit, (int64_t)ncu * f.wg_per_cu / f.nsuper) * per_split * 8 + 255) & ~(size_t)255;
  if (f.other_nsuper > 0)
    g.ws4_bytes = std::max(g.ws4_bytes, ((size_t)((int64_t)ncu * f.wg_per_cu / f.other_nsuper) * f.other_njobs * f.other_nq * nwt * 64 * 8 + 255) & ~(size_t)255);
  g.reduce_block = g.nsplit >= 128 ? 1024 : g.nsplit >= 32 ? 512 : 256;
  return g;
}

// dynamic LDS bytes of the kernel in this form
inline size_t gram3_lds_bytes(const Gram3Facts& f, const Gram3Form& F) {
  const int nfull4 = (f.nfull + 3) / 4 * 4;
  return (size_t)(LDS3_DOUBLES + (F.kind == GRAM3_PCS ? 2 * nfull4 * 16 : 0) + (F.kind == GRAM3_EXT ? LDS3_GAUSS_DOUBLES : 0)) * sizeof(double);
}

// Fits may share a launch only while a LONE launch's splits are shorter than max_kps tiles (kp_gram3_groupable; f.n = 1)
inline bool gram3_lone_splits_shorter(const Gram3Facts& f, int64_t max_kps) {
  const Gram3Geometry g = gram3_geometry(f);
  return std::min<int64_t>(g.ktiles, g.kps) < max_kps;     // (kps <= ktiles but for no tiles at all: 0)
}

// What the launch ran, for kp_timer_get
struct Gram3Ran {
  // timer 10: executed on the matrix pipe per pair, of the plan THIS launch ran: jobs (padding included) x quads x weights MFMAs per 4 snapshots, 512 flop
  // each; dim_red: + the projection pcs' psi of every workgroup of a split (2 x nfull4 / 4 MFMAs per wave and tile)
  double mfma_flop_per_pair = 0.0;
  double two_group_jobs = 0.0;     // timer 15: jobs of this launch's plan that span two A groups (0: a one-A-group plan)
  double table_entries = 0.0;      // timer 16: table entries per raw value that the in-loop build of this launch's kernel writes (0: a form without that build)
  double lift_order = 0.0;         // timer 20: 1 the dictionary's slot table, 0 the order e = tid + 256 j (a form without the in-kernel monomial lift too)
  double early_barrier = 0.0;      // timer 26: where this launch's tiles had their barrier: 1 in front of the last quad steps, 0 behind the last one
};

inline Gram3Ran gram3_ran(const Gram3Facts& f, const Gram3Form& F) {
  Gram3Ran r;
  const int nwt = (f.m + 1) * (f.m + 2) / 2, nfull4 = (f.nfull + 3) / 4 * 4;
  r.mfma_flop_per_pair = (double)f.njobs * f.nq * nwt * 128.0 + (F.kind == GRAM3_PCS ? (double)f.nsuper * nfull4 * 128.0 : 0.0);
  r.two_group_jobs = (double)f.two_group_jobs;
  r.table_entries = F.kind == GRAM3_PRE || F.kind == GRAM3_EXT ? 0.0 : F.p3 ? 3.0 : 4.0;
  r.lift_order = F.lo ? 1.0 : 0.0;
  r.early_barrier = F.eb ? 1.0 : 0.0;
  return r;
}
