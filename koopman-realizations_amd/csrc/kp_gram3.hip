// Fused lift + Gram kernel for BILINEAR monomial dictionaries, exploiting the Kronecker
// structure of the bilinear rows  Psi = psi (x) [1; u]  (Ksysid.m:510-511, 1594-1604):
//
//   Px'Px = sum_k (ut ut') (x) (psi_x psi_x')     Px'Py = sum_k (ut ut') (x) (psi_x psi_y')
//
// with ut = [1; u_k].  Only the (m+1)(m+2)/2 distinct weights w_ab = ut_a ut_b are needed, and
// only psi (N columns per side, not N(m+1)) is lifted into LDS.  For every weight the kernel
// accumulates  S_w = sum_k w psi_x psi_x'  (symmetric: circulant half) and T_w = sum_k w psi_x psi_y'
// in 4x4 blocks with v_mfma_f64_4x4x4_4b_f64:  A = one 4-column group of psi_x scaled by the
// weight (one v_mul per group and weight), B = four 4-column groups of [psi_x | psi_y]
// (one LDS read feeds all weights).  Executed flops are 62.5 % of the dense W x W products the
// reference forms (W = N(m+1)); the result is the same matrices G = Px'Px, C = Px'Py.
//
// Design rule this kernel is built around (tools/mfma_coissue_bench.hip, profiles/r01_coissue.txt):
// on gfx950 NO VALU instruction (integer or floating point) overlaps with the FP64 MFMA stream of
// its SIMD -- each costs ~5.5 cycles of MFMA time even with two waves per SIMD -- while LDS reads
// are free up to about one per MFMA.  So the LDS layout is a compile-time constant (every operand
// read is `ds_read_b64 v, vaddr offset:imm`, the tile loop is unrolled by two so that the buffer
// index is an immediate too), the weights ut_a ut_b come from LDS (written once per snapshot by the
// lift) and the tail mask lives in the power table's constant entry.
//
// Round 6 (0.396 -> 0.358 ms per 1e5 pairs at W = 336; what each step gave is in DESIGN.md 3.1 "Round 6", measured with the
// timing-only builds (removed; see HISTORY.md): MFMAs and their operand reads alone take 0.305 ms):
//  * m = 3: TWO weights per weighted A operand (TUP below) - 5 weight multiplies per A group and k-step instead of 9;
//  * the power table of the tile after next is built INSIDE the MFMA loop by every thread, branch-free (x .. x^4 at a
//    compile-time entry stride, raw value loaded a tile ahead; INL), not behind it with a run-time loop and exec masks;
//  * the Kronecker weights are lifted like columns (no separate step at the head of the tile);
//  * LDS traffic is NOT free at this instruction mix: table rows at a stride of 62 doubles (bank conflicts of the lift's
//    16-byte reads 77 -> 57 cycles per chunk), a lane's five tuple weights contiguous (two 16-byte reads and one 8-byte read
//    instead of the ds_read2_b64 pairs the compiler formed at half the LDS rate);
//  * the lift's (item, snapshot pair) jobs dealt over 3 x 256 slots: three lift steps per tile instead of four;
//  * the first three raw tiles requested in front of the one-time LDS setup.
// Measured and NOT kept: lift stores as two ds_write_b64 at immediate offsets instead of ds_write2_b64 + v_add (slower: 0.3718
// against 0.3659 ms), the k-step's weights kept in registers across the wave's two A groups (slower), 7 quads per wave
// (147 spilled registers), the items with three real factors gathered in the last wave so that the others skip a read and a multiply (branches and the
// scattered stores cost more), B operands 2 / 4 steps ahead and the raw load behind other steps (no difference), cbsz / abid
// (they do not broadcast blocks on v_mfma_f64_4x4x4_4b: tools/mfma_bcast_probe.hip).
// Later, on the one-A-group plan: a dictionary without fourth powers runs a form whose in-loop table build writes
// three entries, not four (P3: 0.3068 -> 0.3044 ms per fit, kept).  Measured and NOT kept THEN: the lift's jobs in an order built on
// the host, every job of three real factors in lift step 0, so that steps 1 and 2 read two factors and multiply once - 4 v_mul_f64
// and 2 ds_read_b128 less per wave and tile, but the compiler then reloads 5 spilled address registers inside every tile (none
// before), behind the tile's raw load in the vmcnt order: 0.3068 -> 0.3127 ms.  Kept since DESIGN 6.7 (LO below): with the lift's
// LDS byte addresses formed once and passed through an empty asm at the top of the tile body no tile loop holds a scratch
// access and the loop is 5.5 vector instructions per wave and tile shorter: 0.2884 -> 0.2844 ms of kernel per fit.
// DESIGN 6.8 (EB below): the tile's barrier in front of its last two quad steps, the next tile's first operands requested right
// behind it - every wave's operand pipeline used to drain at the barrier and refill in front of five weight multiplies; the
// same instructions and bits.
//
// Replaces the per-row lift loop of Ksysid.get_Koopman (Ksysid.m:1030-1065) and the products
// PxTPx, PxTPy (Ksysid.m:1114,1125) for model_type 'bilinear'.
#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "kp_internal.h"

#ifndef KP_RAW_STEP
#define KP_RAW_STEP 1   // MFMA step of a tile behind which the raw loads of the tile after next are issued
#endif
// (the LDS layout constants KT3 .. LDS3_GAUSS_DOUBLES and gram3_tile_timing: kp_gram3_launch.h, shared with the launch decisions)
#ifndef KP_PCS_REGS
#define KP_PCS_REGS 24                 // k-steps of the pcs projection whose matrix operand stays in registers (<= 96 full columns)
#endif

#include "kp_gram3_args.h"
#include "kp_gram3_cover.h"
#include "kp_gram3_lift.h"
#include "kp_gram3_launch.h"

// the constant row of the in-loop power table "loads" its 1.0 like the raw rows load their values (kp_gram3_kernel, INL); not
// `const`: a pointer that may be this or a kernel argument must stay a GLOBAL pointer (constant address space: flat loads)
__device__ double kp_gram3_ones[KT3] = {1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0};

// PCS: econ lift through a projection matrix (dim_red dictionaries)
// EXT: fourier (def_fourierLift, Ksysid.m:694-731) and gaussian (def_gaussianLift, :790-817) blocks through the same table
// TUP (round 6; m = 3 and m = 2: an even number of weights): the four blocks of a weighted A operand carry TWO weights - tuple p = (w_2p, w_2p, w_2p+1, w_2p+1) -
// against B operands (g0, g1, g0, g1) and (g2, g3, g2, g3) of the quad: the same 10 MFMAs per quad and k-step produce the same
// 40 (weight, group) blocks, bit for bit, with 5 weight multiplies per A group and k-step instead of 9 (nothing on the vector
// pipe overlaps the f64 MFMA stream: each costs ~5.5 cycles of it) and 10 operand registers less; the price is a second
// operand read per quad.  The weights sit in the 12 weight entries of a Psi row in tuple order (wslot), w_0 = 1 stored.
// P3 (the in-kernel-lift monomial form without a projection; dictionaries of powers <= 3): the in-loop table build writes x, x^2, x^3 and no
// x^4 entry that nothing reads - a v_mul_f64 and a ds_write_b64 less per wave and tile.
// LO (the same form; kp_gram3_lift.h): the lift's jobs sit in the slots of a table built on the host - every job of three
// real factors in lift step 0, real factors first - so that lift steps 1 and 2 read two table entries and multiply once: 4
// v_mul_f64 and 2 ds_read_b128 less per wave and tile, the same bits (a dropped factor is exactly 1.0).
// EB (the same form, every plan): the tile's barrier sits at the end of quad step NSTEP - 1 - PF, not
// behind the last one, the lift's chunks finish in front of it, and the operand reads that found nothing left to request (the
// last PF steps' B operands, the last k-step's A fragment and weights) request the NEXT tile's first operands from the other
// Psi buffer: the tile's last PF steps of MFMAs run from registers over that latency, and the next tile opens with its
// operands present instead of a drained pipeline behind a barrier.  The same instructions, the same accumulation order.
// gram3_tile_timing says which tiles take it (the ordered lift LO with NQ = 4, 5, 6); the others keep today's tile.
template <int NQ, int BM, bool PCS, bool EXT = false, bool PRE = false, bool P3 = false, bool LO = false, bool EB = false>
__global__ __launch_bounds__(256, 2) void kp_gram3_kernel(Gram3Args a) {
  constexpr int NWT = (BM + 1) * (BM + 2) / 2;
  constexpr bool TUP = BM >= 2;
  static_assert(!EB || (!PCS && !EXT && !PRE), "early tile barrier: the in-kernel-lift monomial form");
  static_assert(!P3 || (!PCS && !EXT && !PRE), "three-entry table: the in-kernel-lift monomial form");
  static_assert(!LO || (!PCS && !EXT && !PRE), "ordered lift slots: the in-kernel-lift monomial form");
  static_assert(!TUP || NWT % 2 == 0, "paired weights: an even number of weights (m = 3: 10 = 5 tuples, m = 2: 6 = 3 tuples)");
  // TUP: weight w sits in slot 6 (w & 1) + (w >> 1) of the 12 weight entries of a Psi row (w_0 = 1 stored in slot 0): the five
  // weights a lane multiplies in - w_{2p+h}, p = 0..4, h = blk >> 1 - are contiguous and 16-byte aligned (two ds_read_b128 and a
  // ds_read_b64; as 8-byte reads at stride 2 the compiler paired them into ds_read2_b64, half the LDS rate)
  auto wslot = [](int w) { return TUP ? 6 * (w & 1) + (w >> 1) : w - 1; };
  extern __shared__ __align__(16) double sm[];
  const BasisDev& b = a.b;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  // XCD-aware order: workgroups b and b + 8 share an XCD (round-robin dispatch) and its L2, so consecutive LOGICAL ids -
  // the nsuper workgroups of one snapshot split, which read the same raw tiles - are dealt to one XCD: the tile is
  // fetched from HBM once per split instead of once per workgroup (a speed matter only; any mapping is correct)
  const int per_xcd = gridDim.x / 8;
  const int logical = (int)blockIdx.x < per_xcd * 8 ? ((int)blockIdx.x % 8) * per_xcd + (int)blockIdx.x / 8 : (int)blockIdx.x;
  const int super = logical % a.nsuper;
  const int split = logical / a.nsuper;
  // Pipelined fits that share the launch (INL form without a projection; kp_fit.hip's Gram queue): fit `fit` owns the global
  // splits [fit nsplit_fit, (fit + 1) nsplit_fit) - it walks ITS snapshots in nsplit_fit pieces and reads its own arrays, and its
  // partials land at the global split index, where the reduction finds them.  Both are wave-uniform (scalar).
  constexpr bool GRP = !PCS && !EXT && !PRE;
  const int fit = GRP ? __builtin_amdgcn_readfirstlane(split / a.nsplit_fit) : 0;
  const int split_local = split - fit * a.nsplit_fit;
  const double* const src_alpha = GRP ? a.grp[fit].alpha : a.alpha;
  const double* const src_beta = GRP ? a.grp[fit].beta : a.beta;
  const double* const src_u = GRP ? a.grp[fit].u : a.u;
  const int job = super * 4 + wave;
  const int nzm = b.nzeta + b.m;
  const int nrawrows = 2 * nzm;
  const int D = a.D;
  // INL (monomial dictionaries lifted in the kernel): the power table of the tile after next is built INSIDE the MFMA loop -
  // branch-free, four powers per raw value at a compile-time entry stride - instead of behind it (round 6: the end-of-tile
  // build with its run-time power loop, its exec-mask branches and its wait for the raw load cost 29 of 389 us, timing-only
  // build; removed, see HISTORY.md).  kp_gram3_applicable admits monomial dictionaries with powers <= 4 only (others: kp_gram2 / general kernel).
  constexpr bool INL = !EXT && !PRE;
  // Table layout (doubles): row r (raw rows, then the constant's row) at r * RB, its entry e at + e * PST3, KT3 snapshots each.
  // EXT keeps the dense id order of its recipes (RB = D entries).  INL: 4 entries per row and, when the table has the room, a row
  // stride of 62 doubles - the lift's 16-byte reads of 64 columns with unrelated ids then spread over the banks as well as the
  // 3-entry rows of rounds 1-5 did (57 LDS cycles per chunk of a workgroup for the poly-3 dictionary on 6 states against 77 at
  // the dense stride 40; tools/lds_layout_sim.py).
  const int RB = !INL ? D * PST3 : ((nrawrows + 1) * 62 + 4 * PST3 <= POWBUF3 ? 62 : 4 * PST3);
  const int CA = nrawrows * RB;                    // address of the constant 1 (0 for snapshots past Ns: the tail mask)

  // ---- MFMA operand offsets (doubles, Psi buffer 0): row (lane>>4) of k-step 0 ----
  const uint32_t* jd = a.desc + (size_t)job * (1 + NQ);
  const uint32_t jh = jd[0];
  const int lrow = (lane >> 4) * RS3, blk = (lane >> 2) & 3, lc = lane & 3;
  const int ao0 = PSI03 + lrow + 4 * (int)(jh & 255u) + lc;      // A group replicated over the 4 blocks
  const int ao1 = PSI03 + lrow + 4 * (int)((jh >> 8) & 255u) + lc;
  const int qs = __builtin_amdgcn_readfirstlane((int)((jh >> 16) & 255u));   // wave-uniform
  int bo[NQ];
  int bo2[TUP ? NQ : 1];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    // TUP: block b of the first B operand reads group (b & 1) of the quad, of the second one group 2 + (b & 1)
    const int g = (int)((jd[1 + q] >> (8 * (TUP ? (blk & 1) : blk))) & 255u);
    bo[q] = PSI03 + lrow + (g < a.G4 ? 4 * g : g < 2 * a.G4 ? YOFF3 + 4 * (g - a.G4) : ZOFF3) + lc;
    if (TUP) {
      const int g2 = (int)((jd[1 + q] >> (8 * (2 + (blk & 1)))) & 255u);
      bo2[q] = PSI03 + lrow + (g2 < a.G4 ? 4 * g2 : g2 < 2 * a.G4 ? YOFF3 + 4 * (g2 - a.G4) : ZOFF3) + lc;
    }
  }
  // TUP: this lane's weight of tuple p is entry 2 p + (blk >> 1)
  const int wo = PSI03 + lrow + WOFF3 + (TUP ? 6 * (blk >> 1) : 0);

  double acc[NQ][NWT];
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int w = 0; w < NWT; ++w) acc[q][w] = 0.0;

  // ---- lifting thread constants: thread = one (side, column), all KT3 snapshots of the tile ----
  // power table layout [id][snapshot]: the KT3 values of one entry are contiguous (16-byte reads of snapshot pairs)
  // The NWT - 1 Kronecker weights ut_x ut_y (pair index w + 1 in (x <= y) order) are lifted like columns: thread 2 nfull + w
  // multiplies the table entries of u_x and u_y (and the constant) for all KT3 snapshots and writes entry WOFF3 + WSH + w of the
  // Psi rows.  (Until round 6 a separate step at the head of every tile formed them: an LDS round trip and a branch in front
  // of the tile's first operand reads.)
  // item -> its three table addresses and its destination column in a Psi row
  auto item_setup = [&](int item, int (&fa_)[NF3], int& woff_) __attribute__((always_inline)) {
    const bool lvalid = item >= 0 && item < 2 * b.nfull;
    const int lside = (lvalid && item >= b.nfull) ? 1 : 0;
    const int lcol = lvalid ? item - lside * b.nfull : 0;
    const int lw = item - 2 * b.nfull;             // weight item: 0 <= lw < NWT - 1
    const bool lwt = lw >= 0 && lw < NWT - 1;
    const uint32_t r = lvalid ? a.recipes[lcol] : 0xffffffffu;
#pragma unroll
    for (int f = 0; f < NF3; ++f) {
      const int id = (int)((r >> (8 * f)) & 255u);
      fa_[f] = id == 255 ? CA : (EXT && id >= 128) ? CA + (1 + lside * a.ng + (id - 128)) * PST3 : (lside * nzm + id / D) * RB + (id % D) * PST3;
    }
    if (lwt) {
      int cnt = 0;
      for (int x = 0; x <= BM; ++x)
        for (int y = x; y <= BM; ++y) {
          if (cnt == lw + 1) {
            if (x > 0) fa_[0] = (b.nzeta + x - 1) * RB;
            if (y > 0) fa_[1] = (b.nzeta + y - 1) * RB;
          }
          ++cnt;
        }
    }
    woff_ = PSI03 + (lvalid ? lside * YOFF3 + lcol : lwt ? WOFF3 + wslot(lw + 1) : SOFF3 + (tid & 31));
  };
  // The 4 (2 nfull + NWT - 1) (item, snapshot pair) jobs of a tile dealt over 3 x 256 slots: three lift steps per tile instead of
  // four (item = thread, one step per snapshot pair: 256 lanes for 177 items at N = 84).  A slot's snapshot pair is part of its
  // addresses, not an immediate: 12 address registers per thread instead of 4.  kp_gram3_applicable: 2 nfull + NWT - 1 <= 192.
  constexpr int NLS = 3;
  int fs[NLS][NF3], ws[NLS];
  {
    const int nitems = 2 * b.nfull + NWT - 1;
#pragma unroll
    for (int j = 0; j < NLS; ++j) {
      if constexpr (LO) {
        // slot word (kp_gram3_lift.h): item | pair << 8 | three 2-bit factor sources from bit 10 (3: the constant)
        const uint32_t sw = a.lift[tid + 256 * j];
        const bool on = sw != GRAM3_LIFT_IDLE;
        const int ch = on ? (int)((sw >> 8) & 3u) : 0;
        int fr[NF3];
        item_setup(on ? (int)(sw & 255u) : -1, fr, ws[j]);
#pragma unroll
        for (int f = 0; f < NF3; ++f) {
          const int p = on ? (int)((sw >> (10 + 2 * f)) & 3u) : 3;
          fs[j][f] = (p == 0 ? fr[0] : p == 1 ? fr[1] : p == 2 ? fr[2] : CA) + 2 * ch;
        }
        ws[j] += 2 * ch * RS3;
      } else {
        const int e = tid + 256 * j;
        const bool on = e < 4 * nitems;
        const int ch = on ? e / nitems : 0;
        item_setup(on ? e - ch * nitems : -1, fs[j], ws[j]);
#pragma unroll
        for (int f = 0; f < NF3; ++f) fs[j][f] += 2 * ch;
        ws[j] += 2 * ch * RS3;
      }
    }
  }

  // LO: the lift's LDS BYTE addresses, formed once (what the tile body pins: see there)
  uint32_t fsb[NLS][NF3], wsb[NLS];
#pragma unroll
  for (int j = 0; j < NLS; ++j) {
#pragma unroll
    for (int f = 0; f < NF3; ++f) fsb[j][f] = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) double*)(sm + fs[j][f]);
    wsb[j] = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) double*)(sm + ws[j]);
  }
  const int64_t kt0 = (int64_t)split_local * a.ktiles_per_split;
  const int64_t ktiles_total = (a.Ns + KT3 - 1) / KT3;
  const int nkt = (int)max((int64_t)0, min((int64_t)a.ktiles_per_split, ktiles_total - kt0));

  // ---- raw loader; rows: [alpha(nzeta) u(m) | beta(nzeta) u(m)] ----
  // value e = tid + j*256 of a tile -> (row e / KT3, snapshot e % KT3); tiles are loaded in order, so every
  // thread keeps a running pointer and a running count of the snapshots left in its row
  constexpr int LR = 1;                             // 2 (nzeta + m) KT3 <= 256 raw values per tile (kp_gram3_applicable): one per thread
  const int nld = (nrawrows * KT3 + 255) / 256;     // wave-uniform number of active j
  constexpr int LG = EXT ? 2 : 0;                   // gaussian items (side, centre, snapshot) per thread
  struct RawRegs { double v[LR]; bool ok; };
  bool ld_on[LR];
  bool ld_isz[LR];                                  // row of a state variable (EXT: gets the trigonometric entries)
  const double* ld_ptr[LR];
  const int ld_s = tid & (KT3 - 1);                 // the same snapshot for every j (256 is a multiple of KT3)
  const int ld_dst0 = (tid / KT3) * RB + ld_s;
  int ld_rem = (int)max((int64_t)-1000000, min((int64_t)1 << 30, a.Ns - (kt0 * KT3 + ld_s)));
#pragma unroll
  for (int j = 0; j < LR; ++j) {
    const int e = tid + j * 256;
    ld_on[j] = e < nrawrows * KT3;
    const int r = ld_on[j] ? e / KT3 : 0;
    const int rr = r % nzm;
    const double* src = rr < b.nzeta ? ((r < nzm ? src_alpha : src_beta) + (int64_t)rr * a.Ns) : (src_u + (int64_t)(rr - b.nzeta) * a.Ns);
    ld_ptr[j] = src + kt0 * KT3 + ld_s;
    ld_isz[j] = ld_on[j] && rr < b.nzeta;
  }
  // EXT: gaussian item q of this thread = (side, centre) for snapshot ld_s; it reads the nzeta raw values of its side itself
  // (the same cache lines the row loaders fetch) and writes exp(-|zeta - c|^2) into the table entry of its centre
  bool g_on[LG > 0 ? LG : 1];
  const double* g_ptr[LG > 0 ? LG : 1];
  int g_dst[LG > 0 ? LG : 1], g_cen[LG > 0 ? LG : 1];
  if (EXT) {
#pragma unroll
    for (int q = 0; q < LG; ++q) {
      const int gi = tid + q * 256;
      g_on[q] = gi < 2 * a.ng * KT3;
      const int gc = g_on[q] ? (gi / KT3) % a.ng : 0, gside = g_on[q] ? gi / (KT3 * a.ng) : 0;
      g_ptr[q] = (gside ? src_beta : src_alpha) + kt0 * KT3 + ld_s;
      g_dst[q] = CA + (1 + gside * a.ng + gc) * PST3 + ld_s;
      g_cen[q] = GC03 + gc * b.nzeta;
    }
  }
  auto load_raw = [&]() __attribute__((always_inline)) -> RawRegs {                // next tile of this workgroup's range
    RawRegs x;
    x.ok = ld_rem > 0;
#pragma unroll
    for (int j = 0; j < LR; ++j) {
      x.v[j] = 0.0;
      if (j < nld) {
        x.v[j] = *ld_ptr[j];        // no arithmetic on the loaded value here: its first use (store_raw, at the END of a tile) is
                                    // where the wave waits for the load - the tail mask is applied there
        ld_ptr[j] += KT3;
      }
    }
    ld_rem -= KT3;
    return x;
  };
  auto store_raw = [&](auto buf_c, const RawRegs& x) __attribute__((always_inline)) {   // powers x^1..x^D, and the constant / tail-mask entry
    constexpr int BUF = decltype(buf_c)::value;
#pragma unroll
    for (int j = 0; j < LR; ++j) {
      if (j < nld && ld_on[j]) {
        double* dst = sm + BUF * POWBUF3 + ld_dst0 + j * 32 * RB;
        const double xv = x.ok ? x.v[j] : 0.0;        // snapshots past Ns: every power is 0 (the tail mask)
        double p = xv;
        const int Dp = EXT ? a.Dp : D;
        for (int e = 0; e < Dp; ++e) {
          dst[e * PST3] = p;
          p *= xv;
        }
        if (EXT && a.df > 0 && ld_isz[j]) {
          // cos / sin(2 pi j x), j = 1..df, by the angle-addition recurrence; 0 past Ns (the tail mask: cos 0 = 1 would count)
          double s1, c1;
          sincospi(2.0 * xv, &s1, &c1);               // exact range reduction (the argument is 2 x, not 2 pi x)
          double cj = x.ok ? c1 : 0.0, sj = x.ok ? s1 : 0.0, cm = x.ok ? 1.0 : 0.0, sm1 = 0.0;
          for (int h = 0; h < a.df; ++h) {
            dst[(Dp + 2 * h) * PST3] = cj;
            dst[(Dp + 2 * h + 1) * PST3] = sj;
            const double cn = 2.0 * c1 * cj - cm, sn = 2.0 * c1 * sj - sm1;
            cm = cj; sm1 = sj; cj = cn; sj = sn;
          }
        }
      }
    }
    if (EXT) {
      // the raw values of the item's snapshot are fetched HERE, not with the row loads at the start of the tile: the row
      // loaders have pulled the same cache lines a tile ago, and 16 doubles held across the tile's MFMA loop would spill
#pragma unroll
      for (int q = 0; q < LG; ++q)
        if (g_on[q]) {
          double r2 = 0.0;
          for (int i = 0; i < b.nzeta; ++i) {
            const double dlt = g_ptr[q][(int64_t)i * a.Ns] - sm[g_cen[q] + i];
            r2 += dlt * dlt;
          }
          g_ptr[q] += KT3;
          sm[BUF * POWBUF3 + g_dst[q]] = x.ok ? exp(-r2) : 0.0;
        }
    }
    if (tid < KT3) sm[BUF * POWBUF3 + CA + tid] = x.ok ? 1.0 : 0.0;
  };

  // ---- INL: raw value -> register a tile ahead, table entries x, x^2, x^3, x^4 inside the next MFMA loop ----
  // EVERY thread fills a table row - no exec masking, no branch in the steady state: thread tid / KT3 = row; raw rows, then ONE
  // constant row (it "loads" 1.0 from a constant buffer with a pointer that does not advance; its first entry is the constant /
  // tail-mask address CA); the threads behind it repeat rows 0, 1, .. (the same values to the same addresses; within a wave the
  // addresses stay distinct).  Whether a raw tile lies wholly inside [0, Ns) is wave-uniform (scalar counter): only the range's
  // last tile can be partial, and only then does a thread look at its own snapshot index.
  const int tb_r = (tid / KT3) % (nrawrows + 1);
  const double* tb_ptr;
  int tb_inc = KT3;
  {
    const int rr = tb_r % nzm;
    tb_ptr = (rr < b.nzeta ? ((tb_r < nzm ? src_alpha : src_beta) + (int64_t)rr * a.Ns) : (src_u + (int64_t)(rr - b.nzeta) * a.Ns)) + kt0 * KT3 + ld_s;
    if (tb_r == nrawrows) { tb_ptr = kp_gram3_ones; tb_inc = 0; }
  }
  const uint32_t tb_dst = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) double*)(sm + tb_r * RB + ld_s);
  double tb_v = 0.0;                                               // the tile in flight
  int tb_tile = 0;                                                 // local index of the next tile to load (scalar)
  const int tb_full = (int)max((int64_t)0, min((int64_t)1 << 30, a.Ns / KT3 - kt0));   // local tiles wholly inside [0, Ns)
  auto load_tb = [&]() __attribute__((always_inline)) {
    tb_v = *tb_ptr;
    tb_ptr += tb_inc;
    ++tb_tile;
  };
  auto store_tb_v = [&](auto buf_c, double xv, int tile) __attribute__((always_inline)) {   // tile: local index of xv's tile (scalar)
    constexpr int BUF = decltype(buf_c)::value;
    if (__builtin_expect(tile >= tb_full, 0)) {                    // (scalar branch; at most once per workgroup)
      const int64_t s_glob = (kt0 + tile) * KT3 + ld_s;
      if (s_glob >= a.Ns) xv = 0.0;
    }
    const double x2 = xv * xv, x3 = x2 * xv;
    const uint32_t tb_dst_b = tb_dst;                              // (an asm operand alone does not capture in a generic lambda)
    // (8-byte stores at immediate offsets from one address register: four entries 80 bytes apart, no ds_write2 pairs them without
    // an add; 0.3640 against 0.3659 ms for the compiler's stores.  Not counted by the compiler: see lds_store_barrier)
    asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(tb_dst_b), "v"(xv), "n"((BUF * POWBUF3) * 8) : "memory");
    asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(tb_dst_b), "v"(x2), "n"((BUF * POWBUF3 + PST3) * 8) : "memory");
    asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(tb_dst_b), "v"(x3), "n"((BUF * POWBUF3 + 2 * PST3) * 8) : "memory");
    if constexpr (!P3) {   // (P3: no recipe holds a fourth power; the entry keeps the zeros of the one-time setup)
      const double x4 = x2 * x2;
      asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(tb_dst_b), "v"(x4), "n"((BUF * POWBUF3 + 3 * PST3) * 8) : "memory");
    }
  };
  auto store_tb = [&](auto buf_c) __attribute__((always_inline)) { store_tb_v(buf_c, tb_v, tb_tile - 1); };
  // the first three tiles' raw values are requested HERE, in front of the one-time LDS setup and its barriers: the setup runs in
  // the shadow of their latency (until round 6: setup, load tile 0, wait, table, barrier, lift, load tile 1, wait, ... - three
  // memory latencies in a row at the head of every workgroup, ~4 us of a 62 us launch at the arm data's 11 999 pairs)
  double tb_v0 = 0.0, tb_v1 = 0.0;
  if constexpr (INL) {
    load_tb(); tb_v0 = tb_v;
    load_tb(); tb_v1 = tb_v;
    load_tb();
  }

  // ---- one-time LDS setup: everything zero (padding columns and the zero group stay zero) ----
  for (int e = tid; e < LDS3_DOUBLES; e += 256) sm[e] = 0.0;
  if (TUP) {   // w_0 = 1 in every row of both Psi buffers (rows past Ns have psi = 0: the tail mask needs no weight)
    __syncthreads();
    if (tid < 2 * KT3) sm[PSI03 + (tid / KT3) * PSIBUF3 + (tid & (KT3 - 1)) * RS3 + WOFF3] = 1.0;
  }
  if (EXT) {   // gaussian centres (centre-major, nzeta coordinates each)
    for (int e = tid; e < a.ng * b.nzeta; e += 256) sm[GC03 + e] = a.centres[e];
  }
  if (PCS) {   // projection matrix, zero padded to (nfull4 x 32)
    const int nf4 = a.nfull4;
    for (int e = tid; e < 2 * nf4 * 16; e += 256) {
      const int ct = e / (nf4 * 16), r = e - ct * nf4 * 16, c = r >> 4, p = 16 * ct + (r & 15);
      sm[PCS03 + e] = (c < b.nfull && p < b.k_pcs) ? a.pcs[c + (size_t)p * b.nfull] : 0.0;
    }
  }

  // ---- PRE: the tile comes lifted from memory (kp_gram3_prelift_kernel): entries [psi_x | psi_y | weights] x KT3 snapshots, two 16-byte pieces per thread ----
  struct PreRegs { double2 v[2]; };
  const int pre_n2 = PRE ? KT3 * a.pre_rl / 2 : 0;   // 16-byte pieces per tile (<= 512)
  const double2* pre_ptr = PRE ? reinterpret_cast<const double2*>(a.pre + kt0 * KT3 * a.pre_rl) + tid : nullptr;
  int pre_left = nkt;
  bool pre_on[2] = {false, false};
  int pre_dst[2] = {0, 0};
  if (PRE) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int e = tid + j * 256;
      pre_on[j] = e < pre_n2;
      // tile layout [snapshot pair][row entry c][2]: a piece = snapshots (s, s + 1) of entry c; consecutive lanes = consecutive
      // entries of one pair, so the 16 lanes of a store group write 16 different columns of two Psi rows (the round-4 layout
      // [entry][8 snapshots] put the four pairs of one entry on neighbouring lanes: rows 240 doubles apart, the same bank - 32 %
      // of this kernel's LDS cycles were conflicts)
      const int e1 = pre_on[j] ? e : 0;
      const int sp = e1 / a.pre_rl, c = e1 - sp * a.pre_rl, srow = 2 * sp;
      // (the lifted rows carry w_1 .. w_{NWT-1} and zeros up to 12 entries: the zeros go to the unused weight slots and the scratch entry behind them)
      const int cw = c - 8 * a.G4;
      const int off = c < 4 * a.G4 ? c : c < 8 * a.G4 ? YOFF3 + (c - 4 * a.G4) : WOFF3 + (!TUP ? cw : cw < NWT - 1 ? wslot(cw + 1) : (cw - (NWT - 1)) < 2 * (6 - NWT / 2) ? ((cw - (NWT - 1)) / (6 - NWT / 2)) * 6 + NWT / 2 + (cw - (NWT - 1)) % (6 - NWT / 2) : 12);
      pre_dst[j] = PSI03 + srow * RS3 + off;
    }
  }
  auto load_pre = [&]() __attribute__((always_inline)) -> PreRegs {
    PreRegs x;
    x.v[0] = make_double2(0.0, 0.0);
    x.v[1] = make_double2(0.0, 0.0);
    if (pre_left > 0) {
      if (pre_on[0]) x.v[0] = pre_ptr[0];
      if (pre_on[1]) x.v[1] = pre_ptr[256];
      pre_ptr += pre_n2;
    }
    --pre_left;
    return x;
  };
  auto store_pre = [&](auto buf_c, const PreRegs& x) __attribute__((always_inline)) {
    constexpr int BUF = decltype(buf_c)::value;
    if (pre_on[0]) { sm[BUF * PSIBUF3 + pre_dst[0]] = x.v[0].x; sm[BUF * PSIBUF3 + pre_dst[0] + RS3] = x.v[0].y; }
    if (pre_on[1]) { sm[BUF * PSIBUF3 + pre_dst[1]] = x.v[1].x; sm[BUF * PSIBUF3 + pre_dst[1] + RS3] = x.v[1].y; }
  };

  // ---- lift of a snapshot tile: power-table buffer B -> Psi buffer B, in pipelined chunks ----
  constexpr int NCH = NLS;                           // lift steps per tile
  double2 lf[NF3];
  typedef double lds_d2 __attribute__((ext_vector_type(2)));   // (a 16-byte LDS read through an address-space pointer: no class type there)
  auto lift_nf = [](int j) { return LO && j > 0 ? 2 : NF3; };   // factors a job of lift step j multiplies
  auto lift_read = [&](int j, auto buf_c) __attribute__((always_inline)) {
    constexpr int BUF = decltype(buf_c)::value;
#pragma unroll
    for (int f = 0; f < NF3; ++f)      // (RB, PST3, CA and the pair offset are even: 16-byte aligned, one ds_read_b128)
      if (f < lift_nf(j)) {
        if constexpr (LO) {
          const lds_d2 v = *(const __attribute__((address_space(3))) lds_d2*)(uintptr_t)(fsb[j][f] + (uint32_t)(BUF * POWBUF3 * 8));
          lf[f].x = v.x;
          lf[f].y = v.y;
        } else lf[f] = *reinterpret_cast<const double2*>(__builtin_assume_aligned(&sm[BUF * POWBUF3 + fs[j][f]], 16));
      }
  };
  auto lift_write = [&](int j, auto buf_c) __attribute__((always_inline)) {
    constexpr int BUF = decltype(buf_c)::value;
    if constexpr (LO) {
      const double px = lift_nf(j) == 2 ? lf[0].x * lf[1].x : (lf[0].x * lf[1].x) * lf[2].x;
      const double py = lift_nf(j) == 2 ? lf[0].y * lf[1].y : (lf[0].y * lf[1].y) * lf[2].y;
      *(__attribute__((address_space(3))) double*)(uintptr_t)(wsb[j] + (uint32_t)(BUF * PSIBUF3 * 8)) = px;
      *(__attribute__((address_space(3))) double*)(uintptr_t)(wsb[j] + (uint32_t)((BUF * PSIBUF3 + RS3) * 8)) = py;
    } else if (lift_nf(j) == 2) {
      sm[BUF * PSIBUF3 + ws[j]] = lf[0].x * lf[1].x;
      sm[BUF * PSIBUF3 + ws[j] + RS3] = lf[0].y * lf[1].y;
    } else {
      sm[BUF * PSIBUF3 + ws[j]] = (lf[0].x * lf[1].x) * lf[2].x;
      sm[BUF * PSIBUF3 + ws[j] + RS3] = (lf[0].y * lf[1].y) * lf[2].y;
    }
  };
  // Workgroup barrier behind LDS stores.  The table stores of store_tb_v are inline-assembly ds_write_b64: the compiler's
  // waitcnt insertion does not count them, so a bare __syncthreads() would not wait for them.  Every barrier that publishes
  // a table or a lifted tile goes through here: s_waitcnt lgkmcnt(0) first (the compiler's own counted waits only become
  // more conservative), then the barrier.
  // gfx9 s_waitcnt immediate: vmcnt[3:0] | expcnt[6:4] | lgkmcnt[11:8] | vmcnt[5:4] in bits [15:14]
  constexpr int WAIT_LGKM0 = 0xc07f;
  static_assert(WAIT_LGKM0 == ((63 & 15) | (7 << 4) | (0 << 8) | ((63 >> 4) << 14)), "vmcnt = 63 and expcnt = 7 (no wait), lgkmcnt = 0");
  auto lds_store_barrier = [&]() __attribute__((always_inline)) {
    __builtin_amdgcn_s_waitcnt(WAIT_LGKM0);
    __syncthreads();
  };
  using B0 = std::integral_constant<int, 0>;
  using B1 = std::integral_constant<int, 1>;

  // ---- dim_red: econ lift of a lifted tile in place (Ksysid.m:1594-1618: [zeta ; pcs' psi_full ; 1]) ----
  // The lift above has left the FULL dictionary in the Psi buffer (columns [0, nfull) per side).  pcs' psi is a small
  // product on the matrix pipe: wave = (side, 4-snapshot group), two 4 x 16 output tiles (32 PCs), contraction over the
  // full columns.  Reads first, barrier, then the PCs overwrite columns nzeta.., the constant moves to column N - 1 and
  // the padding of the last 4-column group is cleared; the Gram MFMAs only touch columns < 4 G4 afterwards.
  // The projection's matrix operand is the same in every tile: this lane's entries of the FIRST 16 components (one per
  // k-step, KP_PCS_REGS of them at most) stay in registers for the whole kernel - the shape is bound by the LDS pipe
  // (DESIGN 6), and of the 3 operand reads per 2 MFMAs of this loop one goes away.  (Both component tiles would be 84
  // registers: measured, 75 spilled dwords in the <3,3,true> instantiation and 0.21 -> 0.25 ms; half of them: no gain.)
  constexpr int PREG = PCS ? KP_PCS_REGS : 1;
  double pcs_r[PREG];
  if (PCS) {
    __syncthreads();                                    // the staged matrix is visible
    const int bbase0 = PCS03 + (lane >> 4) * 16 + 4 * blk + lc;
#pragma unroll
    for (int kk = 0; kk < PREG; ++kk) pcs_r[kk] = kk < a.nfull4 / 4 ? sm[bbase0 + kk * 64] : 0.0;
  }
  auto project = [&](auto buf_c) __attribute__((always_inline)) {
    constexpr int BUF = decltype(buf_c)::value;
    const int side = wave >> 1, rg = wave & 1;
    const int abase = BUF * PSIBUF3 + PSI03 + (4 * rg + lc) * RS3 + side * YOFF3 + (lane >> 4);
    const int bbase = PCS03 + (lane >> 4) * 16 + 4 * blk + lc;
    const int nf4 = a.nfull4;
    double p0 = 0.0, p1 = 0.0;
    const int bb1 = bbase + nf4 * 16;
    const int nk = nf4 / 4;
#pragma unroll
    for (int kk = 0; kk < PREG; ++kk) {
      if (kk < nk) {                                    // (uniform)
        const double av = sm[abase + 4 * kk];
        const double b1 = sm[bb1 + kk * 64];
        p0 = __builtin_amdgcn_mfma_f64_4x4x4f64(av, pcs_r[kk], p0, 0, 0, 0);
        p1 = __builtin_amdgcn_mfma_f64_4x4x4f64(av, b1, p1, 0, 0, 0);
      }
    }
#pragma unroll 3
    for (int kk = PREG; kk < nk; ++kk) {                // dictionaries with more than 4 KP_PCS_REGS full columns
      const double av = sm[abase + 4 * kk];
      const double b0 = sm[bbase + kk * 64], b1 = sm[bb1 + kk * 64];
      p0 = __builtin_amdgcn_mfma_f64_4x4x4f64(av, b0, p0, 0, 0, 0);
      p1 = __builtin_amdgcn_mfma_f64_4x4x4f64(av, b1, p1, 0, 0, 0);
    }
    // the full dictionary's constant (0 past Ns: the tail mask) is read BEFORE the barrier: with nzeta + k_pcs >= nfull
    // the components written below land on its column
    const int crow = BUF * PSIBUF3 + PSI03 + (tid & (KT3 - 1)) * RS3 + ((tid / KT3) & 1) * YOFF3;
    const double one = sm[crow + b.nfull - 1];
    __syncthreads();
    {
      const int srow = BUF * PSIBUF3 + PSI03 + (4 * rg + (lane >> 4)) * RS3 + side * YOFF3;
      const int pc = 4 * blk + lc;
      if (pc < b.k_pcs) sm[srow + b.nzeta + pc] = p0;
      if (pc + 16 < b.k_pcs) sm[srow + b.nzeta + pc + 16] = p1;
    }
    if (tid < 2 * KT3) {
      sm[crow + b.N - 1] = one;
      for (int c = b.N; c < 4 * a.G4; ++c) sm[crow + c] = 0.0;
    }
    __syncthreads();
  };

  __syncthreads();
  if constexpr (PRE) {
    store_pre(B0{}, load_pre());
    __syncthreads();
  } else {
    if constexpr (INL) store_tb_v(B0{}, tb_v0, 0);
    else store_raw(B0{}, load_raw());
    lds_store_barrier();
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      lift_read(i, B0{});
      lift_write(i, B0{});
    }
    if constexpr (INL) store_tb_v(B1{}, tb_v1, 1);
    else store_raw(B1{}, load_raw());
    lds_store_barrier();
    if (PCS) project(B0{});
  }

  constexpr int NSTEP = (KT3 / 4) * NQ;                 // quad steps (NWT MFMAs each) per snapshot tile
  constexpr Gram3TileTiming TT = gram3_tile_timing(NQ, LO, EB);
  constexpr int SP = TT.sp;
  constexpr int LAG = TT.lag;
  constexpr int PF = TT.pf;                             // B operands requested this many quad steps ahead
  // EBT: this instantiation places the tile's barrier at the end of step BS (EB, and the lift's chunks fit in front of it).
  //
  // Why that is free of races (tile t on Psi buffer CUR, the other one NXT; pow[] the two power tables):
  //  * Reads of the current buffer.  Every LDS read of Psi[CUR] by tile t - B operands (PF steps ahead, so the last at step
  //    NSTEP - 1 - PF <= BS, or held back to behind the barrier where fewer steps stay behind it), A fragments (first step of
  //    the k-step before), weights (last step of the k-step before; the second A group's re-read never later than BS) - is
  //    issued at or before step BS and retired by the s_waitcnt lgkmcnt(0) in front of the barrier.  The next stores into
  //    Psi[CUR] are the lift stores of tile t + 1, from its step LAG on, behind that barrier: a fast wave cannot overtake a
  //    slow wave's reads.  Behind the barrier tile t reads Psi[NXT] only, which every wave's lift has completed in front of it.
  //  * The power table.  Tile t reads pow[NXT] at its lift reads, all in front of the barrier, and writes pow[CUR] at step
  //    KP_RAW_STEP.  Tile t + 1 writes pow[NXT] - the table tile t read - only behind the barrier, and reads pow[CUR], which tile
  //    t wrote in front of it.
  //  * The final tile.  Behind its barrier the redirected reads fetch LDS that is initialised but stale (a Psi buffer of an
  //    earlier tile, or the one-time zeros); nothing uses the values.  Keeping the reads is simpler than a branch.
  constexpr int BS = TT.bs;
  constexpr bool EBT = BS >= 0;
  static_assert(!EBT || (EB && BS < NSTEP - 1 && BS >= (KT3 / 4 - 1) * NQ && BS >= KP_RAW_STEP && (NCH - 1) * SP + LAG <= BS && LAG <= SP),
                "early barrier: behind the table store, the last lift store and the last k-step's first step, in front of the tile's last step");
  constexpr int NAW = TUP ? NWT / 2 : NWT;           // weighted A operands per A group (TUP: tuples of two weights)
  // operands in flight; EBT: they live across the tile boundary (the last steps of a tile request the next tile's first ones)
  double bvs[NSTEP];
  double bvs2[TUP ? NSTEP : 1];                      // TUP: the quad's second B operand (groups 2, 3)
  double wt[NAW];
  double avn0 = 0.0, avn1 = 0.0;                     // raw A fragments of the NEXT k-step (prefetched)
  // B operands of quad step i of the tile in the Psi buffer at pb
  auto load_b = [&](int pb, int i) __attribute__((always_inline)) {
    bvs[i] = sm[pb + (i / NQ) * 4 * RS3 + bo[i % NQ]];
    if constexpr (TUP) bvs2[i] = sm[pb + (i / NQ) * 4 * RS3 + bo2[i % NQ]];
  };
  // the NWT-1 weights of k-step kk, as 16-byte LDS reads (a pair each; immediate offsets, no address arithmetic);
  // TUP: this lane's weight of each of the 5 tuples, 8-byte reads at immediate offsets from its own base
  auto load_wt = [&](int pb, int kk) __attribute__((always_inline)) {
    if constexpr (TUP) {
#pragma unroll
      for (int w = 0; w + 1 < NAW; w += 2) {
        const double2 v = *reinterpret_cast<const double2*>(&sm[pb + kk * 4 * RS3 + wo + w]);
        wt[w] = v.x;
        wt[w + 1] = v.y;
      }
      wt[NAW - 1] = sm[pb + kk * 4 * RS3 + wo + NAW - 1];
    } else {
#pragma unroll
      for (int w = 0; w < NWT - 1; w += 2) {
        const double2 v = *reinterpret_cast<const double2*>(&sm[pb + kk * 4 * RS3 + wo + w]);
        wt[w + 1] = v.x;
        if (w + 2 < NWT) wt[w + 2] = v.y;
      }
    }
  };
  // a tile's first operands: the first PF steps' B operands, the A fragments and the weights of k-step 0
  auto head_reads = [&](int pb, bool two_groups) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < PF; ++i) load_b(pb, i);
    avn0 = sm[pb + ao0];
    if (two_groups) avn1 = sm[pb + ao1];
    load_wt(pb, 0);
  };

  // one snapshot tile: MFMAs on Psi buffer CUR, lift of the next tile into buffer 1-CUR, raw prefetch two ahead.
  // QS = number of leading quads that use A group a0 (wave-uniform, selected once outside the loop).
  auto tile = [&](auto cur_c, auto qs_c) __attribute__((always_inline)) {
    constexpr int CUR = decltype(cur_c)::value;
    constexpr int QS = decltype(qs_c)::value;
    using NXT = std::integral_constant<int, 1 - CUR>;
    constexpr int PB = CUR * PSIBUF3;
    constexpr int NPB = (1 - CUR) * PSIBUF3;
    // The raw loads of the tile after next are issued INSIDE the MFMA loop (behind step KP_RAW_STEP), not here: registers the
    // compiler has spilled are reloaded at the top of the tile, and a scratch reload behind a global load waits for that
    // load too (vmcnt counts in order) - with the load up here every wave sat out its HBM latency at the start of every tile.
    RawRegs rawreg;
    PreRegs prereg;
    // LO: the lift's address registers pass through an empty asm at the top of every tile body.  Without it the allocator,
    // two addresses lighter, spills one of them and reloads it inside every other tile body - behind the tile's raw load in the
    // vmcnt order (the register table of every arrangement tried); with it no tile loop holds a scratch access.
    // The BYTE addresses, not the offsets in doubles: behind the asm the value is opaque, and from a pinned offset the compiler
    // re-formed base + 8 offset for all ten in every tile body (ten v_lshl_add_u32: measured, 1.9 % slower than the old order).
    if constexpr (LO) {
#pragma unroll
      for (int j = 0; j < NLS; ++j) {
#pragma unroll
        for (int f = 0; f < NF3; ++f)
          if (f < lift_nf(j)) asm volatile("" : "+v"(fsb[j][f]));
        asm volatile("" : "+v"(wsb[j]));
      }
    }
    double aw[NAW];
    double av1 = 0.0;
    auto weigh = [&](double av) __attribute__((always_inline)) {
#pragma unroll
      for (int w = 0; w < NAW; ++w) {
        aw[w] = (!TUP && w == 0) ? av : av * wt[w];
      }
    };
    if constexpr (!EBT) head_reads(PB, QS < NQ);       // (EBT: requested by the tile before, or in front of the first one)
#pragma unroll
    for (int step = 0; step < NSTEP; ++step) {
      const int kk = step / NQ, q = step % NQ;
      if (step == (NSTEP > KP_RAW_STEP ? KP_RAW_STEP : 0)) {
        if constexpr (PRE) prereg = load_pre();        // the NEXT tile, lifted; stored behind the MFMA loop
        else if constexpr (INL) {                      // table of the tile after next from the value loaded a tile ago, then
          store_tb(cur_c);                             // the load for the tile behind it
          load_tb();
        } else rawreg = load_raw();
      }
      if (q == 0) {
        weigh(avn0);
        if (QS < NQ) av1 = avn1;
        if (kk + 1 < KT3 / 4) {
          avn0 = sm[PB + (kk + 1) * 4 * RS3 + ao0];
          if (QS < NQ) avn1 = sm[PB + (kk + 1) * 4 * RS3 + ao1];
        }
      }
      if (QS < NQ && q == QS) weigh(av1);
      // fetch the weights one step before they are multiplied in (LDS reads are free, registers are not); EBT: no later
      // than the barrier step
      const int wstep = kk * NQ + QS - 1;
      if (QS < NQ && QS > 1 && step == (EBT && wstep > BS ? BS : wstep)) load_wt(PB, kk);
      if (q == NQ - 1) {
        if (kk + 1 < KT3 / 4) load_wt(PB, kk + 1);
        else if constexpr (EBT) {                      // the next tile's weights and A fragments of k-step 0
          load_wt(NPB, 0);
          avn0 = sm[NPB + ao0];
          if (QS < NQ) avn1 = sm[NPB + ao1];
        }
      }
      if (step + PF < NSTEP) load_b(PB, step + PF);
      else if constexpr (EBT) {
        if (step > BS) load_b(NPB, step + PF - NSTEP);  // the next tile's first B operands, into slots this tile has used up
      }
      const double bv = bvs[step];
      const double bv2 = TUP ? bvs2[step] : 0.0;
      if constexpr (TUP) {
        // accumulator 2 p + h: blocks b = (weight 2 p + (b >> 1), group 2 h + (b & 1) of the quad)
#pragma unroll
        for (int w = 0; w < NAW; ++w) {
          acc[q][2 * w] = __builtin_amdgcn_mfma_f64_4x4x4f64(aw[w], bv, acc[q][2 * w], 0, 0, 0);
          acc[q][2 * w + 1] = __builtin_amdgcn_mfma_f64_4x4x4f64(aw[w], bv2, acc[q][2 * w + 1], 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int w = 0; w < NWT; ++w) acc[q][w] = __builtin_amdgcn_mfma_f64_4x4x4f64(aw[w], bv, acc[q][w], 0, 0, 0);
      }
      // one register set for the chunk in flight: the write of chunk i precedes the read of chunk i+1
      if constexpr (!PRE) {
        if (step >= LAG && (step - LAG) % SP == 0 && (step - LAG) / SP < NCH) lift_write((step - LAG) / SP, NXT{});
        if (step % SP == 0 && step / SP < NCH) lift_read(step / SP, NXT{});
      }
      if constexpr (EBT) {
        if (step == BS) {
          // the tile's barrier: behind this step's MFMAs and the last lift store (the table stores are inline assembly the
          // compiler does not count: the explicit wait stays), then the B operands that were due in front of it
          lds_store_barrier();
#pragma unroll
          for (int s = NSTEP - PF; s <= BS; ++s) load_b(NPB, s + PF - NSTEP);
        }
      }
      __builtin_amdgcn_sched_barrier(0);   // keep the hand-made software pipeline: no hoisting of later steps' LDS reads
    }
    if constexpr (!PRE) {
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        if (i * SP >= NSTEP) lift_read(i, NXT{});
        if (i * SP + LAG >= NSTEP) lift_write(i, NXT{});
      }
    }
    if constexpr (PRE) {
      store_pre(NXT{}, prereg);
      __syncthreads();
    } else if constexpr (!EBT) {
      if constexpr (!INL) store_raw(cur_c, rawreg);
      lds_store_barrier();
    }
    if (PCS) project(NXT{});
  };
  // nkt tiles, two per round (the buffer index is an immediate) and a remainder.  EBT: only the first tile's operands are
  // requested here - the setup's last barrier has published Psi buffer 0 -, every tile requests those of the one behind it
  auto run_tiles = [&](auto qs_c) __attribute__((always_inline)) {
    if constexpr (EBT) head_reads(0, decltype(qs_c)::value < NQ);
    int t = 0;
    for (; t + 1 < nkt; t += 2) {
      tile(B0{}, qs_c);
      tile(B1{}, qs_c);
    }
    if (t < nkt) tile(B0{}, qs_c);
  };
  switch (qs) {
    case 1: run_tiles(std::integral_constant<int, 1>{}); break;
    case 2: run_tiles(std::integral_constant<int, (NQ >= 2 ? 2 : NQ)>{}); break;
    case 3: run_tiles(std::integral_constant<int, (NQ >= 3 ? 3 : NQ)>{}); break;
    case 4: run_tiles(std::integral_constant<int, (NQ >= 4 ? 4 : NQ)>{}); break;
    case 5: run_tiles(std::integral_constant<int, (NQ >= 5 ? 5 : NQ)>{}); break;
    default: run_tiles(std::integral_constant<int, NQ>{}); break;
  }

  // epilogue: [split][job][q][w][lane]
  double* dst = a.part + (((size_t)split * a.njobs + job) * NQ) * NWT * 64 + lane;
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int w = 0; w < NWT; ++w) dst[(q * NWT + w) * 64] = acc[q][w];
}

// Sums the partials of one (job, quad, weight) block vector in split order and scatters the
// 4 blocks (4x4 each) into G and C.  lane l: block = (l>>2)&3, row r = l>>4, col c = l&3.
// BM >= 2 (the kernel's paired-weight form, TUP): accumulator w' = 2 p + h of a quad holds, in block b, weight 2 p + (b >> 1)
// against group 2 h + (b & 1) of the quad.
// blockDim.x / 64 = 4, 8 or 16 waves share the split sum (the launcher picks by the split count: a dim_red fit at the arm data's
// size has 167 splits of 184 KB - four waves walked 42 dependent-latency loads each, 14 us for a 23 us Gram kernel), each wave
// with four loads in flight; every order is fixed: bitwise reproducible.
// blockIdx.y = fit of a group launch (kp_gram3_kernel, GRP): it sums that fit's nsplit splits - the global splits
// [y nsplit, (y + 1) nsplit) - into that fit's [G | C] slot, 2 W^2 doubles behind the previous one.
// dst_off != nullptr (cover plan, kp_gram3_cover.h): an element of an S block is written to every entry (i <= j) of psi_x psi_x'
// whose monomial it is the designated source of - dst[dst_off[e] .. dst_off[e + 1]) of element e = ((job NQ + q) 4 + B slot) 16 +
// 4 row + column - with the same four stores per entry; an element that is nobody's source writes nothing.  T blocks as ever.
__global__ __launch_bounds__(1024) void kp_gram3_reduce_kernel(const double* __restrict__ part, int nsplit, int njobs, int NQ, int NWT,
                                                              int BM, const uint32_t* __restrict__ desc, int G4, int N, int W,
                                                              double* __restrict__ G, double* __restrict__ C,
                                                              const uint32_t* __restrict__ dst_off, const uint32_t* __restrict__ dst) {
  const int idx = blockIdx.x;                 // (job*NQ + q)*NWT + w
  int w = idx % NWT;
  const int jq = idx / NWT, q = jq % NQ, job = jq / NQ;
  const int l = threadIdx.x & 63, wv = threadIdx.x >> 6, nwv = blockDim.x >> 6;
  __shared__ double red[16][64];
  const size_t per_split = (size_t)njobs * NQ * NWT * 64;
  const double* src = part + (size_t)blockIdx.y * nsplit * per_split + (size_t)idx * 64 + l;
  G += (size_t)blockIdx.y * 2 * W * W;
  C += (size_t)blockIdx.y * 2 * W * W;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int p = wv;
  for (; p + 3 * nwv < nsplit; p += 4 * nwv) {
    const double v0 = src[(size_t)p * per_split], v1 = src[(size_t)(p + nwv) * per_split];
    const double v2 = src[(size_t)(p + 2 * nwv) * per_split], v3 = src[(size_t)(p + 3 * nwv) * per_split];
    s0 += v0; s1 += v1; s2 += v2; s3 += v3;
  }
  for (; p < nsplit; p += nwv) s0 += src[(size_t)p * per_split];
  red[wv][l] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (wv) return;
  double s = red[0][l];
  for (int v = 1; v < nwv; ++v) s += red[v][l];
  const uint32_t* jd = desc + (size_t)job * (1 + NQ);
  const int ga = q < (int)((jd[0] >> 16) & 255u) ? (int)(jd[0] & 255u) : (int)((jd[0] >> 8) & 255u);
  int gsel = (l >> 2) & 3;
  if (BM >= 2) {
    const int b = gsel;
    gsel = 2 * (w & 1) + (b & 1);
    w = (w & ~1) + (b >> 1);
  }
  const int gb = (int)((jd[1 + q] >> (8 * gsel)) & 255u);
  if (gb >= 2 * G4) return;                   // zero group: padding of the last quad / idle job
  // weight index -> (x, y), x <= y
  int wa = 0, wb = 0, cnt = 0;
  for (int x = 0; x <= BM; ++x)
    for (int y = x; y <= BM; ++y) {
      if (cnt == w) { wa = x; wb = y; }
      ++cnt;
    }
  const int ia = 4 * ga + (l >> 4);
  if (ia >= N) return;
  if (gb < G4 && dst_off) {                   // S block of a cover plan: by monomial
    const int e = (jq * 4 + gsel) * 16 + (l >> 4) * 4 + (l & 3);
    for (uint32_t k = dst_off[e]; k < dst_off[e + 1]; ++k) {
      const uint32_t d = dst[k];
      const size_t di = d & 0xffffu, dj = d >> 16;
      const size_t r1 = (size_t)wa * N + di, c1 = (size_t)wb * N + dj;
      const size_t r2 = (size_t)wb * N + di, c2 = (size_t)wa * N + dj;
      G[c1 * W + r1] = s; G[r1 * W + c1] = s;
      G[c2 * W + r2] = s; G[r2 * W + c2] = s;
    }
  } else if (gb < G4) {                       // S block: psi_x' psi_x  ->  G (symmetric)
    const int jb = 4 * gb + (l & 3);
    if (jb >= N) return;
    if (ga == gb && ia > jb) return;          // diagonal block: keep the upper half, mirror below (exact symmetry)
    const size_t r1 = (size_t)wa * N + ia, c1 = (size_t)wb * N + jb;
    const size_t r2 = (size_t)wb * N + ia, c2 = (size_t)wa * N + jb;
    G[c1 * W + r1] = s; G[r1 * W + c1] = s;
    G[c2 * W + r2] = s; G[r2 * W + c2] = s;
  } else {                                    // T block: psi_x' psi_y  ->  C
    const int jb = 4 * (gb - G4) + (l & 3);
    if (jb >= N) return;
    C[((size_t)wb * N + jb) * W + (size_t)wa * N + ia] = s;
    C[((size_t)wa * N + jb) * W + (size_t)wb * N + ia] = s;
  }
}

struct kp_gram3_plan {
  int G4 = 0, nq = 0, njobs = 0, nsuper = 0;
  int two_group_jobs = 0;    // jobs that span two A groups: their waves weigh two A fragments per k-step (kp_timer_get(15))
  uint32_t* desc = nullptr;  // device
  // cover plan (kp_gram3_cover.h): the reduction's destination lists, device; nullptr in a circulant plan
  uint32_t* dst_off = nullptr;
  uint32_t* dst = nullptr;
  // the circulant plan of a dictionary owns its cover plan, built on first use (gram3_cover_plan); nullptr: none is kept
  kp_gram3_plan* cover = nullptr;
  bool cover_tried = false;
  // ... and the dictionary's lift slot table (kp_gram3_lift.h), device, built on first use; nullptr behind lift_tried: the
  // dictionary keeps the order e = tid + 256 j
  uint32_t* lift = nullptr;
  bool lift_tried = false;
};

void kp_gram3_plan_free(kp_gram3_plan* p) {
  if (!p) return;
  kp_gram3_plan_free(p->cover);
  if (p->desc) (void)hipFree(p->desc);
  if (p->dst_off) (void)hipFree(p->dst_off);
  if (p->dst) (void)hipFree(p->dst);
  if (p->lift) (void)hipFree(p->lift);
  delete p;
}

static hipError_t plan3_upload(uint32_t** dev, const std::vector<uint32_t>& host) {
  hipError_t e = hipMalloc((void**)dev, std::max<size_t>(host.size(), 1) * 4);
  if (e == hipSuccess && !host.empty()) e = hipMemcpy(*dev, host.data(), host.size() * 4, hipMemcpyHostToDevice);
  return e;
}

// Row g of psi_x (one 4-column group) is paired with: its circulant half of the psi_x groups
// (g, g+1, ..., g+floor(G4/2) mod G4; antipodal pairs once) and all G4 groups of psi_y.
// All quads (A group, 4 B groups) of all rows form one list; a job (one wave) is nq CONSECUTIVE quads,
// so it spans at most two A groups when nq <= quads per row, and whole workgroups (4 jobs) fill evenly (gram3_pack_rows).
static int make_plan3(kp_ctx* ctx, int N, int nwt, int nq_cap, kp_gram3_plan** out) {
  kp_gram3_plan* p = new kp_gram3_plan();
  const int G4 = (N + 3) / 4;
  p->G4 = G4;
  size_t maxq = 0;
  const std::vector<std::vector<int>> rows = gram3_circulant_rows(G4, &maxq);
  Gram3JobsHost jobs;
  gram3_pack_rows(rows, G4, nwt, nq_cap, maxq, &jobs);     // (quads, quads per job, job list: kp_gram3_cover.h)
  p->nq = jobs.nq;
  p->njobs = jobs.njobs;
  p->nsuper = jobs.njobs / GRAM3_WAVES;
  p->two_group_jobs = gram3_two_group_jobs(jobs);
  hipError_t e = plan3_upload(&p->desc, jobs.desc);
  if (e != hipSuccess) {
    kp_gram3_plan_free(p);
    return ctx->fail(KP_ERR_HIP, std::string("kp_fit_gram: plan upload: ") + hipGetErrorString(e));
  }
  *out = p;
  return KP_OK;
}

template <int NQ, int BM, bool PCS, bool EXT = false, bool PRE = false, bool P3 = false, bool LO = false, bool EB = false>
static hipError_t launch3(const Gram3Args& a, int grid, size_t lds, hipStream_t st) {
  static KpLdsCache lds_cache;
  {
    const size_t lds_max = (size_t)(LDS3_DOUBLES + (PCS ? LDS3_PCS_DOUBLES : 0) + (EXT ? LDS3_GAUSS_DOUBLES : 0)) * sizeof(double);
    hipError_t e = kp_ensure_lds(lds_cache, (const void*)kp_gram3_kernel<NQ, BM, PCS, EXT, PRE, P3, LO, EB>, lds_max);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((kp_gram3_kernel<NQ, BM, PCS, EXT, PRE, P3, LO, EB>), dim3(grid), dim3(256), lds, st, a);
  return hipGetLastError();
}

// From the form of a launch (gram3_form, kp_gram3_launch.h) to its instantiation - the one place that names them.  The guards
// bound the set: PCS to NQ <= 4 (more quads per wave spill once the projection is inlined; plans of dim_red dictionaries stay
// below), P3 / LO to the monomial form, EB to the tiles that have the room - which only a tile of the ordered lift has.
template <int NQ, int BM>
static hipError_t gram3_dispatch_at(const Gram3Form& f, const Gram3Args& a, int grid, size_t lds, hipStream_t st) {
  static_assert(gram3_tile_timing(NQ, false, true).bs < 0, "early tile barrier: with the ordered lift only");
  switch (f.kind) {
    case GRAM3_PRE: return launch3<NQ, BM, false, false, true>(a, grid, lds, st);
    case GRAM3_PCS:
      if constexpr (NQ <= 4) return launch3<NQ, BM, true>(a, grid, lds, st);
      else return hipErrorInvalidValue;
    case GRAM3_EXT: return launch3<NQ, BM, false, true>(a, grid, lds, st);
    case GRAM3_MONO: break;
  }
  if constexpr (gram3_tile_timing(NQ, true, true).bs >= 0) {
    if (f.eb) return f.p3 ? launch3<NQ, BM, false, false, false, true, true, true>(a, grid, lds, st) : launch3<NQ, BM, false, false, false, false, true, true>(a, grid, lds, st);
  }
  if (f.lo) return f.p3 ? launch3<NQ, BM, false, false, false, true, true>(a, grid, lds, st) : launch3<NQ, BM, false, false, false, false, true>(a, grid, lds, st);
  return f.p3 ? launch3<NQ, BM, false, false, false, true>(a, grid, lds, st) : launch3<NQ, BM, false>(a, grid, lds, st);
}

template <int NQ>
static hipError_t gram3_dispatch_nq(const Gram3Form& f, const Gram3Args& a, int grid, size_t lds, hipStream_t st) {
  return f.bm == 1 ? gram3_dispatch_at<NQ, 1>(f, a, grid, lds, st) : f.bm == 2 ? gram3_dispatch_at<NQ, 2>(f, a, grid, lds, st) : gram3_dispatch_at<NQ, 3>(f, a, grid, lds, st);
}

static hipError_t gram3_dispatch(const Gram3Form& f, const Gram3Args& a, int grid, size_t lds, hipStream_t st) {
  switch (f.nq) {
    case 1: return gram3_dispatch_nq<1>(f, a, grid, lds, st);
    case 2: return gram3_dispatch_nq<2>(f, a, grid, lds, st);
    case 3: return gram3_dispatch_nq<3>(f, a, grid, lds, st);
    case 4: return gram3_dispatch_nq<4>(f, a, grid, lds, st);
    case 5: return gram3_dispatch_nq<5>(f, a, grid, lds, st);
    default: return gram3_dispatch_nq<6>(f, a, grid, lds, st);
  }
}

// The switches of the launch decisions (Gram3Switches).  Read once, when the first question is asked: KP_GRAM3_NO_PRELIFT;
// KP_GRAM3_PRELIFT_MIN_NS; KP_GRAM3_POW3=0 - the in-loop table build keeps its x^4 entry for every dictionary;
// KP_GRAM3_LIFT_ORDER=0 - the lift keeps the order e = tid + 256 j for every dictionary; KP_GRAM3_EARLY_BARRIER=0 - every tile
// keeps its barrier behind the last quad step (the three: A/B runs, tests).  Read at every question: KP_NO_GRAM3_EXT.
static Gram3Switches gram3_switches() {
  static const Gram3Switches once = gram3_switches_read(getenv);
  Gram3Switches s = once;
  s.ext = !getenv("KP_NO_GRAM3_EXT");
  return s;
}

// the facts of a dictionary that the launch decisions read ...
static Gram3Facts gram3_dict_facts(const kp_basis* basis) {
  const BasisDev& b = basis->dev;
  Gram3Facts f;
  f.N = b.N; f.m = b.m; f.nfull = b.nfull; f.nzeta = b.nzeta; f.k_pcs = b.k_pcs; f.pow_depth = basis->pow_depth;
  f.fast = basis->fast; f.fast_ext = basis->fast_ext;
  f.ext_Dp = basis->ext_Dp; f.ext_df = basis->ext_df; f.ext_ng = basis->ext_ng;
  return f;
}

static bool gram3_ext(const kp_basis* basis) { return gram3_ext(gram3_dict_facts(basis), gram3_switches()); }
static bool gram3_mono(const kp_basis* basis) { return gram3_mono(gram3_dict_facts(basis), gram3_switches()); }


bool kp_gram3_applicable(const kp_basis* basis) {
  const BasisDev& b = basis->dev;
  if (getenv("KP_NO_GRAM3")) return false;
  // the lift deals 4 (2 nfull + weights) (item, snapshot pair) jobs over 3 x 256 slots (NLS = 3 in kp_gram3_kernel)
  if (2 * b.nfull + (b.m + 1) * (b.m + 2) / 2 - 1 > 192) return false;
  if (gram3_ext(basis))
    return b.model_type == KP_MODEL_BILINEAR && basis->ext_max_factors <= NF3 && b.nfull <= YOFF3 && b.m >= 1 && b.m <= 3 &&
           2 * (b.nzeta + b.m) * KT3 <= 256 &&
           2 * (b.nzeta + b.m) * (basis->ext_Dp + 2 * basis->ext_df) + 1 + 2 * basis->ext_ng <= NIDMAX3;
  // dim_red dictionaries: econ layout [zeta | k_pcs principal components | 1], at most 32 components
  if (b.k_pcs > 0 && (b.k_pcs > PCSMAX3 || b.N != b.nzeta + b.k_pcs + 1 || getenv("KP_NO_GRAM3_PCS"))) return false;
  // (powers <= 4: the in-loop table build writes x .. x^4 at an entry stride of 4; the constant row's 4 entries follow the raw rows)
  return b.model_type == KP_MODEL_BILINEAR && basis->fast && basis->max_factors <= NF3 && b.nfull <= YOFF3 && basis->pow_depth <= 4 &&
         b.m >= 1 && b.m <= 3 && (2 * (b.nzeta + b.m) + 1) * KT3 <= 256 && 2 * (b.nzeta + b.m) * 4 + 4 <= NIDMAX3;   // (+ 1: the constant's table row has a thread)
}

// the dictionary's plan, built on first use
static int gram3_plan(kp_ctx* ctx, kp_basis* basis) {
  if (basis->plan3) return KP_OK;
  const BasisDev& b = basis->dev;
  const int N = b.N, BM = b.m, NWT = (BM + 1) * (BM + 2) / 2;
  // fourier / gaussian tables: the transcendental code's constants and temporaries cost ~40 registers, so fewer quads
  // (accumulators) per wave or the kernel spills (measured: 4 quads per wave is the fastest cap, tools/gram_shapes_probe.py)
  static const int ext_cap = [] { const char* e = getenv("KP_GRAM3_EXT_NQ"); return e ? atoi(e) : 4; }();
  return make_plan3(ctx, N, NWT, b.k_pcs > 0 ? 4 : gram3_ext(basis) ? ext_cap : 6, &basis->plan3);     // (one plan serves both forms of a dim_red / fourier / gaussian fit)
}

// KP_GRAM3_COVER (read once): 0 - no launch takes a cover plan; unset or 1 - the launches of kp_fit's deferred-solve branch do
// (the Gram queue of the pipelined fits and its immediate dispatch: kp_gram3_launch_group, kp_gram3_launch's `cover`); 2 - every launch of a qualifying dictionary,
// kp_fit_gram included (tests and A/B runs only)
static int gram3_cover_mode() {
  static const int v = [] { const char* e = getenv("KP_GRAM3_COVER"); return e ? std::min(2, std::max(0, atoi(e))) : 1; }();
  return v;
}

// KP_GRAM3_ONEA=0 (read once): the cover plan of gram3_cover_build even where the dictionary has a one-A-group plan (A/B runs, tests)
static bool gram3_onea_on() {
  static const bool on = [] { const char* e = getenv("KP_GRAM3_ONEA"); return !e || atoi(e) != 0; }();
  return on;
}

// The dictionary's cover plan (kp_gram3_cover.h), built on first use: for the in-kernel-lift monomial form (gram3_mono)
// only - every column a pure monomial, no projection, no fourier / gaussian table entries - and KEPT only when it has
// fewer jobs (whole workgroups) than the circulant plan and passes its own coverage check on the host.  *out = nullptr: this
// dictionary runs the circulant plan everywhere.
// A kept cover plan is replaced by the dictionary's one-A-group plan (gram3_onea_build: same quads per job, no job spans two A
// groups, so no wave weighs a second A fragment) where the search finds one with no more jobs; where it finds none, or with
// KP_GRAM3_ONEA=0, the cover plan stays byte for byte what gram3_cover_build made.  The search costs ~35 ms of host time for
// the headline dictionary, once per dictionary, here on its first pipelined fit.
static int gram3_cover_plan(kp_ctx* ctx, kp_basis* basis, kp_gram3_plan** out) {
  kp_gram3_plan& circ = *basis->plan3;
  *out = nullptr;
  if (!circ.cover_tried) {
    circ.cover_tried = true;
    const BasisDev& b = basis->dev;
    const int N = b.N, NWT = (b.m + 1) * (b.m + 2) / 2;
    if (!gram3_mono(basis) || !basis->fast || b.nfull != N || (int)basis->h_recipes.size() != N) return KP_OK;
    Gram3CoverHost cov;
    if (!gram3_cover_build(basis->h_recipes.data(), N, basis->pow_depth, NWT, 6, &cov) || cov.jobs.njobs >= circ.njobs) return KP_OK;
    if (gram3_onea_on()) {
      Gram3CoverHost one;
      if (gram3_onea_build(basis->h_recipes.data(), N, basis->pow_depth, cov, &one) && one.jobs.nq == cov.jobs.nq && one.jobs.njobs <= cov.jobs.njobs) cov = std::move(one);
    }
    kp_gram3_plan* p = new kp_gram3_plan();
    p->G4 = circ.G4;
    p->two_group_jobs = gram3_two_group_jobs(cov.jobs);
    p->nq = cov.jobs.nq;
    p->njobs = cov.jobs.njobs;
    p->nsuper = cov.jobs.njobs / GRAM3_WAVES;
    p->cover_tried = true;
    hipError_t e = plan3_upload(&p->desc, cov.jobs.desc);
    if (e == hipSuccess) e = plan3_upload(&p->dst_off, cov.dst_off);
    if (e == hipSuccess) e = plan3_upload(&p->dst, cov.dst);
    if (e != hipSuccess) {
      kp_gram3_plan_free(p);
      circ.cover_tried = false;
      return ctx->fail(KP_ERR_HIP, std::string("kp_fit_gram: plan upload: ") + hipGetErrorString(e));
    }
    circ.cover = p;
  }
  *out = circ.cover;
  return KP_OK;
}

// The dictionary's lift slot table (kp_gram3_lift.h), built and uploaded on first use and kept with its circulant plan;
// *out = nullptr: the dictionary keeps today's order (more jobs of three real factors than lift step 0 has slots).
static int gram3_lift_table(kp_ctx* ctx, kp_basis* basis, const uint32_t** out) {
  kp_gram3_plan& circ = *basis->plan3;
  *out = nullptr;
  if (!circ.lift_tried) {
    const BasisDev& b = basis->dev;
    Gram3LiftOrderHost lo;
    if (basis->fast && (int)basis->h_recipes.size() == b.nfull && gram3_lift_order_build(basis->h_recipes.data(), b.nfull, b.m, &lo)) {
      hipError_t e = plan3_upload(&circ.lift, lo.slot);
      if (e != hipSuccess) {
        if (circ.lift) (void)hipFree(circ.lift);
        circ.lift = nullptr;
        return ctx->fail(KP_ERR_HIP, std::string("kp_fit_gram: lift table upload: ") + hipGetErrorString(e));
      }
    }
    circ.lift_tried = true;
  }
  *out = circ.lift;
  return KP_OK;
}

// the plan a launch runs: the dictionary's circulant plan, or its cover plan where the caller's path takes one and one is kept
static int gram3_plan_for(kp_ctx* ctx, kp_basis* basis, bool deferred, kp_gram3_plan** out) {
  int rc = gram3_plan(ctx, basis);
  if (rc) return rc;
  *out = basis->plan3;
  if (gram3_cover_mode() == 2 || (gram3_cover_mode() == 1 && deferred)) {
    kp_gram3_plan* cov = nullptr;
    rc = gram3_cover_plan(ctx, basis, &cov);
    if (rc) return rc;
    if (cov) *out = cov;
  }
  return KP_OK;
}

// ... and of a launch of n fits of Ns snapshots each on `plan` (Gram3Facts, kp_gram3_launch.h).  KP_GRAM3_WGPCU is read at every
// question.  The dictionary's lift slot table is the launcher's to ask (gram3_lift_table: it builds one).
static Gram3Facts gram3_facts(const kp_ctx* ctx, const kp_basis* basis, const kp_gram3_plan& plan, int64_t Ns, int n) {
  Gram3Facts f = gram3_dict_facts(basis);
  f.nq = plan.nq; f.nsuper = plan.nsuper; f.njobs = plan.njobs; f.two_group_jobs = plan.two_group_jobs;
  for (const kp_gram3_plan* o : {(const kp_gram3_plan*)basis->plan3, (const kp_gram3_plan*)basis->plan3->cover})
    if (o && o != &plan) { f.other_nq = o->nq; f.other_nsuper = o->nsuper; f.other_njobs = o->njobs; }
  f.Ns = Ns;
  f.n = n;
  f.num_cu = ctx->num_cu;
  if (const char* ov = getenv("KP_GRAM3_WGPCU")) f.wg_per_cu = std::max(1, atoi(ov));
  f.hbm_bytes = ctx->hbm_bytes;
  return f;
}

// Fits that may share a Gram launch (kp_fit.hip's queue of pipelined fits): the in-kernel-lift monomial form of kp_gram3_kernel -
// no projection, no fourier / gaussian table entries, hence no prelift buffer either (gram3_mono); and only while
// a lone launch's splits are shorter than KP_GRAM_GROUP_MAX_KPS tiles.  What sharing saves is a fixed cost per fit (head, write-out
// and reduction of one accumulator set per wave slot: ~30 us at W = 336, some 15 tile times); what it costs is whole-split
// granularity, 1 - 1.4 % of the kernel time (a fit of a group of 8 gets 9 of the 73 splits: 504 of 512 slots) - measured at
// 1e6 / 1e7 pairs (1 713 / 17 124 tiles per split) the group was 1.3 / 1.5 % SLOWER per fit, at 1e5 (172) 4.6 % faster.  Where
// between 172 and 1 713 the two cross was NOT measured: 512 is the estimate from those figures (fixed saving ~22 us = 1.36 % of a
// kernel of 1.6 ms, ~800 tiles per split at W = 336), rounded down.
bool kp_gram3_groupable(kp_ctx* ctx, const kp_basis* basis_c, const kp_snapshots* s) {
  kp_basis* basis = const_cast<kp_basis*>(basis_c);
  const BasisDev& b = basis->dev;
  if (!(kp_gram3_applicable(basis) && gram3_mono(basis) && s->nzeta == b.nzeta && s->m == b.m)) return false;
  kp_gram3_plan* plan = nullptr;                 // (the plan the queue's launch will run: kp_gram3_launch_group)
  if (gram3_plan_for(ctx, basis, true, &plan) != KP_OK) return false;      // (a plan that cannot be built: the immediate dispatch reports it)
  static const int64_t max_kps = [] { const char* e = getenv("KP_GRAM_GROUP_MAX_KPS"); return e ? (int64_t)atoll(e) : (int64_t)512; }();
  return gram3_lone_splits_shorter(gram3_facts(ctx, basis, *plan, s->Ns, 1), max_kps);
}

// The events around a launch of n fits.  Every event record is a barrier packet the command processor works through between two
// Gram kernels.  A synchronous launch records ev0 and evp[0] in front of the kernel, evp[1] behind it, ev1 and evp[2] behind the
// reduction.  The pipelined path (ring_timing) keeps two (kernel start / end) of its ring of event pairs, averaged at
// kp_synchronize, and those for every 4th launch only (the mean over the ring is what kp_synchronize reports).  A group launch
// (ring_group: the Gram queue of kp_fit.hip, group size > 1) of several fits is always timed - one event pair per group is the
// packet rate of every 4th single launch - and so is its reduction (ring_red, timer 6).  A group of ONE keeps the every-4th rule
// and records no third event: what a single launch recorded before.
namespace {
struct Gram3Events {
  kp_ctx* ctx;
  bool timed = false;
  hipEvent_t ev_start = nullptr, ev_end = nullptr, ev_red = nullptr;

  hipError_t begin(int n) {
    if (!ctx->ring_timing) {
      hipError_t e = hipEventRecord(ctx->ev0, ctx->stream);
      if (e != hipSuccess) return e;
    }
    ev_start = ctx->evp[0];
    ev_end = ctx->evp[1];
    timed = !ctx->ring_timing || (ctx->ring_group && n > 1) || (ctx->ring_skip++ & 3) == 0;
    if (ctx->ring_timing && timed) {
      ev_start = ctx->ring[2 * ctx->ring_pos];
      ev_end = ctx->ring[2 * ctx->ring_pos + 1];
      ctx->ring_members[ctx->ring_pos] = n;
      ctx->ring_has_red[ctx->ring_pos] = false;
      if (ctx->ring_group && n > 1) {
        ev_red = ctx->ring_red[ctx->ring_pos];
        ctx->ring_has_red[ctx->ring_pos] = ev_red != nullptr;
      }
      ctx->ring_pos = (ctx->ring_pos + 1) % 64;
      if (ctx->ring_n < 64) ++ctx->ring_n;
    }
    return timed ? hipEventRecord(ev_start, ctx->stream) : hipSuccess;
  }
  hipError_t after_kernel() { return timed ? hipEventRecord(ev_end, ctx->stream) : hipSuccess; }
  hipError_t after_reduction() {
    hipError_t e = ev_red ? hipEventRecord(ev_red, ctx->stream) : hipSuccess;
    if (e == hipSuccess && !ctx->ring_timing) e = hipEventRecord(ctx->ev1, ctx->stream);
    if (e == hipSuccess && !ctx->ring_timing) e = hipEventRecord(ctx->evp[2], ctx->stream);
    return e;
  }
};
}  // namespace

// the kernel's arguments for a launch in `form` with geometry `g`; lift: the dictionary's slot table where form.lo
static Gram3Args gram3_args(const kp_basis* basis, const kp_gram3_plan& plan, const Gram3Form& form, const Gram3Geometry& g, const kp_snapshots* const* ss, int n,
                            double* part, const double* pre_buf, const uint32_t* lift) {
  const BasisDev& b = basis->dev;
  const kp_snapshots* s = ss[0];
  const bool ext = form.ext;
  Gram3Args a;
  a.b = b;
  a.alpha = s->alpha;
  a.beta = s->beta;
  a.u = s->u;
  a.Ns = s->Ns;
  a.G4 = plan.G4;
  a.nsuper = plan.nsuper;
  a.ktiles_per_split = g.kps;
  a.D = ext ? basis->ext_Dp + 2 * basis->ext_df : basis->pow_depth;
  a.recipes = (const uint32_t*)(ext ? basis->d_recipes_ext : basis->d_recipes);
  a.Dp = ext ? basis->ext_Dp : basis->pow_depth;
  a.df = ext ? basis->ext_df : 0;
  a.ng = ext ? basis->ext_ng : 0;
  a.centres = b.centres;
  a.desc = plan.desc;
  a.part = part;
  a.njobs = plan.njobs;
  a.pcs = form.kind == GRAM3_PCS ? b.pcs : nullptr;
  a.nfull4 = (b.nfull + 3) / 4 * 4;
  a.pre = form.kind == GRAM3_PRE ? pre_buf : nullptr;
  a.pre_rl = form.pre_rl;
  a.nsplit_fit = g.nsplit;
  for (int f = 0; f < n; ++f) a.grp[f] = Gram3Src{ss[f]->alpha, ss[f]->beta, ss[f]->u};
  a.pow3 = form.p3;      // (pow3 and eb: nothing reads them; they keep the kernel's argument block the size it has)
  a.lift = form.lo ? lift : nullptr;
  a.eb = form.eb;
  return a;
}

// ss[0 .. n): the snapshot objects of n fits of one dictionary and ONE snapshot count (n > 1: kp_gram3_groupable); their [G | C]
// pairs go to GC_dev + f 2 W^2.  The launch is dealt over the fits (gram3_geometry).  n = 1 is the launch of a single fit, bit for bit.
static int gram3_launch_n(kp_ctx* ctx, const kp_basis* basis_c, const kp_snapshots* const* ss, int n, double* GC_dev, bool cover) {
  kp_basis* basis = const_cast<kp_basis*>(basis_c);
  const BasisDev& b = basis->dev;
  const kp_snapshots* s = ss[0];
  if (n < 1 || n > KP_GRAM_GROUP_MAX) return ctx->fail(KP_ERR_ARG, "kp_fit_gram: bad group size");
  for (int f = 0; f < n; ++f)
    if (ss[f]->nzeta != b.nzeta || ss[f]->m != b.m || ss[f]->Ns != s->Ns) return ctx->fail(KP_ERR_ARG, "kp_fit_gram: snapshot/basis dimension mismatch");
  const int W = b.W, N = b.N, BM = b.m, NWT = (BM + 1) * (BM + 2) / 2;
  const Gram3Switches sw = gram3_switches();
  // 1. the plan this launch runs - and the dictionary's cover plan built now if it has one: workspace 4 is sized for both
  kp_gram3_plan* planp = nullptr;
  int rc = gram3_plan_for(ctx, basis, cover, &planp);
  if (rc) return rc;
  const kp_gram3_plan& plan = *planp;
  if (gram3_cover_mode() != 0) {
    kp_gram3_plan* cov = nullptr;
    rc = gram3_cover_plan(ctx, basis, &cov);
    if (rc) return rc;
  }
  Gram3Facts f = gram3_facts(ctx, basis, plan, s->Ns, n);
  const uint32_t* lift = nullptr;
  if (gram3_mono(f, sw) && sw.lift_order) {
    rc = gram3_lift_table(ctx, basis, &lift);
    if (rc) return rc;
  }
  f.lift_table = lift != nullptr;
  // 2. geometry, 3. the split partials
  const Gram3Geometry g = gram3_geometry(f);
  double* part = (double*)ctx->workspace(4, g.ws4_bytes);
  if (!part) return ctx->fail(KP_ERR_HIP, "kp_fit_gram: out of device memory");
  // 4. form: asked once, the prelift buffer tried where one is wanted, asked again where there is none
  Gram3Form form = gram3_form(f, sw, true);
  if (form.refusal) return ctx->fail(KP_ERR_ARG, form.refusal);
  double* pre_buf = form.want_buffer ? (double*)ctx->workspace(14, form.pre_bytes) : nullptr;
  if (form.want_buffer && !pre_buf) {
    (void)hipGetLastError();
    form = gram3_form(f, sw, false);
  }
  const bool pre = form.kind == GRAM3_PRE;
  if (pre && !form.ext && !basis->d_pcsT) {
    if (hipMalloc(&basis->d_pcsT, (size_t)b.nfull * 32 * 8) != hipSuccess) return ctx->fail(KP_ERR_HIP, "kp_fit_gram: out of device memory");
    KP_HIP(ctx, kp_gram3_pcs_transpose_launch(b.pcs, b.nfull, b.k_pcs, (double*)basis->d_pcsT, ctx->stream));
  }
  // 5. arguments, 6. prelift, 7. kernel, 8. reduction
  const Gram3Args a = gram3_args(basis, plan, form, g, ss, n, part, pre_buf, lift);
  Gram3Events ev{ctx};
  KP_HIP(ctx, ev.begin(n));
  if (pre && form.ext)
    KP_HIP(ctx, kp_gram3_prelift_ext_launch(BM, s->alpha, s->beta, s->u, s->Ns, g.ktiles * KT3, b.nzeta, basis->ext_Dp, basis->ext_df, basis->ext_ng, b.nfull, plan.G4,
                                            (const uint32_t*)basis->d_recipes_ext, b.centres, pre_buf, form.pre_rl, ctx->stream));
  else if (pre)
    KP_HIP(ctx, kp_gram3_prelift_launch(BM, s->alpha, s->beta, s->u, s->Ns, g.ktiles * KT3, b.nzeta, basis->pow_depth, b.nfull, b.k_pcs, N, plan.G4,
                                        (const uint32_t*)basis->d_recipes, (const double*)basis->d_pcsT, pre_buf, form.pre_rl, ctx->stream));
  KP_HIP(ctx, gram3_dispatch(form, a, g.grid, gram3_lds_bytes(f, form), ctx->stream));
  KP_HIP(ctx, ev.after_kernel());
  hipLaunchKernelGGL(kp_gram3_reduce_kernel, dim3(plan.njobs * plan.nq * NWT, n), dim3(g.reduce_block), 0, ctx->stream, part, g.nsplit, plan.njobs,
                     plan.nq, NWT, BM, plan.desc, plan.G4, N, W, GC_dev, GC_dev + (size_t)W * W, plan.dst_off, plan.dst);
  KP_HIP(ctx, hipGetLastError());
  KP_HIP(ctx, ev.after_reduction());
  // 9. what ran
  const Gram3Ran ran = gram3_ran(f, form);
  ctx->gram_flops_per_pair = (double)W * (W + 1) + 2.0 * W * W;
  ctx->timers[10] = ran.mfma_flop_per_pair;
  ctx->timers[15] = ran.two_group_jobs;
  ctx->timers[16] = ran.table_entries;
  ctx->timers[20] = ran.lift_order;
  ctx->timers[26] = ran.early_barrier;
  return KP_OK;
}

int kp_gram3_launch(kp_ctx* ctx, const kp_basis* basis, const kp_snapshots* s, double* GC_dev, bool cover) { return gram3_launch_n(ctx, basis, &s, 1, GC_dev, cover); }

int kp_gram3_launch_group(kp_ctx* ctx, const kp_basis* basis, const kp_snapshots* const* ss, int n, double* GC_dev) {
  return gram3_launch_n(ctx, basis, ss, n, GC_dev, true);
}
