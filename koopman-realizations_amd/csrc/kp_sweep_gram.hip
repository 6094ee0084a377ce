// The Gram pass of the nested sweep (kp_sweep_eval_nested, kp_sweep.hip) in its three generations, oldest first, and the one
// host launcher that chooses among them: kp_sweep_gram_launch at the end of the file.
#include "kp_small_tile.h"
#include <algorithm>
#include <vector>

// ---------------------------------------------------------------------------------------------------------------------
// Gram pass of the nested sweep: G = Px'Px, C = Px'Py of every system straight from its (scaled) trajectories, monomial /
// Chebyshev dictionaries through the power-table recipes, W <= 16.  One workgroup per system, 128 snapshot pairs per tile:
//   * thread (side, p) lifts ONE side of ONE pair: fills its own column of the power table (no barrier between the fill
//     and the reads: a thread only reads what it wrote), forms the N columns and writes its row of Px or Py;
//   * the raw values of the NEXT tile are loaded into registers before the current tile is processed (the global-memory
//     latency is off the critical path; the per-tile chain raw load -> barrier -> table -> barrier -> lift -> barrier of
//     kp_small_fit_kernel is what kept that kernel at a tenth of the f64 rate);
//   * accumulation as there: a lane owns one 4 x 4 block of G and of C for 8 of the 128 pairs, three 16-byte LDS reads
//     per 32 FMAs, the 16 snapshot groups summed in a fixed order at the end.
// Two barriers per 128 pairs.  No solve here: kp_sweep_sub_kernel factors the sub-blocks of every degree.
// ---------------------------------------------------------------------------------------------------------------------
#define TG_TS 128
__global__ __launch_bounds__(256) void kp_traj_gram_kernel(BasisDev b, const uint32_t* __restrict__ recipes, int D, int nfmax, TrajView tv,
                                                           int Ns, int cheb, double* __restrict__ Gout, double* __restrict__ Cout) {
  extern __shared__ __align__(16) double sm[];
  // LDS: Px[TS][LD] | Py[TS][LD] | pw[side][v * D + e - 1][TS] | Gs[16][LD] | Cs[16][LD]
  const int nv = b.nvars, m = b.m, N = b.N, W = b.W, nz = b.nzeta;
  double* Px = sm;
  double* Py = Px + TG_TS * SB_LD;
  double* pw = Py + TG_TS * SB_LD;
  double* Gs = pw + 2 * nv * D * TG_TS;
  double* Cs = Gs + 16 * SB_LD;
  __shared__ uint32_t recs[SB_W];
  const int tid = threadIdx.x, sys = blockIdx.x;
  if (tid < N) recs[tid] = recipes[tid];
  for (int e = tid; e < 2 * TG_TS * SB_LD; e += 256) Px[e] = 0.0;          // unused columns stay zero
  const int side = tid >> 7, p = tid & (TG_TS - 1);
  const int blk = tid & 15, grp = tid >> 4;
  const int bi = (blk >> 2) * 4, bj = (blk & 3) * 4;
  const int Tm1 = tv.T - 1;
  double g[4][4], c[4][4];
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) g[x][y] = c[x][y] = 0.0;
  // raw values of a pair for this thread's side: the nv dictionary variables ([y] or [y; u]), then the m inputs
  double raw[KP_MAX_VARS > 8 ? 8 : KP_MAX_VARS], rin[3];
  auto load_raw = [&](int r0) {
    const int pair = r0 + p;
    const bool ok = pair < Ns;
    const int tr = ok ? (int)(((unsigned long long)pair * tv.div_magic) >> 40) : 0;
    const int row = ok ? tr * tv.T + (pair - tr * Tm1) : 0;
#pragma unroll
    for (int v = 0; v < 8; ++v)
      if (v < nv) {
        // no arithmetic on the loaded value here (not even the tail mask): the wave would wait for the load on the spot
        // instead of at its use, a whole accumulation phase later
        raw[v] = v < nz ? tv.Y[((size_t)sys * tv.n + v) * tv.rows + row + side] : tv.U[((size_t)sys * tv.m + (v - nz)) * tv.rows + row];
      }
#pragma unroll
    for (int i = 0; i < 3; ++i)
      if (i < m) rin[i] = tv.U[((size_t)sys * tv.m + i) * tv.rows + row];
    return ok;
  };
  bool ok_next = load_raw(0);
  __syncthreads();
  for (int r0 = 0; r0 < Ns; r0 += TG_TS) {
    // ---- lift of this thread's (side, pair) from the registers loaded one tile ago ----
    const bool ok = ok_next;
    double* mypw = pw + (size_t)side * nv * D * TG_TS + p;
#pragma unroll
    for (int v = 0; v < 8; ++v)
      if (v < nv) {
        const double x = ok ? raw[v] : 0.0;               // pairs past Ns: zero row (the constant column carries `ok` too)
        double q = x, qm = 1.0;
        for (int k = 0; k < D; ++k) {
          mypw[(v * D + k) * TG_TS] = q;
          const double qn = cheb ? 2.0 * x * q - qm : q * x;
          qm = q;
          q = qn;
        }
      }
    double uin[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) uin[i] = (i < m && ok) ? rin[i] : 0.0;
    double* P = (side ? Py : Px) + p * SB_LD;
    for (int col = 0; col < N; ++col) {
      const uint32_t rc = recs[col];
      double val = ok ? 1.0 : 0.0;
      for (int f = 0; f < nfmax; ++f) {
        const uint32_t id = (rc >> (8 * f)) & 255u;
        const double t = mypw[(id == 255u ? 0u : id) * TG_TS];
        val *= id == 255u ? 1.0 : t;
      }
      P[col] = val;
      if (b.model_type == KP_MODEL_BILINEAR)
#pragma unroll
        for (int i = 0; i < 3; ++i)
          if (i < m) P[(i + 1) * N + col] = val * uin[i];
    }
    if (b.model_type == KP_MODEL_LINEAR)
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (i < m) P[N + i] = uin[i];
    // the next tile's raw values: in flight while this tile is accumulated
    ok_next = load_raw(r0 + TG_TS);
    __syncthreads();
    // ---- accumulation: 16 blocks x 16 snapshot groups of 8 ----
#pragma unroll 2
    for (int s_ = 0; s_ < TG_TS / 16; ++s_) {
      const double* xr = Px + (grp * (TG_TS / 16) + s_) * SB_LD;
      const double* yr = Py + (grp * (TG_TS / 16) + s_) * SB_LD;
      const double2 xa = *reinterpret_cast<const double2*>(xr + bi), xb = *reinterpret_cast<const double2*>(xr + bi + 2);
      const double2 ja = *reinterpret_cast<const double2*>(xr + bj), jb = *reinterpret_cast<const double2*>(xr + bj + 2);
      const double2 ya = *reinterpret_cast<const double2*>(yr + bj), yb = *reinterpret_cast<const double2*>(yr + bj + 2);
      const double xi[4] = {xa.x, xa.y, xb.x, xb.y}, xj[4] = {ja.x, ja.y, jb.x, jb.y}, yj[4] = {ya.x, ya.y, yb.x, yb.y};
#pragma unroll
      for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) {
          g[x][y] += xi[x] * xj[y];
          c[x][y] += xi[x] * yj[y];
        }
    }
    __syncthreads();
  }
  // sum of the 16 snapshot groups in a fixed order
  const int gi = tid >> 4, gj = tid & 15;
  Gs[gi * SB_LD + gj] = 0.0;
  Cs[gi * SB_LD + gj] = 0.0;
  for (int t = 0; t < 16; ++t) {
    __syncthreads();
    if (grp == t) {
#pragma unroll
      for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) {
          Gs[(bi + x) * SB_LD + bj + y] += g[x][y];
          Cs[(bi + x) * SB_LD + bj + y] += c[x][y];
        }
    }
  }
  __syncthreads();
  if (gi < W && gj < W) {
    Gout[(size_t)sys * W * W + (size_t)gj * W + gi] = Gs[gi * SB_LD + gj];
    Cout[(size_t)sys * W * W + (size_t)gj * W + gi] = Cs[gi * SB_LD + gj];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The same Gram pass on the matrix pipe (round 3).  kp_traj_gram_kernel above writes the lifted rows Px, Py to LDS and every
// thread re-reads them for its register block (three 16-byte reads per 32 FMAs): the LDS was busy 60 % of the time and the pass
// ran at 0.15-0.23 of the f64 rate.  Here NO lifted row exists: the power table (T_e(x_v) or x_v^e, the inputs, the tail
// mask, 1 and 0 as extra entries, per (side, pair)) is the only thing in LDS, and a lane builds the operands of
// v_mfma_f64_4x4x4_4b itself as products of F table entries through byte offsets fixed at kernel start:
//   A (row group g)  psi_x[pair k][col 4g + i],  i = lane & 3, k = lane >> 4       (4 values)
//   B                psi_x | psi_y [pair k][col 4 blk + i],  blk = (lane >> 2) & 3   (1 + 1 values)
// 6 F ds_read_b64 and 8 MFMAs per 4 pairs and wave (G and C, 16 x 16 each), no address arithmetic (the k-step enters the
// immediate offset); entry stride 129 doubles: the 16 lanes of a read pass that want 16 different entries of one pair hit 16
// different bank pairs.  A wave owns every fourth 4-pair step of a tile; the four partial sums meet in LDS at the end.
// One barrier per 128 pairs (the table is double buffered).  F = factors per operand value: bilinear columns psi_c u_i get
// their own table entries (UPRO: the filling thread multiplies once per pair what every lane would multiply per step).
// Measured per pass of 1024 systems x 9999 pairs (linear degree 13 | bilinear 6 | nonlinear 4): 0.74 | 0.59 | 0.88 ms ->
// 0.29 | 0.30 | 0.35 ms.  Timing-only ablations of the linear pass: without the MFMA phase 0.12 ms, with an empty tile loop
// 0.04 ms - the matrix phase (0.17 ms) runs at the instruction's rate (4 workgroups per CU x 78 tiles x 64 MFMAs x 16.5
// cycles), and since nothing on the VALU overlaps an f64 MFMA on the same SIMD the table fill and the loads ADD to it.  What
// mattered on the way: raw values 4 tiles ahead instead of 1, and ONE copy of the tile body (unrolled over the prefetch
// stages, the variables and the tail case the kernel was 115 KB of code and no faster than 0.33 ms).
// ---------------------------------------------------------------------------------------------------------------------
#define TGM_STR 129
#define TGM_PD 4                                      // tiles of raw values in flight per thread
#define TGM_NV 4                                      // dictionary variables ([zeta] or [zeta; u]) this kernel takes
template <int F, int DC, int NVC, bool UPRO>
__global__ __launch_bounds__(256, 2) void kp_traj_gram_mfma_kernel(BasisDev b, const uint32_t* __restrict__ recipes, int D_rt, TrajView tv, int Ns,
                                                                    int cheb, double* __restrict__ Gout, double* __restrict__ Cout) {
  extern __shared__ __align__(16) double sm[];
  const int nv = b.nvars, m = b.m, N = b.N, W = b.W, nz = b.nzeta;
  const int D = DC > 0 ? DC : D_rt;                   // DC: the table depth at compile time (the sweep's 13 / 6 / 4): unrolled fill
  // table entries per (side, pair): powers | inputs | mask | 1 | 0 [| u_i x powers, i < m: `upro`, bilinear dictionaries - a
  // column psi_c u_i then costs the lanes no extra factor (6 multiplies per 4 pairs and lane) but the filling thread D]
  const int E = nv * D + m + 3 + (UPRO ? m * nv * D : 0);   // powers | inputs | mask | 0 | 1 [| input x powers]
  // (the 0 entry sits before the 1 entry: the padding columns of a B read use it, and with the sweep's linear dictionary
  //  - 13 powers, input, mask - it is then entry 15 of a read that spans entries 0 .. 15, one bank pair each; as entry 16 it
  //  shared a bank pair with entry 0: 20 % of the kernel's LDS cycles were conflicts, rocprofv3 SQ_LDS_BANK_CONFLICT)
  const int id_u = nv * D, id_mask = id_u + m, id_zero = id_mask + 1, id_one = id_mask + 2, id_up = id_mask + 3;
  const int buf_doubles = 2 * E * TGM_STR;            // one buffer: [side][entry][TGM_STR]
  double* tab = sm;                                   // two buffers
  double* Gs = sm;                                    // [4 waves][2][16][16]: the partial sums, over the table once it is dead
  __shared__ uint32_t recs[SB_W];
  const int tid = threadIdx.x, sys = blockIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < N) recs[tid] = recipes[tid];
  const int side = tid >> 7, p = tid & (TG_TS - 1);
  // constant entries of both buffers
  for (int e = tid; e < 2 * 2 * 2 * TGM_STR; e += 256) {
    const int pp = e % TGM_STR, which = (e / TGM_STR) & 1, sd = (e / (2 * TGM_STR)) & 1, bf = e / (4 * TGM_STR);
    tab[bf * buf_doubles + (sd * E + (which ? id_zero : id_one)) * TGM_STR + pp] = which ? 0.0 : 1.0;
  }
  __syncthreads();
  // ---- this lane's six operand values as F byte offsets each (entries of pair lane >> 4 of k-step `wave`) ----
  const int li = lane & 3, kq = lane >> 4, blk = (lane >> 2) & 3;
  int off[6][F];
#pragma unroll
  for (int sl = 0; sl < 6; ++sl) {
    const int c = sl < 4 ? 4 * sl + li : 4 * blk + li;          // column of Px (slots 0-4) or Py (slot 5)
    const int sd = sl == 5 ? 1 : 0;
    int ids[F];
#pragma unroll
    for (int f = 0; f < F; ++f) ids[f] = id_one;
    if (c >= W) ids[0] = id_zero;
    else {
      int pc = c, iu = -1;                                      // dictionary column and input factor of Px column c
      if (b.model_type == KP_MODEL_LINEAR) { if (c >= N) { pc = -1; iu = c - N; } }
      else if (b.model_type == KP_MODEL_BILINEAR) { pc = c % N; iu = c / N - 1; }
      int nf = 0;
      if (pc >= 0) {
        const uint32_t rc = recs[pc];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          const int id = (int)((rc >> (8 * f)) & 255u);
          if (id != 255 && nf < F) ids[nf++] = id;
        }
      }
      if (iu >= 0) {
        if (UPRO && nf > 0) ids[0] = id_up + iu * nv * D + ids[0];
        else if (nf < F) ids[nf++] = id_u + iu;
      }
      if (nf == 0) ids[0] = id_mask;                            // the constant column: 1 inside the data, 0 past it
    }
#pragma unroll
    for (int f = 0; f < F; ++f) off[sl][f] = (((sd * E + ids[f]) * TGM_STR) + 4 * wave + kq) * 8;
  }
  double accG[4] = {0.0, 0.0, 0.0, 0.0}, accC[4] = {0.0, 0.0, 0.0, 0.0};
  // Raw values of this thread's (side, pair), TGM_PD tiles ahead: a tile is ~0.6 us of matrix work now, less than a trip to
  // HBM under load - fetched ONE tile ahead (as kp_traj_gram_kernel does for its 4.7 us tiles) every tile waited for its data.
  // The stages rotate through register moves (a handful per tile): ONE copy of the tile body - unrolled over the stages the
  // kernel was 115 KB of code.
  constexpr int NVL = NVC > 0 ? NVC : TGM_NV;         // variables at compile time (the sweep: 1 or 2), else up to TGM_NV
  double raw[TGM_PD][NVL], rin[TGM_PD][3];
  double okq[TGM_PD];
  // base addresses of this thread's columns (the per-tile part of an address is the row alone)
  const double* pv[NVL];
  const double* pu[3];
#pragma unroll
  for (int v = 0; v < NVL; ++v)
    pv[v] = v < nz ? tv.Y + ((size_t)sys * tv.n + v) * tv.rows + side : tv.U + ((size_t)sys * tv.m + (v < nv ? v - nz : 0)) * tv.rows;
#pragma unroll
  for (int i = 0; i < 3; ++i) pu[i] = tv.U + ((size_t)sys * tv.m + (i < m ? i : 0)) * tv.rows;
  auto load_raw = [&](int r0, double (&rw)[NVL], double (&ri)[3]) {
    const int pair = r0 + p;
    const bool ok = pair < Ns;
    const int tr = ok ? (int)(((unsigned long long)pair * tv.div_magic) >> 40) : 0;
    const int row = ok ? tr + pair : 0;                // = tr T + (pair - tr (T - 1))
#pragma unroll
    for (int v = 0; v < NVL; ++v)
      if (v < nv) rw[v] = pv[v][row];
#pragma unroll
    for (int i = 0; i < 3; ++i)
      if (i < m) ri[i] = pu[i][row];
    return ok ? 1.0 : 0.0;
  };
#pragma unroll
  for (int st = 0; st < TGM_PD; ++st) okq[st] = load_raw(st * TG_TS, raw[st], rin[st]);
  int bufsel = 0;
  for (int rr = 0; rr < Ns; rr += TG_TS, bufsel ^= 1) {
    // ---- table of this thread's (side, pair): T_1 .. T_D of every variable (the Chebyshev internal basis of the nested
    // sweep), the inputs, the mask.  Entries of a pair past Ns are 0 (times the mask), so that every product is.
    const double okf = okq[0];
    double* my = tab + bufsel * buf_doubles + side * E * TGM_STR + p;
    double ui[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) ui[i] = i < m ? rin[0][i] * okf : 0.0;
    {
#pragma unroll
      for (int v = 0; v < NVL; ++v)
        if (v < nv) {
          const double x = raw[0][v], x2 = x + x;
          double q = x * okf, qm = okf;                // masked recurrence: T_k(x) okf for every k
          auto put = [&](int k, double val) {          // entry (v, k) and, for bilinear dictionaries, its products with the inputs
            my[(v * D + k) * TGM_STR] = val;
            if constexpr (UPRO) {
#pragma unroll
              for (int i = 0; i < 3; ++i)
                if (i < m) my[(id_up + i * nv * D + v * D + k) * TGM_STR] = val * ui[i];
            }
          };
          if constexpr (DC > 0) {
#pragma unroll
            for (int k = 0; k < DC; ++k) {
              put(k, q);
              const double qn = cheb ? x2 * q - qm : x * q;       // T_(k+1)(x) okf, or x^(k+1) okf for a sparse table
              qm = q;
              q = qn;
            }
          } else {
            for (int k = 0; k < D; ++k) {
              put(k, q);
              const double qn = cheb ? x2 * q - qm : x * q;       // T_(k+1)(x) okf, or x^(k+1) okf for a sparse table
              qm = q;
              q = qn;
            }
          }
        }
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (i < m) my[(id_u + i) * TGM_STR] = ui[i];
      my[id_mask * TGM_STR] = okf;
    }
    // rotate the stages, refill the last one
#pragma unroll
    for (int st = 0; st + 1 < TGM_PD; ++st) {
      okq[st] = okq[st + 1];
#pragma unroll
      for (int v = 0; v < NVL; ++v) raw[st][v] = raw[st + 1][v];
#pragma unroll
      for (int i = 0; i < 3; ++i) rin[st][i] = rin[st + 1][i];
    }
    okq[TGM_PD - 1] = load_raw(rr + TGM_PD * TG_TS, raw[TGM_PD - 1], rin[TGM_PD - 1]);
    __syncthreads();
    // ---- 8 of the tile's 32 four-pair steps on this wave ----
    const char* tb = (const char*)(tab + bufsel * buf_doubles);
    {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        double v6[6];
#pragma unroll
        for (int sl = 0; sl < 6; ++sl) {
          double pr = *reinterpret_cast<const double*>(tb + off[sl][0] + j * 128);
#pragma unroll
          for (int f = 1; f < F; ++f) pr *= *reinterpret_cast<const double*>(tb + off[sl][f] + j * 128);
          v6[sl] = pr;
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          accG[g] = __builtin_amdgcn_mfma_f64_4x4x4f64(v6[g], v6[4], accG[g], 0, 0, 0);
          accC[g] = __builtin_amdgcn_mfma_f64_4x4x4f64(v6[g], v6[5], accC[g], 0, 0, 0);
        }
      }
    }
  }
  // ---- the four waves' partial sums, added in a fixed order; D layout: row 4 g + (lane >> 4), column 4 blk + (lane & 3) ----
  __syncthreads();
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    Gs[((wave * 2 + 0) * 16 + 4 * g + kq) * 16 + 4 * blk + li] = accG[g];
    Gs[((wave * 2 + 1) * 16 + 4 * g + kq) * 16 + 4 * blk + li] = accC[g];
  }
  __syncthreads();
  const int gi = tid >> 4, gj = tid & 15;
  if (gi < W && gj < W) {
    double sg = 0.0, sc = 0.0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      sg += Gs[((w * 2 + 0) * 16 + gi) * 16 + gj];
      sc += Gs[((w * 2 + 1) * 16 + gi) * 16 + gj];
    }
    Gout[(size_t)sys * W * W + (size_t)gj * W + gi] = sg;
    Cout[(size_t)sys * W * W + (size_t)gj * W + gi] = sc;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Round 4: the Gram pass of the sweep's own shapes (1 state, 1 input; linear / bilinear / nonlinear polynomial dictionaries in
// the order of def_polyLift) with the COLUMNS of the rows in the table.  kp_traj_gram_mfma_kernel above ran at 0.37-0.45 of the
// f64 matrix rate with 1.3-2.1 VALU instructions beside every MFMA (rocprofv3: SQ_INSTS_VALU / SQ_INSTS_VALU_MFMA_MOPS_F64 =
// 2.3 | 2.4 | 3.1), and on this chip nothing on the VALU overlaps an f64 MFMA of the same SIMD.  Its ISA says where they came
// from: (1) the prefetch stages rotated through register moves - and the move out of the newest stage made every tile wait
// for the load issued one tile earlier (`s_waitcnt vmcnt(0)` at the top of the loop: the "4 tiles ahead" were 1); (2) LDS
// addresses re-formed per tile for the run-time buffer index and column count; (3) selects on the run-time input count;
// (4) for the nonlinear dictionary, every LANE multiplied two table entries per operand value, 48 v_mul_f64 per tile.
// Here: the thread that owns a (side, pair) writes the row's W <= 16 column values themselves (Chebyshev recurrence in
// registers, mixed monomials multiplied ONCE per pair), every MFMA operand is one ds_read with an immediate offset, the tile
// loop is unrolled over the four prefetch stages (fixed registers, no moves, loads really 4 tiles ahead; 6 KB of code), the
// buffer index and the dictionary are compile-time.  Left per tile and wave: the D recurrence steps, <= D products, a 5-
// instruction row index - against 64 MFMAs.
// ---------------------------------------------------------------------------------------------------------------------
template <int MT, int D>
struct TgcShape {
  static constexpr int NV = MT == KP_MODEL_NONLINEAR ? 2 : 1;
  static constexpr int N = MT == KP_MODEL_NONLINEAR ? (D + 1) * (D + 2) / 2 : D + 1;        // dictionary functions, constant included
  static constexpr int W = MT == KP_MODEL_LINEAR ? N + 1 : MT == KP_MODEL_BILINEAR ? 2 * N : N;
  static constexpr int E = W < 16 ? W + 1 : W;                                                 // + one zero entry for the padding columns
};

template <int MT, int D>
__global__ __launch_bounds__(256, 4) void kp_traj_gram_cols_kernel(TrajView tv, int Ns, double* __restrict__ Gout, double* __restrict__ Cout) {
  using S = TgcShape<MT, D>;
  constexpr int W = S::W, E = S::E, N = S::N;
  static_assert(W <= 16, "one 16 x 16 tile");
  // ONE table buffer [side][entry][TGM_STR] and NO barrier in the tile loop: a wave owns pairs [32 wave, 32 wave + 32) of every
  // 128-pair tile - its 64 lanes write exactly the 2 x 32 (side, pair) rows its own eight 4-pair steps read, and the LDS
  // executes one wave's operations in order.  33 KB per workgroup: four workgroups (16 waves) per CU, the whole sweep resident.
  extern __shared__ __align__(16) double sm[];
  double* Gs = sm;                                    // the four waves' partial sums, over the table once it is dead
  const int tid = threadIdx.x, sys = blockIdx.x, lane = tid & 63, wave = tid >> 6;
  const int side = lane >> 5, p = 32 * wave + (lane & 31);
  if (E > W)                                          // the zero entry of both sides
    for (int e = tid; e < 2 * TGM_STR; e += 256) sm[((e / TGM_STR) * E + W) * TGM_STR + e % TGM_STR] = 0.0;
  // ---- MFMA operands.  The four blocks of v_mfma_f64_4x4x4_4b take four different PAIR groups (block = pairs 4 blk .. 4 blk + 3
  // of a 16-pair step), not four column groups: one instruction then adds 16 pairs to ONE 4 x 4 output block (g, h), its four
  // blocks being partial sums that meet in the epilogue.  The A fragment of column group g and the B fragment of the same group
  // are the same register (lane (blk, k, i): psi[pair 4 blk + k][column 4 g + i]), so a 16-pair step reads the four groups of
  // psi_x and of psi_y ONCE - 8 ds_read_b64 for 26 MFMAs (10 for the upper triangle of G = Px'Px, 16 for C = Px'Py) where the
  // column-group form read 24 values for 32 MFMAs and kept the CU's LDS pipe as busy as its matrix pipes ----
  const int li = lane & 3, kq = lane >> 4, blk = (lane >> 2) & 3;
  // column groups 0-2 are always inside the row (W >= 12): base + immediate; group 3 may run into the padding (zero entry)
  // Which of the wave's 32 pairs a (step jj, block, k) slot takes is free (every pair once per tile): position
  // 16 (kq & 1) + 4 blk + 2 jj + (kq >> 1), so that the 32 lanes of a read pass (kq in {0, 1} or {2, 3}; entry stride = 1 mod 32
  // bank pairs) hit bank pairs li + 4 blk + 16 (kq & 1) + const - all different.  (With position 4 blk + kq the two k of a
  // pass overlapped on 15 of 16 bank pairs: rocprofv3 SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.25.)
  const int ppos = 32 * wave + 16 * (kq & 1) + 4 * blk + (kq >> 1);
  const int offa = li * TGM_STR + ppos;
  const int off3 = ((12 + li) < W ? 12 + li : W) * TGM_STR + ppos;
  static_assert(W >= 12, "column groups 0-2 full");
  double accG[10], accC[16];
#pragma unroll
  for (int k = 0; k < 10; ++k) accG[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 16; ++k) accC[k] = 0.0;
  // ---- raw values of this thread's (side, pair), four tiles ahead in FIXED registers (the loop below is unrolled over them) ----
  const int Tm1 = tv.T - 1;
  const double* py = tv.Y + (size_t)sys * tv.rows + side;      // side 1 lifts the successor row (Py)
  const double* pu = tv.U + (size_t)sys * tv.rows;
  // pair -> row = pair + pair / (T - 1), advanced tile by tile without a division: (trial, offset in trial)
  int tr = p / Tm1, rem = p - tr * Tm1, pair = p;
  const int q128 = TG_TS / Tm1, r128 = TG_TS - q128 * Tm1;
  constexpr int PD = 4;                                // tiles of raw values in flight (fixed registers; the mask is re-derived from the pair index)
  double ry[PD], ru[PD];
  auto load_next = [&](double& y, double& u) __attribute__((always_inline)) {
    const bool in = pair < Ns;
    const int row = in ? pair + tr : 0;
    y = py[row];
    u = pu[row];
    pair += TG_TS;
    tr += q128;
    rem += r128;
    if (rem >= Tm1) { rem -= Tm1; ++tr; }
  };
#pragma unroll
  for (int st = 0; st < PD; ++st) load_next(ry[st], ru[st]);
  __syncthreads();                                     // (the zero entries)
  double* const my = sm + side * E * TGM_STR + p;
  auto tile = [&](auto st_c) __attribute__((always_inline)) {
    constexpr int ST = decltype(st_c)::value;
    // ---- the row of this (side, pair): Chebyshev internal basis, T_e(x_v) where the monomial has x_v^e; every entry carries
    // the mask (0 for pairs past Ns), so that every product does ----
    {
      const double okf = (pair - PD * TG_TS) < Ns ? 1.0 : 0.0;      // `pair` runs PD tiles ahead of the tile being lifted
      const double x = ry[ST], uu = ru[ST] * okf, x2 = x + x;
      if constexpr (MT == KP_MODEL_LINEAR) {            // [T_1 .. T_D, 1, u]: written as the recurrence produces them
        double q = x * okf, qm = okf;
#pragma unroll
        for (int k = 0; k < D; ++k) {
          my[k * TGM_STR] = q;
          const double qn = x2 * q - qm;
          qm = q;
          q = qn;
        }
        my[D * TGM_STR] = okf;
        my[(D + 1) * TGM_STR] = uu;
      } else if constexpr (MT == KP_MODEL_BILINEAR) {   // [psi, u psi], psi = [T_1 .. T_D, 1]
        double q = x * okf, qm = okf;
#pragma unroll
        for (int k = 0; k < D; ++k) {
          my[k * TGM_STR] = q;
          my[(N + k) * TGM_STR] = q * uu;
          const double qn = x2 * q - qm;
          qm = q;
          q = qn;
        }
        my[D * TGM_STR] = okf;
        my[(N + D) * TGM_STR] = uu;
      } else {                                          // monomials of [y; u] by total degree, exponent of u ascending inside a degree
        double ty[D], tu[D];
        {
          double q = x * okf, qm = okf;
#pragma unroll
          for (int k = 0; k < D; ++k) {
            ty[k] = q;
            const double qn = x2 * q - qm;
            qm = q;
            q = qn;
          }
        }
        {
          const double xu = ru[ST], xu2 = xu + xu;
          double q = xu * okf, qm = okf;
#pragma unroll
          for (int k = 0; k < D; ++k) {
            tu[k] = q;
            const double qn = xu2 * q - qm;
            qm = q;
            q = qn;
          }
        }
        int c = 0;
#pragma unroll
        for (int d = 1; d <= D; ++d)
#pragma unroll
          for (int e2 = 0; e2 <= d; ++e2) {
            const int e1 = d - e2;
            my[c * TGM_STR] = e2 == 0 ? ty[e1 - 1] : e1 == 0 ? tu[e2 - 1] : ty[e1 - 1] * tu[e2 - 1];
            ++c;
          }
        my[c * TGM_STR] = okf;
      }
    }
    load_next(ry[ST], ru[ST]);                           // this stage's registers are free again: the tile PD ahead
    // ---- this wave's eight 4-pair steps (its own 32 pairs): 6 reads, 8 MFMAs each.  No barrier: the rows were written by
    // this wave, and a wave's LDS operations complete in order ----
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {                        // this wave's 32 pairs: two 16-pair steps
      double v[8];
#pragma unroll
      for (int sl = 0; sl < 8; ++sl)
        v[sl] = sm[((sl & 3) < 3 ? offa + 4 * (sl & 3) * TGM_STR : off3) + (sl >= 4 ? E * TGM_STR : 0) + jj * 2];
      int k = 0;
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int h = g; h < 4; ++h) {
          accG[k] = __builtin_amdgcn_mfma_f64_4x4x4f64(v[g], v[h], accG[k], 0, 0, 0);
          ++k;
        }
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int h = 0; h < 4; ++h) accC[4 * g + h] = __builtin_amdgcn_mfma_f64_4x4x4f64(v[g], v[4 + h], accC[4 * g + h], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);                 // one 16-pair step's operands in registers at a time (128 VGPRs: 4 workgroups per CU)
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the reads above precede the next tile's writes of the same rows
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  const int ntiles = (Ns + TG_TS - 1) / TG_TS;
  for (int t = 0; t < ntiles; t += PD) {                 // tiles past Ns inside the last group are all mask: they add zeros
    tile(std::integral_constant<int, 0>{});
    tile(std::integral_constant<int, 1>{});
    tile(std::integral_constant<int, 2>{});
    tile(std::integral_constant<int, 3>{});
  }
  // ---- epilogue: the four blocks of an accumulator (lanes that differ in blk) are partial sums of one 4 x 4 output block -
  // added first (fixed order: xor 4, then xor 8), then the four waves' sums through LDS, in wave order.  Output block (g, h):
  // row 4 g + (lane >> 4), column 4 h + (lane & 3); G is mirrored from its upper blocks (exactly symmetric) ----
  auto blk_sum = [&](double x) __attribute__((always_inline)) {
    x += __shfl_xor(x, 4, 64);
    x += __shfl_xor(x, 8, 64);
    return x;
  };
  __syncthreads();                                     // the table is dead: Gs = [wave][26][16] doubles (13 KB)
#pragma unroll
  for (int k = 0; k < 10; ++k) {
    const double sg = blk_sum(accG[k]);
    if (blk == 0) Gs[(wave * 26 + k) * 16 + kq * 4 + li] = sg;
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const double sc = blk_sum(accC[k]);
    if (blk == 0) Gs[(wave * 26 + 10 + k) * 16 + kq * 4 + li] = sc;
  }
  __syncthreads();
  const int gi = tid >> 4, gj = tid & 15;                // output entry (row gi, column gj)
  if (gi < W && gj < W) {
    const int gq = gi >> 2, hq = gj >> 2;
    // G: block (g, h) with g <= h is stored; the entry below the block diagonal comes from the transposed block
    const int ga = gq <= hq ? gq : hq, gb = gq <= hq ? hq : gq;
    const int ri = gq <= hq ? gi & 3 : gj & 3, rj = gq <= hq ? gj & 3 : gi & 3;
    const int kg = ga * 4 - ga * (ga - 1) / 2 + (gb - ga);                  // index of (ga, gb) in the order g = 0..3, h = g..3
    double sg = 0.0, sc = 0.0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      sg += Gs[(w * 26 + kg) * 16 + ri * 4 + rj];
      sc += Gs[(w * 26 + 10 + 4 * gq + hq) * 16 + (gi & 3) * 4 + (gj & 3)];
    }
    Gout[(size_t)sys * W * W + (size_t)gj * W + gi] = sg;
    Cout[(size_t)sys * W * W + (size_t)gj * W + gi] = sc;
  }
}

// the recipes def_polyLift gives a degree-D dictionary over nv <= 2 variables (what kp_traj_gram_cols_kernel hard-codes)
static bool tgc_canonical(const kp_basis* basis, int nv, int D) {
  if (!basis->fast || (int)basis->h_recipes.size() != basis->dev.nfull || basis->pow_depth != D) return false;
  std::vector<uint32_t> want;
  for (int d = 1; d <= D; ++d)
    for (int e2 = 0; e2 <= (nv == 2 ? d : 0); ++e2) {
      const int e1 = d - e2;
      uint32_t r = 0xffffffffu;
      int nf = 0;
      auto push = [&](int v, int e) { r = (r & ~(0xffu << (8 * nf))) | ((uint32_t)(v * D + e - 1) << (8 * nf)); ++nf; };
      if (e1 > 0) push(0, e1);
      if (e2 > 0) push(1, e2);
      want.push_back(r);
    }
  want.push_back(0xffffffffu);                         // the constant
  if (want.size() != basis->h_recipes.size()) return false;
  for (size_t i = 0; i < want.size(); ++i)
    if (want[i] != basis->h_recipes[i]) return false;
  return true;
}

int kp_sweep_gram_launch(kp_ctx* ctx, const kp_traj* traj, const kp_basis* basis, int Ns, bool cheb, double* dGc, double* dCc, double* code) {
  const BasisDev& b = basis->dev;
  const int nb = traj->nb, n = traj->n, m = traj->m, nv = b.nvars, Dp = basis->pow_depth;
  hipStream_t s = ctx->stream;
  if (!basis->d_recipes || nv > 8) return ctx->fail(KP_ERR_ARG, "kp_sweep_eval_nested: dictionary not supported by the power-table lift");
  const size_t lds = ((size_t)2 * TG_TS * SB_LD + (size_t)2 * nv * Dp * TG_TS + 2 * 16 * SB_LD) * sizeof(double);
  // the matrix-pipe form: factors per operand value = monomial factors (+ the input of a bilinear column); two table buffers
  const int nfac0 = basis->max_factors > 0 ? basis->max_factors : 1;
  const size_t lds_up = (size_t)2 * 2 * (nv * Dp * (1 + m) + m + 3) * TGM_STR * sizeof(double);
  const int upro = b.model_type == KP_MODEL_BILINEAR && lds_up <= 78 * 1024;        // input products in the table
  const int nfac = nfac0 + (b.model_type == KP_MODEL_BILINEAR && !upro ? 1 : 0);
  const size_t lds_m = std::max(upro ? lds_up : (size_t)2 * 2 * (nv * Dp + m + 3) * TGM_STR * sizeof(double), (size_t)4 * 2 * 256 * sizeof(double));
  static const bool gram_old = getenv("KP_SWEEP_GRAM_OLD") != nullptr;
  const bool use_mfma = !gram_old && nfac <= 5 && nv <= TGM_NV && lds_m <= 78 * 1024;      // two workgroups per CU
  if (!use_mfma && lds > 150 * 1024) return ctx->fail(KP_ERR_ARG, "kp_sweep_eval_nested: dictionary too large for the power-table lift");
  // round 4: the sweep's own shapes (1 state, 1 input, canonical polynomial dictionary) with the row's columns in the table
  static const bool cols_off = getenv("KP_SWEEP_GRAM_V1") != nullptr;
  bool use_cols = false;
  int code_g = 1, code_f = 0, code_u = 0;              // timer 14: which Gram kernel this call runs (koopman_hip.h)
  if (!cols_off && !gram_old && n == 1 && m == 1 && b.nzeta == 1 && b.k_pcs == 0 && tgc_canonical(basis, nv, Dp)) {
#define KP_TGC(MT_, D_)                                                                                                           \
    {                                                                                                                             \
      static KpLdsCache tgc_lds;                                                                                                  \
      const size_t lds_c = std::max((size_t)2 * TgcShape<MT_, D_>::E * TGM_STR * sizeof(double), (size_t)4 * 26 * 16 * sizeof(double)); \
      KP_HIP(ctx, kp_ensure_lds(tgc_lds, (const void*)kp_traj_gram_cols_kernel<MT_, D_>, lds_c));                                 \
      KP_HIP(ctx, hipEventRecord(ctx->ev0, s));                                                                                   \
      hipLaunchKernelGGL((kp_traj_gram_cols_kernel<MT_, D_>), dim3(nb), dim3(256), lds_c, s, traj_view(traj), Ns, dGc, dCc);      \
      use_cols = true;                                                                                                            \
      code_g = 2;                                                                                                                 \
      ctx->timers[10] = 26.0 * 512.0 / 16.0;   /* executed on the matrix pipe per pair: 10 + 16 MFMAs per 16 pairs */            \
    }
    if (b.model_type == KP_MODEL_LINEAR && Dp == 13) KP_TGC(KP_MODEL_LINEAR, 13)
    else if (b.model_type == KP_MODEL_BILINEAR && Dp == 6) KP_TGC(KP_MODEL_BILINEAR, 6)
    else if (b.model_type == KP_MODEL_NONLINEAR && Dp == 4) KP_TGC(KP_MODEL_NONLINEAR, 4)
#undef KP_TGC
  }
  if (use_cols) {
  } else if (use_mfma) {
    ctx->timers[10] = 8.0 * 512.0 / 4.0;         // 8 MFMAs per 4 pairs (one padded 16 x 16 tile for G and for C)
#define KP_TGM(F_, DC_, NV_, UP_)                                                                                               \
    {                                                                                                                             \
      static KpLdsCache tgm_lds;                                                                                                  \
      KP_HIP(ctx, kp_ensure_lds(tgm_lds, (const void*)kp_traj_gram_mfma_kernel<F_, DC_, NV_, UP_>, lds_m));                       \
      KP_HIP(ctx, hipEventRecord(ctx->ev0, s));                                                                                   \
      hipLaunchKernelGGL((kp_traj_gram_mfma_kernel<F_, DC_, NV_, UP_>), dim3(nb), dim3(256), lds_m, s, b,                         \
                         (const uint32_t*)basis->d_recipes, Dp, traj_view(traj), Ns, cheb ? 1 : 0, dGc, dCc);                     \
      code_g = (DC_) > 0 ? 3 : 4; code_f = F_; code_u = (UP_) ? 1 : 0;                                                            \
    }
    // the shapes of evaluate_rand_models.m (1-D systems: linear degree 13, bilinear 6, nonlinear 4) with the table depth and
    // the variable count at compile time; everything else with run-time values
    if (nfac == 1 && Dp == 13 && nv == 1 && !upro) KP_TGM(1, 13, 1, false)
    else if (nfac == 1 && Dp == 6 && nv == 1 && upro) KP_TGM(1, 6, 1, true)
    else if (nfac == 2 && Dp == 4 && nv == 2 && !upro) KP_TGM(2, 4, 2, false)
    else if (upro) switch (nfac) {
      case 1: KP_TGM(1, 0, 0, true) break;
      case 2: KP_TGM(2, 0, 0, true) break;
      case 3: KP_TGM(3, 0, 0, true) break;
      default: KP_TGM(4, 0, 0, true) break;
    }
    else switch (nfac) {
      case 1: KP_TGM(1, 0, 0, false) break;
      case 2: KP_TGM(2, 0, 0, false) break;
      case 3: KP_TGM(3, 0, 0, false) break;
      case 4: KP_TGM(4, 0, 0, false) break;
      default: KP_TGM(5, 0, 0, false) break;
    }
#undef KP_TGM
  } else {
    static KpLdsCache tg_lds;
    KP_HIP(ctx, kp_ensure_lds(tg_lds, (const void*)kp_traj_gram_kernel, lds));
    KP_HIP(ctx, hipEventRecord(ctx->ev0, s));
    hipLaunchKernelGGL(kp_traj_gram_kernel, dim3(nb), dim3(256), lds, s, b, (const uint32_t*)basis->d_recipes, Dp, basis->max_factors > 0 ? basis->max_factors : 1,
                       traj_view(traj), Ns, cheb ? 1 : 0, dGc, dCc);
  }
  KP_HIP(ctx, hipGetLastError());
  *code = 1000.0 * code_g + 100.0 * code_f + 10.0 * code_u;
  return KP_OK;
}
