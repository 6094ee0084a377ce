// Internal declarations shared by the translation units of libkoopman_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "koopman_hip.h"
#include "kp_col_desc.h"   // COL_* kinds and ColDesc (HIP-free)

#define KP_MAX_VARS 32
#define KP_GRAM_GROUP_MAX 8   // pipelined fits that may share one Gram launch (kp_fit.hip: KP_GRAM_GROUP)

void kp_set_global_error(const std::string& s);
// kp_traj.hip: the device blocks of a new kp_traj (0 Y, 1 U, 2 Yv, 3 Uv), marked as put - the caller fills them on the
// context's stream, then kp_traj_finish scales them as for an upload
void kp_traj_device_blocks(kp_traj* t, double** blocks);
struct kp_comm_state;   // RCCL communicator of a multi-process run (kp_comm.hip)

struct kp_stage;   // kp_upload.hip: copy stream, pinned staging ring and copy threads of the host -> HBM path

struct kp_ctx {
  int device = 0;
  kp_stage* stage = nullptr;
  std::vector<void*> host_blocks;       // kp_host_alloc: page-locked host buffers handed to the caller
  // device blocks of destroyed trajectory objects, kept for the next kp_traj_upload (a sweep that uploads chunk after chunk
  // paid 5 hipMalloc + 5 hipFree per chunk: 1.3 ms of the 16.5 ms of 1024 systems); at most KP_TRAJ_POOL_MAX blocks,
  // freed by kp_destroy
  std::vector<std::pair<void*, size_t>> traj_pool;
  std::mutex host_mu;                   // ... a gathering host thread may ask for one while another thread drives the device
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t evp[6] = {nullptr};   // gram start, gram end, reduce end, solve end, spare x2
  // second stream of the synchronous fit: the plain solve beside the rank-revealing one of a dictionary with a rank hint
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_gram_done = nullptr;
  // ---- pipelined fits (kp_fit with K_out == NULL; kp_fit.hip): everything runs on `stream` ----
  // A fit takes the next free slot of the [G | C] ring (GC) and, as fit number q of the current batch (the fits since the last
  // kp_synchronize), slot q % kring_cap of the result ring (Kres).  Invariants:
  //   * slots are consecutive: the pend_solves fits awaiting their solve hold [G | C] slots 0 .. pend_solves - 1 and result
  //     slots pend_first .. pend_first + pend_solves - 1 (mod kring_cap); the pend_ngrams newest of them also await their Gram
  //     launch, their [G | C] slots starting at pend_gram_gc
  //   * pend_first is set (to async_count) when pend_solves == 0, i.e. by the first fit of every solve batch
  //   * a failed group launch takes its members back: pend_solves and async_count drop by the group's size, so that no solve
  //     factors an unwritten [G | C] slot and no kp_fit_get_K serves one
  // Everything that enqueues on `stream`, reads a result or frees what a queued fit points to launches the Gram queue first
  // (kp_flush_grams); kp_synchronize launches the solves (kp_flush_pending) and waits.
  bool async_pending = false;  // fits were enqueued since the last kp_synchronize
  int kring_cap = 128;         // result slots; = the default solve batch: a full 128-fit batch needs no kp_fit_async_slots call
  int async_count = 0;         // fits issued in the current batch
  bool batch_closed = true;    // kp_synchronize closed the batch: the next pipelined fit starts a new one
  bool kres_is_ring = false;   // Kres currently holds a pipelined batch (kp_fit_get_K indexes the ring)
  const void* pend_basis = nullptr;   // dictionary / snapshot count / width of the fits in flight: a change drains the pipeline
  int64_t pend_Ns = 0;
  int pend_W = 0;
  // solve queue: the Gram pairs of up to KP_SOLVE_BATCH fits wait in the [G | C] ring and are factored / solved by ONE
  // batched launch sequence (kp_chol_solve_batch_dev)
  int pend_solves = 0, pend_first = 0;
  hipEvent_t ev_solve0 = nullptr, ev_solve1 = nullptr;   // around the most recent batched solve (timer 1)
  int* sticky_info = nullptr;         // device word: set by any deferred factorisation that hit a non-positive pivot
  // Gram queue: up to KP_GRAM_GROUP fits of one dictionary and snapshot count wait here and run as ONE Gram launch and ONE
  // partial reduction (kp_gram3_launch_group)
  const kp_snapshots* pend_grams[KP_GRAM_GROUP_MAX] = {};
  int pend_ngrams = 0;
  const kp_basis* pend_gram_basis = nullptr;
  double* pend_gram_gc = nullptr;
  // timers: start / end events of the most recent pipelined Gram launches (a ring of 64 pairs): kp_synchronize reports the
  // MEAN kernel duration over them (timer 0), not just the last launch
  bool ring_timing = false;           // set around a pipelined Gram launch: it times itself with the event ring and records nothing else
  bool ring_group = false;            // set around a launch of the Gram queue: the launch and its reduction are timed per group
  unsigned ring_skip = 0;
  hipEvent_t ring[2 * 64] = {};
  int ring_pos = 0, ring_n = 0;
  // ... a launch of the Gram queue serves ring_members fits, and a third event follows its partial reduction (timers 0 and 6
  // are sums over the ring divided by the fits served)
  hipEvent_t ring_red[64] = {};
  int ring_members[64] = {};
  bool ring_has_red[64] = {};
  // ---- end of the pipelined fits' state ----
  kp_comm_state* comm = nullptr;      // set by kp_comm_create: rank / world / RCCL communicator
  std::atomic<bool> comm_abandoned{false};   // kp_comm_abandon: a bootstrap still blocked in another thread must not publish `comm`
  bool gc_preloaded = false;          // kp_multi_fit_sharded: ctx->GC already holds the summed [G | C] of all devices - kp_fit skips its Gram launch
  bool reduce_grams = false;          // kp_fit_sharded: all-reduce [G | C] over the ranks between the Gram kernel and the solve
  bool test_hooks = false;          // KP_TEST_HOOKS was set when the context was created: kp_fit honours KP_RANK_HINT_TEST (tests only)
  void* pin_scratch = nullptr;      // growable page-locked host scratch (kp_pinned_scratch): small results read back by direct DMA
  size_t pin_scratch_bytes = 0;
  double* pin_small = nullptr;      // 64 bytes of page-locked host memory: small results (info word + pivot ratio) come back in ONE direct DMA
  int num_cu = 0;
  int64_t hbm_bytes = 0;
  std::string name;
  mutable std::string err;
  double timers[28] = {0};            // (27: bit mask of the kernels the iteration loop of the most recent lasso batch launched, not a time; kp_lasso.hip; 26: where the tiles of the last Kronecker Gram launch had their barrier, 1 in front of the last quad steps, 0 behind the last one; kp_gram3.hip; 25: 1000 x model staged + the tile width of the most recent kp_validate_horizon, not a time; 24: its two kernels, ms; kp_validate_horizon.hip; 23: the regime of the most recent kp_eig, not a time; 22: its kernel, ms; kp_eig_general.hip; 21: kernel of the most recent kp_nmpc_simulate, ms; kp_nmpc.hip; 20: the lift order of the last Kronecker Gram launch, 1 the slot table, 0 tid + 256 j; kp_gram3.hip; 19: kernel of the most recent kp_mpc_simulate, ms; kp_mpc.hip; 18: entry, workgroup order and copies of the most recent batched solve, not a time; kp_solve.hip; 17: which panel kernel and substitution form the most recent rank-revealing solve ran, not a time; kp_pivchol.hip; 16: power-table entries per raw value written by the in-loop build of the last Kronecker Gram launch, 3 or 4; 15: jobs of the last Kronecker Gram launch's plan that span two A groups; kp_gram3.hip; 12: the group size of the Gram queue, 13: fits served by the launches of timer 7; kp_fit.hip; 14: kernel code of the most recent sweep call, not a time; kp_sweep.hip, kp_sweep_gram.hip)
  double gram_flops_per_pair = 0;
  // growable device workspaces
  void* ws[21] = {nullptr};     // slot 8: staging of the collectives, 9: rank-revealing solve, 10 / 11: Grams of the shadow dictionary of a dim_red fit, their half-transformed form
  size_t ws_bytes[21] = {0};   // 12 / 13: column states and results of the lasso homotopy (kp_lasso_path.hip); 14: econ-lifted rows of a dim_red fit (kp_gram3.hip)
                                // 15 / 16: lifted snapshot panels of a wide dictionary, 17: split partials of its products, 18: scratch of the blocked factorisation (kp_wide.hip, kp_solve.hip)
                                // 20: inputs, per-row blocks and results of the batched load observer (kp_observer.hip)
  int last_rank = -1;           // rank found by the most recent solve (W when the Gram matrix was positive definite)
  double last_pivot_ratio = 1.0; // min_i L_ii^2 / G_ii of the most recent synchronous least-squares solve (~1 / cond(G))
  // results of the last kp_fit
  double* Kres = nullptr;   // n_lasso x W x W
  size_t Kres_bytes = 0;
  int Kres_W = 0, Kres_n = 0;
  // last gram (device): G then C, W x W each, column-major
  double* GC = nullptr;
  size_t GC_bytes = 0;
  int GC_W = 0;

  int fail(int code, const std::string& s) const {
    err = s;
    kp_set_global_error(s);
    return code;
  }
  void* workspace(int slot, size_t bytes);  // returns nullptr on failure
};

#define KP_HIP(ctx, expr)                                                                  \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess)                                                                  \
      return (ctx)->fail(KP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));   \
  } while (0)

// Device view of a dictionary, passed by value to kernels.
struct BasisDev {
  int model_type, nzeta, m, nvars;
  int nfull, N, W, k_pcs;
  const ColDesc* cols;    // nfull
  const uint8_t* exps;    // n_mono x nvars
  const double* centres;  // n_gauss x nvars (centre-major)
  const double* pcs;      // nfull x k_pcs column-major
};

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a PER-DEVICE setting: one cache entry per (call site, device), so a
// second context on another GPU of the same process gets its own attribute call
struct KpLdsCache { size_t set[32] = {}; };
inline hipError_t kp_ensure_lds(KpLdsCache& c, const void* func, size_t lds) {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 32) return hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (lds > c.set[dev]) {
    hipError_t e = hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    c.set[dev] = lds;
  }
  return hipSuccess;
}

struct kp_gram_plan;
void kp_gram_plan_free(kp_gram_plan* p);
struct kp_gram2_plan;
void kp_gram2_plan_free(kp_gram2_plan* p);
struct kp_gram3_plan;
void kp_gram3_plan_free(kp_gram3_plan* p);
struct kp_gram5_plan;
void kp_gram5_plan_free(kp_gram5_plan* p);

struct kp_basis {
  kp_ctx* ctx = nullptr;
  BasisDev dev{};
  void* d_cols = nullptr;
  void* d_exps = nullptr;
  void* d_centres = nullptr;
  void* d_pcs = nullptr;
  void* d_recipes = nullptr;   // [nfull] uint32: 4 x 8-bit power-table ids (255 = 1.0)
  void* d_pcsT = nullptr;      // dim_red: pcs as [full column][32 components], zero padded (kp_gram3_prelift_kernel; built on first use)
  int max_degree = 0;
  mutable int rank_hint = 0;   // rank found by the last synchronous fit of this dictionary when its Gram matrix was rank deficient (0: it was not):
                               // only the ORDER of the next fit's work depends on it (kp_fit), never its result
  bool pure_fourier = false;   // every column behind the variables is the constant or a fourier function of fourier_degree with packed digits (ColDesc::pad)
  int fourier_degree = 0;      // degree of the dictionary's fourier block (0: none, or blocks of different degrees): kp_lift_kernel's harmonic table
  int pow_depth = 1;           // largest single-variable exponent
  bool fast = false;           // every column is a product of <= 4 single-variable powers
  int max_factors = 1;         // largest number of single-variable powers in one column (valid if fast)
  kp_gram_plan* plan = nullptr;  // tile->wave plan of the fused Gram kernel (built on first use)
  kp_gram2_plan* plan2 = nullptr;  // plan of the 4x4x4-MFMA Gram kernel (monomial dictionaries)
  kp_gram3_plan* plan3 = nullptr;  // plan of the Kronecker (bilinear) Gram kernel
  kp_gram5_plan* plan5 = nullptr;  // plan of the dense 4x4x4 Gram kernel (linear / nonlinear monomial dictionaries)
  kp_basis* shadow_bil = nullptr;  // linear dim_red dictionaries: the same dictionary as a BILINEAR one (shares every device array; kp_gram_shadow.hip)
  kp_basis* shadow_full = nullptr; // linear / nonlinear dim_red dictionaries: the same dictionary WITHOUT the projection (kp_gram_shadow.hip)
  std::vector<uint32_t> h_recipes; // host copy of the recipes (valid if fast)
  // extended recipes of the Kronecker Gram kernel (kp_gram3): besides powers, the per-variable table may hold the
  // harmonics cos / sin(2 pi j x) of fourier blocks (Ksysid.m:694-731) and, behind the per-variable entries, one entry per
  // gaussian centre (Ksysid.m:790-817).  Entry layout per variable: x^1 .. x^Dp | cos(2 pi x), sin(2 pi x), ... (df pairs);
  // recipe ids: < 128 variable entries (v * D + e, D = Dp + 2 df), 128 + c gaussian centre c, 255 the constant
  bool fast_ext = false;
  int ext_Dp = 1, ext_df = 0, ext_ng = 0, ext_max_factors = 1;
  void* d_recipes_ext = nullptr;
};

struct kp_snapshots {
  kp_ctx* ctx = nullptr;
  int64_t Ns = 0;
  int nzeta = 0, m = 0;
  double* alpha = nullptr;  // Ns x nzeta col-major
  double* beta = nullptr;
  double* u = nullptr;      // Ns x m
  int64_t cap_rows = 0;     // rows the arrays were allocated for (kp_snapshots_update refills them in place)
  // kp_snapshots_update (kp_upload.hip): the refill runs on the copy stream; `ev_ready` follows its last DMA, `ev_read`
  // the last kernel that read the arrays (recorded only once the object has been refilled: `streaming`)
  hipEvent_t ev_ready = nullptr, ev_read = nullptr;
  mutable bool dma_pending = false, read_pending = false;
  bool streaming = false;
};
// page-locked host scratch of at least `bytes` (contents not preserved across calls that grow it); nullptr on failure
void* kp_pinned_scratch(kp_ctx* ctx, size_t bytes);
// a device array of n doubles in *dst (nullptr when n = 0), filled from src unless src is nullptr (kp_context.hip)
int kp_dev_alloc_copy(kp_ctx* ctx, double** dst, const double* src, size_t n);
void kp_stage_destroy(kp_ctx* ctx);
void kp_host_free_all(kp_ctx* ctx);
void kp_traj_pool_free(kp_ctx* ctx);
// ---- launchers of the W <= 16 kernels (kp_small_tile.h) that another file launches, on ctx->stream; the caller checks hipGetLastError ----
struct TrajView;
// kp_small_fit_kernel (kp_small_fit.hip), nb systems of Ns rows: snapshots from alpha / beta / u (Ns_total rows in all) or, with
// tv.Y set, from the trajectories.  Reads KP_BATCH_REFINE; returns whether the power-table recipes lift.
bool kp_small_fit_launch(kp_ctx* ctx, const kp_basis* basis, int nb, const double* alpha, const double* beta, const double* u, int64_t Ns_total,
                         int Ns, const TrajView& tv, double* dK, double* dG, double* dC, int* dS);
// kp_small_project_kernel (kp_small_fit.hip): the M-projection of nb linear models; dM and dS may be nullptr
void kp_small_project_launch(kp_ctx* ctx, int nb, const double* dK, const double* dG, const double* dC, int N, int m, double* dA, double* dB,
                             double* dM, int* dS);
// The Gram pass of the nested sweep (kp_sweep_gram.hip): picks the kernel (KP_SWEEP_GRAM_OLD, KP_SWEEP_GRAM_V1), records ctx->ev0 and
// launches it; timers[10] for a matrix-pipe kernel, *code = the part 1000 G + 100 F + 10 U of the timer-14 code (koopman_hip.h)
int kp_sweep_gram_launch(kp_ctx* ctx, const kp_traj* traj, const kp_basis* basis, int Ns, bool cheb, double* dGc, double* dCc, double* code);
// Workspace 6 of kp_sweep_eval_nested (SweepWs in kp_sweep.hip, which kp_sweep_nested_get_K reads K through): Gc | Cc (nb x Wmax x Wmax)
// | K | G | C | A | B (n_deg x nb x 256 doubles each) | err (n_deg x nb x n) | nb spare status words | status | L1 flags (n_deg x nb
// ints each) | SweepDeg table | ColDesc table (both 64-byte aligned)
// Around every launch sequence that reads a snapshot object.  All readers run on ctx->stream, so one wait orders the
// later ones too.
inline hipError_t kp_snaps_acquire(const kp_snapshots* s, hipStream_t st) {
  if (!s->dma_pending) return hipSuccess;
  s->dma_pending = false;
  return hipStreamWaitEvent(st, s->ev_ready, 0);
}
inline hipError_t kp_snaps_release(const kp_snapshots* s, hipStream_t st) {
  if (!s->streaming) return hipSuccess;
  s->read_pending = true;
  return hipEventRecord(s->ev_read, st);
}

// --- device helpers shared by the lift and gram kernels -----------------------------

// Value of full-basis column `c` at the point whose variables are v[0..nvars) (stride vs).
__device__ __forceinline__ double kp_eval_col(const BasisDev& b, const ColDesc c, const double* v, int vs) {
  switch (c.kind) {
    case COL_VAR:
      return v[c.arg * vs];
    case COL_MONO: {
      const uint8_t* e = b.exps + (size_t)c.arg * b.nvars;
      double p = 1.0;
      for (int i = 0; i < b.nvars; ++i) {
        int ei = e[i];
        if (ei) {
          double x = v[i * vs];
          for (int k = 0; k < ei; ++k) p *= x;
        }
      }
      return p;
    }
    case COL_FOURIER: {
      // index = sum_i digit_i * radix^(nvars-1-i); digit 0 -> 1, 2j-1 -> cos(2 pi j x), 2j -> sin(2 pi j x)
      int radix = 2 * c.aux + 1;
      int idx = c.arg;
      double p = 1.0;
      for (int i = b.nvars - 1; i >= 0; --i) {
        int d = idx % radix;
        idx /= radix;
        if (d) {
          int j = (d + 1) >> 1;
          double a = 2.0 * 3.14159265358979323846 * (double)j * v[i * vs];
          p *= (d & 1) ? cos(a) : sin(a);
        }
      }
      return p;
    }
    case COL_GAUSS: {
      const double* ctr = b.centres + (size_t)c.arg * b.nvars;
      double r2 = 0.0;
      for (int i = 0; i < b.nvars; ++i) {
        double d = v[i * vs] - ctr[i];
        r2 += d * d;
      }
      return exp(-r2);
    }
    case COL_HERMITE: {
      // product of physicists' Hermite polynomials: H0 = 1, H1 = 2x, H_{k+1} = 2x H_k - 2k H_{k-1}
      const uint8_t* e = b.exps + (size_t)c.arg * b.nvars;
      double p = 1.0;
      for (int i = 0; i < b.nvars; ++i) {
        int n = e[i];
        if (n) {
          double x = v[i * vs], h0 = 1.0, h1 = 2.0 * x;
          for (int k = 1; k < n; ++k) {
            double h2 = 2.0 * x * h1 - 2.0 * (double)k * h0;
            h0 = h1;
            h1 = h2;
          }
          p *= h1;
        }
      }
      return p;
    }
    case COL_FSPARSE: {
      const uint8_t* sm = b.exps + (size_t)c.arg * b.nvars;  // sine multipliers, then cosine multipliers
      const uint8_t* cm = sm + b.nvars;
      double p = 1.0;
      for (int i = 0; i < b.nvars; ++i)
        if (sm[i]) p *= sin(2.0 * 3.14159265358979323846 * (double)sm[i] * v[i * vs]);
      for (int i = 0; i < b.nvars; ++i)
        if (cm[i]) p *= cos(2.0 * 3.14159265358979323846 * (double)cm[i] * v[i * vs]);
      return p;
    }
    default:
      return 1.0;
  }
}

// host-side launchers implemented in the .hip files
int kp_gram_launch(kp_ctx* ctx, const kp_basis* basis, const kp_snapshots* s, double* GC_dev);
bool kp_gram2_applicable(const kp_basis* basis);
int kp_gram2_launch(kp_ctx* ctx, const kp_basis* basis, const kp_snapshots* s, double* GC_dev);
// picks the 4x4x4-MFMA kernel when the dictionary allows it, else the general kernel
bool kp_gram3_applicable(const kp_basis* basis);
// cover: the caller is kp_fit's deferred-solve branch - the launch takes the dictionary's cover plan where it has one (kp_gram3_cover.h)
int kp_gram3_launch(kp_ctx* ctx, const kp_basis* basis, const kp_snapshots* s, double* GC_dev, bool cover = false);
// n fits of one dictionary and snapshot count in one launch and one reduction; [G | C] of fit f at GC_dev + f 2 W^2 (kp_gram3.hip).
// Both are the Gram queue's (kp_fit.hip): they plan with the dictionary's cover plan where it has one
bool kp_gram3_groupable(kp_ctx* ctx, const kp_basis* basis, const kp_snapshots* s);
int kp_gram3_launch_group(kp_ctx* ctx, const kp_basis* basis, const kp_snapshots* const* ss, int n, double* GC_dev);
bool kp_gram_congruence_applicable(const kp_basis* basis);
int kp_gram_congruence_launch(kp_ctx* ctx, const kp_basis* basis, const kp_snapshots* s, double* GC_dev);
bool kp_gram3_linear_applicable(const kp_basis* basis);
int kp_gram3_linear_launch(kp_ctx* ctx, const kp_basis* basis, const kp_snapshots* s, double* GC_dev);
void kp_gram3_shadow_free(kp_basis* basis);
bool kp_gram5_applicable(const kp_basis* basis);
int kp_gram5_launch(kp_ctx* ctx, const kp_basis* basis, const kp_snapshots* s, double* GC_dev);
inline int kp_gram_dispatch(kp_ctx* ctx, const kp_basis* basis, const kp_snapshots* s, double* GC_dev, bool cover = false) {
  if (s->Ns > 0 && (!s->alpha || !s->beta || (s->m > 0 && !s->u)))    // an object whose refill failed part-way (kp_snapshots_update)
    return ctx->fail(KP_ERR_ARG, "kp_fit: the snapshot object holds no device arrays (a failed kp_snapshots_update?)");
  KP_HIP(ctx, kp_snaps_acquire(s, ctx->stream));
  const int rc = kp_gram3_applicable(basis)   ? kp_gram3_launch(ctx, basis, s, GC_dev, cover)
                 : kp_gram_congruence_applicable(basis) ? kp_gram_congruence_launch(ctx, basis, s, GC_dev)
                 : kp_gram3_linear_applicable(basis) ? kp_gram3_linear_launch(ctx, basis, s, GC_dev)
                 : kp_gram5_applicable(basis) ? kp_gram5_launch(ctx, basis, s, GC_dev)
                 : kp_gram2_applicable(basis) ? kp_gram2_launch(ctx, basis, s, GC_dev)
                                              : kp_gram_launch(ctx, basis, s, GC_dev);
  if (rc) return rc;
  KP_HIP(ctx, kp_snaps_release(s, ctx->stream));
  return KP_OK;
}
// kp_chol_ll.hip: left-looking single-workgroup Cholesky for n <= 352 (in place, lower triangle; `info` as kp_chol_kernel)
bool kp_chol_ll_applicable(int n);
hipError_t kp_chol_ll_launch(double* Gp, int n, int nb, int* info, int* sticky, int prof, hipStream_t st, const double* thr = nullptr);
// substitution with a factor the caller already holds (kp_solve.hip)
int kp_factor_substitute_dev(kp_ctx* ctx, double* Lp, int n, double* Cp, int ncp, double* Dinv, hipStream_t st, int* form = nullptr);
int kp_copy_to_host_async(kp_ctx* ctx, const void* src_dev, void* dst_host, size_t bytes, int mapped, hipStream_t s);
int kp_pivchol_solve_dev(kp_ctx* ctx, const double* G_dev, const double* C_dev, int W, int ncols, double* K_dev, int* rank, int rank_hint = 0,
                         void* k_host = nullptr, size_t k_bytes = 0, hipEvent_t ev_solved = nullptr, int k_host_mapped = 0);
int kp_comm_allreduce_dev(kp_ctx* ctx, double* buf_dev, size_t count, hipStream_t s);
// queued (deferred) solves of the asynchronous pipeline are launched; nothing is waited for, no status is consumed (kp_fit.hip)
int kp_flush_pending(kp_ctx* ctx);
// the queued Gram launches of the asynchronous pipeline are launched (kp_fit.hip); a no-op when nothing is queued
int kp_flush_grams(kp_ctx* ctx);
int kp_gram_group_size();   // KP_GRAM_GROUP (read once); kp_timer_get(12) reports it
int kp_snapshots_update_rows(kp_ctx* ctx, kp_snapshots* s, const double* alpha, const double* beta, const double* u, int64_t Ns, int64_t ld);
int kp_ensure_gc(kp_ctx* ctx, int W);   // the context's [G | C] buffer for width W (kp_fit.hip)
int kp_lift_dev(kp_ctx* ctx, const kp_basis* basis, int what, const double* dz, const double* du, int64_t rows, double* dout);
// the same with leading dimensions: `rows` rows of input columns ldi apart into output columns ldo apart
int kp_lift_dev_ld(kp_ctx* ctx, const kp_basis* basis, int what, const double* dz, const double* du, int64_t rows, int64_t ldi, double* dout, int64_t ldo);
// dictionaries too wide for the LDS-staged Gram kernels: lifted panels in HBM + TN products on the matrix pipe (kp_wide.hip)
int kp_gram_wide_launch(kp_ctx* ctx, const kp_basis* basis, const kp_snapshots* s, double* GC_dev);
// The dense solver (kp_solve.hip).  Systems up to KP_NARROW_NMAX (padded) are factored by one workgroup and substituted by
// kp_trsm2_kernel; wider ones take the blocked path over all CUs, one system at a time.
#define KP_NARROW_NMAX 512
int kp_chol_solve_dev(kp_ctx* ctx, double* G_dev, double* C_dev, int W, int ncols, double* K_dev, hipStream_t st = nullptr, int* sticky = nullptr);
// the info word and pivot ratio of the kp_chol_solve_dev that ran last on `st` (phases: kp_solve.hip)
int kp_read_chol_info(kp_ctx* ctx, int W, int ncols, int* bad, const double* G_dev = nullptr, hipStream_t st = nullptr, int phase = 0);
// Where kp_chol_solve_dev leaves its info word (non-zero: a non-positive pivot) in workspace 5, behind the padded copies of
// G (np x np), C (np x ncp) and the inverted diagonal blocks: the ONE place that knows the layout (kp_solve.hip, kp_lasso.hip and
// kp_more.hip read the word through it).
inline size_t kp_chol_info_offset(int W, int ncols) {
  const size_t np = (size_t)(W + 15) / 16 * 16, ncp = (size_t)(ncols + 15) / 16 * 16;
  return np * np * 8 + np * ncp * 8 + (np / 16) * 256 * 8;
}
int kp_chol_solve_batch_dev(kp_ctx* ctx, const double* G_dev, const double* C_dev, int W, int ncols, int nb, size_t gc_stride, double* K_dev,
                            int k_first, int k_cap, hipStream_t st, int* sticky);
// least-squares solution, PSD guard and Lipschitz constant shared by all lasso values of one fit (kp_lasso.hip)
struct kp_lasso_prep {
  bool ready = false;
  double L = 0.0, l1_ls = 0.0;
  int bad = 0;
  bool guarded = false;    // the 1e-6 PSD guard of Ksysid.m:1117-1120 was applied (cond(Gw) >= lambda_max / 1e-6)
  double pivot_ratio = 1.0; // min_i L_ii^2 / G_ii of the least-squares factorisation (~1 / cond(G))
  double* Kls = nullptr;   // device, W x ncols
  double* Gw = nullptr;    // device copy of G (with the PSD guard applied when needed)
};
int kp_lasso_dev(kp_ctx* ctx, const double* G_dev, const double* C_dev, int W, int ncols, double t, int max_iter, double tol,
                 double* K_dev, int* iters, kp_lasso_prep* prep = nullptr);
// the lasso values of one fit by the regularisation-path homotopy (kp_lasso_path.hip); stats: steps, largest support, ms, inverse in memory
int kp_lasso_path_batch_dev(kp_ctx* ctx, const double* G_dev, const double* C_dev, int W, int ncols, const double* t, int nv, double* const* K_dev,
                            double* stats, bool known_active = false);
// all lasso values of one fit at once (one wide G*[K_1..K_nv] product per FISTA iteration, active-set polish)
int kp_lasso_batch_dev(kp_ctx* ctx, const double* G_dev, const double* C_dev, int W, int ncols, const double* t, int nv,
                       int max_iter, double tol, double* const* K_dev, int* iters, kp_lasso_prep* prep = nullptr);
