// Host entry points of the EDMD fit  K = Px \ Py  (Ksysid.m:1069): Gram launch (kp_gram*.hip), then the normal-equation solve
// G K = C (kp_solve.hip).  No kernels here.
//
//   kp_fit with a K_out   one fit, synchronous (fit_now): Gram, solve, K and its rank back to the caller
//   kp_fit without        pipelined (fit_enqueue): the fit joins the Gram queue and the solve queue of the context; nothing is
//                         waited for until kp_synchronize / kp_fit_get_K.  Queue state and its invariants: kp_ctx, kp_internal.h
#include <cstdlib>

#include <vector>
#include <algorithm>
#include <cstring>

#include "kp_internal.h"

extern "C" int kp_synchronize(kp_ctx* ctx);

// timers: 0 = fused lift+Gram kernel, 6 = partial-tile reduction, 1 = solve (when run)
static void collect_gram_timers(kp_ctx* ctx, bool solved) {
  float ms = 0;
  bool red_done = false;
  if (ctx->ring_n > 0) {                          // pipelined fits: mean over the last ring_n Gram launches
    // (a launch of the Gram queue serves ring_members fits: time per FIT = sum of the launches / sum of their fits; the same for
    // the reductions that were timed)
    double sum = 0.0, rsum = 0.0;
    int cnt = 0, fits = 0, rfits = 0;
    for (int i = 0; i < ctx->ring_n; ++i) {
      const int p = (ctx->ring_pos - 1 - i + 2 * 64) % 64;
      if (hipEventElapsedTime(&ms, ctx->ring[2 * p], ctx->ring[2 * p + 1]) == hipSuccess) {
        sum += ms;
        fits += std::max(1, ctx->ring_members[p]);
        ++cnt;
        if (ctx->ring_has_red[p] && hipEventElapsedTime(&ms, ctx->ring[2 * p + 1], ctx->ring_red[p]) == hipSuccess) {
          rsum += ms;
          rfits += std::max(1, ctx->ring_members[p]);
        }
      }
    }
    if (cnt) ctx->timers[0] = (float)(sum / fits);
    ctx->timers[7] = (float)cnt;
    ctx->timers[13] = (float)fits;
    ctx->ring_n = 0;
    if (rfits) ctx->timers[6] = (float)(rsum / rfits);
    red_done = rfits > 0;
  } else if (hipEventElapsedTime(&ms, ctx->evp[0], ctx->evp[1]) == hipSuccess) {
    ctx->timers[0] = ms;
    ctx->timers[7] = 1.0f;
    ctx->timers[13] = 1.0f;
  }
  if (!red_done && hipEventElapsedTime(&ms, ctx->evp[1], ctx->evp[2]) == hipSuccess) ctx->timers[6] = ms;
  if (solved && hipEventElapsedTime(&ms, ctx->evp[2], ctx->evp[3]) == hipSuccess) ctx->timers[1] = ms;
  (void)hipGetLastError();   // an event pair that was not recorded in this mode leaves a sticky error behind: not a failure
}

static int ensure_gc(kp_ctx* ctx, int W, int slots = 2) {
  size_t need = (size_t)std::max(2, slots) * 2 * W * W * 8;   // [G | C] buffers: pipelined fits queue in a ring
  if (ctx->GC_bytes < need) {
    if (ctx->GC) (void)hipFree(ctx->GC);
    ctx->GC = nullptr;
    ctx->GC_bytes = 0;
    KP_HIP(ctx, hipMalloc((void**)&ctx->GC, need));
    ctx->GC_bytes = need;
  }
  ctx->GC_W = W;
  return KP_OK;
}

static int ensure_kres(kp_ctx* ctx, int W, int n) {
  size_t need = (size_t)n * W * W * 8;
  if (ctx->Kres_bytes < need) {
    if (ctx->Kres) (void)hipFree(ctx->Kres);
    ctx->Kres = nullptr;
    ctx->Kres_bytes = 0;
    KP_HIP(ctx, hipMalloc((void**)&ctx->Kres, need));
    ctx->Kres_bytes = need;
  }
  ctx->Kres_W = W;
  ctx->Kres_n = n;
  return KP_OK;
}

int kp_ensure_gc(kp_ctx* ctx, int W) { return ensure_gc(ctx, W); }

extern "C" int kp_fit_gram(kp_ctx* ctx, const kp_basis* basis, const kp_snapshots* snaps, double* G, double* C) {
  if (!ctx || !basis || !snaps) return ctx ? ctx->fail(KP_ERR_ARG, "kp_fit_gram: NULL handle") : KP_ERR_ARG;
  KP_HIP(ctx, hipSetDevice(ctx->device));
  const int W = basis->dev.W;
  int rc = ctx->async_pending ? kp_synchronize(ctx) : KP_OK;
  if (rc) return rc;
  rc = ensure_gc(ctx, W);
  if (rc) return rc;
  rc = kp_gram_dispatch(ctx, basis, snaps, ctx->GC);
  if (rc) return rc;
  size_t bW = (size_t)W * W * 8;
  if (G) KP_HIP(ctx, hipMemcpyAsync(G, ctx->GC, bW, hipMemcpyDeviceToHost, ctx->stream));
  if (C) KP_HIP(ctx, hipMemcpyAsync(C, ctx->GC + (size_t)W * W, bW, hipMemcpyDeviceToHost, ctx->stream));
  KP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  collect_gram_timers(ctx, false);
  return KP_OK;
}

extern "C" int kp_fit_solve(kp_ctx* ctx, const double* G, const double* C, int W, int ncols, double* K) {
  if (!ctx || !G || !C || !K || W < 1 || ncols < 1) return ctx ? ctx->fail(KP_ERR_ARG, "kp_fit_solve: bad argument") : KP_ERR_ARG;
  KP_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->async_pending) {
    int rc0 = kp_synchronize(ctx);
    if (rc0) return rc0;
  }
  size_t bG = (size_t)W * W * 8, bC = (size_t)W * ncols * 8;
  char* ws = (char*)ctx->workspace(6, bG + 2 * bC);
  if (!ws) return ctx->fail(KP_ERR_HIP, "kp_fit_solve: out of device memory");
  double* Gd = (double*)ws;
  double* Cd = (double*)(ws + bG);
  double* Kd = (double*)(ws + bG + bC);
  KP_HIP(ctx, hipMemcpyAsync(Gd, G, bG, hipMemcpyHostToDevice, ctx->stream));
  KP_HIP(ctx, hipMemcpyAsync(Cd, C, bC, hipMemcpyHostToDevice, ctx->stream));
  KP_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  int rc = kp_chol_solve_dev(ctx, Gd, Cd, W, ncols, Kd);
  if (rc) return rc;
  KP_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  KP_HIP(ctx, hipMemcpyAsync(K, Kd, bC, hipMemcpyDeviceToHost, ctx->stream));
  int bad = 0;
  rc = kp_read_chol_info(ctx, W, ncols, &bad, Gd);
  if (rc) return rc;
  float ms = 0;
  (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
  ctx->timers[1] = ms;
  ctx->last_rank = W;
  if (bad) {
    // rank-deficient dictionary: MATLAB's `\` warns and returns a basic solution (QR with column pivoting); same here
    int r = 0;
    rc = kp_pivchol_solve_dev(ctx, Gd, Cd, W, ncols, Kd, &r);
    if (rc) return rc;
    ctx->last_rank = r;
    KP_HIP(ctx, hipMemcpyAsync(K, Kd, bC, hipMemcpyDeviceToHost, ctx->stream));
    KP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->err = "warning: Gram matrix is rank deficient; basic solution returned (kp_fit_last_rank)";
  }
  return KP_OK;
}

extern "C" int kp_fit_last_pivot_ratio(const kp_ctx* ctx, double* ratio) {
  if (!ctx || !ratio) return KP_ERR_ARG;
  *ratio = ctx->last_pivot_ratio;
  return KP_OK;
}

extern "C" int kp_fit_last_rank(const kp_ctx* ctx, int* rank) {
  if (!ctx || !rank) return KP_ERR_ARG;
  *rank = ctx->last_rank;
  return KP_OK;
}

// Pipelined fits, deferred solves: the queued Gram pairs are factored and solved by one batched launch sequence on the Gram
// stream (Cholesky: one workgroup per fit, all at once; TRSM: W/16 workgroups per fit).  KP_SOLVE_BATCH (read once) = fits per
// sequence; 1, or anything below it: every fit is solved as soon as its Gram is launched.
static int solve_batch_size() {
  static const int v = [] { const char* e = getenv("KP_SOLVE_BATCH"); return e ? std::max(1, atoi(e)) : 128; }();   // (128 against 64: 0.4171 against 0.4191 ms per pipelined fit; capped by the result ring)
  return v;
}

// Fits per Gram launch of the deferred-solve pipeline: KP_GRAM_GROUP (read once; 1: every fit is launched at once, on its own)
int kp_gram_group_size() {
  static const int v = [] { const char* e = getenv("KP_GRAM_GROUP"); return e ? std::min(KP_GRAM_GROUP_MAX, std::max(1, atoi(e))) : 5; }();   // (5 / 6 / 7 / 8 measured with the cover plan's six workgroups per split - 85 split units: 17 per fit fill 510 of 512 slots - DESIGN 6.2; 2 / 4 / 8 before it: 6.1)
  return v;
}

// The queued fits as ONE Gram launch and ONE partial reduction.  Called by everything that enqueues behind them, reads a result
// or frees what they point to (DESIGN 3.2 lists the entries).
int kp_flush_grams(kp_ctx* ctx) {
  const int n = ctx->pend_ngrams;
  if (n == 0) return KP_OK;
  ctx->pend_ngrams = 0;                 // (whatever happens below: the queue is not launched twice)
  // A launch that fails leaves the members' [G | C] slots unwritten: they - the n newest of the solve batch and of the result
  // ring - are taken back, so that no later solve factors them and no kp_fit_get_K serves them
  auto failed = [&](int rc) {
    ctx->pend_solves = std::max(0, ctx->pend_solves - n);
    ctx->async_count = std::max(0, ctx->async_count - n);
    return rc;
  };
  if (hipError_t e = hipSetDevice(ctx->device); e != hipSuccess)
    return failed(ctx->fail(KP_ERR_HIP, std::string("kp_flush_grams: hipSetDevice: ") + hipGetErrorString(e)));
  // (an acquire only makes the stream wait for a member's refill: members acquired before a failing one hold nothing that would
  // have to be released - kp_snaps_release marks a READ, and nothing has read; the failing member's refill stays pending)
  for (int f = 0; f < n; ++f) {
    const bool was_pending = ctx->pend_grams[f]->dma_pending;
    if (hipError_t e = kp_snaps_acquire(ctx->pend_grams[f], ctx->stream); e != hipSuccess) {
      ctx->pend_grams[f]->dma_pending = was_pending;
      return failed(ctx->fail(KP_ERR_HIP, std::string("kp_flush_grams: ") + hipGetErrorString(e)));
    }
  }
  ctx->ring_timing = true;
  ctx->ring_group = true;
  const int rc = kp_gram3_launch_group(ctx, ctx->pend_gram_basis, ctx->pend_grams, n, ctx->pend_gram_gc);
  ctx->ring_timing = false;
  ctx->ring_group = false;
  if (rc) return failed(rc);
  for (int f = 0; f < n; ++f) KP_HIP(ctx, kp_snaps_release(ctx->pend_grams[f], ctx->stream));
  return KP_OK;
}

static int flush_solves(kp_ctx* ctx) {
  {
    int rcg = kp_flush_grams(ctx);
    if (rcg) return rcg;
  }
  if (ctx->pend_solves == 0) return KP_OK;
  const int W = ctx->pend_W;
  KP_HIP(ctx, hipEventRecord(ctx->ev_solve0, ctx->stream));
  int rc = kp_chol_solve_batch_dev(ctx, ctx->GC, ctx->GC + (size_t)W * W, W, W, ctx->pend_solves, (size_t)2 * W * W, ctx->Kres, ctx->pend_first,
                                   ctx->kring_cap, ctx->stream, ctx->sticky_info);
  ctx->pend_solves = 0;
  if (rc) return rc;
  KP_HIP(ctx, hipEventRecord(ctx->ev_solve1, ctx->stream));
  return KP_OK;
}

int kp_flush_pending(kp_ctx* ctx) { return flush_solves(ctx); }

// A pipelined fit (kp_fit without K_out): its [G | C] goes into the next slot of the ring and its K will go into the next slot
// of the result ring; nothing else runs beside the Gram kernel and nothing is waited for.  The caller (kp_fit) has drained the
// pipeline if the dictionary, the snapshot count or W changed.
static int fit_enqueue(kp_ctx* ctx, const kp_basis* basis, const kp_snapshots* snaps, int W) {
  if (ctx->batch_closed) {
    ctx->async_count = 0;
    ctx->batch_closed = false;
  }
  int rc = ensure_kres(ctx, W, ctx->kring_cap);
  if (rc) return rc;
  ctx->kres_is_ring = true;
  ctx->pend_basis = (const void*)basis;
  ctx->pend_Ns = snaps->Ns;
  ctx->pend_W = W;
  const int sbatch = std::min(solve_batch_size(), ctx->kring_cap);
  rc = ensure_gc(ctx, W, sbatch);
  if (rc) return rc;
  {   // the batched solve's padded workspace, sized for a full batch NOW: growing it at the first full flush would put a
      // hipFree / hipMalloc of ~150 MB (tens of ms) in the middle of the pipeline
    const int np_ = (W + 15) / 16 * 16;
    const size_t per = (size_t)np_ * np_ * 8 * 2 + (size_t)(np_ / 16) * 256 * 8;
    if (!ctx->workspace(5, (size_t)sbatch * per + (size_t)sbatch * 4 + 64)) return ctx->fail(KP_ERR_HIP, "kp_fit: out of device memory");
  }
  if (ctx->pend_solves == 0) ctx->pend_first = ctx->async_count;
  double* GCs = ctx->GC + (size_t)ctx->pend_solves * 2 * W * W;
  // Fits of the Kronecker kernel's plain form wait for up to KP_GRAM_GROUP of their kind (same dictionary, snapshot count and
  // width: any change has drained the pipeline) and share ONE Gram launch and ONE partial reduction: each gets a share of the
  // chip's wave slots, so its split partials - written and read back once per fit - are 1 / group of a lone launch's.  The
  // solves are deferred anyway: no K is available before the caller synchronises.
  if (kp_gram_group_size() > 1 && kp_gram3_groupable(ctx, basis, snaps)) {
    if (snaps->Ns > 0 && (!snaps->alpha || !snaps->beta || (snaps->m > 0 && !snaps->u)))
      return ctx->fail(KP_ERR_ARG, "kp_fit: the snapshot object holds no device arrays (a failed kp_snapshots_update?)");
    if (ctx->pend_ngrams == 0) ctx->pend_gram_gc = GCs;
    ctx->pend_gram_basis = basis;
    ctx->pend_grams[ctx->pend_ngrams++] = snaps;
    ++ctx->pend_solves;
    ++ctx->async_count;
    ctx->async_pending = true;
    // (a full group, or no room left in the solve batch - the batch can be as small as the result ring)
    if (ctx->pend_solves >= sbatch) return flush_solves(ctx);
    if (ctx->pend_ngrams >= kp_gram_group_size()) return kp_flush_grams(ctx);
    return KP_OK;
  }
  rc = kp_flush_grams(ctx);
  if (rc) return rc;
  ctx->ring_timing = true;
  rc = kp_gram_dispatch(ctx, basis, snaps, GCs, true);           // (a fit too long to share a launch: the same plan as the queue's)
  ctx->ring_timing = false;
  if (rc) return rc;
  ++ctx->pend_solves;
  ++ctx->async_count;
  ctx->async_pending = true;
  if (ctx->pend_solves >= sbatch) return flush_solves(ctx);
  return KP_OK;
}

// One fit, synchronous: Gram, solve(s), K_out (or the context's Kres for kp_fit_get_K) and the rank.  The caller (kp_fit) has
// drained the pipeline.
static int fit_now(kp_ctx* ctx, const kp_basis* basis, const kp_snapshots* snaps, const double* lasso, int n_lasso, double* K_out, int W, int N,
                   bool all_ls) {
  int rc = ensure_kres(ctx, W, n_lasso);
  if (rc) return rc;
  ctx->kres_is_ring = false;
  ctx->batch_closed = true;
  if (!ctx->gc_preloaded) {
    rc = kp_gram_dispatch(ctx, basis, snaps, ctx->GC);  // records ev0/ev1 around gram+reduce
    if (rc) return rc;
  }
  if (ctx->reduce_grams) {   // one fit sharded over snapshots: the only exchange is this all-reduce of [G | C]
    rc = kp_comm_allreduce_dev(ctx, ctx->GC, (size_t)2 * W * W, ctx->stream);
    if (rc) return rc;
  }
  double* Gd = ctx->GC;
  double* Cd = ctx->GC + (size_t)W * W;
  int ls_index = -1;
  if (ctx->test_hooks) {                    // (contexts created with KP_TEST_HOOKS set: a remembered rank that is wrong in a chosen way)
    if (const char* e = getenv("KP_RANK_HINT_TEST")) basis->rank_hint = atoi(e);
  }
  // (see below) least-squares values only, the narrow path, a second stream to run on
  const bool concurrent = basis->rank_hint > 0 && all_ls && ctx->stream2 && W <= KP_NARROW_NMAX && !ctx->reduce_grams && !ctx->gc_preloaded &&
                          !getenv("KP_NO_RANK_HINT");
  bool conc_done = false, conc_copied = false;
  int conc_bad = 0, conc_rank = 0;
  const size_t k_bytes = (size_t)n_lasso * W * W * 8;
  double* k_pin = (K_out && k_bytes <= ((size_t)64 << 20)) ? (double*)kp_pinned_scratch(ctx, k_bytes) : nullptr;
  // the least-squares solution is also the inactive-constraint answer of the lasso path; all lasso values run as one batch
  std::vector<double> tv;
  std::vector<double*> tdst;
  for (int i = 0; i < n_lasso; ++i) {
    double* Ki = ctx->Kres + (size_t)i * W * W;
    bool is_ls = (!lasso || !(lasso[i] < 1e6));  // Ksysid.m:1068 (Inf was mapped to 1e6 at :155-157)
    if (is_ls) {
      if (ls_index >= 0) {
        KP_HIP(ctx, hipMemcpyAsync(Ki, ctx->Kres + (size_t)ls_index * W * W, (size_t)W * W * 8, hipMemcpyDeviceToDevice, ctx->stream));
      } else if (concurrent) {
        // The dictionary's last fit was rank deficient: the plain factorisation - still what DECIDES, so that no result depends
        // on the history - runs on the second stream into a scratch K, beside the rank-revealing solve that will most likely
        // be the answer, instead of in front of it with a host round trip between the two (~50 us of a 0.64 ms fit).
        double* Ks = (double*)ctx->workspace(19, (size_t)W * W * 8);
        if (!Ks) return ctx->fail(KP_ERR_HIP, "kp_fit: out of device memory");
        KP_HIP(ctx, hipEventRecord(ctx->ev_gram_done, ctx->stream));
        KP_HIP(ctx, hipStreamWaitEvent(ctx->stream2, ctx->ev_gram_done, 0));
        rc = kp_chol_solve_dev(ctx, Gd, Cd, W, W, Ks, ctx->stream2, nullptr);
        if (rc) return rc;
        ls_index = i;
        if (ctx->pin_small) {                                                                   // (its verdict is ready long before it is read)
          rc = kp_read_chol_info(ctx, W, W, &conc_bad, Gd, ctx->stream2, 1);
          if (rc) return rc;
        }
        // (one value: its K goes to the caller's page-locked block in front of the solve's own synchronisation, not behind it)
        conc_copied = K_out && n_lasso == 1;
        rc = kp_pivchol_solve_dev(ctx, Gd, Cd, W, W, Ki, &conc_rank, basis->rank_hint, conc_copied ? (k_pin ? (void*)k_pin : (void*)K_out) : nullptr,
                                  k_bytes, ctx->evp[3], k_pin ? 1 : 0);      // (synchronises the first stream)
        if (rc) return rc;
        rc = kp_read_chol_info(ctx, W, W, &conc_bad, Gd, ctx->stream2, ctx->pin_small ? 2 : 0);  // (and the second)
        if (rc) return rc;
        if (!conc_bad) {                                                                        // full rank after all
          KP_HIP(ctx, hipMemcpyAsync(Ki, Ks, (size_t)W * W * 8, hipMemcpyDeviceToDevice, ctx->stream));
          conc_copied = false;
        }
        conc_done = true;
      } else {
        rc = kp_chol_solve_dev(ctx, Gd, Cd, W, W, Ki);
        if (rc) return rc;
        ls_index = i;
      }
    } else {
      tv.push_back(lasso[i] * N);   // t = lasso*N, Ksysid.m:996
      tdst.push_back(Ki);
    }
  }
  if (!tv.empty()) {
    KP_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    rc = kp_lasso_batch_dev(ctx, Gd, Cd, W, W, tv.data(), (int)tv.size(), 20000, 1e-10, tdst.data(), nullptr, nullptr);
    if (rc) return rc;
    KP_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    // the lasso solvers take the same growable page-locked block for their records: a request larger than k_bytes has
    // replaced (and freed) the block k_pin pointed into - take it again (nothing of theirs is live any more)
    if (k_pin) k_pin = (double*)kp_pinned_scratch(ctx, k_bytes);
  }
  if (!conc_done) KP_HIP(ctx, hipEventRecord(ctx->evp[3], ctx->stream));
  // K to the caller: the caller's array is pageable, and a device-to-host copy into pageable memory goes through the
  // runtime's own staging (0.16 ms for the 0.9 MB of one W = 336 matrix); a direct DMA into the context's page-locked
  // block and a memcpy from there take 0.05 ms
  // (a dictionary whose previous fit was rank deficient: the copy of a K that will most likely be replaced waits for the verdict)
  const bool k_late = K_out && ls_index >= 0 && basis->rank_hint > 0 && !conc_done;
  // (the copy engine here, not kp_copy_to_host_async's stores: it runs beside the ratio kernel that follows - 0.815 against 0.823 ms)
  if (K_out && !k_late && !conc_copied) KP_HIP(ctx, hipMemcpyAsync(k_pin ? k_pin : K_out, ctx->Kres, k_bytes, hipMemcpyDeviceToHost, ctx->stream));
  int bad = 0;
  if (conc_done) {
    bad = conc_bad;
    if (!conc_copied) KP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  } else if (ls_index >= 0) {
    rc = kp_read_chol_info(ctx, W, W, &bad, Gd);
    if (rc) return rc;
    if (k_late && !bad) {
      KP_HIP(ctx, hipMemcpyAsync(k_pin ? k_pin : K_out, ctx->Kres, k_bytes, hipMemcpyDeviceToHost, ctx->stream));
      KP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
  } else {
    KP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  collect_gram_timers(ctx, true);
  if (!tv.empty()) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) ctx->timers[3] = ms;
  }
  ctx->last_rank = W;
  if (!bad && ls_index >= 0) basis->rank_hint = 0;
  if (k_pin && (!bad || conc_done)) memcpy(K_out, k_pin, k_bytes);      // (conc_done: whichever K it is, it is final)
  if (bad && conc_done) {
    ctx->last_rank = conc_rank;
    basis->rank_hint = conc_rank < W ? conc_rank : 0;
    ctx->err = "warning: Gram matrix is rank deficient; basic solution returned (kp_fit_last_rank)";
    return KP_OK;
  }
  if (bad) {
    // rank-deficient dictionary (Ksysid.m:1069 on the arm data without dim_red): basic solution + rank, like MATLAB's `\`
    int r = 0;
    double* Kls = ctx->Kres + (size_t)ls_index * W * W;
    rc = kp_pivchol_solve_dev(ctx, Gd, Cd, W, W, Kls, &r, basis->rank_hint);
    if (rc) return rc;
    ctx->last_rank = r;
    basis->rank_hint = r < W ? r : 0;
    for (int i = 0; i < n_lasso; ++i)
      if (i != ls_index && (!lasso || !(lasso[i] < 1e6)))
        KP_HIP(ctx, hipMemcpyAsync(ctx->Kres + (size_t)i * W * W, Kls, (size_t)W * W * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if (K_out) KP_HIP(ctx, hipMemcpyAsync(k_pin ? k_pin : K_out, ctx->Kres, k_bytes, hipMemcpyDeviceToHost, ctx->stream));
    KP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (k_pin) memcpy(K_out, k_pin, k_bytes);
    ctx->err = "warning: Gram matrix is rank deficient; basic solution returned (kp_fit_last_rank)";
  }
  return KP_OK;
}

extern "C" int kp_fit(kp_ctx* ctx, const kp_basis* basis, const kp_snapshots* snaps, const double* lasso, int n_lasso,
                      double* K_out) {
  // (a context whose [G | C] was handed in - kp_multi_fit's peers - needs no snapshot object)
  if (!ctx || !basis || (!snaps && !ctx->gc_preloaded) || n_lasso < 1) return ctx ? ctx->fail(KP_ERR_ARG, "kp_fit: bad argument") : KP_ERR_ARG;
  KP_HIP(ctx, hipSetDevice(ctx->device));
  const int W = basis->dev.W, N = basis->dev.N;
  const bool all_ls = [&] {
    for (int i = 0; i < n_lasso; ++i)
      if (lasso && lasso[i] < 1e6) return false;
    return true;
  }();
  // (wide dictionaries, W > 512, take the synchronous path: a ring of 128 [G | C] pairs of that size would be tens of GB)
  const bool go_async = !K_out && n_lasso == 1 && all_ls && ctx->stream2 && ctx->sticky_info && !ctx->reduce_grams && !ctx->gc_preloaded && W <= 512 && !getenv("KP_NO_ASYNC");
  // The [G | C] ring may hold queued Gram pairs that are not solved yet (deferred, batched solves): drain the pipeline
  // BEFORE any buffer of it can be reallocated for another width - ensure_gc frees and reallocates GC when the new W needs
  // more room - and before a synchronous fit reuses it.  The ring slots and the split-partial buffer are addressed with THIS
  // call's W and partial size, so a change of dictionary or snapshot count drains it as well.
  if (ctx->async_pending && (!go_async || ctx->pend_basis != (const void*)basis || ctx->pend_Ns != snaps->Ns || ctx->pend_W != W)) {
    int rc = kp_synchronize(ctx);
    if (rc) return rc;
  }
  int rc = ensure_gc(ctx, W);
  if (rc) return rc;
  return go_async ? fit_enqueue(ctx, basis, snaps, W) : fit_now(ctx, basis, snaps, lasso, n_lasso, K_out, W, N, all_ls);
}

extern "C" int kp_synchronize(kp_ctx* ctx) {
  if (!ctx) return KP_ERR_ARG;
  KP_HIP(ctx, hipSetDevice(ctx->device));
  {
    int rcf = flush_solves(ctx);
    if (rcf) return rcf;
  }
  KP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->stream2) KP_HIP(ctx, hipStreamSynchronize(ctx->stream2));
  int bad = 0;
  if (ctx->async_pending) {
    collect_gram_timers(ctx, false);
    float ms = 0;
    if (hipEventElapsedTime(&ms, ctx->ev_solve0, ctx->ev_solve1) == hipSuccess) ctx->timers[1] = ms;
    KP_HIP(ctx, hipMemcpy(&bad, ctx->sticky_info, sizeof(int), hipMemcpyDeviceToHost));
    if (bad) KP_HIP(ctx, hipMemset(ctx->sticky_info, 0, sizeof(int)));
  }
  ctx->async_pending = false;
  ctx->batch_closed = true;
  if (bad) return ctx->fail(KP_ERR_NOT_SPD, "kp_synchronize: a deferred fit hit a Gram matrix that is not numerically positive definite");
  return KP_OK;
}

extern "C" int kp_fit_get_K(kp_ctx* ctx, int index, int W, double* K) {
  if (!ctx || !K || index < 0 || W != ctx->Kres_W) return ctx ? ctx->fail(KP_ERR_ARG, "kp_fit_get_K: bad argument") : KP_ERR_ARG;
  KP_HIP(ctx, hipSetDevice(ctx->device));
  {
    int rc = kp_synchronize(ctx);
    if (rc) return rc;
  }
  size_t slot = (size_t)index;
  if (ctx->kres_is_ring) {
    // asynchronous batch: fit number `index` since the previous kp_synchronize; the ring keeps the last kring_cap of them
    if (index >= ctx->async_count || index < ctx->async_count - ctx->kring_cap)
      return ctx->fail(KP_ERR_ARG, "kp_fit_get_K: that fit of the asynchronous batch is not (or no longer) in the result ring "
                                   "(kp_fit_async_slots sets its size)");
    slot = (size_t)(index % ctx->kring_cap);
  } else if (index >= ctx->Kres_n) {
    return ctx->fail(KP_ERR_ARG, "kp_fit_get_K: index out of range");
  }
  KP_HIP(ctx, hipMemcpy(K, ctx->Kres + slot * W * W, (size_t)W * W * 8, hipMemcpyDeviceToHost));
  return KP_OK;
}

extern "C" int kp_fit_async_slots(kp_ctx* ctx, int n_slots) {
  if (!ctx || n_slots < 1 || n_slots > (1 << 20)) return ctx ? ctx->fail(KP_ERR_ARG, "kp_fit_async_slots: bad argument") : KP_ERR_ARG;
  int rc = kp_synchronize(ctx);
  if (rc) return rc;
  ctx->kring_cap = n_slots;
  ctx->kres_is_ring = false;   // whatever the ring held is addressed with the old size: start over
  ctx->Kres_n = 0;
  ctx->async_count = 0;
  return KP_OK;
}

// One fit whose snapshot pairs are sharded over the ranks of the communicator: every rank runs the fused Gram kernel on
// its shard, ONE all-reduce of [G | C] (2 W^2 doubles, device to device over RCCL) is the only exchange, and every
// rank solves the same system (identical K on all ranks).  Without a communicator this is kp_fit.
extern "C" int kp_fit_sharded(kp_ctx* ctx, const kp_basis* basis, const kp_snapshots* snaps_local, const double* lasso, int n_lasso,
                              double* K_out) {
  if (!ctx) return KP_ERR_ARG;
  if (ctx->async_pending) {
    int rc0 = kp_synchronize(ctx);
    if (rc0) return rc0;
  }
  ctx->reduce_grams = true;
  std::vector<double> tmpK;
  double* dst = K_out;
  if (!dst && basis) {            // keep the synchronous path (K_out == NULL selects the asynchronous pipeline otherwise)
    tmpK.resize((size_t)std::max(1, n_lasso) * basis->dev.W * basis->dev.W);
    dst = tmpK.data();
  }
  int rc = kp_fit(ctx, basis, snaps_local, lasso, n_lasso, dst);
  ctx->reduce_grams = false;
  return rc;
}

// the Gram pair alone, summed over the ranks' shards
extern "C" int kp_fit_gram_sharded(kp_ctx* ctx, const kp_basis* basis, const kp_snapshots* snaps_local, double* G, double* C) {
  if (!ctx || !basis || !snaps_local) return ctx ? ctx->fail(KP_ERR_ARG, "kp_fit_gram_sharded: NULL handle") : KP_ERR_ARG;
  int rc = kp_fit_gram(ctx, basis, snaps_local, nullptr, nullptr);
  if (rc) return rc;
  const int W = basis->dev.W;
  rc = kp_comm_allreduce_dev(ctx, ctx->GC, (size_t)2 * W * W, ctx->stream);
  if (rc) return rc;
  size_t bW = (size_t)W * W * 8;
  if (G) KP_HIP(ctx, hipMemcpyAsync(G, ctx->GC, bW, hipMemcpyDeviceToHost, ctx->stream));
  if (C) KP_HIP(ctx, hipMemcpyAsync(C, ctx->GC + (size_t)W * W, bW, hipMemcpyDeviceToHost, ctx->stream));
  KP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return KP_OK;
}
