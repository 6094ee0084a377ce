// The trajectory store of the random-system sweep: the training and validation trials of nb systems resident on the device
// (struct kp_traj, kp_small_tile.h), uploaded once and scaled in place, so that every (model type, degree) call of the sweep
// reads them where they lie.  Device blocks of destroyed objects wait in the context's pool for the next upload.
#include "kp_small_tile.h"
#include <string>

// min / max per column over the training rows of one system -> offset (max+min)/2, factor (max-min)/2 (1 when the range
// is zero), Ksysid.m:187-210
__global__ __launch_bounds__(256) void kp_traj_scale_kernel(const double* __restrict__ Y, const double* __restrict__ U, int rows, int n, int m,
                                                            double* __restrict__ sc) {
  __shared__ double rmin[4], rmax[4];
  const int sys = blockIdx.x, tid = threadIdx.x;
  double* out = sc + (size_t)sys * 2 * (n + m);
  for (int v = 0; v < n + m; ++v) {
    const double* col = v < n ? Y + ((size_t)sys * n + v) * rows : U + ((size_t)sys * m + (v - n)) * rows;
    double lo = 1e300, hi = -1e300;
    for (int r = tid; r < rows; r += 256) { const double x = col[r]; lo = fmin(lo, x); hi = fmax(hi, x); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo = fmin(lo, __shfl_xor(lo, o, 64)); hi = fmax(hi, __shfl_xor(hi, o, 64)); }
    __syncthreads();
    if ((tid & 63) == 0) { rmin[tid >> 6] = lo; rmax[tid >> 6] = hi; }
    __syncthreads();
    if (tid == 0) {
      lo = fmin(fmin(rmin[0], rmin[1]), fmin(rmin[2], rmin[3]));
      hi = fmax(fmax(rmax[0], rmax[1]), fmax(rmax[2], rmax[3]));
      const double off = (hi + lo) / 2.0, fac = (hi - lo) / 2.0;
      if (v < n) { out[v] = off; out[n + v] = fac == 0.0 ? 1.0 : fac; }
      else { out[2 * n + (v - n)] = off; out[2 * n + m + (v - n)] = fac == 0.0 ? 1.0 : fac; }
    }
  }
}

// scale_data (Ksysid.m:308-343) once, in place: training and validation trials with the training factors
__global__ void kp_traj_apply_scale_kernel(double* __restrict__ X, int rows, int width, int n, int m, int is_u, const double* __restrict__ sc) {
  const int sys = blockIdx.y;
  const double* s = sc + (size_t)sys * 2 * (n + m);
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < rows * width; e += gridDim.x * blockDim.x) {
    const int v = e / rows;
    const double off = is_u ? s[2 * n + v] : s[v], fac = is_u ? s[2 * n + m + v] : s[n + v];
    double* x = X + (size_t)sys * rows * width + e;
    *x = (*x - off) / fac;
  }
}

#define KP_TRAJ_POOL_MAX 10
static bool traj_no_pool() {
  static const bool no_pool = getenv("KP_NO_TRAJ_POOL") != nullptr;
  return no_pool;
}
// a block of at least `bytes` (and at most twice that) from the context's pool, else a new one; cap = its real size
static hipError_t traj_alloc(kp_ctx* ctx, double** p, size_t bytes, size_t* cap) {
  if (!traj_no_pool()) {
    std::lock_guard<std::mutex> lk(ctx->host_mu);     // the pool is shared with a host thread that builds the next object
    int best = -1;
    for (size_t i = 0; i < ctx->traj_pool.size(); ++i) {
      const size_t c = ctx->traj_pool[i].second;
      if (c >= bytes && c <= 2 * bytes + 4096 && (best < 0 || c < ctx->traj_pool[best].second)) best = (int)i;
    }
    if (best >= 0) {
      *p = (double*)ctx->traj_pool[best].first;
      *cap = ctx->traj_pool[best].second;
      ctx->traj_pool.erase(ctx->traj_pool.begin() + best);
      return hipSuccess;
    }
  }
  *cap = bytes;
  return hipMalloc((void**)p, bytes);
}
static void traj_release(kp_ctx* ctx, void* p, size_t cap) {
  if (!p) return;
  if (traj_no_pool() || !ctx) { (void)hipFree(p); return; }
  std::lock_guard<std::mutex> lk(ctx->host_mu);
  ctx->traj_pool.push_back({p, cap});
  while (ctx->traj_pool.size() > KP_TRAJ_POOL_MAX) {       // the oldest goes
    (void)hipFree(ctx->traj_pool.front().first);
    ctx->traj_pool.erase(ctx->traj_pool.begin());
  }
}
void kp_traj_pool_free(kp_ctx* ctx) {
  std::lock_guard<std::mutex> lk(ctx->host_mu);
  for (auto& b : ctx->traj_pool) (void)hipFree(b.first);
  ctx->traj_pool.clear();
}

// The object in three steps, so that a caller that assembles the four blocks one after the other (the host mirror gathers
// them from thousands of small trial arrays) has each one on its way to the device while it prepares the next:
//   kp_traj_create (device blocks), kp_traj_put (which = 0 Y, 1 U, 2 Yv, 3 Uv: ONE host-to-device copy enqueued on the
//   context's stream - asynchronous when `host` is page-locked, e.g. a kp_host_alloc block, which must then stay untouched
//   until kp_traj_finish), kp_traj_finish (scaling on the device, stream synchronised: the object is ready).
extern "C" int kp_traj_create(kp_ctx* ctx, int nb, int ntrials, int T, int n, int m, int Tv, kp_traj** out) {
  if (!ctx || !out || nb < 1 || ntrials < 1 || T < 3 || n < 1 || m < 1 || Tv < 2 || (int64_t)ntrials * T >= (1 << 24))
    return ctx ? ctx->fail(KP_ERR_ARG, "kp_traj_upload: bad argument") : KP_ERR_ARG;
  KP_HIP(ctx, hipSetDevice(ctx->device));
  kp_traj* t = new kp_traj;
  t->ctx = ctx; t->nb = nb; t->ntrials = ntrials; t->T = T; t->n = n; t->m = m; t->Tv = Tv;
  const size_t rows = (size_t)ntrials * T;
  const size_t bY = (size_t)nb * rows * n * 8, bU = (size_t)nb * rows * m * 8, bYv = (size_t)nb * Tv * n * 8, bUv = (size_t)nb * Tv * m * 8;
  hipError_t e = traj_alloc(ctx, &t->Y, bY, &t->cap[0]);
  if (e == hipSuccess) e = traj_alloc(ctx, &t->U, bU, &t->cap[1]);
  if (e == hipSuccess) e = traj_alloc(ctx, &t->Yv, bYv, &t->cap[2]);
  if (e == hipSuccess) e = traj_alloc(ctx, &t->Uv, bUv, &t->cap[3]);
  if (e == hipSuccess) e = traj_alloc(ctx, &t->sc, (size_t)nb * 2 * (n + m) * 8, &t->cap[4]);
  if (e != hipSuccess) {
    double* bufs[] = {t->Y, t->U, t->Yv, t->Uv, t->sc};
    for (double* p : bufs)
      if (p) (void)hipFree(p);
    delete t;
    return ctx->fail(KP_ERR_HIP, std::string("kp_traj_upload: ") + hipGetErrorString(e));
  }
  *out = t;
  return KP_OK;
}

// Internal (not in the C ABI): the four device blocks of a new object (0 Y, 1 U, 2 Yv, 3 Uv; layouts as kp_traj_upload),
// marked as put.  A device producer (kp_rsys.hip) fills them on the context's stream and then calls kp_traj_finish.
void kp_traj_device_blocks(kp_traj* t, double** blocks) {
  blocks[0] = t->Y; blocks[1] = t->U; blocks[2] = t->Yv; blocks[3] = t->Uv;
  t->have = 15;
}

extern "C" int kp_traj_put(kp_traj* t, int which, const double* host) {
  if (!t || !host || which < 0 || which > 3) return t ? t->ctx->fail(KP_ERR_ARG, "kp_traj_put: bad argument") : KP_ERR_ARG;
  kp_ctx* ctx = t->ctx;
  // a finished object holds SCALED data: a raw block put behind kp_traj_finish would never be rescaled (finish is a no-op
  // then) and the sweep would run on a mix of scaled and raw values
  if (t->have == 31) return ctx->fail(KP_ERR_ARG, "kp_traj_put: the object is finished (scaled); create a new one");
  KP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t rows = (size_t)t->ntrials * t->T;
  double* dst[4] = {t->Y, t->U, t->Yv, t->Uv};
  const size_t bytes[4] = {(size_t)t->nb * rows * t->n * 8, (size_t)t->nb * rows * t->m * 8, (size_t)t->nb * t->Tv * t->n * 8,
                           (size_t)t->nb * t->Tv * t->m * 8};
  KP_HIP(ctx, hipMemcpyAsync(dst[which], host, bytes[which], hipMemcpyHostToDevice, ctx->stream));
  t->have |= 1 << which;
  return KP_OK;
}

extern "C" int kp_traj_finish(kp_traj* t) {
  if (!t) return KP_ERR_ARG;
  kp_ctx* ctx = t->ctx;
  if (t->have == 31) return KP_OK;
  if (t->have != 15) return ctx->fail(KP_ERR_ARG, "kp_traj_finish: a block is missing (kp_traj_put of Y, U, Yv, Uv)");
  KP_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int nb = t->nb, n = t->n, m = t->m, Tv = t->Tv;
  const size_t rows = (size_t)t->ntrials * t->T;
  hipLaunchKernelGGL(kp_traj_scale_kernel, dim3(nb), dim3(256), 0, s, t->Y, t->U, (int)rows, n, m, t->sc);
  hipLaunchKernelGGL(kp_traj_apply_scale_kernel, dim3(16, nb), dim3(256), 0, s, t->Y, (int)rows, n, n, m, 0, t->sc);
  hipLaunchKernelGGL(kp_traj_apply_scale_kernel, dim3(16, nb), dim3(256), 0, s, t->U, (int)rows, m, n, m, 1, t->sc);
  hipLaunchKernelGGL(kp_traj_apply_scale_kernel, dim3(2, nb), dim3(256), 0, s, t->Yv, Tv, n, n, m, 0, t->sc);
  hipLaunchKernelGGL(kp_traj_apply_scale_kernel, dim3(2, nb), dim3(256), 0, s, t->Uv, Tv, m, n, m, 1, t->sc);
  KP_HIP(ctx, hipGetLastError());
  KP_HIP(ctx, hipStreamSynchronize(s));
  t->have = 31;                                       // scaled: a second finish would scale again
  return KP_OK;
}

extern "C" int kp_traj_upload(kp_ctx* ctx, const double* Y, const double* U, int nb, int ntrials, int T, int n, int m, const double* Yv,
                              const double* Uv, int Tv, kp_traj** out) {
  if (!ctx || !Y || !U || !Yv || !Uv || !out) return ctx ? ctx->fail(KP_ERR_ARG, "kp_traj_upload: bad argument") : KP_ERR_ARG;
  kp_traj* t = nullptr;
  int rc = kp_traj_create(ctx, nb, ntrials, T, n, m, Tv, &t);
  if (rc) return rc;
  const double* src[4] = {Y, U, Yv, Uv};
  for (int w = 0; w < 4 && rc == KP_OK; ++w) rc = kp_traj_put(t, w, src[w]);
  if (rc == KP_OK) rc = kp_traj_finish(t);
  if (rc) {
    (void)hipStreamSynchronize(ctx->stream);
    double* bufs[] = {t->Y, t->U, t->Yv, t->Uv, t->sc};
    for (double* p : bufs)
      if (p) (void)hipFree(p);
    delete t;
    return rc;
  }
  *out = t;
  return KP_OK;
}

extern "C" int kp_traj_destroy(kp_traj* t) {
  if (!t) return KP_OK;
  double* bufs[] = {t->Y, t->U, t->Yv, t->Uv, t->sc};
  // the blocks go back to the context's pool - once the device is done with them (every entry point that used them has
  // synchronised its stream before returning; an object abandoned between kp_traj_put and kp_traj_finish may still have
  // copies in flight)
  if (t->have != 0 && t->have != 31 && t->ctx) {
    (void)hipSetDevice(t->ctx->device);
    (void)hipStreamSynchronize(t->ctx->stream);
  }
  for (int i = 0; i < 5; ++i) traj_release(t->ctx, bufs[i], t->cap[i]);
  delete t;
  return KP_OK;
}

extern "C" int kp_traj_dims(const kp_traj* t, int* nb, int* ntrials, int* T, int* n, int* m, int* Tv) {
  if (!t) return KP_ERR_ARG;
  if (nb) *nb = t->nb;
  if (ntrials) *ntrials = t->ntrials;
  if (T) *T = t->T;
  if (n) *n = t->n;
  if (m) *m = t->m;
  if (Tv) *Tv = t->Tv;
  return KP_OK;
}

extern "C" int kp_traj_scale(kp_traj* t, double* sc_out) {
  if (!t || !sc_out) return KP_ERR_ARG;
  kp_ctx* ctx = t->ctx;
  if (t->have != 31) return ctx->fail(KP_ERR_ARG, "kp_traj_scale: trajectory object not finished (kp_traj_finish)");
  KP_HIP(ctx, hipMemcpy(sc_out, t->sc, (size_t)t->nb * 2 * (t->n + t->m) * 8, hipMemcpyDeviceToHost));
  return KP_OK;
}
