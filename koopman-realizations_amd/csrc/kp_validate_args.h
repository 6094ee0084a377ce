// The argument checks that kp_validate (kp_validate.hip), kp_validate_ct (kp_validate_ct.hip) and kp_validate_horizon
// (kp_validate_horizon.hip) share.
#pragma once
#include <string>

#include "kp_internal.h"

// The argument checks of kp_validate and kp_validate_ct (`fn`), ctx not null: KP_OK or the refusal.
inline int val_check_args(kp_ctx* ctx, const std::string& fn, const kp_basis* basis, int model_type, int N, int m, int n, int nzeta,
                          int nw, int nmod, const double* A, const double* B, int ntr, const int64_t* trial_off, const double* zeta0,
                          const double* U, const double* Yreal, const double* yfactor, int want_sim, const double* err_out,
                          const int* status_out, const double* Ysim) {
  if (!basis || !A || !trial_off || !zeta0 || !Yreal || !yfactor || !err_out || !status_out || nmod < 1 || ntr < 1 || N < 1 || m < 0 ||
      n < 1 || nzeta < 1 || nw < 0)
    return ctx->fail(KP_ERR_ARG, fn + ": bad argument");
  if (model_type != KP_MODEL_LINEAR && model_type != KP_MODEL_BILINEAR && model_type != KP_MODEL_NONLINEAR)
    return ctx->fail(KP_ERR_ARG, fn + ": unknown model type");
  const bool nl = model_type == KP_MODEL_NONLINEAR;
  const BasisDev& b = basis->dev;
  if (b.model_type != model_type)
    return ctx->fail(KP_ERR_ARG, fn + ": the dictionary is of model type " + std::to_string(b.model_type) + ", the models of type " +
                                     std::to_string(model_type));
  if (b.N != N || b.m != m || b.nzeta != nzeta)
    return ctx->fail(KP_ERR_ARG, fn + ": N, m and nzeta must be those of the dictionary (" + std::to_string(b.N) + ", " +
                                     std::to_string(b.m) + ", " + std::to_string(b.nzeta) + ")");
  if (n > N || (nl && n > nzeta))
    return ctx->fail(KP_ERR_ARG, fn + ": n = " + std::to_string(n) + " outputs, but the state has " + std::to_string(nl ? nzeta : N) +
                                     " entries");
  if (!nl && !B) return ctx->fail(KP_ERR_ARG, fn + ": B required");
  if (m > 0 && !U) return ctx->fail(KP_ERR_ARG, fn + ": U required");
  if (want_sim && !Ysim) return ctx->fail(KP_ERR_ARG, fn + ": Ysim required with want_sim");
  if (trial_off[0] != 0) return ctx->fail(KP_ERR_ARG, fn + ": trial_off must start at 0");
  for (int q = 0; q < ntr; ++q) {
    const int64_t Tq = trial_off[q + 1] - trial_off[q];
    if (Tq < 1) return ctx->fail(KP_ERR_ARG, fn + ": trial " + std::to_string(q) + " is empty");
    if (Tq > INT32_MAX) return ctx->fail(KP_ERR_ARG, fn + ": trial " + std::to_string(q) + " is too long");
  }
  if ((int64_t)nmod * ntr > INT32_MAX) return ctx->fail(KP_ERR_ARG, fn + ": too many (model, trial) pairs");
  return KP_OK;
}

// What kp_validate_horizon (kp_validate_horizon.hip) checks beyond val_check_args, which it calls with its Zeta as zeta0 and
// Yreal: the real outputs are the first n columns of Zeta.
inline int val_check_horizon_args(kp_ctx* ctx, const std::string& fn, int n, int nzeta, int H, int stride, const int64_t* nstart_out) {
  if (!nstart_out) return ctx->fail(KP_ERR_ARG, fn + ": bad argument");
  if (H < 1 || stride < 1)
    return ctx->fail(KP_ERR_ARG, fn + ": the horizon H = " + std::to_string(H) + " and the stride = " + std::to_string(stride) +
                                     " must be at least 1");
  if (n > nzeta)
    return ctx->fail(KP_ERR_ARG, fn + ": n = " + std::to_string(n) + " outputs, but Zeta has " + std::to_string(nzeta) + " columns");
  return KP_OK;
}
