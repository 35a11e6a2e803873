// Host side of the recording converters, shared by gacq_ingest.hip, gacq_mitigate.hip, gacq_ddc.hip, gacq_requant.hip, gacq_cancel.hip
// and gacq_aprompt.hip (these two through gacq_cancelcore.h), gacq_null.hip and gacq_stap.hip (through gacq_arrayhost.h): the checks
// every "absolute sample index in, absolute sample index out" entry point makes in the same words, the status of a launch, and the
// device block of an open handle.  Host code only.  `who` is the entry point's name as its messages carry it; `ctx` is the context
// the message goes to, nullptr from a gacq_*_check.
#pragma once

#include "gacq_common.h"

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <memory>

namespace {

constexpr long long kStreamMaxIndex = 1ll << 48;

inline int st_check_range(gacq_ctx* ctx, const char* who, long long in_first, long long in_count, long long out_first, long long n_out) {
  for (long long v : {in_first, in_count, out_first, n_out})
    if (v < 0 || v > kStreamMaxIndex)
      return gacq::set_error(ctx, GACQ_ERR_BAD_ARG, "%s: need 0 <= in_first, in_count, out_first, n_out <= 2^48 (%lld, %lld, %lld, %lld)", who, in_first,
                             in_count, out_first, n_out);
  return GACQ_OK;
}

// the gain as a double and as the float the kernels multiply with; `wording` is the caller's own ("must be ..", "is not ..")
inline int st_check_gain(gacq_ctx* ctx, const char* who, const char* wording, double gain) {
  const float g = (float)gain;
  if (!std::isfinite(gain) || !(gain > 0.0) || !std::isfinite(g) || !(g > 0.0f))
    return gacq::set_error(ctx, GACQ_ERR_BAD_ARG, "%s: the gain %s (%g)", who, wording, gain);
  return GACQ_OK;
}

// the support rule: outputs out_first .. out_first + n_out - 1 (n_out > 0) need inputs need_lo .. need_hi, all of them present
inline int st_check_support(gacq_ctx* ctx, const char* who, long long out_first, long long n_out, long long need_lo, long long need_hi,
                            long long in_first, long long in_count) {
  if (need_lo < in_first || need_hi >= in_first + in_count)
    return gacq::set_error(ctx, GACQ_ERR_SHORT_INPUT, "%s: outputs %lld .. %lld need input samples %lld .. %lld, present are %lld .. %lld", who, out_first,
                           out_first + n_out - 1, need_lo, need_hi, in_first, in_first + in_count - 1);
  return GACQ_OK;
}

// ... where output j of block b = j div Lb needs j itself and blocks max(b - W, 0) .. max(b, W) - 1 whole
inline int st_check_block_support(gacq_ctx* ctx, const char* who, long long Lb, long long W, long long out_first, long long n_out, long long in_first,
                                  long long in_count) {
  return st_check_support(ctx, who, out_first, n_out, std::max(out_first / Lb - W, 0ll) * Lb, std::max(out_first + n_out, W * Lb) - 1, in_first, in_count);
}

// the refusal of a gacq_*_check, which has no context, onto the context of the call that made it
inline int st_forward(gacq_ctx* ctx, int rc) { return gacq::set_error(ctx, rc, "%s", gacq_last_error(nullptr)); }

inline int st_launched(gacq_ctx* ctx, const char* who) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? GACQ_OK : gacq::set_error(ctx, GACQ_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(e));
}

// The device block of an open handle.  alloc and upload run under the caller's GACQ_DEVICE; an upload is a blocking copy from pageable
// memory, which has landed when it returns.  Freed with the handle, on its device; a block that was never allocated frees nothing.
struct StDevBlock {
  void* p = nullptr;
  int device = 0;
  StDevBlock() = default;
  StDevBlock(const StDevBlock&) = delete;
  StDevBlock& operator=(const StDevBlock&) = delete;
  ~StDevBlock() {
    if (!p) return;
    gacq::DeviceGuard guard(device);
    (void)hipFree(p);
  }
  hipError_t alloc(gacq_ctx* ctx, size_t bytes) {
    device = ctx->device;
    return hipMalloc(&p, bytes);
  }
  hipError_t upload(size_t at, const void* src, size_t bytes) { return hipMemcpy((char*)p + at, src, bytes, hipMemcpyHostToDevice); }
};

}  // namespace
