// Host side of the antenna-array tools, shared by gacq_null.hip, gacq_stap.hip and gacq_beams.hip on top of gacq_streamhost.h: the
// configuration check, the checks of a gacq_*_check, the open handle, gacq_*_open, the front of gacq_*_run_dev and its chunk loop --
// the one place that decides which block covariances a block's weights see.  Host code only; each file includes it after its kernels
// and hands in what really differs: the names in its messages, its blocks per chunk, where the weights begin in the workspace, and
// three callables that fill and launch its own kernels.
#pragma once

#include "gacq_arraycore.h"
#include "gacq_streamhost.h"

#include <cstdio>
#include <type_traits>

namespace {

// One constraint: its 2 M components finite, not all zero.  beam < 0: the cfg's only one.
inline int ar_check_constraint(const char* who, const double* c, int M, int beam) {
  bool any = false;
  for (int i = 0; i < 2 * M; i++) {
    if (!std::isfinite(c[i])) {
      if (beam < 0) return gacq::set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: constraint component %d is not finite", who, i);
      return gacq::set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: beam %d: constraint component %d is not finite", who, beam, i);
    }
    any = any || c[i] != 0.0;
  }
  if (any) return GACQ_OK;
  if (beam < 0) return gacq::set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: the constraint is all zero", who);
  return gacq::set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: beam %d: the constraint is all zero", who, beam);
}

// The fields every array cfg has, refused in the order include/gacq.h promises: the antennas, what `extra` checks (gacq_stap: the taps
// and M T; gacq_beams: the beams), then the block, the window, load_shift and the constraint -- of a cfg whose c has a row per beam,
// those of its `beams` rows.  `who` is the prefix of the messages.
template <class Cfg, class Extra>
int ar_check_cfg(const char* who, int min_antennas, const Cfg* c, Extra extra) {
  if (!c) return gacq::set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: NULL argument", who);
  if (c->antennas < min_antennas || c->antennas > kArMaxM)
    return gacq::set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: %d antennas: need %d..%d", who, c->antennas, min_antennas, kArMaxM);
  if (const int rc = extra(*c); rc < 0) return rc;
  if (c->block < 64 || c->block > kArMaxLb || c->block % 64)
    return gacq::set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: the block length %d is no multiple of 64 in 64..%d", who, c->block, kArMaxLb);
  if (c->window < 1 || c->window > kArMaxWindow)
    return gacq::set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: the window %d lies outside 1..%d", who, c->window, kArMaxWindow);
  if (c->load_shift < 0 || c->load_shift > kArMaxShift)
    return gacq::set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: load_shift %d lies outside 0..%d", who, c->load_shift, kArMaxShift);
  if constexpr (std::is_array_v<std::remove_reference_t<decltype(c->c[0])>>) {
    for (int k = 0; k < c->beams; k++)
      if (const int rc = ar_check_constraint(who, c->c[k], c->antennas, k); rc < 0) return rc;
    return GACQ_OK;
  } else {
    return ar_check_constraint(who, c->c, c->antennas, -1);
  }
}

// A gacq_*_check behind its cfg check, whose result is rc: the gain (with `gains` the `beams` gains of gacq_beams, none of them
// missing), the range, and the support rule of gacq_streamhost.h's blocks and window, stretched by the `reach` samples that taps look
// to either side (none below sample 0)
template <class Cfg>
int ar_check_call(const char* who, int rc, const Cfg* c, long long reach, long long in_first, long long in_count, long long out_first, long long n_out,
                  double gain, const double* gains = nullptr, int beams = 0) {
  if (rc == GACQ_OK && beams && !gains) rc = gacq::set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: NULL argument", who);
  if (rc == GACQ_OK && !beams) rc = st_check_gain(nullptr, who, "is not finite and positive", gain);
  for (int k = 0; rc == GACQ_OK && k < beams; k++) {
    char wording[64];
    snprintf(wording, sizeof wording, "of beam %d is not finite and positive", k);
    rc = st_check_gain(nullptr, who, wording, gains[k]);
  }
  if (rc == GACQ_OK) rc = st_check_range(nullptr, who, in_first, in_count, out_first, n_out);
  if (rc < 0 || n_out == 0) return rc;
  const long long Lb = c->block, W = c->window;
  return st_check_support(nullptr, who, out_first, n_out, std::max(std::max(out_first / Lb - W, 0ll) * Lb - reach, 0ll),
                          std::max(out_first + n_out, W * Lb) - 1 + reach, in_first, in_count);
}

template <class Cfg>
struct ArHandle {
  gacq_ctx* ctx = nullptr;
  Cfg cfg{};
  StDevBlock dev;               // the block covariances of a triple of launches, then the weights of its blocks
};

// gacq_*_open: `check` is the tool's gacq_*_check; `workspace(handle)` finishes the handle and says how many bytes its device block takes
template <class H, class Cfg, class Check, class Workspace>
int ar_open(const char* who, gacq_ctx* ctx, const Cfg* cfg, H** out, Check check, Workspace workspace) {
  if (!ctx) return GACQ_ERR_BAD_ARG;
  if (!out) return gacq::set_error(ctx, GACQ_ERR_BAD_ARG, "%s: NULL argument", who);
  *out = nullptr;
  const int rc = check(cfg, 0, 0, 0, 0, 1.0, 0);
  if (rc < 0) return st_forward(ctx, rc);
  std::unique_ptr<H> h(new H);
  h->ctx = ctx;
  h->cfg = *cfg;
  {
    GACQ_DEVICE(ctx);
    const hipError_t e = h->dev.alloc(ctx, workspace(*h));
    if (e != hipSuccess) return gacq::set_error(ctx, GACQ_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
  }
  *out = h.release();
  return GACQ_OK;
}

// A gacq_*_run_dev: its arguments, then what the chunk loop derives for one triple of launches
struct ArRun {
  const void* const* d_in;
  long long in_first, in_count, out_first, n_out;
  double gain;
  int out_complex64;
  void *d_out, *d_stats, *d_weights, *d_cov;
  int beams;                    // gacq_beams: the outputs d_outs[k] under gains[k], k < beams, for d_out and gain; else 0
  const double* gains;
  void* const* d_outs;
  long long o, o_end, b0, b_hi; // the triple's outputs o .. o_end - 1, which lie in blocks b0 .. b_hi
  long long pb0, ncov;          // the covariances the weights of those blocks need: blocks pb0 .. pb0 + ncov - 1, C[0] is block pb0
  long long own_first;          // the call's first owned block
  int p_off;                    // b0 less pb0
  int warm;                     // blocks b0 + i with i < warm are in the warm-up: their window is C[0 .. W - 1]
  unsigned long long owned;     // blocks that begin in o .. o_end - 1
  float s;                      // the output scale: gain over the weight scale
  float sk[kArMaxBeams];        // ... of beam k
  int *dC, *dWq;                // the workspace: covariances, weights
  unsigned grid;                // workgroups of the apply launch
};

// antenna p's address of absolute sample `at`, for every slot of a kernel's in[] (the slots from M up repeat antenna 0)
inline void ar_inputs(const uint8_t* (&in)[kArMaxM], const ArRun& r, int M, long long at) {
  for (int p = 0; p < kArMaxM; p++) in[p] = (const uint8_t*)r.d_in[p < M ? p : 0] + (at - r.in_first) * 2;
}

// the fields NlWgtArgs, StWgtArgs and BmWgtArgs have in common
template <class Args, class Cfg>
void ar_fill_weights(Args& wg, const Cfg& c, const ArRun& r) {
  wg.C = r.dC;
  wg.Wq = r.dWq;
  wg.cov = (long long*)r.d_cov;
  wg.wout = (int*)r.d_weights;
  if constexpr (!std::is_array_v<std::remove_reference_t<decltype(c.c[0])>>)      // gacq_beams keeps its constraints on the device
    for (int i = 0; i < 2 * kArMaxM; i++) wg.c[i] = i < 2 * c.antennas ? c.c[i] : 0.0;
  wg.b_first = r.b0;
  wg.own_first = r.own_first;
  wg.nblk = (int)(r.b_hi - r.b0 + 1);
  wg.p_off = r.p_off;
  wg.warm = r.warm;
  wg.W = c.window;
  wg.M = c.antennas;
  wg.shift = c.load_shift;
}

// the fields NlApplyArgs and StApplyArgs have in common
template <class Args, class Cfg>
void ar_fill_apply(Args& ap, const Cfg& c, const ArRun& r) {
  ar_inputs(ap.in, r, c.antennas, r.o);
  ap.out = (uint8_t*)r.d_out + (r.o - r.out_first) * (r.out_complex64 ? 8 : 2);
  ap.Wq = r.dWq;
  ap.stats = (unsigned long long*)r.d_stats;
  ap.owned = r.owned;
  ap.s = r.s;
  ap.Lb = c.block;
  ap.M = c.antennas;
}

// gacq_*_run_dev: everything is checked before anything is launched; then, per chunk of `chunk` blocks, the covariances the weights of
// its blocks need, those weights, and the outputs.  dWq lies `wq_at` ints into the handle's workspace.
template <class H, class Check, class Cov, class Wgt, class Apply>
int ar_run_dev(const char* who, H& h, Check check, ArRun r, long long chunk, size_t wq_at, Cov cov, Wgt weights, Apply apply) {
  gacq_ctx* ctx = h.ctx;
  const auto& c = h.cfg;
  if (!r.d_in || (r.beams ? !r.d_outs || !r.gains : !r.d_out)) return gacq::set_error(ctx, GACQ_ERR_BAD_ARG, "%s: NULL argument", who);
  for (int p = 0; p < c.antennas; p++)
    if (!r.d_in[p]) return gacq::set_error(ctx, GACQ_ERR_BAD_ARG, "%s: the pointer of antenna %d is NULL", who, p);
  int rc = check(&c, r.in_first, r.in_count, r.out_first, r.n_out, r.gain, r.out_complex64);
  if (rc < 0) return st_forward(ctx, rc);
  for (int k = 0; k < r.beams; k++)
    if (!r.d_outs[k]) return gacq::set_error(ctx, GACQ_ERR_BAD_ARG, "%s: the pointer of output %d is NULL", who, k);
  for (int k = 0; k < std::max(r.beams, 1); k++)
    if (r.out_complex64 && (uintptr_t)(r.beams ? r.d_outs[k] : r.d_out) % 8u)
      return gacq::set_error(ctx, GACQ_ERR_BAD_ARG, "%s: complex64 output must be 8-byte aligned", who);
  if ((uintptr_t)r.d_stats % 8u) return gacq::set_error(ctx, GACQ_ERR_BAD_ARG, "%s: d_stats must be 8-byte aligned", who);
  if ((uintptr_t)r.d_weights % 4u) return gacq::set_error(ctx, GACQ_ERR_BAD_ARG, "%s: d_weights must be 4-byte aligned", who);
  if ((uintptr_t)r.d_cov % 8u) return gacq::set_error(ctx, GACQ_ERR_BAD_ARG, "%s: d_cov must be 8-byte aligned", who);
  if (r.n_out == 0) return GACQ_OK;
  const long long Lb = c.block, W = c.window, out_end = r.out_first + r.n_out;
  r.own_first = (r.out_first + Lb - 1) / Lb;
  r.s = (float)r.gain * (1.0f / (float)kArWq);
  for (int k = 0; k < r.beams; k++) r.sk[k] = (float)r.gains[k] * (1.0f / (float)kArWq);
  r.dC = (int*)h.dev.p;
  r.dWq = r.dC + wq_at;
  GACQ_DEVICE(ctx);
  for (r.o = r.out_first; r.o < out_end; r.o = r.o_end) {
    r.b0 = r.o / Lb;
    r.o_end = std::min(out_end, (r.b0 + chunk) * Lb);
    r.b_hi = (r.o_end - 1) / Lb;
    r.pb0 = std::max(r.b0 - W, 0ll);
    r.ncov = std::max(r.b_hi, W) - r.pb0;
    r.p_off = (int)(r.b0 - r.pb0);
    r.warm = (int)std::max(W - r.b0, 0ll);
    r.owned = (unsigned long long)((r.o_end + Lb - 1) / Lb - (r.o + Lb - 1) / Lb);
    r.grid = (unsigned)std::min<long long>((r.o_end - 1) / kArTile - r.o / kArTile + 1, (long long)kArMaxGrid);
    cov(r);
    if ((rc = st_launched(ctx, who)) < 0) return rc;
    weights(r);
    if ((rc = st_launched(ctx, who)) < 0) return rc;
    apply(r);
    if ((rc = st_launched(ctx, who)) < 0) return rc;
  }
  return GACQ_OK;
}

}  // namespace
