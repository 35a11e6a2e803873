// Host side of the tracking handles, shared by gacq_trackloop.hip, gacq_longtrack.hip and gacq_chiptrack.hip: the checks of the
// K channel specs, the code-boundary alignment, the uploads, the bookkeeping around a launch, state and close.  Host code only.
// Each file includes it after its kernels, defines its own handle type on TlHandle and keeps the one hipLaunchKernelGGL of its
// own kernel, which it hands to tl_run as a callable.  What the three entry points check differently is in TlLimits.
#pragma once

#include "gacq_trackcore.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <vector>

namespace {

struct TlHandle {
  gacq_ctx* ctx = nullptr;
  int K = 0;
  int subs_max = 1;
  gacq::DevBuf d_specs, d_runs, d_states, d_recs;
  const double2* d_tab = nullptr;
};

struct TlLimits {
  const char* who;                  // the entry point's name, for the messages
  unsigned kinds;                   // bit k set: correlator kind k is accepted
  int max_subs;
  int max_chips;                    // 0: codes of any length
  double max_spacing;               // spacing must lie below it (HUGE_VAL: any)
  bool lazy_chips;                  // generate a chip table only when the context's cache lacks it (chip_table_host)
};

struct TlPrep {                     // what tl_prepare hands to tl_upload
  std::vector<TlSpec> specs;
  std::vector<gacq_track_chstate> init;
  std::vector<gacq::ChipTable> tabs;
  int subs_max = 1;
};

// Checks the K specs in order, each against `lim`, and fills the device form of the specs (all but the chip pointers) and the state
// every channel starts from.  Touches no device.
inline int tl_prepare(gacq_ctx* ctx, const TlLimits& lim, const gacq_track_spec* specs, int K, TlPrep& p) {
  using gacq::set_error;
  const char* who = lim.who;
  p.specs.resize(K);
  p.init.resize(K);
  p.tabs.resize(K);
  for (int k = 0; k < K; k++) {
    const gacq_track_spec& s = specs[k];
    if (!s.code) return set_error(ctx, GACQ_ERR_BAD_ARG, "%s: channel %d has no code", who, k);
    const int L = gacq_code_length(s.code);
    if (L < 0) return set_error(ctx, GACQ_ERR_UNKNOWN_CODE, "%s: channel %d: unknown code '%s'", who, k, s.code);
    if (lim.max_chips && L > lim.max_chips)
      return set_error(ctx, GACQ_ERR_UNSUPPORTED, "%s: channel %d: code '%s' is longer than %d chips", who, k, s.code, lim.max_chips);
    const bool fin = std::isfinite(s.fs) && std::isfinite(s.period) && std::isfinite(s.rate) && std::isfinite(s.ratio) &&
                     std::isfinite(s.spacing) && std::isfinite(s.coffset) && std::isfinite(s.fm) && std::isfinite(s.code_offset) &&
                     std::isfinite(s.doppler) && std::isfinite(s.carrier_phase) && std::isfinite(s.chip_rate);
    if (!fin || !(s.fs > 0.0)) return set_error(ctx, GACQ_ERR_BAD_ARG, "%s: channel %d: bad sample rate or parameter", who, k);
    if (!(s.code_offset >= 0.0 && s.code_offset < (double)L))
      return set_error(ctx, GACQ_ERR_BAD_ARG, "%s: channel %d: code offset %g outside [0, %d)", who, k, s.code_offset, L);
    if (s.kind < 0 || s.kind > 31 || !((lim.kinds >> s.kind) & 1u) || s.subs < 1 || s.subs > lim.max_subs || !(s.period > 0.0) ||
        !(s.rate > 0.0) || s.ratio == 0.0 || !(s.spacing >= 0.0) || !(s.spacing < lim.max_spacing))
      return set_error(ctx, GACQ_ERR_BAD_ARG, "%s: channel %d: bad tracker parameters", who, k);
    const double fo = s.glonass ? s.fm : -s.coffset / s.fs;
    if (!(std::fabs(fo) < 7.0) || !(std::fabs(s.carrier_phase) < 7.0) || !(std::fabs(s.doppler / s.fs) < 7.0))
      return set_error(ctx, GACQ_ERR_BAD_ARG, "%s: channel %d: NCO frequency or phase out of range", who, k);
    // one table per code and PRN: a channel that repeats an earlier one's finds it in the cache once that one is uploaded
    int first = 0;
    while (first < k && (specs[first].prn != s.prn || std::strcmp(specs[first].code, s.code))) first++;
    if (first < k) {
      p.tabs[k].key = p.tabs[first].key;
    } else {
      const int rc = gacq::chip_table_host(ctx, s.code, s.prn, L, lim.lazy_chips, p.tabs[k]);
      if (rc < 0) return set_error(ctx, rc, "%s: channel %d: no PRN %d in '%s'", who, k, s.prn, s.code);
    }
    TlSpec& t = p.specs[k];
    t.chips = nullptr;
    t.L = L; t.kind = s.kind; t.subs = s.subs; t.fixed_pll = s.fixed_pll ? 1 : 0; t.glonass = s.glonass ? 1 : 0; t.pad = 0;
    t.fs = s.fs; t.period = s.period; t.ratio = s.ratio; t.spacing = s.spacing;
    t.fll_k_wide = s.fll_k_wide; t.fll_k_narrow = s.fll_k_narrow; t.pll_k1 = s.pll_k1; t.pll_k2 = s.pll_k2; t.dll_k1 = s.dll_k1; t.dll_k2 = s.dll_k2;
    t.coffset = s.coffset; t.fm = s.fm;
    t.dfo = (long long)std::floor(fo * kTwo60);
    t.dwell_wide = s.dwell_wide; t.dwell_narrow = s.dwell_narrow;
    // alignment with the code boundary (track-gps-l1.py:141-143, track-gps-l2cl.py:133-136), on the host:
    // n = int(fs*period*((L-code_offset)/L)), code_offset += n*rate*L/fs
    const long long n0 = (long long)(s.fs * s.period * (((double)L - s.code_offset) / (double)L));
    gacq_track_chstate& g = p.init[k];
    std::memset(&g, 0, sizeof(g));
    g.code_p = s.code_offset + n0 * s.rate * (double)L / s.fs;
    g.code_f = s.chip_rate;
    g.carrier_p = s.carrier_phase;
    g.carrier_f = s.doppler;
    g.mode = s.fixed_pll ? kModePll : kModeFllWide;
    g.pos = n0;
    p.subs_max = std::max(p.subs_max, s.subs);
  }
  return GACQ_OK;
}

// Chip tables and NCO table into the context's cache, the handle's buffers, specs and initial states onto the device
inline int tl_upload(gacq_ctx* ctx, const char* who, TlPrep& p, TlHandle* h) {
  using gacq::ensure;
  const int K = (int)p.specs.size();
  h->ctx = ctx;
  h->K = K;
  h->subs_max = p.subs_max;
  int rc = GACQ_OK;
  for (int k = 0; k < K && rc == GACQ_OK; k++) rc = gacq::chip_table_dev(ctx, p.tabs[k], &p.specs[k].chips);
  if (rc == GACQ_OK) rc = nco_table(ctx, &h->d_tab);
  if (rc == GACQ_OK) rc = ensure(ctx, h->d_specs, sizeof(TlSpec) * K);
  if (rc == GACQ_OK) rc = ensure(ctx, h->d_runs, sizeof(TlRun) * K);
  if (rc == GACQ_OK) rc = ensure(ctx, h->d_states, sizeof(gacq_track_chstate) * K);
  if (rc == GACQ_OK && hipMemcpy(h->d_specs.p, p.specs.data(), sizeof(TlSpec) * K, hipMemcpyHostToDevice) != hipSuccess)
    rc = gacq::set_error(ctx, GACQ_ERR_HIP, "%s: upload failed", who);
  if (rc == GACQ_OK && hipMemcpy(h->d_states.p, p.init.data(), sizeof(gacq_track_chstate) * K, hipMemcpyHostToDevice) != hipSuccess)
    rc = gacq::set_error(ctx, GACQ_ERR_HIP, "%s: upload failed", who);
  return rc;
}

template <class H>
void tl_close(H* h, std::initializer_list<gacq::DevBuf*> more = {}) {
  if (!h) return;
  {
    gacq::DeviceGuard g(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    for (gacq::DevBuf* b : {&h->d_specs, &h->d_runs, &h->d_states, &h->d_recs})
      if (b->p) (void)hipFree(b->p);
    for (gacq::DevBuf* b : more)
      if (b->p) (void)hipFree(b->p);
  }
  delete h;
}

// gacq_track_open and gacq_longtrack_open whole; gacq_chiptrack_open has checks and buffers of its own around the same steps
template <class H>
int tl_open(gacq_ctx* ctx, const TlLimits& lim, const gacq_track_spec* specs, int K, H** out) {
  if (!ctx || !out) return gacq::set_error(ctx, GACQ_ERR_BAD_ARG, "%s: NULL argument", lim.who);
  *out = nullptr;
  if (!specs || K <= 0) return gacq::set_error(ctx, GACQ_ERR_BAD_ARG, "%s: need at least one channel (K = %d)", lim.who, K);
  TlPrep p;
  int rc = tl_prepare(ctx, lim, specs, K, p);
  if (rc != GACQ_OK) return rc;
  GACQ_DEVICE(ctx);
  H* h = new H();
  if ((rc = tl_upload(ctx, lim.who, p, h)) != GACQ_OK) {
    tl_close(h);
    return rc;
  }
  *out = h;
  return GACQ_OK;
}

// One launch: the K sample windows are checked against where each channel stands, `launch(stream)` starts the file's kernel, and
// states and records come back.  written_only: copy back only the records each channel wrote, after a synchronisation of its own
// (long-code handles hold thousands of records per channel); otherwise the whole K x rec_cap block in the same one.
template <class Launch>
int tl_run(TlHandle* h, const char* who, bool written_only, const void* const* d_x, const long long* base, const long long* avail,
           int max_records, gacq_track_record* recs, int rec_cap, int* counts, int* status, Launch launch) {
  using gacq::set_error;
  if (!h) return GACQ_ERR_BAD_ARG;
  gacq_ctx* ctx = h->ctx;
  if (!d_x || !base || !avail || !recs || !counts || !status || max_records < h->subs_max || rec_cap < max_records)
    return set_error(ctx, GACQ_ERR_BAD_ARG, "%s: bad argument (need %d <= max_records <= rec_cap)", who, h->subs_max);
  const int K = h->K;
  std::vector<gacq_track_chstate> now(K);
  GACQ_DEVICE(ctx);
  hipStream_t stream = ctx->stream;
  GACQ_HIP(ctx, hipMemcpyAsync(now.data(), h->d_states.p, sizeof(gacq_track_chstate) * K, hipMemcpyDeviceToHost, stream));
  GACQ_HIP(ctx, hipStreamSynchronize(stream));
  std::vector<TlRun> runs(K);
  for (int k = 0; k < K; k++) {
    if (!d_x[k] || base[k] < 0 || avail[k] < 0) return set_error(ctx, GACQ_ERR_BAD_ARG, "%s: channel %d: bad samples", who, k);
    // the samples handed over must start at or before the channel's next block
    if (base[k] > now[k].pos)
      return set_error(ctx, GACQ_ERR_BAD_ARG, "%s: channel %d: samples start at %lld, the next block at %lld", who, k, base[k],
                       now[k].pos);
    runs[k].x = (const int8_t*)d_x[k];
    runs[k].base = base[k];
    runs[k].end = base[k] + avail[k];
  }
  int rc;
  if ((rc = gacq::ensure(ctx, h->d_recs, sizeof(gacq_track_record) * (size_t)K * rec_cap)) != GACQ_OK) return rc;
  GACQ_HIP(ctx, hipMemcpyAsync(h->d_runs.p, runs.data(), sizeof(TlRun) * K, hipMemcpyHostToDevice, stream));
  launch(stream);
  GACQ_HIP(ctx, hipGetLastError());
  GACQ_HIP(ctx, hipMemcpyAsync(now.data(), h->d_states.p, sizeof(gacq_track_chstate) * K, hipMemcpyDeviceToHost, stream));
  if (written_only) GACQ_HIP(ctx, hipStreamSynchronize(stream));
  else GACQ_HIP(ctx, hipMemcpyAsync(recs, h->d_recs.p, sizeof(gacq_track_record) * (size_t)K * rec_cap, hipMemcpyDeviceToHost, stream));
  for (int k = 0; k < K; k++) {
    status[k] = now[k].status;
    counts[k] = now[k].last_records;
    if (written_only && counts[k] > 0)      // a channel's count is in its state
      GACQ_HIP(ctx, hipMemcpyAsync(recs + (size_t)k * rec_cap, (const gacq_track_record*)h->d_recs.p + (size_t)k * rec_cap,
                                   sizeof(gacq_track_record) * (size_t)counts[k], hipMemcpyDeviceToHost, stream));
  }
  GACQ_HIP(ctx, hipStreamSynchronize(stream));
  return GACQ_OK;
}

inline int tl_state(TlHandle* h, const char* who, int k, gacq_track_chstate* out) {
  if (!h) return GACQ_ERR_BAD_ARG;
  gacq_ctx* ctx = h->ctx;
  if (!out || k < 0 || k >= h->K) return gacq::set_error(ctx, GACQ_ERR_BAD_ARG, "%s: bad channel %d", who, k);
  GACQ_DEVICE(ctx);
  GACQ_HIP(ctx, hipMemcpyAsync(out, (const gacq_track_chstate*)h->d_states.p + k, sizeof(gacq_track_chstate), hipMemcpyDeviceToHost, ctx->stream));
  GACQ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return GACQ_OK;
}

}  // namespace
