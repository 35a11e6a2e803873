// The replica of a tracked signal and its segment table, shared by gacq_cancel.hip (project, subtract) and gacq_aprompt.hip (the
// projection of M antennas at once): the device form of a satellite and of a segment, the sample's carrier and chip
//   theta(j) = (p0 + i F) mod 2^64,  pos(j) = c0 + i Cf,  i = j - s0,   r(j) = w(pos(j)) exp(2 pi i theta(j) / 2^64)
// and, on the host, the checks of the gacq_cancel_sat / gacq_cancel_seg arrays, their conversion to fixed point, the chip-table lookup
// and the upload.  One definition of each: what the two files compute for a sample is the same instruction sequence on the same table.
// The sine / cosine (turn_sincos), the conversions to 2^-64 fixed point (turn_fraction, turn_fixed) and the TMBOC mask are
// gacq_turn.h's, the very routines of gacq_simcore.h: that is what makes the cancellation of a simulated signal exact.
// A file includes it under `#pragma clang fp contract(off)`: w cos and w sin are products rounded on their own.
// `who` is the entry point's name as its messages carry it.
#pragma once

#include "gacq_common.h"
#include "gacq_streamhost.h"
#include "gacq_turn.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

constexpr int kCanBlock = 256;
constexpr int kCanMaxK = 32;
constexpr int kCanMaxSegs = 1 << 20;
constexpr long long kCanMaxN = 1ll << 24;
constexpr int kCanMaxChips = 10240;             // the tracking loops' limit
constexpr unsigned kCanMaxGrid = 1u << 16;      // workgroups; a longer call loops

struct CanSat {                                 // device form of a satellite
  const uint8_t* chips;                         // L bytes, 0 / 1
  double inv_l;
  unsigned L, kind;
  unsigned first, nseg;                         // its segments are segs[first .. first + nseg)
};

struct CanSeg {                                 // device form of a segment, 64 bytes
  long long s0;
  unsigned long long F, p0;                     // carrier step per sample and phase at s0, 2^-64 turn
  unsigned long long cf_frac, frac0;            // code step per sample (fraction) and subchip fraction at s0, 2^-64 chip
  unsigned n, cf_int, chip0;                    // samples; code step (whole chips, < 16); chip index at s0
  float ar, ai;                                 // float32(A)
  unsigned sat_touch;                           // satellite index | (the call works on this segment) << 8
};

// r = (rr, ri) and w of sample i = u of a segment.  (chip_at, cbit): the chip index whose byte the lane holds
__device__ __forceinline__ void cancel_replica(const CanSat& s, const CanSeg& g, unsigned u, unsigned& chip_at, unsigned& cbit, float& rr, float& ri,
                                               float& w) {
  const unsigned long long th = g.p0 + (unsigned long long)u * g.F;
  const unsigned long long lo = (unsigned long long)u * g.cf_frac, frac = g.frac0 + lo;
  const unsigned ct = g.chip0 + u * g.cf_int + (unsigned)__umul64hi((unsigned long long)u, g.cf_frac) + (frac < lo ? 1u : 0u);      // < 2^29
  unsigned chip = ct - (unsigned)((double)ct * s.inv_l) * s.L;
  if ((int)chip < 0) chip += s.L;
  if (chip >= s.L) chip -= s.L;
  if (chip != chip_at) {
    cbit = s.chips[chip];
    chip_at = chip;
  }
  const unsigned b1 = (unsigned)(frac >> 63);
  unsigned neg = cbit;
  float mag = 1.0f;
  if (s.kind == 1u) {
    neg ^= b1;
  } else if (s.kind == 2u || s.kind == 3u) {
    const unsigned b6 = (unsigned)__umul64hi(frac, 12ull) & 1u;
    if (s.kind == 2u) {
      neg ^= b1;                                                  // w (c1 s1 + c6 s6) = w s1 (c1 +- c6)
      mag = (b1 != b6) ? (float)(0.953463 - 0.301511) : (float)(0.953463 + 0.301511);
    } else {
      neg ^= ((gacq::kTmbocMask >> (chip % 33u)) & 1ull) ? b6 : b1;
    }
  } else if (s.kind >= 4u) {
    if ((s.kind == 4u) != (b1 == 0u)) mag = 0.0f;
  }
  w = __uint_as_float(__float_as_uint(mag) ^ (neg << 31));
  float c, sn;
  gacq::turn_sincos(th, c, sn);
  rr = w * c;
  ri = w * sn;
}

// ---- host ----

inline int can_check_rate(const char* who, int K, double fs) {
  if (K < 1 || K > kCanMaxK) return gacq::set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: need 1 <= K <= %d satellites (K %d)", who, kCanMaxK, K);
  if (!std::isfinite(fs) || !(fs > 0.0)) return gacq::set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: fs must be finite and positive", who);
  return GACQ_OK;
}

// the satellites and their segments (K is in range); amps: amp_re and amp_im are looked at; Ls (NULL or K ints) receives the code
// lengths, *total_out the number of segments
inline int can_check_table(const char* who, const gacq_cancel_sat* sats, int K, const gacq_cancel_seg* segs, double fs, bool amps, int* Ls,
                           long long* total_out) {
  long long total = 0;
  for (int k = 0; k < K; k++) {
    const gacq_cancel_sat& s = sats[k];
    if (!s.code) return gacq::set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: satellite %d has no code", who, k);
    const int L = gacq_code_length(s.code);
    if (L < 0) return gacq::set_error(nullptr, GACQ_ERR_UNKNOWN_CODE, "%s: satellite %d: unknown code '%s'", who, k, s.code);
    if (L > kCanMaxChips)
      return gacq::set_error(nullptr, GACQ_ERR_UNSUPPORTED, "%s: satellite %d: '%s' has %d chips, more than the %d served", who, k, s.code, L, kCanMaxChips);
    if (Ls) Ls[k] = L;
    std::vector<uint8_t> chips(L);
    const int rc = gacq_code_chips(s.code, s.prn, chips.data(), L);
    if (rc < 0) return gacq::set_error(nullptr, rc, "%s: satellite %d: no PRN %d in '%s'", who, k, s.prn, s.code);
    if (s.kind < 0 || s.kind > 5) return gacq::set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: satellite %d: kind %d outside 0..5", who, k, s.kind);
    if (s.nseg < 0 || s.nseg > kCanMaxSegs || (total += s.nseg) > kCanMaxSegs)
      return gacq::set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: satellite %d: need 0 <= nseg and at most %d segments in all", who, k, kCanMaxSegs);
  }
  const gacq_cancel_seg* g = segs;
  for (int k = 0; k < K; k++) {
    const int L = gacq_code_length(sats[k].code);
    for (int i = 0; i < sats[k].nseg; i++, g++) {
      if (!std::isfinite(g->carrier_hz) || !std::isfinite(g->carrier_phase) || !std::isfinite(g->code_rate_hz) || !std::isfinite(g->code_phase) ||
          (amps && (!std::isfinite(g->amp_re) || !std::isfinite(g->amp_im))))
        return gacq::set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: satellite %d, segment %d: a parameter is not finite", who, k, i);
      if (g->n < 1 || g->n > kCanMaxN || g->s0 < 0 || g->s0 > kStreamMaxIndex - g->n)
        return gacq::set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: satellite %d, segment %d: need 1 <= n <= 2^24, s0 >= 0 and s0 + n <= 2^48 (s0 %lld, n %lld)",
                               who, k, i, g->s0, g->n);
      if (!(g->code_rate_hz > 0.0) || !(g->code_rate_hz / fs < 16.0))
        return gacq::set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: satellite %d, segment %d: need 0 < code rate / fs < 16 (%g / %g)", who, k, i, g->code_rate_hz,
                               fs);
      if (!(g->code_phase >= 0.0 && g->code_phase < (double)L))
        return gacq::set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: satellite %d, segment %d: code phase %g outside [0, %d)", who, k, i, g->code_phase, L);
      if (i > 0 && g->s0 < g[-1].s0 + g[-1].n)
        return gacq::set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: satellite %d: segment %d (from %lld) starts before segment %d ends (%lld)", who, k, i, g->s0,
                               i - 1, g[-1].s0 + g[-1].n);
    }
  }
  if (total_out) *total_out = total;
  return GACQ_OK;
}

// The table of a checked call on the host and its place on the device (the context's "cancel:sats" and "cancel:segs": every call that
// uses them waits for its stream before it returns).
struct CanTable {
  std::vector<CanSat> sats;
  std::vector<CanSeg> segs;                     // at least one entry: still a valid address
  size_t S = 0;                                 // segments
  bool any = false;                             // some segment has its flag
  CanSat* d_sats = nullptr;
  CanSeg* d_segs = nullptr;
};

// Chip tables (looked up or generated, then on the device), fixed point, flags: flag(segment) says whether the call works on it.  Under
// the caller's GACQ_DEVICE.  who: the _dev entry point.
template <class Flag>
int can_table_build(gacq_ctx* ctx, const char* who, const gacq_cancel_sat* sats, int K, const gacq_cancel_seg* segs, const int* Ls, double fs, Flag flag,
                    CanTable& t) {
  int rc;
  std::vector<gacq::ChipTable> tabs(K);
  for (int k = 0; k < K; k++)
    if ((rc = gacq::chip_table_host(ctx, sats[k].code, sats[k].prn, Ls[k], true, tabs[k])) < 0)
      return gacq::set_error(ctx, rc, "%s: satellite %d: no PRN %d in '%s'", who, k, sats[k].prn, sats[k].code);
  t.S = 0;
  for (int k = 0; k < K; k++) t.S += (size_t)sats[k].nseg;
  t.sats.assign(K, CanSat());
  t.segs.assign(std::max<size_t>(t.S, 1), CanSeg());
  t.any = false;
  size_t at = 0;
  for (int k = 0; k < K; k++) {
    CanSat& ds = t.sats[k];
    if ((rc = gacq::chip_table_dev(ctx, tabs[k], &ds.chips)) != GACQ_OK) return rc;
    ds.L = (unsigned)Ls[k];
    ds.inv_l = 1.0 / (double)Ls[k];
    ds.kind = (unsigned)sats[k].kind;
    ds.first = (unsigned)at;
    ds.nseg = (unsigned)sats[k].nseg;
    for (int i = 0; i < sats[k].nseg; i++, at++) {
      const gacq_cancel_seg& g = segs[at];
      CanSeg& d = t.segs[at];
      std::memset(&d, 0, sizeof(d));
      d.s0 = g.s0;
      d.n = (unsigned)g.n;
      d.F = gacq::turn_fraction(g.carrier_hz / fs);
      d.p0 = gacq::turn_fraction(g.carrier_phase);
      unsigned long long ci, cw;
      gacq::turn_fixed(g.code_rate_hz / fs, ci, d.cf_frac);
      d.cf_int = (unsigned)ci;
      gacq::turn_fixed(g.code_phase, cw, d.frac0);
      d.chip0 = (unsigned)cw;
      d.ar = (float)g.amp_re;
      d.ai = (float)g.amp_im;
      const bool on = flag(g);
      t.any = t.any || on;
      d.sat_touch = (unsigned)k | (on ? 1u << 8 : 0u);
    }
  }
  gacq::DevBuf& d_sats = ctx->tables["cancel:sats"];
  gacq::DevBuf& d_segs = ctx->tables["cancel:segs"];
  if ((rc = gacq::ensure(ctx, d_sats, sizeof(CanSat) * kCanMaxK)) != GACQ_OK) return rc;
  if ((rc = gacq::ensure(ctx, d_segs, sizeof(CanSeg) * t.segs.size())) != GACQ_OK) return rc;
  t.d_sats = (CanSat*)d_sats.p;
  t.d_segs = (CanSeg*)d_segs.p;
  return GACQ_OK;
}

// The two uploads, queued: from pageable memory, so the caller waits for the stream on every way out
inline hipError_t can_table_queue(const CanTable& t, hipStream_t stream) {
  const hipError_t e = hipMemcpyAsync(t.d_sats, t.sats.data(), sizeof(CanSat) * t.sats.size(), hipMemcpyHostToDevice, stream);
  if (e != hipSuccess) return e;
  return hipMemcpyAsync(t.d_segs, t.segs.data(), sizeof(CanSeg) * t.segs.size(), hipMemcpyHostToDevice, stream);
}

}  // namespace
