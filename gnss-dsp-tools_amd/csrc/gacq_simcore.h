// What the recording generators share (gacq_simulate.hip, gacq_scene.hip): the device form of a satellite and its conversion from a
// gacq_sim_sat on the host (exact state at j0), Philox4x32-10 and the Box-Muller draw.  The quarter-turn sine / cosine, the
// conversions to 2^-64 fixed point and the TMBOC mask are gacq_turn.h's, shared with the cancel replica (gacq_cancelcore.h) and
// gacq_cohfold.hip.
// Both files compile with `#pragma clang fp contract(off)`; the functions below are inlined into their kernels and keep the
// operations, and so the bits, gacq_simulate.hip had when they lived there.
#pragma once

#include "gacq_common.h"
#include "gacq_turn.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace gacq {

constexpr int kSimMaxK = 32;
constexpr int kSimMaxSym = 1 << 20;
constexpr long long kSimMaxJ = 1ll << 48;

struct SimSat {                                 // device form of a satellite, state at j0
  const uint8_t* chips;                         // L bytes, 0 / 1
  const unsigned* symbits;                      // nsym bits (1 = symbol -1), or unused when nsym = 0
  unsigned long long F, th0;                    // carrier step per sample and phase at j0, 2^-64 turn
  unsigned long long cf_frac, frac0;            // code step per sample (fraction) and subchip fraction at j0, 2^-64 chip
  unsigned cf_int, chip0;                       // code step (whole chips, < 16) and chip index at j0
  unsigned L, kind, pps, nsym;
  unsigned sub0, sym0;                          // period mod pps and symbol index at j0
  float a0, a1;                                 // amplitude; CBOC: amp (0.953463 + 0.301511) and amp (0.953463 - 0.301511)
};

// words 0 and 1 of Philox4x32-10 for the counter (c0, c1, c2, c3)
__host__ __device__ __forceinline__ void simulate_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned& r0,
                                                         unsigned& r1) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1;
    c3 = (unsigned)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  r0 = c0;
  r1 = c1;
}

// Box-Muller of the draw of counter (j lo32, j hi32, c2, c3): sigma sqrt(-2 ln u1) (cos 2 pi u2, sin 2 pi u2)
__device__ __forceinline__ void simulate_noise(unsigned long long seed, unsigned long long j, unsigned c2, unsigned c3, float sigma, float& re,
                                               float& im) {
  unsigned r0, r1;
  simulate_philox((unsigned)j, (unsigned)(j >> 32), c2, c3, (unsigned)seed, (unsigned)(seed >> 32), r0, r1);
  // u1 = (2 (r0 >> 8) + 1) 2^-25 has 25 significant bits: ln u1 = ln(fp32 rounding) + (u1 - rounding) / rounding, the second term
  // at most 2^-25 / u1 and exact enough in fp32 (it is nonzero only for u1 >= 1/2)
  const unsigned m = 2u * (r0 >> 8) + 1u;
  const float fm = (float)m;
  const float e = (float)((int)m - (int)fm);
  const float u = fm * 2.98023223876953125e-08f;
  const float lnu = fmaf(e * 2.98023223876953125e-08f, 1.0f / u, logf(u));
  const float rad = sigma * sqrtf(-2.0f * lnu);
  float c, s;
  turn_sincos((unsigned long long)(2u * (r1 >> 8) + 1u) << 39, c, s);
  re = rad * c;
  im = rad * s;
}

// the checks of a call's range, rate and noise level; ctx may be NULL (the message then goes to gacq_last_error(NULL))
inline int sim_check_call(gacq_ctx* ctx, const char* who, double fs, double sigma, long long j0, long long n) {
  if (n < 1 || j0 < 0 || j0 > kSimMaxJ || n > kSimMaxJ - j0)
    return set_error(ctx, GACQ_ERR_BAD_ARG, "%s: need n >= 1, j0 >= 0 and j0 + n <= 2^48 (j0 %lld, n %lld)", who, j0, n);
  if (!std::isfinite(fs) || !(fs > 0.0) || !std::isfinite(sigma) || !(sigma >= 0.0))
    return set_error(ctx, GACQ_ERR_BAD_ARG, "%s: fs must be finite and positive, sigma finite and not negative", who);
  return GACQ_OK;
}

// the checks of K satellites; fills the code lengths and counts the 32-bit words their symbols take
inline int sim_check_sats(gacq_ctx* ctx, const char* who, const gacq_sim_sat* sats, int K, double fs, std::vector<int>& Ls, size_t& symwords) {
  Ls.assign(K, 0);
  symwords = 0;
  for (int k = 0; k < K; k++) {
    const gacq_sim_sat& s = sats[k];
    if (!s.code) return set_error(ctx, GACQ_ERR_BAD_ARG, "%s: satellite %d has no code", who, k);
    if (!std::isfinite(s.amp) || !std::isfinite(s.carrier_hz) || !std::isfinite(s.carrier_phase) || !std::isfinite(s.code_rate_hz) ||
        !std::isfinite(s.code_phase))
      return set_error(ctx, GACQ_ERR_BAD_ARG, "%s: satellite %d: a parameter is not finite", who, k);
    const int L = gacq_code_length(s.code);
    if (L < 0) return set_error(ctx, GACQ_ERR_UNKNOWN_CODE, "%s: satellite %d: unknown code '%s'", who, k, s.code);
    Ls[k] = L;
    if (!(s.code_rate_hz > 0.0) || !(s.code_rate_hz / fs < 16.0))
      return set_error(ctx, GACQ_ERR_BAD_ARG, "%s: satellite %d: need 0 < code rate / fs < 16 (%g / %g)", who, k, s.code_rate_hz, fs);
    if (!(s.code_phase >= 0.0 && s.code_phase < (double)L))
      return set_error(ctx, GACQ_ERR_BAD_ARG, "%s: satellite %d: code phase %g outside [0, %d)", who, k, s.code_phase, L);
    if (s.kind < 0 || s.kind > 5) return set_error(ctx, GACQ_ERR_BAD_ARG, "%s: satellite %d: kind %d outside 0..5", who, k, s.kind);
    if (s.nsym < 0 || s.nsym > kSimMaxSym || s.periods_per_symbol < 1 || (s.nsym > 0 && !s.symbols))
      return set_error(ctx, GACQ_ERR_BAD_ARG, "%s: satellite %d: need 0 <= nsym <= %d with symbols, periods_per_symbol >= 1", who, k, kSimMaxSym);
    for (int i = 0; i < s.nsym; i++)
      if (s.symbols[i] != 1 && s.symbols[i] != -1)
        return set_error(ctx, GACQ_ERR_BAD_ARG, "%s: satellite %d: symbol %d is %d, not +-1", who, k, i, (int)s.symbols[i]);
    symwords += ((size_t)s.nsym + 31) / 32;
  }
  return GACQ_OK;
}

// chip tables, on the host first: one per code and PRN, generated only when the context's cache lacks it (GLONASS P is 5.11 M chips)
inline int sim_chip_tables(gacq_ctx* ctx, const char* who, const gacq_sim_sat* sats, int K, const std::vector<int>& Ls, std::vector<ChipTable>& tabs) {
  tabs.assign(K, ChipTable());
  for (int k = 0; k < K; k++) {
    int first = 0;
    while (first < k && (sats[first].prn != sats[k].prn || std::strcmp(sats[first].code, sats[k].code))) first++;
    if (first < k) {
      tabs[k].key = tabs[first].key;
    } else {
      const int rc = chip_table_host(ctx, sats[k].code, sats[k].prn, Ls[k], true, tabs[k]);
      if (rc < 0) return set_error(ctx, rc, "%s: satellite %d: no PRN %d in '%s'", who, k, sats[k].prn, sats[k].code);
    }
  }
  return GACQ_OK;
}

// The device forms of K checked satellites at j0 into h[0 .. K), their symbol bits into hsym; d_sym is the device address hsym is
// copied to.
inline void sim_fill_sats(const gacq_sim_sat* sats, int K, const std::vector<int>& Ls, const std::vector<const uint8_t*>& d_chips, double fs,
                          long long j0, SimSat* h, unsigned* hsym, const unsigned* d_sym) {
  size_t w0 = 0;
  for (int k = 0; k < K; k++) {
    const gacq_sim_sat& s = sats[k];
    const unsigned L = (unsigned)Ls[k];
    SimSat& t = h[k];
    std::memset(&t, 0, sizeof(t));
    t.chips = d_chips[k];
    t.F = turn_fraction(s.carrier_hz / fs);
    t.th0 = turn_fraction(s.carrier_phase) + (unsigned long long)j0 * t.F;
    unsigned long long ci, cw;
    turn_fixed(s.code_rate_hz / fs, ci, t.cf_frac);
    t.cf_int = (unsigned)ci;
    turn_fixed(s.code_phase, cw, t.frac0);
    // pos(j0) = c0 + j0 Cf, exact: j0 < 2^48 and Cf < 2^68
    const unsigned __int128 pos = (((unsigned __int128)cw << 64) | t.frac0) + (unsigned __int128)(unsigned long long)j0 * ((((unsigned __int128)ci) << 64) | t.cf_frac);
    t.frac0 = (unsigned long long)pos;
    const unsigned long long ct = (unsigned long long)(pos >> 64), per = ct / L;
    t.chip0 = (unsigned)(ct - per * L);
    t.L = L;
    t.kind = (unsigned)s.kind;
    t.pps = (unsigned)s.periods_per_symbol;
    t.nsym = (unsigned)s.nsym;
    t.sub0 = (unsigned)(per % t.pps);
    t.sym0 = t.nsym ? (unsigned)((per / t.pps) % t.nsym) : 0u;
    t.a0 = (float)(s.kind == 2 ? s.amp * (0.953463 + 0.301511) : s.amp);
    t.a1 = (float)(s.amp * (0.953463 - 0.301511));
    t.symbits = d_sym + w0;
    const size_t nw = ((size_t)s.nsym + 31) / 32;
    for (size_t w = 0; w < nw; w++) hsym[w0 + w] = 0u;
    for (int i = 0; i < s.nsym; i++)
      if (s.symbols[i] < 0) hsym[w0 + (size_t)(i >> 5)] |= 1u << (i & 31);
    w0 += nw;
  }
}

}  // namespace gacq
