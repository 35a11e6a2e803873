// Synthetic multi-satellite recordings (gacq_simulate_dev, include/gacq.h): samples j = j0 .. j0 + n - 1 of one endless recording that is
// an exact function of (scene, seed, absolute sample index j),
//   v(j) = noise(seed, j) + sum_{k<K} amp_k w_k(j) d_k(j) exp(2 pi i theta_k(j) / 2^64),
// as complex64 or as interleaved int8 clip(rint(v), -127, 127).  Which chip, subcarrier half, symbol and noise draw a sample gets is
// integer arithmetic on j, so the bytes do not depend on how a caller cuts the recording into calls:
//   theta(j) = (p0 + j F) mod 2^64                    carrier phase, 2^-64 turn
//   pos(j)   = c0 + j Cf                              code position, 2^-64 chip, exact (up to 116 bits)
//   chip = (pos >> 64) mod L, period = (pos >> 64) div L, subchip fraction = pos mod 2^64
//   noise: Philox4x32-10, key = seed, counter = (j, 0, 0); words r0, r1 -> Box-Muller
//
// The host converts F, p0, Cf, c0 from the doubles of the scene and evaluates (theta, period, chip, fraction) exactly at j0
// (unsigned __int128), so the device part fits 64 bits: a lane owns kRun = 8 consecutive samples, multiplies its offset from j0 into
// each satellite's state once (one 64 x 64 -> 128 product and one division by L per lane and satellite, 32-bit whenever the chips
// since j0 fit 32 bits) and then advances by additions: 64-bit for the carrier, 64 + 32 bits with carry for the code, wrapped at L by
// compare-subtract.  The satellite parameters are read at wave-uniform addresses.  Chips come from the context's cached byte tables
// ("chips:<code>:<prn>", shared with the tracking loops); consecutive samples mostly hit the same byte, which is reloaded only when
// the chip index moves.  Symbols are bit-packed in the call's parameter block.
//
// sin / cos of the carrier and of the Box-Muller angle: the fixed-point quarter-turn reduction and polynomials of gacq_cohfold.hip
// in a copy of their own (that file's bits stay what they are).  ln u1 is the accurate logf of u1 rounded to fp32 plus the
// first-order term of the rounding, so the radius keeps its relative accuracy where u1 -> 1.
// The int8 output is rint / clamp of the very fp32 values the complex64 output stores: same operations, same order.
#pragma clang fp contract(off)

#include "gacq_common.h"

#include <cmath>
#include <cstring>
#include <vector>

using namespace gacq;

namespace {

constexpr int kSimBlock = 256;
constexpr int kRun = 8;                         // samples per lane and pass: one 16-byte store of int8 I/Q
constexpr int kSimMaxK = 32;
constexpr int kSimMaxSym = 1 << 20;
constexpr unsigned kSimMaxGrid = 1u << 16;      // workgroups; a longer call loops
constexpr long long kSimMaxJ = 1ll << 48;
constexpr unsigned long long kTmbocMask = (1ull << 0) | (1ull << 4) | (1ull << 6) | (1ull << 29);      // 64 bits: it is shifted by up to 32

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

struct SimArgs {
  const SimSat* sats;
  void* out;
  long long j0, n;
  unsigned long long seed;
  float sigma;
  int K;
  int aligned;                                  // out is 16-byte aligned
};

// (cos, sin) of 2 pi ph / 2^64
__device__ __forceinline__ void simulate_sincos_turn(unsigned long long ph, float& c, float& s) {
  const unsigned u = (unsigned)(ph >> 32) + 0x20000000u;          // + 1/8 turn: the quadrant index rounds to nearest
  const unsigned q = u >> 30;
  const float t = (float)((int)(u & 0x3fffffffu) - 0x20000000) * 9.31322574615478515625e-10f;      // quarter turns, [-1/2, 1/2)
  const float t2 = t * t;
  float ps = fmaf(t2, -4.602163099e-03f, 7.968021929e-02f);
  ps = fmaf(ps, t2, -6.459634900e-01f);
  ps = fmaf(ps, t2, 1.570796371e+00f) * t;
  float pc = fmaf(t2, 9.036298725e-04f, -2.086007036e-02f);
  pc = fmaf(pc, t2, 2.536692023e-01f);
  pc = fmaf(pc, t2, -1.233700514e+00f);
  pc = fmaf(pc, t2, 1.0f);
  const float a = (q & 1u) ? ps : pc, b = (q & 1u) ? pc : ps;     // quarter turns: (c, s), (-s, c), (-c, -s), (s, -c)
  c = __uint_as_float(__float_as_uint(a) ^ ((((q + 1u) >> 1) & 1u) << 31));
  s = __uint_as_float(__float_as_uint(b) ^ (((q >> 1) & 1u) << 31));
}

// words 0 and 1 of Philox4x32-10 for the counter (c0, c1, 0, 0)
__host__ __device__ __forceinline__ void simulate_philox(unsigned c0, unsigned c1, unsigned k0, unsigned k1, unsigned& r0, unsigned& r1) {
  unsigned c2 = 0u, c3 = 0u;
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

// (nI, nQ) of absolute sample j
__device__ __forceinline__ void simulate_noise(unsigned long long seed, unsigned long long j, float sigma, float& re, float& im) {
  unsigned r0, r1;
  simulate_philox((unsigned)j, (unsigned)(j >> 32), (unsigned)seed, (unsigned)(seed >> 32), r0, r1);
  // u1 = (2 (r0 >> 8) + 1) 2^-25 has 25 significant bits: ln u1 = ln(fp32 rounding) + (u1 - rounding) / rounding, the second term
  // at most 2^-25 / u1 and exact enough in fp32 (it is nonzero only for u1 >= 1/2)
  const unsigned m = 2u * (r0 >> 8) + 1u;
  const float fm = (float)m;
  const float e = (float)((int)m - (int)fm);
  const float u = fm * 2.98023223876953125e-08f;
  const float lnu = fmaf(e * 2.98023223876953125e-08f, 1.0f / u, logf(u));
  const float rad = sigma * sqrtf(-2.0f * lnu);
  float c, s;
  simulate_sincos_turn((unsigned long long)(2u * (r1 >> 8) + 1u) << 39, c, s);
  re = rad * c;
  im = rad * s;
}

// grid-stride over runs of kRun samples; lane-run r covers samples [r kRun, r kRun + kRun) of the call
template <bool CPLX>
__global__ __launch_bounds__(kSimBlock) void simulate_kernel(const SimArgs a) {
  const long long nruns = (a.n + kRun - 1) / kRun;
  const SimSat* __restrict__ sats = a.sats;
  for (long long r = (long long)blockIdx.x * kSimBlock + threadIdx.x; r < nruns; r += (long long)gridDim.x * kSimBlock) {
    const unsigned long long m = (unsigned long long)r * kRun;      // offset from j0, < 2^48
    float vr[kRun], vi[kRun];
#pragma unroll
    for (int i = 0; i < kRun; i++) simulate_noise(a.seed, (unsigned long long)a.j0 + m + i, a.sigma, vr[i], vi[i]);
    for (int k = 0; k < a.K; k++) {
      const SimSat s = sats[k];                                     // the same address in every lane
      unsigned long long th = s.th0 + m * s.F;
      // pos(j0 + m) = pos(j0) + m Cf: fraction with carry, whole chips since j0 < 2^53
      const unsigned long long lo = m * s.cf_frac, fsum = s.frac0 + lo;
      const unsigned long long ct = (unsigned long long)s.chip0 + m * s.cf_int + __umul64hi(m, s.cf_frac) + (fsum < lo ? 1ull : 0ull);
      unsigned long long frac = fsum;
      unsigned long long per;
      unsigned chip;
      if ((ct >> 32) == 0ull) {
        per = (unsigned)ct / s.L;
        chip = (unsigned)ct - (unsigned)per * s.L;
      } else {
        per = ct / s.L;
        chip = (unsigned)(ct - per * s.L);
      }
      unsigned sub = 0u, sym = 0u, dneg = 0u;
      if (s.nsym) {
        const unsigned long long t = (unsigned long long)s.sub0 + per;
        unsigned long long q;
        if ((t >> 32) == 0ull) {
          q = (unsigned)t / s.pps;
          sub = (unsigned)t - (unsigned)q * s.pps;
        } else {
          q = t / s.pps;
          sub = (unsigned)(t - q * s.pps);
        }
        sym = (unsigned)(((unsigned long long)s.sym0 + q) % s.nsym);
        dneg = (s.symbits[sym >> 5] >> (sym & 31u)) & 1u;
      }
      unsigned cbit = s.chips[chip];
#pragma unroll
      for (int i = 0; i < kRun; i++) {
        const unsigned b1 = (unsigned)(frac >> 63);
        unsigned neg = cbit ^ dneg;
        float mag = s.a0;
        if (s.kind == 1u) {
          neg ^= b1;
        } else if (s.kind == 2u || s.kind == 3u) {
          const unsigned b6 = (unsigned)__umul64hi(frac, 12ull) & 1u;
          if (s.kind == 2u) {
            neg ^= b1;                                              // w (c1 s1 + c6 s6) = w s1 (c1 +- c6)
            mag = (b1 != b6) ? s.a1 : s.a0;
          } else {
            neg ^= ((kTmbocMask >> (chip % 33u)) & 1ull) ? b6 : b1;
          }
        } else if (s.kind >= 4u) {
          if ((s.kind == 4u) != (b1 == 0u)) mag = 0.0f;
        }
        const float amp = __uint_as_float(__float_as_uint(mag) ^ (neg << 31));
        float c, sn;
        simulate_sincos_turn(th, c, sn);
        vr[i] = fmaf(amp, c, vr[i]);
        vi[i] = fmaf(amp, sn, vi[i]);
        if (i + 1 < kRun) {
          th += s.F;
          const unsigned long long f2 = frac + s.cf_frac;
          unsigned step = s.cf_int + (f2 < frac ? 1u : 0u);
          frac = f2;
          if (step) {
            chip += step;
            while (chip >= s.L) {                                   // one code period
              chip -= s.L;
              if (s.nsym && ++sub == s.pps) {
                sub = 0u;
                if (++sym == s.nsym) sym = 0u;
                dneg = (s.symbits[sym >> 5] >> (sym & 31u)) & 1u;
              }
            }
            cbit = s.chips[chip];
          }
        }
      }
    }
    const long long left = a.n - (long long)m;
    if (CPLX) {
      float2* __restrict__ o = reinterpret_cast<float2*>(a.out) + m;
      if (left >= kRun && a.aligned) {
#pragma unroll
        for (int i = 0; i < kRun; i += 2) reinterpret_cast<float4*>(o)[i / 2] = make_float4(vr[i], vi[i], vr[i + 1], vi[i + 1]);
      } else {
#pragma unroll
        for (int i = 0; i < kRun; i++)
          if (i < left) o[i] = make_float2(vr[i], vi[i]);
      }
    } else {
      unsigned b[2 * kRun];
#pragma unroll
      for (int i = 0; i < kRun; i++) {
        b[2 * i] = (unsigned)(int)fminf(fmaxf(rintf(vr[i]), -127.0f), 127.0f) & 0xffu;      // rintf: half to even
        b[2 * i + 1] = (unsigned)(int)fminf(fmaxf(rintf(vi[i]), -127.0f), 127.0f) & 0xffu;
      }
      uint8_t* __restrict__ o = reinterpret_cast<uint8_t*>(a.out) + 2 * m;
      if (left >= kRun && a.aligned) {
        uint4 w;
        w.x = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        w.y = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
        w.z = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
        w.w = b[12] | (b[13] << 8) | (b[14] << 16) | (b[15] << 24);
        *reinterpret_cast<uint4*>(o) = w;
      } else {
#pragma unroll
        for (int i = 0; i < kRun; i++)
          if (i < left) {
            o[2 * i] = (uint8_t)b[2 * i];
            o[2 * i + 1] = (uint8_t)b[2 * i + 1];
          }
      }
    }
  }
}

// floor(frac(v) 2^64) mod 2^64, in IEEE double operations (tests/simulate_oracle.py restates it)
unsigned long long sim_turns(double v) {
  const double t = v - std::floor(v);                               // [0, 1]; 1 only when a tiny negative v rounds up
  return t >= 1.0 ? 0ull : (unsigned long long)std::floor(std::ldexp(t, 64));
}

// whole part and floor(fraction 2^64) of v >= 0
void sim_fixed(double v, unsigned long long& whole, unsigned long long& frac) {
  const double w = std::floor(v);
  whole = (unsigned long long)w;
  frac = (unsigned long long)std::floor(std::ldexp(v - w, 64));     // v - w is exact and below 1
}

}  // namespace

extern "C" int gacq_simulate_dev(gacq_ctx* ctx, const gacq_sim_sat* sats, int K, double fs, double sigma, unsigned long long seed, long long j0,
                                 long long n, int out_complex64, void* d_out) {
  if (!ctx) return GACQ_ERR_BAD_ARG;
  if (!sats || !d_out) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_simulate_dev: NULL argument");
  // everything is checked before anything is allocated or launched
  if (K < 1 || K > kSimMaxK) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_simulate_dev: need 1 <= K <= %d satellites (K %d)", kSimMaxK, K);
  if (n < 1 || j0 < 0 || j0 > kSimMaxJ || n > kSimMaxJ - j0)
    return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_simulate_dev: need n >= 1, j0 >= 0 and j0 + n <= 2^48 (j0 %lld, n %lld)", j0, n);
  if (!std::isfinite(fs) || !(fs > 0.0) || !std::isfinite(sigma) || !(sigma >= 0.0))
    return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_simulate_dev: fs must be finite and positive, sigma finite and not negative");
  if ((uintptr_t)d_out % (out_complex64 ? 8u : 1u)) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_simulate_dev: complex64 output must be 8-byte aligned");
  std::vector<int> Ls(K);
  size_t symwords = 0;
  for (int k = 0; k < K; k++) {
    const gacq_sim_sat& s = sats[k];
    if (!s.code) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_simulate_dev: satellite %d has no code", k);
    if (!std::isfinite(s.amp) || !std::isfinite(s.carrier_hz) || !std::isfinite(s.carrier_phase) || !std::isfinite(s.code_rate_hz) ||
        !std::isfinite(s.code_phase))
      return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_simulate_dev: satellite %d: a parameter is not finite", k);
    const int L = gacq_code_length(s.code);
    if (L < 0) return set_error(ctx, GACQ_ERR_UNKNOWN_CODE, "gacq_simulate_dev: satellite %d: unknown code '%s'", k, s.code);
    Ls[k] = L;
    if (!(s.code_rate_hz > 0.0) || !(s.code_rate_hz / fs < 16.0))
      return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_simulate_dev: satellite %d: need 0 < code rate / fs < 16 (%g / %g)", k, s.code_rate_hz, fs);
    if (!(s.code_phase >= 0.0 && s.code_phase < (double)L))
      return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_simulate_dev: satellite %d: code phase %g outside [0, %d)", k, s.code_phase, L);
    if (s.kind < 0 || s.kind > 5) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_simulate_dev: satellite %d: kind %d outside 0..5", k, s.kind);
    if (s.nsym < 0 || s.nsym > kSimMaxSym || s.periods_per_symbol < 1 || (s.nsym > 0 && !s.symbols))
      return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_simulate_dev: satellite %d: need 0 <= nsym <= %d with symbols, periods_per_symbol >= 1", k, kSimMaxSym);
    for (int i = 0; i < s.nsym; i++)
      if (s.symbols[i] != 1 && s.symbols[i] != -1)
        return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_simulate_dev: satellite %d: symbol %d is %d, not +-1", k, i, (int)s.symbols[i]);
    symwords += ((size_t)s.nsym + 31) / 32;
  }
  // chip tables, on the host first: one per code and PRN, generated only when the context's cache lacks it (GLONASS P is 5.11 M chips)
  std::vector<ChipTable> tabs(K);
  for (int k = 0; k < K; k++) {
    int first = 0;
    while (first < k && (sats[first].prn != sats[k].prn || std::strcmp(sats[first].code, sats[k].code))) first++;
    if (first < k) {
      tabs[k].key = tabs[first].key;
    } else {
      const int rc = chip_table_host(ctx, sats[k].code, sats[k].prn, Ls[k], true, tabs[k]);
      if (rc < 0) return set_error(ctx, rc, "gacq_simulate_dev: satellite %d: no PRN %d in '%s'", k, sats[k].prn, sats[k].code);
    }
  }
  const size_t o_sym = sizeof(SimSat) * (size_t)K, bytes = o_sym + sizeof(unsigned) * symwords;
  GACQ_DEVICE(ctx);
  hipStream_t stream = ctx->stream;
  int rc;
  std::vector<const uint8_t*> d_chips(K);
  for (int k = 0; k < K; k++)
    if ((rc = chip_table_dev(ctx, tabs[k], &d_chips[k])) != GACQ_OK) return rc;
  // the parameter block is staged in pinned memory, two slots in turn, as gacq_fold_dev does: a slot is rewritten only after the
  // launch that last used it has finished (its event), so the call returns as soon as the copy and the kernel are queued
  const int slot = ctx->sim_slot;
  if (ctx->sim_done[slot]) GACQ_HIP(ctx, hipEventSynchronize(ctx->sim_done[slot]));
  else GACQ_HIP(ctx, hipEventCreateWithFlags(&ctx->sim_done[slot], hipEventDisableTiming));
  DevBuf& d_par = ctx->tables[slot ? "simulate:params1" : "simulate:params0"];
  if ((rc = ensure_pinned(ctx, ctx->pin_sim[slot], bytes)) != GACQ_OK) return rc;
  if ((rc = ensure(ctx, d_par, bytes)) != GACQ_OK) return rc;
  unsigned char* host = (unsigned char*)ctx->pin_sim[slot].p;
  SimSat* h = (SimSat*)host;
  unsigned* hsym = (unsigned*)(host + o_sym);
  size_t w0 = 0;
  for (int k = 0; k < K; k++) {
    const gacq_sim_sat& s = sats[k];
    const unsigned L = (unsigned)Ls[k];
    SimSat& t = h[k];
    std::memset(&t, 0, sizeof(t));
    t.chips = d_chips[k];
    t.F = sim_turns(s.carrier_hz / fs);
    t.th0 = sim_turns(s.carrier_phase) + (unsigned long long)j0 * t.F;
    unsigned long long ci, cw;
    sim_fixed(s.code_rate_hz / fs, ci, t.cf_frac);
    t.cf_int = (unsigned)ci;
    sim_fixed(s.code_phase, cw, t.frac0);
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
    t.symbits = (const unsigned*)((const unsigned char*)d_par.p + o_sym) + w0;
    const size_t nw = ((size_t)s.nsym + 31) / 32;
    for (size_t w = 0; w < nw; w++) hsym[w0 + w] = 0u;
    for (int i = 0; i < s.nsym; i++)
      if (s.symbols[i] < 0) hsym[w0 + (size_t)(i >> 5)] |= 1u << (i & 31);
    w0 += nw;
  }
  // from here on the slot's pinned block may be in use by a queued copy: the event is recorded on every way out, failures included
  hipError_t e = hipMemcpyAsync(d_par.p, host, bytes, hipMemcpyHostToDevice, stream);
  if (e != hipSuccess) {
    (void)hipEventRecord(ctx->sim_done[slot], stream);
    return set_error(ctx, GACQ_ERR_HIP, "gacq_simulate_dev: parameter upload failed: %s", hipGetErrorString(e));
  }
  SimArgs a;
  a.sats = (const SimSat*)d_par.p;
  a.out = d_out;
  a.j0 = j0;
  a.n = n;
  a.seed = seed;
  a.sigma = (float)sigma;
  a.K = K;
  a.aligned = ((uintptr_t)d_out % 16u) == 0u;
  const long long nblk = ((n + kRun - 1) / kRun + kSimBlock - 1) / kSimBlock;
  const unsigned grid = (unsigned)std::min<long long>(nblk, (long long)kSimMaxGrid);
  if (out_complex64) hipLaunchKernelGGL((simulate_kernel<true>), dim3(grid), dim3(kSimBlock), 0, stream, a);
  else hipLaunchKernelGGL((simulate_kernel<false>), dim3(grid), dim3(kSimBlock), 0, stream, a);
  e = hipGetLastError();
  const hipError_t e2 = hipEventRecord(ctx->sim_done[slot], stream);
  if (e != hipSuccess) return set_error(ctx, GACQ_ERR_HIP, "gacq_simulate_dev: launch failed: %s", hipGetErrorString(e));
  GACQ_HIP(ctx, e2);
  ctx->sim_slot = slot ^ 1;
  return GACQ_OK;
}
