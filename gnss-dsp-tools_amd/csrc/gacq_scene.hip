// Array-and-interference scenes (gacq_scene_dev, include/gacq.h): samples j = j0 .. j0 + n - 1 of antennas a = a0 .. a0 + M - 1 of one
// endless multi-antenna recording that is an exact function of (scene, seed, antenna, absolute sample index),
//   v_a(j) = noise_a(j) + sum_{e < K + I} G[a][e] z_e(j),
// the K satellites of gacq_simulate_dev first, then I emitters (tone, sawtooth chirp, triangle chirp, broadband noise), each waveform
// z_e(j) evaluated once per sample and spread over the antennas by the complex gains.  One launch.
//
// A lane owns a run of consecutive samples of every antenna of the call: 8 samples with one antenna, 4 with two to six, 2 with seven
// or eight, so the accumulators are at most 48 registers and every instantiation stays within 128 VGPRs (four waves per SIMD) without
// scratch; longer runs spilled.  The kernel is instantiated per antenna count; the run length, the antenna
// count, first_antenna, j0 and n decide only which lane evaluates a sample, never how: every phase is integer arithmetic mod 2^64 on
// the absolute index, and the fp32 operations on a sample of an antenna are the same in every instantiation.
//   per sample and source:  z = (zr, zi) once; per antenna  vr = fma(-Gi, zi, fma(Gr, zr, vr)),  vi = fma(Gi, zr, fma(Gr, zi, vi))
//   per sample and antenna: the noise draw of counter (j lo32, j hi32, antenna, 0), before every source
// The host evaluates every state exactly at j0 (satellites: gacq_simcore.h; emitters: the sweep count and the place in the sweep, the
// phase at the start of that sweep, the place in the gate period), so the device part fits 64 bits; a lane multiplies its offset
// from j0 into each state once and then advances by additions.  The gains are stored source-major so that a source's M gains are one
// wave-uniform block.  The int8 output is rint / clamp of the very fp32 values the complex64 output stores.
#pragma clang fp contract(off)

#include "gacq_simcore.h"

using namespace gacq;

namespace {

constexpr int kScBlock = 256;
constexpr int kScMaxM = 8;
constexpr int kScMaxI = 8;
constexpr unsigned kScMaxGrid = 1u << 16;       // workgroups; a longer call loops
constexpr long long kScMaxSweep = 1ll << 31;

constexpr int scene_run(int M) { return M == 1 ? 8 : M <= 6 ? 4 : 2; }      // samples per lane and pass

struct SceneEm {                                // device form of an emitter, state at j0
  unsigned long long th0;                       // tone: theta(j0); chirp: p0 + (j0 div P) Phi, the phase at the start of j0's sweep
  unsigned long long F0, R, Phi;                // 2^-64 turn: start frequency word, ramp step, phase gained by one sweep
  unsigned long long g0, gper, gon;             // gate: (j0 - first) mod period, period (0: always on), samples on
  unsigned u0, P, H;                            // chirp: j0 mod P, sweep length, samples of the rising ramp (sawtooth: P)
  unsigned kind;
  float amp;
  unsigned pad;
};

// In the parameter block, not in the kernel arguments: a lane reads the first antenna before its noise draws and a row's address before
// its stores, so that neither the antennas' Philox products nor the addresses are held in scalar registers across the sources.
struct SceneRows {
  void* out[kScMaxM];
  unsigned a0;                                  // first antenna
  unsigned pad;
};

struct SceneArgs {
  const SimSat* sats;
  const SceneEm* ems;
  const float2* gains;                          // [K + I][M]
  const SceneRows* rows;
  long long j0, n;
  unsigned long long seed;
  float sigma;
  int K, I;
};

// sum of ramp(t) over t < u
__device__ __forceinline__ unsigned long long scene_ramp_sum(unsigned long long u, unsigned long long P, unsigned long long H) {
  const unsigned long long tri = (u * (u - 1ull)) >> 1;            // u (u - 1) < 2^62
  return u <= H ? tri : H * (H - 1ull) + (u - H) * (P - 1ull) - tri;
}

template <int M, int RUN>
__device__ __forceinline__ void scene_spread(const float2* __restrict__ g, float zr, float zi, int i, float (&vr)[M][RUN], float (&vi)[M][RUN]) {
#pragma unroll
  for (int a = 0; a < M; a++) {
    const float2 w = g[a];                                          // the same address in every lane
    vr[a][i] = fmaf(-w.y, zi, fmaf(w.x, zr, vr[a][i]));
    vi[a][i] = fmaf(w.y, zr, fmaf(w.x, zi, vi[a][i]));
  }
}

// grid-stride over runs of RUN samples; lane-run r covers samples [r RUN, r RUN + RUN) of the call, of all M antennas
template <bool CPLX, int M>
__global__ __launch_bounds__(kScBlock, 4) void scene_kernel(const SceneArgs a) {
  constexpr int RUN = scene_run(M);
  const long long nruns = (a.n + RUN - 1) / RUN;
  const SimSat* __restrict__ sats = a.sats;
  const SceneEm* __restrict__ ems = a.ems;
  for (long long r = (long long)blockIdx.x * kScBlock + threadIdx.x; r < nruns; r += (long long)gridDim.x * kScBlock) {
    const unsigned long long m = (unsigned long long)r * RUN;       // offset from j0, < 2^48
    const unsigned long long j = (unsigned long long)a.j0 + m;
    float vr[M][RUN], vi[M][RUN];
    const unsigned a0 = a.rows->a0;                                 // the same address in every lane
#pragma unroll
    for (int p = 0; p < M; p++)
#pragma unroll
      for (int i = 0; i < RUN; i++) simulate_noise(a.seed, j + i, a0 + (unsigned)p, 0u, a.sigma, vr[p][i], vi[p][i]);
    // ---- satellites: the walk of gacq_simulate.hip
    for (int k = 0; k < a.K; k++) {
      const SimSat s = sats[k];                                     // the same address in every lane
      const float2* __restrict__ g = a.gains + (size_t)k * M;
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
      for (int i = 0; i < RUN; i++) {
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
        turn_sincos(th, c, sn);
        scene_spread<M, RUN>(g, amp * c, amp * sn, i, vr, vi);
        if (i + 1 < RUN) {
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
    // ---- emitters
    for (int e = 0; e < a.I; e++) {
      const SceneEm s = ems[e];                                     // the same address in every lane
      const float2* __restrict__ g = a.gains + (size_t)(a.K + e) * M;
      unsigned long long gp = 0ull;                                 // place in the gate period; without a gate it never reaches gon
      if (s.gper) {
        const unsigned long long t = s.g0 + m;                      // < 2^49
        gp = ((t | s.gper) >> 32) == 0ull ? (unsigned long long)((unsigned)t % (unsigned)s.gper) : t % s.gper;
      }
      unsigned long long th = 0ull;
      unsigned u = 0u;
      if (s.kind == 0u) {
        th = s.th0 + m * s.F0;
      } else if (s.kind != 3u) {
        const unsigned long long t = (unsigned long long)s.u0 + m;  // < 2^49
        unsigned long long ds;
        if ((t >> 32) == 0ull) {
          ds = (unsigned)t / s.P;
          u = (unsigned)t - (unsigned)ds * s.P;
        } else {
          ds = t / s.P;
          u = (unsigned)(t - ds * s.P);
        }
        th = s.th0 + ds * s.Phi + (unsigned long long)u * s.F0 + s.R * scene_ramp_sum(u, s.P, s.H);
      }
#pragma unroll
      for (int i = 0; i < RUN; i++) {
        const bool on = gp < s.gon;
        float zr, zi;
        if (s.kind == 3u) {
          simulate_noise(a.seed, j + i, (unsigned)e, 1u, s.amp, zr, zi);
          zr = on ? zr : 0.0f;
          zi = on ? zi : 0.0f;
        } else {
          const float amp = on ? s.amp : 0.0f;
          float c, sn;
          turn_sincos(th, c, sn);
          zr = amp * c;
          zi = amp * sn;
        }
        scene_spread<M, RUN>(g, zr, zi, i, vr, vi);
        if (i + 1 < RUN) {
          if (s.kind == 0u) {
            th += s.F0;
          } else if (s.kind != 3u) {
            th += s.F0 + s.R * (unsigned long long)(u < s.H ? u : s.P - 1u - u);      // the frequency word of sample u
            if (++u == s.P) u = 0u;
          }
          if (++gp == s.gper) gp = 0ull;
        }
      }
    }
    // ---- stores
    const long long left = a.n - (long long)m;
#pragma unroll
    for (int p = 0; p < M; p++) {
      void* const row = a.rows->out[p];                                   // the same address in every lane
      if (CPLX) {
        float2* __restrict__ o = reinterpret_cast<float2*>(row) + m;
        if (left >= RUN && ((uintptr_t)row % 16u) == 0u) {
#pragma unroll
          for (int i = 0; i < RUN; i += 2) reinterpret_cast<float4*>(o)[i / 2] = make_float4(vr[p][i], vi[p][i], vr[p][i + 1], vi[p][i + 1]);
        } else {
#pragma unroll
          for (int i = 0; i < RUN; i++)
            if (i < left) o[i] = make_float2(vr[p][i], vi[p][i]);
        }
      } else {
        unsigned b[2 * RUN];
#pragma unroll
        for (int i = 0; i < RUN; i++) {
          b[2 * i] = (unsigned)(int)fminf(fmaxf(rintf(vr[p][i]), -127.0f), 127.0f) & 0xffu;      // rintf: half to even
          b[2 * i + 1] = (unsigned)(int)fminf(fmaxf(rintf(vi[p][i]), -127.0f), 127.0f) & 0xffu;
        }
        uint8_t* __restrict__ o = reinterpret_cast<uint8_t*>(row) + 2 * m;
        if (left >= RUN && ((uintptr_t)row % (2u * RUN)) == 0u) {
          unsigned w[RUN / 2];
#pragma unroll
          for (int q = 0; q < RUN / 2; q++) w[q] = b[4 * q] | (b[4 * q + 1] << 8) | (b[4 * q + 2] << 16) | (b[4 * q + 3] << 24);
          if constexpr (RUN == 8) *reinterpret_cast<uint4*>(o) = make_uint4(w[0], w[1], w[2], w[3]);
          else if constexpr (RUN == 4) *reinterpret_cast<uint2*>(o) = make_uint2(w[0], w[1]);
          else *reinterpret_cast<unsigned*>(o) = w[0];
        } else {
#pragma unroll
          for (int i = 0; i < RUN; i++)
            if (i < left) {
              o[2 * i] = (uint8_t)b[2 * i];
              o[2 * i + 1] = (uint8_t)b[2 * i + 1];
            }
        }
      }
    }
  }
}

template <bool CPLX>
void scene_launch(int M, unsigned grid, hipStream_t stream, const SceneArgs& a) {
  switch (M) {
    case 1: hipLaunchKernelGGL((scene_kernel<CPLX, 1>), dim3(grid), dim3(kScBlock), 0, stream, a); break;
    case 2: hipLaunchKernelGGL((scene_kernel<CPLX, 2>), dim3(grid), dim3(kScBlock), 0, stream, a); break;
    case 3: hipLaunchKernelGGL((scene_kernel<CPLX, 3>), dim3(grid), dim3(kScBlock), 0, stream, a); break;
    case 4: hipLaunchKernelGGL((scene_kernel<CPLX, 4>), dim3(grid), dim3(kScBlock), 0, stream, a); break;
    case 5: hipLaunchKernelGGL((scene_kernel<CPLX, 5>), dim3(grid), dim3(kScBlock), 0, stream, a); break;
    case 6: hipLaunchKernelGGL((scene_kernel<CPLX, 6>), dim3(grid), dim3(kScBlock), 0, stream, a); break;
    case 7: hipLaunchKernelGGL((scene_kernel<CPLX, 7>), dim3(grid), dim3(kScBlock), 0, stream, a); break;
    default: hipLaunchKernelGGL((scene_kernel<CPLX, 8>), dim3(grid), dim3(kScBlock), 0, stream, a); break;
  }
}

// floor(v 2^64) of |v| <= 1 as a signed integer mod 2^64 (the scaling is exact)
unsigned long long scene_ramp_step(double v) {
  const double w = std::floor(std::ldexp(v, 64));
  if (std::fabs(w) >= 18446744073709551616.0) return 0ull;          // v = +-1: a whole turn
  return w >= 0.0 ? (unsigned long long)w : 0ull - (unsigned long long)(-w);
}

// every check of a call but the one that needs the chip generator (an unknown PRN); the code lengths and symbol words of the satellites
int scene_check(const gacq_sim_sat* sats, int K, const gacq_scene_emitter* emitters, int I, const double* gains, double fs, double sigma,
                long long first_antenna, int M, long long j0, long long n, int out_complex64, void* const* d_out, std::vector<int>& Ls,
                size_t& symwords) {
  const char* who = "gacq_scene";
  if (K < 0 || K > kSimMaxK) return set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: need 0 <= K <= %d satellites (K %d)", who, kSimMaxK, K);
  if (I < 0 || I > kScMaxI) return set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: need 0 <= I <= %d emitters (I %d)", who, kScMaxI, I);
  if (M < 1 || M > kScMaxM || first_antenna < 0 || first_antenna > (1ll << 31) - M)
    return set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: need 1 <= M <= %d antennas from first_antenna in 0 .. 2^31 - M (M %d, first %lld)", who, kScMaxM, M,
                     first_antenna);
  if ((K > 0 && !sats) || (I > 0 && !emitters) || (K + I > 0 && !gains) || !d_out) return set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: NULL argument", who);
  int rc = sim_check_call(nullptr, who, fs, sigma, j0, n);
  if (rc < 0) return rc;
  for (int p = 0; p < M; p++) {
    if (!d_out[p]) return set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: the output pointer of antenna %d is NULL", who, p);
    if (out_complex64 && (uintptr_t)d_out[p] % 8u) return set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: complex64 output %d must be 8-byte aligned", who, p);
  }
  if ((rc = sim_check_sats(nullptr, who, sats, K, fs, Ls, symwords)) < 0) return rc;
  for (int i = 0; i < I; i++) {
    const gacq_scene_emitter& e = emitters[i];
    if (e.kind < 0 || e.kind > 3) return set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: emitter %d: kind %d outside 0..3", who, i, e.kind);
    if (!std::isfinite(e.amp) || !std::isfinite(e.f0_hz) || !std::isfinite(e.f1_hz) || !std::isfinite(e.phase))
      return set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: emitter %d: a parameter is not finite", who, i);
    if (e.kind == 1 || e.kind == 2) {
      if (e.sweep < 2 || e.sweep > kScMaxSweep || (e.kind == 2 && (e.sweep & 1)))
        return set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: emitter %d: need a sweep of 2 .. 2^31 samples, even for a triangle (%lld)", who, i, e.sweep);
      if (!(std::fabs(e.f1_hz - e.f0_hz) <= fs))
        return set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: emitter %d: need |f1 - f0| <= fs (%g, %g)", who, i, e.f0_hz, e.f1_hz);
    }
    if (e.gate_period < 0 || e.gate_period > kSimMaxJ ||
        (e.gate_period > 0 && (e.gate_first < 0 || e.gate_first >= e.gate_period || e.gate_on < 1 || e.gate_on > e.gate_period)))
      return set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: emitter %d: need gate_period 0, or 0 <= gate_first < gate_period <= 2^48 and 1 <= gate_on <= gate_period",
                       who, i);
  }
  for (int q = 0; q < 2 * M * (K + I); q++)
    if (!std::isfinite(gains[q]) || !std::isfinite((float)gains[q]))
      return set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: gain %d of antenna %d is not finite in fp32", who, (q / 2) % (K + I), q / (2 * (K + I)));
  return GACQ_OK;
}

}  // namespace

extern "C" int gacq_scene_check(const gacq_sim_sat* sats, int K, const gacq_scene_emitter* emitters, int I, const double* gains, double fs,
                                double sigma, long long first_antenna, int M, long long j0, long long n, int out_complex64, void* const* d_out) {
  std::vector<int> Ls;
  size_t symwords = 0;
  return scene_check(sats, K, emitters, I, gains, fs, sigma, first_antenna, M, j0, n, out_complex64, d_out, Ls, symwords);
}

extern "C" int gacq_scene_dev(gacq_ctx* ctx, const gacq_sim_sat* sats, int K, const gacq_scene_emitter* emitters, int I, const double* gains,
                              double fs, double sigma, unsigned long long seed, long long first_antenna, int M, long long j0, long long n,
                              int out_complex64, void* const* d_out) {
  if (!ctx) return GACQ_ERR_BAD_ARG;
  // everything is checked before anything is allocated or launched
  std::vector<int> Ls;
  size_t symwords = 0;
  int rc = scene_check(sats, K, emitters, I, gains, fs, sigma, first_antenna, M, j0, n, out_complex64, d_out, Ls, symwords);
  if (rc < 0) return set_error(ctx, rc, "%s", gacq_last_error(nullptr));
  std::vector<ChipTable> tabs;
  if ((rc = sim_chip_tables(ctx, "gacq_scene_dev", sats, K, Ls, tabs)) < 0) return rc;
  const int E = K + I;
  const size_t o_em = sizeof(SimSat) * (size_t)K, o_gain = o_em + sizeof(SceneEm) * (size_t)I, o_out = o_gain + sizeof(float2) * (size_t)E * M,
               o_sym = o_out + sizeof(SceneRows);
  const size_t bytes = o_sym + sizeof(unsigned) * symwords;
  GACQ_DEVICE(ctx);
  hipStream_t stream = ctx->stream;
  std::vector<const uint8_t*> d_chips(K);
  for (int k = 0; k < K; k++)
    if ((rc = chip_table_dev(ctx, tabs[k], &d_chips[k])) != GACQ_OK) return rc;
  // the parameter block goes through the two pinned slots gacq_simulate_dev stages its own in, by the same rule: a slot is rewritten
  // only after the launch that last used it has finished (its event)
  const int slot = ctx->sim_slot;
  if (ctx->sim_done[slot]) GACQ_HIP(ctx, hipEventSynchronize(ctx->sim_done[slot]));
  else GACQ_HIP(ctx, hipEventCreateWithFlags(&ctx->sim_done[slot], hipEventDisableTiming));
  DevBuf& d_par = ctx->tables[slot ? "simulate:params1" : "simulate:params0"];
  if ((rc = ensure_pinned(ctx, ctx->pin_sim[slot], bytes)) != GACQ_OK) return rc;
  if ((rc = ensure(ctx, d_par, bytes)) != GACQ_OK) return rc;
  unsigned char* host = (unsigned char*)ctx->pin_sim[slot].p;
  const unsigned char* dev = (const unsigned char*)d_par.p;
  sim_fill_sats(sats, K, Ls, d_chips, fs, j0, (SimSat*)host, (unsigned*)(host + o_sym), (const unsigned*)(dev + o_sym));
  SceneEm* hem = (SceneEm*)(host + o_em);
  for (int i = 0; i < I; i++) {
    const gacq_scene_emitter& e = emitters[i];
    SceneEm& t = hem[i];
    std::memset(&t, 0, sizeof(t));
    t.kind = (unsigned)e.kind;
    t.amp = (float)e.amp;
    t.gper = (unsigned long long)e.gate_period;
    t.gon = e.gate_period ? (unsigned long long)e.gate_on : ~0ull;
    if (e.gate_period) t.g0 = (unsigned long long)((((j0 - e.gate_first) % e.gate_period) + e.gate_period) % e.gate_period);
    if (e.kind == 3) continue;
    t.F0 = turn_fraction(e.f0_hz / fs);
    const unsigned long long p0 = turn_fraction(e.phase);
    if (e.kind == 0) {
      t.th0 = p0 + (unsigned long long)j0 * t.F0;
      continue;
    }
    const unsigned long long P = (unsigned long long)e.sweep, H = e.kind == 2 ? P / 2 : P;
    t.R = scene_ramp_step((e.f1_hz - e.f0_hz) / fs / (double)H);
    t.P = (unsigned)P;                                              // 2^31 fits
    t.H = (unsigned)H;
    const unsigned long long TP = e.kind == 2 ? H * (H - 1ull) : (P * (P - 1ull)) >> 1;
    t.Phi = P * t.F0 + t.R * TP;
    t.u0 = (unsigned)((unsigned long long)j0 % P);
    t.th0 = p0 + ((unsigned long long)j0 / P) * t.Phi;
  }
  float2* hg = (float2*)(host + o_gain);
  for (int e = 0; e < E; e++)
    for (int p = 0; p < M; p++) hg[(size_t)e * M + p] = make_float2((float)gains[2 * ((size_t)p * E + e)], (float)gains[2 * ((size_t)p * E + e) + 1]);
  SceneRows* hr = (SceneRows*)(host + o_out);
  for (int p = 0; p < kScMaxM; p++) hr->out[p] = d_out[p < M ? p : 0];
  hr->a0 = (unsigned)first_antenna;
  hr->pad = 0u;
  // from here on the slot's pinned block may be in use by a queued copy: the event is recorded on every way out, failures included
  hipError_t err = hipMemcpyAsync(d_par.p, host, bytes, hipMemcpyHostToDevice, stream);
  if (err != hipSuccess) {
    (void)hipEventRecord(ctx->sim_done[slot], stream);
    return set_error(ctx, GACQ_ERR_HIP, "gacq_scene_dev: parameter upload failed: %s", hipGetErrorString(err));
  }
  SceneArgs a;
  a.sats = (const SimSat*)dev;
  a.ems = (const SceneEm*)(dev + o_em);
  a.gains = (const float2*)(dev + o_gain);
  a.rows = (const SceneRows*)(dev + o_out);
  a.j0 = j0;
  a.n = n;
  a.seed = seed;
  a.sigma = (float)sigma;
  a.K = K;
  a.I = I;
  const int run = scene_run(M);
  const long long nblk = ((n + run - 1) / run + kScBlock - 1) / kScBlock;
  const unsigned grid = (unsigned)std::min<long long>(nblk, (long long)kScMaxGrid);
  if (out_complex64) scene_launch<true>(M, grid, stream, a);
  else scene_launch<false>(M, grid, stream, a);
  err = hipGetLastError();
  const hipError_t e2 = hipEventRecord(ctx->sim_done[slot], stream);
  if (err != hipSuccess) return set_error(ctx, GACQ_ERR_HIP, "gacq_scene_dev: launch failed: %s", hipGetErrorString(err));
  GACQ_HIP(ctx, e2);
  ctx->sim_slot = slot ^ 1;
  return GACQ_OK;
}
