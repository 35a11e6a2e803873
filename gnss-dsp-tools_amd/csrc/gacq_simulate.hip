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
// sin / cos of the carrier and of the Box-Muller angle: the fixed-point quarter-turn reduction and polynomials of gacq_turn.h
// (turn_sincos, which gacq_cohfold.hip and the cancel replica call too).  ln u1 is the accurate logf of u1 rounded to fp32 plus the
// first-order term of the rounding, so the radius keeps its relative accuracy where u1 -> 1.
// The int8 output is rint / clamp of the very fp32 values the complex64 output stores: same operations, same order.
// The device form of a satellite, its conversion on the host, Philox and the Box-Muller draw are in gacq_simcore.h, which
// gacq_scene.hip shares.
#pragma clang fp contract(off)

#include "gacq_simcore.h"

using namespace gacq;

namespace {

constexpr int kSimBlock = 256;
constexpr int kRun = 8;                         // samples per lane and pass: one 16-byte store of int8 I/Q
constexpr unsigned kSimMaxGrid = 1u << 16;      // workgroups; a longer call loops

struct SimArgs {
  const SimSat* sats;
  void* out;
  long long j0, n;
  unsigned long long seed;
  float sigma;
  int K;
  int aligned;                                  // out is 16-byte aligned
};

// grid-stride over runs of kRun samples; lane-run r covers samples [r kRun, r kRun + kRun) of the call
template <bool CPLX>
__global__ __launch_bounds__(kSimBlock) void simulate_kernel(const SimArgs a) {
  const long long nruns = (a.n + kRun - 1) / kRun;
  const SimSat* __restrict__ sats = a.sats;
  for (long long r = (long long)blockIdx.x * kSimBlock + threadIdx.x; r < nruns; r += (long long)gridDim.x * kSimBlock) {
    const unsigned long long m = (unsigned long long)r * kRun;      // offset from j0, < 2^48
    float vr[kRun], vi[kRun];
#pragma unroll
    for (int i = 0; i < kRun; i++) simulate_noise(a.seed, (unsigned long long)a.j0 + m + i, 0u, 0u, a.sigma, vr[i], vi[i]);
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
        turn_sincos(th, c, sn);
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

}  // namespace

extern "C" int gacq_simulate_dev(gacq_ctx* ctx, const gacq_sim_sat* sats, int K, double fs, double sigma, unsigned long long seed, long long j0,
                                 long long n, int out_complex64, void* d_out) {
  if (!ctx) return GACQ_ERR_BAD_ARG;
  if (!sats || !d_out) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_simulate_dev: NULL argument");
  // everything is checked before anything is allocated or launched
  if (K < 1 || K > kSimMaxK) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_simulate_dev: need 1 <= K <= %d satellites (K %d)", kSimMaxK, K);
  if (const int rc = sim_check_call(ctx, "gacq_simulate_dev", fs, sigma, j0, n)) return rc;
  if ((uintptr_t)d_out % (out_complex64 ? 8u : 1u)) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_simulate_dev: complex64 output must be 8-byte aligned");
  std::vector<int> Ls;
  size_t symwords = 0;
  int rc = sim_check_sats(ctx, "gacq_simulate_dev", sats, K, fs, Ls, symwords);
  if (rc < 0) return rc;
  std::vector<ChipTable> tabs;
  if ((rc = sim_chip_tables(ctx, "gacq_simulate_dev", sats, K, Ls, tabs)) < 0) return rc;
  const size_t o_sym = sizeof(SimSat) * (size_t)K, bytes = o_sym + sizeof(unsigned) * symwords;
  GACQ_DEVICE(ctx);
  hipStream_t stream = ctx->stream;
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
  sim_fill_sats(sats, K, Ls, d_chips, fs, j0, (SimSat*)host, (unsigned*)(host + o_sym), (const unsigned*)((const unsigned char*)d_par.p + o_sym));
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
