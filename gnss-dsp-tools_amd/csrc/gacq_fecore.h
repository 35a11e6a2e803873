// Device code of the front-end shared by the single-window kernels (gacq_frontend.hip) and the batched ones (gacq_scan.hip): the
// mixer expression, the odd extension, one tile of a filtfilt pass and one resampled output.  Both files inline the same text, so a
// window of a batch gets the bits gacq_frontend_dev writes for it.
#pragma once
#include "gacq_common.h"
#include "gacq_cplx.h"

namespace gacq {

constexpr int kFeBlock = 256;
constexpr int kMaxTaps = 512;

// nco.mix_ for sample i: (I + jQ) * table[((dp + i*df) >> 50) & 1023]   (gnsstools/nco.py:30-41); one expression for every kernel
// that mixes, so that the stand-alone mix kernel and the FIR kernel that mixes while it loads its tile produce the same bits
__device__ __forceinline__ float2 mix_sample(const char2* __restrict__ iq, long i, long long dp, long long df, const float2* __restrict__ tab) {
  const char2 s = iq[i];
  const unsigned long long ph = (unsigned long long)dp + (unsigned long long)i * (unsigned long long)df;   // wraps like int64
  const float2 w = tab[(ph >> 50) & (kNcoTableSize - 1)];
  const float re = (float)(signed char)s.x, im = (float)(signed char)s.y;
  // products and FMAs spelled out: left to fp-contract, the two kernels this is inlined into could fuse different halves
  return make_float2(__builtin_fmaf(re, w.x, -(im * w.y)), __builtin_fmaf(re, w.y, im * w.x));
}

// the mixed input as an indexable source for odd_ext_at (the FIR kernel that reads int8 samples directly)
struct MixedInput {
  const char2* iq;
  long long dp, df;
  const float2* tab;
  __device__ __forceinline__ float2 operator[](long i) const { return mix_sample(iq, i, dp, df, tab); }
};

// value of the odd extension of x (length n, pad p) at extended index j in [0, n + 2p)   (scipy.signal._arraytools.odd_ext)
template <typename Src>
__device__ __forceinline__ float2 odd_ext_at(const Src& x, long n, int p, long j) {
  if (j < p) {
    const float2 e = x[0], v = x[p - j];
    return make_float2(2.f * e.x - v.x, 2.f * e.y - v.y);
  }
  if (j >= n + p) {
    const float2 e = x[n - 1], v = x[2 * (n - 1) - (j - p)];
    return make_float2(2.f * e.x - v.x, 2.f * e.y - v.y);
  }
  return x[j - p];
}

// PASS 1 (forward):  y1[j] = sum_k h[k] * e[j-k],  e = odd extension, e[m<0] := e[0];   j in [0, L), L = n + 2p
// PASS 2 (backward): y2[j] = sum_k h[k] * y1[j+k], y1[m>=L] := y1[L-1];                 j in [p, p+n) -> out[j-p]
// Each thread produces kOut adjacent outputs from a sliding register window: one LDS read feeds kOut taps' worth of
// FMAs.  The tile is stored with one pad element per 32 (phys = i + i/32) so the stride-kOut lane pattern is
// bank-conflict free; the taps are wave-uniform scalar loads.
constexpr int kOut = 4;
constexpr int kTile = kFeBlock * kOut;
__device__ __forceinline__ int phys(int i) { return i + (i >> 5); }

// tile `tile` of one pass, any tap count; s_x: (kTile + ntaps) padded elements of LDS
template <int PASS>
__device__ __forceinline__ void fir_tile(float2* s_x, long tile, const float2* __restrict__ in, float2* __restrict__ out, long n, int p,
                                         const float* __restrict__ taps, int ntaps) {
  const long L = n + 2 * (long)p;
  const long j0 = tile * kTile + (PASS == 1 ? 0 : p);      // first output index of this tile (extended coords)
  const int halo = ntaps - 1;
  // tile of inputs: PASS 1 needs e[j0-halo .. j0+kTile-1], PASS 2 needs y1[j0 .. j0+kTile-1+halo]
  for (int m = threadIdx.x; m < kTile + halo; m += kFeBlock) {
    const long idx = (PASS == 1) ? (j0 - halo + m) : (j0 + m);
    float2 v;
    if (PASS == 1) v = odd_ext_at(in, n, p, idx < 0 ? 0 : (idx >= L ? L - 1 : idx));
    else v = in[idx >= L ? L - 1 : idx];
    s_x[phys(m)] = v;
  }
  __syncthreads();
  const int r = threadIdx.x * kOut;
  float ar[kOut], ai[kOut];
#pragma unroll
  for (int c = 0; c < kOut; c++) { ar[c] = 0.f; ai[c] = 0.f; }
  float2 w[kOut];
  if (PASS == 1) {
    // out_c = sum_k h[k] * s[r + c + halo - k]; window w[c] = s[r + c + halo - k]
#pragma unroll
    for (int c = 0; c < kOut; c++) w[c] = s_x[phys(r + c + halo)];
    for (int k = 0; k < ntaps; k++) {
      const float hk = taps[k];
#pragma unroll
      for (int c = 0; c < kOut; c++) { ar[c] = fmaf(hk, w[c].x, ar[c]); ai[c] = fmaf(hk, w[c].y, ai[c]); }
#pragma unroll
      for (int c = kOut - 1; c > 0; c--) w[c] = w[c - 1];                 // next k: every index moves down by one
      const int nxt = r + halo - (k + 1);
      w[0] = s_x[phys(nxt < 0 ? 0 : nxt)];
    }
  } else {
    // out_c = sum_k h[k] * s[r + c + k]; window w[c] = s[r + c + k]
#pragma unroll
    for (int c = 0; c < kOut; c++) w[c] = s_x[phys(r + c)];
    for (int k = 0; k < ntaps; k++) {
      const float hk = taps[k];
#pragma unroll
      for (int c = 0; c < kOut; c++) { ar[c] = fmaf(hk, w[c].x, ar[c]); ai[c] = fmaf(hk, w[c].y, ai[c]); }
#pragma unroll
      for (int c = 0; c < kOut - 1; c++) w[c] = w[c + 1];
      const int nxt = r + kOut + k;                                        // = r + (kOut-1) + (k+1)
      w[kOut - 1] = s_x[phys(nxt > kTile + halo - 1 ? kTile + halo - 1 : nxt)];
    }
  }
  const long jend = (PASS == 1) ? L : (long)p + n;
#pragma unroll
  for (int c = 0; c < kOut; c++) {
    const long j = j0 + r + c;
    if (j < jend) out[PASS == 1 ? j : j - p] = make_float2(ar[c], ai[c]);
  }
}

// The reference's filter length (161 taps in every acquire script, acquire-gps-l1.py:89) gets its own instantiation: five
// outputs per thread, so that the lane stride of the window reads is odd (5 elements = 10 banks: conflict-free without padding),
// the tap loop fully unrolled so that every LDS read is `ds_read_b64 v, vaddr offset:imm` from one per-thread base address, the
// taps in SGPRs, and the accumulators as (re, im) pairs: one v_pk_fma_f32 per output and tap with the tap broadcast from its SGPR.
// Same products, same summation order (k ascending) as the generic kernel: bit-identical outputs, 2.4 x faster
// (the generic loop spends more instructions on window moves and padded-address arithmetic than on FMAs).
constexpr int kOutF = 5;
constexpr int kTileF = kFeBlock * kOutF;
// Src: const float2* (a buffer), or MixedInput for PASS 1 -- then the carrier wipe-off happens while the tile is loaded and the
// mixed signal never exists in HBM (one launch and 95 MB of traffic per 6 M samples less).
// s_x: kTileF + NTAPS - 1 elements of LDS
template <int PASS, int NTAPS, typename Src>
__device__ __forceinline__ void fir_fixed_tile(v2* s_x, long tile, const Src in, float2* __restrict__ out, long n, int p,
                                               const float* __restrict__ taps) {
  constexpr int halo = NTAPS - 1;
  const long L = n + 2 * (long)p;
  const long j0 = tile * kTileF + (PASS == 1 ? 0 : p);
  for (int m = threadIdx.x; m < kTileF + halo; m += kFeBlock) {
    const long idx = (PASS == 1) ? (j0 - halo + m) : (j0 + m);
    float2 v;
    if (PASS == 1) v = odd_ext_at(in, n, p, idx < 0 ? 0 : (idx >= L ? L - 1 : idx));
    else v = in[idx >= L ? L - 1 : idx];
    s_x[m] = v2{v.x, v.y};
  }
  __syncthreads();
  const v2* base = s_x + threadIdx.x * kOutF;
  v2 acc[kOutF], w[kOutF];
#pragma unroll
  for (int c = 0; c < kOutF; c++) acc[c] = v2{0.f, 0.f};
  // Taps go in chunks of kChunk (a multiple of kOutF, so the rotating window is back in its starting slots at every chunk
  // boundary): inside a chunk everything is unrolled and every LDS offset is an immediate; a fully unrolled 161-tap body made
  // hipcc hoist all 165 LDS reads to the top (256 VGPRs + spills).
  constexpr int kChunk = 4 * kOutF;
  constexpr int kMain = (NTAPS / kChunk) * kChunk;
#define GACQ_FIR_FMA(C, SLOT, HK) acc[C] = v2{fmaf(HK, w[SLOT].x, acc[C].x), fmaf(HK, w[SLOT].y, acc[C].y)}
  if (PASS == 1) {
    // out_c = sum_k h[k] * s[r + c + halo - k]: the window w[c] = s[r + c + halo - k] moves down by one element per tap
#pragma unroll
    for (int c = 0; c < kOutF; c++) w[c] = base[c + halo];
    const v2* bp = base + halo;                                        // s[r + halo - k0]
    for (int k0 = 0; k0 < kMain; k0 += kChunk, bp -= kChunk) {
#pragma unroll
      for (int kk = 0; kk < kChunk; kk++) {
        const float hk = taps[k0 + kk];
#pragma unroll
        for (int c = 0; c < kOutF; c++) GACQ_FIR_FMA(c, (c + kChunk - kk) % kOutF, hk);
        w[(kOutF - 1 + kChunk - kk) % kOutF] = bp[-(kk + 1)];           // s[r + halo - (k+1)] replaces the element output kOutF-1 just used
      }
    }
#pragma unroll
    for (int kk = 0; kk < NTAPS - kMain; kk++) {
      const float hk = taps[kMain + kk];
#pragma unroll
      for (int c = 0; c < kOutF; c++) GACQ_FIR_FMA(c, (c + kChunk - kk) % kOutF, hk);
      if (kk + 1 < NTAPS - kMain) w[(kOutF - 1 + kChunk - kk) % kOutF] = bp[-(kk + 1)];
    }
  } else {
    // out_c = sum_k h[k] * s[r + c + k]: the window w[c] = s[r + c + k] moves up by one element per tap
#pragma unroll
    for (int c = 0; c < kOutF; c++) w[c] = base[c];
    const v2* bp = base + kOutF;                                       // s[r + kOutF + k0]
    for (int k0 = 0; k0 < kMain; k0 += kChunk, bp += kChunk) {
#pragma unroll
      for (int kk = 0; kk < kChunk; kk++) {
        const float hk = taps[k0 + kk];
#pragma unroll
        for (int c = 0; c < kOutF; c++) GACQ_FIR_FMA(c, (c + kk) % kOutF, hk);
        w[kk % kOutF] = bp[kk];                                        // slot of output 0 at tap k now holds s[r + kOutF + k]
      }
    }
#pragma unroll
    for (int kk = 0; kk < NTAPS - kMain; kk++) {
      const float hk = taps[kMain + kk];
#pragma unroll
      for (int c = 0; c < kOutF; c++) GACQ_FIR_FMA(c, (c + kk) % kOutF, hk);
      if (kk + 1 < NTAPS - kMain) w[kk % kOutF] = bp[kk];
    }
  }
#undef GACQ_FIR_FMA
  const long jend = (PASS == 1) ? L : (long)p + n;
#pragma unroll
  for (int c = 0; c < kOutF; c++) {
    const long j = j0 + threadIdx.x * kOutF + c;
    if (j < jend) out[PASS == 1 ? j : j - p] = make_float2(acc[c].x, acc[c].y);
  }
}

// np.interp of y (n samples) at t: clamps to fp[-1] right of the last sample, slope*(x - xp[i]) + fp[i] left of it
__device__ __forceinline__ float2 interp_pair(float2 a, float2 b, double t, long i) {
  const float fr = (float)(t - (double)i);
  return make_float2(fmaf(b.x - a.x, fr, a.x), fmaf(b.y - a.y, fr, a.y));
}

// output k of the resampler: position t_k = step * k in fp64   ((1/fsr)*np.arange(...), acquire-gps-l1.py:94)
__device__ __forceinline__ float2 resample_at(const float2* __restrict__ y, long n, long k, double step) {
  const double t = __dmul_rn(step, (double)k);
  if (t >= (double)(n - 1)) return y[n - 1];
  const long i = (long)floor(t);
  return interp_pair(y[i], y[i + 1], t, i);
}

}  // namespace gacq
