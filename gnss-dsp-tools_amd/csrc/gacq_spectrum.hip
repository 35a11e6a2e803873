// The reference's two signal-inspection utilities on the GPU:
//   spectrum.py:48-57                                    Welch power spectrum of a raw int8 recording (psd_kernel, psd_finish_kernel)
//   squaring.py:28-40 + gnsstools/squaring.py:14-23      squaring-loop carrier detector (squaring_kernel), with nco.mix_ (nco.py:30-41)
//
// Spectrum.  One workgroup transforms frame after frame in LDS (int8 -> float, Hann window, in-place decimation-in-frequency
// radix-4 passes and one radix-2 pass when log2 n is odd; the result stays in digit-reversed order) and keeps the fp64 power sums
// of its bins in registers.  A spectrum of at most kMinSegFrames frames is finished by the same workgroup.  The frames of a longer one are cut into at most kMaxSegments segments whose length
// depends on ns alone; every segment's sum is written as an fp64 partial, and psd_finish_kernel adds the partials in segment order,
// divides by ns, undoes the digit reversal, shifts and takes 10 log10.  How many workgroups share a spectrum (the `split` argument)
// only decides which workgroup computes which segments: the bits of the output do not depend on it, and nothing is accumulated
// with atomics.
//
// Squaring.  One workgroup per output r[chunk][block]: thread k sums the n mixed samples of boxcar k in fp64, squares, divides by
// n; the m results are added in a fixed tree.  The mixed signal never exists in memory.
#pragma clang fp contract(off)
#include "gacq_common.h"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"      // the loop discriminators of gacq_trackcore.h are not used here
#include "gacq_trackcore.h"
#pragma clang diagnostic pop

#include <cmath>

using namespace gacq;

namespace {

constexpr int kPsdMinLog2 = 6, kPsdMaxLog2 = 14;
constexpr int kMaxSegments = 16;       // partial sums per spectrum
constexpr int kMinSegFrames = 8;       // a segment is at least this long.  A spectrum of one segment (ns <= 8) writes no partial at all; otherwise a
                                       // partial is 8 bytes per bin and segment, written and read once, against 2 bytes per sample: about
                                       // the input's traffic again for 8 < ns < 128, 256 / ns of it from there on (a quarter at ns = 1000)

constexpr int psd_threads(int log2n) { return (1 << log2n) / 4 > 1024 ? 1024 : ((1 << log2n) / 4 < 64 ? 64 : (1 << log2n) / 4); }

__host__ __device__ inline int psd_seg_frames(int ns) {
  const int l = (ns + kMaxSegments - 1) / kMaxSegments;
  return l < kMinSegFrames ? kMinSegFrames : l;
}

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cmul(float2 a, float2 w) {
  return make_float2(__builtin_fmaf(a.x, w.x, -(a.y * w.y)), __builtin_fmaf(a.x, w.y, a.y * w.x));
}

// One decimation-in-frequency radix-4 pass of span s on x[j + {0, q, 2q, 3q}], q = s/4, in place: quarter r of every block receives
// the residue-r outputs times W_s^(r k).  tw[k] = exp(-2 pi i k / N), k < 3N/4.  After the passes (and one radix-2 pass when log2 N is
// odd) position i holds bin psd_bin_of(i): the base-4 digits of i in reverse order, the odd length's last bit on top.
template <int N, int T>
__device__ __forceinline__ void dif_pass4(float2* x, const float2* __restrict__ tw, int s, int tid) {
  const int q = s >> 2, stride = N / s;
  // N >= 8192 holds 8 or 16 fp64 sums per thread across the transform: its butterflies go one at a time, or the sums spill
  constexpr int kUnroll = N / T >= 8 ? 1 : 2;
#pragma unroll kUnroll
  for (int bf = tid; bf < N / 4; bf += T) {
    const int k = bf & (q - 1);
    const int j = ((bf - k) << 2) + k;
    const float2 e0 = x[j], e1 = x[j + q], e2 = x[j + 2 * q], e3 = x[j + 3 * q];
    const float2 w1 = tw[k * stride], w2 = tw[2 * k * stride], w3 = tw[3 * k * stride];
    const float2 t0 = cadd(e0, e2), t1 = csub(e0, e2), t2 = cadd(e1, e3);
    const float2 d = csub(e1, e3);
    const float2 t3 = make_float2(d.y, -d.x);                     // -i (e1 - e3)
    x[j] = cadd(t0, t2);
    x[j + q] = cmul(cadd(t1, t3), w1);
    x[j + 2 * q] = cmul(csub(t0, t2), w2);
    x[j + 3 * q] = cmul(csub(t1, t3), w3);
  }
}

// position of bin k after the passes: swap the bits of every base-4 digit (pairs from bit 0; an odd length's top bit stays), then
// reverse all log2n bits
__device__ __forceinline__ unsigned psd_position_of(unsigned k, int log2n) {
  const unsigned pairs = (1u << (log2n & ~1)) - 1u;
  const unsigned lo = k & pairs;
  const unsigned sw = ((lo & 0x55555555u) << 1) | ((lo & 0xaaaaaaaau) >> 1) | (k & ~pairs);
  return __brev(sw) >> (32 - log2n);
}

// the bin that position i holds: the inverse of psd_position_of
__device__ __forceinline__ unsigned psd_bin_of(unsigned i, int log2n) {
  const unsigned rv = __brev(i) >> (32 - log2n);
  const unsigned pairs = (1u << (log2n & ~1)) - 1u;
  const unsigned lo = rv & pairs;
  return ((lo & 0x55555555u) << 1) | ((lo & 0xaaaaaaaau) >> 1) | (rv & ~pairs);
}

// the dB value of a bin from the fp64 sum over its segments' partials (0.0 + first partial + ...): one expression for both kernels
__device__ __forceinline__ double psd_db(double sum, int ns) { return 10.0 * log10(sum / (double)ns); }

// nseg == 1: out_db[spec][o] directly (psd_finish_kernel's value: 0.0 + the only partial is that partial).  Otherwise
// partial[(spec * nseg + seg) * N + i] = sum over the frames of segment seg of |FFT(frame * window)|^2 at position i (psd_position_of)
template <int LOG2N>
__global__ __launch_bounds__(psd_threads(LOG2N)) void psd_kernel(const int8_t* __restrict__ iq, const float* __restrict__ win,
                                                                  const float2* __restrict__ tw, double* __restrict__ partial,
                                                                  double* __restrict__ out_db, int ns, int nseg, int split) {
  constexpr int N = 1 << LOG2N, T = psd_threads(LOG2N), R = N / T;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float2* x = reinterpret_cast<float2*>(smem);
  const int tid = threadIdx.x;
  const long spec = blockIdx.x / split;
  const int part = blockIdx.x % split;
  const int seg0 = (int)((long)part * nseg / split), seg1 = (int)((long)(part + 1) * nseg / split);
  const int L = psd_seg_frames(ns);
  for (int seg = seg0; seg < seg1; seg++) {
    double acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = 0.0;
    const int f1 = (seg + 1) * L < ns ? (seg + 1) * L : ns;
    for (int f = seg * L; f < f1; f++) {
      // eight samples (16 bytes) per load
      const uint4* src = reinterpret_cast<const uint4*>(iq + ((spec * ns + f) << (LOG2N + 1)));
#pragma unroll 1
      for (int v = tid; v < N / 8; v += T) {
        const uint4 raw = src[v];
        const float4 wa = reinterpret_cast<const float4*>(win)[2 * v], wb = reinterpret_cast<const float4*>(win)[2 * v + 1];
        const unsigned u[4] = {raw.x, raw.y, raw.z, raw.w};
        const float w[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const unsigned h = u[e >> 1] >> ((e & 1) * 16);
          x[8 * v + e] = make_float2((float)(signed char)(h & 0xff) * w[e], (float)(signed char)((h >> 8) & 0xff) * w[e]);
        }
      }
      __syncthreads();
      constexpr int kPassUnroll = T >= 1024 ? 1 : LOG2N / 2;    // 1024 threads (128 registers): one copy of the pass, or the sums spill
#pragma unroll kPassUnroll
      for (int l = LOG2N; l >= 2; l -= 2) {
        dif_pass4<N, T>(x, tw, 1 << l, tid);
        __syncthreads();
      }
      if (LOG2N & 1) {
#pragma unroll 1
        for (int j = tid; j < N / 2; j += T) {
          const float2 a = x[2 * j], b = x[2 * j + 1];
          x[2 * j] = cadd(a, b);
          x[2 * j + 1] = csub(a, b);
        }
        __syncthreads();
      }
#pragma unroll
      for (int r = 0; r < R; r++) {
        const float2 z = x[tid + r * T];
        const double re = (double)z.x, im = (double)z.y;
        acc[r] = acc[r] + (re * re + im * im);
      }
      __syncthreads();
    }
    if (nseg == 1) {
#pragma unroll
      for (int r = 0; r < R; r++) {
        const unsigned o = (psd_bin_of((unsigned)(tid + r * T), LOG2N) + (unsigned)(N >> 1)) & (unsigned)(N - 1);
        out_db[(spec << LOG2N) + o] = psd_db(0.0 + acc[r], ns);
      }
    } else {
      double* out = partial + ((spec * nseg + seg) << LOG2N);
#pragma unroll
      for (int r = 0; r < R; r++) out[tid + r * T] = acc[r];
    }
  }
}

// out[spec][o] = 10 log10(sum_seg partial[spec][seg][position of bin o + N/2 mod N] / ns): segment order, fftshift, dB.  A zero sum gives -inf.
__global__ __launch_bounds__(256) void psd_finish_kernel(const double* __restrict__ partial, double* __restrict__ out, int log2n, int nseg,
                                                          int ns, long total) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const int n = 1 << log2n;
  const long spec = g >> log2n;
  const unsigned o = (unsigned)(g & (n - 1));
  const unsigned k = (o + (unsigned)(n >> 1)) & (unsigned)(n - 1);
  const unsigned i = psd_position_of(k, log2n);
  const double* p = partial + ((spec * nseg) << log2n) + i;
  double s = 0.0;
  for (int seg = 0; seg < nseg; seg++) s = s + p[(long)seg << log2n];
  out[g] = psd_db(s, ns);
}

constexpr int kSqBlock = 128;

// r[blk] = sum_k (sum_l x[(blk*m + k)*n + l] * nco)^2 / n in complex128, the products rounded to complex64 as x[i] *= tab[idx] on a
// c8 array does; y = the script's int16 stream.  WIDE: n is a multiple of 8 and iq is 16-byte aligned, eight samples per load.
template <bool WIDE>
__global__ __launch_bounds__(kSqBlock) void squaring_kernel(const int8_t* __restrict__ iq, const double* __restrict__ phase0, double f,
                                                             const double2* __restrict__ tab, int b, int n, int m, double2* __restrict__ r,
                                                             short* __restrict__ y, unsigned long long* __restrict__ clamped) {
  __shared__ double2 part[kSqBlock];
  const int tid = threadIdx.x;
  const long blk = blockIdx.x;
  const long chunk = blk / b;
  const unsigned long long dp0 = (unsigned long long)nco_fixed(phase0[chunk]);        // nco.py:33
  const unsigned long long df = (unsigned long long)nco_fixed(f);                     // nco.py:34
  const long i0 = (blk - chunk * b) * (long)n * m;                                    // first sample of the block within its chunk
  const int8_t* src = iq + 2 * blk * (long)n * m;
  double accr = 0.0, acci = 0.0;
  for (int k = tid; k < m; k += kSqBlock) {
    double sr = 0.0, si = 0.0;
    const long base = (long)k * n;
    auto one = [&](long l, int vi, int vq) {
      const unsigned long long ph = dp0 + (unsigned long long)(i0 + l) * df;            // dp after i0 + l additions of df, wrapping like int64
      const double2 t = tab[(ph >> 50) & (kNT - 1)];
      const float2 p = mix_c64(make_float2((float)vi, (float)vq), t);
      sr = sr + (double)p.x;
      si = si + (double)p.y;
    };
    if (WIDE) {
      const uint4* v = reinterpret_cast<const uint4*>(src + 2 * base);
      for (int g = 0; g < n / 8; g++) {
        const uint4 raw = v[g];
        const unsigned u[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const unsigned h = u[e >> 1] >> ((e & 1) * 16);
          one(base + 8 * g + e, (signed char)(h & 0xff), (signed char)((h >> 8) & 0xff));
        }
      }
    } else {
      for (int l = 0; l < n; l++) one(base + l, src[2 * (base + l)], src[2 * (base + l) + 1]);
    }
    const double qr = sr * sr - si * si, qi = sr * si + si * sr;                        // s*s
    accr = accr + qr / (double)n;
    acci = acci + qi / (double)n;
  }
  part[tid] = make_double2(accr, acci);
  __syncthreads();
  for (int h = kSqBlock / 2; h > 0; h >>= 1) {
    if (tid < h) part[tid] = make_double2(part[tid].x + part[tid + h].x, part[tid].y + part[tid + h].y);
    __syncthreads();
  }
  if (tid == 0) {
    const double2 s = part[0];
    r[blk] = s;
    const double v[2] = {rint(20.0 * s.x), rint(20.0 * s.y)};                           // np.round: half to even
    unsigned nclamp = 0;
    for (int c = 0; c < 2; c++) {
      double w = v[c];
      if (w > 32767.0) { w = 32767.0; nclamp++; }
      if (w < -32768.0) { w = -32768.0; nclamp++; }
      y[2 * blk + c] = (short)(int)w;
    }
    if (nclamp) atomicAdd(clamped, (unsigned long long)nclamp);
  }
}

template <int LOG2N>
int psd_launch(gacq_ctx* ctx, const int8_t* iq, const float* win, const float2* tw, double* partial, double* out_db, int ns, int nseg,
               int split, size_t nspectra) {
  constexpr unsigned lds = sizeof(float2) << LOG2N;
  if (lds > 64 * 1024)
    GACQ_HIP(ctx, hipFuncSetAttribute((const void*)psd_kernel<LOG2N>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  hipLaunchKernelGGL(psd_kernel<LOG2N>, dim3((unsigned)(nspectra * split)), dim3(psd_threads(LOG2N)), lds, ctx->stream, iq, win, tw, partial,
                     out_db, ns, nseg, split);
  GACQ_HIP(ctx, hipGetLastError());
  return GACQ_OK;
}

}  // namespace

extern "C" {

int gacq_psd_int8_dev(gacq_ctx* ctx, const void* d_iq_int8, size_t nspectra, int n, int ns, const void* d_window, int split, void* d_out_db) {
  int log2n = 0;
  while ((1 << log2n) < n && log2n < 30) log2n++;
  if (n < (1 << kPsdMinLog2) || n > (1 << kPsdMaxLog2) || (1 << log2n) != n)
    return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_psd_int8_dev: n = %d is not a power of two from %d to %d", n, 1 << kPsdMinLog2, 1 << kPsdMaxLog2);
  if (ns < 1 || nspectra == 0) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_psd_int8_dev: no frames (ns = %d, %zu spectra)", ns, nspectra);
  if (split < 0) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_psd_int8_dev: split = %d", split);
  if (!ctx || !d_iq_int8 || !d_window || !d_out_db) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_psd_int8_dev: NULL argument");
  if (((uintptr_t)d_iq_int8 | (uintptr_t)d_window) & 15)
    return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_psd_int8_dev: samples and window must be 16-byte aligned");
  const int nseg = (ns + psd_seg_frames(ns) - 1) / psd_seg_frames(ns);
  if (nspectra * (size_t)nseg >= ((size_t)1 << 27)) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_psd_int8_dev: %zu spectra in one call", nspectra);
  GACQ_DEVICE(ctx);
  // workgroups per spectrum: enough to put two on every CU when there are few spectra, never more than there are segments
  if (split == 0) split = (int)((512 + nspectra - 1) / nspectra);
  if (split > nseg) split = nseg;
  int rc;
  if (nseg > 1 && (rc = ensure(ctx, ctx->partial, sizeof(double) * nspectra * (size_t)nseg * (size_t)n)) != GACQ_OK) return rc;
  const float2* tw = nullptr;
  if ((rc = twiddle_cache(ctx, "psd:tw" + std::to_string(n), n, 3 * n / 4, &tw)) != GACQ_OK) return rc;
  const int8_t* iq = (const int8_t*)d_iq_int8;
  const float* win = (const float*)d_window;
  double* partial = nseg > 1 ? (double*)ctx->partial.p : nullptr;
  double* out = (double*)d_out_db;
  switch (log2n) {
    case 6: rc = psd_launch<6>(ctx, iq, win, tw, partial, out, ns, nseg, split, nspectra); break;
    case 7: rc = psd_launch<7>(ctx, iq, win, tw, partial, out, ns, nseg, split, nspectra); break;
    case 8: rc = psd_launch<8>(ctx, iq, win, tw, partial, out, ns, nseg, split, nspectra); break;
    case 9: rc = psd_launch<9>(ctx, iq, win, tw, partial, out, ns, nseg, split, nspectra); break;
    case 10: rc = psd_launch<10>(ctx, iq, win, tw, partial, out, ns, nseg, split, nspectra); break;
    case 11: rc = psd_launch<11>(ctx, iq, win, tw, partial, out, ns, nseg, split, nspectra); break;
    case 12: rc = psd_launch<12>(ctx, iq, win, tw, partial, out, ns, nseg, split, nspectra); break;
    case 13: rc = psd_launch<13>(ctx, iq, win, tw, partial, out, ns, nseg, split, nspectra); break;
    default: rc = psd_launch<14>(ctx, iq, win, tw, partial, out, ns, nseg, split, nspectra); break;
  }
  if (rc != GACQ_OK || nseg == 1) return rc;
  const long total = (long)nspectra << log2n;
  hipLaunchKernelGGL(psd_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)partial, (double*)d_out_db,
                     log2n, nseg, ns, total);
  GACQ_HIP(ctx, hipGetLastError());
  return GACQ_OK;
}

int gacq_squaring_int8_dev(gacq_ctx* ctx, const void* d_iq_int8, size_t nchunks, size_t chunk, int n, int m, const void* d_phase0, double f,
                           void* d_r, void* d_y, void* d_clamped) {
  if (n < 1 || m < 1 || chunk == 0 || chunk % ((size_t)n * (size_t)m) != 0)
    return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_squaring_int8_dev: a chunk of %zu samples is not a positive multiple of n*m = %d*%d", chunk, n, m);
  if (nchunks == 0) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_squaring_int8_dev: no chunks");
  if (!std::isfinite(f) || !(std::fabs(f) < 7.0)) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_squaring_int8_dev: f = %g cycles per sample", f);
  if (!ctx || !d_iq_int8 || !d_phase0 || !d_r || !d_y || !d_clamped) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_squaring_int8_dev: NULL argument");
  const size_t b = chunk / ((size_t)n * (size_t)m);
  if (b >= ((size_t)1 << 30) || nchunks * b >= ((size_t)1 << 31) || chunk >= ((size_t)1 << 40))
    return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_squaring_int8_dev: %zu chunks of %zu blocks in one call", nchunks, b);
  GACQ_DEVICE(ctx);
  const double2* tab = nullptr;
  int rc;
  if ((rc = nco_table(ctx, &tab)) != GACQ_OK) return rc;
  GACQ_HIP(ctx, hipMemsetAsync(d_clamped, 0, sizeof(unsigned long long), ctx->stream));
  const bool wide = n % 8 == 0 && ((uintptr_t)d_iq_int8 & 15) == 0;
  const dim3 grid((unsigned)(nchunks * b)), block(kSqBlock);
  if (wide)
    hipLaunchKernelGGL(squaring_kernel<true>, grid, block, 0, ctx->stream, (const int8_t*)d_iq_int8, (const double*)d_phase0, f, tab, (int)b, n, m,
                       (double2*)d_r, (short*)d_y, (unsigned long long*)d_clamped);
  else
    hipLaunchKernelGGL(squaring_kernel<false>, grid, block, 0, ctx->stream, (const int8_t*)d_iq_int8, (const double*)d_phase0, f, tab, (int)b, n, m,
                       (double2*)d_r, (short*)d_y, (unsigned long long*)d_clamped);
  GACQ_HIP(ctx, hipGetLastError());
  return GACQ_OK;
}

}  // extern "C"
