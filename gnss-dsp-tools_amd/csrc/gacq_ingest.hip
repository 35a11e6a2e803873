// Recording ingest (gacq_ingest_dev, include/gacq.h): packed 1 / 2 / 4-bit, 8-bit signed or unsigned, 16-bit and float32 recordings,
// I/Q or real IF, to the interleaved int8 I/Q (or complex64) every tool downstream takes.  Output sample m is an exact function of
// (format, gain, absolute sample index m): integer arithmetic and one fp32 multiply per component, so the bytes do not depend on how a
// caller cuts the recording into calls.
//
// Both kernels read the input as a stream of values: value t sits at bit t * (bits per value) from d_in.  load16 hands a lane 16
// consecutive values from any value index -- one wide load when the lane's bytes are all present and naturally aligned (16 B for
// s8 / u8, 2 x 16 B for s16, 4 x 16 B for f32, 2 / 4 / 8 B for 1 / 2 / 4-bit codes), byte loads guarded one by one otherwise (a
// misaligned d_in, the edges of the recording); a value that is not present reads as 0.  Packed codes: the host hands over the LUT with
// its index bits reversed when the first code of a byte is in its top bits; the device then reverses the bits of every byte and both
// orders extract with the same constant shifts.  The LUT travels as two 64-bit kernel arguments and is indexed by a shift.
//
// I/Q: a lane owns kRun = 8 consecutive output samples, 16 values: u(m) = v[2m] + i v[2m + 1].
// Real IF: fs/4 down-shift, 47-tap half-band low-pass, decimation by two, in integers:
//     acc(m) = sum_{k = -21..21} g[k] x[2m - k] (-i)^(2m - k),      u(m) = acc(m) 2^-14,       x[n] = 0 for n < 0.
//   g[even k != 0] = 0 leaves Re acc = (-1)^m 2^14 x[2m]; for odd k, (-i)^(2m - k) = (-1)^m i^k with i^k = +i (k = 1 mod 4) or -i
//   (k = 3 mod 4), and i^-k = -i^k, so Im acc = (-1)^m sum_{k odd > 0} g[k] s(k) (x[2m - k] - x[2m + k]); g[k] s(k) is positive for
//   every odd k (GACQ_INGEST_TAPS).  |acc| <= 128 * 53736 < 2^23: exact in int32 and in fp32.
//   A workgroup owns kTile = 2048 outputs: it unpacks inputs 2 M0 - 32 .. 2 M0 + 4127 (M0 its first output; the 43-sample supports
//   reach from 2 M0 - 21 to 2 M0 + 4115) into LDS as int8, 16 values per lane and store (ds_write_b128, conflict-free); a lane then
//   reads the 80 bytes around its outputs with five ds_read_b128 (consecutive lanes 16 bytes apart: conflict-free), keeps the 29 odd-
//   index inputs of its 8 outputs in registers and forms each output with 11 subtractions and 11 multiply-adds.  The LDS image is
//   aligned to the output index, so with out_first a multiple of 8 and d_in + (2 out_first - in_first) 16-byte aligned the fill is one
//   16-byte load per lane.
// The int8 output is rint / clamp of the very fp32 values the complex64 output stores (NaN, which only f32 input can bring, gives 0).
#pragma clang fp contract(off)

#include "gacq_common.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace gacq;

namespace {

constexpr int kIngBlock = 256;
constexpr int kRun = 8;                          // output samples per lane: one 16-byte store of int8 I/Q
constexpr int kTile = kIngBlock * kRun;          // real mode: outputs per workgroup and pass
constexpr int kLead = 32;                        // real mode: LDS slot 0 holds input 2 M0 - kLead (>= 21, a multiple of 16)
constexpr int kLdsVals = 2 * kTile + 64;         // 4160 >= kLead + 2 (kTile - 1) + 21 + 1, a multiple of 16; the last lane reads up to 4159
constexpr unsigned kIngMaxGrid = 1u << 16;       // workgroups; a longer call loops

constexpr int kCentre = 16384;                   // g[0]
// g[k] s(k), k = 1, 3, .., 21: the odd taps of the Hann-windowed sinc (include/gacq.h has g) times the sign of i^k
#define GACQ_INGEST_TAPS {10382, 3333, 1852, 1175, 774, 506, 320, 188, 97, 40, 9}

enum Kind { kS8 = 0, kU8 = 1, kS16 = 2, kF32 = 3, kP1 = 4, kP2 = 5, kP4 = 6 };

template <int KIND> struct KindInfo {
  static constexpr bool packed = KIND >= kP1;
  static constexpr int bits = KIND == kP1 ? 1 : KIND == kP2 ? 2 : KIND == kP4 ? 4 : KIND == kS16 ? 16 : KIND == kF32 ? 32 : 8;
  static constexpr int wide_bytes = 2 * bits;                        // the 16 values of a lane
};

struct IngArgs {
  const uint8_t* in;
  void* out;
  long long t0;                 // value index of I of output 0 (I/Q), of LDS slot 0 of the first tile (real); may be negative
  long long nvals;              // values present at `in`
  long long nbytes;             // bytes present at `in`
  long long n_out;
  unsigned long long lut_lo, lut_hi;
  // packed codes, int8 output of the I/Q kernel: the output byte of every code, clip(rint(float(lut[code]) * gain)), as I and as Q
  // (conj negates before the multiply) -- the same operations on the same values as the complex64 path and store_run, evaluated
  // once on the host instead of once per value
  unsigned long long ibyte_lo, ibyte_hi, qbyte_lo, qbyte_hi;
  float gain;
  int conj;
  int brev;                     // packed: the first code of a byte is in its top bits
  int odd0;                     // real: parity of out_first
  int out_aligned;              // out is 16-byte aligned
};

// entry `code` of a 16-byte table held in two 64-bit words
template <int BITS>
__device__ __forceinline__ unsigned table_at(unsigned long long lo, unsigned long long hi, unsigned code) {
  if (BITS <= 2) return ((unsigned)lo >> (8u * code)) & 0xffu;       // four entries at the most
  return (unsigned)((code < 8u ? lo : hi) >> (8u * (code & 7u))) & 0xffu;
}

template <int BITS>
__device__ __forceinline__ int lut_at(const IngArgs& a, unsigned code) {
  return (int)(signed char)(unsigned char)table_at<BITS>(a.lut_lo, a.lut_hi, code);
}

// packed codes t .. t + 15 of the stream at a.in: code i in bits [b i, b i + b) of the result, bit-reversed when a.brev; bytes that are
// not present read as 0
template <int KIND>
__device__ __forceinline__ unsigned long long codes16(const IngArgs& a, long long t, bool inside) {
  using K = KindInfo<KIND>;
  constexpr int b = K::bits;
  const long long q = t * b;
  const long long byte0 = q >> 3;                                     // floor, also for t < 0
  const unsigned sh = (unsigned)q & 7u;
  const uint8_t* p = a.in + byte0;
  unsigned long long w = 0ull;
  if (inside && sh == 0u && ((uintptr_t)p % (unsigned)K::wide_bytes) == 0u) {
    if (b == 1) w = *reinterpret_cast<const uint16_t*>(p);
    else if (b == 2) w = *reinterpret_cast<const uint32_t*>(p);
    else w = *reinterpret_cast<const unsigned long long*>(p);
  } else {
    constexpr int nb = b == 4 ? 8 : 2 * b + 1;                        // 16 b + sh bits; sh = 0 for b = 4 (t is even)
#pragma unroll
    for (int i = 0; i < nb; i++) {
      const long long at = byte0 + i;
      if (at >= 0 && at < a.nbytes) w |= (unsigned long long)p[i] << (8 * i);
    }
  }
  if (a.brev) w = __brevll(__builtin_bswap64(w));                     // the bits of every byte reversed, the bytes where they were
  return w >> sh;
}

// v[i] = value t + i of the stream at a.in, i < 16; 0 where that value is not present (t + i outside [0, nvals))
template <int KIND, class T>
__device__ __forceinline__ void load16(const IngArgs& a, long long t, T (&v)[16]) {
  using K = KindInfo<KIND>;
  const bool inside = t >= 0 && t + 16 <= a.nvals;
  if constexpr (K::packed) {
    constexpr int b = K::bits;
    const unsigned long long w = codes16<KIND>(a, t, inside);
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const int x = lut_at<b>(a, (unsigned)(w >> (b * i)) & ((1u << b) - 1u));
      v[i] = (T)((inside || (t + i >= 0 && t + i < a.nvals)) ? x : 0);
    }
  } else {
    constexpr int bv = K::bits / 8;                                   // bytes per value
    const uint8_t* p = a.in + t * bv;
    unsigned r[4 * bv];
    if (inside && ((uintptr_t)p % 16u) == 0u) {
#pragma unroll
      for (int i = 0; i < bv; i++) {
        const uint4 w = reinterpret_cast<const uint4*>(p)[i];
        r[4 * i] = w.x;
        r[4 * i + 1] = w.y;
        r[4 * i + 2] = w.z;
        r[4 * i + 3] = w.w;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4 * bv; i++) r[i] = 0u;
#pragma unroll
      for (int i = 0; i < 16; i++)
        if (inside || (t + i >= 0 && t + i < a.nvals)) {
#pragma unroll
          for (int k = 0; k < bv; k++) r[(i * bv + k) >> 2] |= (unsigned)p[i * bv + k] << (8 * ((i * bv + k) & 3));
        }
    }
#pragma unroll
    for (int i = 0; i < 16; i++) {
      if constexpr (KIND == kF32) {
        v[i] = (T)__uint_as_float(r[i]);
      } else if constexpr (KIND == kS16) {
        v[i] = (T)(short)(unsigned short)(r[i >> 1] >> (16 * (i & 1)));
      } else {
        const int x = (int)(signed char)(unsigned char)(r[i >> 2] >> (8 * (i & 3)));
        // u8: byte - 128; a value that is not present stays 0
        v[i] = (T)(KIND == kU8 ? ((inside || (t + i >= 0 && t + i < a.nvals)) ? (x ^ -128) : 0) : x);
      }
    }
  }
}

__host__ __device__ __forceinline__ unsigned to_i8(float x) {
  const float r = fminf(fmaxf(rintf(x), -127.0f), 127.0f);            // rintf: half to even
  return (x != x) ? 0u : ((unsigned)(int)r & 0xffu);
}

// the int8 form of the lane's run: bytes I, Q, I, Q, .. of samples m .. m + kRun - 1, `left` of them inside the call's output
__device__ __forceinline__ void store_bytes(const IngArgs& a, long long m, long long left, const unsigned (&b)[2 * kRun]) {
  uint8_t* __restrict__ o = reinterpret_cast<uint8_t*>(a.out) + 2 * m;
  if (left >= kRun && a.out_aligned) {
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

// the lane's run: samples m .. m + kRun - 1 of the call's output, `left` of them inside it
template <bool CPLX>
__device__ __forceinline__ void store_run(const IngArgs& a, long long m, long long left, const float (&vr)[kRun], const float (&vi)[kRun]) {
  if (CPLX) {
    float2* __restrict__ o = reinterpret_cast<float2*>(a.out) + m;
    if (left >= kRun && a.out_aligned) {
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
      b[2 * i] = to_i8(vr[i]);
      b[2 * i + 1] = to_i8(vi[i]);
    }
    store_bytes(a, m, left, b);
  }
}

// grid-stride over runs of kRun output samples
template <int KIND, bool CPLX>
__global__ __launch_bounds__(kIngBlock) void ingest_iq_kernel(const IngArgs a) {
  const long long nruns = (a.n_out + kRun - 1) / kRun;
  for (long long r = (long long)blockIdx.x * kIngBlock + threadIdx.x; r < nruns; r += (long long)gridDim.x * kIngBlock) {
    const long long m = r * kRun;
    if constexpr (KindInfo<KIND>::packed && !CPLX) {                  // code -> output byte, one table look-up per value
      constexpr int b = KindInfo<KIND>::bits;
      const long long t = a.t0 + 2 * m;
      const unsigned long long w = codes16<KIND>(a, t, t >= 0 && t + 16 <= a.nvals);
      unsigned o[2 * kRun];
#pragma unroll
      for (int i = 0; i < 2 * kRun; i++) {
        const unsigned code = (unsigned)(w >> (b * i)) & ((1u << b) - 1u);
        o[i] = (i & 1) ? table_at<b>(a.qbyte_lo, a.qbyte_hi, code) : table_at<b>(a.ibyte_lo, a.ibyte_hi, code);
      }
      store_bytes(a, m, a.n_out - m, o);
      continue;
    }
    float v[16];
    if constexpr (KIND == kF32) {
      load16<KIND>(a, a.t0 + 2 * m, v);
    } else {
      int x[16];
      load16<KIND>(a, a.t0 + 2 * m, x);
#pragma unroll
      for (int i = 0; i < 16; i++) v[i] = (float)x[i];
    }
    float vr[kRun], vi[kRun];
#pragma unroll
    for (int i = 0; i < kRun; i++) {
      vr[i] = v[2 * i] * a.gain;
      vi[i] = (a.conj ? -v[2 * i + 1] : v[2 * i + 1]) * a.gain;
    }
    store_run<CPLX>(a, m, a.n_out - m, vr, vi);
  }
}

// one tile of kTile outputs per workgroup and pass
template <int KIND, bool CPLX>
__global__ __launch_bounds__(kIngBlock) void ingest_real_kernel(const IngArgs a) {
  __shared__ uint4 lds[kLdsVals / 16];
  constexpr int tap[11] = GACQ_INGEST_TAPS;
  const long long ntiles = (a.n_out + kTile - 1) / kTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long m0 = tile * kTile;                                // offset of the tile's first output from out_first
    for (int c = threadIdx.x; c < kLdsVals / 16; c += kIngBlock) {
      int x[16];
      load16<KIND>(a, a.t0 + 2 * m0 + 16 * c, x);
      uint4 w;
      w.x = (x[0] & 0xff) | ((x[1] & 0xff) << 8) | ((x[2] & 0xff) << 16) | ((unsigned)x[3] << 24);
      w.y = (x[4] & 0xff) | ((x[5] & 0xff) << 8) | ((x[6] & 0xff) << 16) | ((unsigned)x[7] << 24);
      w.z = (x[8] & 0xff) | ((x[9] & 0xff) << 8) | ((x[10] & 0xff) << 16) | ((unsigned)x[11] << 24);
      w.w = (x[12] & 0xff) | ((x[13] & 0xff) << 8) | ((x[14] & 0xff) << 16) | ((unsigned)x[15] << 24);
      lds[c] = w;
    }
    __syncthreads();
    const long long m = m0 + (long long)threadIdx.x * kRun;
    if (m < a.n_out) {
      // slots 16 tid .. 16 tid + 79; output j of the lane has its centre x[2m] at slot 16 tid + kLead + 2 j
      unsigned w[20];
#pragma unroll
      for (int i = 0; i < 5; i++) {
        const uint4 q = lds[threadIdx.x + i];
        w[4 * i] = q.x;
        w[4 * i + 1] = q.y;
        w[4 * i + 2] = q.z;
        w[4 * i + 3] = q.w;
      }
      // odd-index inputs: o[i] = slot kLead - 21 + 2 i, i < 29; output j takes o[j + 10 - t] - o[j + 11 + t] for tap t
      int o[29];
#pragma unroll
      for (int i = 0; i < 29; i++) {
        const int s = kLead - 21 + 2 * i;
        o[i] = (int)(signed char)(unsigned char)(w[s >> 2] >> (8 * (s & 3)));
      }
      float vr[kRun], vi[kRun];
#pragma unroll
      for (int j = 0; j < kRun; j++) {
        const int s = kLead + 2 * j;
        int re = kCentre * (int)(signed char)(unsigned char)(w[s >> 2] >> (8 * (s & 3)));
        int im = 0;
#pragma unroll
        for (int t = 0; t < 11; t++) im += tap[t] * (o[j + 10 - t] - o[j + 11 + t]);
        if ((a.odd0 ^ j) & 1) {                                       // (-1)^m: m = out_first + m0 + 8 tid + j, m0 and 8 tid even
          re = -re;
          im = -im;
        }
        if (a.conj) im = -im;
        vr[j] = ((float)re * 6.103515625e-05f) * a.gain;              // 2^-14: exact
        vi[j] = ((float)im * 6.103515625e-05f) * a.gain;
      }
      store_run<CPLX>(a, m, a.n_out - m, vr, vi);
    }
    __syncthreads();
  }
}

template <int KIND>
void launch(bool real, bool cplx, unsigned grid, hipStream_t stream, const IngArgs& a) {
  if (real) {
    if (KIND == kS16 || KIND == kF32) return;                         // refused before
    constexpr int RK = (KIND == kS16 || KIND == kF32) ? (int)kS8 : KIND;
    if (cplx) hipLaunchKernelGGL((ingest_real_kernel<RK, true>), dim3(grid), dim3(kIngBlock), 0, stream, a);
    else hipLaunchKernelGGL((ingest_real_kernel<RK, false>), dim3(grid), dim3(kIngBlock), 0, stream, a);
  } else {
    if (cplx) hipLaunchKernelGGL((ingest_iq_kernel<KIND, true>), dim3(grid), dim3(kIngBlock), 0, stream, a);
    else hipLaunchKernelGGL((ingest_iq_kernel<KIND, false>), dim3(grid), dim3(kIngBlock), 0, stream, a);
  }
}

}  // namespace

#include "gacq_streamhost.h"

extern "C" int gacq_ingest_dev(gacq_ctx* ctx, const gacq_ingest_fmt* fmt, const void* d_in, long long in_first, long long in_count,
                               long long out_first, long long n_out, double gain, int out_complex64, void* d_out) {
  if (!ctx) return GACQ_ERR_BAD_ARG;
  if (!fmt || !d_in || !d_out) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_ingest_dev: NULL argument");
  // everything is checked before anything is launched
  if (fmt->container < GACQ_INGEST_S8 || fmt->container > GACQ_INGEST_PACKED)
    return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_ingest_dev: unknown container %d", fmt->container);
  const bool packed = fmt->container == GACQ_INGEST_PACKED, real = fmt->real != 0;
  if (packed && fmt->bits != 1 && fmt->bits != 2 && fmt->bits != 4)
    return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_ingest_dev: packed codes have 1, 2 or 4 bits, not %d", fmt->bits);
  if (real && (fmt->container == GACQ_INGEST_S16 || fmt->container == GACQ_INGEST_F32))
    return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_ingest_dev: real mode takes s8, u8 and packed input only");
  const float g = (float)gain;
  int rc = st_check_gain(ctx, "gacq_ingest_dev", "must be finite and positive in fp32", gain);
  if (rc == GACQ_OK) rc = st_check_range(ctx, "gacq_ingest_dev", in_first, in_count, out_first, n_out);
  if (rc < 0) return rc;
  const int vbits = packed ? fmt->bits : fmt->container == GACQ_INGEST_S16 ? 16 : fmt->container == GACQ_INGEST_F32 ? 32 : 8;
  const int vps = real ? 1 : 2;                                       // values per input sample
  if ((in_first * vps * vbits) % 8)
    return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_ingest_dev: in_first %lld is not on a byte boundary (%d bits per sample)", in_first, vps * vbits);
  if ((uintptr_t)d_out % (out_complex64 ? 8u : 1u)) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_ingest_dev: complex64 output must be 8-byte aligned");
  if (n_out == 0) return GACQ_OK;
  // what the outputs need: I/Q sample m; real inputs 2m - 21 .. 2m + 21, those below 0 being zero
  const long long last = out_first + n_out - 1;
  const long long need_lo = real ? std::max(0ll, 2 * out_first - 21) : out_first, need_hi = real ? 2 * last + 21 : last;
  if ((rc = st_check_support(ctx, "gacq_ingest_dev", out_first, n_out, need_lo, need_hi, in_first, in_count)) < 0) return rc;
  IngArgs a;
  a.in = (const uint8_t*)d_in;
  a.out = d_out;
  a.t0 = real ? 2 * out_first - kLead - in_first : 2 * (out_first - in_first);
  a.nvals = in_count * vps;
  a.nbytes = (a.nvals * vbits + 7) / 8;
  a.n_out = n_out;
  // the first code of a byte in its top bits: the device reverses the bits of every byte, so the LUT is indexed by the reversed code
  a.brev = packed && fmt->msb_first;
  uint8_t lut[16];
  for (int c = 0; c < 16; c++) {
    int src = c;
    if (a.brev) {
      src = 0;
      for (int k = 0; k < fmt->bits; k++) src |= ((c >> k) & 1) << (fmt->bits - 1 - k);
    }
    lut[c] = packed && c < (1 << fmt->bits) ? (uint8_t)fmt->lut[src] : 0;
  }
  std::memcpy(&a.lut_lo, lut, 8);
  std::memcpy(&a.lut_hi, lut + 8, 8);
  a.gain = g;
  a.conj = fmt->conj != 0;
  uint8_t ibyte[16], qbyte[16];
  for (int c = 0; c < 16; c++) {
    const float x = (float)(int8_t)lut[c];
    ibyte[c] = (uint8_t)to_i8(x * g);
    qbyte[c] = (uint8_t)to_i8((a.conj ? -x : x) * g);
  }
  std::memcpy(&a.ibyte_lo, ibyte, 8);
  std::memcpy(&a.ibyte_hi, ibyte + 8, 8);
  std::memcpy(&a.qbyte_lo, qbyte, 8);
  std::memcpy(&a.qbyte_hi, qbyte + 8, 8);
  a.odd0 = (int)(out_first & 1);
  a.out_aligned = ((uintptr_t)d_out % 16u) == 0u;
  GACQ_DEVICE(ctx);
  const long long nblk = real ? (n_out + kTile - 1) / kTile : ((n_out + kRun - 1) / kRun + kIngBlock - 1) / kIngBlock;
  const unsigned grid = (unsigned)std::min<long long>(nblk, (long long)kIngMaxGrid);
  const bool cplx = out_complex64 != 0;
  switch (fmt->container) {
    case GACQ_INGEST_S8: launch<kS8>(real, cplx, grid, ctx->stream, a); break;
    case GACQ_INGEST_U8: launch<kU8>(real, cplx, grid, ctx->stream, a); break;
    case GACQ_INGEST_S16: launch<kS16>(real, cplx, grid, ctx->stream, a); break;
    case GACQ_INGEST_F32: launch<kF32>(real, cplx, grid, ctx->stream, a); break;
    default:
      if (fmt->bits == 1) launch<kP1>(real, cplx, grid, ctx->stream, a);
      else if (fmt->bits == 2) launch<kP2>(real, cplx, grid, ctx->stream, a);
      else launch<kP4>(real, cplx, grid, ctx->stream, a);
  }
  return st_launched(ctx, "gacq_ingest_dev");
}
