// What the antenna-array kernels share (gacq_null.hip, gacq_stap.hip, gacq_beams.hip): the bounds and the launch constants, the 16-byte load at any
// address, the weight quantiser, the byte selects of a covariance fragment and the output epilogue of the apply kernels.  Both files
// begin with `#pragma clang fp contract(off)` ahead of every include, and this header relies on it: what is here keeps the operations,
// and so the bits and the instructions, it had when each file held its own copy.
// The epilogue is two macros, not a function template: a forced-inline function is simplified on its own before it is inlined, and
// with it all eighteen apply kernels came out with other instructions (block order, registers; profiles/arraynull_refactor.log).  The
// macros hand the compiler the text the kernels had, so every kernel keeps its instruction stream.
#pragma once

#include "gacq_common.h"

#include <cmath>

namespace gacq {

// null_cov_kernel, which lives in gacq_null.hip alone, launched for another file of the library: C_b of the nblk blocks of Lb samples
// that begin at in[p] (kArMaxM device pointers, the slots from M up any valid one), into C [block][8][8][2]
void null_launch_cov(const uint8_t* const* in, int* C, long long nblk, int Lb, int M, hipStream_t stream);

}  // namespace gacq

namespace {

constexpr int kArBlock = 256;                        // threads a workgroup
constexpr int kArMaxM = 8, kArMaxWindow = 64, kArMaxLb = 32768, kArMaxShift = 40;
constexpr int kArMaxBeams = 16;                      // outputs of one gacq_beams call
constexpr long long kArMaxChunk = 1ll << 14;         // blocks whose outputs one triple of launches writes, at most (2^29 samples)
constexpr int kArRuns = 8;                           // runs a lane works through
constexpr int kArTile = kArBlock * kArRuns * 8;      // 16384 samples a workgroup
constexpr unsigned kArMaxGrid = 1u << 16;            // workgroups; a longer call loops
constexpr int kArWq = 1 << 14;                       // weight scale 2^14
constexpr int kArWqMax = 131071;
constexpr unsigned kArSelI = 0x06040200u, kArSelQ = 0x07050301u;      // bytes 0, 2 (I) or 1, 3 (Q) of two dwords

typedef int ar_v4i __attribute__((ext_vector_type(4)));

// 16 bytes at any address: a byte-aligned copy, for which the compiler emits one wide load
__device__ __forceinline__ uint4 ar_load16(const uint8_t* p) {
  uint4 v;
  __builtin_memcpy(&v, p, 16);
  return v;
}

__device__ __forceinline__ int ar_quantise(double w) {
  const double s = w * (double)kArWq;
  if (!__builtin_isfinite(s)) return 0;
  return (int)fmin(fmax(rint(s), -(double)kArWqMax), (double)kArWqMax);
}

// The end of a lane's run in an apply kernel<F32>: the 8 samples yr + i yi from sample j on, scaled by s, as complex64 or as int8 pairs
// clip(rintf(.), -127, 127) -- whole where `full`, else the samples j + e in j0 .. j_end - 1 one by one.  `out` is the address of output
// sample j0; a sample outside the range arrives as 0 and clips nothing; nclip counts the components the clip changed.  The indices
// keep the kernel's own type: absolute and 64-bit in null_apply_kernel, relative and 32-bit in stap_apply_kernel, whose j0 is 0.
#define AR_STORE_RUN(F32, yr, yi, s, out, full, j, j0, j_end, nclip)                                                                   \
  if constexpr (F32) {                                                                                                                 \
    float o[16];                                                                                                                       \
    _Pragma("unroll") for (int e = 0; e < 8; e++) {                                                                                    \
      o[2 * e] = (float)yr[e] * (s);                                                                                                   \
      o[2 * e + 1] = (float)yi[e] * (s);                                                                                               \
    }                                                                                                                                  \
    float* po = reinterpret_cast<float*>(out) + (j - (j0)) * 2;                                                                        \
    if (full) {                                                                                                                        \
      __builtin_memcpy(reinterpret_cast<uint8_t*>(po), o, 64); /* four 16-byte stores; the output lies on 8 bytes */                   \
    } else {                                                                                                                           \
      _Pragma("unroll") for (int e = 0; e < 8; e++)                                                                                    \
        if (j + e >= (j0) && j + e < (j_end)) *reinterpret_cast<float2*>(po + 2 * e) = make_float2(o[2 * e], o[2 * e + 1]);            \
    }                                                                                                                                  \
  } else {                                                                                                                             \
    unsigned q[4] = {0u, 0u, 0u, 0u};                                                                                                  \
    _Pragma("unroll") for (int e = 0; e < 16; e++) {                                                                                   \
      const float v = (float)((e & 1) ? yi[e >> 1] : yr[e >> 1]) * (s);                                                                \
      const float rv = rintf(v); /* half to even */                                                                                    \
      const float cv = fminf(fmaxf(rv, -127.0f), 127.0f);                                                                              \
      nclip += cv != rv ? 1u : 0u;                                                                                                     \
      q[e >> 2] |= ((unsigned)(int)cv & 0xffu) << (8 * (e & 3));                                                                       \
    }                                                                                                                                  \
    uint8_t* po = (out) + (j - (j0)) * 2;                                                                                              \
    if (full) {                                                                                                                        \
      __builtin_memcpy(po, q, 16);                                                                                                     \
    } else {                                                                                                                           \
      _Pragma("unroll") for (int e = 0; e < 16; e++)                                                                                   \
        if (j + (e >> 1) >= (j0) && j + (e >> 1) < (j_end)) po[e] = (uint8_t)(q[e >> 2] >> (8 * (e & 3)));                             \
    }                                                                                                                                  \
  }

// the end of an apply kernel<F32>: the wave's clipped components onto stats[0], the launch's owned blocks onto stats[1]
#define AR_ADD_STATS(F32, stats, nclip, owned, tid)                                                                                    \
  if (stats) {                                                                                                                         \
    if (!F32) {                                                                                                                        \
      for (int off = 1; off < 64; off <<= 1) nclip += __shfl_xor(nclip, off, 64);                                                      \
      if ((tid & 63) == 0 && nclip) atomicAdd(stats, (unsigned long long)nclip);                                                       \
    }                                                                                                                                  \
    if (blockIdx.x == 0 && tid == 0 && owned) atomicAdd(stats + 1, owned);                                                             \
  }

}  // namespace
