// What the antenna-array kernels share (gacq_null.hip, gacq_stap.hip, gacq_beams.hip, gacq_bearing.hip): the bounds and the launch
// constants, the weight quantiser, the byte selects of a covariance fragment, the output epilogue of the apply kernels and the front
// of the weights kernels in the lane layout 8 r + c -- window sum, diagonal loading, Gaussian elimination (null_weights_kernel,
// beams_weights_kernel; bearing_factor_kernel takes the loading and the elimination).  "Output k of beams is what nulling writes" and
// "bearing factors the matrix nulling solves" hold because these are one definition.  stap_weights_kernel keeps its matrix in LDS,
// four threads to a row, and shares none of it.  The 16-byte load at any address is gacq_common.h's load16_any.
// Every file begins with `#pragma clang fp contract(off)` ahead of every include, and this header relies on it: what is here keeps
// the operations, and so the bits, it had when each file held its own copy.
// The epilogue is two macros, not a function template: a forced-inline function is simplified on its own before it is inlined, and
// with it all eighteen apply kernels came out with other instructions (block order, registers; profiles/arraynull_refactor.log).  The
// macros hand the compiler the text the kernels had, so every apply kernel keeps its instruction stream.  The weights front is plain
// functions: the three kernels that call them come out with the same operations in other registers and another block order, no
// scratch and no more VGPRs (profiles/array_turn_refactor.log).
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

__device__ __forceinline__ int ar_quantise(double w) {
  const double s = w * (double)kArWq;
  if (!__builtin_isfinite(s)) return 0;
  return (int)fmin(fmax(rint(s), -(double)kArWqMax), (double)kArWqMax);
}

// ---- The front of a weights kernel: a wave per block, lane 8 r + c holds entry [r][c] of the 8 x 8 matrix.

// the window sum: the lane's entry of W block covariances, pc at the first, 128 ints from one block to the next
__device__ __forceinline__ void ar_window_sum(const int* pc, int W, long long& Rre, long long& Rim) {
  Rre = 0, Rim = 0;
  for (int j = 0; j < W; j++) {
    const int2 v = *reinterpret_cast<const int2*>(pc + 128 * (long long)j);
    Rre += v.x;
    Rim += v.y;
  }
}

// the loading: A = R + d I with d = (trace R >> shift) + 1, as doubles; the entries outside M x M are 0
__device__ __forceinline__ void ar_load_diagonal(long long Rre, long long Rim, int shift, int M, int r, int c, double& Are, double& Aim) {
  const bool in = r < M && c < M;
  long long t = 0;
  for (int p = 0; p < M; p++) t += __shfl(Rre, 9 * p, 64);
  const long long d = (t >> shift) + 1;
  Are = in ? (double)(Rre + (r == c ? d : 0)) : 0.0;
  Aim = in ? (double)Rim : 0.0;
}

// Gaussian elimination without pivoting: A[r][c] -= m A[k][c] for r > k, c > k, with m = A[r][k] / piv_k, the pivot row, the pivot
// and the multiplier's numerator fetched from their lanes.  A lane below the diagonal is left with A[r][c] as step c found it, the
// numerator of its multiplier.  With RHS the right-hand side rides along, b[r] in every lane of row r: b[r] -= m b[k].
template <bool RHS>
__device__ __forceinline__ void ar_eliminate(double& Are, double& Aim, double& bre, double& bim, int M, int r, int c) {
  for (int k = 0; k < M; k++) {
    const double piv = __shfl(Are, 9 * k, 64);
    const double lre = __shfl(Are, 8 * r + k, 64), lim = __shfl(Aim, 8 * r + k, 64);
    const double ure = __shfl(Are, 8 * k + c, 64), uim = __shfl(Aim, 8 * k + c, 64);
    double kre = 0.0, kim = 0.0;
    if constexpr (RHS) kre = __shfl(bre, 8 * k, 64), kim = __shfl(bim, 8 * k, 64);
    if (r > k && r < M) {
      const double mre = lre / piv, mim = lim / piv;
      if (c > k && c < M) {
        Are = Are - (mre * ure - mim * uim);
        Aim = Aim - (mre * uim + mim * ure);
      }
      if constexpr (RHS) {
        bre = bre - (mre * kre - mim * kim);
        bim = bim - (mre * kim + mim * kre);
      }
    }
  }
}
__device__ __forceinline__ void ar_eliminate(double& Are, double& Aim, int M, int r, int c) {
  double none = 0.0;
  ar_eliminate<false>(Are, Aim, none, none, M, r, c);
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
