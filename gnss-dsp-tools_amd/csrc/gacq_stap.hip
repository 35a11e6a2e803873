// Space-time adaptive nulling (gacq_stap_*, include/gacq.h): M int8 I/Q recordings on one clock in, one recording out, every antenna
// under T taps.  The N = M T stacked rows z_e(j) = x_p(j + t_c - t), e = p T + t, take the place of gacq_null's M antennas: exact integer
// covariances of the stacked vectors, the same written-out fp64 solve with M replaced by N, an integer apply.  Every output byte is a
// function of (configuration, absolute sample index) alone, and T = 1 computes what gacq_null computes.
//
// Three launches per call (per chunk of blocks), on one stream:
//   stap_cov_kernel      the direct form: the Gram matrix of the 2N real rows (I and Q of every stacked element) in 16-row tiles, upper
//      tile pairs only, one 16 x 16 x 64 int8 matrix instruction per pair and 64 samples.  Lane l builds the fragment of row l & 15 of a
//      tile at samples 16 (l >> 4) .. + 15 of the group: its element's antenna, shifted by t_c - t samples, two 16-byte loads at any
//      address, the I or the Q bytes picked with four byte permutes.  The fragment of the row tile is the A operand, that of the
//      column tile the B operand (lane l holds column l & 15 at the same k): both take their bytes with one pattern, so sample j meets
//      sample j.  A wave owns (block, row tile): it keeps the row tile's fragment and walks the column tiles tu .. nt - 1 with one
//      accumulator each, over the whole block, so no partial tiles meet anywhere.  It writes C[e][f] and, from an off-diagonal tile, the
//      conjugate at C[f][e]: the workspace holds the full matrix.  Samples below index 0 are zeros made in registers; the taps' reach
//      of t_c samples past either end of a block lies inside the input by the support rule.
//   stap_weights_kernel  a workgroup per block.  The window sum in int64, the loading, then A as two fp64 planes in LDS.  Elimination
//      step k: the thread of row r (four threads a row) divides A[r][k] by the pivot and updates its columns of the whole trailing
//      submatrix; step k reads row k and column k only, which it does not write: one rendezvous a step.  Back substitution: the
//      products A[k][q] u[q] of a row are formed by the lanes q, the subtractions run in ascending q.  Every element runs the fp64
//      sequence of tests/stap_oracle.py; which thread runs it does not change a bit.
//   stap_apply_kernel    a lane's run is the 8 samples at a multiple of 8 of the ABSOLUTE sample index; it reads samples j - 8 ..
//      j + 15 of every antenna with three 16-byte loads where all of them are present, sample by sample (absent ones zero) where not,
//      and unpacks them once; the taps are a compile-time count, so every tap reads registers at a fixed offset.  4 N 24-bit
//      multiply-adds a sample, one 16-byte store (int8) or four (complex64).  A workgroup owns the 16384 samples at a multiple of 16384.
#pragma clang fp contract(off)

#include "gacq_common.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace gacq;

namespace {

constexpr int kStBlock = 256;
constexpr int kStMaxM = 8, kStMaxT = 15, kStMaxN = 56, kStMaxWindow = 64, kStMaxLb = 32768, kStMaxShift = 40;
constexpr long long kStMaxChunk = 1ll << 14;         // blocks whose outputs one triple of launches writes, at most
constexpr size_t kStWorkspace = 64u << 20;           // bytes of the handle's workspace, at most
constexpr int kStRuns = 8;                           // runs a lane works through
constexpr int kStTile = kStBlock * kStRuns * 8;      // 16384 samples a workgroup
constexpr unsigned kStMaxGrid = 1u << 16;            // workgroups; a longer call loops
constexpr int kStWq = 1 << 14;                       // weight scale 2^14
constexpr int kStWqMax = 131071;
constexpr int kStMaxTiles = (2 * kStMaxN + 15) / 16; // 7 tiles of 16 real rows
constexpr int kStStride = kStMaxN + 1;               // doubles between the rows of a plane in LDS: odd, so rows fall on different banks

typedef int st_v4i __attribute__((ext_vector_type(4)));

// 16 bytes at any address: a byte-aligned copy, for which the compiler emits one wide load
__device__ __forceinline__ uint4 st_load16(const uint8_t* p) {
  uint4 v;
  __builtin_memcpy(&v, p, 16);
  return v;
}

// ---- block covariances

struct StCovArgs {
  const uint8_t* in[kStMaxM];   // antenna p: the address of the first sample of block 0 of the launch
  int* C;                       // [block][N][N][2]
  long long nblk;
  long long abs0;               // the absolute index of that sample
  int Lb, M, T, N, nt;          // nt: tiles of 16 real rows
};

// The fragment of a lane's row over 16 samples that begin at absolute sample s (the address p): the I or the Q bytes.  Samples below
// 0 do not exist: they are zeros, and nothing below the recording's first byte is read.
__device__ __forceinline__ st_v4i st_fragment(const uint8_t* p, long long s, unsigned sel, bool live) {
  st_v4i f = {0, 0, 0, 0};
  if (live) {
    unsigned w[8];
    if (s >= 0) {
      const uint4 lo = st_load16(p), hi = st_load16(p + 16);
      w[0] = lo.x, w[1] = lo.y, w[2] = lo.z, w[3] = lo.w, w[4] = hi.x, w[5] = hi.y, w[6] = hi.z, w[7] = hi.w;
    } else {
#pragma unroll
      for (int i = 0; i < 8; i++) {
        unsigned v = 0u;
        if (s + 2 * i >= 0) v |= (unsigned)p[4 * i] | ((unsigned)p[4 * i + 1] << 8);
        if (s + 2 * i + 1 >= 0) v |= ((unsigned)p[4 * i + 2] | ((unsigned)p[4 * i + 3] << 8)) << 16;
        w[i] = v;
      }
    }
    f.x = (int)__builtin_amdgcn_perm(w[1], w[0], sel);
    f.y = (int)__builtin_amdgcn_perm(w[3], w[2], sel);
    f.z = (int)__builtin_amdgcn_perm(w[5], w[4], sel);
    f.w = (int)__builtin_amdgcn_perm(w[7], w[6], sel);
  }
  return f;
}

// two workgroups a compute unit at the least, as null_cov_kernel: the accumulators stay in VGPRs
__global__ __launch_bounds__(kStBlock, 2) void stap_cov_kernel(const StCovArgs a) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row = lane & 15, kg = lane >> 4, tc = (a.T - 1) >> 1;
  const unsigned sel = (row & 1) ? 0x07050301u : 0x06040200u;           // bytes 1, 3 (Q) or 0, 2 (I) of two dwords
  const long long units = a.nblk * a.nt, step = (long long)gridDim.x * (kStBlock / 64);
  const int groups = a.Lb >> 6;
  for (long long unit = (long long)blockIdx.x * (kStBlock / 64) + wave; unit < units; unit += step) {
    const long long bl = unit / a.nt;
    const int tu = (int)(unit - bl * a.nt);
    // the lane's row of every tile of the unit: where its samples begin, in the block's coordinates
    const uint8_t* src[kStMaxTiles];
    int shift[kStMaxTiles];
    bool live[kStMaxTiles];
    st_v4i acc[kStMaxTiles];
#pragma unroll
    for (int d = 0; d < kStMaxTiles; d++) {
      const int e = 8 * (tu + d) + (row >> 1);
      live[d] = tu + d < a.nt && e < a.N;
      const int p = live[d] ? e / a.T : 0, t = live[d] ? e - p * a.T : tc;
      const uint8_t* s = a.in[0];
#pragma unroll
      for (int q = 1; q < kStMaxM; q++)
        if (p == q) s = a.in[q];
      shift[d] = 16 * kg + tc - t;
      src[d] = s + (bl * a.Lb + shift[d]) * 2;
      acc[d] = st_v4i{0, 0, 0, 0};
    }
    const long long first = a.abs0 + bl * a.Lb;
    for (int g = 0; g < groups; g++) {
      const st_v4i fu = st_fragment(src[0] + 128 * (long long)g, first + 64 * g + shift[0], sel, live[0]);
      acc[0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fu, fu, acc[0], 0, 0, 0);
#pragma unroll
      for (int d = 1; d < kStMaxTiles; d++) {
        if (tu + d < a.nt) {
          const st_v4i fv = st_fragment(src[d] + 128 * (long long)g, first + 64 * g + shift[d], sel, live[d]);
          acc[d] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fu, fv, acc[d], 0, 0, 0);
        }
      }
    }
    // the lane holds G[16 tu + 4 kg + i][16 (tu + d) + (lane & 15)], i < 4: rows I, Q of elements 8 tu + 2 kg and + 1
    int* Cb = a.C + bl * a.N * a.N * 2;
#pragma unroll
    for (int d = 0; d < kStMaxTiles; d++) {
      if (tu + d < a.nt) {
        const int g[4] = {acc[d].x, acc[d].y, acc[d].z, acc[d].w};
        int n[4];
#pragma unroll
        for (int i = 0; i < 4; i++) n[i] = __shfl_xor(g[i], 1, 64);     // the same rows of the neighbouring column
        const int f = 8 * (tu + d) + (row >> 1);
        if (!(lane & 1) && f < a.N) {
#pragma unroll
          for (int h = 0; h < 2; h++) {
            const int e = 8 * tu + 2 * kg + h;
            if (e < a.N) {
              const int re = g[2 * h] + n[2 * h + 1], im = g[2 * h + 1] - n[2 * h];
              *reinterpret_cast<int2*>(Cb + (e * a.N + f) * 2) = make_int2(re, im);
              if (d) *reinterpret_cast<int2*>(Cb + (f * a.N + e) * 2) = make_int2(re, -im);
            }
          }
        }
      }
    }
  }
}

// ---- weights

struct StWgtArgs {
  const int* C;                 // C[i] is block pb0 + i
  int* Wq;                      // [block][N][2]
  long long* cov;               // d_cov, or NULL
  int* wout;                    // d_weights, or NULL
  double c[2 * kStMaxM];
  long long b_first;            // the absolute index of the launch's block 0
  long long own_first;          // the call's first owned block
  int nblk;
  int p_off;                    // b_first less the block of C[0]
  int warm;                     // blocks b_first + i with i < warm are in the warm-up: their window is C[0 .. W - 1]
  int W, M, T, N, shift;
};

__device__ __forceinline__ int st_quantise(double w) {
  const double s = w * (double)kStWq;
  if (!__builtin_isfinite(s)) return 0;
  return (int)fmin(fmax(rint(s), -(double)kStWqMax), (double)kStWqMax);
}

__global__ __launch_bounds__(kStBlock) void stap_weights_kernel(const StWgtArgs a) {
  __shared__ double Are[kStMaxN * kStStride], Aim[kStMaxN * kStStride];
  __shared__ double bre[kStMaxN], bim[kStMaxN], pre[2][kStMaxN], pim[2][kStMaxN];
  const int tid = threadIdx.x, i = blockIdx.x, N = a.N, tc = (a.T - 1) >> 1;
  const long long b = a.b_first + i;
  const bool owned = b >= a.own_first;
  // ---- the window sum
  const long long nn = (long long)N * N;
  const int* pc = a.C + (long long)(i >= a.warm ? a.p_off + i - a.W : 0) * nn * 2;
  for (int el = tid; el < N * N; el += kStBlock) {
    long long Rre = 0, Rim = 0;
    for (int j = 0; j < a.W; j++) {
      const int2 v = *reinterpret_cast<const int2*>(pc + (j * nn + el) * 2);
      Rre += v.x;
      Rim += v.y;
    }
    if (owned && a.cov) {
      long long* o = a.cov + ((b - a.own_first) * nn + el) * 2;
      o[0] = Rre;
      o[1] = Rim;
    }
    const int r = el / N, c = el - r * N;
    Are[r * kStStride + c] = (double)Rre;                               // exact: below 2^53
    Aim[r * kStStride + c] = (double)Rim;
  }
  // the constraint on the centre taps
  double cre = 0.0, cim = 0.0;
  if (tid < N) {
    const int p = tid / a.T;
    if (tid - p * a.T == tc) {
#pragma unroll
      for (int q = 0; q < kStMaxM; q++)
        if (p == q) cre = a.c[2 * q], cim = a.c[2 * q + 1];
    }
    bre[tid] = cre;
    bim[tid] = cim;
  }
  __syncthreads();
  // ---- the loading
  long long loaded = 0;
  if (tid < N) {
    long long t = 0;
    for (int p = 0; p < N; p++) t += (long long)Are[p * kStStride + p];
    loaded = (long long)Are[tid * kStStride + tid] + (t >> a.shift) + 1;
  }
  __syncthreads();                                                      // every diagonal is read before one is written
  if (tid < N) Are[tid * kStStride + tid] = (double)loaded;
  __syncthreads();
  // ---- elimination: A[r][q] -= m A[k][q], b[r] -= m b[k] with m = A[r][k] / piv, for r > k, over the whole trailing submatrix
  const int r = tid >> 2, cg = tid & 3;
  for (int k = 0; k < N; k++) {
    if (r > k && r < N) {
      const double piv = Are[k * kStStride + k];
      const double mre = Are[r * kStStride + k] / piv, mim = Aim[r * kStStride + k] / piv;
      for (int q = k + 1 + cg; q < N; q += 4) {
        const double ure = Are[k * kStStride + q], uim = Aim[k * kStStride + q];
        Are[r * kStStride + q] = Are[r * kStStride + q] - (mre * ure - mim * uim);
        Aim[r * kStStride + q] = Aim[r * kStStride + q] - (mre * uim + mim * ure);
      }
      if (cg == 0) {
        const double kre = bre[k], kim = bim[k];
        bre[r] = bre[r] - (mre * kre - mim * kim);
        bim[r] = bim[r] - (mre * kim + mim * kre);
      }
    }
    __syncthreads();
  }
  // ---- back substitution: lane q keeps u[q]; the products of row k in pre / pim [k & 1], the subtractions in ascending q
  double ucr = 0.0, uci = 0.0;
  for (int k = N - 1; k >= 0; k--) {
    if (tid > k && tid < N) {
      const double xr = Are[k * kStStride + tid], xi = Aim[k * kStStride + tid];
      pre[k & 1][tid] = xr * ucr - xi * uci;
      pim[k & 1][tid] = xr * uci + xi * ucr;
    }
    __syncthreads();
    if (tid < 64) {
      double sre = bre[k], sim = bim[k];
      for (int q = k + 1; q < N; q++) {
        sre = sre - pre[k & 1][q];
        sim = sim - pim[k & 1][q];
      }
      const double piv = Are[k * kStStride + k];
      const double xr = sre / piv, xi = sim / piv;
      if (tid == k) ucr = xr, uci = xi;
    }
  }
  // ---- the constraint's scale: den = t_0 + t_1 + .. left to right
  __syncthreads();
  if (tid < N) pre[0][tid] = cre * ucr + cim * uci;
  __syncthreads();
  if (tid < N) {
    double den = pre[0][0];
    for (int p = 1; p < N; p++) den = den + pre[0][p];
    const int qr = st_quantise(ucr / den), qi = st_quantise(uci / den);
    *reinterpret_cast<int2*>(a.Wq + ((long long)i * N + tid) * 2) = make_int2(qr, qi);
    if (owned && a.wout) {
      int* o = a.wout + ((b - a.own_first) * N + tid) * 2;
      o[0] = qr;
      o[1] = qi;
    }
  }
}

// ---- outputs

// Sample indices are relative to j0, the launch's first output: a launch covers at most 2^29 samples, so they are 32-bit.
struct StApplyArgs {
  const uint8_t* in[kStMaxM];   // antenna p: the address of input sample j0 (it may lie before the input; lo says what is there)
  uint8_t* out;                 // the address of output sample j0
  const int* Wq;                // the weights of block b_first + i at Wq[2 N i]
  unsigned long long* stats;
  unsigned long long owned;     // what the launch adds to stats[1]
  int n;                        // the launch's outputs: samples 0 .. n - 1
  int phase;                    // j0 mod the tile: tiles and runs lie on multiples of the ABSOLUTE index
  int lo, hi;                   // the input present: samples lo .. hi - 1 (cut to +-2^30: a run reaches 16 samples at the most)
  int boff;                     // j0 less the first sample of block b_first
  float s;
  int Lb, M;
};

template <bool F32, int T>
__global__ __launch_bounds__(kStBlock) void stap_apply_kernel(const StApplyArgs a) {
  constexpr int TC = (T - 1) / 2, PM = kStMaxN / T < kStMaxM ? kStMaxN / T : kStMaxM;
  const int tid = threadIdx.x, N = a.M * T;
  const int ntiles = (a.phase + a.n - 1) / kStTile + 1;
  unsigned nclip = 0;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
#pragma unroll 1
    for (int rr = 0; rr < kStRuns; rr++) {
      const int j = tile * kStTile - a.phase + (rr * kStBlock + tid) * 8;
      if (j + 8 <= 0 || j >= a.n) continue;
      const bool full = j >= 0 && j + 8 <= a.n;
      const bool wide = j - 8 >= a.lo && j + 16 <= a.hi;               // samples j - 8 .. j + 15 are all present
      const int* w = a.Wq + 2 * N * (int)((unsigned)(j + a.boff) / (unsigned)a.Lb);
      int yr[8], yi[8];
#pragma unroll
      for (int e = 0; e < 8; e++) yr[e] = yi[e] = 0;
#pragma unroll
      for (int p = 0; p < PM; p++) {
        if (p < a.M) {
          const uint8_t* ps = a.in[p] + (j - 8) * 2;                   // sample j - 8
          unsigned x[12];
          if (wide) {
            __builtin_memcpy(x, ps, 48);
          } else {
#pragma unroll
            for (int e = 0; e < 24; e++) {
              unsigned v = 0u;
              if (j - 8 + e >= a.lo && j - 8 + e < a.hi) v = (unsigned)ps[2 * e] | ((unsigned)ps[2 * e + 1] << 8);
              if (e & 1) x[e >> 1] |= v << 16;
              else x[e >> 1] = v;
            }
          }
          // samples j - TC .. j + 7 + TC, unpacked once
          int xr[8 + 2 * TC], xi[8 + 2 * TC];
#pragma unroll
          for (int e = 0; e < 8 + 2 * TC; e++) {
            const int at = 8 - TC + e;
            xr[e] = (int)(signed char)(unsigned char)(x[at >> 1] >> (16 * (at & 1)));
            xi[e] = (int)(signed char)(unsigned char)(x[at >> 1] >> (16 * (at & 1) + 8));
          }
#pragma unroll
          for (int t = 0; t < T; t++) {
            const int2 wq = *reinterpret_cast<const int2*>(w + 2 * (p * T + t));
#pragma unroll
            for (int e = 0; e < 8; e++) {                               // z(j + e) = x(j + e + TC - t)
              yr[e] += __mul24(wq.x, xr[e + 2 * TC - t]) + __mul24(wq.y, xi[e + 2 * TC - t]);
              yi[e] += __mul24(wq.x, xi[e + 2 * TC - t]) - __mul24(wq.y, xr[e + 2 * TC - t]);
            }
          }
        }
      }
      if (!full) {                                                      // a sample outside the range is 0: it clips nothing
#pragma unroll
        for (int e = 0; e < 8; e++)
          if (j + e < 0 || j + e >= a.n) yr[e] = yi[e] = 0;
      }
      if constexpr (F32) {
        float o[16];
#pragma unroll
        for (int e = 0; e < 8; e++) {
          o[2 * e] = (float)yr[e] * a.s;
          o[2 * e + 1] = (float)yi[e] * a.s;
        }
        float* po = reinterpret_cast<float*>(a.out) + j * 2;
        if (full) {
          __builtin_memcpy(reinterpret_cast<uint8_t*>(po), o, 64);      // four 16-byte stores; the output lies on 8 bytes
        } else {
#pragma unroll
          for (int e = 0; e < 8; e++)
            if (j + e >= 0 && j + e < a.n) *reinterpret_cast<float2*>(po + 2 * e) = make_float2(o[2 * e], o[2 * e + 1]);
        }
      } else {
        unsigned q[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 16; e++) {
          const float v = (float)((e & 1) ? yi[e >> 1] : yr[e >> 1]) * a.s;
          const float rv = rintf(v);                                    // half to even
          const float cv = fminf(fmaxf(rv, -127.0f), 127.0f);
          nclip += cv != rv ? 1u : 0u;
          q[e >> 2] |= ((unsigned)(int)cv & 0xffu) << (8 * (e & 3));
        }
        uint8_t* po = a.out + j * 2;
        if (full) {
          __builtin_memcpy(po, q, 16);
        } else {
#pragma unroll
          for (int e = 0; e < 16; e++)
            if (j + (e >> 1) >= 0 && j + (e >> 1) < a.n) po[e] = (uint8_t)(q[e >> 2] >> (8 * (e & 3)));
        }
      }
    }
  }
  if (a.stats) {
    if (!F32) {
      for (int off = 1; off < 64; off <<= 1) nclip += __shfl_xor(nclip, off, 64);
      if ((tid & 63) == 0 && nclip) atomicAdd(a.stats, (unsigned long long)nclip);
    }
    if (blockIdx.x == 0 && tid == 0 && a.owned) atomicAdd(a.stats + 1, a.owned);
  }
}

template <bool F32>
void launch_apply(int T, unsigned grid, hipStream_t stream, const StApplyArgs& ap) {
  switch (T) {
    case 1: hipLaunchKernelGGL((stap_apply_kernel<F32, 1>), dim3(grid), dim3(kStBlock), 0, stream, ap); break;
    case 3: hipLaunchKernelGGL((stap_apply_kernel<F32, 3>), dim3(grid), dim3(kStBlock), 0, stream, ap); break;
    case 5: hipLaunchKernelGGL((stap_apply_kernel<F32, 5>), dim3(grid), dim3(kStBlock), 0, stream, ap); break;
    case 7: hipLaunchKernelGGL((stap_apply_kernel<F32, 7>), dim3(grid), dim3(kStBlock), 0, stream, ap); break;
    case 9: hipLaunchKernelGGL((stap_apply_kernel<F32, 9>), dim3(grid), dim3(kStBlock), 0, stream, ap); break;
    case 11: hipLaunchKernelGGL((stap_apply_kernel<F32, 11>), dim3(grid), dim3(kStBlock), 0, stream, ap); break;
    case 13: hipLaunchKernelGGL((stap_apply_kernel<F32, 13>), dim3(grid), dim3(kStBlock), 0, stream, ap); break;
    default: hipLaunchKernelGGL((stap_apply_kernel<F32, 15>), dim3(grid), dim3(kStBlock), 0, stream, ap); break;
  }
}

int check_cfg(const gacq_stap_cfg* c) {
  if (!c) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_stap: NULL argument");
  if (c->antennas < 1 || c->antennas > kStMaxM)
    return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_stap: %d antennas: need 1..%d", c->antennas, kStMaxM);
  if (c->taps < 1 || c->taps > kStMaxT || c->taps % 2 == 0)
    return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_stap: %d taps: need an odd number in 1..%d", c->taps, kStMaxT);
  if (c->antennas * c->taps > kStMaxN)
    return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_stap: %d antennas x %d taps: need at most %d weights", c->antennas, c->taps, kStMaxN);
  if (c->block < 64 || c->block > kStMaxLb || c->block % 64)
    return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_stap: the block length %d is no multiple of 64 in 64..%d", c->block, kStMaxLb);
  if (c->window < 1 || c->window > kStMaxWindow)
    return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_stap: the window %d lies outside 1..%d", c->window, kStMaxWindow);
  if (c->load_shift < 0 || c->load_shift > kStMaxShift)
    return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_stap: load_shift %d lies outside 0..%d", c->load_shift, kStMaxShift);
  bool any = false;
  for (int i = 0; i < 2 * c->antennas; i++) {
    if (!std::isfinite(c->c[i])) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_stap: constraint component %d is not finite", i);
    any = any || c->c[i] != 0.0;
  }
  if (!any) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_stap: the constraint is all zero");
  return GACQ_OK;
}

// blocks a triple of launches covers: the covariances of chunk + W blocks and the weights of chunk blocks fit the workspace
long long chunk_blocks(const gacq_stap_cfg& c) {
  const size_t N = (size_t)c.antennas * c.taps, cov = N * N * 2 * sizeof(int), wgt = N * 2 * sizeof(int);
  return std::min<long long>(kStMaxChunk, (long long)((kStWorkspace - (size_t)c.window * cov) / (cov + wgt)));
}

}  // namespace

#include "gacq_streamhost.h"

struct gacq_stap {
  gacq_ctx* ctx = nullptr;
  gacq_stap_cfg cfg{};
  long long chunk = 0;
  StDevBlock dev;               // the block covariances of a triple of launches, then the weights of its blocks
};

extern "C" int gacq_stap_tile(const gacq_stap_cfg* cfg) {
  if (!cfg || check_cfg(cfg) < 0) return GACQ_ERR_BAD_ARG;
  return kStTile;
}

extern "C" long long gacq_stap_workspace(const gacq_stap_cfg* cfg) {
  if (!cfg || check_cfg(cfg) < 0) return GACQ_ERR_BAD_ARG;
  const size_t N = (size_t)cfg->antennas * cfg->taps, K = (size_t)chunk_blocks(*cfg);
  return (long long)(((K + cfg->window) * N * N * 2 + K * N * 2) * sizeof(int));
}

extern "C" int gacq_stap_check(const gacq_stap_cfg* cfg, long long in_first, long long in_count, long long out_first, long long n_out, double gain,
                               int out_complex64) {
  (void)out_complex64;                                                  // either form takes every range
  int rc = check_cfg(cfg);
  if (rc == GACQ_OK) rc = st_check_gain(nullptr, "gacq_stap", "is not finite and positive", gain);
  if (rc == GACQ_OK) rc = st_check_range(nullptr, "gacq_stap", in_first, in_count, out_first, n_out);
  if (rc < 0 || n_out == 0) return rc;
  const long long Lb = cfg->block, W = cfg->window, tc = (cfg->taps - 1) / 2;
  return st_check_support(nullptr, "gacq_stap", out_first, n_out, std::max(std::max(out_first / Lb - W, 0ll) * Lb - tc, 0ll),
                          std::max(out_first + n_out, W * Lb) - 1 + tc, in_first, in_count);
}

extern "C" int gacq_stap_open(gacq_ctx* ctx, const gacq_stap_cfg* cfg, gacq_stap** out) {
  if (!ctx) return GACQ_ERR_BAD_ARG;
  if (!out) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_stap_open: NULL argument");
  *out = nullptr;
  const int rc = gacq_stap_check(cfg, 0, 0, 0, 0, 1.0, 0);
  if (rc < 0) return st_forward(ctx, rc);
  std::unique_ptr<gacq_stap> h(new gacq_stap);
  h->ctx = ctx;
  h->cfg = *cfg;
  h->chunk = chunk_blocks(*cfg);
  {
    GACQ_DEVICE(ctx);
    const hipError_t e = h->dev.alloc(ctx, (size_t)gacq_stap_workspace(cfg));
    if (e != hipSuccess) return set_error(ctx, GACQ_ERR_HIP, "gacq_stap_open: %s", hipGetErrorString(e));
  }
  *out = h.release();
  return GACQ_OK;
}

extern "C" void gacq_stap_close(gacq_stap* h) { delete h; }

extern "C" int gacq_stap_run_dev(gacq_stap* h, const void* const* d_in, long long in_first, long long in_count, long long out_first, long long n_out,
                                 double gain, int out_complex64, void* d_out, void* d_stats, void* d_weights, void* d_cov) {
  if (!h) return GACQ_ERR_BAD_ARG;
  gacq_ctx* ctx = h->ctx;
  const gacq_stap_cfg& c = h->cfg;
  if (!d_in || !d_out) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_stap_run_dev: NULL argument");
  for (int p = 0; p < c.antennas; p++)
    if (!d_in[p]) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_stap_run_dev: the pointer of antenna %d is NULL", p);
  // everything is checked before anything is launched
  int rc = gacq_stap_check(&c, in_first, in_count, out_first, n_out, gain, out_complex64);
  if (rc < 0) return st_forward(ctx, rc);
  if (out_complex64 && (uintptr_t)d_out % 8u) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_stap_run_dev: complex64 output must be 8-byte aligned");
  if ((uintptr_t)d_stats % 8u) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_stap_run_dev: d_stats must be 8-byte aligned");
  if ((uintptr_t)d_weights % 4u) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_stap_run_dev: d_weights must be 4-byte aligned");
  if ((uintptr_t)d_cov % 8u) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_stap_run_dev: d_cov must be 8-byte aligned");
  if (n_out == 0) return GACQ_OK;
  const int M = c.antennas, T = c.taps, N = M * T;
  const long long Lb = c.block, W = c.window, out_end = out_first + n_out;
  const long long own_first = (out_first + Lb - 1) / Lb;
  int* dC = (int*)h->dev.p;
  int* dWq = dC + (size_t)(h->chunk + W) * N * N * 2;
  GACQ_DEVICE(ctx);
  for (long long o = out_first; o < out_end;) {
    const long long b0 = o / Lb, o_end = std::min(out_end, (b0 + h->chunk) * Lb), b_hi = (o_end - 1) / Lb;
    // ---- the covariances the weights of blocks b0 .. b_hi need
    StCovArgs cv;
    const long long pb0 = std::max(b0 - W, 0ll);
    for (int p = 0; p < kStMaxM; p++) cv.in[p] = (const uint8_t*)d_in[p < M ? p : 0] + (pb0 * Lb - in_first) * 2;
    cv.C = dC;
    cv.nblk = std::max(b_hi, W) - pb0;
    cv.abs0 = pb0 * Lb;
    cv.Lb = (int)Lb;
    cv.M = M;
    cv.T = T;
    cv.N = N;
    cv.nt = (2 * N + 15) / 16;
    const long long nwg = (cv.nblk * cv.nt + kStBlock / 64 - 1) / (kStBlock / 64);
    hipLaunchKernelGGL(stap_cov_kernel, dim3((unsigned)std::min<long long>(nwg, (long long)kStMaxGrid)), dim3(kStBlock), 0, ctx->stream, cv);
    if ((rc = st_launched(ctx, "gacq_stap_run_dev")) < 0) return rc;
    // ---- the weights of blocks b0 .. b_hi
    StWgtArgs wg;
    wg.C = dC;
    wg.Wq = dWq;
    wg.cov = (long long*)d_cov;
    wg.wout = (int*)d_weights;
    for (int i = 0; i < 2 * kStMaxM; i++) wg.c[i] = i < 2 * M ? c.c[i] : 0.0;
    wg.b_first = b0;
    wg.own_first = own_first;
    wg.nblk = (int)(b_hi - b0 + 1);
    wg.p_off = (int)(b0 - pb0);
    wg.warm = (int)std::max(W - b0, 0ll);
    wg.W = (int)W;
    wg.M = M;
    wg.T = T;
    wg.N = N;
    wg.shift = c.load_shift;
    hipLaunchKernelGGL(stap_weights_kernel, dim3((unsigned)wg.nblk), dim3(kStBlock), 0, ctx->stream, wg);
    if ((rc = st_launched(ctx, "gacq_stap_run_dev")) < 0) return rc;
    // ---- the outputs o .. o_end - 1
    StApplyArgs ap;
    for (int p = 0; p < kStMaxM; p++) ap.in[p] = (const uint8_t*)d_in[p < M ? p : 0] + (o - in_first) * 2;
    ap.out = (uint8_t*)d_out + (o - out_first) * (out_complex64 ? 8 : 2);
    ap.Wq = dWq;
    ap.stats = (unsigned long long*)d_stats;
    ap.n = (int)(o_end - o);
    ap.phase = (int)(o % kStTile);
    ap.lo = (int)std::max(in_first - o, -(1ll << 30));
    ap.hi = (int)std::min(in_first + in_count - o, 1ll << 30);
    ap.boff = (int)(o - b0 * Lb);
    ap.owned = (unsigned long long)((o_end + Lb - 1) / Lb - (o + Lb - 1) / Lb);
    ap.s = (float)gain * (1.0f / (float)kStWq);
    ap.Lb = (int)Lb;
    ap.M = M;
    const long long ntiles = (o_end - 1) / kStTile - o / kStTile + 1;
    const unsigned grid = (unsigned)std::min<long long>(ntiles, (long long)kStMaxGrid);
    if (out_complex64) launch_apply<true>(T, grid, ctx->stream, ap);
    else launch_apply<false>(T, grid, ctx->stream, ap);
    if ((rc = st_launched(ctx, "gacq_stap_run_dev")) < 0) return rc;
    o = o_end;
  }
  return GACQ_OK;
}
