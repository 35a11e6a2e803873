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

#include "gacq_arraycore.h"

#include <algorithm>
#include <cstring>

using namespace gacq;

namespace {

constexpr int kStMaxT = 15, kStMaxN = 56;
constexpr size_t kStWorkspace = 64u << 20;           // bytes of the handle's workspace, at most
constexpr int kStMaxTiles = (2 * kStMaxN + 15) / 16; // 7 tiles of 16 real rows
constexpr int kStStride = kStMaxN + 1;               // doubles between the rows of a plane in LDS: odd, so rows fall on different banks

// ---- block covariances

struct StCovArgs {
  const uint8_t* in[kArMaxM];   // antenna p: the address of the first sample of block 0 of the launch
  int* C;                       // [block][N][N][2]
  long long nblk;
  long long abs0;               // the absolute index of that sample
  int Lb, M, T, N, nt;          // nt: tiles of 16 real rows
};

// The fragment of a lane's row over 16 samples that begin at absolute sample s (the address p): the I or the Q bytes.  Samples below
// 0 do not exist: they are zeros, and nothing below the recording's first byte is read.
__device__ __forceinline__ ar_v4i st_fragment(const uint8_t* p, long long s, unsigned sel, bool live) {
  ar_v4i f = {0, 0, 0, 0};
  if (live) {
    unsigned w[8];
    if (s >= 0) {
      const uint4 lo = load16_any(p), hi = load16_any(p + 16);
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
__global__ __launch_bounds__(kArBlock, 2) void stap_cov_kernel(const StCovArgs a) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row = lane & 15, kg = lane >> 4, tc = (a.T - 1) >> 1;
  const unsigned sel = (row & 1) ? kArSelQ : kArSelI;
  const long long units = a.nblk * a.nt, step = (long long)gridDim.x * (kArBlock / 64);
  const int groups = a.Lb >> 6;
  for (long long unit = (long long)blockIdx.x * (kArBlock / 64) + wave; unit < units; unit += step) {
    const long long bl = unit / a.nt;
    const int tu = (int)(unit - bl * a.nt);
    // the lane's row of every tile of the unit: where its samples begin, in the block's coordinates
    const uint8_t* src[kStMaxTiles];
    int shift[kStMaxTiles];
    bool live[kStMaxTiles];
    ar_v4i acc[kStMaxTiles];
#pragma unroll
    for (int d = 0; d < kStMaxTiles; d++) {
      const int e = 8 * (tu + d) + (row >> 1);
      live[d] = tu + d < a.nt && e < a.N;
      const int p = live[d] ? e / a.T : 0, t = live[d] ? e - p * a.T : tc;
      const uint8_t* s = a.in[0];
#pragma unroll
      for (int q = 1; q < kArMaxM; q++)
        if (p == q) s = a.in[q];
      shift[d] = 16 * kg + tc - t;
      src[d] = s + (bl * a.Lb + shift[d]) * 2;
      acc[d] = ar_v4i{0, 0, 0, 0};
    }
    const long long first = a.abs0 + bl * a.Lb;
    for (int g = 0; g < groups; g++) {
      const ar_v4i fu = st_fragment(src[0] + 128 * (long long)g, first + 64 * g + shift[0], sel, live[0]);
      acc[0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fu, fu, acc[0], 0, 0, 0);
#pragma unroll
      for (int d = 1; d < kStMaxTiles; d++) {
        if (tu + d < a.nt) {
          const ar_v4i fv = st_fragment(src[d] + 128 * (long long)g, first + 64 * g + shift[d], sel, live[d]);
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
  double c[2 * kArMaxM];
  long long b_first;            // the absolute index of the launch's block 0
  long long own_first;          // the call's first owned block
  int nblk;
  int p_off;                    // b_first less the block of C[0]
  int warm;                     // blocks b_first + i with i < warm are in the warm-up: their window is C[0 .. W - 1]
  int W, M, T, N, shift;
};

__global__ __launch_bounds__(kArBlock) void stap_weights_kernel(const StWgtArgs a) {
  __shared__ double Are[kStMaxN * kStStride], Aim[kStMaxN * kStStride];
  __shared__ double bre[kStMaxN], bim[kStMaxN], pre[2][kStMaxN], pim[2][kStMaxN];
  const int tid = threadIdx.x, i = blockIdx.x, N = a.N, tc = (a.T - 1) >> 1;
  const long long b = a.b_first + i;
  const bool owned = b >= a.own_first;
  // ---- the window sum
  const long long nn = (long long)N * N;
  const int* pc = a.C + (long long)(i >= a.warm ? a.p_off + i - a.W : 0) * nn * 2;
  for (int el = tid; el < N * N; el += kArBlock) {
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
      for (int q = 0; q < kArMaxM; q++)
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
    const int qr = ar_quantise(ucr / den), qi = ar_quantise(uci / den);
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
  const uint8_t* in[kArMaxM];   // antenna p: the address of input sample j0 (it may lie before the input; lo says what is there)
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
__global__ __launch_bounds__(kArBlock) void stap_apply_kernel(const StApplyArgs a) {
  constexpr int TC = (T - 1) / 2, PM = kStMaxN / T < kArMaxM ? kStMaxN / T : kArMaxM;
  const int tid = threadIdx.x, N = a.M * T;
  const int ntiles = (a.phase + a.n - 1) / kArTile + 1;
  unsigned nclip = 0;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
#pragma unroll 1
    for (int rr = 0; rr < kArRuns; rr++) {
      const int j = tile * kArTile - a.phase + (rr * kArBlock + tid) * 8;
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
      AR_STORE_RUN(F32, yr, yi, a.s, a.out, full, j, 0, a.n, nclip)
    }
  }
  AR_ADD_STATS(F32, a.stats, nclip, a.owned, tid)
}

template <bool F32>
void launch_apply(int T, unsigned grid, hipStream_t stream, const StApplyArgs& ap) {
  switch (T) {
    case 1: hipLaunchKernelGGL((stap_apply_kernel<F32, 1>), dim3(grid), dim3(kArBlock), 0, stream, ap); break;
    case 3: hipLaunchKernelGGL((stap_apply_kernel<F32, 3>), dim3(grid), dim3(kArBlock), 0, stream, ap); break;
    case 5: hipLaunchKernelGGL((stap_apply_kernel<F32, 5>), dim3(grid), dim3(kArBlock), 0, stream, ap); break;
    case 7: hipLaunchKernelGGL((stap_apply_kernel<F32, 7>), dim3(grid), dim3(kArBlock), 0, stream, ap); break;
    case 9: hipLaunchKernelGGL((stap_apply_kernel<F32, 9>), dim3(grid), dim3(kArBlock), 0, stream, ap); break;
    case 11: hipLaunchKernelGGL((stap_apply_kernel<F32, 11>), dim3(grid), dim3(kArBlock), 0, stream, ap); break;
    case 13: hipLaunchKernelGGL((stap_apply_kernel<F32, 13>), dim3(grid), dim3(kArBlock), 0, stream, ap); break;
    default: hipLaunchKernelGGL((stap_apply_kernel<F32, 15>), dim3(grid), dim3(kArBlock), 0, stream, ap); break;
  }
}

}  // namespace

#include "gacq_arrayhost.h"

struct gacq_stap : ArHandle<gacq_stap_cfg> {
  long long chunk = 0;          // blocks a triple of launches covers
};

static int check_cfg(const gacq_stap_cfg* cfg) {
  return ar_check_cfg("gacq_stap", 1, cfg, [](const gacq_stap_cfg& c) {
    if (c.taps < 1 || c.taps > kStMaxT || c.taps % 2 == 0)
      return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_stap: %d taps: need an odd number in 1..%d", c.taps, kStMaxT);
    if (c.antennas * c.taps > kStMaxN)
      return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_stap: %d antennas x %d taps: need at most %d weights", c.antennas, c.taps, kStMaxN);
    return (int)GACQ_OK;
  });
}

// blocks a triple of launches covers: the covariances of chunk + W blocks and the weights of chunk blocks fit the workspace
static long long chunk_blocks(const gacq_stap_cfg& c) {
  const size_t N = (size_t)c.antennas * c.taps, cov = N * N * 2 * sizeof(int), wgt = N * 2 * sizeof(int);
  return std::min<long long>(kArMaxChunk, (long long)((kStWorkspace - (size_t)c.window * cov) / (cov + wgt)));
}

extern "C" int gacq_stap_tile(const gacq_stap_cfg* cfg) {
  if (!cfg || check_cfg(cfg) < 0) return GACQ_ERR_BAD_ARG;
  return kArTile;
}

extern "C" long long gacq_stap_workspace(const gacq_stap_cfg* cfg) {
  if (!cfg || check_cfg(cfg) < 0) return GACQ_ERR_BAD_ARG;
  const size_t N = (size_t)cfg->antennas * cfg->taps, K = (size_t)chunk_blocks(*cfg);
  return (long long)(((K + cfg->window) * N * N * 2 + K * N * 2) * sizeof(int));
}

extern "C" int gacq_stap_check(const gacq_stap_cfg* cfg, long long in_first, long long in_count, long long out_first, long long n_out, double gain,
                               int out_complex64) {
  (void)out_complex64;                                                  // either form takes every range
  return ar_check_call("gacq_stap", check_cfg(cfg), cfg, cfg ? (cfg->taps - 1) / 2 : 0, in_first, in_count, out_first, n_out, gain);
}

extern "C" int gacq_stap_open(gacq_ctx* ctx, const gacq_stap_cfg* cfg, gacq_stap** out) {
  return ar_open("gacq_stap_open", ctx, cfg, out, gacq_stap_check, [](gacq_stap& h) {
    h.chunk = chunk_blocks(h.cfg);
    return (size_t)gacq_stap_workspace(&h.cfg);
  });
}

extern "C" void gacq_stap_close(gacq_stap* h) { delete h; }

extern "C" int gacq_stap_run_dev(gacq_stap* h, const void* const* d_in, long long in_first, long long in_count, long long out_first, long long n_out,
                                 double gain, int out_complex64, void* d_out, void* d_stats, void* d_weights, void* d_cov) {
  if (!h) return GACQ_ERR_BAD_ARG;
  const gacq_stap_cfg& c = h->cfg;
  const int T = c.taps, N = c.antennas * T;
  hipStream_t stream = h->ctx->stream;
  return ar_run_dev(
      "gacq_stap_run_dev", *h, gacq_stap_check, ArRun{d_in, in_first, in_count, out_first, n_out, gain, out_complex64, d_out, d_stats, d_weights, d_cov},
      h->chunk, (size_t)(h->chunk + c.window) * N * N * 2,
      [&](const ArRun& r) {
        StCovArgs cv;
        cv.abs0 = r.pb0 * c.block;
        ar_inputs(cv.in, r, c.antennas, cv.abs0);
        cv.C = r.dC;
        cv.nblk = r.ncov;
        cv.Lb = c.block;
        cv.M = c.antennas;
        cv.T = T;
        cv.N = N;
        cv.nt = (2 * N + 15) / 16;
        const long long nwg = (cv.nblk * cv.nt + kArBlock / 64 - 1) / (kArBlock / 64);
        hipLaunchKernelGGL(stap_cov_kernel, dim3((unsigned)std::min<long long>(nwg, (long long)kArMaxGrid)), dim3(kArBlock), 0, stream, cv);
      },
      [&](const ArRun& r) {
        StWgtArgs wg;
        ar_fill_weights(wg, c, r);
        wg.T = T;
        wg.N = N;
        hipLaunchKernelGGL(stap_weights_kernel, dim3((unsigned)wg.nblk), dim3(kArBlock), 0, stream, wg);
      },
      [&](const ArRun& r) {
        StApplyArgs ap;
        ar_fill_apply(ap, c, r);
        ap.n = (int)(r.o_end - r.o);
        ap.phase = (int)(r.o % kArTile);
        ap.lo = (int)std::max(r.in_first - r.o, -(1ll << 30));
        ap.hi = (int)std::min(r.in_first + r.in_count - r.o, 1ll << 30);
        ap.boff = (int)(r.o - r.b0 * c.block);
        if (r.out_complex64) launch_apply<true>(T, r.grid, stream, ap);
        else launch_apply<false>(T, r.grid, stream, ap);
      });
}

