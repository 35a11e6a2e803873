// Spatial nulling with an antenna array (gacq_null_*, include/gacq.h): M int8 I/Q recordings on one clock in, one recording out, under
// block-wise weights that minimise the output power subject to one linear constraint.  The covariances are exact integers and the
// solve is one written-out fp64 sequence, so every output byte is a function of (configuration, absolute sample index) alone.
//
// Three launches per call (per 2^14 blocks), on one stream:
//   null_cov_kernel      C_b of every block the call's weights need, into the handle's workspace.  The spatial covariance of M complex
//      antennas is the Gram matrix of 2M real rows (I_0, Q_0, I_1, ..), rows from 2M up zero: one 16 x 16 x 64 int8 matrix instruction
//      per 64 samples, accumulated in int32.  Lane l holds row l & 15 at samples 16 (l >> 4) .. + 15 of the group: two 16-byte loads
//      at any address (lanes 2p and 2p + 1 load the same 32 bytes), the I or the Q bytes picked with four byte permutes.  The product is
//      G = A A^T, and the B fragment of lane l (column l & 15, k-group l >> 4) holds the bytes of its A fragment: the same four registers
//      are both operands, so the result does not depend on the order of k inside a fragment, and rows I_p and Q_p see sample j at the
//      same k because both take their bytes with the same permute pattern.  min(4, Lb / 64) waves share a block (4, 2 or 1 blocks a
//      workgroup), their partial tiles meet in LDS; the lane that holds column 2q takes column 2q + 1 from its neighbour and writes
//      Re C = G[2p][2q] + G[2p+1][2q+1], Im C = G[2p+1][2q] - G[2p][2q+1] -- no negated row, -(-128) does not fit int8.
//   null_weights_kernel  a wave per block, lane 8 r + c holds A[r][c]: the window sum in int64, the loading, Gaussian elimination and back
//      substitution in the order of the header, the pivot row, the multiplier and the partial products fetched from their lanes;
//      every lane runs the same fp64 sequence as tests/nulling_oracle.py.  No per-lane array: nothing goes to scratch.
//   null_apply_kernel    a lane's run is the 8 samples at a multiple of 8 of the ABSOLUTE sample index, so a run lies in one block
//      (Lb is a multiple of 64) whatever out_first is: M 16-byte loads, 24-bit integer multiply-adds, one 16-byte store (int8) or four
//      (complex64).  A workgroup owns the 16384 samples at a multiple of 16384 (run r of a lane is run 256 r + lane of the tile); only
//      the runs over the ends of the output range work sample by sample.  The weights of a run's block come from the workspace (the
//      lanes of a wave read the same 64 bytes).
#pragma clang fp contract(off)

#include "gacq_arraycore.h"

#include <algorithm>
#include <cstring>

using namespace gacq;

namespace {

// ---- block covariances

struct NlCovArgs {
  const uint8_t* in[kArMaxM];   // antenna p: the address of the first sample of block 0 of the launch
  int* C;                       // [block][8][8][2]
  long long nblk;
  int Lb, M;
  int wpb_log2;                 // waves per block: 1, 2 or 4
};

// two workgroups a compute unit at the least: with at most 256 registers a wave the compiler keeps the matrix instruction's
// accumulator in VGPRs (with all 512 in reach it takes accumulator registers)
__global__ __launch_bounds__(kArBlock, 2) void null_cov_kernel(const NlCovArgs a) {
  __shared__ int red[kArBlock / 64][4][64];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int row = lane & 15, kg = lane >> 4, p = row >> 1;
  const unsigned sel = (row & 1) ? kArSelQ : kArSelI;
  const uint8_t* src = a.in[0];
#pragma unroll
  for (int q = 1; q < kArMaxM; q++)
    if (p == q && q < a.M) src = a.in[q];
  const bool live = p < a.M;
  const int wpb = 1 << a.wpb_log2, per = (kArBlock / 64) >> a.wpb_log2;
  const int blw = wave >> a.wpb_log2, sub = wave & (wpb - 1);
  const int groups = a.Lb >> 6;
  const long long npass = (a.nblk + per - 1) / per;
  for (long long pass = blockIdx.x; pass < npass; pass += gridDim.x) {
    const long long bl = pass * per + blw;
    ar_v4i acc = {0, 0, 0, 0};
    if (bl < a.nblk) {
      const uint8_t* pb = src + (bl * a.Lb + 16 * kg) * 2;
      for (int g = sub; g < groups; g += wpb) {
        ar_v4i f = {0, 0, 0, 0};
        if (live) {
          const uint4 lo = load16_any(pb + 128 * (long long)g), hi = load16_any(pb + 128 * (long long)g + 16);
          f.x = (int)__builtin_amdgcn_perm(lo.y, lo.x, sel);
          f.y = (int)__builtin_amdgcn_perm(lo.w, lo.z, sel);
          f.z = (int)__builtin_amdgcn_perm(hi.y, hi.x, sel);
          f.w = (int)__builtin_amdgcn_perm(hi.w, hi.z, sel);
        }
        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(f, f, acc, 0, 0, 0);
      }
    }
    red[wave][0][lane] = acc.x;
    red[wave][1][lane] = acc.y;
    red[wave][2][lane] = acc.z;
    red[wave][3][lane] = acc.w;
    __syncthreads();
    if (sub == 0 && bl < a.nblk) {
      // the lane holds G[4 kg + i][lane & 15], i < 4: rows I, Q of antenna 2 kg and I, Q of antenna 2 kg + 1
      int g[4], n[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        g[i] = 0;
        for (int s = 0; s < wpb; s++) g[i] += red[wave + s][i][lane];
        n[i] = __shfl_xor(g[i], 1, 64);                                 // the same rows of the neighbouring column
      }
      if (!(lane & 1)) {
        const int q = (lane & 15) >> 1;
#pragma unroll
        for (int h = 0; h < 2; h++) {
          int* o = a.C + ((bl * 8 + 2 * kg + h) * 8 + q) * 2;
          *reinterpret_cast<int2*>(o) = make_int2(g[2 * h] + n[2 * h + 1], g[2 * h + 1] - n[2 * h]);
        }
      }
    }
    __syncthreads();
  }
}

}  // namespace

void gacq::null_launch_cov(const uint8_t* const* in, int* C, long long nblk, int Lb, int M, hipStream_t stream) {
  NlCovArgs cv;
  for (int p = 0; p < kArMaxM; p++) cv.in[p] = in[p];
  cv.C = C;
  cv.nblk = nblk;
  cv.Lb = Lb;
  cv.M = M;
  cv.wpb_log2 = Lb >= 256 ? 2 : Lb >= 128 ? 1 : 0;
  const long long per = (kArBlock / 64) >> cv.wpb_log2, npass = (cv.nblk + per - 1) / per;
  hipLaunchKernelGGL(null_cov_kernel, dim3((unsigned)std::min<long long>(npass, (long long)kArMaxGrid)), dim3(kArBlock), 0, stream, cv);
}

namespace {

// ---- weights

struct NlWgtArgs {
  const int* C;                 // C[i] is block pb0 + i
  int* Wq;                      // [block][8][2]: the launch's block i at Wq[16 i]
  long long* cov;               // d_cov, or NULL
  int* wout;                    // d_weights, or NULL
  double c[2 * kArMaxM];
  long long b_first;            // the absolute index of the launch's block 0
  long long own_first;          // the call's first owned block
  int nblk;
  int p_off;                    // b_first less the block of C[0]
  int warm;                     // blocks b_first + i with i < warm are in the warm-up: their window is C[0 .. W - 1]
  int W, M, shift;
};

__global__ __launch_bounds__(kArBlock) void null_weights_kernel(const NlWgtArgs a) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (kArBlock / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (i >= a.nblk) return;
  const int r = lane >> 3, c = lane & 7, M = a.M;
  const bool in = r < M && c < M;
  // ---- the window sum, the loading (gacq_arraycore.h)
  const int* pc = a.C + ((long long)(i >= a.warm ? a.p_off + i - a.W : 0) * 64 + lane) * 2;
  long long Rre, Rim;
  ar_window_sum(pc, a.W, Rre, Rim);
  const long long b = a.b_first + i;
  const bool owned = b >= a.own_first;
  if (owned && a.cov && in) {
    long long* o = a.cov + (((b - a.own_first) * M + r) * M + c) * 2;
    o[0] = Rre;
    o[1] = Rim;
  }
  double Are, Aim;
  ar_load_diagonal(Rre, Rim, a.shift, M, r, c, Are, Aim);
  double cre = 0.0, cim = 0.0, bre = 0.0, bim = 0.0;                    // c of the lane's column, b of its row
#pragma unroll
  for (int q = 0; q < kArMaxM; q++) {
    if (c == q && q < M) cre = a.c[2 * q], cim = a.c[2 * q + 1];
    if (r == q && q < M) bre = a.c[2 * q], bim = a.c[2 * q + 1];
  }
  // ---- elimination, b along with A
  ar_eliminate<true>(Are, Aim, bre, bim, M, r, c);
  // ---- back substitution: the lane keeps u of its column
  double ucr = 0.0, uci = 0.0;
  for (int k = M - 1; k >= 0; k--) {
    const double pre = Are * ucr - Aim * uci, pim = Are * uci + Aim * ucr;      // A[r][c] u[c]
    double sre = __shfl(bre, 8 * k, 64), sim = __shfl(bim, 8 * k, 64);
    for (int q = k + 1; q < M; q++) {
      sre = sre - __shfl(pre, 8 * k + q, 64);
      sim = sim - __shfl(pim, 8 * k + q, 64);
    }
    const double piv = __shfl(Are, 9 * k, 64);
    const double xr = sre / piv, xi = sim / piv;
    if (c == k) ucr = xr, uci = xi;
  }
  // ---- the constraint's scale
  const double tp = cre * ucr + cim * uci;
  double den = __shfl(tp, 0, 64);
  for (int p = 1; p < M; p++) den = den + __shfl(tp, p, 64);
  const int qr = c < M ? ar_quantise(ucr / den) : 0, qi = c < M ? ar_quantise(uci / den) : 0;
  if (r == 0) {
    *reinterpret_cast<int2*>(a.Wq + 16 * (long long)i + 2 * c) = make_int2(qr, qi);
    if (owned && a.wout && c < M) {
      int* o = a.wout + ((b - a.own_first) * M + c) * 2;
      o[0] = qr;
      o[1] = qi;
    }
  }
}

// ---- outputs

struct NlApplyArgs {
  const uint8_t* in[kArMaxM];   // antenna p: the address of input sample j0
  uint8_t* out;                 // the address of output sample j0
  const int* Wq;                // the weights of block b_first + i at Wq[16 i]
  unsigned long long* stats;
  long long j0, n;              // the launch's outputs: absolute samples j0 .. j0 + n - 1
  long long blk0;               // the first sample of block b_first (<= j0)
  unsigned long long owned;     // what the launch adds to stats[1]
  float s;
  int Lb, M;
};

template <bool F32>
__global__ __launch_bounds__(kArBlock) void null_apply_kernel(const NlApplyArgs a) {
  const int tid = threadIdx.x;
  const long long t0 = a.j0 / kArTile, j_end = a.j0 + a.n;
  const long long ntiles = (j_end - 1) / kArTile - t0 + 1;
  unsigned nclip = 0;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
#pragma unroll 1
    for (int rr = 0; rr < kArRuns; rr++) {
      const long long j = (t0 + tile) * kArTile + (rr * kArBlock + tid) * 8;
      if (j + 8 <= a.j0 || j >= j_end) continue;
      const bool full = j >= a.j0 && j + 8 <= j_end;
      const int* w = a.Wq + 16 * (long long)((unsigned)(j - a.blk0) / (unsigned)a.Lb);
      int yr[8], yi[8];
#pragma unroll
      for (int e = 0; e < 8; e++) yr[e] = yi[e] = 0;
#pragma unroll
      for (int p = 0; p < kArMaxM; p++) {
        if (p < a.M) {
          const int2 wq = *reinterpret_cast<const int2*>(w + 2 * p);
          const uint8_t* ps = a.in[p] + (j - a.j0) * 2;
          unsigned x[4];
          if (full) {
            __builtin_memcpy(x, ps, 16);
          } else {
#pragma unroll
            for (int e = 0; e < 8; e++) {
              unsigned v = 0u;
              if (j + e >= a.j0 && j + e < j_end) v = (unsigned)ps[2 * e] | ((unsigned)ps[2 * e + 1] << 8);
              if (e & 1) x[e >> 1] |= v << 16;
              else x[e >> 1] = v;
            }
          }
#pragma unroll
          for (int e = 0; e < 8; e++) {
            const int xr = (int)(signed char)(unsigned char)(x[e >> 1] >> (16 * (e & 1)));
            const int xi = (int)(signed char)(unsigned char)(x[e >> 1] >> (16 * (e & 1) + 8));
            yr[e] += __mul24(wq.x, xr) + __mul24(wq.y, xi);
            yi[e] += __mul24(wq.x, xi) - __mul24(wq.y, xr);
          }
        }
      }
      AR_STORE_RUN(F32, yr, yi, a.s, a.out, full, j, a.j0, j_end, nclip)
    }
  }
  AR_ADD_STATS(F32, a.stats, nclip, a.owned, tid)
}

}  // namespace

#include "gacq_arrayhost.h"

struct gacq_null : ArHandle<gacq_null_cfg> {};

static int check_cfg(const gacq_null_cfg* c) {
  return ar_check_cfg("gacq_null", 2, c, [](const gacq_null_cfg&) { return GACQ_OK; });
}

extern "C" int gacq_null_tile(const gacq_null_cfg* cfg) {
  if (!cfg || check_cfg(cfg) < 0) return GACQ_ERR_BAD_ARG;
  return kArTile;
}

extern "C" int gacq_null_check(const gacq_null_cfg* cfg, long long in_first, long long in_count, long long out_first, long long n_out, double gain,
                               int out_complex64) {
  (void)out_complex64;                                                  // either form takes every range
  return ar_check_call("gacq_null", check_cfg(cfg), cfg, 0, in_first, in_count, out_first, n_out, gain);
}

extern "C" int gacq_null_open(gacq_ctx* ctx, const gacq_null_cfg* cfg, gacq_null** out) {
  return ar_open("gacq_null_open", ctx, cfg, out, gacq_null_check,
                 [](gacq_null&) { return ((size_t)(kArMaxChunk + kArMaxWindow) * 128 + (size_t)kArMaxChunk * 16) * sizeof(int); });
}

extern "C" void gacq_null_close(gacq_null* h) { delete h; }

extern "C" int gacq_null_run_dev(gacq_null* h, const void* const* d_in, long long in_first, long long in_count, long long out_first, long long n_out,
                                 double gain, int out_complex64, void* d_out, void* d_stats, void* d_weights, void* d_cov) {
  if (!h) return GACQ_ERR_BAD_ARG;
  const gacq_null_cfg& c = h->cfg;
  hipStream_t stream = h->ctx->stream;
  return ar_run_dev(
      "gacq_null_run_dev", *h, gacq_null_check, ArRun{d_in, in_first, in_count, out_first, n_out, gain, out_complex64, d_out, d_stats, d_weights, d_cov},
      kArMaxChunk, (size_t)(kArMaxChunk + kArMaxWindow) * 128,
      [&](const ArRun& r) {
        const uint8_t* in[kArMaxM];
        ar_inputs(in, r, c.antennas, r.pb0 * c.block);
        null_launch_cov(in, r.dC, r.ncov, c.block, c.antennas, stream);
      },
      [&](const ArRun& r) {
        NlWgtArgs wg;
        ar_fill_weights(wg, c, r);
        hipLaunchKernelGGL(null_weights_kernel, dim3((unsigned)((wg.nblk + kArBlock / 64 - 1) / (kArBlock / 64))), dim3(kArBlock), 0, stream, wg);
      },
      [&](const ArRun& r) {
        NlApplyArgs ap;
        ar_fill_apply(ap, c, r);
        ap.j0 = r.o;
        ap.n = r.o_end - r.o;
        ap.blk0 = r.b0 * c.block;
        if (r.out_complex64) hipLaunchKernelGGL(null_apply_kernel<true>, dim3(r.grid), dim3(kArBlock), 0, stream, ap);
        else hipLaunchKernelGGL(null_apply_kernel<false>, dim3(r.grid), dim3(kArBlock), 0, stream, ap);
      });
}

