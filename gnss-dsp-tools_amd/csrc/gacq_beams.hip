// Per-satellite beams (gacq_beams_*, include/gacq.h): gacq_null with K constraints at once.  M int8 I/Q recordings in, K recordings out;
// the block covariances, the window sums and the loading are formed once, and every byte of output k is what gacq_null_run_dev writes
// under constraint c_k and gain_k.
//
// Three launches per call (per 2^14 blocks), on one stream:
//   null_cov_kernel       gacq_null.hip's own, through gacq::null_launch_cov: the covariance does not know the beams.
//   beams_weights_kernel  a wave per block, lane 8 r + c holds A[r][c] as in null_weights_kernel.  A is eliminated once, without a
//      right-hand side.  After step k lane 8 r + k, r > k, still holds the numerator of the multiplier A[r][k] (no later step writes
//      column k below the diagonal) and lane 9 k the pivot, so the forward pass on a right-hand side runs afterwards, m = A[r][k] /
//      piv_k formed again by the same division on the same bits.  The right-hand sides go in groups of eight: lane 8 r + c holds
//      b[r] of beam c of the group, later u[r] of that beam; the forward pass in ascending k, the back substitution with q ascending,
//      den left to right and the quantiser are the header's operations on the header's operands, for eight beams in the eight columns.
//      The constraints come from the handle's workspace, where gacq_beams_open put them.  No per-lane array: nothing goes to scratch.
//   beams_apply_kernel    tiles and runs as null_apply_kernel.  A lane loads the M x 16 bytes of its run once and then, beam by beam,
//      takes the beam's weights of the run's block, makes the 32 M multiply-adds of 24 bits into 16 accumulators and stores the run
//      to out[k].  The clipped components of a beam are counted in LDS (only a run that clipped adds) and added to stats[k] once per
//      workgroup, with vector atomics.
#pragma clang fp contract(off)

#include "gacq_arraycore.h"

#include <algorithm>
#include <cstring>

using namespace gacq;

namespace {

// ---- weights

struct BmWgtArgs {
  const int* C;                 // C[i] is block pb0 + i
  int* Wq;                      // [block][K][8][2]: beam k of the launch's block i at Wq[16 (i K + k)]
  long long* cov;               // d_cov, or NULL
  int* wout;                    // d_weights, or NULL
  const double* cst;            // [kArMaxBeams][8][2]: the constraints; entries from M up and rows from K up are 0
  long long b_first;            // the absolute index of the launch's block 0
  long long own_first;          // the call's first owned block
  int nblk;
  int p_off;                    // b_first less the block of C[0]
  int warm;                     // blocks b_first + i with i < warm are in the warm-up: their window is C[0 .. W - 1]
  int W, M, shift;
  int K;
};

__global__ __launch_bounds__(kArBlock) void beams_weights_kernel(const BmWgtArgs a) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (kArBlock / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (i >= a.nblk) return;
  const int r = lane >> 3, c = lane & 7, M = a.M, K = a.K;
  const bool in = r < M && c < M;
  // ---- the window sum, the loading and the elimination of A alone: nulling's own (gacq_arraycore.h)
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
  ar_eliminate(Are, Aim, M, r, c);
  // ---- the right-hand sides, eight beams at a time: the lane's column is beam 8 g + c
  for (int g = 0; 8 * g < K; g++) {
    const int beam = 8 * g + c;
    const bool live = beam < K && r < M;
    const double2 cc = reinterpret_cast<const double2*>(a.cst)[(beam & (kArMaxBeams - 1)) * 8 + r];
    const double cre = live ? cc.x : 0.0, cim = live ? cc.y : 0.0;
    double bre = cre, bim = cim;
    // the forward pass: b[r] -= m b[k]
    for (int k = 0; k < M; k++) {
      const double piv = __shfl(Are, 9 * k, 64);
      const double lre = __shfl(Are, 8 * r + k, 64), lim = __shfl(Aim, 8 * r + k, 64);
      const double kre = __shfl(bre, 8 * k + c, 64), kim = __shfl(bim, 8 * k + c, 64);
      if (r > k && r < M) {
        const double mre = lre / piv, mim = lim / piv;
        bre = bre - (mre * kre - mim * kim);
        bim = bim - (mre * kim + mim * kre);
      }
    }
    // back substitution: u[k] = (b[k] - A[k][k+1] u[k+1] - .. ) / piv_k, kept by row k
    double ur = 0.0, ui = 0.0;
    for (int k = M - 1; k >= 0; k--) {
      double sre = __shfl(bre, 8 * k + c, 64), sim = __shfl(bim, 8 * k + c, 64);
      for (int q = k + 1; q < M; q++) {
        const double are = __shfl(Are, 8 * k + q, 64), aim = __shfl(Aim, 8 * k + q, 64);
        const double qre = __shfl(ur, 8 * q + c, 64), qim = __shfl(ui, 8 * q + c, 64);
        sre = sre - (are * qre - aim * qim);
        sim = sim - (are * qim + aim * qre);
      }
      const double piv = __shfl(Are, 9 * k, 64);
      const double xr = sre / piv, xi = sim / piv;
      if (r == k) ur = xr, ui = xi;
    }
    // the constraint's scale
    const double tp = cre * ur + cim * ui;
    double den = __shfl(tp, c, 64);
    for (int p = 1; p < M; p++) den = den + __shfl(tp, 8 * p + c, 64);
    const int qr = live ? ar_quantise(ur / den) : 0, qi = live ? ar_quantise(ui / den) : 0;
    if (beam < K) {
      *reinterpret_cast<int2*>(a.Wq + 16 * ((long long)i * K + beam) + 2 * r) = make_int2(qr, qi);
      if (owned && a.wout && r < M) {
        int* o = a.wout + (((b - a.own_first) * K + beam) * M + r) * 2;
        o[0] = qr;
        o[1] = qi;
      }
    }
  }
}

// ---- outputs

struct BmApplyArgs {
  const uint8_t* in[kArMaxM];   // antenna p: the address of input sample lo
  uint8_t* out[kArMaxBeams];    // beam k: the address of output sample lo
  const int* Wq;                // the weights of beam k of block b_first + i at Wq[16 (i K + k)]
  unsigned long long* stats;
  unsigned long long owned;     // what the launch adds to stats[K]
  float s[kArMaxBeams];
  int lo, hi;                   // the launch's outputs, counted from the first sample of the tile of its first output (a multiple of
                                // 16384 of the absolute index): lo < 16384, hi <= 2^29 + 2^14
  int boff;                     // that tile's first sample less the first sample of block b_first
  int ntiles;
  int Lb, M, K;
};

// four waves a SIMD: at most 128 registers
template <bool F32>
__global__ __launch_bounds__(kArBlock, 4) void beams_apply_kernel(const BmApplyArgs a) {
  __shared__ unsigned clips[kArMaxBeams];
  const int tid = threadIdx.x;
  if (!F32) {
    if (tid < kArMaxBeams) clips[tid] = 0u;
    __syncthreads();
  }
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
#pragma unroll 1
    for (int rr = 0; rr < kArRuns; rr++) {
      const int j = tile * kArTile + (rr * kArBlock + tid) * 8;
      if (j + 8 <= a.lo || j >= a.hi) continue;
      const bool full = j >= a.lo && j + 8 <= a.hi;
      // the run's bytes of every antenna, once
      unsigned x[kArMaxM][4];
      if (full) {
#pragma unroll
        for (int p = 0; p < kArMaxM; p++) {
#pragma unroll
          for (int e = 0; e < 4; e++) x[p][e] = 0u;
          if (p < a.M) __builtin_memcpy(x[p], a.in[p] + (j - a.lo) * 2, 16);
        }
      } else {
        // over an end of the range: sample by sample, a sample outside as 0 -- read from the nearest sample inside, so that no
        // address outside the range is touched and no lane branches
#pragma unroll
        for (int p = 0; p < kArMaxM; p++) {
#pragma unroll
          for (int e = 0; e < 4; e++) x[p][e] = 0u;
        }
#pragma unroll 1
        for (int e = 0; e < 8; e++) {
          const bool inside = j + e >= a.lo && j + e < a.hi;
          const int at = (min(max(j + e, a.lo), a.hi - 1) - a.lo) * 2;
#pragma unroll
          for (int p = 0; p < kArMaxM; p++) {
            if (p < a.M) {
              const uint8_t* ps = a.in[p] + at;
              const unsigned v = inside ? (unsigned)ps[0] | ((unsigned)ps[1] << 8) : 0u;
#pragma unroll
              for (int h = 0; h < 4; h++) x[p][h] |= (e >> 1) == h ? v << (16 * (e & 1)) : 0u;
            }
          }
        }
      }
      const int* wb = a.Wq + 16 * (long long)((unsigned)(j + a.boff) / (unsigned)a.Lb) * a.K;
#pragma unroll 1
      for (int k = 0; k < a.K; k++) {
        const int* w = wb + 16 * k;
        // the packed bytes pass through an empty statement: the 16 M unpacked components would not fit the registers if the compiler
        // took the unpacking out of this loop
#pragma unroll
        for (int p = 0; p < kArMaxM; p++) {
#pragma unroll
          for (int h = 0; h < 4; h++) asm volatile("" : "+v"(x[p][h]));
        }
        int yr[8], yi[8];
#pragma unroll
        for (int e = 0; e < 8; e++) yr[e] = yi[e] = 0;
#pragma unroll
        for (int p = 0; p < kArMaxM; p++) {
          if (p < a.M) {
            const int2 wq = *reinterpret_cast<const int2*>(w + 2 * p);
#pragma unroll
            for (int e = 0; e < 8; e++) {
              const int xr = (int)(signed char)(unsigned char)(x[p][e >> 1] >> (16 * (e & 1)));
              const int xi = (int)(signed char)(unsigned char)(x[p][e >> 1] >> (16 * (e & 1) + 8));
              yr[e] += __mul24(wq.x, xr) + __mul24(wq.y, xi);
              yi[e] += __mul24(wq.x, xi) - __mul24(wq.y, xr);
            }
          }
        }
        const float s = a.s[k];
        uint8_t* const out = a.out[k];
        unsigned nclip = 0;
        AR_STORE_RUN(F32, yr, yi, s, out, full, j, a.lo, a.hi, nclip)
        if (!F32 && nclip) atomicAdd(&clips[k], nclip);
      }
    }
  }
  if (a.stats) {
    if (!F32) {
      __syncthreads();
      if (tid < a.K && clips[tid]) atomicAdd(a.stats + tid, (unsigned long long)clips[tid]);
    }
    if (blockIdx.x == 0 && tid == 0 && a.owned) atomicAdd(a.stats + a.K, a.owned);
  }
}

}  // namespace

#include "gacq_arrayhost.h"

struct gacq_beams : ArHandle<gacq_beams_cfg> {};

// the workspace in ints: the covariances, the weights of every beam, then the constraints (doubles, on 8 bytes)
static size_t wq_at() { return (size_t)(kArMaxChunk + kArMaxWindow) * 128; }
static size_t cst_at(const gacq_beams_cfg& c) { return wq_at() + (size_t)kArMaxChunk * c.beams * 16; }

static int check_cfg(const gacq_beams_cfg* c) {
  return ar_check_cfg("gacq_beams", 2, c, [](const gacq_beams_cfg& c) {
    if (c.beams < 1 || c.beams > kArMaxBeams)
      return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_beams: %d beams: need 1..%d", c.beams, kArMaxBeams);
    return (int)GACQ_OK;
  });
}

extern "C" int gacq_beams_tile(const gacq_beams_cfg* cfg) {
  if (!cfg || check_cfg(cfg) < 0) return GACQ_ERR_BAD_ARG;
  return kArTile;
}

extern "C" int gacq_beams_check(const gacq_beams_cfg* cfg, long long in_first, long long in_count, long long out_first, long long n_out,
                                const double* gain, int out_complex64) {
  (void)out_complex64;                                                  // either form takes every range
  const int rc = check_cfg(cfg);
  return ar_check_call("gacq_beams", rc, cfg, 0, in_first, in_count, out_first, n_out, 1.0, gain, rc == GACQ_OK ? cfg->beams : 0);
}

extern "C" int gacq_beams_open(gacq_ctx* ctx, const gacq_beams_cfg* cfg, gacq_beams** out) {
  double ones[kArMaxBeams];
  std::fill(ones, ones + kArMaxBeams, 1.0);
  const int rc = ar_open(
      "gacq_beams_open", ctx, cfg, out,
      [&](const gacq_beams_cfg* c, long long a, long long b, long long o, long long n, double, int f) { return gacq_beams_check(c, a, b, o, n, ones, f); },
      [](gacq_beams& h) { return cst_at(h.cfg) * sizeof(int) + (size_t)kArMaxBeams * 16 * sizeof(double); });
  if (rc < 0) return rc;
  std::unique_ptr<gacq_beams> h(*out);
  *out = nullptr;
  double cst[kArMaxBeams][16] = {};
  for (int k = 0; k < cfg->beams; k++)
    for (int i = 0; i < 2 * cfg->antennas; i++) cst[k][i] = cfg->c[k][i];
  {
    GACQ_DEVICE(ctx);
    const hipError_t e = h->dev.upload(cst_at(h->cfg) * sizeof(int), cst, sizeof cst);
    if (e != hipSuccess) return set_error(ctx, GACQ_ERR_HIP, "gacq_beams_open: %s", hipGetErrorString(e));
  }
  *out = h.release();
  return GACQ_OK;
}

extern "C" void gacq_beams_close(gacq_beams* h) { delete h; }

extern "C" int gacq_beams_run_dev(gacq_beams* h, const void* const* d_in, long long in_first, long long in_count, long long out_first, long long n_out,
                                  const double* gain, int out_complex64, void* const* d_out, void* d_stats, void* d_weights, void* d_cov) {
  if (!h) return GACQ_ERR_BAD_ARG;
  const gacq_beams_cfg& c = h->cfg;
  hipStream_t stream = h->ctx->stream;
  ArRun run{d_in, in_first, in_count, out_first, n_out, 1.0, out_complex64, nullptr, d_stats, d_weights, d_cov};
  run.beams = c.beams;
  run.gains = gain;
  run.d_outs = d_out;
  return ar_run_dev(
      "gacq_beams_run_dev", *h,
      [&](const gacq_beams_cfg* cf, long long a, long long b, long long o, long long n, double, int f) { return gacq_beams_check(cf, a, b, o, n, gain, f); },
      run, kArMaxChunk, wq_at(),
      [&](const ArRun& r) {
        const uint8_t* in[kArMaxM];
        ar_inputs(in, r, c.antennas, r.pb0 * c.block);
        null_launch_cov(in, r.dC, r.ncov, c.block, c.antennas, stream);
      },
      [&](const ArRun& r) {
        BmWgtArgs wg;
        ar_fill_weights(wg, c, r);
        wg.cst = (const double*)(r.dC + cst_at(c));
        wg.K = c.beams;
        hipLaunchKernelGGL(beams_weights_kernel, dim3((unsigned)((wg.nblk + kArBlock / 64 - 1) / (kArBlock / 64))), dim3(kArBlock), 0, stream, wg);
      },
      [&](const ArRun& r) {
        BmApplyArgs ap;
        ar_inputs(ap.in, r, c.antennas, r.o);
        for (int k = 0; k < kArMaxBeams; k++) {
          const int q = k < c.beams ? k : 0;
          ap.out[k] = (uint8_t*)r.d_outs[q] + (r.o - r.out_first) * (r.out_complex64 ? 8 : 2);
          ap.s[k] = r.sk[q];
        }
        ap.Wq = r.dWq;
        ap.stats = (unsigned long long*)r.d_stats;
        const long long tile0 = r.o / kArTile * kArTile;
        ap.lo = (int)(r.o - tile0);
        ap.hi = (int)(r.o_end - tile0);
        ap.boff = (int)(tile0 - r.b0 * c.block);
        ap.ntiles = (int)((r.o_end - 1 - tile0) / kArTile + 1);
        ap.owned = r.owned;
        ap.Lb = c.block;
        ap.M = c.antennas;
        ap.K = c.beams;
        if (r.out_complex64) hipLaunchKernelGGL(beams_apply_kernel<true>, dim3(r.grid), dim3(kArBlock), 0, stream, ap);
        else hipLaunchKernelGGL(beams_apply_kernel<false>, dim3(r.grid), dim3(kArBlock), 0, stream, ap);
      });
}
