// Coherent fold of M code periods ahead of the search (gacq_fold_dev, include/gacq.h).  For D Doppler values f_d, H sign patterns
// W[h][m] in {-1, 0, +1} and a start table start[d][m] (samples of x; j0 = absolute index of x[0]),
//   y[d,h,i] = sum_{m<M} W[h,m] x[start[d,m] + i] exp(-2 pi i frac(f_d (j0 + start[d,m] + i) / fs)),   0 <= i < n_out.
// The correlation of y[d,h] with a code is the coherent sum, under sign pattern h, of the correlations of the M carrier-wiped periods.
//
// A lane owns kIpl values of i, 256 apart, and for each tile of TH hypotheses (8, 16, 24 or 32: the narrowest that holds H in ceil(H / 32) tiles) a register tile of kIpl x TH complex fp32 accumulators.
// It walks m: loads its samples (8-byte loads, coalesced along i, whatever the parity of start), rotates each once and adds it into
// every accumulator of the tile with a fused multiply-add by the weight -1, 0 or +1 -- exact, so an accumulator is the running sum
// rounded once per period, in the order of m.  The weights of a (tile, m) are TH consecutive floats that every lane reads at the same
// address: wave-uniform, no per-lane gather.  H > TH loops over tiles and forms the rotations again.
//
// Phase: a 64-bit fixed-point fraction of a cycle, exact per sample and reduced before anything becomes fp32.  The host forms
// S = frac(f_d / fs) 2^128 in two extended-precision pieces, base[d][m] = (j0 + start[d][m]) S / 2^64 mod 2^64 in integer arithmetic
// and step[d] = S / 2^64 rounded; a lane adds i step[d].  Nothing on the Doppler axis comes from a neighbouring bin.  The top bits
// pick the nearest quarter turn, the remaining 30 go through polynomials for sin / cos of (pi/2) t, |t| <= 1/2 (1e-7 absolute):
// turn_sincos of gacq_turn.h, the scheme of gacq_corrgrid.hip with longer polynomials (that file keeps its own).
//
// Every output element is the same chain of operations whatever D, H, the tile, the lanes per sample or the caller's chunking of d
// are: its bits depend on row d's inputs and W[h] alone.  No atomics, no LDS.
#pragma clang fp contract(off)

#include "gacq_common.h"
#include "gacq_turn.h"

#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

using namespace gacq;

namespace {

constexpr int kFoldBlock = 256;
constexpr int kFoldMaxM = 128;
constexpr int kFoldMaxH = 256;
constexpr int kFoldTileMax = 32;

template <bool WIDE>
__device__ __forceinline__ float2 fold_load(const void* __restrict__ x, long long j) {
  if (WIDE) {
    const double2 v = reinterpret_cast<const double2*>(x)[j];
    return make_float2((float)v.x, (float)v.y);                   // complex128 input: rounded once, here
  }
  return reinterpret_cast<const float2*>(x)[j];
}

// grid: D * nblk workgroups, nblk = ceil(n_out / (256 IPL)); workgroup bid serves row d = bid / nblk
template <int TH, int IPL, bool WIDE>
__global__ __launch_bounds__(kFoldBlock) void cohfold_kernel(const void* __restrict__ x, const unsigned long long* __restrict__ step,
                                                             const unsigned long long* __restrict__ base, const long long* __restrict__ start,
                                                             const float* __restrict__ wf, float2* __restrict__ y, int n_out, int M, int H,
                                                             int nblk) {
  const int d = (int)(blockIdx.x / (unsigned)nblk);
  const int bi = (int)(blockIdx.x - (unsigned)d * (unsigned)nblk);
  const unsigned long long st = step[d];
  const unsigned long long* __restrict__ bd = base + (long long)d * M;
  const long long* __restrict__ sd = start + (long long)d * M;
  int ii[IPL];
  bool ok[IPL];
  unsigned long long ps[IPL];
#pragma unroll
  for (int k = 0; k < IPL; k++) {
    const int i = bi * (kFoldBlock * IPL) + k * kFoldBlock + (int)threadIdx.x;
    ok[k] = i < n_out;
    ii[k] = ok[k] ? i : n_out - 1;                                // a lane past the row's end repeats the last sample and stores nothing
    ps[k] = (unsigned long long)ii[k] * st;
  }
  for (int h0 = 0; h0 < H; h0 += TH) {
    float ar[IPL][TH], ai[IPL][TH];
#pragma unroll
    for (int k = 0; k < IPL; k++) {
#pragma unroll
      for (int h = 0; h < TH; h++) ar[k][h] = ai[k][h] = 0.0f;
    }
    const float* __restrict__ wt = wf + (long long)(h0 / TH) * M * TH;
    for (int m = 0; m < M; m++) {
      const long long s0 = sd[m];
      const unsigned long long b0 = bd[m];
      float vr[IPL], vi[IPL];
#pragma unroll
      for (int k = 0; k < IPL; k++) {
        const float2 v = fold_load<WIDE>(x, s0 + ii[k]);
        float c, s;
        turn_sincos(b0 + ps[k], c, s);
        vr[k] = fmaf(v.y, s, v.x * c);                            // x exp(-i phi)
        vi[k] = fmaf(-v.x, s, v.y * c);
      }
#pragma unroll
      for (int h = 0; h < TH; h++) {
        const float w = wt[m * TH + h];                           // the same address in every lane
#pragma unroll
        for (int k = 0; k < IPL; k++) {
          ar[k][h] = fmaf(w, vr[k], ar[k][h]);
          ai[k][h] = fmaf(w, vi[k], ai[k][h]);
        }
      }
    }
#pragma unroll
    for (int h = 0; h < TH; h++) {
      if (h0 + h < H) {
        float2* __restrict__ row = y + ((long long)d * H + (h0 + h)) * n_out;
#pragma unroll
        for (int k = 0; k < IPL; k++)
          if (ok[k]) row[ii[k]] = make_float2(ar[k][h], ai[k][h]);
      }
    }
  }
}

// S = frac(f / fs) 2^128 as hi:lo, from the extended-precision quotient and its exact remainder
void fold_step128(double f, double fs, unsigned long long& hi, unsigned long long& lo) {
  const long double two64 = 18446744073709551616.0L;
  const long double a = fabsl((long double)f), b = (long double)fs;
  const long double q = a / b;
  const long double r = fmal(-q, b, a) / b;                       // a / b = q + r, |r| <= ulp(q) / 2
  const long double t = q - floorl(q);                            // exact
  long double A = floorl(t * two64);                              // the scaling is exact
  long double B = ((t * two64 - A) + r * two64) * two64;          // [-eps, 2^64 + eps]
  if (B < 0.0L) {
    if (A >= 1.0L) { A -= 1.0L; B += two64; } else B = 0.0L;
  }
  if (B >= two64) { A += 1.0L; B -= two64; }
  hi = A >= two64 ? 0ull : (unsigned long long)A;                 // a carry out of the top is a whole cycle
  lo = B >= 18446744073709551615.0L ? ~0ull : (unsigned long long)B;
  if (f < 0.0) {                                                  // frac(-v) = 1 - frac(v): two's complement of the 128 bits
    lo = ~lo + 1ull;
    hi = ~hi + (lo == 0ull ? 1ull : 0ull);
  }
}

// J S / 2^64 mod 2^64
unsigned long long fold_base(long long J, unsigned long long hi, unsigned long long lo) {
  const bool neg = J < 0;
  const unsigned long long j = neg ? 0ull - (unsigned long long)J : (unsigned long long)J;
  const unsigned long long v = j * hi + (unsigned long long)(((unsigned __int128)j * lo) >> 64);
  return neg ? 0ull - v : v;
}

template <int TH, int IPL>
void fold_launch(bool wide, unsigned grid, hipStream_t stream, const void* x, const unsigned long long* step, const unsigned long long* base,
                 const long long* start, const float* wf, float2* y, int n_out, int M, int H, int nblk) {
  if (wide)
    hipLaunchKernelGGL((cohfold_kernel<TH, IPL, true>), dim3(grid), dim3(kFoldBlock), 0, stream, x, step, base, start, wf, y, n_out, M, H, nblk);
  else
    hipLaunchKernelGGL((cohfold_kernel<TH, IPL, false>), dim3(grid), dim3(kFoldBlock), 0, stream, x, step, base, start, wf, y, n_out, M, H, nblk);
}

}  // namespace

extern "C" int gacq_fold_dev(gacq_ctx* ctx, const void* d_x, int wide, long long avail, int n_out, int M, int D, int H, const long long* start,
                             const double* f_d, double fs, long long j0, const signed char* W, void* d_y) {
  if (!ctx) return GACQ_ERR_BAD_ARG;
  if (!d_x || !start || !f_d || !W || !d_y) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_fold_dev: NULL argument");
  // everything is checked before anything is allocated or launched
  if (n_out < 1 || M < 1 || D < 1 || H < 1 || M > kFoldMaxM || H > kFoldMaxH)
    return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_fold_dev: need n_out >= 1, 1 <= M <= %d, D >= 1, 1 <= H <= %d (n_out %d, M %d, D %d, H %d)",
                     kFoldMaxM, kFoldMaxH, n_out, M, D, H);
  if (!std::isfinite(fs) || !(fs > 0.0)) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_fold_dev: fs must be finite and positive");
  if (j0 < -(1ll << 62) || j0 > (1ll << 62)) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_fold_dev: j0 = %lld is outside +-2^62", j0);
  const int ipl = n_out >= 16384 ? 2 : 1;
  // tiles of 8, 16, 24 or 32 hypotheses: as few tiles as 32 allow, then the narrowest width that holds H in them
  const int ntile = (H + kFoldTileMax - 1) / kFoldTileMax;
  const int th = ((H + ntile - 1) / ntile + 7) / 8 * 8;
  const int nblk = (int)(((long long)n_out + kFoldBlock * ipl - 1) / (kFoldBlock * ipl));
  if ((long long)nblk * D > 0x7fffffffll) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_fold_dev: more than 2^31 - 1 workgroups (D %d, n_out %d)", D, n_out);
  for (int d = 0; d < D; d++)
    if (!std::isfinite(f_d[d])) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_fold_dev: Doppler value %d is not finite", d);
  for (long k = 0; k < (long)H * M; k++)
    if (W[k] < -1 || W[k] > 1) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_fold_dev: W[%ld][%ld] = %d is outside -1..1", k / M, k % M, (int)W[k]);
  for (long k = 0; k < (long)D * M; k++)
    if (start[k] < 0 || start[k] > avail - n_out)
      return set_error(ctx, GACQ_ERR_SHORT_INPUT, "gacq_fold_dev: row %ld, period %ld: samples [%lld, %lld) needed, %lld available", k / M, k % M,
                       start[k], start[k] + n_out, avail);
  const size_t o_step = 0, o_base = o_step + sizeof(unsigned long long) * (size_t)D, o_start = o_base + sizeof(unsigned long long) * (size_t)D * M,
               o_w = o_start + sizeof(long long) * (size_t)D * M, bytes = o_w + sizeof(float) * (size_t)ntile * M * th;
  GACQ_DEVICE(ctx);
  hipStream_t stream = ctx->stream;
  // the parameter block is staged in pinned memory, two slots in turn: a slot is rewritten only after the launch that last used it has
  // finished (its event), so the call returns as soon as the copy and the kernel are queued
  const int slot = ctx->fold_slot;
  if (ctx->fold_done[slot]) GACQ_HIP(ctx, hipEventSynchronize(ctx->fold_done[slot]));
  else GACQ_HIP(ctx, hipEventCreateWithFlags(&ctx->fold_done[slot], hipEventDisableTiming));
  DevBuf& d_par = ctx->tables[slot ? "cohfold:params1" : "cohfold:params0"];
  int rc;
  if ((rc = ensure_pinned(ctx, ctx->pin_fold[slot], bytes)) != GACQ_OK) return rc;
  if ((rc = ensure(ctx, d_par, bytes)) != GACQ_OK) return rc;
  unsigned char* host = (unsigned char*)ctx->pin_fold[slot].p;
  unsigned long long* h_step = (unsigned long long*)(host + o_step);
  unsigned long long* h_base = (unsigned long long*)(host + o_base);
  float* h_w = (float*)(host + o_w);
  for (int d = 0; d < D; d++) {
    unsigned long long hi, lo;
    fold_step128(f_d[d], fs, hi, lo);
    h_step[d] = hi + (lo >> 63);
    for (int m = 0; m < M; m++) h_base[(size_t)d * M + m] = fold_base(j0 + start[(size_t)d * M + m], hi, lo);
  }
  std::memcpy(host + o_start, start, sizeof(long long) * (size_t)D * M);
  for (int t = 0; t < ntile; t++)
    for (int m = 0; m < M; m++)
      for (int h = 0; h < th; h++) h_w[((size_t)t * M + m) * th + h] = t * th + h < H ? (float)W[(size_t)(t * th + h) * M + m] : 0.0f;
  // from here on the slot's pinned block may be in use by a queued copy: the event is recorded on every way out, failures included
  hipError_t e = hipMemcpyAsync(d_par.p, host, bytes, hipMemcpyHostToDevice, stream);
  if (e != hipSuccess) {
    (void)hipEventRecord(ctx->fold_done[slot], stream);
    return set_error(ctx, GACQ_ERR_HIP, "gacq_fold_dev: parameter upload failed: %s", hipGetErrorString(e));
  }
  const unsigned char* p = (const unsigned char*)d_par.p;
  const unsigned grid = (unsigned)((long long)nblk * D);
  const auto go = [&](auto TH, auto IPL) {
    fold_launch<decltype(TH)::value, decltype(IPL)::value>(wide != 0, grid, stream, d_x, (const unsigned long long*)(p + o_step),
                                                           (const unsigned long long*)(p + o_base), (const long long*)(p + o_start),
                                                           (const float*)(p + o_w), (float2*)d_y, n_out, M, H, nblk);
  };
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  const auto width = [&](auto IPL) {
    switch (th) {
      case 8: go(std::integral_constant<int, 8>{}, IPL); break;
      case 16: go(std::integral_constant<int, 16>{}, IPL); break;
      case 24: go(std::integral_constant<int, 24>{}, IPL); break;
      default: go(std::integral_constant<int, 32>{}, IPL); break;
    }
  };
  if (ipl == 1) width(I1{}); else width(I2{});
  e = hipGetLastError();
  const hipError_t e2 = hipEventRecord(ctx->fold_done[slot], stream);
  if (e != hipSuccess) return set_error(ctx, GACQ_ERR_HIP, "gacq_fold_dev: launch failed: %s", hipGetErrorString(e));
  GACQ_HIP(ctx, e2);
  ctx->fold_slot = slot ^ 1;
  return GACQ_OK;
}
