// Front-end for many windows of one recording at once (gacq_frontend_batch_dev, include/gacq.h): window w is the nsamp_in samples that
// begin at sample starts[w] of the int8 recording, and row w of the output is what gacq_frontend_dev writes for that slice, bit for bit
// -- the mixer phase restarts at 0 in every window, every window has its own odd extension, and the device code is the text both files
// inline from gacq_fecore.h.  The window axis is the grid's y dimension: one launch set serves all windows of a chunk.
//
//   161 taps (the reference's filter):
//     scan_fe_fir1_fixed_kernel      mix + forward pass, as fe_fir_fixed_kernel<1>                      int8 -> y1 [W][n + 2p]
//     scan_fe_back_resample_kernel   backward pass + np.interp in one: output k needs y[i], y[i+1] for i = floor(step*k) only, so each
//                                    thread runs the two tap chains of its own output from a tile of y1 in LDS.  Going down in rate
//                                    (69.984 -> 4.096 MS/s) that is 2 of every ~17 backward outputs; the backward pass's full-rate
//                                    output buffer does not exist.                                       y1 -> out [W][nsamp_out]
//   any other tap count, or GACQ_OPT_FE_GENERIC: mix, forward, backward and resample kernels as in gacq_frontend.hip, batched.
#include "gacq_fecore.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace gacq;

namespace {

constexpr int kScanMaxWin = 32768;      // windows per launch set (grid y)

__global__ __launch_bounds__(kFeBlock) void scan_fe_mix_kernel(const char2* __restrict__ iq, const long long* __restrict__ starts,
                                                                float2* __restrict__ out, long n, long long df, const float2* __restrict__ tab) {
  const long i = (long)blockIdx.x * kFeBlock + threadIdx.x;
  if (i >= n) return;
  out[(size_t)blockIdx.y * n + i] = mix_sample(iq + starts[blockIdx.y], i, 0LL, df, tab);
}

template <int PASS>
__global__ __launch_bounds__(kFeBlock) void scan_fe_fir_kernel(const float2* __restrict__ in, float2* __restrict__ out, long n, int p,
                                                                const float* __restrict__ taps, int ntaps) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const size_t L = (size_t)n + 2 * (size_t)p, w = blockIdx.y;
  fir_tile<PASS>(reinterpret_cast<float2*>(smem), (long)blockIdx.x, in + w * (PASS == 1 ? (size_t)n : L), out + w * (PASS == 1 ? L : (size_t)n), n, p,
                 taps, ntaps);
}

template <int NTAPS>
__global__ __launch_bounds__(kFeBlock) void scan_fe_fir1_fixed_kernel(const char2* __restrict__ iq, const long long* __restrict__ starts,
                                                                       float2* __restrict__ y1, long n, int p, long long df,
                                                                       const float2* __restrict__ tab, const float* __restrict__ taps) {
  __shared__ v2 s_x[kTileF + NTAPS - 1];
  MixedInput src;
  src.iq = iq + starts[blockIdx.y];
  src.dp = 0LL;                                           // nco.mix(x, f, 0): the phase restarts in every window
  src.df = df;
  src.tab = tab;
  fir_fixed_tile<1, NTAPS, MixedInput>(s_x, (long)blockIdx.x, src, y1 + (size_t)blockIdx.y * ((size_t)n + 2 * (size_t)p), n, p, taps);
}

__global__ __launch_bounds__(kFeBlock) void scan_fe_resample_kernel(const float2* __restrict__ y, long n, float2* __restrict__ out, long nout,
                                                                     double step) {
  const long k = (long)blockIdx.x * kFeBlock + threadIdx.x;
  if (k >= nout) return;
  out[(size_t)blockIdx.y * nout + k] = resample_at(y + (size_t)blockIdx.y * n, n, k, step);
}

// smallest k >= 0 whose resampling position step*k, rounded as the resampler rounds it, reaches `a`
__device__ __forceinline__ long first_output_at(double step, double a) {
  long k = (long)ceil(a / step);
  if (k < 0) k = 0;
  while (k > 0 && __dmul_rn(step, (double)(k - 1)) >= a) k--;
  while (__dmul_rn(step, (double)k) < a) k++;
  return k;
}

// Backward pass and resampler in one.  Workgroup (tile, window) owns the outputs whose left neighbour y[i] lies in [tile*T, tile*T + T);
// the last tile also owns the outputs np.interp clamps to y[n-1].  It loads y1[i0+p .. i0+p+T+NTAPS) once, and every thread runs
//   y[i] = sum_k h[k] y1[i+p+k],  y[i+1] = sum_k h[k] y1[i+1+p+k]      (taps ascending, fmaf chains from zero: the backward pass's bits)
// for its own output; the two chains share all but one LDS read.  Outputs are walked with the block's stride, so the same kernel
// serves a resampler that goes up in rate (several outputs per y pair, more than kFeBlock outputs per tile).
// The tile is dynamic LDS, (T + NTAPS) elements: 3.3 KB at T = 256 (going up in rate, or down by little), 34 KB at the cap.
constexpr int kScanMaxT = 4096;
template <int NTAPS>
__global__ __launch_bounds__(kFeBlock) void scan_fe_back_resample_kernel(const float2* __restrict__ y1, float2* __restrict__ out, long n, int p,
                                                                          long nout, double step, int T, const float* __restrict__ taps) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  v2* s_y = reinterpret_cast<v2*>(smem);
  const long L = n + 2 * (long)p;
  const float2* yw = y1 + (size_t)blockIdx.y * (size_t)L;
  float2* ow = out + (size_t)blockIdx.y * (size_t)nout;
  const long i0 = (long)blockIdx.x * T;
  for (int m = threadIdx.x; m < T + NTAPS; m += kFeBlock) {
    const long idx = i0 + p + m;
    const float2 v = yw[idx >= L ? L - 1 : idx];          // y1[m >= L] := y1[L-1], as the backward pass
    s_y[m] = v2{v.x, v.y};
  }
  __syncthreads();
  const long k_lo = first_output_at(step, (double)i0);
  const long k_hi = blockIdx.x == gridDim.x - 1 ? nout : min(nout, first_output_at(step, (double)(i0 + T)));
  for (long k = k_lo + threadIdx.x; k < k_hi; k += kFeBlock) {
    const double t = __dmul_rn(step, (double)k);
    const bool clamped = t >= (double)(n - 1);            // np.interp: fp[-1] right of the last sample
    const long i = clamped ? n - 2 : (long)floor(t);
    const v2* sp = s_y + (int)(i - i0);
    v2 a0 = v2{0.f, 0.f}, a1 = v2{0.f, 0.f}, prev = sp[0];
#pragma unroll 7
    for (int j = 0; j < NTAPS; j++) {
      const float h = taps[j];
      const v2 cur = sp[j + 1];
      a0 = v2{fmaf(h, prev.x, a0.x), fmaf(h, prev.y, a0.y)};
      a1 = v2{fmaf(h, cur.x, a1.x), fmaf(h, cur.y, a1.y)};
      prev = cur;
    }
    const float2 ya = make_float2(a0.x, a0.y), yb = make_float2(a1.x, a1.y);
    ow[k] = clamped ? yb : interp_pair(ya, yb, t, i);
  }
}

}  // namespace

namespace gacq {

int frontend_batch_check(gacq_ctx* ctx, const void* d_iq_int8, long long nsamp_avail, const long long* starts, int nwin, size_t nsamp_in,
                         double fs_in, double carrier_offset_hz, const double* taps, int ntaps, double fs_out, size_t nsamp_out, const void* d_out) {
  if (!ctx) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_frontend_batch_dev: ctx is NULL");
  if (!d_iq_int8 || !starts || !taps || !d_out || nwin < 1 || ntaps < 1 || ntaps > kMaxTaps || !(fs_in > 0.0) || !(fs_out > 0.0) ||
      !std::isfinite(fs_in) || !std::isfinite(fs_out) || !std::isfinite(carrier_offset_hz) || nsamp_out == 0)
    return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_frontend_batch_dev: bad argument");
  if (nsamp_in <= (size_t)(3 * ntaps))
    return set_error(ctx, GACQ_ERR_SHORT_INPUT, "gacq_frontend_batch_dev: %zu input samples per window, filtfilt needs more than %d", nsamp_in,
                     3 * ntaps);
  for (int w = 0; w < nwin; w++)
    if (starts[w] < 0 || nsamp_avail < 0 || (unsigned long long)starts[w] + nsamp_in > (unsigned long long)nsamp_avail)
      return set_error(ctx, GACQ_ERR_SHORT_INPUT, "gacq_frontend_batch_dev: window %d: %zu samples from %lld needed, %lld available", w, nsamp_in,
                       starts[w], nsamp_avail);
  return GACQ_OK;
}

}  // namespace gacq

extern "C" int gacq_frontend_batch_dev(gacq_ctx* ctx, const void* d_iq_int8, long long nsamp_avail, const long long* starts, int nwin,
                                       size_t nsamp_in, double fs_in, double carrier_offset_hz, const double* taps, int ntaps, double fs_out,
                                       size_t nsamp_out, void* d_out) {
  // everything is checked before anything is allocated or launched
  int rc = frontend_batch_check(ctx, d_iq_int8, nsamp_avail, starts, nwin, nsamp_in, fs_in, carrier_offset_hz, taps, ntaps, fs_out, nsamp_out, d_out);
  if (rc != GACQ_OK) return rc;
  GACQ_DEVICE(ctx);
  hipStream_t st = ctx->stream;
  const int p = 3 * ntaps;                               // filtfilt default padlen
  const long n = (long)nsamp_in, L = n + 2L * p, nout = (long)nsamp_out;
  const bool fused = ntaps == 161 && !ctx->opt[GACQ_OPT_FE_GENERIC];
  // windows per launch set: the intermediates of a chunk -- y1 [W][L], and on the generic path the mixed signal / backward output
  // [W][n] -- come out of the workspace budget
  const size_t per_win = sizeof(float2) * ((size_t)L + (fused ? 0 : (size_t)n));
  const int Wc = (int)std::max<size_t>(1, std::min<size_t>(std::min(nwin, kScanMaxWin), ws_budget(ctx) / per_win));
  if ((rc = ensure(ctx, ctx->fe_b, sizeof(float2) * (size_t)L * Wc)) != GACQ_OK) return rc;
  if (!fused && (rc = ensure(ctx, ctx->fe_a, sizeof(float2) * (size_t)n * Wc)) != GACQ_OK) return rc;
  if ((rc = frontend_taps(ctx, taps, ntaps)) != GACQ_OK) return rc;
  // the window starts are staged in pinned memory, two slots in turn, as gacq_fold_dev does: a slot is rewritten only after the
  // launches that last used it have finished (its event), so the call returns as soon as the copy and the kernels are queued
  const int slot = ctx->scan_slot;
  if (ctx->scan_done[slot]) GACQ_HIP(ctx, hipEventSynchronize(ctx->scan_done[slot]));
  else GACQ_HIP(ctx, hipEventCreateWithFlags(&ctx->scan_done[slot], hipEventDisableTiming));
  DevBuf& d_par = ctx->tables[slot ? "scan:starts1" : "scan:starts0"];
  const size_t bytes = sizeof(long long) * (size_t)nwin;
  // a failure here returns without recording the slot's event: nothing has been queued yet, and waiting for an unrecorded event returns at once
  if ((rc = ensure_pinned(ctx, ctx->pin_scan[slot], bytes)) != GACQ_OK) return rc;
  if ((rc = ensure(ctx, d_par, bytes)) != GACQ_OK) return rc;
  std::memcpy(ctx->pin_scan[slot].p, starts, bytes);
  // from here on the slot's pinned block may be in use by a queued copy: the event is recorded on every way out, failures included
  hipError_t e = hipMemcpyAsync(d_par.p, ctx->pin_scan[slot].p, bytes, hipMemcpyHostToDevice, st);
  const char2* iq = (const char2*)d_iq_int8;
  const float2* tab = (const float2*)ctx->tab.p;
  const float* h = (const float*)ctx->fe_taps.p;
  float2* a = (float2*)ctx->fe_a.p;
  float2* b = (float2*)ctx->fe_b.p;
  const long long df = frontend_mix_step(fs_in, carrier_offset_hz);
  const double step = 1.0 / (fs_out / fs_in);            // acquire-gps-l1.py:91,94, as gacq_frontend_dev
  for (int w0 = 0; w0 < nwin && e == hipSuccess; w0 += Wc) {
    const unsigned W = (unsigned)std::min(Wc, nwin - w0);
    const long long* d_starts = (const long long*)d_par.p + w0;
    float2* o = (float2*)d_out + (size_t)w0 * nsamp_out;
    if (fused) {
      hipLaunchKernelGGL((scan_fe_fir1_fixed_kernel<161>), dim3((unsigned)((L + kTileF - 1) / kTileF), W), dim3(kFeBlock), 0, st, iq, d_starts, b, n, p,
                         df, tab, h);
      // input tile of a workgroup: about kFeBlock outputs' worth of y going down in rate, never less than kFeBlock samples
      const int T = (int)std::min<double>(kScanMaxT, std::max<double>(kFeBlock, std::ceil(kFeBlock * step)));
      hipLaunchKernelGGL((scan_fe_back_resample_kernel<161>), dim3((unsigned)((n - 1 + T - 1) / T), W), dim3(kFeBlock), sizeof(float2) * (size_t)(T + 161), st, (const float2*)b, o, n,
                         p, nout, step, T, h);
    } else {
      hipLaunchKernelGGL(scan_fe_mix_kernel, dim3((unsigned)((n + kFeBlock - 1) / kFeBlock), W), dim3(kFeBlock), 0, st, iq, d_starts, a, n, df, tab);
      const int tile_elems = kTile + ntaps;
      const size_t smem = sizeof(float2) * (size_t)(tile_elems + tile_elems / 32 + 2);
      hipLaunchKernelGGL(scan_fe_fir_kernel<1>, dim3((unsigned)((L + kTile - 1) / kTile), W), dim3(kFeBlock), smem, st, (const float2*)a, b, n, p, h,
                         ntaps);
      hipLaunchKernelGGL(scan_fe_fir_kernel<2>, dim3((unsigned)((n + kTile - 1) / kTile), W), dim3(kFeBlock), smem, st, (const float2*)b, a, n, p, h,
                         ntaps);
      hipLaunchKernelGGL(scan_fe_resample_kernel, dim3((unsigned)((nout + kFeBlock - 1) / kFeBlock), W), dim3(kFeBlock), 0, st, (const float2*)a, n, o,
                         nout, step);
    }
    e = hipGetLastError();
  }
  const hipError_t e2 = hipEventRecord(ctx->scan_done[slot], st);
  if (e != hipSuccess) return set_error(ctx, GACQ_ERR_HIP, "gacq_frontend_batch_dev: upload or launch failed: %s", hipGetErrorString(e));
  GACQ_HIP(ctx, e2);
  ctx->scan_slot = slot ^ 1;
  return GACQ_OK;
}
