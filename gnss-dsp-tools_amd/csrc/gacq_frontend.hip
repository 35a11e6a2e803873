// Front-end of the acquire scripts on the GPU (SURVEY.md section 8f "next #1", component C10):
//   int8 I/Q  ->  carrier-offset wipe-off with the fixed-point table NCO  ->  161-tap FIR applied forward-backward
//   (scipy.signal.filtfilt semantics)  ->  linear-interpolation resample to the signal's internal rate.
// Reference: acquire-gps-l1.py:78-96, gnsstools/io.py:3-12, gnsstools/nco.py:30-41.
//
// All three kernels are streaming kernels (HBM-bound at the input rate; the FIR keeps its taps and a tile + halo in LDS).
//   fe_mix_kernel       x[i] = (I + jQ) * table[((dp + i*df) >> 50) & 1023]        nco.mix_: 50-bit fixed-point phase, int64 wrap
//   fe_fir_kernel<DIR>  one direction of filtfilt over the odd-extended signal, history initialised to the edge value
//                       (that is what filtfilt's lfilter_zi initial condition means for an FIR)
//   fe_resample_kernel  np.interp at t_k = (1/fsr) * k, fp64 positions
#include "gacq_fecore.h"

#include <cmath>

using namespace gacq;

namespace {

// The kernels' bodies live in gacq_fecore.h, where the batched front-end (gacq_scan.hip) finds them too.
__global__ __launch_bounds__(kFeBlock) void fe_mix_kernel(const char2* __restrict__ iq, float2* __restrict__ out, long n, long long dp,
                                                           long long df, const float2* __restrict__ tab) {
  const long i = (long)blockIdx.x * kFeBlock + threadIdx.x;
  if (i >= n) return;
  out[i] = mix_sample(iq, i, dp, df, tab);
}

template <int PASS>
__global__ __launch_bounds__(kFeBlock) void fe_fir_kernel(const float2* __restrict__ in, float2* __restrict__ out, long n, int p,
                                                           const float* __restrict__ taps, int ntaps) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  fir_tile<PASS>(reinterpret_cast<float2*>(smem), (long)blockIdx.x, in, out, n, p, taps, ntaps);
}

template <int PASS, int NTAPS, typename Src>
__global__ __launch_bounds__(kFeBlock) void fe_fir_fixed_kernel(const Src in, float2* __restrict__ out, long n, int p,
                                                                 const float* __restrict__ taps) {
  __shared__ v2 s_x[kTileF + NTAPS - 1];
  fir_fixed_tile<PASS, NTAPS, Src>(s_x, (long)blockIdx.x, in, out, n, p, taps);
}

__global__ __launch_bounds__(kFeBlock) void fe_resample_kernel(const float2* __restrict__ y, long n, float2* __restrict__ out, long nout,
                                                                double step) {
  const long k = (long)blockIdx.x * kFeBlock + threadIdx.x;
  if (k >= nout) return;
  out[k] = resample_at(y, n, k, step);
}

}  // namespace

namespace gacq {

// nco.mix(x, -coffset/fs, 0) on int8 I/Q already on the device: dp = floor(p*NT*2^50) = 0, df = floor(f*NT*2^50)   gnsstools/nco.py:33-34
long long frontend_mix_step(double fs_in, double carrier_offset_hz) {
  const double f = -carrier_offset_hz / fs_in;
  return (long long)std::floor(f * (double)kNcoTableSize * (double)(1LL << 50));
}

// the filter in fp32 in ctx->fe_taps
int frontend_taps(gacq_ctx* ctx, const double* taps, int ntaps) {
  int rc;
  if ((rc = ensure(ctx, ctx->fe_taps, sizeof(float) * kMaxTaps)) != GACQ_OK) return rc;
  std::vector<float> h(ntaps);
  for (int i = 0; i < ntaps; i++) h[i] = (float)taps[i];
  if (h != ctx->up_taps) {
    GACQ_HIP(ctx, hipMemcpyAsync(ctx->fe_taps.p, h.data(), sizeof(float) * ntaps, hipMemcpyHostToDevice, ctx->stream));
    GACQ_HIP(ctx, hipStreamSynchronize(ctx->stream));   // h dies with this frame; a repeated filter skips copy and sync
    ctx->up_taps = h;
  }
  return GACQ_OK;
}

int frontend_mix(gacq_ctx* ctx, const void* d_iq_int8, long n, double fs_in, double carrier_offset_hz, float2* d_out) {
  const long long df = frontend_mix_step(fs_in, carrier_offset_hz);
  hipLaunchKernelGGL(fe_mix_kernel, dim3((unsigned)((n + kFeBlock - 1) / kFeBlock)), dim3(kFeBlock), 0, ctx->stream, (const char2*)d_iq_int8, d_out, n,
                     0LL, df, (const float2*)ctx->tab.p);
  GACQ_HIP(ctx, hipGetLastError());
  return GACQ_OK;
}

}  // namespace gacq

extern "C" {

// scipy.signal.firwin(ntaps, cutoff_norm, window='hann') (low-pass, unity DC gain); cutoff_norm = cutoff / (fs/2)
int gacq_firwin_hann(int ntaps, double cutoff_norm, double* taps) {
  if (ntaps < 3 || ntaps > kMaxTaps || !(cutoff_norm > 0.0 && cutoff_norm < 1.0) || !taps)
    return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_firwin_hann: bad argument");
  const double alpha = 0.5 * (ntaps - 1);
  double sum = 0.0;
  for (int i = 0; i < ntaps; i++) {
    const double m = (double)i - alpha;
    const double arg = cutoff_norm * m;
    const double sinc = (arg == 0.0) ? 1.0 : std::sin(M_PI * arg) / (M_PI * arg);
    const double win = 0.5 - 0.5 * std::cos(2.0 * M_PI * (double)i / (double)(ntaps - 1));      // symmetric Hann
    taps[i] = cutoff_norm * sinc * win;
    sum += taps[i];
  }
  for (int i = 0; i < ntaps; i++) taps[i] /= sum;
  return GACQ_OK;
}

int gacq_frontend_dev(gacq_ctx* ctx, const void* d_iq_int8, size_t nsamp_in, double fs_in, double carrier_offset_hz,
                      const double* taps, int ntaps, double fs_out, size_t nsamp_out, void* d_out) {
  if (!ctx || !d_iq_int8 || !taps || !d_out || ntaps < 1 || ntaps > kMaxTaps || !(fs_in > 0.0) || !(fs_out > 0.0) || nsamp_out == 0)
    return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_frontend_dev: bad argument");
  const int p = 3 * ntaps;                              // filtfilt default padlen = 3*max(len(a), len(b))
  if (nsamp_in <= (size_t)p)
    return set_error(ctx, GACQ_ERR_SHORT_INPUT, "gacq_frontend_dev: %zu input samples, filtfilt needs more than %d", nsamp_in, p);
  GACQ_DEVICE(ctx);
  hipStream_t st = ctx->stream;
  const long n = (long)nsamp_in, L = n + 2L * p;
  int rc;
  if ((rc = ensure(ctx, ctx->fe_a, sizeof(float2) * (size_t)n)) != GACQ_OK) return rc;
  if ((rc = ensure(ctx, ctx->fe_b, sizeof(float2) * (size_t)L)) != GACQ_OK) return rc;
  if ((rc = frontend_taps(ctx, taps, ntaps)) != GACQ_OK) return rc;
  float2* a = (float2*)ctx->fe_a.p;
  float2* b = (float2*)ctx->fe_b.p;
  if (ntaps == 161 && !ctx->opt[GACQ_OPT_FE_GENERIC]) {
    // the reference's filter length: mix + forward pass in one kernel, then the backward pass (fe_fir_fixed_kernel)
    MixedInput src;
    src.iq = (const char2*)d_iq_int8;
    src.dp = 0LL;                                                                      // nco.mix(x, f, 0): phase 0
    src.df = gacq::frontend_mix_step(fs_in, carrier_offset_hz);
    src.tab = (const float2*)ctx->tab.p;
    hipLaunchKernelGGL((fe_fir_fixed_kernel<1, 161, MixedInput>), dim3((unsigned)((L + kTileF - 1) / kTileF)), dim3(kFeBlock), 0, st, src, b, n, p,
                       (const float*)ctx->fe_taps.p);
    GACQ_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL((fe_fir_fixed_kernel<2, 161, const float2*>), dim3((unsigned)((n + kTileF - 1) / kTileF)), dim3(kFeBlock), 0, st,
                       (const float2*)b, a, n, p, (const float*)ctx->fe_taps.p);
    GACQ_HIP(ctx, hipGetLastError());
  } else {
    if ((rc = frontend_mix(ctx, d_iq_int8, n, fs_in, carrier_offset_hz, a)) != GACQ_OK) return rc;
    const int tile_elems = kTile + ntaps;
    const size_t smem = sizeof(float2) * (size_t)(tile_elems + tile_elems / 32 + 2);
    hipLaunchKernelGGL(fe_fir_kernel<1>, dim3((unsigned)((L + kTile - 1) / kTile)), dim3(kFeBlock), smem, st, (const float2*)a, b, n, p,
                       (const float*)ctx->fe_taps.p, ntaps);
    GACQ_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(fe_fir_kernel<2>, dim3((unsigned)((n + kTile - 1) / kTile)), dim3(kFeBlock), smem, st, (const float2*)b, a, n, p,
                       (const float*)ctx->fe_taps.p, ntaps);
    GACQ_HIP(ctx, hipGetLastError());
  }
  const double fsr = fs_out / fs_in;                    // acquire-gps-l1.py:91
  hipLaunchKernelGGL(fe_resample_kernel, dim3((unsigned)((nsamp_out + kFeBlock - 1) / kFeBlock)), dim3(kFeBlock), 0, st, (const float2*)a, n,
                     (float2*)d_out, (long)nsamp_out, 1.0 / fsr);
  GACQ_HIP(ctx, hipGetLastError());
  return GACQ_OK;
}

}  // extern "C"
