// Device-resident tracking loops: the template family of the reference's track-*.py scripts (track-gps-l1.py:33-94 and the 27
// scripts that differ from it only in constants), one workgroup per channel, each walking its own blocks with no host round trip.
//
// Per outer block (one code period, or 4 / 10 / 20 of them for E1B/E1C, L1C/B1C, L2CM) the workgroup
//   1. takes the block length from code_p, exactly as the script writes it: int(fs*period*(L-code_p)/L) (or 2L-code_p);
//   2. mixes the offset wipe-off over the whole block and, per sub-block, the carrier wipe-off -- both the 50-bit fixed-point
//      table NCO of gnsstools/nco.py:30-41, each product a complex128 multiply (complex128 table) rounded to complex64, as the
//      reference stores it into its c8 array;
//   3. forms early / prompt / late with the closed-form phases of gacq_tracking.hip (floor(fma(incr, i, cp0)) mod L), the chip
//      weight in fp64 as the reference's complex64 x float64 product has it, and sums them in fp64;
//   4. lets lane 0 run the FLL / PLL / DLL update of the script in the script's own evaluation order, and writes one record.
// The state lives in device memory between launches; a launch stops a channel at the first block its samples cannot fill, after
// max_records records, or -- with a status code -- at a block length that is NaN or not positive or an NCO phase out of range.
// Nothing waits on another workgroup and every loop is bounded by max_records and by the samples given.
//
// Contraction is off for the whole file: the loop update must round every product and sum on its own (a*b+c as the script has
// it); the phases that are fused on purpose are spelled as fma().
#pragma clang fp contract(off)

#include "gacq_common.h"
#include "gacq_fft64.h"
#include "gacq_trackcore.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace gacq;

namespace {

constexpr int kTlBlock = 256;
constexpr int kMaxChips = 10240;              // the longest in-scope code is 10230 chips

__global__ __launch_bounds__(kTlBlock) void track_loop_kernel(const TlSpec* __restrict__ specs, const TlRun* __restrict__ runs,
                                                              gacq_track_chstate* __restrict__ states, const double2* __restrict__ nco_tab,
                                                              gacq_track_record* __restrict__ recs, int rec_cap,
                                                              int max_records) {
  __shared__ double2 s_tab[kNT];
  __shared__ uint8_t s_chips[kMaxChips];
  __shared__ double s_red[6][kTlBlock / 16];
  __shared__ double s_sum[6];
  __shared__ gacq_track_chstate st;
  __shared__ TlSpec sp;               // read from LDS where used: a copy in registers overflows the SGPR file
  const int ch = blockIdx.x;
  const int tid = threadIdx.x;
  const TlRun run = runs[ch];
  if (tid == 0) {
    st = states[ch];
    sp = specs[ch];
  }
  for (int k = tid; k < kNT; k += kTlBlock) s_tab[k] = nco_tab[k];
  __syncthreads();
  for (int k = tid; k < sp.L; k += kTlBlock) s_chips[k] = sp.chips[k];
  __syncthreads();
  const long L = sp.L;
  const double Ld = (double)sp.L;
  const double inv_l = 1.0 / Ld;
  const double fs = sp.fs;
  int nrec = 0;
  // every record is one track() call (1 ms of signal in every template script): an outer block runs only if all its records fit
  while (nrec + sp.subs <= max_records) {
    if (st.status != 0) break;
    // mode switches, once per outer block against the record counter (track-gps-l1.py:156-159)
    const int mode = sp.fixed_pll ? kModePll
                   : ((double)st.block >= sp.dwell_wide + sp.dwell_narrow ? kModePll
                   : ((double)st.block >= sp.dwell_wide ? kModeFllNarrow : st.mode));
    const double code_p = st.code_p;
    const double nf = code_p < Ld / 2 ? (fs * sp.period * (Ld - code_p)) / Ld : (fs * sp.period * (2 * Ld - code_p)) / Ld;
    if (!(nf >= 1.0) || !(nf < 4.0e15)) {            // NaN, or int(nf) <= 0: nothing the reference could read sensibly
      __syncthreads();
      if (tid == 0) st.status = GACQ_TRACK_BAD_BLOCK;
      __syncthreads();
      break;
    }
    const long long n = (long long)nf;
    if (st.pos < run.base || st.pos + n > run.end) break;   // io.get_samples_complex would return None
    const long long dpo = nco_fixed(st.coffset_phase);
    const int8_t* xb = run.x + 2 * (st.pos - run.base);
    for (int j = 0; j < sp.subs; j++) {
      const long long a = (long long)((double)((long long)j * n) / (double)sp.subs);
      const long long b = (long long)((double)((long long)(j + 1) * n) / (double)sp.subs);
      const long long m = b - a;
      const double carrier_p = st.carrier_p, carrier_f = st.carrier_f, code_f = st.code_f, cp_code = st.code_p;
      const double fc = -carrier_f / fs;
      const double cf = (code_f + carrier_f / sp.ratio) / fs;
      if (!nco_ok(carrier_p) || !nco_ok(fc) || !(fabs(cp_code) < 1.0e9) || !(fabs(cf) < 1.0e3)) {
        __syncthreads();
        if (tid == 0) st.status = GACQ_TRACK_BAD_PHASE;
        __syncthreads();
        break;
      }
      const long long dpc = nco_fixed(carrier_p), dfc = nco_fixed(fc);
      double cp0[3], bp0[3], bp60[3];
      for (int t = 0; t < 3; t++) {
        const double frac = t == 0 ? cp_code - sp.spacing : (t == 1 ? cp_code : cp_code + sp.spacing);
        cp0[t] = pymod(frac, Ld);
        bp0[t] = pymod(2.0 * frac, 2.0);
        bp60[t] = pymod(12.0 * frac, 2.0);
      }
      double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      for (long long i = tid; i < m; i += kTlBlock) {
        const long long k = a + i;
        const unsigned long long po = (unsigned long long)dpo + (unsigned long long)k * (unsigned long long)sp.dfo;
        const unsigned long long pc = (unsigned long long)dpc + (unsigned long long)i * (unsigned long long)dfc;
        float2 v = mix_c64(make_float2((float)xb[2 * k], (float)xb[2 * k + 1]), s_tab[(po >> 50) & (kNT - 1)]);
        v = mix_c64(v, s_tab[(pc >> 50) & (kNT - 1)]);
        const double vr = (double)v.x, vi = (double)v.y, di = (double)i;
#pragma unroll
        for (int t = 0; t < 3; t++) {
          const double w = chip_weight(s_chips, L, inv_l, sp.kind, cp0[t], bp0[t], bp60[t], cf, di);
          acc[2 * t] = acc[2 * t] + vr * w;                                       // p += x[i]*w: product rounded, then the sum
          acc[2 * t + 1] = acc[2 * t + 1] + vi * w;
        }
      }
      // row sums by DPP (lanes 0, 16, 32, 48 of each wave), then through LDS: reading the rows out with v_readlane would hold the six
      // sums in 48 SGPRs at once, more than the scalar file has left
#pragma unroll
      for (int t = 0; t < 6; t++) {
        double v = acc[t];
        v += gacq::f64::dpp_f64(v, 0);
        v += gacq::f64::dpp_f64(v, 1);
        v += gacq::f64::dpp_f64(v, 2);
        v += gacq::f64::dpp_f64(v, 3);
        acc[t] = v;
      }
      if ((tid & 15) == 0)
        for (int t = 0; t < 6; t++) s_red[t][tid >> 4] = acc[t];
      __syncthreads();
      if (tid < 6) {                    // one lane per sum, in a fixed order
        double s = 0.0;
        for (int w = 0; w < kTlBlock / 64; w++)
          s = s + ((s_red[tid][4 * w] + s_red[tid][4 * w + 1]) + (s_red[tid][4 * w + 2] + s_red[tid][4 * w + 3]));
        s_sum[tid] = s;
      }
      __syncthreads();
      if (tid == 0) {
        double p[6];
        for (int t = 0; t < 6; t++) p[t] = s_sum[t];
        const double md = (double)m;
        // carrier NCO phase (track-gps-l1.py:36-42)
        double cpn = carrier_p - (md * carrier_f) / fs;
        const double ct = pymod(cpn, 1.0);
        st.carrier_cyc += (long long)rint(cpn - ct);
        st.carrier_p = ct;
        // carrier loop (:52-70)
        double cfn = carrier_f;
        const double pr = p[2], pi_ = p[3];
        if (mode == kModePll) {
          const double e = pll_costas(pr, pi_);
          cfn = carrier_f + sp.pll_k1 * e + sp.pll_k2 * (e - st.carrier_e1);
          st.carrier_e1 = e;
        } else {
          const double e = fll_atan(pr, pi_, st.prompt1_re, st.prompt1_im);
          cfn = carrier_f + (mode == kModeFllWide ? sp.fll_k_wide : sp.fll_k_narrow) * e;
          st.prompt1_re = pr;
          st.prompt1_im = pi_;
        }
        st.carrier_f = cfn;
        // code loop (:74-92)
        const double early = hypot(p[0], p[1]), prompt = hypot(pr, pi_), late = hypot(p[4], p[5]);
        const double e = (late + early) == 0.0 ? 0.0 : (late - early) / (late + early);
        st.code_f = code_f + sp.dll_k1 * e + sp.dll_k2 * (e - st.code_e1);
        st.code_e1 = e;
        const double cpc = cp_code + md * cf;
        const double t = pymod(cpc, Ld);
        st.code_cyc += (long long)rint(cpc - t);
        st.code_p = t;
        st.mode = mode;
        if (j == 0) st.samp += n;
        if (nrec < rec_cap) {
          gacq_track_record& r = recs[(long)ch * rec_cap + nrec];
          r.p_re = pr; r.p_im = pi_; r.carrier_f = cfn; r.code_f = st.code_f;
          r.early = early; r.prompt = prompt; r.late = late; r.code_p = st.code_p; r.carrier_p = st.carrier_p;
          r.block = st.block; r.code_cyc = st.code_cyc; r.carrier_cyc = st.carrier_cyc; r.samp = st.samp;
        }
        st.block += 1;
      }
      nrec++;
      __syncthreads();
    }
    if (st.status != 0) break;
    if (tid == 0) {
      // offset wipe-off phase, the script's own expression (track-gps-l1.py:171-173; GLONASS adds n*fm instead)
      const double nd = (double)n;
      const double cph = sp.glonass ? st.coffset_phase + nd * sp.fm : st.coffset_phase - (nd * sp.coffset) / fs;
      st.coffset_phase = pymod(cph, 1.0);
      st.pos += n;
    }
    __syncthreads();
  }
  __syncthreads();
  if (tid == 0) {
    st.last_records = nrec;            // the count travels in the state: one pointer less held across the whole kernel
    states[ch] = st;
  }
}

// The two wipe-offs of track_loop_kernel alone, over n samples (offset NCO at sample k, carrier NCO at sample k): the same helpers and
// index arithmetic, so the complex64 values it writes are what the correlators of the loop see (gacq_track_debug_mix)
__global__ __launch_bounds__(kTlBlock) void track_mix_kernel(const int8_t* __restrict__ x, long long n, long long dpo, long long dfo,
                                                             long long dpc, long long dfc, const double2* __restrict__ nco_tab,
                                                             float2* __restrict__ out) {
  for (long long k = (long long)blockIdx.x * kTlBlock + threadIdx.x; k < n; k += (long long)gridDim.x * kTlBlock) {
    const unsigned long long po = (unsigned long long)dpo + (unsigned long long)k * (unsigned long long)dfo;
    const unsigned long long pc = (unsigned long long)dpc + (unsigned long long)k * (unsigned long long)dfc;
    float2 v = mix_c64(make_float2((float)x[2 * k], (float)x[2 * k + 1]), nco_tab[(po >> 50) & (kNT - 1)]);
    out[k] = mix_c64(v, nco_tab[(pc >> 50) & (kNT - 1)]);
  }
}

__global__ void nco_fixed_kernel(double p0, double f0, double p1, double f1, long long* out) {
  out[0] = nco_fixed(p0);
  out[1] = nco_fixed(f0);
  out[2] = nco_fixed(p1);
  out[3] = nco_fixed(f1);
}

}  // namespace

extern "C" int gacq_track_debug_mix(gacq_ctx* ctx, const void* d_iq_int8, size_t n, double f_offset, double p_offset, double f_carrier,
                                    double p_carrier, void* d_out) {
  if (!ctx || !d_iq_int8 || !d_out || n == 0 || n > ((size_t)1 << 40))
    return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_track_debug_mix: bad argument");
  for (double v : {f_offset, p_offset, f_carrier, p_carrier})
    if (!(std::fabs(v) < 7.0)) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_track_debug_mix: NCO frequency or phase out of range");
  GACQ_DEVICE(ctx);
  const double2* tab = nullptr;
  int rc = nco_table(ctx, &tab);
  if (rc != GACQ_OK) return rc;
  // the fixed-point phases exactly as the loop forms them: on the device
  long long* d_fix = nullptr;
  GACQ_HIP(ctx, hipMalloc(&d_fix, 4 * sizeof(long long)));
  long long fix[4];
  hipLaunchKernelGGL(nco_fixed_kernel, dim3(1), dim3(1), 0, ctx->stream, p_offset, f_offset, p_carrier, f_carrier, d_fix);
  hipError_t e = hipMemcpyAsync(fix, d_fix, sizeof(fix), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(d_fix);
  if (e != hipSuccess) return set_error(ctx, GACQ_ERR_HIP, "gacq_track_debug_mix: %s", hipGetErrorString(e));
  const unsigned grid = (unsigned)std::min<size_t>((n + kTlBlock - 1) / kTlBlock, 4096);
  hipLaunchKernelGGL(track_mix_kernel, dim3(grid), dim3(kTlBlock), 0, ctx->stream, (const int8_t*)d_iq_int8, (long long)n, fix[0], fix[1],
                     fix[2], fix[3], tab, (float2*)d_out);
  GACQ_HIP(ctx, hipGetLastError());
  GACQ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return GACQ_OK;
}

#include "gacq_trackhost.h"

struct gacq_track : TlHandle {};

extern "C" int gacq_track_open(gacq_ctx* ctx, const gacq_track_spec* specs, int K, gacq_track** out) {
  static const TlLimits lim = {"gacq_track_open", 0x3f, 64, kMaxChips, HUGE_VAL, false};
  return tl_open(ctx, lim, specs, K, out);
}

extern "C" int gacq_track_run_dev(gacq_track* h, const void* const* d_x, const long long* base, const long long* avail, int max_records,
                                  gacq_track_record* recs, int rec_cap, int* counts, int* status) {
  return tl_run(h, "gacq_track_run_dev", false, d_x, base, avail, max_records, recs, rec_cap, counts, status, [&](hipStream_t stream) {
    hipLaunchKernelGGL(track_loop_kernel, dim3((unsigned)h->K), dim3(kTlBlock), 0, stream, (const TlSpec*)h->d_specs.p, (const TlRun*)h->d_runs.p,
                       (gacq_track_chstate*)h->d_states.p, h->d_tab, (gacq_track_record*)h->d_recs.p, rec_cap, max_records);
  });
}

extern "C" int gacq_track_state(gacq_track* h, int k, gacq_track_chstate* out) { return tl_state(h, "gacq_track_state", k, out); }

extern "C" void gacq_track_close(gacq_track* h) { tl_close(h); }
