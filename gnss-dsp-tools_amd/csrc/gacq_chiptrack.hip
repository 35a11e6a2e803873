// Tracking loops with the chip accumulator: track-beidou-b2bi.py and track-beidou-b2bq.py, one workgroup per channel.
//
// The loop is a copy of track_loop_kernel's (gacq_trackloop.hip), step for step, with its comments and the same helpers
// (gacq_trackcore.h), so its records are bit-identical to that kernel's for the same spec (tests/test_chiptrack_gpu.py checks it).
// A change to the template loop must be made here too.  One step is added after each block's E/P/L reduction and before the loop
// update, the script's
//     if s.nframe > 200:  nco.accum(x if real(p_prompt) > 0 else -x, s.code_p, cf, s.chips, L)
// with nframe the record's block and 200 the channel's accum_after.  accum adds wiped-off sample i to bin int(cp), cp advancing by
// cf from code_p; the bin is the prompt correlator's closed-form index floor(fma(cf, i, code_p)) mod L.  Each bin must come out as the
// reference's sequential fp64 sum in sample order, across blocks and launches, so nothing is summed out of order or atomically:
//   - the complex128 accumulator (L <= 10240 bins, 160 KiB: the whole LDS of a CU) lives in device memory, one row per channel;
//   - lane t owns bins t, t + 256, t + 512, ...  Unwrapped, floor(fma(cf, i, code_p)) is monotone in i for cf > 0, so the samples of
//     unwrapped chip u = bin + q L form one run [i(u), i(u + 1)), i(u) the first sample at or past u: an estimate (u - code_p) / cf
//     corrected exactly against the fused phase.  The lane walks its bin's runs in order of q (a block with code_p >= L/2 spans up to
//     1.5 L chips, so a bin may get two runs), recomputing each sample's two wipe-offs exactly as the correlator loop forms them, and
//     adds them to the bin held in registers -- a plain sequential sum, and no bin is written by two lanes;
//   - a block with cf < 2^-10 (a loop gone astray, or above 10 GS/s) or a phase past 2^26 is outside the run search's range; lane 0
//     then walks the block in sample order on its own.
//
// Contraction is off for the whole file, as in gacq_trackloop.hip.
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

constexpr int kCtBlock = 256;
constexpr int kCtMaxChips = 10240;            // accumulator row stride, bins
constexpr double kCtMinRate = 1.0 / 1024;     // the run search's range (ct_first_at); blocks outside it are walked serially
constexpr double kCtMaxPhase = 67108864.0;    // 2^26

struct CtBlock {
  long long dpo, dfo, dpc, dfc, a, m, frame, thr;
  double c0, cf;
};

// wiped-off sample k of the outer block (sample i = k - a of its sub-block): both NCO products, as the correlator loop forms them
__device__ __forceinline__ float2 ct_sample(const int8_t* xb, const double2* tab, long long dpo, long long dfo, long long dpc,
                                            long long dfc, long long k, long long i) {
  const unsigned long long po = (unsigned long long)dpo + (unsigned long long)k * (unsigned long long)dfo;
  const unsigned long long pc = (unsigned long long)dpc + (unsigned long long)i * (unsigned long long)dfc;
  const float2 v = mix_c64(make_float2((float)xb[2 * k], (float)xb[2 * k + 1]), tab[(po >> 50) & (kNT - 1)]);
  return mix_c64(v, tab[(pc >> 50) & (kNT - 1)]);
}

// first sample i in [0, m] whose fused phase fma(cf, i, cp0) is >= u (m if none).  With cf >= 2^-10 and every phase below 2^26 the
// estimate ceil((u - cp0) / cf) is within one sample of it (both roundings move the crossing by < 2^-15 samples), so one exact
// step either way finds it; the phase is monotone in i for cf > 0
__device__ __forceinline__ long long ct_first_at(double u, double cp0, double cf, double rcf, long long m) {
  double e = ceil((u - cp0) * rcf);
  e = fmin(fmax(e, 0.0), (double)m);
  long long i = (long long)e;
  if (i > 0 && fma(cf, (double)(i - 1), cp0) >= u) i--;
  else if (i < m && fma(cf, (double)i, cp0) < u) i++;
  return i;
}

__global__ __launch_bounds__(kCtBlock) void chip_track_kernel(const TlSpec* __restrict__ specs, const TlRun* __restrict__ runs,
                                                              gacq_track_chstate* __restrict__ states, const double2* __restrict__ nco_tab,
                                                              const long long* __restrict__ accum_after, double2* __restrict__ bins,
                                                              gacq_track_record* __restrict__ recs, int rec_cap, int max_records) {
  __shared__ double2 s_tab[kNT];
  __shared__ uint8_t s_chips[kCtMaxChips];
  __shared__ double s_red[6][kCtBlock / 16];
  __shared__ double s_sum[6];
  __shared__ gacq_track_chstate st;
  __shared__ TlSpec sp;               // read from LDS where used: a copy in registers overflows the SGPR file
  __shared__ CtBlock sb;              // the accumulation's block constants (lane 0 writes them before the reduction's barrier)
  const int ch = blockIdx.x;
  const int tid = threadIdx.x;
  const TlRun run = runs[ch];
  if (tid == 0) {
    st = states[ch];
    sp = specs[ch];
  }
  for (int k = tid; k < kNT; k += kCtBlock) s_tab[k] = nco_tab[k];
  __syncthreads();
  for (int k = tid; k < sp.L; k += kCtBlock) s_chips[k] = sp.chips[k];
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
      for (long long i = tid; i < m; i += kCtBlock) {
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
      if (tid == 0) {
        sb.dpo = dpo; sb.dfo = sp.dfo; sb.dpc = dpc; sb.dfc = dfc; sb.a = a; sb.m = m;
        sb.c0 = cp0[1]; sb.cf = cf; sb.frame = st.block; sb.thr = accum_after[ch];
      }
      __syncthreads();
      if (tid < 6) {                    // one lane per sum, in a fixed order
        double s = 0.0;
        for (int w = 0; w < kCtBlock / 64; w++)
          s = s + ((s_red[tid][4 * w] + s_red[tid][4 * w + 1]) + (s_red[tid][4 * w + 2] + s_red[tid][4 * w + 3]));
        s_sum[tid] = s;
      }
      __syncthreads();
      // nco.accum: every lane reads the prompt's sign from s_sum before lane 0's update below; s_sum is rewritten only after the
      // __syncthreads that ends this sub-block
      if (sb.frame > sb.thr) {
        double2* const row = bins + (long)ch * kCtMaxChips;
        const bool neg = !(s_sum[2] > 0.0);
        const double c0 = sb.c0, cfa = sb.cf;    // c0 = pymod(code_p, L): the prompt correlator's start phase
        const long long am = sb.a, mm = sb.m;
        const long long dpo_ = sb.dpo, dfo_ = sb.dfo, dpc_ = sb.dpc, dfc_ = sb.dfc;
        const double last = floor(fma(cfa, (double)(mm - 1), c0));      // the block's last unwrapped chip
        if (cfa >= kCtMinRate && last < kCtMaxPhase) {
          const double rcf = 1.0 / cfa;
          for (long c = tid; c < L; c += kCtBlock) {
            double2 s = row[c];
            for (double u = (double)c; u <= last; u += Ld) {
              if (u + 1.0 <= floor(c0)) continue;                    // chip u lies before the block's first sample
              const long long i0 = ct_first_at(u, c0, cfa, rcf, mm);
              const long long i1 = ct_first_at(u + 1.0, c0, cfa, rcf, mm);
              for (long long i = i0; i < i1; i++) {
                const float2 v = ct_sample(xb, s_tab, dpo_, dfo_, dpc_, dfc_, am + i, i);
                s.x = s.x + (double)(neg ? -v.x : v.x);
                s.y = s.y + (double)(neg ? -v.y : v.y);
              }
            }
            row[c] = s;
          }
        } else if (tid == 0) {
          for (long long i = 0; i < mm; i++) {
            const double pos = fma(cfa, (double)i, c0);
            long idx = (long)floor(pos) - (long)floor(pos * inv_l) * L;
            if (idx < 0) idx += L;
            if (idx >= L) idx -= L;
            const float2 v = ct_sample(xb, s_tab, dpo_, dfo_, dpc_, dfc_, am + i, i);
            row[idx].x = row[idx].x + (double)(neg ? -v.x : v.x);
            row[idx].y = row[idx].y + (double)(neg ? -v.y : v.y);
          }
        }
      }
      if (tid == 0) {
        // the block's inputs re-read from LDS (unchanged until here): kept in registers across the accumulation they overflow the
        // scalar file
        const double carrier_p = st.carrier_p, carrier_f = st.carrier_f, code_f = st.code_f, cp_code = st.code_p, cf = sb.cf;
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

}  // namespace

#include "gacq_trackhost.h"

struct gacq_chiptrack : TlHandle {
  std::vector<int> L;
  gacq::DevBuf d_thr, d_bins;
};

extern "C" int gacq_chiptrack_open(gacq_ctx* ctx, const gacq_track_spec* specs, int K, const long long* accum_after, gacq_chiptrack** out) {
  if (!ctx || !out) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_chiptrack_open: NULL argument");
  *out = nullptr;
  if (!specs || K <= 0 || !accum_after)
    return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_chiptrack_open: need at least one channel and its threshold (K = %d)", K);
  for (int k = 0; k < K; k++) {
    const gacq_track_spec& s = specs[k];
    if (!s.code) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_chiptrack_open: channel %d has no code", k);
    const int L = gacq_code_length(s.code);
    if (L < 0) return set_error(ctx, GACQ_ERR_UNKNOWN_CODE, "gacq_chiptrack_open: channel %d: unknown code '%s'", k, s.code);
    if (s.kind != 0 || L > kCtMaxChips || s.glonass)
      return set_error(ctx, GACQ_ERR_UNSUPPORTED, "gacq_chiptrack_open: channel %d: the chip accumulator takes plain codes (kind 0) of at most "
                       "%d chips, not '%s' kind %d", k, kCtMaxChips, s.code, s.kind);
  }
  // the loop's own checks, spec layout and code-boundary alignment are the template's and report under its name.  With no GLONASS
  // channel past the check above, every offset NCO step is floor(-coffset / fs * 2^60)
  static const TlLimits lim = {"gacq_track_open", 0x3f, 64, kCtMaxChips, HUGE_VAL, false};
  TlPrep p;
  int rc = tl_prepare(ctx, lim, specs, K, p);
  if (rc != GACQ_OK) return rc;
  GACQ_DEVICE(ctx);
  gacq_chiptrack* h = new gacq_chiptrack();
  for (const TlSpec& t : p.specs) h->L.push_back(t.L);
  rc = tl_upload(ctx, "gacq_chiptrack_open", p, h);
  if (rc == GACQ_OK) rc = ensure(ctx, h->d_thr, sizeof(long long) * K);
  if (rc == GACQ_OK) rc = ensure(ctx, h->d_bins, sizeof(double2) * kCtMaxChips * (size_t)K);
  if (rc == GACQ_OK && (hipMemcpy(h->d_thr.p, accum_after, sizeof(long long) * K, hipMemcpyHostToDevice) != hipSuccess ||
                        hipMemset(h->d_bins.p, 0, sizeof(double2) * kCtMaxChips * (size_t)K) != hipSuccess))
    rc = set_error(ctx, GACQ_ERR_HIP, "gacq_chiptrack_open: upload failed");
  if (rc != GACQ_OK) {
    gacq_chiptrack_close(h);
    return rc;
  }
  *out = h;
  return GACQ_OK;
}

extern "C" int gacq_chiptrack_run_dev(gacq_chiptrack* h, const void* const* d_x, const long long* base, const long long* avail,
                                      int max_records, gacq_track_record* recs, int rec_cap, int* counts, int* status) {
  return tl_run(h, "gacq_chiptrack_run_dev", false, d_x, base, avail, max_records, recs, rec_cap, counts, status, [&](hipStream_t stream) {
    hipLaunchKernelGGL(chip_track_kernel, dim3((unsigned)h->K), dim3(kCtBlock), 0, stream, (const TlSpec*)h->d_specs.p, (const TlRun*)h->d_runs.p,
                       (gacq_track_chstate*)h->d_states.p, h->d_tab, (const long long*)h->d_thr.p, (double2*)h->d_bins.p,
                       (gacq_track_record*)h->d_recs.p, rec_cap, max_records);
  });
}

extern "C" int gacq_chiptrack_state(gacq_chiptrack* h, int k, gacq_track_chstate* out) { return tl_state(h, "gacq_chiptrack_state", k, out); }

extern "C" int gacq_chiptrack_chips(gacq_chiptrack* h, int k, double* out) {
  if (!h) return GACQ_ERR_BAD_ARG;
  gacq_ctx* ctx = h->ctx;
  if (!out || k < 0 || k >= h->K) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_chiptrack_chips: bad channel %d", k);
  GACQ_DEVICE(ctx);
  GACQ_HIP(ctx, hipMemcpyAsync(out, (const double2*)h->d_bins.p + (size_t)k * kCtMaxChips, sizeof(double2) * h->L[k], hipMemcpyDeviceToHost,
                               ctx->stream));
  GACQ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return GACQ_OK;
}

extern "C" void gacq_chiptrack_close(gacq_chiptrack* h) {
  if (h) tl_close(h, {&h->d_thr, &h->d_bins});
}
