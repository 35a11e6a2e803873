// Device-resident tracking loops for the long-code scripts: track-gps-l2cl.py (767 250-chip RZ code, 1.5 s outer block in 1500
// track() calls) and track-glonass-l1-p.py / -l2-p.py (5 110 000-chip code, 1 s outer block in 1000 calls), one workgroup per
// channel.  Their track() and main loop differ from the template (gacq_trackloop.hip) only in constants and in dropping the cycle
// counters, so the arithmetic here is the template's, step for step:
//   - the offset wipe-off over the whole outer block and the carrier wipe-off per sub-block, both the 50-bit fixed-point table NCO
//     of gnsstools/nco.py:30-41, each product rounded to complex64; the offset phase is closed form over the sample's index
//     within the outer block (dpo + k*dfo mod 2^64);
//   - early / prompt / late with the closed-form phases floor(fma(incr, i, cp0)) mod L, each term rounded before it is summed,
//     and the template's fixed-order reduction;
//   - lane 0 runs the FLL / PLL / DLL update in the script's order and writes one record per track() call; the mode switches are
//     checked once per outer block against the record counter.
// What is new is the chip source.  The code table stays in device memory (table_cache's "chips:<code>:<prn>", shared with the
// long-code search); per sub-block the workgroup stages the chips it will touch -- from floor(cp0 of early) to the last chip late
// reaches, wrapped mod L -- into an LDS window and indexes it with exact integer offsets, which give the same chip as the
// template's floor(pos) mod L.  A sub-block whose span exceeds the window (a code rate far off) stops the channel with
// GACQ_TRACK_BAD_WINDOW before it is correlated; no record is ever computed from a partial window.
//
// Nothing waits on another workgroup and every loop is bounded by max_records and by the samples given.
//
// Contraction is off for the whole file, as in gacq_trackloop.hip: every product and sum is rounded on its own, and the phases that
// are fused on purpose are spelled as fma().
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

constexpr int kLtBlock = 256;
constexpr int kMaxSubs = 1500;                // track-gps-l2cl.py: 1500 calls per outer block
// LDS chip window: a sub-block spans at most 1.5 code-ms (n = fs*period*(2L-code_p)/L with code_p just above L/2) -- 767 chips
// for L2CL, 7665 for GLONASS P -- plus the early/late spacing on each side
constexpr int kWinChips = 16384;

// the chip weight of window chip q = floor(pos) + qoff (the window holds chips base .. base+span-1 mod L, and qoff = off - floor(cp0)
// maps the correlator's own start chip to its place there) times the RZ half-chip gate; kinds 0 (plain), 4 and 5 (RZ) only
__device__ __forceinline__ double window_weight(const uint8_t* win, int qoff, int kind, double cp0, double bp0, double incr, double di) {
  const double pos = fma(incr, di, cp0);
  double w = win[(int)floor(pos) + qoff] ? -1.0 : 1.0;
  if (kind != 0) {
    const int b1 = (int)floor(fma(2.0 * incr, di, bp0)) & 1;
    w = ((kind == 4) == (b1 == 0)) ? w : 0.0;                                         // rz = [1,0] (kind 4) / [0,1] (kind 5)
  }
  return w;
}

__global__ __launch_bounds__(kLtBlock) void longtrack_kernel(const TlSpec* __restrict__ specs, const TlRun* __restrict__ runs,
                                                             gacq_track_chstate* __restrict__ states, const double2* __restrict__ nco_tab,
                                                             gacq_track_record* __restrict__ recs, int rec_cap, int max_records) {
  __shared__ double2 s_tab[kNT];
  __shared__ uint8_t s_win[kWinChips];
  __shared__ double s_red[6][kLtBlock / 16];
  __shared__ double s_sum[6];
  __shared__ gacq_track_chstate st;
  __shared__ TlSpec sp;
  const int ch = blockIdx.x;
  const int tid = threadIdx.x;
  const TlRun run = runs[ch];
  if (tid == 0) {
    st = states[ch];
    sp = specs[ch];
  }
  for (int k = tid; k < kNT; k += kLtBlock) s_tab[k] = nco_tab[k];
  __syncthreads();
  const long L = sp.L;
  const double Ld = (double)sp.L;
  const double fs = sp.fs;
  int nrec = 0;
  while (nrec + sp.subs <= max_records) {
    if (st.status != 0) break;
    // mode switches, once per outer block against the record counter (track-gps-l2cl.py:147-150)
    const int mode = sp.fixed_pll ? kModePll
                   : ((double)st.block >= sp.dwell_wide + sp.dwell_narrow ? kModePll
                   : ((double)st.block >= sp.dwell_wide ? kModeFllNarrow : st.mode));
    const double code_p = st.code_p;
    const double nf = code_p < Ld / 2 ? (fs * sp.period * (Ld - code_p)) / Ld : (fs * sp.period * (2 * Ld - code_p)) / Ld;
    if (!(nf >= 1.0) || !(nf < 4.0e15)) {
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
      // a,b = int(j*n/subs),int((j+1)*n/subs): j*n < 2^53, so the true division is one correctly rounded fp64 division
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
      double cp0[3], bp0[3];
      long fl0[3];
      for (int t = 0; t < 3; t++) {
        const double frac = t == 0 ? cp_code - sp.spacing : (t == 1 ? cp_code : cp_code + sp.spacing);
        cp0[t] = pymod(frac, Ld);
        bp0[t] = pymod(2.0 * frac, 2.0);
        fl0[t] = (long)floor(cp0[t]);
      }
      // the window starts at early's first chip; correlator t's first chip sits off[t] = (fl0[t] - base) mod L into it, and its
      // last one -- the phases are non-decreasing in i for cf >= 0 -- at the same fma() for i = m - 1
      const long base = fl0[0];
      long off[3], span = 0;
      for (int t = 0; t < 3; t++) {
        off[t] = fl0[t] - base;
        if (off[t] < 0) off[t] += L;
        if (m > 0) span = std::max(span, (long)floor(fma(cf, (double)(m - 1), cp0[t])) - fl0[t] + off[t] + 1);
      }
      if (!(cf >= 0.0) || span > kWinChips) {
        __syncthreads();
        if (tid == 0) st.status = GACQ_TRACK_BAD_WINDOW;
        __syncthreads();
        break;
      }
      for (long q = tid; q < span; q += kLtBlock) {
        long g = base + q;
        if (g >= L) g %= L;
        s_win[q] = sp.chips[g];
      }
      __syncthreads();
      const int qoff[3] = {(int)(off[0] - fl0[0]), (int)(off[1] - fl0[1]), (int)(off[2] - fl0[2])};
      double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      for (long long i = tid; i < m; i += kLtBlock) {
        const long long k = a + i;
        const unsigned long long po = (unsigned long long)dpo + (unsigned long long)k * (unsigned long long)sp.dfo;
        const unsigned long long pc = (unsigned long long)dpc + (unsigned long long)i * (unsigned long long)dfc;
        float2 v = mix_c64(make_float2((float)xb[2 * k], (float)xb[2 * k + 1]), s_tab[(po >> 50) & (kNT - 1)]);
        v = mix_c64(v, s_tab[(pc >> 50) & (kNT - 1)]);
        const double vr = (double)v.x, vi = (double)v.y, di = (double)i;
#pragma unroll
        for (int t = 0; t < 3; t++) {
          const double w = window_weight(s_win, qoff[t], sp.kind, cp0[t], bp0[t], cf, di);
          acc[2 * t] = acc[2 * t] + vr * w;                                       // p += x[i]*w: product rounded, then the sum
          acc[2 * t + 1] = acc[2 * t + 1] + vi * w;
        }
      }
      // the template's reduction: DPP within rows of 16, then the 16 row sums in a fixed order
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
      if (tid < 6) {
        double s = 0.0;
        for (int w = 0; w < kLtBlock / 64; w++)
          s = s + ((s_red[tid][4 * w] + s_red[tid][4 * w + 1]) + (s_red[tid][4 * w + 2] + s_red[tid][4 * w + 3]));
        s_sum[tid] = s;
      }
      __syncthreads();
      if (tid == 0) {
        double p[6];
        for (int t = 0; t < 6; t++) p[t] = s_sum[t];
        const double md = (double)m;
        // carrier NCO phase (track-gps-l2cl.py:35-37): np.mod only; the cycle count is kept for the record, the script drops it
        double cpn = carrier_p - (md * carrier_f) / fs;
        const double ct = pymod(cpn, 1.0);
        st.carrier_cyc += (long long)rint(cpn - ct);
        st.carrier_p = ct;
        // carrier loop (:41-65)
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
        // code loop (:69-84)
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
      // offset wipe-off phase (track-gps-l2cl.py:162-164; GLONASS P adds n*fm, track-glonass-l1-p.py:161-164)
      const double nd = (double)n;
      const double cph = sp.glonass ? st.coffset_phase + nd * sp.fm : st.coffset_phase - (nd * sp.coffset) / fs;
      st.coffset_phase = pymod(cph, 1.0);
      st.pos += n;
    }
    __syncthreads();
  }
  __syncthreads();
  if (tid == 0) {
    st.last_records = nrec;
    states[ch] = st;
  }
}

}  // namespace

#include "gacq_trackhost.h"

struct gacq_longtrack : TlHandle {};

// no limit on the code's length: the kernel reads the chips through its LDS window.  A table is generated only when the context's
// cache lacks it (5.11 M chips for GLONASS P)
extern "C" int gacq_longtrack_open(gacq_ctx* ctx, const gacq_track_spec* specs, int K, gacq_longtrack** out) {
  static const TlLimits lim = {"gacq_longtrack_open", 1u << 0 | 1u << 4 | 1u << 5, kMaxSubs, 0, 0.25 * kWinChips, true};
  return tl_open(ctx, lim, specs, K, out);
}

extern "C" int gacq_longtrack_run_dev(gacq_longtrack* h, const void* const* d_x, const long long* base, const long long* avail,
                                      int max_records, gacq_track_record* recs, int rec_cap, int* counts, int* status) {
  return tl_run(h, "gacq_longtrack_run_dev", true, d_x, base, avail, max_records, recs, rec_cap, counts, status, [&](hipStream_t stream) {
    hipLaunchKernelGGL(longtrack_kernel, dim3((unsigned)h->K), dim3(kLtBlock), 0, stream, (const TlSpec*)h->d_specs.p, (const TlRun*)h->d_runs.p,
                       (gacq_track_chstate*)h->d_states.p, h->d_tab, (gacq_track_record*)h->d_recs.p, rec_cap, max_records);
  });
}

extern "C" int gacq_longtrack_state(gacq_longtrack* h, int k, gacq_track_chstate* out) { return tl_state(h, "gacq_longtrack_state", k, out); }

extern "C" void gacq_longtrack_close(gacq_longtrack* h) { tl_close(h); }
