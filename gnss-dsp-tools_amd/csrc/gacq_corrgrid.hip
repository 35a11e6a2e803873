// Correlation grid on the raw recording: for K candidates in one launch, the prompt correlation over M blocks of n samples, D Doppler
// hypotheses and P code-phase hypotheses (gacq_corr_grid_dev, include/gacq.h).  With j = s0 + m n + i the absolute sample index,
//   C[k,m,d,p] = sum_{i<n} x[j] exp(-2 pi i frac((carrier_hz + f_d) j / fs)) w(code0 + off[p] + cf j)
// where w is the chip weight of the tracking loops (chip_weight of gacq_trackcore.h: plain, BOC(1,1), CBOC, TMBOC, RZ).
//
// One workgroup per (candidate, block).  The chip table sits in LDS; a tile of kTD x kTP complex fp32 accumulators sits in each lane's
// registers and larger grids loop over tiles, so a sample is read once per tile.  Per sample and tile a lane forms
//   * the kTP chip weights: the code position (code0 + off[p]) + cf j in fp64, two roundings, exactly as numpy evaluates it, so that
//     a chip boundary falls on the same sample as in an fp64 restatement; floor and modulo in fp64, all integers below 2^53;
//   * the kTD rotations: the carrier phase of every hypothesis is a 64-bit fixed-point fraction of a cycle, j * step_d mod 2^64 with
//     step_d = frac((carrier_hz + f_d) / fs) 2^64 formed on the host in extended precision.  It is reduced before anything is
//     converted to fp32: the top two bits (after rounding to the nearest quarter turn) pick the quadrant, the remaining 30 bits go
//     through degree-7 / degree-6 polynomials for sin / cos of (pi/2) t, |t| <= 1/2 (1e-7 absolute).  Every hypothesis has its own
//     exact phase; nothing on the Doppler axis is extrapolated from partial sums.
// The lane sums are added across the wave by an xor butterfly and across the four waves in fp64 in wave order, so the bits of a result
// depend on nothing but its own candidate and block.
//
// Contraction is off for the whole file (the code positions must round product and sum separately); what is fused is spelled fmaf().
#pragma clang fp contract(off)

#include "gacq_common.h"
#include "gacq_turn.h"

#include <cmath>
#include <cstring>
#include <vector>

using namespace gacq;

namespace {

constexpr int kCgBlock = 256;
constexpr int kCgMaxChips = 10240;            // the longest template code is 10230 chips
constexpr int kCgMaxHyp = 33;                 // D, P <= 33
constexpr int kTD = 5, kTP = 10;              // accumulator tile: 50 complex fp32 per lane
constexpr int kCgPadD = (kCgMaxHyp + kTD - 1) / kTD * kTD;
constexpr int kCgPadP = (kCgMaxHyp + kTP - 1) / kTP * kTP;

struct CgSpec {                               // one candidate, device form
  const int8_t* x;                            // interleaved int8 I/Q, sample j at x[2 j], x[2 j + 1]
  const uint8_t* chips;
  long long s0, out0;                         // first sample; first output element
  double cf, cf12, inv_l;
  int L, kind, n, M, D, P, wg0, pad;          // wg0: the candidate's first workgroup
  double cpp[kCgMaxHyp];                      // code0 + off[p]
  unsigned long long step[kCgMaxHyp];         // frac((carrier_hz + f_d) / fs) 2^64
};

// (cos, sin) of 2 pi ph / 2^64.  Not gacq_turn.h's turn_sincos: these are shorter polynomials, whose coefficients
// tests/refine_oracle.py and its goldens restate.
__device__ __forceinline__ void sincos_turn(unsigned long long ph, float& c, float& s) {
  const unsigned u = (unsigned)(ph >> 32) + 0x20000000u;          // + 1/8 turn: the quadrant index rounds to nearest
  const unsigned q = u >> 30;
  const float t = (float)((int)(u & 0x3fffffffu) - 0x20000000) * 9.31322574615478515625e-10f;      // quarter turns, [-1/2, 1/2)
  const float t2 = t * t;
  float ps = fmaf(t2, -4.592275197e-03f, 7.967589690e-02f);
  ps = fmaf(ps, t2, -6.459629374e-01f);
  ps = fmaf(ps, t2, 1.570796305e+00f) * t;
  float pc = fmaf(t2, -2.040825547e-02f, 2.535986077e-01f);
  pc = fmaf(pc, t2, -1.233697011e+00f);
  pc = fmaf(pc, t2, 9.999999724e-01f);
  const float a = (q & 1u) ? ps : pc, b = (q & 1u) ? pc : ps;     // quarter turns: (c, s), (-s, c), (-c, -s), (s, -c)
  c = __uint_as_float(__float_as_uint(a) ^ ((((q + 1u) >> 1) & 1u) << 31));
  s = __uint_as_float(__float_as_uint(b) ^ (((q >> 1) & 1u) << 31));
}

__device__ __forceinline__ double parity(double v) {             // floor(v) & 1 without leaving fp64
  return floor(v) - 2.0 * floor(0.5 * v);
}

// chip weight at code position pos (= cpp + t) as chip_weight (gacq_trackcore.h) has it; pos12 = 12 cpp + 12 cf j for the 6 x subcarrier
__device__ __forceinline__ float grid_weight(const uint8_t* chips, int L, double Ld, double inv_l, int kind, double pos, double pos12) {
  const double fl = floor(pos);
  int idx = (int)(fl - floor(pos * inv_l) * Ld);
  if (idx < 0) idx += L;
  if (idx >= L) idx -= L;
  float w = chips[idx] ? -1.0f : 1.0f;
  if (kind != 0) {
    const bool b1 = parity(2.0 * pos) != 0.0;                     // 2 pos is exact: the phase 2 cpp + (2 cf) j of the loops
    if (kind == 1) {
      w = b1 ? -w : w;
    } else if (kind == 2 || kind == 3) {
      const bool b6 = parity(pos12) != 0.0;
      if (kind == 2) {
        const double s1 = b1 ? -1.0 : 1.0, s6 = b6 ? -1.0 : 1.0;
        w = w * (float)(0.953463 * s1 + 0.301511 * s6);
      } else {
        w = ((kTmbocMask >> (idx % 33)) & 1ull) ? (b6 ? -w : w) : (b1 ? -w : w);
      }
    } else {
      w = ((kind == 4) == !b1) ? w : 0.0f;
    }
  }
  return w;
}

__global__ __launch_bounds__(kCgBlock) void corr_grid_kernel(const CgSpec* __restrict__ specs, int K, double2* __restrict__ out) {
  __shared__ uint8_t s_chips[kCgMaxChips];
  __shared__ double s_cpp[kCgPadP];
  __shared__ unsigned long long s_step[kCgPadD];
  __shared__ float s_red[kCgBlock / 64][2 * kTD * kTP];
  const int tid = threadIdx.x;
  const int bid = blockIdx.x;
  int lo = 0, hi = K - 1;
  while (lo < hi) {                           // the candidate this workgroup belongs to: the last one with wg0 <= bid
    const int mid = (lo + hi + 1) >> 1;
    if (specs[mid].wg0 <= bid) lo = mid; else hi = mid - 1;
  }
  const CgSpec* __restrict__ sp = specs + lo;
  const int m = bid - sp->wg0;
  const int L = sp->L, kind = sp->kind, n = sp->n, D = sp->D, P = sp->P;
  const double Ld = (double)L, inv_l = sp->inv_l, cf = sp->cf, cf12 = sp->cf12;
  const int8_t* __restrict__ x = sp->x;
  for (int k = tid; k < L; k += kCgBlock) s_chips[k] = sp->chips[k];
  if (tid < kCgPadP) s_cpp[tid] = sp->cpp[tid < P ? tid : P - 1];
  if (tid < kCgPadD) s_step[tid] = tid < D ? sp->step[tid] : 0ull;
  __syncthreads();
  const long long jb = sp->s0 + (long long)m * n;          // the block's first sample
  double2* __restrict__ ob = out + sp->out0 + (long long)m * D * P;

  for (int d0 = 0; d0 < D; d0 += kTD) {
    for (int p0 = 0; p0 < P; p0 += kTP) {
      float ar[kTD][kTP], ai[kTD][kTP];
      unsigned long long ph[kTD], inc[kTD];
      double cp[kTP];
#pragma unroll
      for (int d = 0; d < kTD; d++) {
        const unsigned long long st = s_step[d0 + d];
        ph[d] = (unsigned long long)(jb + tid) * st;
        inc[d] = (unsigned long long)kCgBlock * st;
#pragma unroll
        for (int p = 0; p < kTP; p++) ar[d][p] = ai[d][p] = 0.0f;
      }
#pragma unroll
      for (int p = 0; p < kTP; p++) cp[p] = s_cpp[p0 + p];
      for (int i = tid; i < n; i += kCgBlock) {
        const long long j = jb + i;
        const float xr = (float)x[2 * j], xi = (float)x[2 * j + 1];
        const double dj = (double)j;
        const double t = cf * dj, t12 = cf12 * dj;
        float w[kTP];
#pragma unroll
        for (int p = 0; p < kTP; p++) w[p] = grid_weight(s_chips, L, Ld, inv_l, kind, cp[p] + t, 12.0 * cp[p] + t12);
#pragma unroll
        for (int d = 0; d < kTD; d++) {
          float c, s;
          sincos_turn(ph[d], c, s);
          ph[d] += inc[d];
          const float vr = fmaf(xi, s, xr * c);            // x exp(-i phi)
          const float vi = fmaf(-xr, s, xi * c);
#pragma unroll
          for (int p = 0; p < kTP; p++) {
            ar[d][p] = fmaf(vr, w[p], ar[d][p]);
            ai[d][p] = fmaf(vi, w[p], ai[d][p]);
          }
        }
      }
      // across the wave: xor butterfly, the same order in every lane; then the four waves in fp64, in wave order
#pragma unroll
      for (int d = 0; d < kTD; d++) {
#pragma unroll
        for (int p = 0; p < kTP; p++) {
          float a = ar[d][p], b = ai[d][p];
#pragma unroll
          for (int sh = 1; sh < 64; sh <<= 1) {
            a += __shfl_xor(a, sh, 64);
            b += __shfl_xor(b, sh, 64);
          }
          if ((tid & 63) == 0) {
            s_red[tid >> 6][2 * (d * kTP + p)] = a;
            s_red[tid >> 6][2 * (d * kTP + p) + 1] = b;
          }
        }
      }
      __syncthreads();
      if (tid < kTD * kTP) {
        const int d = d0 + tid / kTP, p = p0 + tid % kTP;
        if (d < D && p < P) {
          double re = 0.0, im = 0.0;
          for (int wv = 0; wv < kCgBlock / 64; wv++) {
            re = re + (double)s_red[wv][2 * tid];
            im = im + (double)s_red[wv][2 * tid + 1];
          }
          ob[(long long)d * P + p] = make_double2(re, im);
        }
      }
      __syncthreads();
    }
  }
}

}  // namespace

extern "C" int gacq_corr_grid_dev(gacq_ctx* ctx, const gacq_grid_spec* specs, int K, const void* const* d_x, const long long* avail,
                                  double* out) {
  if (!ctx) return GACQ_ERR_BAD_ARG;
  if (!specs || !d_x || !avail || !out || K < 1) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_corr_grid_dev: NULL argument or K = %d < 1", K);
  // every candidate is checked before anything is allocated or launched
  std::vector<CgSpec> cs(K);
  std::vector<ChipTable> tabs(K);
  long long nout = 0, nwg = 0;
  int short_k = -1;
  for (int k = 0; k < K; k++) {
    const gacq_grid_spec& s = specs[k];
    if (!s.code || !s.offsets || !d_x[k]) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_corr_grid_dev: candidate %d: NULL code, offsets or samples", k);
    const int L = gacq_code_length(s.code);
    if (L < 0) return set_error(ctx, GACQ_ERR_UNKNOWN_CODE, "gacq_corr_grid_dev: candidate %d: unknown code '%s'", k, s.code);
    if (L > kCgMaxChips) return set_error(ctx, GACQ_ERR_UNSUPPORTED, "gacq_corr_grid_dev: candidate %d: code '%s' is longer than %d chips", k, s.code, kCgMaxChips);
    const int rc = chip_table_host(ctx, s.code, s.prn, L, false, tabs[k]);
    if (rc < 0) return set_error(ctx, rc, "gacq_corr_grid_dev: candidate %d: no PRN %d in '%s'", k, s.prn, s.code);
    if (s.kind < 0 || s.kind > 5) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_corr_grid_dev: candidate %d: correlator kind %d", k, s.kind);
    const bool fin = std::isfinite(s.fs) && std::isfinite(s.carrier_hz) && std::isfinite(s.chip_rate) && std::isfinite(s.ratio) &&
                     std::isfinite(s.doppler0) && std::isfinite(s.code0) && std::isfinite(s.df);
    if (!fin || !(s.fs > 0.0) || s.ratio == 0.0)
      return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_corr_grid_dev: candidate %d: fs, carrier_hz, chip_rate, ratio, doppler0, code0 and df must be finite, fs > 0, ratio != 0", k);
    if (s.n < 1 || s.M < 1 || s.D < 1 || s.D > kCgMaxHyp || s.P < 1 || s.P > kCgMaxHyp)
      return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_corr_grid_dev: candidate %d: need n >= 1, M >= 1, 1 <= D, P <= %d (n %d, M %d, D %d, P %d)", k,
                       kCgMaxHyp, s.n, s.M, s.D, s.P);
    if (s.s0 < 0 || s.s0 > (1ll << 40) || avail[k] < 0)
      return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_corr_grid_dev: candidate %d: first sample %lld, %lld samples available", k, s.s0, avail[k]);
    const long long end = s.s0 + (long long)s.M * s.n;
    CgSpec& c = cs[k];
    std::memset(&c, 0, sizeof(c));
    c.cf = (s.chip_rate + s.doppler0 / s.ratio) / s.fs;
    c.cf12 = 12.0 * c.cf;
    double amax = 0.0;
    for (int p = 0; p < s.P; p++) {
      if (!std::isfinite(s.offsets[p])) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_corr_grid_dev: candidate %d: code offset %d is not finite", k, p);
      c.cpp[p] = s.code0 + s.offsets[p];
      amax = std::max(amax, std::fabs(c.cpp[p]));
    }
    // floor and modulo of the code position stay exact in fp64
    if (!std::isfinite(c.cf) || !(12.0 * (amax + std::fabs(c.cf) * (double)end) < 4.0e15))
      return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_corr_grid_dev: candidate %d: code positions out of range", k);
    if (end > avail[k] && short_k < 0) short_k = k;
    for (int d = 0; d < s.D; d++) {
      const double f = s.carrier_hz + (s.doppler0 + ((double)d - (double)(s.D - 1) / 2.0) * s.df);
      long double r = (long double)f / (long double)s.fs;
      r -= floorl(r);
      const long double v = r * 18446744073709551616.0L;
      c.step[d] = v >= 18446744073709551615.0L ? ~0ull : (unsigned long long)v;
    }
    c.x = (const int8_t*)d_x[k];
    c.s0 = s.s0;
    c.out0 = nout;
    c.inv_l = 1.0 / (double)L;
    c.L = L; c.kind = s.kind; c.n = s.n; c.M = s.M; c.D = s.D; c.P = s.P;
    if (nwg + s.M > 0x7fffffffll) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_corr_grid_dev: more than 2^31 - 1 (candidate, block) pairs");
    c.wg0 = (int)nwg;
    nwg += s.M;
    nout += (long long)s.M * s.D * s.P;
  }
  if (short_k >= 0) {
    const gacq_grid_spec& s = specs[short_k];
    return set_error(ctx, GACQ_ERR_SHORT_INPUT, "gacq_corr_grid_dev: candidate %d: samples [%lld, %lld) needed, %lld available", short_k, s.s0,
                     s.s0 + (long long)s.M * s.n, avail[short_k]);
  }
  GACQ_DEVICE(ctx);
  hipStream_t stream = ctx->stream;
  int rc;
  for (int k = 0; k < K; k++)
    if ((rc = chip_table_dev(ctx, tabs[k], &cs[k].chips)) != GACQ_OK) return rc;
  DevBuf& d_specs = ctx->tables["corrgrid:specs"];
  DevBuf& d_out = ctx->tables["corrgrid:out"];
  if ((rc = ensure(ctx, d_specs, sizeof(CgSpec) * (size_t)K)) != GACQ_OK) return rc;
  if ((rc = ensure(ctx, d_out, sizeof(double2) * (size_t)nout)) != GACQ_OK) return rc;
  // the specs leave pageable memory before this returns: the copy is synchronous with respect to the host buffer
  GACQ_HIP(ctx, hipMemcpyAsync(d_specs.p, cs.data(), sizeof(CgSpec) * (size_t)K, hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(corr_grid_kernel, dim3((unsigned)nwg), dim3(kCgBlock), 0, stream, (const CgSpec*)d_specs.p, K, (double2*)d_out.p);
  GACQ_HIP(ctx, hipGetLastError());
  GACQ_HIP(ctx, hipMemcpyAsync(out, d_out.p, sizeof(double2) * (size_t)nout, hipMemcpyDeviceToHost, stream));
  GACQ_HIP(ctx, hipStreamSynchronize(stream));
  return GACQ_OK;
}
