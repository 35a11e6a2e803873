// Device helpers and the device-side structs shared by the tracking loops (gacq_trackloop.hip: the template scripts;
// gacq_longtrack.hip: the long-code scripts; gacq_chiptrack.hip: the B2b scripts).  The host side of their handles -- spec checks,
// uploads, the bookkeeping around a launch -- is in gacq_trackhost.h, which each file includes after its kernels.  chip_track_kernel (gacq_chiptrack.hip) carries a copy of track_loop_kernel's loop
// body: a change to one belongs in the other.  Include it after `#pragma clang fp contract(off)`: the helpers round every product and sum on their own, as the
// reference does, and only the phases written as fma() are fused.
#pragma once

#include "gacq_common.h"
#include "gacq_turn.h"                         // kTmbocMask

#include <cmath>
#include <vector>

namespace {

constexpr int kNcoBits = 10;                  // NT = 1024
constexpr int kNT = 1 << kNcoBits;
constexpr double kTwo60 = 1152921504606846976.0;    // NT * 2^50

enum { kModeFllWide = 0, kModeFllNarrow = 1, kModePll = 2 };

struct TlSpec {                     // constant per channel
  const uint8_t* chips;
  int L, kind, subs, fixed_pll, glonass, pad;
  double fs, period, ratio, spacing;
  double fll_k_wide, fll_k_narrow, pll_k1, pll_k2, dll_k1, dll_k2;
  double coffset, fm;               // offset wipe-off: -coffset/fs (or fm = -(coffset + step*chan)/fs for GLONASS)
  long long dfo;                    // floor(f_offset * NT * 2^50)
  double dwell_wide, dwell_narrow;
};

struct TlRun {                      // per launch
  const int8_t* x;                  // interleaved I/Q int8; sample s of the channel's recording is x[2 (s - base)]
  long long base, end;              // samples [base, end) are present
};

__device__ __forceinline__ double pymod(double a, double m) {   // Python / numpy float modulo (result takes m's sign)
  double r = fmod(a, m);
  if (r != 0.0) {
    if ((r < 0.0) != (m < 0.0)) r = r + m;
  } else {
    r = copysign(0.0, m);
  }
  return r;
}

// complex64 x complex128 -> complex128, rounded to complex64 (x[i] *= tab[idx] on a c8 array); every product rounded on its own.
// Plain operators on purpose: HIP's __dmul_rn / __dadd_rn are defined in headers compiled before this file's pragma, carry the
// `contract` flag and are fused into v_fma_f64; written here they are not (tests/test_track_loop_cpu.py checks the ISA).
__device__ __forceinline__ float2 mix_c64(float2 x, double2 t) {
  const double xr = (double)x.x, xi = (double)x.y;
  const double re = xr * t.x - xi * t.y;
  const double im = xr * t.y + xi * t.x;
  return make_float2((float)re, (float)im);
}

// the chip weight (1.0-2.0*c[int(cp)]) [* subcarrier] of sample i for start phases (cp0, bp0, bp60) and rate incr, in fp64
__device__ __forceinline__ double chip_weight(const uint8_t* chips, long L, double inv_l, int kind, double cp0, double bp0, double bp60,
                                              double incr, double di) {
  const double pos = fma(incr, di, cp0);
  long idx = (long)floor(pos) - (long)floor(pos * inv_l) * L;
  if (idx < 0) idx += L;
  if (idx >= L) idx -= L;
  double w = chips[idx] ? -1.0 : 1.0;
  if (kind != 0) {
    const long b1 = (long)floor(fma(2.0 * incr, di, bp0)) & 1;
    if (kind == 1) {
      w = b1 ? -w : w;                                                              // boc11 = [1, -1]
    } else if (kind == 2 || kind == 3) {
      const long b6 = (long)floor(fma(12.0 * incr, di, bp60)) & 1;
      const double s1 = b1 ? -1.0 : 1.0, s6 = b6 ? -1.0 : 1.0;
      if (kind == 2) w = w * (0.953463 * s1 + 0.301511 * s6);              // CBOC
      else w = ((gacq::kTmbocMask >> (idx % 33)) & 1ull) ? w * s6 : w * s1;               // TMBOC: u = int(cp % 33)
    } else {
      w = ((kind == 4) == (b1 == 0)) ? w : 0.0;                                     // rz = [1,0] (kind 4) / [0,1] (kind 5)
    }
  }
  return w;
}

__device__ __forceinline__ long long nco_fixed(double p) { return (long long)floor(p * kTwo60); }   // int(np.floor(p*NT*(1<<50)))
__device__ __forceinline__ bool nco_ok(double p) { return fabs(p) < 7.0; }                       // p * 2^60 fits an int64

__device__ double fll_atan(double ar, double ai, double br, double bi) {    // gnsstools/discriminator.py fll_atan
  const double pi = 3.141592653589793;
  const double t = ar == 0.0 ? pi / 2 : atan(ai / ar);
  const double t1 = br == 0.0 ? pi / 2 : atan(bi / br);
  double d = t - t1;
  if (d > pi / 2) d = pi - d;
  if (d < -pi / 2) d = -pi - d;
  return d;
}

__device__ double pll_costas(double re, double im) { return re > 0.0 ? atan2(im, re) : atan2(-im, -re); }

// nco_table = np.exp(2*pi*1j*np.arange(NT)*(1.0/NT)) (gnsstools/nco.py:3-4) in device memory, shared through the context's table cache
inline int nco_table(gacq_ctx* ctx, const double2** out) {
  // the argument is fl(2 pi k) / NT, the value (cos, sin)
  std::vector<double2> tab(kNT);
  for (int k = 0; k < kNT; k++) {
    const double y = (2.0 * M_PI * (double)k) * (1.0 / kNT);
    tab[k] = make_double2(std::cos(y), std::sin(y));
  }
  const void* d = nullptr;
  const int rc = gacq::table_cache(ctx, "track:nco1024", tab.data(), sizeof(double2) * kNT, &d);
  *out = (const double2*)d;
  return rc;
}

}  // namespace
