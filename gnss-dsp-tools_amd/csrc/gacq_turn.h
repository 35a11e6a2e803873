// Phases as 64-bit fixed-point fractions of a turn, one definition of each piece: the quarter-turn sine / cosine of the replicas
// (gacq_simcore.h: simulate, scene; gacq_cancelcore.h: cancel, aprompt; gacq_cohfold.hip), the host conversions of a double to 2^-64
// turns or chips (gacq_simcore.h, gacq_scene.hip, gacq_cancelcore.h) and the TMBOC chip mask of every file that forms a chip weight.
// cancel's replica is simulate's because both call turn_sincos on a phase that turn_fraction and turn_fixed made.
// gacq_corrgrid.hip keeps a sincos_turn of its own: a shorter polynomial with other coefficients, which tests/refine_oracle.py and
// its goldens restate.
#pragma once

#include "gacq_common.h"

#include <cmath>

namespace gacq {

// tmboc_pattern of gnsstools/gps/l1cp.py:202 as a bit mask (bits 0, 4, 6, 29 set); 64 bits: it is shifted by up to 32
constexpr unsigned long long kTmbocMask = (1ull << 0) | (1ull << 4) | (1ull << 6) | (1ull << 29);

// (cos, sin) of 2 pi ph / 2^64.  Every product and sum is spelled out (fmaf or a single operation), so the bits do not depend on
// the including file's contraction setting.
__device__ __forceinline__ void turn_sincos(unsigned long long ph, float& c, float& s) {
  const unsigned u = (unsigned)(ph >> 32) + 0x20000000u;          // + 1/8 turn: the quadrant index rounds to nearest
  const unsigned q = u >> 30;
  const float t = (float)((int)(u & 0x3fffffffu) - 0x20000000) * 9.31322574615478515625e-10f;      // quarter turns, [-1/2, 1/2)
  const float t2 = t * t;
  float ps = fmaf(t2, -4.602163099e-03f, 7.968021929e-02f);
  ps = fmaf(ps, t2, -6.459634900e-01f);
  ps = fmaf(ps, t2, 1.570796371e+00f) * t;
  float pc = fmaf(t2, 9.036298725e-04f, -2.086007036e-02f);
  pc = fmaf(pc, t2, 2.536692023e-01f);
  pc = fmaf(pc, t2, -1.233700514e+00f);
  pc = fmaf(pc, t2, 1.0f);
  const float a = (q & 1u) ? ps : pc, b = (q & 1u) ? pc : ps;     // quarter turns: (c, s), (-s, c), (-c, -s), (s, -c)
  c = __uint_as_float(__float_as_uint(a) ^ ((((q + 1u) >> 1) & 1u) << 31));
  s = __uint_as_float(__float_as_uint(b) ^ (((q >> 1) & 1u) << 31));
}

// floor(frac(v) 2^64) mod 2^64, in IEEE double operations (tests/simulate_oracle.py restates it)
inline unsigned long long turn_fraction(double v) {
  const double t = v - std::floor(v);                               // [0, 1]; 1 only when a tiny negative v rounds up
  return t >= 1.0 ? 0ull : (unsigned long long)std::floor(std::ldexp(t, 64));
}

// whole part and floor(fraction 2^64) of v >= 0
inline void turn_fixed(double v, unsigned long long& whole, unsigned long long& frac) {
  const double w = std::floor(v);
  whole = (unsigned long long)w;
  frac = (unsigned long long)std::floor(std::ldexp(v - w, 64));     // v - w is exact and below 1
}

}  // namespace gacq
