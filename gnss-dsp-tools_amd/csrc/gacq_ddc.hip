// Digital down-converter (gacq_ddc_*, include/gacq.h): a band out of a wide int8 I/Q recording -- table NCO mixer, integer FIR low-pass,
// integer decimation -- as int8 I/Q or complex64.  Output sample m is an exact function of (configuration, gain, absolute sample
// index): integer arithmetic up to one int32 -> fp32 conversion and one fp32 multiply per component, so the bytes do not depend on how
// a caller cuts the recording into calls.
//
// One kernel, two output forms.  A workgroup of 256 lanes owns `tile` outputs (tile_of(D): 1024 for D <= 8, 512 / 256 / 128 up to
// D = 16 / 32 / 64, so that D tile <= 8192 inputs and the filter's reach fit the LDS image):
//   1. Mix.  A lane takes 8 consecutive input samples with one 16-byte load (the image starts `lead` < 8 samples below the first
//      sample the tile needs, so that the load is aligned whenever d_in is even; byte loads, guarded one by one, at the edges of the
//      data and for an odd d_in; a sample that is not present reads 0), forms the 64-bit phase of its first sample with one multiply
//      and of the others by adding dP, looks the table up, multiplies in 24-bit integers and stores z as an int16 pair, one dword.
//      The mixed signal never exists in HBM.
//   2. Filter.  The image is stored in polyphase order: slot i = q D + r (r < D) of the image lies at dword r pitch + q.  The taps
//      that meet row r for output m are g[H + lead - r - t D] at q = m + t, t = 0, 1, ..: a lane that owns outputs m .. m + 3 reads
//      row r as consecutive 16-byte words (ds_read_b128; consecutive lanes 16 bytes apart, pitch a multiple of 4 dwords: aligned
//      and conflict-free for every D, where adjacent outputs read in input order would be D dwords apart, a 16- or 32-way conflict
//      at D = 16 or 32) and slides a window of eight samples over them: 32 multiply-adds (v_mad_i32_i24) per 16-byte read of samples
//      and 16-byte broadcast read of four taps.  The host lays the taps out row by row for each of the eight values of lead, zero
//      where a row's t reaches past the filter, with the number of four-tap steps of every row in front.
//      tile / 4 lanes cover the tile's outputs; for D > 8 the 1024 / tile lane groups share the rows (row r to group r mod G) and
//      their int32 partial sums are added through LDS: exact in any order, |acc| < 23171 * 65536 < 2^31.
//   3. Output.  float(acc) * (float(gain) * 2^-22), rint / clamp for int8: one 8-byte store of int8 pairs or two 16-byte stores of
//      complex64 per lane when d_out allows, single stores otherwise.
// The stores of step 1 meet up to D / 8 lanes on a bank (consecutive lanes are 8 samples apart and 8 pitch = 0 mod 32): that is free
// up to D = 16 (ds_write_b32 moves its operands in twice the array's cycles), twice the store time at 32 and four times at 64, and
// the stores are a small part of the kernel.
// GACQ_DDC_TABLE_LDS: the 16 KB table copied into LDS by every workgroup (1) or read through the vector cache (0, the product: the LDS
// form measured 1.45 to 1.53 times slower).
#pragma clang fp contract(off)

#include "gacq_common.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#ifndef GACQ_DDC_TABLE_LDS
#define GACQ_DDC_TABLE_LDS 0
#endif

using namespace gacq;

namespace {

constexpr int kDdcBlock = 256;
constexpr int kDdcRun = 4;                       // adjacent outputs per lane
constexpr int kDdcTable = 4096;
constexpr int kDdcMaxTaps = 513, kDdcMaxDecim = 64;
constexpr int kDdcLeads = 8;                     // image slot 0 lies 0..7 samples below the first sample the tile needs
constexpr int kDdcZWords = 9216;                 // >= D pitch for every (D, T): 8960 at D = 64, T = 513 (gacq_ddc_open checks)
constexpr int kDdcTapWords = 768;                // >= D nt4 for every (D, T): at D = 61..64
constexpr int kDdcLeadWords = kDdcMaxDecim + kDdcTapWords;      // per lead: the rows' step counts, then the rows' taps
constexpr unsigned kDdcMaxGrid = 1u << 16;       // workgroups; a longer call loops
constexpr bool kTableInLds = GACQ_DDC_TABLE_LDS != 0;

struct DdcLayout {
  int tile;                     // outputs per workgroup
  int gsz;                      // lanes per group, tile / 4; 256 / gsz groups share the rows
  int nt4;                      // taps per row, worst lead, a multiple of 4
  int pitch;                    // dwords per row, a multiple of 4
  int nl;                       // image slots a tile fills: D (tile - 1) + T + 7
};

int tile_of(int D) { return D <= 8 ? 1024 : D <= 16 ? 512 : D <= 32 ? 256 : 128; }

DdcLayout layout_of(int D, int T) {
  DdcLayout l;
  l.tile = tile_of(D);
  l.gsz = l.tile / kDdcRun;
  const int nt = (T + kDdcLeads - 1 + D - 1) / D;
  l.nt4 = (nt + 3) / 4 * 4;
  l.nl = D * (l.tile - 1) + T + kDdcLeads - 1;
  // a row holds what the filter reads, tile + nt4 slots, and what the mix writes: it fills whole groups of 8 slots, up to 7 past nl
  l.pitch = (std::max(l.tile + l.nt4, ((l.nl + 7) / 8 * 8 - 1) / D + 1) + 3) / 4 * 4;
  return l;
}

typedef unsigned DdcWord4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) DdcWord4 DdcLdsWord4;             // in LDS: a volatile read through a generic pointer would be a flat load

struct DdcArgs {
  const uint8_t* in;
  void* out;
  const unsigned* tab;          // 4096 x (cos | sin << 16), int16 each
  const int* taps;              // this call's lead: kDdcMaxDecim step counts, then D rows of nt4 taps
  long long nbase;              // absolute index of the input sample in image slot 0 of the call's first tile; may be negative
  long long in_first, in_count, n_out;
  unsigned long long dphase;
  unsigned long long magic;     // floor(2^32 / D) + 1: i div D = (i magic) >> 32 for i < 2^17
  float scale;                  // float(gain) * 2^-22
  int D, tile, gsz, nt4, pitch, nl;
  int wrap;                     // D pitch - 1: from the last row of slot column q to the first of q + 1
  int out_aligned;              // d_out on 8 bytes (int8) / 16 bytes (complex64)
};

__host__ __device__ __forceinline__ unsigned ddc_i8(float x) {
  const float r = fminf(fmaxf(rintf(x), -127.0f), 127.0f);            // rintf: half to even
  return (unsigned)(int)r & 0xffu;
}

// z of one sample: x conj(W), rounded to 2^-7, as an int16 pair
__device__ __forceinline__ unsigned ddc_mix(int xr, int xi, unsigned w) {
  const int c = (int)(short)(unsigned short)(w & 0xffffu), s = (int)w >> 16;
  const int pr = __mul24(xr, c) + __mul24(xi, s);
  const int pi = __mul24(xi, c) - __mul24(xr, s);
  return ((unsigned)((pr + 64) >> 7) & 0xffffu) | ((unsigned)((pi + 64) >> 7) << 16);
}

template <bool CPLX>
__global__ __launch_bounds__(kDdcBlock) void ddc_kernel(const DdcArgs a) {
  __shared__ uint4 z4[kDdcZWords / 4];
  __shared__ int4 tp4[kDdcLeadWords / 4];
  __shared__ uint4 tab4[kTableInLds ? kDdcTable / 4 : 1];
  unsigned* const z = reinterpret_cast<unsigned*>(z4);
  const int* const tp = reinterpret_cast<const int*>(tp4);
  const int tid = threadIdx.x;
  for (int i = tid; i < (kDdcMaxDecim + a.D * a.nt4) / 4; i += kDdcBlock) tp4[i] = reinterpret_cast<const int4*>(a.taps)[i];
  if (kTableInLds)
    for (int i = tid; i < kDdcTable / 4; i += kDdcBlock) tab4[i] = reinterpret_cast<const uint4*>(a.tab)[i];
  const unsigned* const tab = kTableInLds ? reinterpret_cast<const unsigned*>(tab4) : a.tab;
  if (kTableInLds) __syncthreads();                                   // the first mix reads table entries that other lanes brought in
  const int grp = tid / a.gsz, l4 = tid - grp * a.gsz, ngrp = kDdcBlock / a.gsz;
  const long long ntiles = (a.n_out + a.tile - 1) / a.tile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long m0 = tile * a.tile;                               // offset of the tile's first output from out_first
    const long long n_tile = a.nbase + m0 * a.D;                      // the sample in image slot 0
    // ---- mix: eight samples a lane and pass
    for (int c = tid; 8 * c < a.nl; c += kDdcBlock) {
      const int i0 = 8 * c;
      const long long n0 = n_tile + i0, rel = n0 - a.in_first;
      const uint8_t* p = a.in + 2 * rel;
      unsigned w[4] = {0u, 0u, 0u, 0u};
      if (rel >= 0 && rel + 8 <= a.in_count && ((uintptr_t)p % 16u) == 0u) {
        const uint4 v = *reinterpret_cast<const uint4*>(p);
        w[0] = v.x;
        w[1] = v.y;
        w[2] = v.z;
        w[3] = v.w;
      } else {
#pragma unroll
        for (int s = 0; s < 8; s++)
          if (rel + s >= 0 && rel + s < a.in_count) w[s >> 1] |= ((unsigned)p[2 * s] | ((unsigned)p[2 * s + 1] << 8)) << (16 * (s & 1));
      }
      const int q = (int)(((unsigned long long)(unsigned)i0 * a.magic) >> 32);
      int r = i0 - q * a.D;
      int at = __mul24(r, a.pitch) + q;                                 // slot q D + r lies at r pitch + q
      unsigned long long ph = (unsigned long long)n0 * a.dphase;
#pragma unroll
      for (int s = 0; s < 8; s++) {                                     // the pass's last lane may fill up to 7 slots past nl: the pitch has room
        const unsigned v = w[s >> 1] >> (16 * (s & 1));
        const int xr = (int)(signed char)(unsigned char)(v & 0xffu), xi = (int)(signed char)(unsigned char)((v >> 8) & 0xffu);
        z[at] = ddc_mix(xr, xi, tab[(unsigned)(ph >> 52)]);
        ph += a.dphase;
        at += a.pitch;
        if (++r == a.D) {
          r = 0;
          at -= a.wrap;
        }
      }
    }
    __syncthreads();
    // ---- filter: outputs 4 l4 .. 4 l4 + 3 of the tile, the rows grp, grp + ngrp, ..
    int ar[kDdcRun] = {0, 0, 0, 0}, ai[kDdcRun] = {0, 0, 0, 0};
    for (int r = grp; r < a.D; r += ngrp) {
      // volatile: the reads stay whole, aligned 16-byte loads (left to itself the compiler moves the window by one sample, which
      // spares a register and turns every read into four single ones with a four-way bank conflict)
      const volatile DdcLdsWord4* row = (const volatile DdcLdsWord4*)z4 + (r * a.pitch) / 4 + l4;
      const int4* g4 = tp4 + (kDdcMaxDecim + r * a.nt4) / 4;
      const int steps = tp[r];
      DdcWord4 prev = row[0];
      for (int c = 0; c < steps; c++) {
        const DdcWord4 cur = row[c + 1];
        const int4 g = g4[c];
        const unsigned u[8] = {prev.x, prev.y, prev.z, prev.w, cur.x, cur.y, cur.z, cur.w};
        int wr[8], wi[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
          wr[k] = (int)(short)(unsigned short)(u[k] & 0xffffu);
          wi[k] = (int)u[k] >> 16;
        }
        const int gt[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
          for (int i = 0; i < kDdcRun; i++) {
            ar[i] += __mul24(gt[t], wr[i + t]);
            ai[i] += __mul24(gt[t], wi[i + t]);
          }
        prev = cur;
      }
    }
    if (ngrp > 1) {                                                   // the groups' partial sums through LDS, over the image
      __syncthreads();
      int4* red = reinterpret_cast<int4*>(z4);
      red[2 * tid] = make_int4(ar[0], ar[1], ar[2], ar[3]);
      red[2 * tid + 1] = make_int4(ai[0], ai[1], ai[2], ai[3]);
      __syncthreads();
      if (grp == 0)
        for (int g = 1; g < ngrp; g++) {
          const int4 pr = red[2 * (g * a.gsz + l4)], pi = red[2 * (g * a.gsz + l4) + 1];
          ar[0] += pr.x;
          ar[1] += pr.y;
          ar[2] += pr.z;
          ar[3] += pr.w;
          ai[0] += pi.x;
          ai[1] += pi.y;
          ai[2] += pi.z;
          ai[3] += pi.w;
        }
    }
    // ---- output
    const long long m = m0 + kDdcRun * l4, left = a.n_out - m;
    if (grp == 0 && left > 0) {
      float vr[kDdcRun], vi[kDdcRun];
#pragma unroll
      for (int i = 0; i < kDdcRun; i++) {
        vr[i] = (float)ar[i] * a.scale;
        vi[i] = (float)ai[i] * a.scale;
      }
      if (CPLX) {
        float2* __restrict__ o = reinterpret_cast<float2*>(a.out) + m;
        if (left >= kDdcRun && a.out_aligned) {
          reinterpret_cast<float4*>(o)[0] = make_float4(vr[0], vi[0], vr[1], vi[1]);
          reinterpret_cast<float4*>(o)[1] = make_float4(vr[2], vi[2], vr[3], vi[3]);
        } else {
#pragma unroll
          for (int i = 0; i < kDdcRun; i++)
            if (i < left) o[i] = make_float2(vr[i], vi[i]);
        }
      } else {
        uint8_t* __restrict__ o = reinterpret_cast<uint8_t*>(a.out) + 2 * m;
        unsigned b[2 * kDdcRun];
#pragma unroll
        for (int i = 0; i < kDdcRun; i++) {
          b[2 * i] = ddc_i8(vr[i]);
          b[2 * i + 1] = ddc_i8(vi[i]);
        }
        if (left >= kDdcRun && a.out_aligned) {
          *reinterpret_cast<uint2*>(o) = make_uint2(b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24), b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24));
        } else {
#pragma unroll
          for (int i = 0; i < kDdcRun; i++)
            if (i < left) {
              o[2 * i] = (uint8_t)b[2 * i];
              o[2 * i + 1] = (uint8_t)b[2 * i + 1];
            }
        }
      }
    }
    __syncthreads();
  }
}

void ddc_table(int16_t* w) {
  for (int t = 0; t < kDdcTable; t++) {
    const double ph = 2.0 * M_PI * (double)t / (double)kDdcTable;
    w[2 * t] = (int16_t)std::rint(16384.0 * std::cos(ph));
    w[2 * t + 1] = (int16_t)std::rint(16384.0 * std::sin(ph));
  }
}

}  // namespace

#include "gacq_streamhost.h"

struct gacq_ddc {
  gacq_ctx* ctx = nullptr;
  gacq_ddc_cfg cfg{};
  std::vector<int32_t> taps;
  DdcLayout lay{};
  StDevBlock dev;               // the table, then kDdcLeads tap layouts
};

extern "C" int gacq_ddc_tile(int D) {
  if (D < 1 || D > kDdcMaxDecim) return GACQ_ERR_BAD_ARG;
  return tile_of(D);
}

extern "C" int gacq_ddc_table(int16_t* table) {
  if (!table) return GACQ_ERR_BAD_ARG;
  ddc_table(table);
  return GACQ_OK;
}

extern "C" int gacq_ddc_check(const gacq_ddc_cfg* cfg, const int32_t* taps, int T, long long in_first, long long in_count, long long out_first,
                              long long n_out, double gain, int out_complex64) {
  (void)out_complex64;
  if (!cfg || !taps) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_ddc: NULL argument");
  if (cfg->decim < 1 || cfg->decim > kDdcMaxDecim)
    return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_ddc: the decimation %d lies outside 1..%d", cfg->decim, kDdcMaxDecim);
  if (T < 1 || T > kDdcMaxTaps || !(T & 1)) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_ddc: %d taps: need an odd number in 1..%d", T, kDdcMaxTaps);
  long long sum = 0;
  for (int k = 0; k < T; k++) sum += std::llabs((long long)taps[k]);
  if (sum > 65536) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_ddc: the taps' magnitudes sum to %lld, above 65536", sum);
  int rc = st_check_gain(nullptr, "gacq_ddc", "must be finite and positive in fp32", gain);
  if (rc == GACQ_OK) rc = st_check_range(nullptr, "gacq_ddc", in_first, in_count, out_first, n_out);
  if (rc < 0 || n_out == 0) return rc;
  const long long H = T / 2, D = cfg->decim;
  return st_check_support(nullptr, "gacq_ddc", out_first, n_out, std::max(0ll, out_first * D - H), (out_first + n_out - 1) * D + H, in_first, in_count);
}

extern "C" int gacq_ddc_open(gacq_ctx* ctx, const gacq_ddc_cfg* cfg, const int32_t* taps, int T, gacq_ddc** out) {
  if (!ctx) return GACQ_ERR_BAD_ARG;
  if (!out) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_ddc_open: NULL argument");
  *out = nullptr;
  const int rc = gacq_ddc_check(cfg, taps, T, 0, 0, 0, 0, 1.0, 0);
  if (rc < 0) return st_forward(ctx, rc);
  const int D = cfg->decim, H = T / 2;
  const DdcLayout lay = layout_of(D, T);
  if (D * lay.pitch > kDdcZWords || D * lay.nt4 > kDdcTapWords || 2 * kDdcBlock * 4 > kDdcZWords)
    return set_error(ctx, GACQ_ERR_INTERNAL, "gacq_ddc_open: the image of D = %d, T = %d does not fit", D, T);
  std::vector<int> host(kDdcTable + kDdcLeads * kDdcLeadWords, 0);
  ddc_table(reinterpret_cast<int16_t*>(host.data()));
  for (int lead = 0; lead < kDdcLeads; lead++) {
    int* steps = host.data() + kDdcTable + lead * kDdcLeadWords;
    int* rows = steps + kDdcMaxDecim;
    for (int r = 0; r < D; r++) {
      // image slot (m D + lead) + j holds input m D - H + j, which meets g[H - j]: row r, step t has j = t D + r - lead
      int last = -1;
      for (int t = 0; t < lay.nt4; t++) {
        const int j = t * D + r - lead;
        if (j >= 0 && j < T) {
          rows[r * lay.nt4 + t] = taps[2 * H - j];                   // taps[] holds g[-H .. H]: g[H - j] is taps[2 H - j]
          last = t;
        }
      }
      steps[r] = (last + 4) / 4;
    }
  }
  std::unique_ptr<gacq_ddc> h(new gacq_ddc);
  h->ctx = ctx;
  h->cfg = *cfg;
  h->taps.assign(taps, taps + T);
  h->lay = lay;
  {
    GACQ_DEVICE(ctx);
    hipError_t e = h->dev.alloc(ctx, host.size() * sizeof(int));
    if (e == hipSuccess) e = h->dev.upload(0, host.data(), host.size() * sizeof(int));
    if (e != hipSuccess) return set_error(ctx, GACQ_ERR_HIP, "gacq_ddc_open: %s", hipGetErrorString(e));
  }
  *out = h.release();
  return GACQ_OK;
}

extern "C" void gacq_ddc_close(gacq_ddc* h) { delete h; }

extern "C" int gacq_ddc_run_dev(gacq_ddc* h, const void* d_in, long long in_first, long long in_count, long long out_first, long long n_out,
                                double gain, int out_complex64, void* d_out) {
  if (!h) return GACQ_ERR_BAD_ARG;
  gacq_ctx* ctx = h->ctx;
  if (!d_in || !d_out) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_ddc_run_dev: NULL argument");
  // everything is checked before anything is launched
  const int T = (int)h->taps.size(), H = T / 2, D = h->cfg.decim;
  const int rc = gacq_ddc_check(&h->cfg, h->taps.data(), T, in_first, in_count, out_first, n_out, gain, out_complex64);
  if (rc < 0) return st_forward(ctx, rc);
  if (out_complex64 && (uintptr_t)d_out % 8u) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_ddc_run_dev: complex64 output must be 8-byte aligned");
  if (n_out == 0) return GACQ_OK;
  // slot 0 of a tile's image: `lead` samples below the first one the tile needs, on a 16-byte boundary of an even d_in (a tile's
  // inputs are a multiple of 8 samples, so one lead serves every tile)
  const long long first_needed = out_first * D - H;
  const long long addr = (long long)((uintptr_t)d_in % 16u) + 2 * ((first_needed - in_first) % 8);
  const int lead = ((uintptr_t)d_in & 1u) ? 0 : (int)(((addr % 16 + 16) % 16) / 2);
  DdcArgs a;
  a.in = (const uint8_t*)d_in;
  a.out = d_out;
  a.tab = (const unsigned*)h->dev.p;
  a.taps = (const int*)h->dev.p + kDdcTable + lead * kDdcLeadWords;
  a.nbase = first_needed - lead;
  a.in_first = in_first;
  a.in_count = in_count;
  a.n_out = n_out;
  a.dphase = h->cfg.dphase;
  a.magic = (1ull << 32) / (unsigned)D + 1ull;
  a.scale = (float)gain * 2.384185791015625e-07f;                    // 2^-22
  a.D = D;
  a.tile = h->lay.tile;
  a.gsz = h->lay.gsz;
  a.nt4 = h->lay.nt4;
  a.pitch = h->lay.pitch;
  a.nl = h->lay.nl;
  a.wrap = D * h->lay.pitch - 1;
  a.out_aligned = ((uintptr_t)d_out % (out_complex64 ? 16u : 8u)) == 0u;
  GACQ_DEVICE(ctx);
  const long long ntiles = (n_out + a.tile - 1) / a.tile;
  const unsigned grid = (unsigned)std::min<long long>(ntiles, (long long)kDdcMaxGrid);
  if (out_complex64) hipLaunchKernelGGL((ddc_kernel<true>), dim3(grid), dim3(kDdcBlock), 0, ctx->stream, a);
  else hipLaunchKernelGGL((ddc_kernel<false>), dim3(grid), dim3(kDdcBlock), 0, ctx->stream, a);
  return st_launched(ctx, "gacq_ddc_run_dev");
}
