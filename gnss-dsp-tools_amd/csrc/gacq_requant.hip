// Level control and requantiser (gacq_requant_*, include/gacq.h): interleaved int8 or int16 I/Q under a block-wise gain into any of
// ingest's containers -- int8, offset uint8, int16, complex64 or 1 / 2 / 4-bit codes packed into bytes.  The gain of block b is a table
// entry chosen by integer comparisons of a sliding sum of block powers, so every output byte is an exact function of (configuration,
// tables, absolute sample index) and does not depend on how a caller cuts the recording into calls.
//
// Two launches per call (per 2^16 blocks or 2^28 components), on one stream:
//   requant_power_kernel     P(b) of every block the call's levels need, into the handle's workspace.  A group of gs lanes owns a block: the
//      power of two at or above the block's 16-byte words up to 64 (a group never spans two waves; 65 .. 255 words take 64 lanes and up
//      to 4 words a lane), the whole workgroup of 256 from 256 words on: 16-byte loads, int8 squares through
//      the packed dot instruction, int16 squares into 64-bit accumulators, the group's sum on wave shuffles and, for a group of 256,
//      across the four waves through LDS; plain vector stores.
//   requant_quantize_kernel  the I/Q stream is handled as a stream of components (component c belongs to sample c div 2, block
//      c div 2 Lb), so that input and output are both contiguous runs.  A lane owns the 16 output bytes at a 16-byte boundary of the
//      output's ADDRESS -- one store per lane whatever d_out and out_first are; only the lanes that overlap the ends of the output range
//      store single bytes.  A workgroup owns 32768 components, 1 to 32 such runs a lane (run r of a lane is run 256 r + lane of the
//      workgroup: 256 runs a workgroup made the chain powers -> level -> gain -> LDS -> barrier in front of every workgroup's work the
//      larger part of the time).  It first forms the gains of the blocks its runs meet: a wave takes a block, sums the W powers at wave-uniform addresses, compares the sum with the thresholds spread over its lanes (four a lane), counts
//      the set bits of the ballots and leaves G[k] in LDS; the workgroup that meets a block's first sample writes its k(b).
//      A lane then works through its run in pieces of at most 32 components: a piece meets at most one block boundary (2 Lb >= 32
//      components), so it takes two gains from LDS and every component picks one by its position: where out_first and d_out are
//      multiples of 16 no piece straddles, and where they are not the store is as wide.  The input of a whole run is read with 16-byte
//      loads at any address (a byte-aligned copy, for which the compiler emits the wide load), element by element only in the runs
//      over the ends of the range, where a component outside it reads 0.
//      Codes are packed first code lowest; for msb_first the groups of every byte are then reversed with three masks a dword.
#pragma clang fp contract(off)

#include "gacq_common.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

using namespace gacq;

namespace {

constexpr int kRqBlock = 256;
constexpr int kRqMaxGains = 256, kRqMaxWindow = 64, kRqMaxLb = 65536;
constexpr long long kRqChunkBlocks = 1ll << 16;      // blocks whose outputs one pair of launches writes, at most
constexpr long long kRqChunkComps = 1ll << 28;       // ... and components: the quantize kernel counts them, and the output's bytes, in 32 bits
constexpr unsigned kRqMaxGrid = 1u << 16;            // workgroups; a longer call loops
constexpr int kRqGainSlots = 1032;                   // >= 256 * 128 / 32 + 2: the blocks one workgroup's runs can meet, and one more

// ---- block powers

struct RqPowerArgs {
  const uint8_t* in;            // the address of input sample in_first
  unsigned long long* P;        // P[i] is block pb0 + i
  long long pb0, nblk, in_first;
  int Lb;
  int words;                    // 16-byte words per block
  int gs, gs_log2;              // lanes per block: a power of two in 2..64, inside one wave, or the whole workgroup of 256
};

template <bool IN16>
__global__ __launch_bounds__(kRqBlock) void requant_power_kernel(const RqPowerArgs a) {
  __shared__ unsigned long long red[kRqBlock / 64];
  const int tid = threadIdx.x;
  const int grp = tid >> a.gs_log2, lig = tid & (a.gs - 1), per = kRqBlock >> a.gs_log2;
  const long long npass = (a.nblk + per - 1) / per;
  for (long long pass = blockIdx.x; pass < npass; pass += gridDim.x) {
    const long long bl = pass * per + grp;
    unsigned long long acc = 0;
    if (bl < a.nblk) {
      const uint8_t* p = a.in + ((a.pb0 + bl) * a.Lb - a.in_first) * (IN16 ? 4 : 2);
      if (IN16) {
        for (int g = lig; g < a.words; g += a.gs) {
          const uint4 v = load16_any(p + 16 * (long long)g);
          const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const int lo = (int)(short)(unsigned short)(w[i] & 0xffffu), hi = (int)w[i] >> 16;
            acc += (unsigned long long)((unsigned)(lo * lo) + (unsigned)(hi * hi));         // each square <= 2^30
          }
        }
      } else {
        int s = 0;                                                      // <= 32 words a lane (4 in a group of 64), 2^18 a word
        for (int g = lig; g < a.words; g += a.gs) {
          const uint4 v = load16_any(p + 16 * (long long)g);
          s = __builtin_amdgcn_sdot4((int)v.x, (int)v.x, s, false);
          s = __builtin_amdgcn_sdot4((int)v.y, (int)v.y, s, false);
          s = __builtin_amdgcn_sdot4((int)v.z, (int)v.z, s, false);
          s = __builtin_amdgcn_sdot4((int)v.w, (int)v.w, s, false);
        }
        acc = (unsigned long long)(unsigned)s;
      }
    }
    const int span = a.gs < 64 ? a.gs : 64;
    for (int off = 1; off < span; off <<= 1) acc += __shfl_xor(acc, off, 64);
    if (a.gs == kRqBlock) {                                             // one block a workgroup: the four waves' sums through LDS
      if ((tid & 63) == 0) red[tid >> 6] = acc;
      __syncthreads();
      if (tid == 0) a.P[bl] = red[0] + red[1] + red[2] + red[3];
      __syncthreads();
    } else if (lig == 0 && bl < a.nblk) {
      a.P[bl] = acc;
    }
  }
}

// ---- gains and outputs

enum { kS8 = 0, kU8 = 1, kS16 = 2, kF32 = 3, kP1 = 4, kP2 = 5, kP4 = 6 };     // the kernel's forms: PACKED by its bits

template <int FORM>
struct RqForm {
  static constexpr int bits = FORM == kP1 ? 1 : FORM == kP2 ? 2 : FORM == kP4 ? 4 : 0;
  static constexpr bool packed = bits != 0;
  static constexpr int run = FORM == kS16 ? 8 : FORM == kF32 ? 4 : packed ? 128 / (bits ? bits : 1) : 16;    // components in 16 output bytes
  static constexpr int piece = run < 32 ? run : bits == 4 ? 16 : 32;      // 4-bit codes in two pieces: the registers of 32 at once pass 128
  static constexpr int pieces = run / piece;
  static constexpr int odw = 4 / pieces;                                // output dwords a piece fills
  static constexpr int runs = 128 / run;                                // runs a lane works through: a workgroup owns 32768 components in every form
};

struct RqQuantArgs {              // one launch writes fewer than 2^28 components: everything but the addresses is 32 bits, relative to the launch
  const uint8_t* in;            // the address of the input component of output component 0
  uint8_t* out;                 // the address of output byte 0
  const unsigned long long* P;  // P[p_off + i - W] is the first power under the level of block b_first + i, once the warm-up is over
  const float* G;
  const unsigned long long* T;  // 256 entries, 2^64 - 1 from K - 1 on
  unsigned long long* stats;
  uint8_t* gidx;                // k(b) of block b_first + i at gidx[i]: the caller's pointer moved to b_first (which may lie one before it)
  unsigned long long enc;       // enc[q] in nibble q
  int ncomp;                    // output components
  int nbytes;                   // output bytes
  int nlanes;                   // 16-byte runs that overlap the output
  int r_first;                  // output component 0 is component r_first of its block, b_first
  int p_off;                    // b_first less the block of P[0]
  int warm;                     // blocks b_first + i with i < warm are in the warm-up: their level is P[0 .. W - 1]
  int a0;                       // d_out mod 16: run 0 starts a0 bytes below output byte 0
  int hc;                       // ... which is hc components
  unsigned twoLb;
  int W, msb;
};

// the groups of every byte in reverse order: code i from bit bits i to bit 8 - bits (i + 1)
template <int BITS>
__device__ __forceinline__ unsigned rq_reverse_groups(unsigned x) {
  if (BITS == 1) return __builtin_bswap32(__builtin_bitreverse32(x));
  if (BITS == 2) return ((x & 0x03030303u) << 6) | ((x & 0x0c0c0c0cu) << 2) | ((x >> 2) & 0x0c0c0c0cu) | ((x >> 6) & 0x03030303u);
  return ((x & 0x0f0f0f0fu) << 4) | ((x >> 4) & 0x0f0f0f0fu);
}

template <int FORM, bool IN16>
__global__ __launch_bounds__(kRqBlock) void requant_quantize_kernel(const RqQuantArgs a) {
  typedef RqForm<FORM> F;
  constexpr int kEsz = IN16 ? 2 : 1;                                    // bytes per input component
  constexpr int kInBytes = F::piece * kEsz;                             // input bytes per piece: 4 .. 64
  constexpr int kInWords = kInBytes / 4;
  __shared__ float gl[kRqGainSlots];
  __shared__ unsigned cnt[2];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  constexpr int tile_runs = kRqBlock * F::runs, tile_comps = tile_runs * F::run;
  const int ntiles = (a.nlanes + tile_runs - 1) / tile_runs;
  // a lane's four thresholds: T[lane], T[lane + 64], ..; past the table's K - 1 entries stands 2^64 - 1, which no level exceeds
  unsigned long long thr[4];
#pragma unroll
  for (int i = 0; i < 4; i++) thr[i] = a.T[lane + 64 * i];
  if (tid == 0) cnt[0] = cnt[1] = 0u;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    // components count from output component 0 of the launch; the tile's first run starts at c_tile (below 0 at most in tile 0)
    const int c_tile = tile * tile_comps - a.hc;
    const int t_lo = c_tile > 0 ? c_tile : 0;
    const int t_hi = c_tile + tile_comps < a.ncomp ? c_tile + tile_comps : a.ncomp;        // the tile's outputs: t_lo .. t_hi - 1, never empty
    const int b_t = (int)((unsigned)(a.r_first + t_lo) / a.twoLb), b_last = (int)((unsigned)(a.r_first + t_hi - 1) / a.twoLb);  // blocks from b_first
    const int B0 = (int)((unsigned)b_t * a.twoLb) - a.r_first;                             // where block b_t starts
    const int nb = b_last - b_t + 1;                                    // <= tile_comps / 32 + 1
    const int base_u = c_tile - B0, lo_u = t_lo - B0, hi_u = t_hi - B0; // relative to that start
    // ---- the gains of blocks b_t .. b_last
    unsigned owned = 0;
    for (int i = wave; i < nb; i += kRqBlock / 64) {
      const int b = b_t + i;
      const unsigned long long* p = a.P + (b >= a.warm ? a.p_off + b - a.W : 0);
      unsigned long long S = 0;
      for (int j = 0; j < a.W; j++) S += p[j];
      int k = 0;
#pragma unroll
      for (int t = 0; t < 4; t++) k += __builtin_popcountll(__builtin_amdgcn_ballot_w64(S > thr[t]));
      if (lane == 0) {
        gl[i] = a.G[k];
        if ((long long)i * a.twoLb >= (long long)lo_u) {                // the block's first sample is one of the tile's outputs
          owned++;
          if (a.gidx) a.gidx[b] = (uint8_t)k;
        }
      }
    }
    if (tid == 0) gl[nb] = 0.0f;                                        // the block past the tile's outputs: read, never used
    __syncthreads();
    // ---- the outputs
    unsigned nclip = 0;
    // run r of the lane is run r * 256 + tid of the tile: the lanes of a wave store 1 KB in a row
#pragma unroll 1
    for (int rt = tid; rt < tile_runs; rt += kRqBlock) {
      const int L = tile * tile_runs + rt;
      if (L >= a.nlanes) break;
      const int u0 = base_u + rt * F::run;
      const bool full = u0 >= lo_u && u0 + F::run <= hi_u;
      const uint8_t* pin = a.in + (long long)(c_tile + rt * F::run) * kEsz;
      unsigned o[4] = {0u, 0u, 0u, 0u};
#pragma unroll 1
      for (int s = 0; s < F::pieces; s++) {
        const int us = u0 + s * F::piece;
        const unsigned ub = us > 0 ? (unsigned)us : 0u;
        unsigned lb = ub / a.twoLb;
        lb = lb < (unsigned)nb ? lb : (unsigned)nb - 1u;                // past the outputs' end: any slot will do
        const int nfirst = (int)((lb + 1u) * a.twoLb) - us;             // the piece's components in block lb; the others are in the next
        // ... as a bit mask: a component picks its gain with two bit-field instructions, where 32 compares would hold 32 lane masks
        const unsigned first = nfirst >= 32 ? 0xffffffffu : (1u << (nfirst > 0 ? nfirst : 0)) - 1u;
        const unsigned g0 = __builtin_bit_cast(unsigned, gl[lb]), g1 = __builtin_bit_cast(unsigned, gl[lb + 1u]);
        const uint8_t* ps = pin + s * kInBytes;
        unsigned w[kInWords];
        if (full) {
          __builtin_memcpy(w, ps, kInBytes);                            // whole 16-byte loads (8, 4 for the short runs) at any address
        } else {
          // a run over an end of the range: element by element, each shifted in from below, last one first
#pragma unroll
          for (int i = 0; i < kInWords; i++) w[i] = 0u;
#pragma unroll 1
          for (int e = F::piece - 1; e >= 0; e--) {
            unsigned x = 0u;
            if (us + e >= lo_u && us + e < hi_u) x = IN16 ? (unsigned)reinterpret_cast<const unsigned short*>(ps)[e] : (unsigned)ps[e];
#pragma unroll
            for (int i = kInWords - 1; i > 0; i--) w[i] = (w[i] << (8 * kEsz)) | (w[i - 1] >> (32 - 8 * kEsz));
            w[0] = (w[0] << (8 * kEsz)) | x;
          }
        }
        unsigned q[F::odw];
#pragma unroll
        for (int i = 0; i < F::odw; i++) q[i] = 0u;
#pragma unroll
        for (int e = 0; e < F::piece; e++) {
          const int x = IN16 ? (int)(short)(unsigned short)((w[e >> 1] >> (16 * (e & 1))) & 0xffffu)
                             : (int)(signed char)(unsigned char)((w[e >> 2] >> (8 * (e & 3))) & 0xffu);
          const unsigned pick = (unsigned)((int)(first << (31 - e)) >> 31);            // all ones in block lb
          const float v = (float)x * __builtin_bit_cast(float, (g0 & pick) | (g1 & ~pick));   // a component outside the range is 0 here: it clips nothing
          if constexpr (FORM == kF32) {
            q[e] = __builtin_bit_cast(unsigned, v);
          } else if constexpr (F::packed) {
            constexpr int n = 1 << F::bits;
            const float f = floorf(v * 0.5f) + (float)(n / 2);
            const float qf = fminf(fmaxf(f, 0.0f), (float)(n - 1));
            nclip += qf != f ? 1u : 0u;
            const unsigned code = (unsigned)(a.enc >> (4 * (int)qf)) & 15u;
            q[(e * F::bits) / 32] |= code << ((e * F::bits) % 32);
          } else {
            const float lim = FORM == kS16 ? 32767.0f : 127.0f;
            const float r = rintf(v);                                   // half to even
            const float c = fminf(fmaxf(r, -lim), lim);
            nclip += c != r ? 1u : 0u;
            if constexpr (FORM == kS16) q[e >> 1] |= ((unsigned)(int)c & 0xffffu) << (16 * (e & 1));
            else q[e >> 2] |= (((unsigned)(int)c + (FORM == kU8 ? 128u : 0u)) & 0xffu) << (8 * (e & 3));
          }
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (i / F::odw == s) o[i] = q[i % F::odw];
      }
      if (F::packed && a.msb) {
#pragma unroll
        for (int i = 0; i < 4; i++) o[i] = rq_reverse_groups<F::packed ? F::bits : 1>(o[i]);
      }
      uint8_t* po = a.out + ((long long)16 * L - a.a0);
      if (full) {
        *reinterpret_cast<uint4*>(po) = make_uint4(o[0], o[1], o[2], o[3]);
      } else {
        const int beta = 16 * L - a.a0;
#pragma unroll
        for (int kb = 0; kb < 16; kb++)
          if (beta + kb >= 0 && beta + kb < a.nbytes) po[kb] = (uint8_t)(o[kb >> 2] >> (8 * (kb & 3)));
      }
    }
    if (a.stats) {
      for (int off = 1; off < 64; off <<= 1) nclip += __shfl_xor(nclip, off, 64);
      if (lane == 0) {
        if (nclip) atomicAdd(&cnt[0], nclip);
        if (owned) atomicAdd(&cnt[1], owned);
      }
    }
    __syncthreads();
    if (tid == 0 && a.stats) {
      if (cnt[0]) atomicAdd(a.stats, (unsigned long long)cnt[0]);
      if (cnt[1]) atomicAdd(a.stats + 1, (unsigned long long)cnt[1]);
      cnt[0] = cnt[1] = 0u;
    }
  }
}

int form_of(const gacq_requant_cfg& c) {
  if (c.container == GACQ_INGEST_PACKED) return c.bits == 1 ? kP1 : c.bits == 2 ? kP2 : kP4;
  return c.container;                                                   // S8, U8, S16, F32 are 0 .. 3
}

int run_of(int form) {
  switch (form) {
    case kS16: return RqForm<kS16>::run;
    case kF32: return RqForm<kF32>::run;
    case kP1: return RqForm<kP1>::run;
    case kP2: return RqForm<kP2>::run;
    case kP4: return RqForm<kP4>::run;
    default: return RqForm<kS8>::run;
  }
}

template <bool IN16>
void launch_quantize(int form, unsigned grid, hipStream_t stream, const RqQuantArgs& a) {
  switch (form) {
    case kS8: hipLaunchKernelGGL((requant_quantize_kernel<kS8, IN16>), dim3(grid), dim3(kRqBlock), 0, stream, a); break;
    case kU8: hipLaunchKernelGGL((requant_quantize_kernel<kU8, IN16>), dim3(grid), dim3(kRqBlock), 0, stream, a); break;
    case kS16: hipLaunchKernelGGL((requant_quantize_kernel<kS16, IN16>), dim3(grid), dim3(kRqBlock), 0, stream, a); break;
    case kF32: hipLaunchKernelGGL((requant_quantize_kernel<kF32, IN16>), dim3(grid), dim3(kRqBlock), 0, stream, a); break;
    case kP1: hipLaunchKernelGGL((requant_quantize_kernel<kP1, IN16>), dim3(grid), dim3(kRqBlock), 0, stream, a); break;
    case kP2: hipLaunchKernelGGL((requant_quantize_kernel<kP2, IN16>), dim3(grid), dim3(kRqBlock), 0, stream, a); break;
    default: hipLaunchKernelGGL((requant_quantize_kernel<kP4, IN16>), dim3(grid), dim3(kRqBlock), 0, stream, a); break;
  }
}

int check_cfg(const gacq_requant_cfg* c, const float* gains, const uint64_t* thresholds) {
  if (!c || !gains) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_requant: NULL argument");
  if (c->in_bits != 8 && c->in_bits != 16) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_requant: in_bits is 8 or 16, not %d", c->in_bits);
  if (c->container < GACQ_INGEST_S8 || c->container > GACQ_INGEST_PACKED)
    return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_requant: unknown container %d", c->container);
  if (c->block < 16 || c->block > kRqMaxLb || c->block % 16)
    return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_requant: the block length %d is no multiple of 16 in 16..%d", c->block, kRqMaxLb);
  if (c->window < 1 || c->window > kRqMaxWindow)
    return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_requant: the window %d lies outside 1..%d", c->window, kRqMaxWindow);
  if (c->ngains < 1 || c->ngains > kRqMaxGains)
    return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_requant: %d gains: need 1..%d", c->ngains, kRqMaxGains);
  if (c->ngains > 1 && !thresholds) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_requant: NULL thresholds");
  if (c->container == GACQ_INGEST_PACKED) {
    if (c->bits != 1 && c->bits != 2 && c->bits != 4) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_requant: %d bits per code: need 1, 2 or 4", c->bits);
    const int n = 1 << c->bits;
    unsigned seen = 0;
    for (int q = 0; q < n; q++)
      if (c->enc[q] < n) seen |= 1u << c->enc[q];
    if (seen != (1u << n) - 1u) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_requant: enc is no permutation of 0..%d", n - 1);
  }
  for (int k = 0; k < c->ngains; k++)
    if (!std::isfinite(gains[k]) || !(gains[k] > 0.0f))
      return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_requant: gain %d is not finite and positive (%g)", k, (double)gains[k]);
  for (int k = 1; k < c->ngains - 1; k++)
    if (thresholds[k] < thresholds[k - 1]) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_requant: threshold %d lies below threshold %d", k, k - 1);
  return GACQ_OK;
}

}  // namespace

#include "gacq_streamhost.h"

struct gacq_requant {
  gacq_ctx* ctx = nullptr;
  gacq_requant_cfg cfg{};
  std::vector<float> gains;
  std::vector<uint64_t> thresholds;
  StDevBlock dev;               // 256 thresholds, the block powers of a pair of launches, 256 gains
};

extern "C" int gacq_requant_tile(const gacq_requant_cfg* cfg) {
  if (!cfg) return GACQ_ERR_BAD_ARG;
  const float one = 1.0f;
  const uint64_t none = 0;
  gacq_requant_cfg c = *cfg;
  c.ngains = 1;
  if (check_cfg(&c, &one, &none) < 0) return GACQ_ERR_BAD_ARG;
  return kRqBlock * 128 / 2;                                             // 32768 components in every form
}

extern "C" int gacq_requant_check(const gacq_requant_cfg* cfg, const float* gains, const uint64_t* thresholds, long long in_first, long long in_count,
                                  long long out_first, long long n_out) {
  int rc = check_cfg(cfg, gains, thresholds);
  if (rc == GACQ_OK) rc = st_check_range(nullptr, "gacq_requant", in_first, in_count, out_first, n_out);
  if (rc < 0) return rc;
  if (cfg->container == GACQ_INGEST_PACKED) {
    const int unit = 4 / cfg->bits;
    if (out_first % unit || n_out % unit)
      return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_requant: out_first and n_out must be multiples of the %d samples of a byte (%lld, %lld)", unit,
                       out_first, n_out);
  }
  if (n_out == 0) return GACQ_OK;
  return st_check_block_support(nullptr, "gacq_requant", cfg->block, cfg->window, out_first, n_out, in_first, in_count);
}

extern "C" int gacq_requant_open(gacq_ctx* ctx, const gacq_requant_cfg* cfg, const float* gains, const uint64_t* thresholds, gacq_requant** out) {
  if (!ctx) return GACQ_ERR_BAD_ARG;
  if (!out) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_requant_open: NULL argument");
  *out = nullptr;
  const int rc = gacq_requant_check(cfg, gains, thresholds, 0, 0, 0, 0);
  if (rc < 0) return st_forward(ctx, rc);
  std::unique_ptr<gacq_requant> h(new gacq_requant);
  h->ctx = ctx;
  h->cfg = *cfg;
  h->gains.assign(gains, gains + cfg->ngains);
  h->thresholds.assign(kRqMaxGains, ~0ull);
  for (int k = 0; k + 1 < cfg->ngains; k++) h->thresholds[k] = thresholds[k];
  const size_t words = kRqMaxGains + (size_t)(kRqChunkBlocks + kRqMaxWindow);
  std::vector<float> g(kRqMaxGains, 0.0f);
  std::copy(h->gains.begin(), h->gains.end(), g.begin());
  {
    GACQ_DEVICE(ctx);
    hipError_t e = h->dev.alloc(ctx, words * 8 + kRqMaxGains * sizeof(float));
    if (e == hipSuccess) e = h->dev.upload(0, h->thresholds.data(), kRqMaxGains * 8);
    if (e == hipSuccess) e = h->dev.upload(words * 8, g.data(), kRqMaxGains * sizeof(float));
    if (e != hipSuccess) return set_error(ctx, GACQ_ERR_HIP, "gacq_requant_open: %s", hipGetErrorString(e));
  }
  *out = h.release();
  return GACQ_OK;
}

extern "C" void gacq_requant_close(gacq_requant* h) { delete h; }

extern "C" int gacq_requant_run_dev(gacq_requant* h, const void* d_in, long long in_first, long long in_count, long long out_first, long long n_out,
                                    void* d_out, void* d_stats, void* d_gain_index) {
  if (!h) return GACQ_ERR_BAD_ARG;
  gacq_ctx* ctx = h->ctx;
  if (!d_in || !d_out) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_requant_run_dev: NULL argument");
  // everything is checked before anything is launched
  const gacq_requant_cfg& c = h->cfg;
  int rc = gacq_requant_check(&c, h->gains.data(), h->thresholds.data(), in_first, in_count, out_first, n_out);
  if (rc < 0) return st_forward(ctx, rc);
  const bool in16 = c.in_bits == 16;
  if (in16 && (uintptr_t)d_in % 2u) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_requant_run_dev: int16 input must be 2-byte aligned");
  if (c.container == GACQ_INGEST_S16 && (uintptr_t)d_out % 2u) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_requant_run_dev: int16 output must be 2-byte aligned");
  if (c.container == GACQ_INGEST_F32 && (uintptr_t)d_out % 8u) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_requant_run_dev: complex64 output must be 8-byte aligned");
  if ((uintptr_t)d_stats % 8u) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_requant_run_dev: d_stats must be 8-byte aligned");
  if (n_out == 0) return GACQ_OK;
  const int form = form_of(c), run = run_of(form), esz = in16 ? 2 : 1;
  const long long Lb = c.block, W = c.window, out_end = out_first + n_out;
  const size_t words = kRqMaxGains + (size_t)(kRqChunkBlocks + kRqMaxWindow);
  const unsigned long long* dT = (const unsigned long long*)h->dev.p;
  unsigned long long* dP = (unsigned long long*)h->dev.p + kRqMaxGains;
  const float* dG = (const float*)((const uint64_t*)h->dev.p + words);
  unsigned long long enc = 0;
  if (c.container == GACQ_INGEST_PACKED)
    for (int q = 0; q < (1 << c.bits); q++) enc |= (unsigned long long)c.enc[q] << (4 * q);
  GACQ_DEVICE(ctx);
  for (long long o = out_first; o < out_end;) {
    const long long b0 = o / Lb, o_end = std::min(out_end, (b0 + std::min(kRqChunkBlocks, kRqChunkComps / (2 * Lb))) * Lb), b_hi = (o_end - 1) / Lb;
    // ---- the block powers the levels of blocks b0 .. b_hi need
    RqPowerArgs p;
    p.in = (const uint8_t*)d_in;
    p.P = dP;
    p.pb0 = std::max(b0 - W, 0ll);
    p.nblk = std::max(b_hi, W) - p.pb0;
    p.in_first = in_first;
    p.Lb = (int)Lb;
    p.words = (int)(Lb * 2 * esz / 16);
    // a group's sum goes over wave shuffles, so a group lies inside one wave -- up to 64 lanes, each taking up to 4 words of a block
    // of fewer than 256 words -- or is the whole workgroup, whose four waves meet in LDS
    p.gs_log2 = 1;
    while ((1 << p.gs_log2) < p.words && p.gs_log2 < 6) p.gs_log2++;
    if (p.words >= kRqBlock) p.gs_log2 = 8;
    p.gs = 1 << p.gs_log2;
    const long long per = kRqBlock >> p.gs_log2, npass = (p.nblk + per - 1) / per;
    const unsigned pgrid = (unsigned)std::min<long long>(npass, (long long)kRqMaxGrid);
    if (in16) hipLaunchKernelGGL((requant_power_kernel<true>), dim3(pgrid), dim3(kRqBlock), 0, ctx->stream, p);
    else hipLaunchKernelGGL((requant_power_kernel<false>), dim3(pgrid), dim3(kRqBlock), 0, ctx->stream, p);
    if ((rc = st_launched(ctx, "gacq_requant_run_dev")) < 0) return rc;
    // ---- the outputs o .. o_end - 1
    RqQuantArgs a;
    a.ncomp = (int)(2 * (o_end - o));
    a.nbytes = (int)((long long)a.ncomp * 16 / run);
    a.in = (const uint8_t*)d_in + (o - in_first) * 2 * esz;
    a.out = (uint8_t*)d_out + 2 * (o - out_first) * 16 / run;
    a.P = dP;
    a.G = dG;
    a.T = dT;
    a.stats = (unsigned long long*)d_stats;
    a.gidx = d_gain_index ? (uint8_t*)d_gain_index + (b0 - (out_first + Lb - 1) / Lb) : nullptr;       // block b0 itself is written only when it is owned
    a.r_first = (int)(2 * (o - b0 * Lb));
    a.p_off = (int)(b0 - p.pb0);
    a.warm = (int)std::max(W - b0, 0ll);
    a.a0 = (int)((uintptr_t)a.out % 16u);
    a.hc = a.a0 * run / 16;                                            // exact: int16 output lies on 2 bytes, complex64 on 8
    a.nlanes = (a.a0 + a.nbytes + 15) / 16;
    a.enc = enc;
    a.twoLb = (unsigned)(2 * Lb);
    a.W = (int)W;
    a.msb = c.msb_first != 0;
    const int tile_runs = kRqBlock * 128 / run, ntiles = (a.nlanes + tile_runs - 1) / tile_runs;      // RqForm::runs runs a lane
    const unsigned grid = std::min((unsigned)ntiles, kRqMaxGrid);
    if (in16) launch_quantize<true>(form, grid, ctx->stream, a);
    else launch_quantize<false>(form, grid, ctx->stream, a);
    if ((rc = st_launched(ctx, "gacq_requant_run_dev")) < 0) return rc;
    o = o_end;
  }
  return GACQ_OK;
}
