// Interference mitigation (gacq_mitigate_dev, include/gacq.h): a time-domain pulse blanker and a frequency-domain excision filter on
// the canonical recording, interleaved int8 I/Q or complex64 in, int8 I/Q or complex64 out.  Every decision is a function of the absolute
// sample index, so the output does not depend on how a caller cuts the recording into calls.
//
// mit_excise_kernel<LOG2N>: N = 2^LOG2N, H = N / 2, T = clamp(N / 8, 64, 512) threads.  A workgroup owns kMitTile consecutive output
//   blocks q0 .. q0 + R - 1 and walks the frames q0 .. q0 + R in order; output block q is the second half of frame q plus the first half
//   of frame q + 1, so one frame in R + 1 is computed twice (by this tile and by the next).  Per frame:
//     load     the H new inputs of block f (the other half is the block the frame before loaded and stays in registers).  With blanking
//              on, the hit bits of inputs f H - 64 .. (f + 1) H + 63 go into an LDS bitset first, one wave ballot per 64 samples, and the
//              owner of a sample tests the 2 hold + 1 bits around it: the blanked recording never exists in memory.
//     forward  x = w z into LDS, radix-4 decimation in frequency in place (one radix-2 pass last when log2 N is odd): position i then holds
//              bin mit_bin_of(i), the digit-reversed order.
//     median   |X|^2 as fp32 bit patterns (they order as uint32, P >= 0) in LDS; radix selection of the (N/2)-th smallest, most
//              significant byte first: four rounds of a 256-bin LDS histogram (integer atomics) and a prefix sum over it in one wave.
//     excise   bins above ratio * median set their bit in a natural-index bitset (LDS atomic or); a position is zeroed when any bit
//              within +-guard of its bin (circular) is set.  Counts are integers.
//     inverse  the exact reversal of the forward passes (decimation in time from the digit-reversed order, conjugate twiddles), so the
//              data is back in natural order without a reordering pass; y = w x / N.
//     output   block f - 1 = kept half of frame f - 1 (registers) + first half of frame f, times gain, stored once.
//   Every frame runs the same instruction sequence wherever it falls in a tile, so the outputs of a call are bit for bit those of any
//   other partition.  Twiddles and window are fp64-evaluated host tables.
// mit_blank_kernel<IN_C64, OUT_C64> (excision off): a workgroup owns 2048 outputs, a lane 8 consecutive ones; the hit bits of the tile
//   and its 64-sample halos go to LDS as one byte per 8 samples, then every lane tests the bits around its outputs.  16-byte loads and
//   stores where the lane's bytes are aligned and present, element-wise otherwise.
#pragma clang fp contract(off)

#include "gacq_common.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

using namespace gacq;

namespace {

constexpr int kMitTile = 8;                      // output blocks per workgroup of the excision kernel
constexpr int kHalo = 64;                        // the largest hold
constexpr int kMaxGuard = 8;
constexpr int kBlkThreads = 256;
constexpr int kRun = 8;                          // blank-only kernel: outputs per lane
constexpr int kBlkTile = kBlkThreads * kRun;
constexpr int kBlkGroups = (kBlkTile + 2 * kHalo) / 8;      // hit bytes of a tile and its halos
constexpr unsigned kMitMaxGrid = 1u << 16;       // workgroups; a longer call loops

constexpr int mit_threads(int log2n) { return (1 << log2n) / 8 < 64 ? 64 : ((1 << log2n) / 8 > 512 ? 512 : (1 << log2n) / 8); }

struct MitArgs {
  const void* in;
  void* out;
  const float* win;             // w[n], n < N
  const float2* tw;             // exp(-2 pi i k / N), k < 3N/4
  unsigned long long* stats;    // blanked, frames, bins; or NULL
  unsigned* frame_bins;         // or NULL
  long long in_first, in_count, out_first, n_out;
  long long q_first, nblocks;   // the output blocks q_first .. q_first + nblocks - 1
  long long f_own;              // the first frame the call owns: ceil(out_first / H)
  float gain, ratio, thr2_f, inv_n;
  int thr2_i;
  int hold, guard, blank, in_c64, out_c64, out_aligned;
};

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cmul(float2 a, float2 w) {
  return make_float2(__builtin_fmaf(a.x, w.x, -(a.y * w.y)), __builtin_fmaf(a.x, w.y, a.y * w.x));
}
__device__ __forceinline__ float2 cmulc(float2 a, float2 w) {       // a conj(w)
  return make_float2(__builtin_fmaf(a.x, w.x, a.y * w.y), __builtin_fmaf(a.y, w.x, -(a.x * w.y)));
}

__device__ __forceinline__ bool mit_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// p(j) > blank_thr^2 of a sanitised sample: int32 for int8 input, fp32 without contraction for complex64
__device__ __forceinline__ bool mit_hit(const MitArgs& a, float2 v) {
  if (a.in_c64) return v.x * v.x + v.y * v.y > a.thr2_f;
  const int x = (int)v.x, y = (int)v.y;
  return x * x + y * y > a.thr2_i;
}

// A tile's view of the call: sample indices relative to the tile's first output sample q0 H fit an int, so the frame loop compares and
// addresses with 32-bit values and three pointers
struct MitTile {
  const void* in;               // input sample q0 H (an address only; samples in_lo .. in_hi - 1 are present)
  void* out;                    // output sample q0 H (outputs out_lo .. out_hi - 1 belong to the call)
  unsigned* fb;                 // the zeroed-bin count of frame q0 (where the call owns it)
  int in_lo, in_hi, out_lo, out_hi;
};

__device__ __forceinline__ int mit_rel(long long v) {      // v as an int; far values stay far on their side
  return (int)(v < -(1ll << 30) ? -(1ll << 30) : (v > (1ll << 30) ? (1ll << 30) : v));
}

// input sample r of the tile, sanitised; 0 where d_in holds nothing (below sample 0 too: in_first >= 0)
__device__ __forceinline__ float2 mit_sample(const MitArgs& a, const MitTile& t, int r, bool& bad) {
  float2 v = make_float2(0.0f, 0.0f);
  if (r >= t.in_lo && r < t.in_hi) {
    if (a.in_c64) {
      v = reinterpret_cast<const float2*>(t.in)[r];
      if (mit_nonfinite(v.x) || mit_nonfinite(v.y)) {
        v = make_float2(0.0f, 0.0f);
        bad = true;
      }
    } else {
      const int8_t* p = reinterpret_cast<const int8_t*>(t.in) + 2 * r;
      v = make_float2((float)p[0], (float)p[1]);
    }
  }
  return v;
}

// any hit among samples lo .. hi of a bitset whose bit s is bit (s & 63) of word s >> 6; 0 <= lo <= hi
__device__ __forceinline__ bool mit_any_hit(const unsigned long long* hitw, int lo, int hi) {
  bool any = false;
  for (int w = lo >> 6; w <= (hi >> 6); w++) {
    const int l = lo - 64 * w > 0 ? lo - 64 * w : 0, h = hi - 64 * w < 63 ? hi - 64 * w : 63;
    const unsigned long long mask = (~0ull >> (63 - (h - l))) << l;
    any = any || (hitw[w] & mask) != 0ull;
  }
  return any;
}

__host__ __device__ __forceinline__ unsigned mit_to_i8(float x) {
  const float r = fminf(fmaxf(rintf(x), -127.0f), 127.0f);            // rintf: half to even
  return (x != x) ? 0u : ((unsigned)(int)r & 0xffu);
}

// the bin that position i holds after the forward passes: the base-4 digits of i in reverse order, an odd length's last bit on top
__device__ __forceinline__ unsigned mit_bin_of(unsigned i, int log2n) {
  const unsigned rv = __brev(i) >> (32 - log2n);
  const unsigned pairs = (1u << (log2n & ~1)) - 1u;
  const unsigned lo = rv & pairs;
  return ((lo & 0x55555555u) << 1) | ((lo & 0xaaaaaaaau) >> 1) | (rv & ~pairs);
}

// One decimation-in-frequency radix-4 pass of span S on x[j + {0, q, 2q, 3q}], q = S/4, in place: quarter r of every block receives the
// residue-r outputs times W_S^(r k)
template <int N, int T, int S>
__device__ __forceinline__ void mit_dif4(float2* x, const float2* __restrict__ tw, int tid) {
  constexpr int q = S / 4, stride = N / S;
  asm volatile("" : "+v"(tid));                   // the pass's addresses are formed here, not kept in registers across the frame loop
#pragma unroll 1
  for (int bf = tid; bf < N / 4; bf += T) {
    const int k = bf & (q - 1);
    const int j = ((bf - k) << 2) + k;
    const float2 e0 = x[j], e1 = x[j + q], e2 = x[j + 2 * q], e3 = x[j + 3 * q];
    const float2 w1 = tw[k * stride], w2 = tw[2 * k * stride], w3 = tw[3 * k * stride];
    const float2 t0 = cadd(e0, e2), t1 = csub(e0, e2), t2 = cadd(e1, e3);
    const float2 d = csub(e1, e3);
    const float2 t3 = make_float2(d.y, -d.x);                     // -i (e1 - e3)
    x[j] = cadd(t0, t2);
    x[j + q] = cmul(cadd(t1, t3), w1);
    x[j + 2 * q] = cmul(csub(t0, t2), w2);
    x[j + 3 * q] = cmul(csub(t1, t3), w3);
  }
}

// the reversal of mit_dif4 (times 4): conjugate twiddles first, then the inverse 4-point transform
template <int N, int T, int S>
__device__ __forceinline__ void mit_dit4(float2* x, const float2* __restrict__ tw, int tid) {
  constexpr int q = S / 4, stride = N / S;
  asm volatile("" : "+v"(tid));                   // the pass's addresses are formed here, not kept in registers across the frame loop
#pragma unroll 1
  for (int bf = tid; bf < N / 4; bf += T) {
    const int k = bf & (q - 1);
    const int j = ((bf - k) << 2) + k;
    const float2 w1 = tw[k * stride], w2 = tw[2 * k * stride], w3 = tw[3 * k * stride];
    const float2 u0 = x[j], u1 = cmulc(x[j + q], w1), u2 = cmulc(x[j + 2 * q], w2), u3 = cmulc(x[j + 3 * q], w3);
    const float2 t0 = cadd(u0, u2), t1 = csub(u0, u2), t2 = cadd(u1, u3);
    const float2 d = csub(u1, u3);
    const float2 t3 = make_float2(-d.y, d.x);                     // i (u1 - u3)
    x[j] = cadd(t0, t2);
    x[j + q] = cadd(t1, t3);
    x[j + 2 * q] = csub(t0, t2);
    x[j + 3 * q] = csub(t1, t3);
  }
}

template <int N, int T>
__device__ __forceinline__ void mit_pass2(float2* x, int tid) {
#pragma unroll 2
  for (int j = tid; j < N / 2; j += T) {
    const float2 a = x[2 * j], b = x[2 * j + 1];
    x[2 * j] = cadd(a, b);
    x[2 * j + 1] = csub(a, b);
  }
}

template <int N, int T, int S>
__device__ __forceinline__ void mit_forward(float2* x, const float2* __restrict__ tw, int tid) {
  if constexpr (S >= 4) {
    mit_dif4<N, T, S>(x, tw, tid);
    __syncthreads();
    mit_forward<N, T, S / 4>(x, tw, tid);
  } else if constexpr (S == 2) {
    mit_pass2<N, T>(x, tid);
    __syncthreads();
  }
}

template <int N, int T, int S>
__device__ __forceinline__ void mit_inverse(float2* x, const float2* __restrict__ tw, int tid) {
  if constexpr (S == 2) {
    mit_pass2<N, T>(x, tid);
    __syncthreads();
    mit_inverse<N, T, 8>(x, tw, tid);
  } else if constexpr (S <= N) {
    mit_dit4<N, T, S>(x, tw, tid);
    __syncthreads();
    mit_inverse<N, T, S * 4>(x, tw, tid);
  }
}

// The (N/2)-th smallest of pw[0 .. N) (1-based), as a bit pattern.  Four rounds, most significant byte first: a histogram of the byte
// among the values that share the bytes found so far, then the bin that holds the wanted rank.  Integer counts only.
template <int N, int T>
__device__ __forceinline__ unsigned mit_median(const unsigned* pw, unsigned* hist, unsigned* sel, int tid) {
  unsigned prefix = 0u, mask = 0u, rank = N / 2 - 1;
#pragma unroll 1
  for (int shift = 24; shift >= 0; shift -= 8) {
    asm volatile("" : "+v"(tid));                   // lane masks (tid < 64, tid >= d) are formed per round, not held in SGPR pairs across it
    for (int i = tid; i < 256; i += T) hist[i] = 0u;
    __syncthreads();
#pragma unroll 1
    for (int i = tid; i < N; i += T) {
      const unsigned v = pw[i];
      if ((v & mask) == prefix) atomicAdd(&hist[(v >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 64) {
      const unsigned c0 = hist[4 * tid], c1 = hist[4 * tid + 1], c2 = hist[4 * tid + 2], c3 = hist[4 * tid + 3];
      const unsigned s = c0 + c1 + c2 + c3;
      unsigned incl = s;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = (unsigned)__shfl_up((int)incl, d, 64);
        if (tid >= d) incl += t;
      }
      const unsigned excl = incl - s;
      if (excl <= rank && rank < incl) {
        unsigned rr = rank - excl, dg = 4u * tid;
        if (rr >= c0) {
          rr -= c0;
          dg++;
          if (rr >= c1) {
            rr -= c1;
            dg++;
            if (rr >= c2) {
              rr -= c2;
              dg++;
            }
          }
        }
        sel[0] = dg;
        sel[1] = rr;
      }
    }
    __syncthreads();
    prefix |= sel[0] << shift;
    mask |= 255u << shift;
    rank = sel[1];
  }
  return prefix;
}

// z of block q0 + b of the tile (b = -1 .. R) into the lane's registers: element i is sample b H + tid + i T of the tile.  `count`: the
// block is one of the tile's own, its forced zeros inside the call's output range are counted.
template <int N, int T, int E>
__device__ __forceinline__ void mit_load_block(const MitArgs& a, const MitTile& t, int b, bool count, unsigned long long* hitw, float2 (&z)[E],
                                               unsigned& nblank, int tid) {
  constexpr int H = N / 2, SPAN = H + 2 * kHalo;
  asm volatile("" : "+v"(tid));                     // the block's lane masks and addresses are formed here, not held across the frame loop
  int hold = __builtin_amdgcn_readfirstlane(a.hold);
  asm volatile("" : "+s"(hold));                    // ... and so are the bounds that derive from the hold
  const bool blank = __builtin_amdgcn_readfirstlane(a.blank) != 0;
  if (blank) {
    __syncthreads();                                   // nobody reads the bits of the block before any more
    const int base = b * H - kHalo;
    for (int s0 = 0; s0 < SPAN; s0 += T) {
      const int s = s0 + tid;
      bool hit = false;
      if (s >= kHalo - hold && s < H + kHalo + hold) {
        bool bad = false;
        hit = mit_hit(a, mit_sample(a, t, base + s, bad));
      }
      const unsigned long long m = __ballot(hit);
      if ((tid & 63) == 0) hitw[s >> 6] = m;
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < E; i++) {
    const int n = tid + i * T;
    z[i] = make_float2(0.0f, 0.0f);
    if (n < H) {
      const int r = b * H + n;
      bool forced = false;
      float2 v = mit_sample(a, t, r, forced);
      if (blank) forced = forced || mit_any_hit(hitw, n + kHalo - hold, n + kHalo + hold);
      if (forced) {
        v = make_float2(0.0f, 0.0f);
        if (count && r >= t.out_lo && r < t.out_hi) nblank++;
      }
      z[i] = v;
    }
  }
}

__device__ __forceinline__ void mit_store(const MitArgs& a, const MitTile& t, int r, float2 y) {      // output sample r of the tile
  const float re = y.x * a.gain, im = y.y * a.gain;
  if (a.out_c64) {
    reinterpret_cast<float2*>(t.out)[r] = make_float2(re, im);
  } else {
    uint8_t* o = reinterpret_cast<uint8_t*>(t.out) + 2 * r;
    o[0] = (uint8_t)mit_to_i8(re);
    o[1] = (uint8_t)mit_to_i8(im);
  }
}

template <int LOG2N>
__global__ __launch_bounds__(mit_threads(LOG2N), 4) void mit_excise_kernel(const MitArgs a) {
  constexpr int N = 1 << LOG2N, H = N / 2, T = mit_threads(LOG2N), E = H / T > 1 ? H / T : 1;
  constexpr int kHitWords = ((H + 2 * kHalo + T - 1) / T) * T / 64;
  __shared__ __attribute__((aligned(16))) float2 x[N];
  __shared__ unsigned pw[N];
  __shared__ unsigned bits[N / 32];
  __shared__ unsigned hist[256];
  __shared__ unsigned long long hitw[kHitWords];
  __shared__ unsigned sel[2];
  __shared__ unsigned ctr[2];                          // zeroed bins of the frame, forced zeros of the tile
  // The call's arguments are read from an LDS copy inside the frame loop: values the loop derives from them are then formed where they
  // are used instead of being held in scalar registers across the whole loop (the kernel argument block would otherwise overflow them)
  __shared__ MitArgs lds_args;
  if (threadIdx.x == 0) lds_args = a;
  __syncthreads();
  const MitArgs& s = lds_args;
  const int tid = threadIdx.x;
  const long long ntiles = (a.nblocks + kMitTile - 1) / kMitTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long q0 = a.q_first + tile * kMitTile;
    const int nb = (int)(a.nblocks - tile * kMitTile < kMitTile ? a.nblocks - tile * kMitTile : kMitTile);
    MitTile t;
    t.in = a.in_c64 ? (const void*)(reinterpret_cast<const float2*>(a.in) + (q0 * H - a.in_first))
                    : (const void*)(reinterpret_cast<const int8_t*>(a.in) + 2 * (q0 * H - a.in_first));
    t.out = a.out_c64 ? (void*)(reinterpret_cast<float2*>(a.out) + (q0 * H - a.out_first)) : (void*)(reinterpret_cast<int8_t*>(a.out) + 2 * (q0 * H - a.out_first));
    t.fb = a.frame_bins ? a.frame_bins + (q0 - a.f_own) : nullptr;
    t.in_lo = mit_rel(a.in_first - q0 * H);
    t.in_hi = mit_rel(a.in_first + a.in_count - q0 * H);
    t.out_lo = mit_rel(a.out_first - q0 * H);
    t.out_hi = mit_rel(a.out_first + a.n_out - q0 * H);
    unsigned nblank = 0u;
    unsigned tile_frames = 0u, tile_bins = 0u;         // thread 0
    float2 zprev[E], znew[E], yprev[E];
    if (tid == 0) ctr[1] = 0u;
    mit_load_block<N, T, E>(s, t, -1, false, hitw, zprev, nblank, tid);
#pragma unroll
    for (int i = 0; i < E; i++) yprev[i] = make_float2(0.0f, 0.0f);
#pragma unroll 1
    for (int fi = 0; fi <= nb; fi++) {
      int tid = threadIdx.x;
      asm volatile("" : "+v"(tid));                   // what a frame derives from the lane index is formed inside the frame
      mit_load_block<N, T, E>(s, t, fi, fi < nb, hitw, znew, nblank, tid);
#pragma unroll
      for (int i = 0; i < E; i++) {
        const int n = tid + i * T;
        if (n < H) {
          const float w0 = s.win[n], w1 = s.win[n + H];
          x[n] = make_float2(zprev[i].x * w0, zprev[i].y * w0);
          x[n + H] = make_float2(znew[i].x * w1, znew[i].y * w1);
          zprev[i] = znew[i];
        }
      }
      for (int w = tid; w < N / 32; w += T) bits[w] = 0u;
      if (tid == 0) ctr[0] = 0u;
      __syncthreads();
      mit_forward<N, T, N>(x, s.tw, tid);
#pragma unroll 1
      for (int i = tid; i < N; i += T) {
        const float2 v = x[i];
        pw[i] = __float_as_uint(v.x * v.x + v.y * v.y);
      }
      const float thr = s.ratio * __uint_as_float(mit_median<N, T>(pw, hist, sel, tid));      // its first barrier publishes pw
#pragma unroll 1
      for (int i = tid; i < N; i += T) {
        if (__uint_as_float(pw[i]) > thr) {
          const unsigned k = mit_bin_of((unsigned)i, LOG2N);
          atomicOr(&bits[k >> 5], 1u << (k & 31u));
        }
      }
      __syncthreads();
      unsigned nz = 0u;
#pragma unroll 1
      for (int i = tid; i < N; i += T) {
        // bits k - guard .. k + guard, circular: those from k up in `up`, those below k in `dn`
        const unsigned k = mit_bin_of((unsigned)i, LOG2N);
        const unsigned wi = k >> 5, b = k & 31u;
        const unsigned w0 = bits[(wi - 1u) & (N / 32 - 1)], w1 = bits[wi], w2 = bits[(wi + 1u) & (N / 32 - 1)];
        const unsigned long long up = (((unsigned long long)w2 << 32) | w1) >> b;
        const unsigned long long dn = (((unsigned long long)w1 << 32) | w0) >> (32u + b - (unsigned)s.guard);
        if ((up & ((2ull << s.guard) - 1ull)) | (dn & ((1ull << s.guard) - 1ull))) {
          x[i] = make_float2(0.0f, 0.0f);
          nz++;
        }
      }
      if (nz) atomicAdd(&ctr[0], nz);
      __syncthreads();
      if (tid == 0 && fi < nb && fi * H >= t.out_lo && fi * H < t.out_hi) {      // the call owns frame q0 + fi
        const unsigned n = ctr[0];
        tile_frames++;
        tile_bins += n;
        if (t.fb) t.fb[fi] = n;
      }
      mit_inverse<N, T, (LOG2N & 1) ? 2 : 4>(x, s.tw, tid);
#pragma unroll
      for (int i = 0; i < E; i++) {
        const int n = tid + i * T;
        if (n < H) {
          const float2 v0 = x[n], v1 = x[n + H];
          const float w0 = s.win[n], w1 = s.win[n + H];
          const float2 y0 = make_float2((v0.x * s.inv_n) * w0, (v0.y * s.inv_n) * w0);
          const int r = (fi - 1) * H + n;
          if (fi > 0 && r >= t.out_lo && r < t.out_hi) mit_store(s, t, r, cadd(yprev[i], y0));
          yprev[i] = make_float2((v1.x * s.inv_n) * w1, (v1.y * s.inv_n) * w1);
        }
      }
      __syncthreads();
    }
    if (a.stats) {
      if (nblank) atomicAdd(&ctr[1], nblank);
      __syncthreads();
      if (tid == 0) {
        if (ctr[1]) atomicAdd(a.stats, (unsigned long long)ctr[1]);
        if (tile_frames) atomicAdd(a.stats + 1, (unsigned long long)tile_frames);
        if (tile_bins) atomicAdd(a.stats + 2, (unsigned long long)tile_bins);
      }
      __syncthreads();
    }
  }
}

// samples j0 .. j0 + 7 (absolute), sanitised; bit i of `bad` when sample i was not finite
template <bool IN_C64>
__device__ __forceinline__ void mit_load8(const MitArgs& a, long long j0, float2 (&v)[kRun], unsigned& bad) {
  const long long i0 = j0 - a.in_first;
  const bool inside = j0 >= 0 && i0 >= 0 && i0 + kRun <= a.in_count;
  bad = 0u;
  if constexpr (IN_C64) {
    const float2* p = reinterpret_cast<const float2*>(a.in) + i0;
    if (inside && ((uintptr_t)p % 16u) == 0u) {
#pragma unroll
      for (int i = 0; i < kRun; i += 2) {
        const float4 w = reinterpret_cast<const float4*>(p)[i / 2];
        v[i] = make_float2(w.x, w.y);
        v[i + 1] = make_float2(w.z, w.w);
      }
    } else {
#pragma unroll
      for (int i = 0; i < kRun; i++) v[i] = (inside || (j0 + i >= 0 && i0 + i >= 0 && i0 + i < a.in_count)) ? p[i] : make_float2(0.0f, 0.0f);
    }
#pragma unroll
    for (int i = 0; i < kRun; i++)
      if (mit_nonfinite(v[i].x) || mit_nonfinite(v[i].y)) {
        v[i] = make_float2(0.0f, 0.0f);
        bad |= 1u << i;
      }
  } else {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(a.in) + 2 * i0;
    unsigned r[4] = {0u, 0u, 0u, 0u};
    if (inside && ((uintptr_t)p % 16u) == 0u) {
      const uint4 w = *reinterpret_cast<const uint4*>(p);
      r[0] = w.x;
      r[1] = w.y;
      r[2] = w.z;
      r[3] = w.w;
    } else {
#pragma unroll
      for (int i = 0; i < kRun; i++)
        if (inside || (j0 + i >= 0 && i0 + i >= 0 && i0 + i < a.in_count))
          r[i >> 1] |= ((unsigned)p[2 * i] | ((unsigned)p[2 * i + 1] << 8)) << (16 * (i & 1));
    }
#pragma unroll
    for (int i = 0; i < kRun; i++) {
      const unsigned h = r[i >> 1] >> (16 * (i & 1));
      v[i] = make_float2((float)(signed char)(h & 0xffu), (float)(signed char)((h >> 8) & 0xffu));
    }
  }
}

template <bool IN_C64, bool OUT_C64>
__global__ __launch_bounds__(kBlkThreads) void mit_blank_kernel(const MitArgs a) {
  __shared__ unsigned long long hitw[(kBlkGroups + 7) / 8];
  __shared__ unsigned ctr;
  const int tid = threadIdx.x;
  const long long ntiles = (a.n_out + kBlkTile - 1) / kBlkTile;
  unsigned nblank = 0u;
  if (tid == 0) ctr = 0u;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long m0 = tile * kBlkTile;              // offset of the tile's first output from out_first
    if (a.blank) {
      uint8_t* hb = reinterpret_cast<uint8_t*>(hitw);  // bit s of the set is bit (s & 7) of byte s >> 3: sample out_first + m0 - 64 + s
      for (int g = tid; g < kBlkGroups; g += kBlkThreads) {
        float2 v[kRun];
        unsigned bad;
        mit_load8<IN_C64>(a, a.out_first + m0 - kHalo + 8 * g, v, bad);
        unsigned byte = 0u;
#pragma unroll
        for (int i = 0; i < kRun; i++) byte |= (mit_hit(a, v[i]) ? 1u : 0u) << i;
        hb[g] = (uint8_t)byte;
      }
    }
    __syncthreads();
    const long long m = m0 + (long long)tid * kRun;
    if (m < a.n_out) {
      const long long left = a.n_out - m;
      float2 v[kRun];
      unsigned bad;
      mit_load8<IN_C64>(a, a.out_first + m, v, bad);
      float vr[kRun], vi[kRun];
#pragma unroll
      for (int i = 0; i < kRun; i++) {
        const int s = tid * kRun + kHalo + i;
        bool forced = (bad >> i) & 1u;
        if (a.blank) forced = forced || mit_any_hit(hitw, s - a.hold, s + a.hold);
        if (forced) {
          v[i] = make_float2(0.0f, 0.0f);
          if (i < left) nblank++;
        }
        vr[i] = v[i].x * a.gain;
        vi[i] = v[i].y * a.gain;
      }
      if (OUT_C64) {
        float2* __restrict__ o = reinterpret_cast<float2*>(a.out) + m;
        if (left >= kRun && a.out_aligned) {
#pragma unroll
          for (int i = 0; i < kRun; i += 2) reinterpret_cast<float4*>(o)[i / 2] = make_float4(vr[i], vi[i], vr[i + 1], vi[i + 1]);
        } else {
#pragma unroll
          for (int i = 0; i < kRun; i++)
            if (i < left) o[i] = make_float2(vr[i], vi[i]);
        }
      } else {
        unsigned b[2 * kRun];
#pragma unroll
        for (int i = 0; i < kRun; i++) {
          b[2 * i] = mit_to_i8(vr[i]);
          b[2 * i + 1] = mit_to_i8(vi[i]);
        }
        uint8_t* __restrict__ o = reinterpret_cast<uint8_t*>(a.out) + 2 * m;
        if (left >= kRun && a.out_aligned) {
          uint4 w;
          w.x = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
          w.y = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
          w.z = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
          w.w = b[12] | (b[13] << 8) | (b[14] << 16) | (b[15] << 24);
          *reinterpret_cast<uint4*>(o) = w;
        } else {
#pragma unroll
          for (int i = 0; i < kRun; i++)
            if (i < left) {
              o[2 * i] = (uint8_t)b[2 * i];
              o[2 * i + 1] = (uint8_t)b[2 * i + 1];
            }
        }
      }
    }
    __syncthreads();
  }
  if (a.stats) {
    if (nblank) atomicAdd(&ctr, nblank);
    __syncthreads();
    if (tid == 0 && ctr) atomicAdd(a.stats, (unsigned long long)ctr);
  }
}

template <int LOG2N>
void launch_excise(unsigned grid, hipStream_t stream, const MitArgs& a) {
  hipLaunchKernelGGL(mit_excise_kernel<LOG2N>, dim3(grid), dim3(mit_threads(LOG2N)), 0, stream, a);
}

int ilog2(int n) {
  int l = 0;
  while ((1 << l) < n) l++;
  return l;
}

}  // namespace

#include "gacq_streamhost.h"

extern "C" int gacq_mitigate_tile(int nfft) {
  if (nfft < 64 || nfft > 4096 || (nfft & (nfft - 1))) return GACQ_ERR_BAD_ARG;
  return kMitTile;
}

extern "C" int gacq_mitigate_check(const gacq_mitigate_cfg* cfg, const void* d_in, int in_complex64, long long in_first, long long in_count,
                                   long long out_first, long long n_out, double gain, int out_complex64, const void* d_out) {
  if (!cfg || !d_in || !d_out) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_mitigate_dev: NULL argument");
  if (!std::isfinite(cfg->blank_thr) || cfg->blank_thr < 0.0)
    return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_mitigate_dev: blank_thr must be finite and not negative (%g)", cfg->blank_thr);
  const bool blank = cfg->blank_thr > 0.0, excise = cfg->nfft != 0;
  if (!blank && !excise) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_mitigate_dev: blanking and excision are both off");
  if (cfg->hold < 0 || cfg->hold > kHalo) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_mitigate_dev: hold %d outside 0..%d", cfg->hold, kHalo);
  if (cfg->guard < 0 || cfg->guard > kMaxGuard)
    return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_mitigate_dev: guard %d outside 0..%d", cfg->guard, kMaxGuard);
  if (excise) {
    if (cfg->nfft < 64 || cfg->nfft > 4096 || (cfg->nfft & (cfg->nfft - 1)))
      return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_mitigate_dev: nfft %d is not a power of two in 64..4096", cfg->nfft);
    if (!std::isfinite(cfg->ratio) || !(cfg->ratio > 1.0))
      return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_mitigate_dev: the ratio must be finite and above 1 (%g)", cfg->ratio);
  }
  int rc = st_check_gain(nullptr, "gacq_mitigate_dev", "must be finite and positive in fp32", gain);
  if (rc == GACQ_OK) rc = st_check_range(nullptr, "gacq_mitigate_dev", in_first, in_count, out_first, n_out);
  if (rc < 0) return rc;
  if ((in_complex64 && (uintptr_t)d_in % 8u) || (out_complex64 && (uintptr_t)d_out % 8u))
    return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_mitigate_dev: a complex64 buffer must be 8-byte aligned");
  if (n_out == 0) return GACQ_OK;
  const long long last = out_first + n_out - 1;
  long long need_lo, need_hi;
  if (excise) {
    const long long H = cfg->nfft / 2;
    need_lo = (out_first / H - 1) * H - cfg->hold;
    need_hi = (last / H + 2) * H - 1 + cfg->hold;
  } else {
    need_lo = out_first - cfg->hold;
    need_hi = last + cfg->hold;
  }
  return st_check_support(nullptr, "gacq_mitigate_dev", out_first, n_out, std::max(0ll, need_lo), need_hi, in_first, in_count);
}

extern "C" int gacq_mitigate_dev(gacq_ctx* ctx, const gacq_mitigate_cfg* cfg, const void* d_in, int in_complex64, long long in_first,
                                 long long in_count, long long out_first, long long n_out, double gain, int out_complex64, void* d_out,
                                 void* d_stats, void* d_frame_bins) {
  // everything is checked before anything is launched
  const int rc = gacq_mitigate_check(cfg, d_in, in_complex64, in_first, in_count, out_first, n_out, gain, out_complex64, d_out);
  if (rc < 0) return ctx ? st_forward(ctx, rc) : rc;
  if (!ctx) return GACQ_ERR_BAD_ARG;
  if (((uintptr_t)d_stats % 8u) || ((uintptr_t)d_frame_bins % 4u))
    return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_mitigate_dev: d_stats must be 8-byte and d_frame_bins 4-byte aligned");
  if (n_out == 0) return GACQ_OK;
  const bool excise = cfg->nfft != 0;
  MitArgs a{};
  a.in = d_in;
  a.out = d_out;
  a.stats = (unsigned long long*)d_stats;
  a.frame_bins = (unsigned*)d_frame_bins;
  a.in_first = in_first;
  a.in_count = in_count;
  a.out_first = out_first;
  a.n_out = n_out;
  a.gain = (float)gain;
  a.blank = cfg->blank_thr > 0.0;
  a.hold = cfg->hold;
  a.guard = cfg->guard;
  a.in_c64 = in_complex64 != 0;
  a.out_c64 = out_complex64 != 0;
  a.out_aligned = ((uintptr_t)d_out % 16u) == 0u;
  // the threshold squared, once, in the arithmetic of the comparison: int32 for int8 input (|x|^2 <= 32768), fp32 for complex64
  const double t2 = cfg->blank_thr * cfg->blank_thr;
  a.thr2_i = t2 >= 32768.0 ? 32768 : (int)std::floor(t2);
  a.thr2_f = (float)cfg->blank_thr * (float)cfg->blank_thr;
  GACQ_DEVICE(ctx);
  if (!excise) {
    const long long nblk = (n_out + kBlkTile - 1) / kBlkTile;
    const unsigned grid = (unsigned)std::min<long long>(nblk, (long long)kMitMaxGrid);
    if (a.in_c64) {
      if (a.out_c64) hipLaunchKernelGGL((mit_blank_kernel<true, true>), dim3(grid), dim3(kBlkThreads), 0, ctx->stream, a);
      else hipLaunchKernelGGL((mit_blank_kernel<true, false>), dim3(grid), dim3(kBlkThreads), 0, ctx->stream, a);
    } else {
      if (a.out_c64) hipLaunchKernelGGL((mit_blank_kernel<false, true>), dim3(grid), dim3(kBlkThreads), 0, ctx->stream, a);
      else hipLaunchKernelGGL((mit_blank_kernel<false, false>), dim3(grid), dim3(kBlkThreads), 0, ctx->stream, a);
    }
  } else {
    const int N = cfg->nfft, H = N / 2;
    const std::string wkey = "mit:win" + std::to_string(N);
    const void* dw = nullptr;
    if (!ctx->tables.count(wkey)) {
      std::vector<float> w(N);
      for (int n = 0; n < N; n++) w[n] = (float)std::sin(M_PI * ((double)n + 0.5) / (double)N);
      const int rcw = table_cache(ctx, wkey, w.data(), sizeof(float) * (size_t)N, &dw);
      if (rcw != GACQ_OK) return rcw;
    } else {
      dw = ctx->tables[wkey].p;
    }
    const int rct = twiddle_cache(ctx, "mit:tw" + std::to_string(N), N, 3 * N / 4, &a.tw);
    if (rct != GACQ_OK) return rct;
    a.win = (const float*)dw;
    a.ratio = (float)cfg->ratio;
    a.inv_n = 1.0f / (float)N;
    a.q_first = out_first / H;
    a.nblocks = (out_first + n_out - 1) / H - a.q_first + 1;
    a.f_own = (out_first + H - 1) / H;
    const long long ntiles = (a.nblocks + kMitTile - 1) / kMitTile;
    const unsigned grid = (unsigned)std::min<long long>(ntiles, (long long)kMitMaxGrid);
    switch (ilog2(N)) {
      case 6: launch_excise<6>(grid, ctx->stream, a); break;
      case 7: launch_excise<7>(grid, ctx->stream, a); break;
      case 8: launch_excise<8>(grid, ctx->stream, a); break;
      case 9: launch_excise<9>(grid, ctx->stream, a); break;
      case 10: launch_excise<10>(grid, ctx->stream, a); break;
      case 11: launch_excise<11>(grid, ctx->stream, a); break;
      default: launch_excise<12>(grid, ctx->stream, a);
    }
  }
  return st_launched(ctx, "gacq_mitigate_dev");
}
