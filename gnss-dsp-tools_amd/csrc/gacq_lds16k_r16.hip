// N = 16384 in ONE 1024-thread workgroup (B1I/B2I padded, GLONASS L1/L2), 16 points per lane, as
//   16 wave-private 1024-point transforms + one radix-16 pass across the waves:
//     n = t + 1024 j  (t = 64 w + l: wave w, lane l; j = register),   k = ka + 16 kk,  kk = k0 + 16 k1 + 256 k2
//   forward (decimation in frequency, natural order in, digit-permuted order out):
//     pass 0  DFT16 over j -> ka, twiddle W_N^{t ka};  exchange 0: lane t sends output ka to wave ka (the only step
//             that crosses waves: one workgroup barrier)
//     then wave ka transforms its 1024 values u[m], m = l + 64 j', WITHOUT any barrier -- a wave runs in lockstep and the
//     LDS executes one wave's accesses in order, so the two transposes inside a wave need no synchronisation:
//     pass 1  DFT16 over j' -> k0, twiddle W_1024^{l k0};   transpose 1: lane (k0, l_lo) collects l = l_lo + 4 l_hi
//     pass 2  DFT16 over l_hi -> k1, twiddle W_64^{l_lo k1}; transpose 2: lane mu = k0 + 16 k1_lo collects (k1_hi, l_lo)
//     pass 3  four DFT4 over l_lo -> k2
//     out: register r = k1_hi + 4 k2 of lane (w, mu) holds X[w + 16 mu + 1024 r]
//   inverse (decimation in time) is the transposed network with conjugated twiddles: it takes exactly that order in and
//   leaves y[t + 1024 j] in register rev16(j) of lane t.  Spectra (X, C_p) therefore live in memory in the order the
//   forward transform produces them ("physical lane-pair layout": element (t, r) at (r >> 1) * 2048 + 2 t + (r & 1)), the
//   pointwise product needs no order at all, and no reordering pass exists anywhere.
// A correlation row costs two workgroup barriers (around the one cross-wave exchange) instead of the seven of the
// 4 x 4096 decomposition of rounds 1-2, and the 16 waves of the CU drift apart everywhere else.
// LDS: 16 regions of 1056 complex (1024 + the padding of the pitch-66 / pitch-65 transposes) = 132 KB + 256 B of reduction
// scratch -> one workgroup (16 waves, 4 per SIMD, <= 128 VGPRs) per CU.  Every LDS access below is (per-lane base) +
// (compile-time offset) and bank-conflict free (checked per 16-lane store group / 32-lane load group).
// This is the radix-16 form (option GACQ_OPT_LDS_VARIANT = 16; plan_search, gacq_engine.hip).  The default at this length is the radix-32
// form of gacq_lds16k.hip, whose header says what the two measured against each other; the r16_* entry points at the end of this file
// are the counterparts of its r32_* ones.
#include "gacq_common.h"
#include "gacq_cplx.h"
#include "gacq_ldsutil.h"

#include <algorithm>

using namespace gacq;

namespace {

constexpr int kBig = 16384;
constexpr int kBigThreads = 1024;
constexpr int kRegion = 1056;                               // complex elements per wave region
constexpr int kBigScratch = 16 * kRegion * (int)sizeof(v2); // byte offset of the cross-wave reduction scratch
constexpr int kBigLdsBytes = kBigScratch + 256;

// Phase timing of lds16k_correlate_kernel (diagnostic builds only, -DGACQ_PHASE_TIMING16; tools/phase_timing16.py): lane 0 of every
// wave accumulates the shader-clock cycles between marks into gacq_phase16[wave][phase] (read back with gacq_debug_phase16).
// Never defined in the product build.
#ifdef GACQ_PHASE_TIMING16
__device__ unsigned long long gacq_phase16[16 * 8];
#define GACQ_MARK16(i) do { const unsigned long long now_ = __builtin_readcyclecounter(); acc16_[i] += now_ - mark16_; mark16_ = now_; } while (0)
#else
#define GACQ_MARK16(i) do { } while (0)
#endif

// Progress-based wave priority.  The four waves that share a SIMD do the same work between two workgroup barriers: VALU
// segments separated by LDS round trips.  Left to the default oldest-first arbitration, the two oldest waves ping-pong
// through all their segments (an LDS round trip is longer than a segment, so the VALU idles in between) and then wait at the
// barrier while the two youngest do the same.  A wave that lowers its own priority at the end of every segment -- right
// after issuing the LDS accesses that end it -- hands the VALU to the waves that are behind: the four waves take turns
// segment by segment and every round trip is covered by the three other waves' arithmetic.
#define GACQ_SETPRIO_(n) asm volatile("s_setprio " #n ::: "memory")
#define GACQ_SETPRIO(n) GACQ_SETPRIO_(n)
// Levels of the four segments between two barrier pairs of the inverse transform (last radix-16 pass + magnitudes | C * x +
// radix-4 | radix-16 | radix-16): measured on B1I, 63 items x 200 bins x 10 blocks (profiles/r03_16k_priority_sweep.log):
// none 3.50 ms, 3-2-1-0 3.06-3.09, 0-1-2-3 3.21, 2-3-1-0 2.98-2.99.
// forward + inverse in one kernel (lds16k_fused_kernel): after barrier A | after the sample loads are issued | after the forward
// exchange | after transpose 1 | after transpose 2 (then GACQ_P3 / GACQ_P4 inside the inverse transform)
#ifndef GACQ_QA
#define GACQ_QA 3
#define GACQ_QX 3
#define GACQ_QF 3
#define GACQ_QT1 2
#define GACQ_QT2 2
#endif
#ifndef GACQ_P1
#define GACQ_P1 2
#define GACQ_P2 3
#define GACQ_P3 1
#define GACQ_P4 0
#endif

// v[k] *= w^k, k = 1..15, registers in natural order (the DIT passes twiddle their inputs); same product tree as apply_powers
__device__ __forceinline__ void apply_powers_nat(v2 (&v)[kR], v2 w1) {
  const v2 w2 = cmul(w1, w1), w3 = cmul(w2, w1), w4 = cmul(w2, w2);
  v[1] = cmul(v[1], w1);    v[2] = cmul(v[2], w2);    v[3] = cmul(v[3], w3);
  const v2 w5 = cmul(w4, w1), w6 = cmul(w3, w3), w7 = cmul(w4, w3), w8 = cmul(w4, w4);
  v[4] = cmul(v[4], w4);    v[5] = cmul(v[5], w5);    v[6] = cmul(v[6], w6);    v[7] = cmul(v[7], w7);
  const v2 w9 = cmul(w8, w1), w10 = cmul(w5, w5), w11 = cmul(w8, w3), w12 = cmul(w6, w6);
  v[8] = cmul(v[8], w8);    v[9] = cmul(v[9], w9);    v[10] = cmul(v[10], w10); v[11] = cmul(v[11], w11);
  v[12] = cmul(v[12], w12);
  const v2 w13 = cmul(w8, w5), w14 = cmul(w7, w7), w15 = cmul(w8, w7);
  v[13] = cmul(v[13], w13); v[14] = cmul(v[14], w14); v[15] = cmul(v[15], w15);
}

// Per-lane twiddle bases of the three twiddled passes: W_N^t, W_1024^l = W_N^{16 l}, W_64^{l >> 4} = W_N^{256 (l >> 4)};
// twn holds W_16384^m for m < 1024.  The powers are rebuilt per pass (14 complex products): tables of the two wave-private
// passes in LDS (8.5 KB, one ds_read_b64 per product) were measured -- B1I 3.04 -> 3.51 ms: the LDS pipe, already carrying
// three exchanges per row, is as loaded as the VALU (profiles/r03_16k_*).
struct Tw16k { v2 w0, w1, w2; };
__device__ __forceinline__ Tw16k tw16k_load(const float2* __restrict__ twn, bool conj) {
  const int t = threadIdx.x, l = t & 63;
  Tw16k k;
  k.w0 = ld2(twn + t);
  k.w1 = ld2(twn + 16 * l);
  k.w2 = ld2(twn + 256 * (l >> 4));
  if (conj) { k.w0.y = -k.w0.y; k.w1.y = -k.w1.y; k.w2.y = -k.w2.y; }
  return k;
}

// Forward transform.  In: v[j] = x[t + 1024 j].  Out: v[r] = X[(t >> 6) + 16 (t & 63) + 1024 r].
// The caller guarantees that no wave still uses its region when the exchange-0 stores start (they go to every region).
__device__ __forceinline__ void fft16k_fwd(v2 (&v)[kR], v2* lds, const Tw16k& tw) {
  const int t = threadIdx.x, l = t & 63;
  v2* reg = lds + (t >> 6) * kRegion;
  dft16<false>(v);
  apply_powers(v, tw.w0);
#pragma unroll
  for (int ka = 0; ka < kR; ka++) LDS_ST1(lds[ka * kRegion + t], v[rev16(ka)]);           // exchange 0: output ka -> wave ka
  lds_barrier();
  GACQ_SETPRIO(GACQ_QF);
#pragma unroll
  for (int j = 0; j < kR; j++) v[j] = LDS_LD(reg[l + 64 * j]);
  dft16<false>(v);
  apply_powers(v, tw.w1);
#pragma unroll
  for (int k0 = 0; k0 < kR; k0++) LDS_ST1(reg[66 * k0 + l], v[rev16(k0)]);                // transpose 1, element (k0, l) at 66 k0 + l
#pragma unroll
  for (int lh = 0; lh < kR; lh++) v[lh] = LDS_LD(reg[66 * (l & 15) + (l >> 4) + 4 * lh]);  // lane (k0 = l & 15, l_lo = l >> 4)
  GACQ_SETPRIO(GACQ_QT1);
  dft16<false>(v);
  apply_powers(v, tw.w2);
#pragma unroll
  for (int k1 = 0; k1 < kR; k1++) LDS_ST1(reg[256 * (l >> 4) + (l & 15) + 16 * k1], v[rev16(k1)]);   // transpose 2, (k0, l_lo, k1) at 256 l_lo + 16 k1 + k0
#pragma unroll
  for (int lo = 0; lo < 4; lo++) {
#pragma unroll
    for (int kh = 0; kh < 4; kh++) v[kh + 4 * lo] = LDS_LD(reg[l + 256 * lo + 64 * kh]);     // lane mu = k0 + 16 k1_lo, k1 = k1_lo + 4 kh
  }
  GACQ_SETPRIO(GACQ_QT2);
#pragma unroll
  for (int kh = 0; kh < 4; kh++) dft4<false, false>(v[kh], v[kh + 4], v[kh + 8], v[kh + 12]);   // over l_lo -> k2 at v[kh + 4 k2]
}

// Inverse transform, wave-private part.  In: v[r] = Y[(t >> 6) + 16 (t & 63) + 1024 r]; on return the wave's region holds
// z[l + 64 j'] (its 1024-point inverse transform), ready for the cross-wave exchange.  tw: conjugated bases.
__device__ __forceinline__ void ifft16k_private(v2 (&v)[kR], v2* reg, const Tw16k& tw) {
  const int l = threadIdx.x & 63;
#pragma unroll
  for (int kh = 0; kh < 4; kh++) dft4<true, false>(v[kh], v[kh + 4], v[kh + 8], v[kh + 12]);    // over k2 -> l_lo at v[kh + 4 l_lo]
#pragma unroll
  for (int lo = 0; lo < 4; lo++) {
#pragma unroll
    for (int kh = 0; kh < 4; kh++) LDS_ST1(reg[64 * (l >> 4) + (l & 15) + 256 * kh + 16 * lo], v[kh + 4 * lo]);   // (k0, l_lo, k1) at 64 k1 + 16 l_lo + k0
  }
#pragma unroll
  for (int k1 = 0; k1 < kR; k1++) v[k1] = LDS_LD(reg[l + 64 * k1]);                         // lane (k0 = l & 15, l_lo = l >> 4)
  GACQ_SETPRIO(GACQ_P3);
  apply_powers_nat(v, tw.w2);
  dft16<true>(v);                                                                   // over k1 -> l_hi
#pragma unroll
  for (int lh = 0; lh < kR; lh++) LDS_ST1(reg[65 * (l & 15) + (l >> 4) + 4 * lh], v[rev16(lh)]);   // element (k0, l = l_lo + 4 l_hi) at 65 k0 + l
#pragma unroll
  for (int k0 = 0; k0 < kR; k0++) v[k0] = LDS_LD(reg[l + 65 * k0]);
  GACQ_SETPRIO(GACQ_P4);
  apply_powers_nat(v, tw.w1);
  dft16<true>(v);                                                                   // over k0 -> j'
#pragma unroll
  for (int j = 0; j < kR; j++) LDS_ST1(reg[l + 64 * j], v[rev16(j)]);
}
// cross-wave part: gather the 16 partial transforms of n = t (mod 1024) ...
__device__ __forceinline__ void ifft16k_gather(v2 (&v)[kR], const v2* lds) {
  const int t = threadIdx.x;
#pragma unroll
  for (int ka = 0; ka < kR; ka++) v[ka] = LDS_LD(lds[ka * kRegion + t]);
}
// ... and combine them: v[rev16(j)] = N y[t + 1024 j]
__device__ __forceinline__ void ifft16k_final(v2 (&v)[kR], const Tw16k& tw) {
  apply_powers_nat(v, tw.w0);
  dft16<true>(v);
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t big_rsrc(const float2* row) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)row, 0, kBig * (int)sizeof(float2), 0x00020000);
}
// elements (t, 2 jp) and (t, 2 jp + 1) of a row in the physical lane-pair layout
__device__ __forceinline__ void ld_pair_big(__amdgpu_buffer_rsrc_t r, unsigned lane_off, int jp, v2& a, v2& b) {
  const f4 q = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(r, lane_off, (unsigned)jp * 16384u, 0));
  a = q.xy;
  b = q.zw;
}

// LDS-DMA of one spectrum row into the wave's own region: 8 x 1 KiB, lane l's 16 bytes of piece jp land at
// region + 1024 jp + 16 l -- no VGPRs are tied up while the row is in flight.
__device__ __forceinline__ void dma_row(const float2* __restrict__ row, v2* reg) {
  const char* src = reinterpret_cast<const char*>(row) + (size_t)threadIdx.x * 16;
#pragma unroll
  for (int jp = 0; jp < kR / 2; jp++)
    __builtin_amdgcn_global_load_lds((gptr_t)(src + jp * 16384), (lptr_t)(reinterpret_cast<char*>(reg) + jp * 1024), 16, 0, 0);
}
__device__ __forceinline__ void dma_wait_read(v2 (&x)[kR], const v2* reg) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const f4* p = reinterpret_cast<const f4*>(reg) + (threadIdx.x & 63);
#pragma unroll
  for (int jp = 0; jp < kR / 2; jp++) { const f4 q = p[jp * 64]; x[2 * jp] = q.xy; x[2 * jp + 1] = q.zw; }
  GACQ_SETPRIO(GACQ_P2);
}

// cross-wave (max, first argmax, sum) of one item through the scratch words behind the regions; thread 0 writes the record
__device__ __forceinline__ void big_reduce_store(char* smem, float peak, unsigned widx, float wsum, float tie_scale, RowRec* dst) {
  float* s_peak = reinterpret_cast<float*>(smem + kBigScratch);
  int* s_idx = reinterpret_cast<int*>(smem + kBigScratch + 64);
  double* s_sum = reinterpret_cast<double*>(smem + kBigScratch + 128);
  const int t = threadIdx.x;
  if ((t & 63) == 0) { s_peak[t >> 6] = peak; s_idx[t >> 6] = (int)widx; s_sum[t >> 6] = (double)wsum; }
  lds_barrier();
  if (t == 0) {
    RowRec r;
    combine_tagged(kBigThreads / 64, [&](int w) { return s_peak[w]; }, [&](int w) { return s_idx[w]; }, tie_scale, r.peak, r.idx);
    double bs = s_sum[0];
    for (int w = 1; w < kBigThreads / 64; w++) bs += s_sum[w];
    r.sum = bs;
    *dst = r;
  }
}

// forward: one workgroup per (e, f, d, b) row; output conj(FFT) in the physical lane-pair layout, 1 KiB per wave and store
template <bool DUMP, bool PLAIN = false>      // PLAIN: code spectra, see lds_forward_kernel
__global__ __launch_bounds__(kBigThreads) void lds16k_forward_kernel(const float2* __restrict__ x, size_t epoch_stride,
                                                                      float2* __restrict__ X, const double* __restrict__ freq,
                                                                      const float2* __restrict__ nco_tab,
                                                                      const float2* __restrict__ twn, int n, int FD, int B) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  v2* lds = reinterpret_cast<v2*>(smem);
  const int t = threadIdx.x;
  const unsigned row = blockIdx.x;
  const int b = (int)(row % (unsigned)B);
  const unsigned r2 = row / (unsigned)B;
  const int fd = (int)(r2 % (unsigned)FD);
  const long e = r2 / (unsigned)FD;
  const double f = PLAIN ? 0.0 : freq[fd];
  const float2* src = x + e * epoch_stride + (size_t)b * n;
  v2 v[kR], w[kR];
#pragma unroll
  for (int j = 0; j < kR; j++) {
    const int i = t + 1024 * j;
    if (PLAIN) { v[j] = ld2(src + i); continue; }
    const int k = nco_index(f, (int)i);   // gnsstools/nco.py:6-9
    if (DUMP) { reinterpret_cast<int*>(X)[row * (long)kBig + i] = k; continue; }
    v[j] = ld2(src + i);
    w[j] = ld2(nco_tab + k);
  }
  if (DUMP) return;
  const Tw16k tw = tw16k_load(twn, false);
  if (!PLAIN) {
#pragma unroll
    for (int j = 0; j < kR; j++) v[j] = cmul(v[j], w[j]);
  }
  fft16k_fwd(v, lds, tw);
  float2* dst = X + row * (long)kBig;
  const float cs = PLAIN ? 1.f : -1.f;
#pragma unroll
  for (int jp = 0; jp < kR / 2; jp++) {
    const v2 a = v[2 * jp], c = v[2 * jp + 1];
    // np.conj(fft.fft(b))  acquire-beidou-b1i.py:32   (PLAIN: the transform itself)
    *reinterpret_cast<float4*>(dst + jp * 2048 + 2 * t) = make_float4(a.x, cs * a.y, c.x, cs * c.y);
  }
}

// correlate: workgroup = (chunk of items, group of `ugroup` (epoch, Doppler) units of one XCD); per (item, unit):
// sum_b |IFFT(C_p * X_b)|/N -> (max, argmax, sum).
// Item-major since round 4: the item's code spectrum is loaded ONCE and stays in registers for every unit of the group and all B
// blocks of each, so a spectrum row crosses into the CU once per (item, group) instead of once per (item, unit) -- B1I (63 spectra =
// 8 MB against 4 MB of L2 per XCD, 200 units) fetched 1.6 GB of code spectra per launch in the unit-major order of round 3, 7.7 x the
// kernel's compulsory bytes.  The workgroups resident on an XCD (consecutive in launch order: same group, different items) walk the
// group's units side by side, so the forward spectrum of the (unit, block) they are all working on is fetched from HBM once and
// served from that XCD's L2 to the rest.
// The forward spectrum of the NEXT row is fetched by LDS-DMA into the wave's own region as soon as the cross-wave exchange of the
// current row has been read out, i.e. under the last radix-16 pass and the magnitudes -- the register file (16 + 16 complex + 16
// accumulators of 128 VGPRs) has no room for a prefetch, the LDS is idle exactly then.  Blocks -> (group, chunk): see lds_correlate().
template <bool QDUMP>
__global__ __launch_bounds__(kBigThreads) void lds16k_correlate_kernel(const float2* __restrict__ X, const float2* __restrict__ C,
                                                                        const int* __restrict__ items, const int* __restrict__ fset,
                                                                        const float2* __restrict__ twn, RowRec* __restrict__ rows,
                                                                        int E, int P, int F, int D, int B, int pch, int nchunk, int ugroup,
                                                                        float tie_scale, float* __restrict__ q_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  v2* lds = reinterpret_cast<v2*>(smem);
  const int t = threadIdx.x;
  // placement: workgroup b runs on XCD b % 8; XCD x owns the units u = x (mod 8), in groups of `ugroup` consecutive owned units
  const int xcd = blockIdx.x & 7;
  const unsigned j = blockIdx.x >> 3;
  const unsigned grp = j / (unsigned)nchunk;
  const int p0 = (int)(j % (unsigned)nchunk) * pch;
  const int p1 = min(P, p0 + pch);
  const unsigned U = (unsigned)E * (unsigned)D;
  const unsigned u0 = grp * (unsigned)ugroup * 8u + (unsigned)xcd;           // first unit of the group; the i-th is u0 + 8 i
  if (u0 >= U) return;
  const int nu = (int)min((unsigned)ugroup, (U - u0 + 7u) / 8u);
  v2* reg = lds + (t >> 6) * kRegion;
  const Tw16k tw = tw16k_load(twn, true);
  const unsigned lane_off = (unsigned)t * 16u;
  const float inv_n = 1.0f / (float)kBig;
  // first forward-spectrum row of (item p, i-th unit of the group)
  auto unit_row = [&](int p, int i) -> const float2* {
    const unsigned u = u0 + 8u * (unsigned)i;
    const long e = u / (unsigned)D;
    const int d = (int)(u % (unsigned)D);
    return X + (((e * F + fset[p]) * D + d) * (long)B) * kBig;
  };
  const float2* xrow = unit_row(p0, 0);
  dma_row(xrow, reg);
#ifdef GACQ_PHASE_TIMING16
  unsigned long long acc16_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long mark16_ = __builtin_readcyclecounter();
#endif
  for (int p = p0; p < p1; p++) {
    const __amdgpu_buffer_rsrc_t cres = big_rsrc(C + (long)items[p] * kBig);
    v2 c[kR];
#pragma unroll
    for (int jp = 0; jp < kR / 2; jp++) ld_pair_big(cres, lane_off, jp, c[2 * jp], c[2 * jp + 1]);
    for (int i = 0; i < nu; i++) {
      const unsigned u = u0 + 8u * (unsigned)i;
      const long e = u / (unsigned)D;
      const int d = (int)(u % (unsigned)D);
      // the row after this unit's last block: the next unit of the group, else the next item's first unit, else nothing
      const float2* xnext_unit = (i + 1 < nu) ? unit_row(p, i + 1) : ((p + 1 < p1) ? unit_row(p + 1, 0) : nullptr);
      float q[kR];
#pragma unroll
      for (int k = 0; k < kR; k++) q[k] = 0.f;
      for (int b = 0; b < B; b++) {
        v2 v[kR];
        GACQ_MARK16(0);                                    // previous row's tail (reduction, code-spectrum loads)
        dma_wait_read(v, reg);
#pragma unroll
        for (int jj = 0; jj < kR; jj++) v[jj] = cmul(c[jj], v[jj]);
        GACQ_MARK16(1);
        ifft16k_private(v, reg, tw);
        GACQ_MARK16(2);
        lds_barrier();
        GACQ_MARK16(3);
        ifft16k_gather(v, lds);
        lds_barrier();                                     // every wave has read this region: it may be overwritten
        GACQ_SETPRIO(GACQ_P1);
        GACQ_MARK16(4);
        const float2* nx = (b + 1 < B) ? xrow + (long)(b + 1) * kBig : xnext_unit;
        if (nx) dma_row(nx, reg);
        GACQ_MARK16(5);
        ifft16k_final(v, tw);
#pragma unroll
        for (int k = 0; k < kR; k++) {
          const v2 r = v[rev16(k)];
          q[k] += __builtin_amdgcn_sqrtf(norm2(r)) * inv_n;
        }
        GACQ_MARK16(6);
      }
      xrow = xnext_unit;
      if (QDUMP) {                                         // gacq_debug_row: the accumulated magnitude row itself (one row per launch)
#pragma unroll
        for (int k = 0; k < kR; k++) q_out[t + 1024 * k] = q[k];
      }
      float sum_f = q[0];
#pragma unroll
      for (int k = 1; k < kR; k++) sum_f += q[k];
      // lane l of wave w holds lags 64 w + l + 1024 k: first maximum as in lds_correlate_kernel
      float peak;
      unsigned widx;
      wave_first_max(q, (unsigned)__builtin_amdgcn_readfirstlane(t & ~63), 1u, 1024u, tie_scale, peak, widx);
      big_reduce_store(smem, peak, widx, wave_add_f32(sum_f), tie_scale, rows + (e * P + p) * (long)D + d);
    }
  }
#ifdef GACQ_PHASE_TIMING16
  if ((t & 63) == 0) {
#pragma unroll
    for (int i = 0; i < 8; i++) if (acc16_[i]) atomicAdd(&gacq_phase16[(t >> 6) * 8 + i], acc16_[i]);
  }
#endif
}

// Fused search for item lists in which every item has its own carrier (F == P: the GLONASS FDMA channels, or a single
// item): the forward spectrum of (e, f, d, b) is used by exactly one item, so writing it to HBM and reading it back
// (8 N bytes each way per row) buys nothing.  Workgroup = (epoch, Doppler bin, item); per block b: mix + forward transform --
// whose output order is the inverse transform's input order, so the spectrum stays in registers -- conj * C_p, inverse
// transform, |.| accumulated in registers.  Three workgroup barriers per block.  Same arithmetic in the same order as
// lds16k_forward_kernel + lds16k_correlate_kernel.
template <bool DUMP>
__global__ __launch_bounds__(kBigThreads) void lds16k_fused_kernel(const float2* __restrict__ x, size_t epoch_stride,
                                                                    const float2* __restrict__ C, const int* __restrict__ items,
                                                                    const int* __restrict__ fset, const double* __restrict__ freq,
                                                                    const float2* __restrict__ nco_tab,
                                                                    const float2* __restrict__ twn, RowRec* __restrict__ rows, int n,
                                                                    int P, int D, int B, float tie_scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  v2* lds = reinterpret_cast<v2*>(smem);
  const int t = threadIdx.x;
  unsigned blk = blockIdx.x;                          // ((e*D + d)*P + p): the P items of one (e, d) run side by side
  const int p = (int)(blk % (unsigned)P);
  blk /= (unsigned)P;
  const int d = (int)(blk % (unsigned)D);
  const long e = blk / (unsigned)D;
  const double f = freq[(long)fset[p] * D + d];
  const __amdgpu_buffer_rsrc_t cres = big_rsrc(C + (long)items[p] * kBig);
  v2* reg = lds + (t >> 6) * kRegion;
  const unsigned lane_off = (unsigned)t * 16u;
  const float inv_n = 1.0f / (float)kBig;
  float q[kR];
#pragma unroll
  for (int k = 0; k < kR; k++) q[k] = 0.f;
  for (int b = 0; b < B; b++) {
    const float2* src = x + e * epoch_stride + (size_t)b * n;
    v2 v[kR], w[kR];
#pragma unroll
    for (int j = 0; j < kR; j++) {
      const int i = t + 1024 * j;
      const int k = nco_index(f, i);                  // gnsstools/nco.py:6-9
      if (DUMP) { reinterpret_cast<int*>(rows)[(long)blockIdx.x * kBig + i] = k; continue; }
      v[j] = ld2(src + i);
      w[j] = ld2(nco_tab + k);
    }
    if (DUMP) return;
    GACQ_SETPRIO(GACQ_QX);
#pragma unroll
    for (int j = 0; j < kR; j++) v[j] = cmul(v[j], w[j]);
    // the twiddle bases are re-read per block (three 8-byte loads, L1 hits): kept live across the block loop, the two sets cost
    // 12 VGPRs the 128-register budget does not have
    const float2* twp = twn;
    asm volatile("" : "+s"(twp));
    fft16k_fwd(v, lds, tw16k_load(twp, false));
    v2 c[kR];
#pragma unroll
    for (int jp = 0; jp < kR / 2; jp++) ld_pair_big(cres, lane_off, jp, c[2 * jp], c[2 * jp + 1]);
    const Tw16k twi = tw16k_load(twp, true);
#pragma unroll
    for (int j = 0; j < kR; j++) v[j] = cmul(c[j], v2{v[j].x, -v[j].y});      // C_p * np.conj(fft.fft(b))
    ifft16k_private(v, reg, twi);
    lds_barrier();
    ifft16k_gather(v, lds);
    lds_barrier();                                    // every wave has read this region: the next block's exchange 0 may overwrite it
    GACQ_SETPRIO(GACQ_QA);
    ifft16k_final(v, twi);
#pragma unroll
    for (int k = 0; k < kR; k++) {
      const v2 r = v[rev16(k)];
      q[k] += __builtin_amdgcn_sqrtf(norm2(r)) * inv_n;
    }
  }
  float sum_f = q[0];
#pragma unroll
  for (int k = 1; k < kR; k++) sum_f += q[k];
  float peak;
  unsigned widx;
  wave_first_max(q, (unsigned)__builtin_amdgcn_readfirstlane(t & ~63), 1u, 1024u, tie_scale, peak, widx);      // lane l of wave w: lags 64 w + l + 1024 k
  big_reduce_store(smem, peak, widx, wave_add_f32(sum_f), tie_scale, rows + (e * P + p) * (long)D + d);
}


}  // namespace

namespace gacq {

#ifdef GACQ_PHASE_TIMING16
extern "C" int gacq_debug_phase16(unsigned long long* out128, int reset) {
  if (hipMemcpyFromSymbol(out128, HIP_SYMBOL(gacq_phase16), sizeof(unsigned long long) * 128) != hipSuccess) return GACQ_ERR_HIP;
  if (reset) {
    unsigned long long z[128] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(gacq_phase16), z, sizeof z) != hipSuccess) return GACQ_ERR_HIP;
  }
  return GACQ_OK;
}
#endif

// code spectra straight from the (complex, zero-extended) replica rows with the engine's own forward transform: no rocFFT plan
int r16_code_spectra(gacq_ctx* ctx, const float2* replica_rows, float2* perm, int nprn) {
  const float2* twn;
  int rcb = twiddle_cache(ctx, "W16384_lo", kBig, 1024, &twn);
  if (rcb != GACQ_OK) return rcb;
  GACQ_HIP(ctx, hipFuncSetAttribute((const void*)lds16k_forward_kernel<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, kBigLdsBytes));
  hipLaunchKernelGGL((lds16k_forward_kernel<false, true>), dim3((unsigned)nprn), dim3(kBigThreads), kBigLdsBytes, ctx->stream, replica_rows,
                     (size_t)kBig, perm, (const double*)nullptr, (const float2*)nullptr, twn, kBig, 1, 1);
  GACQ_HIP(ctx, hipGetLastError());
  return GACQ_OK;
}

int r16_forward(gacq_ctx* ctx, const float2* x, size_t nsamp, int nepoch, int n, const double* d_freq, int FD, int B, const float2* tab,
                float2* X) {
  const float2* twn;
  int rcb = twiddle_cache(ctx, "W16384_lo", kBig, 1024, &twn);
  if (rcb != GACQ_OK) return rcb;
  GACQ_HIP(ctx, hipFuncSetAttribute((const void*)lds16k_forward_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, kBigLdsBytes));
  hipLaunchKernelGGL(lds16k_forward_kernel<false>, dim3((unsigned)((long)nepoch * FD * B)), dim3(kBigThreads), kBigLdsBytes, ctx->stream, x,
                     nsamp, X, d_freq, tab, twn, n, FD, B);
  GACQ_HIP(ctx, hipGetLastError());
  return GACQ_OK;
}

// one carrier per item (F == P): forward + correlate in one kernel, no X buffer
int r16_fused_search(gacq_ctx* ctx, const float2* x, size_t nsamp, int nepoch, int n, const float2* spectra, const int* d_items,
                     const int* d_fset, const double* d_freq, const float2* tab, int nitems, int D, int B, RowRec* rows, float tie_scale) {
  const float2* twn;
  int rc = twiddle_cache(ctx, "W16384_lo", kBig, 1024, &twn);
  if (rc != GACQ_OK) return rc;
  GACQ_HIP(ctx, hipFuncSetAttribute((const void*)lds16k_fused_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, kBigLdsBytes));
  hipLaunchKernelGGL(lds16k_fused_kernel<false>, dim3((unsigned)((long)nepoch * D * nitems)), dim3(kBigThreads), kBigLdsBytes, ctx->stream, x,
                     nsamp, spectra, d_items, d_fset, d_freq, tab, twn, rows, n, nitems, D, B, tie_scale);
  GACQ_HIP(ctx, hipGetLastError());
  return GACQ_OK;
}

int r16_debug_nco(gacq_ctx* ctx, int n, const double* d_freq, bool fused, int* d_idx) {
  if (fused) {
    int rc = ensure(ctx, ctx->fset, sizeof(int));
    if (rc != GACQ_OK) return rc;
    ctx->up_fset.clear();
    GACQ_HIP(ctx, hipMemsetAsync(ctx->fset.p, 0, sizeof(int), ctx->stream));
    GACQ_HIP(ctx, hipFuncSetAttribute((const void*)lds16k_fused_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, kBigLdsBytes));
    hipLaunchKernelGGL(lds16k_fused_kernel<true>, dim3(1), dim3(kBigThreads), kBigLdsBytes, ctx->stream, (const float2*)nullptr, (size_t)0,
                       (const float2*)nullptr, (const int*)ctx->fset.p, (const int*)ctx->fset.p, d_freq, (const float2*)nullptr,
                       (const float2*)nullptr, (RowRec*)d_idx, n, 1, 1, 1, 1.0f);
  } else {
    GACQ_HIP(ctx, hipFuncSetAttribute((const void*)lds16k_forward_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, kBigLdsBytes));
    hipLaunchKernelGGL(lds16k_forward_kernel<true>, dim3(1), dim3(kBigThreads), kBigLdsBytes, ctx->stream, (const float2*)nullptr, (size_t)0,
                       (float2*)d_idx, d_freq, (const float2*)nullptr, (const float2*)nullptr, n, 1, 1);
  }
  GACQ_HIP(ctx, hipGetLastError());
  return GACQ_OK;
}

int r16_correlate(gacq_ctx* ctx, const float2* X, const float2* spectra, const int* d_items, const int* d_fset, int nepoch, int nitems,
                  int F, int D, int B, RowRec* rows, float tie_scale, float* q_out) {
  if (q_out && (nepoch != 1 || nitems != 1 || D != 1)) return set_error(ctx, GACQ_ERR_BAD_ARG, "LDS FFT engine: a row dump takes exactly one row");
  const float2* twn;
  int rcb = twiddle_cache(ctx, "W16384_lo", kBig, 1024, &twn);
  if (rcb != GACQ_OK) return rcb;
  // One 1024-thread workgroup per CU, 32 per XCD.  Workgroup = (one item, a group of G of the XCD's units): the item's code
  // spectrum is read once per workgroup, so G is as large as still leaves ~2 rounds of workgroups per XCD (>= 60; at most 32
  // units), evened out so that the groups of an XCD have the same size where possible.  B1I (63 items, 200 units, B = 10):
  // 25 units per XCD -> G = 25, 63 workgroups of 250 rows per XCD.  Measured (profiles/r04_16k_unit_group_sweep.log): HBM
  // traffic per launch 2.07 GB (round 3, unit-major) -> 1.07 GB (G = 5) -> 0.89 (9) -> 0.78 (13) -> 0.59 GB (25) = 2.2 x the
  // compulsory bytes, kernel time unchanged within 2 % (3.37-3.45 ms in the four-signal step): HBM was never what paced it.
  const long units = (long)nepoch * D;
  int pch = 1;
  if (ctx->opt[GACQ_OPT_LDS_PCH] >= 1) pch = (int)ctx->opt[GACQ_OPT_LDS_PCH];
  pch = std::min(pch, nitems);
  const int nchunk = (nitems + pch - 1) / pch;
  const long units8 = (units + 7) / 8;                                 // units per XCD
  long g0 = std::max<long>(1, std::min<long>(32, units8 * nchunk / 60));
  int ugroup = (int)((units8 + ((units8 + g0 - 1) / g0) - 1) / ((units8 + g0 - 1) / g0));
  if (ctx->opt[GACQ_OPT_LDS_UGROUP] >= 1) ugroup = (int)std::min<long>(ctx->opt[GACQ_OPT_LDS_UGROUP], units8);
  const long groups = (units8 + ugroup - 1) / ugroup;
  auto kern16 = q_out ? lds16k_correlate_kernel<true> : lds16k_correlate_kernel<false>;
  GACQ_HIP(ctx, hipFuncSetAttribute((const void*)kern16, hipFuncAttributeMaxDynamicSharedMemorySize, kBigLdsBytes));
  hipLaunchKernelGGL(kern16, dim3((unsigned)(8 * groups * nchunk)), dim3(kBigThreads), kBigLdsBytes, ctx->stream, X,
                     spectra, d_items, d_fset, twn, rows, nepoch, nitems, F, D, B, pch, nchunk, ugroup, tie_scale, q_out);
  GACQ_HIP(ctx, hipGetLastError());
  return GACQ_OK;
}

}  // namespace gacq
