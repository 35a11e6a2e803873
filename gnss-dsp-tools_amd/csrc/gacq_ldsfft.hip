// LDS-resident FFT engine for gfx950: the whole length-N transform of one correlation row lives in
// one workgroup's registers + LDS, so the stage boundaries of the rocFFT pipeline (mix -> FFT,
// conj-mul -> IFFT -> |.| -> reduce) never touch HBM.
//
//   lds_forward_kernel    x window --(table NCO mix)--> FFT_N --> conj --> X[row]       (K1+F1 fused)
//   lds_correlate_kernel  for p in PRN chunk: q = sum_b | IFFT_N(C_p * X[e,f,d,b]) |/N ; (max, argmax, sum)
//                                                                                        (K2+F2+K3 fused)
//
// Decomposition (N = 4096 = 16*16*16, one wave64-friendly 256-thread workgroup, 16 points per lane):
//   n = n0 + 16 n1 + 256 n2,  k = k0 + 16 k1 + 256 k2
//   pass 1: lane (n0,n1) holds n2=0..15 -> DFT16 over n2 -> k0 ; twiddle W_N^{(n0+16 n1) k0}
//   pass 2: lane (n0,k0) holds n1=0..15 -> DFT16 over n1 -> k1 ; twiddle W_256^{n0 k1}
//   pass 3: lane (k0,k1) holds n0=0..15 -> DFT16 over n0 -> k2
// Global loads/stores are lane-contiguous in every pass-1 load and pass-3 store (index = lane + 256*j);
// the two LDS transposes are bank-conflict free: exchange 1 is lane-contiguous on both sides, exchange 2
// writes with row pitch 257 (odd) so that the 16 lanes of a ds_write_b64 group hit 16 distinct bank pairs.
#include "gacq_common.h"
#include "gacq_cplx.h"
#include "gacq_ldsutil.h"

#include <cmath>
#include <cstdlib>

using namespace gacq;

namespace {

constexpr int kLdsN = 4096;            // supported length (this round)
constexpr int kPitch = 257;            // exchange-2 row pitch in complex elements
constexpr int kLdsElems = 16 * kPitch; // 4112 complex = 32.9 KB -> 4 workgroups per CU

// w^1..w^15 into pw[0..14] (same product tree as apply_powers)
__device__ __forceinline__ void make_powers(v2 (&pw)[15], v2 w1) {
  pw[0] = w1;
  pw[1] = cmul(w1, w1);        pw[2] = cmul(pw[1], w1);      pw[3] = cmul(pw[1], pw[1]);
  pw[4] = cmul(pw[3], w1);     pw[5] = cmul(pw[2], pw[2]);   pw[6] = cmul(pw[3], pw[2]);   pw[7] = cmul(pw[3], pw[3]);
  pw[8] = cmul(pw[7], w1);     pw[9] = cmul(pw[4], pw[4]);   pw[10] = cmul(pw[7], pw[2]);  pw[11] = cmul(pw[5], pw[5]);
  pw[12] = cmul(pw[7], pw[4]); pw[13] = cmul(pw[6], pw[6]);  pw[14] = cmul(pw[7], pw[6]);
}

// Length-4096 transform of the 16 values per lane. In: v[j] = x[t + 256 j]; out: v[rev16(k2)] = X[t + 256 k2].
// wa = W_4096^t, wb = W_256^(t & 15) (forward values; conjugated here when INV).  Three forms:
//   plain               both passes' powers (W_4096^t)^k, (W_256^(t & 15))^k are rebuilt from wa / wb, 14 complex products per pass
//   ROWLOOP (inverse)   for a kernel's row loop (lds_correlate_kernel): pass 1 rebuilt from wa, the pass-2 powers read from an LDS table
//                       (tb2[16 (k - 1)], already conjugated, tb2 already offset by the lane's class t & 15), rising wave priority
//                       through the row (F4K_PRIO below)
//   FUSED (a ROWLOOP)   the fused kernel's item loop: the pass-1 powers too come precomputed, in registers (*pa, already conjugated),
//                       and the last radix-4 layer leaves its outputs planar in *pl instead of in v (dft16_inv_planar, gacq_cplx.h):
//                       pl[j] = (re X[t + 256 j], re X[t + 256 (j + 8)]), pl[8 + j] the imaginary parts
//   RESIDENT (forward)  the fused kernel's forward transform: both passes' powers are the conjugates of the inverse transform's resident
//                       ones (*pa in registers, tb2 in LDS), multiplied through the neg modifiers (cmul_conj).  cmul is sign-symmetric
//                       under IEEE rounding -- conj(cmul(a, b)) and cmul(conj a, conj b) are the same bits -- so these are the values the
//                       plain form rebuilds from wa / wb with its two product trees, 28 complex products per transform less
// Rising wave priority through the segments of a 4096-point row (the caller resets it to GACQ_F4K_P4 at the top of its row loop):
// after the exchange-1 writes | after the exchange-2 writes | after the exchange-2 reads have been issued.  The four
// waves of a SIMD belong to four independent workgroups; letting the one that is furthest into its row issue first keeps the workgroups
// out of phase, so one's LDS round trips and barriers fall under another's arithmetic.  Headline step (1024 epochs x 40 bins x 32 PRNs):
// 5.50-5.53 -> 5.30-5.34 ms, falling levels (3-2-1-0, what the kernels of gacq_lds16k_r16.hip use inside ONE workgroup) 5.56, levels raised only
// in the last segment 5.48 (profiles/r05_headline_kernel_wave_priority_sweep.log).  -1 = leave the priority alone.
// lds_correlate_kernel: table + priorities -2.5 % at B = 10 / 80.  (The same levels in lds_inner_correlate_kernel -- engine 4's writer,
// store-bound -- measured within the run-to-run noise, 0-2 %: not applied there.)
#ifndef GACQ_F4K_P1      // each level has its own default, so that a variant build can set one of them
#define GACQ_F4K_P1 1
#endif
#ifndef GACQ_F4K_P2
#define GACQ_F4K_P2 2
#endif
#ifndef GACQ_F4K_P3
#define GACQ_F4K_P3 3
#endif
#ifndef GACQ_F4K_P4
#define GACQ_F4K_P4 0
#endif
#ifndef GACQ_F4K_P0
#define GACQ_F4K_P0 -1      // at the first radix-16 pass (sweeps only)
#endif
#define F4K_PRIO(n) do { if ((n) >= 0) asm volatile("s_setprio %0" :: "n"(n) : "memory"); } while (0)
template <bool INV, bool ROWLOOP = false, bool FUSED = false, bool RESIDENT = false>
__device__ __forceinline__ void fft4096(v2 (&v)[kR], v2* lds, v2 wa, v2 wb, const v2* tb2 = nullptr, const v2 (*pa)[15] = nullptr,
                                        v2 (*pl)[kR] = nullptr) {
  static_assert(INV || !ROWLOOP, "table and priorities: inverse transform only");
  static_assert(ROWLOOP || !FUSED, "the fused item loop is a row loop");
  static_assert(!RESIDENT || (!INV && !ROWLOOP), "conjugates of the resident powers: forward transform only");
  const int t = threadIdx.x;
  if (INV) { wa.y = -wa.y; wb.y = -wb.y; }
  F4K_PRIO(ROWLOOP ? GACQ_F4K_P0 : -1);
  dft16<INV>(v);
  if (FUSED) {
#pragma unroll
    for (int k = 1; k < kR; k++) v[rev16(k)] = cmul(v[rev16(k)], (*pa)[k - 1]);
  } else if (RESIDENT) {
#pragma unroll
    for (int k = 1; k < kR; k++) v[rev16(k)] = cmul_conj(v[rev16(k)], (*pa)[k - 1]);
  } else apply_powers(v, wa);
  {  // exchange 1: (n0,n1;k0) -> (n0,k0;n1)
    const int wbase = (t & 15) + 256 * (t >> 4);
#pragma unroll
    for (int k = 0; k < kR; k++) lds[wbase + 16 * k] = v[rev16(k)];
    F4K_PRIO(ROWLOOP ? GACQ_F4K_P1 : -1);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kR; j++) v[j] = LDS_LD(lds[t + 256 * j]);
  }
  dft16<INV>(v);
  if (ROWLOOP) {
#pragma unroll
    for (int k = 1; k < kR; k++) v[rev16(k)] = cmul(v[rev16(k)], LDS_LD(tb2[16 * (k - 1)]));
  } else if (RESIDENT) {
#pragma unroll
    for (int k = 1; k < kR; k++) v[rev16(k)] = cmul_conj(v[rev16(k)], LDS_LD(tb2[16 * (k - 1)]));
  } else apply_powers(v, wb);
  __syncthreads();   // all exchange-1 reads done before the buffer is reused
  {  // exchange 2: (n0,k0;k1) -> (k0,k1;n0)
    const int wbase = (t >> 4) + kPitch * (t & 15);
#pragma unroll
    for (int k = 0; k < kR; k++) lds[wbase + 16 * k] = v[rev16(k)];
    F4K_PRIO(ROWLOOP ? GACQ_F4K_P2 : -1);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kR; j++) v[j] = LDS_LD(lds[t + kPitch * j]);
    F4K_PRIO(ROWLOOP ? GACQ_F4K_P3 : -1);
  }
  if (FUSED) dft16_inv_planar(v, *pl);
  else dft16<INV>(v);
}


// Lane-pair layout used for X and C_p inside this engine: natural index i = t + 256 j (t = lane, j = 0..15)
// is stored at (j>>1)*512 + 2 t + (j&1), so one lane's values for j = 2jp, 2jp+1 are 16 contiguous bytes and
// a wave reads/writes 1 KiB per instruction.  Rows are fetched with buffer loads: the row base lives in an
// SGPR resource, the lane offset (16 t) in one VGPR, the piece offset in an SGPR -- no VALU address math.

__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_rsrc(const float2* row) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)row, 0, kLdsN * (int)sizeof(float2), 0x00020000);
}
// values j = 2jp (lo) and 2jp+1 (hi) of this lane
__device__ __forceinline__ void ld_pair(__amdgpu_buffer_rsrc_t r, unsigned lane_off, int jp, v2& a, v2& b) {
  const f4 q = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(r, lane_off, (unsigned)jp * 4096u, 0));
  a = q.xy;
  b = q.zw;
}

// ---- forward: one workgroup per (e, f, d, b) row -------------------------------------------------
// DUMP (test hook gacq_debug_nco_indices): the index expression below, on the same frequency table, is stored as int32 into X
// (reinterpreted) and the kernel returns; x is not read.
// PLAIN (code spectra, once per signal): row r of x is transformed as it is -- no carrier wipe-off, no conjugation -- so the code
// spectra come out of the same transform, in the same layout, as the forward spectra they are multiplied with (c = fft.fft(c),
// acquire-gps-l1.py:24), and building a signal needs no rocFFT plan.
template <bool DUMP, bool PLAIN = false>
__global__ __launch_bounds__(kBlock) void lds_forward_kernel(const float2* __restrict__ x, size_t epoch_stride,
                                                              float2* __restrict__ X, const double* __restrict__ freq,
                                                              const float2* __restrict__ nco_tab,
                                                              const float2* __restrict__ tw, int n, int FD, int B) {
  __shared__ v2 lds[kLdsElems];
  const int t = threadIdx.x;
  const unsigned row = blockIdx.x;        // ((e*FD + fd)*B + b); 32-bit index math (64-bit divisions are ~100 scalar ops)
  const int b = (int)(row % (unsigned)B);
  const unsigned r2 = row / (unsigned)B;
  const int fd = (int)(r2 % (unsigned)FD);
  const long e = r2 / (unsigned)FD;
  const double f = PLAIN ? 0.0 : freq[fd];
  const float2* src = x + e * epoch_stride + (size_t)b * n;
  v2 v[kR], w[kR];
#pragma unroll
  for (int j = 0; j < kR; j++) {
    const int i = t + 256 * j;
    if (PLAIN) { v[j] = ld2(src + i); continue; }
    // table NCO, index in fp64 exactly as numpy: floor((0 + f*i)*1024) mod 1024   (gnsstools/nco.py:6-9)
    const int k = nco_index(f, (int)i);
    if (DUMP) { reinterpret_cast<int*>(X)[row * (long)kLdsN + i] = k; continue; }
    v[j] = ld2(src + i);
    w[j] = ld2(nco_tab + k);
  }
  if (DUMP) return;
  const v2 twa = ld2(tw + t), twb = ld2(tw + 16 * (t & 15));
  if (!PLAIN) {
#pragma unroll
    for (int j = 0; j < kR; j++) v[j] = cmul(v[j], w[j]);
  }
  fft4096<false>(v, lds, twa, twb);
  float2* dst = X + row * (long)kLdsN;
  const float cs = PLAIN ? 1.f : -1.f;
#pragma unroll
  for (int jp = 0; jp < kR / 2; jp++) {
    const v2 a = v[rev16(2 * jp)], b = v[rev16(2 * jp + 1)];
    // store conj(FFT) in the lane-pair layout: np.conj(fft.fft(b))  acquire-gps-l1.py:32   (PLAIN: the transform itself)
    *reinterpret_cast<float4*>(dst + jp * 512 + 2 * t) = make_float4(a.x, cs * a.y, b.x, cs * b.y);
  }
}

// ---- inner transforms of the split engine (N = R * 4096, gacq_split.hip) -----------------------------
// In-place forward FFT of natural-order rows (the outer stage's A[k1][n2]); output in the lane-pair layout,
// conjugated for sample spectra (CONJ) and plain for code spectra.
template <bool CONJ>
__global__ __launch_bounds__(kBlock) void lds_inner_forward_kernel(float2* __restrict__ rows, const float2* __restrict__ tw) {
  __shared__ v2 lds[kLdsElems];
  const int t = threadIdx.x;
  float2* row = rows + (long)blockIdx.x * kLdsN;
  v2 v[kR];
#pragma unroll
  for (int j = 0; j < kR; j++) v[j] = ld2(row + t + 256 * j);
  const v2 twa = ld2(tw + t), twb = ld2(tw + 16 * (t & 15));
  fft4096<false>(v, lds, twa, twb);
  // every lane has read its 16 inputs before the first exchange barrier, so the row can be overwritten in place
#pragma unroll
  for (int jp = 0; jp < kR / 2; jp++) {
    const v2 a = v[rev16(2 * jp)], b = v[rev16(2 * jp + 1)];
    *reinterpret_cast<float4*>(row + jp * 512 + 2 * t) = CONJ ? make_float4(a.x, -a.y, b.x, -b.y) : make_float4(a.x, a.y, b.x, b.y);
  }
}

// Z'[(g,b)][k1][n2] = W_N^{-n2 k1} * IFFT_4096( C_p[k1][.] * X[e,f,d,b][k1][.] )[n2]      (K2 + inner inverse + twiddle)
// Workgroup = (k1, chunk of pch consecutive (epoch, item) pairs, Doppler bin, block).  The X row and the W_N twiddle powers
// depend only on the workgroup, so they stay in registers while the items change (X is reloaded only when its row pointer
// changes: epoch or frequency-set boundary inside the chunk).  Consecutive workgroups share (k1, item chunk), so those pch
// code-spectrum rows are hot in every XCD's L2.  [g0, g0+ng) = (e,p,d) groups whose Z rows exist in this workspace pass.
// twn holds W_N^m for m < 256 R.
__global__ __launch_bounds__(kBlock, 4) void lds_inner_correlate_kernel(const float2* __restrict__ X, const float2* __restrict__ C,
                                                                        const int* __restrict__ items, const int* __restrict__ fset,
                                                                        const float2* __restrict__ tw, const float2* __restrict__ twn,
                                                                        float2* __restrict__ Z, long g0, long ng, long ep_first,
                                                                        int nblk_ep, int pch, int P, int F, int D, int B, int R) {
  __shared__ v2 lds[kLdsElems];
  const int t = threadIdx.x;
  unsigned blk = blockIdx.x;                   // 32-bit index math (64-bit divisions are ~100 scalar ops each)
  const int b = (int)(blk % (unsigned)B);
  blk /= (unsigned)B;
  const int d = (int)(blk % (unsigned)D);
  blk /= (unsigned)D;
  const unsigned epc = blk % (unsigned)nblk_ep;
  const int k1 = (int)(blk / (unsigned)nblk_ep);
  const long ep0 = ep_first + (long)epc * pch;
  long e = ep0 / P;
  int p = (int)(ep0 - e * P) - 1;
  const unsigned lane_off = (unsigned)t * 16u;
  const v2 twa = ld2(tw + t), twb = ld2(tw + 16 * (t & 15));
  // lane holds n2 = t + 256 k: W_N^{-k1 (t + 256 k)} = conj(W_N^{k1 t}) * conj(W_N^{256 k1})^k
  v2 base = ld2(twn + k1 * t), step = ld2(twn + 256 * k1);
  base.y = -base.y;
  step.y = -step.y;
  // the 16 output twiddles of this lane depend on (k1, t) only: built once per workgroup (multiplication depth <= 5), one product
  // per output afterwards instead of up to three (base, step^(k&3), step^(k&~3))
  v2 tk[kR];
  {
    TwPow tp;
    tp.init<15>(step);
    tk[0] = base;
#pragma unroll
    for (int k = 1; k < kR; k++) tk[k] = tp.apply(base, k);
  }
  const float2* have = nullptr;
  v2 xr[kR];
  for (int i = 0; i < pch; i++) {
    if (++p == P) { p = 0; e++; }
    const long g = (ep0 + i) * D + d;
    if (g < g0 || g >= g0 + ng) continue;      // uniform over the workgroup
    const float2* xrow = X + ((((e * F + fset[p]) * D + d) * (long)B + b) * R + k1) * kLdsN;
    const __amdgpu_buffer_rsrc_t cres = row_rsrc(C + ((long)items[p] * R + k1) * kLdsN);
    v2 v[kR];
#pragma unroll
    for (int jp = 0; jp < kR / 2; jp++) ld_pair(cres, lane_off, jp, v[2 * jp], v[2 * jp + 1]);      // loads first, asm afterwards
    if (xrow != have) {
      const __amdgpu_buffer_rsrc_t xres = row_rsrc(xrow);
#pragma unroll
      for (int jp = 0; jp < kR / 2; jp++) ld_pair(xres, lane_off, jp, xr[2 * jp], xr[2 * jp + 1]);
      have = xrow;
    }
#pragma unroll
    for (int jj = 0; jj < kR; jj++) v[jj] = cmul(v[jj], xr[jj]);
    fft4096<true>(v, lds, twa, twb);
    // the row goes out in the lane-pair layout (n2 = t + 256 k at (k >> 1) * 512 + 2 t + (k & 1)): one 16-byte store per two
    // outputs, 1 KiB per wave and instruction; split_outer_inverse_kernel (paired) undoes the permutation in its index arithmetic
    float2* dst = Z + (((g - g0) * B + b) * R + k1) * (long)kLdsN;
    if (k1 == 0) {
#pragma unroll
      for (int kp = 0; kp < kR / 2; kp++) {
        const v2 a = v[rev16(2 * kp)], c = v[rev16(2 * kp + 1)];
        *reinterpret_cast<float4*>(dst + kp * 512 + 2 * t) = make_float4(a.x, a.y, c.x, c.y);
      }
    } else {
#pragma unroll
      for (int kp = 0; kp < kR / 2; kp++) {
        const v2 a = cmul(v[rev16(2 * kp)], tk[2 * kp]), c = cmul(v[rev16(2 * kp + 1)], tk[2 * kp + 1]);
        *reinterpret_cast<float4*>(dst + kp * 512 + 2 * t) = make_float4(a.x, a.y, c.x, c.y);
      }
    }
    __syncthreads();                           // exchange-2 reads done before the next item's exchange-1 writes
  }
}

// ---- correlate: workgroup = (epoch, doppler, chunk of items); epochs pinned to XCDs ---------------
//   B1      single block (B == 1) and one carrier: no q[] accumulator, magnitudes are reduced as they are produced, and the forward
//           spectrum X[e,d] stays in registers across the item loop (halves L2 reads)
//   QDUMP   gacq_debug_row: the accumulated magnitude row itself goes out too
// Two waves per SIMD declared, X cached, the pass-1 twiddle powers left to the compiler to hoist: the winner of the round-1 A/B of ten
// register / occupancy variants (profiles/r01_ab_variants_*.log, all within 5 %); the others are gone from the build.
template <bool B1, bool QDUMP = false>
__global__ __launch_bounds__(kBlock, 2) void lds_correlate_kernel(const float2* __restrict__ X, const float2* __restrict__ C,
                                                                  const int* __restrict__ items, const int* __restrict__ fset,
                                                                  const float2* __restrict__ tw, RowRec* __restrict__ rows,
                                                                  int E, int P, int F, int D, int B, int pch, int nchunk, float tie_scale,
                                                                  float* __restrict__ q_out) {
  __shared__ v2 lds[kLdsElems];
  __shared__ float s_peak[kBlock / 64];
  __shared__ int s_idx[kBlock / 64];
  __shared__ double s_sum[kBlock / 64];
  const int t = threadIdx.x;
  // XCD-aware placement: workgroup b runs on XCD b%8 (MI355X_MICROARCH.md, workgroup dispatch).  The unit of
  // reuse is one (epoch, Doppler) pair u: its forward spectrum X[u] (B*32 KB) is read by all nchunk workgroups
  // of that unit, so they are all placed on XCD u%8 and share that XCD's L2; the code spectra (P*32 KB) end
  // up resident in every XCD's 4 MB L2.  Works for any E (a single-epoch search still fills all 8 XCDs).
  const int xcd = blockIdx.x & 7;
  const unsigned j = blockIdx.x >> 3;
  const unsigned u = (j / (unsigned)nchunk) * 8 + xcd;
  if (u >= (unsigned)E * (unsigned)D) return;
  const long e = u / (unsigned)D;
  const int d = (int)(u % (unsigned)D);
  const int p0 = (int)(j % (unsigned)nchunk) * pch;
  const int p1 = min(P, p0 + pch);
  const v2 wa = ld2(tw + t), wb = ld2(tw + 16 * (t & 15));
  // as in lds_fused4k_kernel: the pass-2 twiddle powers of the inverse transform from a 1.9 KB LDS table built once per workgroup with
  // apply_powers' product tree (bit-identical records), and rising wave priorities through the row (fft4096's ROWLOOP form)
  __shared__ v2 s_tw2[15 * 16];
  if (t < 16) {
    v2 pw[15];
    make_powers(pw, v2{wb.x, -wb.y});
#pragma unroll
    for (int k = 0; k < 15; k++) s_tw2[16 * k + t] = pw[k];
  }
  const float inv_n = 1.0f / (float)kLdsN;
  v2 xr[B1 ? kR : 1];
  const unsigned lane_off = (unsigned)t * 16u;
  if (B1) {
    const __amdgpu_buffer_rsrc_t xres = row_rsrc(X + (((e * F + fset[p0]) * D + d) * (long)B) * kLdsN);   // F == 1 here
#pragma unroll
    for (int jp = 0; jp < kR / 2; jp++) ld_pair(xres, lane_off, jp, xr[2 * jp], xr[2 * jp + 1]);
  }
  for (int p = p0; p < p1; p++) {
    const __amdgpu_buffer_rsrc_t cres = row_rsrc(C + (long)items[p] * kLdsN);
    const float2* xs = X + (((e * F + fset[p]) * D + d) * (long)B) * kLdsN;
    float q[kR];                           // B1: the magnitudes of the one block; else the sum over blocks
    if (!B1) {
#pragma unroll
      for (int k = 0; k < kR; k++) q[k] = 0.f;
    }
    const int nb = B1 ? 1 : B;
    v2 cc[B1 ? 1 : kR];                    // B > 1: the item's code spectrum stays in registers for all blocks
    if (!B1) {
#pragma unroll
      for (int jp = 0; jp < kR / 2; jp++) ld_pair(cres, lane_off, jp, cc[2 * jp], cc[2 * jp + 1]);
    }
    for (int b = 0; b < nb; b++) {
      F4K_PRIO(GACQ_F4K_P4);
      v2 v[kR];
      // all loads are issued before the first asm op: the machine scheduler does not move loads across inline asm, so
      // an interleaved load/cmul loop would wait for every load separately
      if (B1) {
#pragma unroll
        for (int jp = 0; jp < kR / 2; jp++) ld_pair(cres, lane_off, jp, v[2 * jp], v[2 * jp + 1]);
#pragma unroll
        for (int jj = 0; jj < kR; jj++) v[jj] = cmul(v[jj], xr[jj]);
      } else {
        const __amdgpu_buffer_rsrc_t xres = row_rsrc(xs + (long)b * kLdsN);
#pragma unroll
        for (int jp = 0; jp < kR / 2; jp++) ld_pair(xres, lane_off, jp, v[2 * jp], v[2 * jp + 1]);
#pragma unroll
        for (int jj = 0; jj < kR; jj++) v[jj] = cmul(cc[jj], v[jj]);
      }
      if (!B1 && b > 0) __syncthreads();   // previous transform's exchange-2 reads are complete
      fft4096<true, true>(v, lds, wa, wb, s_tw2 + (t & 15));
      if (B1) {
        // magnitudes straight from the transform output; lane holds lags t + 256 k.  The 1/N of ifft is a power of two: it is
        // applied once to the reduced values below instead of to all 16 magnitudes.
#pragma unroll
        for (int k = 0; k < kR; k++) {
          const v2 r = v[rev16(k)];
          q[k] = __builtin_amdgcn_sqrtf(norm2(r));                  // np.absolute(ifft(...)) * N
        }
      } else {
#pragma unroll
        for (int k = 0; k < kR; k++) {
          const v2 r = v[rev16(k)];
          q[k] += __builtin_amdgcn_sqrtf(norm2(r)) * inv_n;
        }
      }
    }
    if (QDUMP) {                                         // gacq_debug_row: the accumulated magnitude row itself (one row per launch)
#pragma unroll
      for (int k = 0; k < kR; k++) q_out[t + 256 * k] = B1 ? q[k] * inv_n : q[k];
    }
    float sum_f = q[0];
#pragma unroll
    for (int k = 1; k < kR; k++) sum_f += q[k];
    float wmaxf;
    unsigned widx;
    wave_first_max(q, (unsigned)__builtin_amdgcn_readfirstlane(t & ~63), 1u, 256u, tie_scale, wmaxf, widx);      // first maximum, like np.argmax
    const unsigned wmax = __builtin_bit_cast(unsigned, B1 ? wmaxf * inv_n : wmaxf);
    const float wsum = wave_add_f32(B1 ? sum_f * inv_n : sum_f);
    if ((t & 63) == 0) { s_peak[t >> 6] = __builtin_bit_cast(float, wmax); s_idx[t >> 6] = (int)widx; s_sum[t >> 6] = (double)wsum; }
    __syncthreads();   // also orders this item's exchange-2 reads before the next item's exchange-1 writes
    if (t == 0) {
      RowRec r;
      combine_tagged(kBlock / 64, [&](int w) { return s_peak[w]; }, [&](int w) { return s_idx[w]; }, tie_scale, r.peak, r.idx);
      r.sum = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
      rows[(e * P + p) * (long)D + d] = r;
    }
  }
}

// ---- N = 4096, one block, one carrier: forward + correlate in ONE kernel ---------------------------------------------------
// Workgroup = (epoch, Doppler bin, chunk of pch items).  Prologue: load the x window, table-NCO mix (fp64 index as in
// lds_forward_kernel), forward FFT, conjugate -- the spectrum never leaves the registers: the transform's output lane/register
// convention (register rev16(k2) of lane t holds X[t + 256 k2]) is the input convention of the inverse transform, so
// xr[j] = conj(v[rev16(j)]) is a compile-time register renaming.  Then the item loop of lds_correlate_kernel<B1>.
// No X buffer (84 MB at the bench shape), no forward launch, no launch boundary; the price is one forward transform per
// workgroup instead of one per (epoch, Doppler bin), i.e. nchunk - 1 redundant ones per unit, which is why this kernel is
// launched with larger item chunks (16-32) than the two-kernel path (8).  Same arithmetic in the same order as
// lds_forward_kernel + lds_correlate_kernel: records are bit-identical (test_fused_4096_kernel_equals_two_kernel_path).
// The 15 pass-1 twiddle powers of the inverse transform stay in registers for the whole item loop (30 VGPRs, 14 complex
// products per row less); the maximum-first peak search freed exactly that much of the 128-register budget of 4 waves per SIMD.
// Records (kRing): lane 0 of each wave writes its partial (peak, idx | tie bit, sum) of item p into slot (p - p0) & 31 of a
// 32 x 4 ring in LDS before the row's closing barrier.  After the barrier of slot 31, or of the chunk's last row, lane s <= slot of
// wave 0 combines the four partials of item p - slot + s (combine_tagged over waves 0..3, sum ((s0 + s1) + s2) + s3 in fp64: the
// values and the order of a combine after every row, so the records are the same bits) and stores its record.  The combine -- four
// dependent LDS round trips, ~45 instructions, three fp64 adds, the record store -- used to run on one lane after every row while
// the other three waves waited for wave 0 at the next row's first barrier; now once per 32 rows, 32 lanes wide (a combine after
// every row was the other side of the A/B in profiles/r14_fused4k_item_loop_ab.log).  The ring is safe for any pch: wave 0
// flushes before it reaches that barrier and no wave writes a slot again before the same row's third one.
// Fetching the next item's code row ahead (behind the magnitudes, in flight across the closing barrier) measured 3 % SLOWER on its
// own and no faster on top of the ring (profiles/r14_fused4k_item_loop_ab.log): not built in.
// (Round 3's single-launch instantiation -- the Doppler scan by the workgroup that completes an item's last bin, records handed
// over with agent-scope stores and an arrival counter -- measured slower than the three short launches it replaced (21.8 us of kernel
// against 6.8 + 12.3 + 6.5 us whose launch latencies overlap, profiles/r03_single_search_latency.log) and had no hook for the tie-safe
// re-evaluation; removed in round 6.)
//
// Unit runs.  A workgroup walks `run` consecutive work items (one work item = one (epoch, Doppler bin, item chunk): what a workgroup
// used to be) and pays what does not depend on the work item once: the two twiddle loads, the pass-1 powers pwa, the pass-2 table
// s_tw2, the lane offset and the decode of its block index.  Per work item, in the same order and the same bits as before: x window,
// NCO mix, forward transform, item loop, ring flush.  The forward transform takes its powers from pwa / s_tw2 (fft4096's RESIDENT form).
// Nothing between two work items needs a barrier of its own: the last row's closing barrier orders its exchange-2 reads before the next
// forward transform's exchange-1 writes, and no wave writes ring slot 0 again before it has passed that transform's barriers, which wave
// 0 reaches only after its flush.
//
// GACQ_F4K_STAMPS (a diagnostic variant built by tools/build_variant.sh for tools/f4k_stamps.py, never the product library): lane 0 of
// every workgroup stores the 100 MHz wall clock at kernel entry, before its first row and after its last row, and where it ran
// (HW_ID, XCC_ID), into a buffer the tool hands over with gacq_debug_f4k_stamps.
#ifdef GACQ_F4K_STAMPS
__device__ unsigned long long* g_f4k_stamps;      // [g_f4k_nstamps][4]: entry, first row, end, XCC_ID << 32 | HW_ID
__device__ unsigned g_f4k_nstamps;
#define F4K_STAMP(slot) do { if (threadIdx.x == 0 && blockIdx.x < g_f4k_nstamps) g_f4k_stamps[4ul * blockIdx.x + (slot)] = (unsigned long long)wall_clock64(); } while (0)
#else
#define F4K_STAMP(slot) do { } while (0)
#endif
struct F4kMap {
  int E, D, nchunk;      // epochs, Doppler bins, item chunks per (epoch, bin)
  int run;               // work items per workgroup, >= 1
  int by_epoch;          // 1: all work of epoch e on XCD e % 8, a run stays inside its epoch; 0: (epoch, bin) units dealt round-robin, a
                         // run walks the units of its own XCD
  int nruns;             // runs per epoch (by_epoch) or per XCD
  int claim;             // 1: persistent workgroups take their work items from eight counters, one queue per XCD (below)
  unsigned grid;
};
struct F4kPos {
  unsigned e, d, c;      // epoch, Doppler bin, item chunk
  int left;              // work items of the run still to do, this one included; <= 0: none
};

// run = 0 picks the fewest runs that still leave four rounds of resident workgroups (4 per CU) and cuts them to equal lengths; any
// run is capped at the work items of one epoch
__host__ __device__ inline F4kMap f4k_map(int E, int D, int nchunk, int run, int cus) {
  F4kMap m;
  m.E = E; m.D = D; m.nchunk = nchunk;
  m.claim = 0;
  m.by_epoch = E >= 64 ? 1 : 0;
  const long per_epoch = (long)D * nchunk;
  const long span = m.by_epoch ? per_epoch : (((long)E * D + 7) / 8) * nchunk;      // work items a run index counts through
  const long groups = m.by_epoch ? 8L * ((E + 7) / 8) : 8;                         // ... and how many such spans the grid has
  const long cap = per_epoch < span ? per_epoch : span;
  long u = run;
  if (u <= 0) {
    u = 1;
    const long want = 16L * cus;
    for (long k = cap; k > 1; k--)
      if (groups * ((span + k - 1) / k) >= want) { u = k; break; }
    const long nruns = (span + u - 1) / u;
    u = (span + nruns - 1) / nruns;      // the same number of runs, of as equal lengths as they come (40 work items: 4 x 10, not 3 x 13 + 1)
  }
  if (u > cap) u = cap;
  m.run = (int)u;
  m.nruns = (int)((span + u - 1) / u);
  m.grid = (unsigned)(groups * m.nruns);
  return m;
}

// first work item of workgroup `block`
__host__ __device__ inline F4kPos f4k_first(const F4kMap& m, unsigned block) {
  F4kPos p;
  const unsigned xcd = block & 7, j = block >> 3;      // workgroup b runs on XCD b % 8
  const unsigned w0 = (j % (unsigned)m.nruns) * (unsigned)m.run;
  p.c = w0 % (unsigned)m.nchunk;
  if (m.by_epoch) {
    p.e = (j / (unsigned)m.nruns) * 8 + xcd;
    p.d = w0 / (unsigned)m.nchunk;
    const int span = m.D * m.nchunk;
    p.left = p.e < (unsigned)m.E ? (m.run < span - (int)w0 ? m.run : span - (int)w0) : 0;
  } else {
    const unsigned units = (unsigned)m.E * (unsigned)m.D;
    const unsigned u = (w0 / (unsigned)m.nchunk) * 8 + xcd;
    p.e = u / (unsigned)m.D;
    p.d = u % (unsigned)m.D;
    const int span = (int)((units + 7) / 8) * m.nchunk;
    p.left = u < units ? (m.run < span - (int)w0 ? m.run : span - (int)w0) : 0;
  }
  return p;
}

// the run's next work item (no division)
__host__ __device__ inline void f4k_next(const F4kMap& m, F4kPos& p) {
  p.left--;
  if (++p.c < (unsigned)m.nchunk) return;
  p.c = 0;
  if (m.by_epoch) { p.d++; return; }
  p.d += 8;
  while (p.d >= (unsigned)m.D) { p.d -= (unsigned)m.D; p.e++; }
  if (p.e >= (unsigned)m.E) p.left = 0;      // the XCD's last units do not exist when E x D is no multiple of 8
}

// Claimed work.  The grid is one workgroup per resident slot (4 per CU) and stays for the whole launch; the work items are eight queues,
// queue q = the work the static map gives to the blocks with b % 8 == q (so a queue's epochs still meet in one L2), in the static map's
// order.  Workgroup b starts with item b / 8 of queue b % 8 and then takes the next unclaimed one with an atomic add on the queue's
// counter (the host sets the counters to grid / 8 before the launch); when its queue is empty it takes from the next queue, and so on
// round the eight: an XCD that runs a few per cent faster than another (they do) helps out instead of standing idle at the end.  The
// set-up is paid once per workgroup as in a run, but a workgroup that is slow takes fewer items, so no slot waits for another at the
// end of the launch for longer than one work item -- what a fixed run longer than 1 loses.
__host__ __device__ inline unsigned f4k_queue_len(const F4kMap& m, unsigned q) {
  const unsigned heads = m.by_epoch ? (unsigned)m.E : (unsigned)m.E * (unsigned)m.D;      // epochs or units, dealt round the queues
  const unsigned per_head = m.by_epoch ? (unsigned)m.D * (unsigned)m.nchunk : (unsigned)m.nchunk;
  return q < heads ? ((heads - q + 7) / 8) * per_head : 0;
}
// item w of queue q
__host__ __device__ inline F4kPos f4k_item(const F4kMap& m, unsigned q, unsigned w) {
  F4kPos p;
  p.left = 1;
  p.c = w % (unsigned)m.nchunk;
  const unsigned r = w / (unsigned)m.nchunk;
  if (m.by_epoch) {
    p.e = (r / (unsigned)m.D) * 8 + q;
    p.d = r % (unsigned)m.D;
  } else {
    const unsigned u = r * 8 + q;
    p.e = u / (unsigned)m.D;
    p.d = u % (unsigned)m.D;
  }
  return p;
}
constexpr int kF4kCntPitch = 16;      // dwords between two queue counters: one 64-byte line each
// Option f4k_claim: 0 = the static map; 1 = claimed work with one workgroup per resident slot (4 per CU) when the longest queue has
// more work items than that gives it workgroups, else the static map (which is then the same thing); n > 1 = claimed work with n
// workgroups (rounded up to a multiple of 8), whatever the shape -- tests and sweeps.  True: claimed work, map.grid is its grid.
inline bool f4k_claim_grid(F4kMap& m, long claim, int cus) {
  if (claim <= 0) return false;
  const unsigned per_queue = claim == 1 ? (unsigned)(4 * cus) / 8 : (unsigned)((claim + 7) / 8);
  if (per_queue == 0 || (claim == 1 && f4k_queue_len(m, 0) <= per_queue)) return false;
  m.claim = 1;
  m.grid = 8 * per_queue;
  return true;
}
// One lane takes the next unclaimed work item, from queue (q0 + q_off) % 8 on; q_off counts the queues it has found empty.  q_out = 8: none.
__device__ __forceinline__ void f4k_claim(unsigned* cnt, const F4kMap& m, unsigned q0, unsigned& q_off, unsigned& q_out, unsigned& w_out) {
  q_out = 8;
  w_out = 0;
  for (; q_off < 8; q_off++) {
    const unsigned q = (q0 + q_off) & 7, len = f4k_queue_len(m, q);
    if (len <= gridDim.x / 8) continue;      // nothing beyond its workgroups' first items
    const unsigned w = atomicAdd(cnt + q * kF4kCntPitch, 1u);
    if (w < len) { q_out = q; w_out = w; return; }
  }
}

__global__ __launch_bounds__(kBlock, 4) void lds_fused4k_kernel(const float2* __restrict__ x, size_t epoch_stride,
                                                                const float2* __restrict__ C, const int* __restrict__ items,
                                                                const double* __restrict__ freq, const float2* __restrict__ nco_tab,
                                                                const float2* __restrict__ tw, RowRec* __restrict__ rows, F4kMap map, int P,
                                                                int pch, float tie_scale, unsigned* __restrict__ cnt) {
  constexpr int kRing = 32;                           // item slots between two flushes: a power of two, at most 64 (one lane each)
  static_assert(kRing >= 1 && kRing <= 64 && (kRing & (kRing - 1)) == 0, "kRing");
  __shared__ v2 lds[kLdsElems];
  __shared__ float s_rpeak[kRing][kBlock / 64];
  __shared__ int s_ridx[kRing][kBlock / 64];
  __shared__ float s_rsum[kRing][kBlock / 64];
  const int t = threadIdx.x;
  // Placement (workgroup b runs on XCD b % 8).  Batches: all D x nchunk workgroups of an epoch go to XCD e % 8, so the epoch's
  // sample block is fetched into one L2 instead of eight (round 2: 8.3 x the compulsory fetch).  Few epochs: (epoch, Doppler)
  // units are dealt round-robin as in lds_correlate_kernel, so that a single-epoch search still fills all eight XCDs.
  // The map itself is f4k_first / f4k_next above.
  __shared__ unsigned s_claim[2];                     // claimed work: the workgroup's next work item (queue, index in the queue); queue 8 = none
  const unsigned q0 = blockIdx.x & 7;
  const unsigned len0 = f4k_queue_len(map, q0);
  unsigned q_off = len0 > gridDim.x / 8 ? 0 : 1;      // lane 0: queues found empty
  F4kPos pos;
  if (map.claim) {
    if ((blockIdx.x >> 3) < len0) pos = f4k_item(map, q0, blockIdx.x >> 3);
    else {                                            // fewer work items in the queue than workgroups: take from the other queues at once
      if (t == 0) {
        unsigned q, w;
        f4k_claim(cnt, map, q0, q_off, q, w);
        s_claim[0] = q;
        s_claim[1] = w;
      }
      __syncthreads();
      const unsigned q = (unsigned)__builtin_amdgcn_readfirstlane((int)s_claim[0]), w = (unsigned)__builtin_amdgcn_readfirstlane((int)s_claim[1]);
      if (q >= 8) return;
      pos = f4k_item(map, q, w);
    }
  } else {
    pos = f4k_first(map, blockIdx.x);
    if (pos.left <= 0) return;
  }
  F4K_STAMP(0);
#ifdef GACQ_F4K_STAMPS
  bool first_row = true;
  if (t == 0 && blockIdx.x < g_f4k_nstamps) {
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    g_f4k_stamps[4ul * blockIdx.x + 3] = ((unsigned long long)xcc << 32) | hw;
  }
#endif
  const int D = map.D;
  v2 wa = ld2(tw + t), wb = ld2(tw + 16 * (t & 15));
  // The pass-2 twiddle powers of the inverse transform, conj(W_256^c)^k for the 16 lane classes
  // c = t & 15, are built once per workgroup with the product tree of apply_powers (same values, so the records stay
  // bit-identical to the two-kernel path) and read back from a 1.9 KB LDS table: one ds_read_b64 per product instead of 14
  // extra complex products per row.  (Pass 1's powers are per-lane and stay in registers, pwa below.)
  __shared__ v2 s_tw2[15 * 16];
  if (t < 16) {
    v2 pw[15];
    make_powers(pw, v2{wb.x, -wb.y});                  // lanes 0..15: wb = W_256^t
#pragma unroll
    for (int k = 0; k < 15; k++) s_tw2[16 * k + t] = pw[k];
  }
  const unsigned lane_off = (unsigned)t * 16u;
  const float inv_n = 1.0f / (float)kLdsN;
  v2 pwa[15];
  make_powers(pwa, v2{wa.x, -wa.y});                  // conjugate: inverse transform
  for (;;) {
    // claimed work: the atomic for the next work item is issued here and its result is looked at behind the forward transform
    unsigned w_ahead = 0;
    if (map.claim && t == 0 && q_off == 0) w_ahead = atomicAdd(cnt + q0 * kF4kCntPitch, 1u);
    const long e = pos.e;
    const int d = (int)pos.d;
    const int p0 = (int)pos.c * pch;
    const int p1 = min(P, p0 + pch);
    v2 xr[kR];
    {
      const double f = freq[d];
      const float2* src = x + e * epoch_stride;
      v2 v[kR], w[kR];
      // The sample numbers are formed again for every work item: as loop invariants the compiler carries the sixteen (double)i across
      // the run, 32 registers the item loop does not have.
      int ti = t;
      asm volatile("" : "+v"(ti));
#pragma unroll
      for (int jj = 0; jj < kR; jj++) {
        const int i = ti + 256 * jj;
        const int k = nco_index(f, i);                  // gnsstools/nco.py:6-9
        v[jj] = ld2(src + i);
        w[jj] = ld2(nco_tab + k);
      }
#pragma unroll
      for (int jj = 0; jj < kR; jj++) v[jj] = cmul(v[jj], w[jj]);
      fft4096<false, false, false, true>(v, lds, wa, wb, s_tw2 + (t & 15), &pwa);
#pragma unroll
      for (int jj = 0; jj < kR; jj++) { const v2 a = v[rev16(jj)]; xr[jj] = v2{a.x, -a.y}; }      // np.conj(fft.fft(b))  acquire-gps-l1.py:32
      if (map.claim && t == 0) {
        unsigned q = q0, w = w_ahead;
        if (q_off != 0 || w >= len0) {                  // own queue empty: the others, one atomic each (only at the end of the launch)
          if (q_off == 0) q_off = 1;
          f4k_claim(cnt, map, q0, q_off, q, w);
        }
        s_claim[0] = q;                                 // read behind the item loop; written again only behind the next transform's barriers
        s_claim[1] = w;
      }
      __syncthreads();                                  // the forward transform's exchange-2 reads are complete
    }
#ifdef GACQ_F4K_STAMPS
    if (first_row) { F4K_STAMP(1); first_row = false; }
#endif
    for (int p = p0; p < p1; p++) {
      F4K_PRIO(GACQ_F4K_P4);
      // No row reads wb any more (pass 2 takes its powers from s_tw2).  The empty statement stays because it pins wb's two registers
      // through the loop, and the register assignment of the whole kernel -- the one every measurement above was made with -- depends on
      // it: without it the kernel compiles to other instructions (tools/isa_diff.py).
      asm volatile("" : "+v"(wb.x), "+v"(wb.y));
      v2 v[kR];
      // (The item number one row ahead -- its scalar load off the row's critical path -- measured no different: 5.29-5.32 against
      // 5.29-5.32 ms, profiles/r17_fused4k_claimed_work_ab.log.  Not built in.)
      const __amdgpu_buffer_rsrc_t cres = row_rsrc(C + (long)items[p] * kLdsN);
#pragma unroll
      for (int jp = 0; jp < kR / 2; jp++) ld_pair(cres, lane_off, jp, v[2 * jp], v[2 * jp + 1]);
#pragma unroll
      for (int jj = 0; jj < kR; jj++) v[jj] = cmul(v[jj], xr[jj]);
      // lane t holds lags t + 256 k.  The 1/N of ifft is a power of two: applied once to the reduced values.
      float m[kR];
      // Epilogue: the transform's last layer delivers (re, re) / (im, im) pairs of lags k and k + 8, so that two
      // squared magnitudes cost one v_pk_mul_f32 + one v_pk_fma_f32 (norm2's two roundings each) instead of two v_mul_f32 + two
      // v_fmac_f32; m[k] is still lag t + 256 k (a renaming).  The sum over k stays the sequential chain, and the wave reductions
      // combine the four rows on DPP too.  Every value is the same bits as with the (re, im) epilogue it replaced.  23 VALU
      // instructions a row less (439 -> 416, SQ_INSTS_VALU agrees); headline step 1.012 x in the medians, every run above every run of the loop before it on two
      // boxes (profiles/r15_fused4k_epilogue_ab.log).
      v2 pl[kR];
      fft4096<true, true, true>(v, lds, wa, wb, s_tw2 + (t & 15), &pwa, &pl);
#pragma unroll
      for (int k = 0; k < kR / 2; k++) {
        const v2 q = norm2_planar(pl[k], pl[k + kR / 2]);
        m[k] = __builtin_amdgcn_sqrtf(q.x);                           // np.absolute(ifft(...)) * N
        m[k + kR / 2] = __builtin_amdgcn_sqrtf(q.y);
      }
      float sum_f = m[0];
#pragma unroll
      for (int k = 1; k < kR; k++) sum_f += m[k];
      float wmaxf;
      unsigned widx;
      wave_first_max<kR, wave_max_u32_bcast>(m, (unsigned)__builtin_amdgcn_readfirstlane(t & ~63), 1u, 256u, tie_scale, wmaxf, widx);
      const float wsum = wave_add_f32_bcast(sum_f * inv_n);
      const unsigned wmax = __builtin_bit_cast(unsigned, wmaxf * inv_n);
      const int slot = (p - p0) & (kRing - 1);
      if ((t & 63) == 0) { s_rpeak[slot][t >> 6] = __builtin_bit_cast(float, wmax); s_ridx[slot][t >> 6] = (int)widx; s_rsum[slot][t >> 6] = wsum; }
      lds_barrier();     // also orders this item's exchange-2 reads before the next item's exchange-1 writes
      if ((slot == kRing - 1 || p == p1 - 1) && t <= slot) {
        RowRec r;
        combine_tagged(kBlock / 64, [&](int w) { return s_rpeak[t][w]; }, [&](int w) { return s_ridx[t][w]; }, tie_scale, r.peak, r.idx);
        r.sum = (((double)s_rsum[t][0] + (double)s_rsum[t][1]) + (double)s_rsum[t][2]) + (double)s_rsum[t][3];
        rows[(e * P + (p - slot + t)) * (long)D + d] = r;
      }
    }
    if (map.claim) {
      const unsigned q = (unsigned)__builtin_amdgcn_readfirstlane((int)s_claim[0]), w = (unsigned)__builtin_amdgcn_readfirstlane((int)s_claim[1]);
      if (q >= 8) break;
      pos = f4k_item(map, q, w);
    } else {
      f4k_next(map, pos);
      if (pos.left <= 0) break;
    }
  }
  F4K_STAMP(2);
}

int twiddle_table(gacq_ctx* ctx, const float2** out) { return twiddle_cache(ctx, "W4096", kLdsN, kLdsN, out); }

}  // namespace

namespace gacq {

// N = 16384: the radix-32 form (gacq_lds16k.hip) or the radix-16 one (gacq_lds16k_r16.hip), as plan_search (gacq_engine.hip) picks
bool lds_supported(int N) { return N == kLdsN || N == 16384; }

// code spectra straight from the (complex, zero-extended) replica rows with the engine's own forward transform: no rocFFT plan
int lds_code_spectra(gacq_ctx* ctx, const float2* replica_rows, float2* perm, int nprn) {
  const float2* tw;
  int rc = twiddle_table(ctx, &tw);
  if (rc != GACQ_OK) return rc;
  hipLaunchKernelGGL((lds_forward_kernel<false, true>), dim3((unsigned)nprn), dim3(kBlock), 0, ctx->stream, replica_rows, (size_t)kLdsN, perm,
                     (const double*)nullptr, (const float2*)nullptr, tw, kLdsN, 1, 1);
  GACQ_HIP(ctx, hipGetLastError());
  return GACQ_OK;
}

int lds_forward(gacq_ctx* ctx, const float2* x, size_t nsamp, int nepoch, int n, const double* d_freq, int FD,
                int B, const float2* tab, float2* X) {
  const float2* tw;
  int rc = twiddle_table(ctx, &tw);
  if (rc != GACQ_OK) return rc;
  const long rows = (long)nepoch * FD * B;
  hipLaunchKernelGGL(lds_forward_kernel<false>, dim3((unsigned)rows), dim3(kBlock), 0, ctx->stream, x, nsamp, X, d_freq, tab, tw, n, FD, B);
  GACQ_HIP(ctx, hipGetLastError());
  return GACQ_OK;
}

int lds_fused4k_search(gacq_ctx* ctx, const float2* x, size_t nsamp, int nepoch, const float2* spectra, const int* d_items,
                       const double* d_freq, const float2* tab, int nitems, int D, RowRec* rows, float tie_scale) {
  const float2* tw;
  int rc = twiddle_table(ctx, &tw);
  if (rc != GACQ_OK) return rc;
  const long units = (long)nepoch * D;
  // one forward transform per workgroup: amortise it over up to 32 items while >= ~2048 workgroups remain
  int pch = 8;
  while (pch < 32 && units * ((nitems + 2 * pch - 1) / (2 * pch)) >= 2048) pch *= 2;
  if (ctx->opt[GACQ_OPT_LDS_PCH] >= 1) pch = (int)ctx->opt[GACQ_OPT_LDS_PCH];
  pch = std::min(pch, nitems);
  const int nchunk = (nitems + pch - 1) / pch;
  if (ctx->cu_count <= 0) {
    int cus = 0;
    ctx->cu_count = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) == hipSuccess && cus > 0 ? cus : 256;
  }
  F4kMap map = f4k_map(nepoch, D, nchunk, (int)ctx->opt[GACQ_OPT_F4K_RUN], ctx->cu_count);
  unsigned* cnt = nullptr;
  if (f4k_claim_grid(map, ctx->opt[GACQ_OPT_F4K_CLAIM], ctx->cu_count)) {
    if ((rc = ensure(ctx, ctx->f4k_cnt, sizeof(unsigned) * 8 * kF4kCntPitch)) != GACQ_OK) return rc;
    cnt = (unsigned*)ctx->f4k_cnt.p;
    GACQ_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)cnt, (int)(map.grid / 8), 8 * kF4kCntPitch, ctx->stream));      // items 0 .. grid / 8 - 1 of a queue are its workgroups' first ones
  }
  hipLaunchKernelGGL(lds_fused4k_kernel, dim3(map.grid), dim3(kBlock), 0, ctx->stream, x, nsamp, spectra, d_items, d_freq, tab, tw, rows,
                     map, nitems, pch, tie_scale, cnt);
  GACQ_HIP(ctx, hipGetLastError());
  return GACQ_OK;
}

#ifdef GACQ_F4K_STAMPS
extern "C" int gacq_debug_f4k_stamps(void* d_stamps, unsigned nblocks) {
  unsigned long long* p = (unsigned long long*)d_stamps;
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_f4k_stamps), &p, sizeof(p)) != hipSuccess || hipMemcpyToSymbol(HIP_SYMBOL(g_f4k_nstamps), &nblocks, sizeof(nblocks)) != hipSuccess)
    return GACQ_ERR_HIP;
  return GACQ_OK;
}
#endif

// test hook (gacq_debug_f4k_map with run < 0): the queues of claimed work, every queue walked in its order
long lds_debug_f4k_queues(int nepoch, int D, int nchunk, long claim, int cus, int* info, int* work, long cap) {
  F4kMap map = f4k_map(nepoch, D, nchunk, 1, cus);
  const bool on = f4k_claim_grid(map, claim, cus);
  if (info) { info[0] = on ? 1 : 0; info[1] = map.by_epoch; info[2] = 0; info[3] = (int)map.grid; }
  long n = 0;
  for (unsigned q = 0; q < 8; q++)
    for (unsigned w = 0; w < f4k_queue_len(map, q); w++, n++) {
      const F4kPos pos = f4k_item(map, q, w);
      if (work && n < cap) { work[4 * n] = (int)q; work[4 * n + 1] = (int)pos.e; work[4 * n + 2] = (int)pos.d; work[4 * n + 3] = (int)pos.c; }
    }
  return n;
}

// test hook (gacq_debug_f4k_map): the walk of every workgroup of the grid a search of this shape would launch, on the host, with the
// functions the kernel walks with
long lds_debug_f4k_map(int nepoch, int D, int nchunk, int run, int cus, int* info, int* work, long cap) {
  const F4kMap map = f4k_map(nepoch, D, nchunk, run, cus);
  if (info) { info[0] = map.run; info[1] = map.by_epoch; info[2] = map.nruns; info[3] = (int)map.grid; }
  long n = 0;
  for (unsigned b = 0; b < map.grid; b++)
    for (F4kPos pos = f4k_first(map, b); pos.left > 0; f4k_next(map, pos), n++)
      if (work && n < cap) { work[4 * n] = (int)b; work[4 * n + 1] = (int)pos.e; work[4 * n + 2] = (int)pos.d; work[4 * n + 3] = (int)pos.c; }
  return n;
}

int lds_debug_nco(gacq_ctx* ctx, int n, const double* d_freq, int* d_idx) {
  hipLaunchKernelGGL(lds_forward_kernel<true>, dim3(1), dim3(kBlock), 0, ctx->stream, (const float2*)nullptr, (size_t)0, (float2*)d_idx, d_freq,
                     (const float2*)nullptr, (const float2*)nullptr, n, 1, 1);
  GACQ_HIP(ctx, hipGetLastError());
  return GACQ_OK;
}

int lds_correlate(gacq_ctx* ctx, const float2* X, const float2* spectra, const int* d_items, const int* d_fset, int nepoch,
                  int nitems, int F, int D, int B, RowRec* rows, float tie_scale, float* q_out) {
  if (q_out && (nepoch != 1 || nitems != 1 || D != 1)) return set_error(ctx, GACQ_ERR_BAD_ARG, "LDS FFT engine: a row dump takes exactly one row");
  const float2* tw;
  int rc = twiddle_table(ctx, &tw);
  if (rc != GACQ_OK) return rc;
  // items per workgroup: keep >= ~2048 workgroups in flight (256 CUs x 4 resident x 2), at most 8 per group
  const long rows_total = (long)nepoch * nitems * D;
  int pch = (int)std::max<long>(1, std::min<long>(8, rows_total / 2048));
  // B > 1: nothing is shared between a workgroup's items (every item walks the unit's B forward-spectrum rows again), but the
  // workgroups of a unit that run side by side on its XCD walk them TOGETHER and share them in that L2: as few items per workgroup as
  // still give it ~8 rows (B = 10, 800 units: 8 -> 1 item per workgroup 1.32 -> 1.23 ms; B = 80: 1 item 0.92 ms, 8 items 1.56 ms --
  // profiles/r05_engine3_writer_wave_priority_sweep.log)
  if (!(B == 1 && F == 1)) pch = std::min(pch, std::max(1, (8 + B - 1) / B));
  if (ctx->opt[GACQ_OPT_LDS_PCH] >= 1) pch = (int)ctx->opt[GACQ_OPT_LDS_PCH];
  pch = std::min(pch, nitems);
  const int nchunk = (nitems + pch - 1) / pch;
  const long units8 = ((long)nepoch * D + 7) / 8;
  const long grid = 8 * units8 * nchunk;
  // register-cached X needs all items of a workgroup to share one forward set
  const bool b1 = (B == 1) && (F == 1);
  auto kern = q_out ? (b1 ? lds_correlate_kernel<true, true> : lds_correlate_kernel<false, true>)
                    : (b1 ? lds_correlate_kernel<true> : lds_correlate_kernel<false>);
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kBlock), 0, ctx->stream, X, spectra, d_items, d_fset, tw, rows, nepoch,
                     nitems, F, D, B, pch, nchunk, tie_scale, q_out);
  GACQ_HIP(ctx, hipGetLastError());
  return GACQ_OK;
}

// ---- inner stages of the split engine (N = R*4096) -------------------------------------------------------
namespace {
// W_N^m for m < 256 R
int big_twiddles(gacq_ctx* ctx, int N, int R, const float2** out) {
  return twiddle_cache(ctx, "WN_lo_" + std::to_string(N), N, 256 * R, out);
}
}  // namespace

int lds_inner_forward(gacq_ctx* ctx, float2* rows, long nrows, bool conj) {
  const float2* tw;
  int rc = twiddle_table(ctx, &tw);
  if (rc != GACQ_OK) return rc;
  if (conj) hipLaunchKernelGGL(lds_inner_forward_kernel<true>, dim3((unsigned)nrows), dim3(kBlock), 0, ctx->stream, rows, tw);
  else hipLaunchKernelGGL(lds_inner_forward_kernel<false>, dim3((unsigned)nrows), dim3(kBlock), 0, ctx->stream, rows, tw);
  GACQ_HIP(ctx, hipGetLastError());
  return GACQ_OK;
}

int lds_inner_correlate(gacq_ctx* ctx, const float2* X, const float2* spectra, const int* d_items, const int* d_fset, long g0,
                        long ng, int P, int F, int D, int B, int R, int N, float2* Z) {
  const float2 *tw, *twn;
  int rc = twiddle_table(ctx, &tw);
  if (rc != GACQ_OK) return rc;
  if ((rc = big_twiddles(ctx, N, R, &twn)) != GACQ_OK) return rc;
  // (epoch, item) rows touched by this pass, cut into chunks of pch per workgroup; >= ~2048 workgroups, <= 8 items each
  const long ep_first = g0 / D, ep_last = (g0 + ng - 1) / D;
  const long nep = ep_last - ep_first + 1;
  int pch = (int)std::max<long>(1, std::min<long>(8, nep * D * B * R / 2048));
  if (ctx->opt[GACQ_OPT_SPLIT_PCH] >= 1) pch = (int)ctx->opt[GACQ_OPT_SPLIT_PCH];
  const int nblk_ep = (int)((nep + pch - 1) / pch);
  hipLaunchKernelGGL(lds_inner_correlate_kernel, dim3((unsigned)((long)R * nblk_ep * D * B)), dim3(kBlock), 0, ctx->stream, X, spectra,
                     d_items, d_fset, tw, twn, Z, g0, ng, ep_first, nblk_ep, pch, P, F, D, B, R);
  GACQ_HIP(ctx, hipGetLastError());
  return GACQ_OK;
}

}  // namespace gacq
