// Engine 5: complex128 verification pipeline (hard part 1: "keep a complex128 build").
//
// The product engines compute in complex64; the reference computes in complex128 (numpy / scipy.fftpack).  This engine is the
// north-star pipeline K1 -> FFT -> K2 -> IFFT -> K3 -> K4 with every value in fp64 on the device (fp64 NCO table, transforms,
// magnitudes and metric), so it agrees with the reference to ~1e-12 instead of ~1e-7.  It exists to bisect: when an fp32 engine
// and the oracle disagree on a near-tied peak, engine 5 says which side the rounding fell on.  Selected only by
// gacq_set_engine(ctx, 5), never by auto.  plan_search (gacq_engine.hip) picks one of five forms, verify_search runs them all on
// one host path:
//   C128Fused4k  N = 4096, B = 1, one carrier: the whole search row in one kernel (fused4k_c128_kernel)
//   C128Lds4k    N = 4096 otherwise: a forward and a correlate kernel on the LDS-resident transform (c128_4k_*_kernel)
//   C128Split    N = 4 x 4096 / 16 x 4096: outer DFT-R around the resident transform, one Z' round trip (c128_split_*_kernel)
//   C128R31      N = 31 x M (61380, 30690): fp64 DFT-31 stages around rocFFT's native length-M transforms (c128_r31_*_kernel)
//   C128Rocfft   every other length, row dumps of N = 4096 and GACQ_OPT_FUSED_C128 = 0: the five-stage pipeline on rocFFT's
//                double-precision transforms, the cross-check of the other four
#include "gacq_common.h"
#define GACQ_F64_UNPAIR 1      // fused4k_c128_kernel: no AGPR spills (244 VGPRs), see gacq_fft64.h
#include "gacq_fft64.h"

#include <cmath>

using namespace gacq;
using f64::ldc;
using f64::RowRec64;
using f64::stc;

namespace {

// K1: y = x * tab64[floor((f*i)*1024) & 1023]   (acquire-gps-l1.py:28,30-31, gnsstools/nco.py:6-10), samples widened to fp64
__global__ __launch_bounds__(kBlock) void mix64_kernel(XSrc x, size_t epoch_stride, double2* __restrict__ y,
                                                        const double* __restrict__ freq, const double2* __restrict__ tab, int n, int span,
                                                        int FD, int B, unsigned cols) {
  const unsigned row = blockIdx.x / cols;           // ((e*FD + fd)*B + b)
  const int b = (int)(row % (unsigned)B);
  const unsigned t = row / (unsigned)B;
  const int fd = (int)(t % (unsigned)FD);
  const long e = t / (unsigned)FD;
  const double f = freq[fd];
  const int i = (int)(blockIdx.x % cols) * kBlock + threadIdx.x;
  if (i >= span) return;
  const double2 s = ld_x(x, e * epoch_stride + (size_t)b * n + i);
  const double2 w = tab[nco_index(f, i)];
  y[row * (long)span + i] = make_double2(s.x * w.x - s.y * w.y, s.x * w.y + s.y * w.x);
}

// K2: Y = C_p * conj(X)   (acquire-gps-l1.py:32)
__global__ __launch_bounds__(kBlock) void conj_mul64_kernel(const double2* __restrict__ X, const double2* __restrict__ C, double2* __restrict__ Y,
                                                             const int* __restrict__ items, const int* __restrict__ fset, long g0, int P, int F,
                                                             int D, int B, int N, unsigned cols) {
  const unsigned ry = blockIdx.x / cols;
  const int b = (int)(ry % (unsigned)B);
  const unsigned g = (unsigned)g0 + ry / (unsigned)B;
  const int d = (int)(g % (unsigned)D);
  const unsigned ep = g / (unsigned)D;
  const int p = (int)(ep % (unsigned)P);
  const long e = ep / (unsigned)P;
  const int i = (int)(blockIdx.x % cols) * kBlock + threadIdx.x;
  if (i >= N) return;
  const double2 xv = X[(((e * F + fset[p]) * D + d) * (long)B + b) * (long)N + i];
  const double2 cv = C[(long)items[p] * N + i];
  Y[ry * (long)N + i] = make_double2(cv.x * xv.x + cv.y * xv.y, cv.y * xv.x - cv.x * xv.y);
}

// K3: q[k] = sum_b |Y_b[k] / N| in fp64 (the reference's ifft carries the 1/N, then np.absolute, then the sum over blocks)
__global__ __launch_bounds__(kBlock) void mag_peak64_kernel(const double2* __restrict__ Y, RowRec64* __restrict__ rows, long g0, int B, int N,
                                                             float* __restrict__ q_out) {
  const long gl = blockIdx.x;
  const double2* ys = Y + gl * (long)B * N;
  const double inv_n = 1.0 / (double)N;
  f64::tree_reduce_row<kBlock, 1>(N, [&](int k) {
    double q = 0.0;
    for (int b = 0; b < B; b++) {
      const double2 v = ys[(long)b * N + k];
      q += hypot(v.x * inv_n, v.y * inv_n);
    }
    if (q_out) q_out[k] = (float)q;
    return q;
  }, rows + g0 + gl);
}

// K4: the Doppler scan of one (epoch, item) per thread
__global__ void best_doppler64_kernel(const RowRec64* __restrict__ rows, gacq_peak* __restrict__ out, long nep, int D, int N, int normalised) {
  const long ep = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (ep >= nep) return;
  gacq_peak o;
  f64::doppler_scan(rows + ep * D, D, N, normalised, [](int d) { return d; }, o.metric, o.idx, o.d_index);
  out[ep] = o;
}

// ---- N = 4096, one block, one carrier: the whole row in one workgroup, complex128 ---------------------------------------------------
// The structure of lds_fused4k_kernel (gacq_ldsfft.hip) in the reference's arithmetic type: workgroup = (epoch, Doppler bin, chunk of
// pch items); prologue: x window, table-NCO mix, forward transform, conjugate -- the spectrum stays in registers (the transform's
// output convention is the inverse transform's input convention); then per item C_p * conj(X), inverse transform, |.| / N and the
// (max, first argmax, sum) of the row.  Nothing but x, the complex128 code spectra (natural order: lane t reads C[t + 256 j], 16
// bytes per lane, 1 KiB per wave and instruction) and one 24-byte record per row touches HBM; the rocFFT pipeline this replaces
// moves 5 x 64 KB per row.  64 KB of LDS per workgroup (gacq_fft64.h) -> two workgroups per CU, <= 256 VGPRs.
#ifndef GACQ_C128_PRIO
#define GACQ_C128_PRIO true      // rising wave priorities (gacq_fft64.h F64_PRIO): 13.67 -> 12.88 ms per 1024-epoch step, profiles/r05_headline_kernel_wave_priority_sweep.log
#endif
__global__ __launch_bounds__(kBlock, 2) void fused4k_c128_kernel(XSrc x, size_t epoch_stride, const double2* __restrict__ C,
                                                                 const int* __restrict__ items, const double* __restrict__ freq,
                                                                 const double2* __restrict__ tab, const double2* __restrict__ tw,
                                                                 RowRec64* __restrict__ rows, int E, int P, int D, int pch, int nchunk) {
  using namespace gacq::f64;
  extern __shared__ __attribute__((aligned(16))) double lds64[];
  const int t = threadIdx.x;
  // placement as in lds_fused4k_kernel: all workgroups of an epoch run on XCD e % 8 (the sample block is fetched into one L2)
  const int xcd = blockIdx.x & 7;
  const unsigned j8 = blockIdx.x >> 3;
  const unsigned per_epoch = (unsigned)D * (unsigned)nchunk;
  const unsigned e8 = (j8 / per_epoch) * 8 + xcd;
  if (e8 >= (unsigned)E) return;
  const long e = e8;
  const int d = (int)((j8 % per_epoch) / (unsigned)nchunk);
  const int p0 = (int)(j8 % (unsigned)nchunk) * pch;
  const int p1 = min(P, p0 + pch);
  const double2 wa2 = tw[t], wb2 = tw[16 * (t & 15)];
  const cd wa = {wa2.x, wa2.y}, wb = {wb2.x, wb2.y};
  // pass-2 twiddle powers of the inverse transform, conj(W_256^c)^k for the 16 lane classes c = t & 15: built once per workgroup,
  // read back from a 3.8 KB LDS table in the item loop (the trick of lds_fused4k_kernel)
  __shared__ cd s_tw2[15 * 16];
  build_tw2(s_tw2, conj(wb), t);                          // lanes 0..15: wb = W_256^t
  cd xr[16];
  {
    const double f = freq[d];
    const XSrc src = x.offset(e * epoch_stride);
    cd v[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const int i = t + 256 * j;
      const double2 sv = ld_x(src, i);
      const double2 w = tab[nco_index(f, i)];                     // gnsstools/nco.py:6-10
      v[j] = cd{sv.x, sv.y} * cd{w.x, w.y};
    }
    fft4096<false>(v, lds64, wa, wb, t);
#pragma unroll
    for (int j = 0; j < 16; j++) xr[j] = conj(v[rev16(j)]);      // np.conj(fft.fft(b))  acquire-gps-l1.py:32
    __syncthreads();
  }
  const double inv_n = 1.0 / (double)kN;
  for (int p = p0; p < p1; p++) {
    const double2* cp = C + (long)items[p] * kN + t;
    if (GACQ_C128_PRIO) asm volatile("s_setprio 0" ::: "memory");
    cd v[16];
#pragma unroll
    for (int j = 0; j < 16; j++) { const double2 c = cp[256 * j]; v[j] = cd{c.x, c.y}; }
#pragma unroll
    for (int j = 0; j < 16; j++) v[j] = v[j] * xr[j];
    fft4096<true, true, GACQ_C128_PRIO>(v, lds64, wa, wb, t, s_tw2 + (t & 15));
    double m[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {                                // lane t holds lags t + 256 k, ascending in k
      const cd r = v[rev16(k)];
      m[k] = sqrt_pos(r.x * r.x + r.y * r.y) * inv_n;             // np.absolute(ifft(...)); 1/N is a power of two
    }
    RowMax row = wave_reduce_lags256(m, t);
    row.block_reduce<kBlock / 64>();      // its barrier also orders this item's exchange-2 reads before the next item's exchange-1 writes
    if (t == 0) rows[(e * P + p) * (long)D + d] = row.rec();
    // no barrier here: the scratch is rewritten only after the next item's transform, whose first exchange barrier thread 0 reaches
    // after it has finished reading it
  }
}

// ---- N = R x 4096 (R = 4: BeiDou B1I / B2I, GLONASS L1 / L2; R = 16: Galileo E1B / E1C) in complex128: the split of engine 4 ----------
// n = 4096 n1 + n2, k = k1 + R k2 (the split of gacq_split.hip and of the re-evaluation's tie_recheck_split_kernel, whose arithmetic this
// follows step by step), with every 4096-point transform on the LDS-resident complex128 transform of gacq_fft64.h:
//   forward   (one workgroup per (forward row, k1), shared by all items):  A[k1][n2] = W_N^{n2 k1} sum_n1 x[4096 n1 + n2] nco[.] W_R^{n1 k1},
//             X[k1][k2] = FFT_4096(A[k1])                                         -> Xs, 16 N bytes per forward row
//   writer    (per correlation row, block, k1):  T = FFT_4096(conj(C_p[k1][.]) X[k1][.]);  Z'[k1][n2] = W_N^{n2 k1} T[n2]   (|ifft(Y)| =
//             |fft(conj Y)| / N: both transforms of the chain are forward ones)     -> Z', 16 N bytes per row and block
//   reader    (per correlation row):  DFT_R over k1 for every n2, |.| / N, sum over the blocks, (max, first argmax, sum)
// One Z' round trip of 32 N bytes per row and block instead of the five stage boundaries of the rocFFT pipeline (5 x 32 N), no rocFFT
// plan.  The writer keeps the forward-spectrum row in registers over the items of its chunk (one carrier for all of them) and streams
// the code-spectrum rows; Z' rows of a pass are ordered (epoch, Doppler bin, item), the records go out in the (epoch, item, Doppler bin)
// order of the Doppler scan.

// C[p][k] (natural order) -> Cs[p][k1][k2] = C[p][k1 + R k2], k2 < M
__global__ __launch_bounds__(kBlock) void c128_split_spectra_kernel(const double2* __restrict__ C, double2* __restrict__ Cs, int R, int M) {
  const long p = blockIdx.x / (unsigned)R;
  const int k1 = (int)(blockIdx.x % (unsigned)R);
  const double2* src = C + p * (long)R * M + k1;
  double2* dst = Cs + (p * R + k1) * (long)M;
  for (int k2 = threadIdx.x; k2 < M; k2 += kBlock) dst[k2] = src[(long)R * k2];
}

// y: the carrier-wiped rows of mix64_kernel (one N-sample window per forward row) -- the table-NCO index arithmetic runs once per sample
// in that streaming kernel instead of once per (sample, k1) here, where two workgroups per CU cannot hide it (GLONASS, a carrier per
// item: forward stage 6.7 -> see profiles/r06_complex128_split_engine.log)
template <int R>
__global__ __launch_bounds__(kBlock, 2) void c128_split_forward_kernel(const double2* __restrict__ y, double2* __restrict__ Xs,
                                                                       const double2* __restrict__ WN, unsigned nrows) {
  using namespace gacq::f64;
  constexpr int M = kN, N = R * kN;
  extern __shared__ __attribute__((aligned(16))) double lds64[];
  const int t = threadIdx.x;
  // the R workgroups of a forward row read the same N mixed samples: placed on ONE XCD (workgroup b runs on XCD b % 8), consecutive in
  // its dispatch order, so that the row crosses the fabric once and the other R - 1 find it in that L2 (GLONASS, a carrier per item:
  // 30 000 rows of 256 KB -- read by k1 = blockIdx % R from four XCDs they came out of HBM four times)
  const unsigned xcd = blockIdx.x & 7u, jx = blockIdx.x >> 3;
  const int k1 = (int)(jx % (unsigned)R);
  const unsigned row = (jx / (unsigned)R) * 8u + xcd;   // ((e*FD + fd)*B + b)
  if (row >= nrows) return;
  const double2* src = y + (long)row * N + t;
  const cd wa = ldc(WN + t * R), wb = ldc(WN + 16 * (t & 15) * R);      // W_4096^t, W_256^(t & 15)
  cd v[16];
#pragma unroll
  for (int j = 0; j < 16; j++) v[j] = cd{0.0, 0.0};
  for (int n1 = 0; n1 < R; n1++) {
    cd sv[16];
#pragma unroll
    for (int j = 0; j < 16; j++) sv[j] = ldc(src + M * n1 + 256 * j);
    const cd wr = ldc(WN + ((n1 * k1) % R) * M);                       // W_R^{n1 k1}
#pragma unroll
    for (int j = 0; j < 16; j++) v[j] = v[j] + sv[j] * wr;
  }
  {
    // W_N^{n2 k1} = W_N^{t k1} x W_N^{256 j k1}: one gather per thread and 16 uniform (scalar) loads instead of 16 gathers
    const cd twb = ldc(WN + t * k1);
#pragma unroll
    for (int j = 0; j < 16; j++) v[j] = v[j] * (twb * ldc(WN + 256 * j * k1));
  }
  fft4096<false>(v, lds64, wa, wb, t);
  double2* dst = Xs + ((long)row * R + k1) * M + t;
#pragma unroll
  for (int j = 0; j < 16; j++) stc(dst + 256 * j, v[rev16(j)]);                  // X[k1 + R k2], k2 = t + 256 j
}

// grid: (units of the pass) x B x R x nchunk; unit = (epoch, Doppler bin)
template <int R>
__global__ __launch_bounds__(kBlock, 2) void c128_split_corr_kernel(const double2* __restrict__ Xs, const double2* __restrict__ Cs,
                                                                    double2* __restrict__ Z, const int* __restrict__ items,
                                                                    const int* __restrict__ fset, const double2* __restrict__ WN, long u0,
                                                                    int P, int F, int D, int B, int pch, int nchunk) {
  using namespace gacq::f64;
  constexpr int M = kN;
  extern __shared__ __attribute__((aligned(16))) double lds64[];
  const int t = threadIdx.x;
  unsigned blk = blockIdx.x;
  const int k1 = (int)(blk % (unsigned)R);
  blk /= (unsigned)R;
  const int p0 = (int)(blk % (unsigned)nchunk) * pch;
  blk /= (unsigned)nchunk;
  const int b = (int)(blk % (unsigned)B);
  const long ul = blk / (unsigned)B;                    // unit within the pass
  const long u = u0 + ul;
  const long e = u / D;
  const int d = (int)(u % D);
  const int p1 = min(P, p0 + pch);
  const cd wa = ldc(WN + t * R), wb = ldc(WN + 16 * (t & 15) * R);
  // pass-2 twiddle powers W_256^{c k} of the 16 lane classes c = t & 15 from a 3.8 KB LDS table (as in fused4k_c128_kernel): rebuilt
  // per transform they cost the registers the resident forward-spectrum row needs
  __shared__ cd s_tw2[15 * 16];
  build_tw2(s_tw2, wb, t);
  __syncthreads();
  const cd twb = ldc(WN + t * k1);
  cd xs[16];
  int have = -1;
  for (int p = p0; p < p1; p++) {
    if (fset[p] != have) {
      have = fset[p];
      const double2* xr = Xs + (((((long)e * F + have) * D + d) * B + b) * R + k1) * (long)M + t;
#pragma unroll
      for (int j = 0; j < 16; j++) xs[j] = ldc(xr + 256 * j);
    }
    const double2* cr = Cs + ((long)items[p] * R + k1) * M + t;
    cd y[16];
#pragma unroll
    for (int j = 0; j < 16; j++) y[j] = ldc(cr + 256 * j);
#pragma unroll
    for (int j = 0; j < 16; j++) y[j] = conj(y[j]) * xs[j];                      // conj(C_p * conj(X))   acquire-beidou-b1i.py:32
    if (p > p0) __syncthreads();                                                 // the previous transform's exchange-2 reads are complete
    fft4096<false, true>(y, lds64, wa, wb, t, s_tw2 + (t & 15));
    double2* zr = Z + ((((ul * P + p) * B + b) * R + k1) * (long)M) + t;
    // W_N^{n2 k1}, n2 = t + 256 j, as W_N^{t k1} (one value per thread, resident) x W_N^{256 j k1} (uniform over the workgroup: scalar
    // loads): a second complex product per output instead of 16 gathers behind the transform (two workgroups per CU hide little of a
    // dependent round trip); all 16 resident, their 64 registers push the transform into scratch
#pragma unroll
    for (int j = 0; j < 16; j++) stc(zr + 256 * j, y[rev16(j)] * (twb * ldc(WN + 256 * j * k1)));
  }
}

// one workgroup per correlation row of the pass (Z' order: (unit, item)); lags M n1 + n2
template <int R>
__global__ __launch_bounds__(kBlock, 2) void c128_split_reader_kernel(const double2* __restrict__ Z, RowRec64* __restrict__ rows, long u0, int P,
                                                                      int D, int B, float* __restrict__ q_out) {
  using namespace gacq::f64;
  constexpr int M = kN, N = R * kN;
  const int t = threadIdx.x;
  const long gl = blockIdx.x;                           // ul * P + p
  const long ul = gl / P;
  const int p = (int)(gl % P);
  const long u = u0 + ul;
  const long e = u / D;
  const int d = (int)(u % D);
  const double inv_n = 1.0 / (double)N;
  const double2* z0 = Z + gl * (long)B * R * M + t;
  RowMax row;
  for (int j = 0; j < 16; j++) {
    const int n2 = t + 256 * j;
    double acc[R];
#pragma unroll
    for (int n1 = 0; n1 < R; n1++) acc[n1] = 0.0;
    for (int b = 0; b < B; b++) {
      cd z[R];
#pragma unroll
      for (int kk = 0; kk < R; kk++) z[kk] = ldc(z0 + ((long)b * R + kk) * M + 256 * j);
      if constexpr (R == 4) {
        dft4<false>(z[0], z[1], z[2], z[3]);
#pragma unroll
        for (int n1 = 0; n1 < 4; n1++) acc[n1] += sqrt_pos(z[n1].x * z[n1].x + z[n1].y * z[n1].y) * inv_n;
      } else {
        dft16<false>(z);
#pragma unroll
        for (int n1 = 0; n1 < 16; n1++) { const cd r = z[rev16(n1)]; acc[n1] += sqrt_pos(r.x * r.x + r.y * r.y) * inv_n; }
      }
    }
#pragma unroll
    for (int n1 = 0; n1 < R; n1++) {
      const int lag = M * n1 + n2;
      if (q_out) q_out[lag] = (float)acc[n1];
      row.take(acc[n1], lag);
    }
  }
  row.wave_reduce();
  row.block_reduce<kBlock / 64>();
  if (t == 0) rows[(e * P + p) * (long)D + d] = row.rec();
}

// ---- N = 31 x M (61380 = 31 x 1980, 30690 = 31 x 990: every 10.23 Mcps script, E6, Xona X5) in complex128 ---------------------------
// rocFFT has no radix-31 butterfly and runs these lengths through Bluestein (three transforms of twice the size per FFT): the pipeline
// above manages 1.4e10 cells/s at BASELINE config 4.  The Cooley-Tukey split of gacq_split.hip in fp64 keeps the prime out of rocFFT:
//   n = M n1 + n2, k = k1 + 31 k2:  X[k1 + 31 k2] = sum_n2 W_M^{n2 k2} (W_N^{n2 k1} sum_n1 x[M n1 + n2] W_31^{n1 k1})
//   forward:  c128_r31_forward_kernel (DFT-31 over n1 + twiddle, thread = n2)  ->  rocFFT double, length M (= 4 x 5 x 9 x 11: native radices),
//             batch 31 x rows, in place  ->  X in [k1][k2] order (the code spectra are reordered once to match)
//   inverse:  conj_mul64_kernel  ->  rocFFT inverse length M  ->  c128_r31_reader_kernel (twiddle, inverse DFT-31, |.| / N, sum over the
//             blocks, first-argmax reduce; one workgroup per correlation row)
// The DFT-31 uses the conjugate symmetry of W_31 like dft_prime of gacq_cplx.h: s_n = x[n] + x[31-n], d_n = x[n] - x[31-n],
// A_k = x[0] + sum cos(2 pi nk/31) s_n, B_k = sum sin(2 pi nk/31) d_n, X[k], X[31-k] = A_k -/+ i B_k (inverse: signs swapped).
__constant__ double kCos31[16] = {1.0, 0.97952994125249448, 0.9189578116202306, 0.82076344120727629, 0.68896691907568663, 0.52896401032696239,
                                  0.34730525284482028, 0.1514277775045767, -0.050649168838712642, -0.25065253225872042, -0.44039415155763439,
                                  -0.61210598254766257, -0.75875812269279086, -0.87434661614458209, -0.95413925640004882, -0.99486932339189504};
__constant__ double kSin31[16] = {0.0, 0.20129852008866006, 0.39435585511331855, 0.57126821509479231, 0.72479278722911988, 0.84864425749475092,
                                  0.93775213214708042, 0.98846832432811138, 0.99871650717105276, 0.96807711886620429, 0.89780453957074158,
                                  0.79077573693769887, 0.65137248272222226, 0.48530196253108104, 0.29936312297335804, 0.10116832198743272};

// out(k, X[k]) for k = 0..30 from x[0] and the folded pairs sn[n] = x[n] + x[31-n], dn[n] = x[n] - x[31-n], n = 1..15
template <bool INV, class Sink> __device__ __forceinline__ void dft31_core_f64(f64::cd x0, const f64::cd (&sn)[16], const f64::cd (&dn)[16], Sink&& out) {
  using f64::cd;
  cd sum = x0;
#pragma unroll
  for (int n = 1; n <= 15; n++) sum = sum + sn[n];
  out(0, sum);
#pragma unroll
  for (int k = 1; k <= 15; k++) {
    cd A = x0, B = cd{0.0, 0.0};
#pragma unroll
    for (int n = 1; n <= 15; n++) {
      const int m = (n * k) % 31;
      const int mm = m <= 15 ? m : 31 - m;
      const double c = kCos31[mm], sg = m <= 15 ? kSin31[mm] : -kSin31[mm];
      A.x = __builtin_fma(c, sn[n].x, A.x);
      A.y = __builtin_fma(c, sn[n].y, A.y);
      B.x = __builtin_fma(sg, dn[n].x, B.x);
      B.y = __builtin_fma(sg, dn[n].y, B.y);
    }
    // forward: X[k] = A - i B, X[31-k] = A + i B
    out(k, INV ? f64::add_i(A, B) : f64::sub_i(A, B));
    out(31 - k, INV ? f64::sub_i(A, B) : f64::add_i(A, B));
  }
}
template <bool INV, class Sink> __device__ __forceinline__ void dft31_f64(f64::cd (&x)[31], Sink&& out) {
  f64::cd sn[16], dn[16];
#pragma unroll
  for (int n = 1; n <= 15; n++) {
    sn[n] = x[n] + x[31 - n];
    dn[n] = x[n] - x[31 - n];
  }
  dft31_core_f64<INV>(x[0], sn, dn, out);
}

// grid: rows x chunks; thread = n2.  y: the carrier-wiped rows of mix64_kernel (N samples per forward row)
__global__ __launch_bounds__(kBlock) void c128_r31_forward_kernel(const double2* __restrict__ y, double2* __restrict__ A, const double2* __restrict__ WN,
                                                                   int M, int chunks) {
  using f64::cd;
  const unsigned row = blockIdx.x / (unsigned)chunks;
  const int n2 = (int)(blockIdx.x % (unsigned)chunks) * kBlock + threadIdx.x;
  if (n2 >= M) return;
  const double2* src = y + (long)row * 31 * M + n2;
  cd v[31];
#pragma unroll
  for (int n1 = 0; n1 < 31; n1++) v[n1] = ldc(src + (long)n1 * M);
  double2* dst = A + (long)row * 31 * M + n2;
  // W_N^{n2 k1}: the outputs arrive as k1 = 0, then the pairs (k, 31 - k): w^k by a chain of products from w = W_N^{n2}, and
  // w^{31-k} = W_M^{n2} conj(w^k) -- two coalesced table reads per column instead of 30 gathers with a lane stride of 16 k1 bytes
  // (64 cache lines per wave and load)
  const cd w1 = ldc(WN + n2), w31 = ldc(WN + 31 * n2);
  cd wk = cd{1.0, 0.0};
  dft31_f64<false>(v, [&](int k1, cd val) {
    if (k1 == 0) { stc(dst, val); return; }
    if (k1 <= 15) { wk = wk * w1; stc(dst + (long)k1 * M, val * wk); }
    else stc(dst + (long)k1 * M, val * (w31 * f64::conj(wk)));
  });
}

// one workgroup per correlation row g (Z: [g][b][k1][n2] after the inner inverse transforms, unnormalised); lags M n1 + n2.
// The magnitudes are summed over the blocks in the thread's own 31 LDS slots (in registers, or reduced on the fly for B = 1, the unrolled
// transform spills 0.3-0.9 KB per lane).  The inputs are loaded and folded pair by pair (x[n], x[31-n]).
__global__ __launch_bounds__(kBlock, 2) void c128_r31_reader_kernel(const double2* __restrict__ Z, RowRec64* __restrict__ rows, const double2* __restrict__ WN,
                                                                     long g0, int M, int B, float* __restrict__ q_out) {
  using f64::cd;
  __shared__ double s_acc[31 * kBlock];
  const int t = threadIdx.x;
  const long gl = blockIdx.x;
  const long N = 31L * M;
  const double inv_n = 1.0 / (double)N;
  f64::RowMax row;
  for (int n2 = t; n2 < M; n2 += kBlock) {
#pragma unroll
    for (int n1 = 0; n1 < 31; n1++) s_acc[n1 * kBlock + t] = 0.0;
    const cd w1c = f64::conj(ldc(WN + n2)), w31c = f64::conj(ldc(WN + 31 * n2));
    for (int b = 0; b < B; b++) {
      const double2* src = Z + ((gl * B + b) * 31L) * M + n2;
      const cd x0 = ldc(src);
      cd sn[16], dn[16];
      // conj(W_N^{n2 k1}): conj(w)^n by a chain of products, conj(w^{31-n}) = conj(W_M^{n2}) w^n (see c128_r31_forward_kernel).  Ten
      // loads at a time: hoisted all together -- the compiler's choice -- the 60 loads of a column take 240 registers
      cd wn = cd{1.0, 0.0};
#pragma unroll
      for (int n = 1; n <= 15; n++) {
        wn = wn * w1c;
        const cd a = ldc(src + (long)n * M) * wn;
        const cd c = ldc(src + (long)(31 - n) * M) * (w31c * f64::conj(wn));
        sn[n] = a + c;
        dn[n] = a - c;
        if (n % 5 == 0) asm volatile("" : "+v"(sn[n].x), "+v"(dn[n].x) :: "memory");
      }
      dft31_core_f64<true>(x0, sn, dn, [&](int n1, cd val) {
        s_acc[n1 * kBlock + t] += f64::sqrt_pos(val.x * val.x + val.y * val.y) * inv_n;
      });
    }
#pragma unroll
    for (int n1 = 0; n1 < 31; n1++) {
      const double m = s_acc[n1 * kBlock + t];
      const int lag = M * n1 + n2;
      if (q_out) q_out[lag] = (float)m;
      row.take(m, lag);
    }
  }
  row.wave_reduce();
  row.block_reduce<kBlock / 64>();
  if (t == 0) rows[g0 + gl] = row.rec();
}

// ---- N = 4096 with several blocks or carriers (GPS L1 / Xona at --time > 1: the reference CLI's own default is --time 80) in complex128 ----
// The two-kernel form of lds_forward_kernel + lds_correlate_kernel on the complex128 transform: forward spectra once per (epoch, carrier,
// Doppler bin, block) -- conj(FFT(x nco)), natural order, 64 KB per row --, then one workgroup per (epoch, Doppler bin, item) that holds the
// item's code spectrum in registers, walks the B rows (C_p conj(X), inverse transform, |.| / N summed over the blocks in registers) and
// reduces.  Nothing but X crosses HBM twice; the rocFFT pipeline it replaces moves five stage boundaries of 32 N per row and block.
__global__ __launch_bounds__(kBlock, 2) void c128_4k_forward_kernel(XSrc x, size_t epoch_stride, double2* __restrict__ X, const double* __restrict__ freq,
                                                                    const double2* __restrict__ tab, const double2* __restrict__ tw, int n, int FD, int B) {
  using namespace gacq::f64;
  extern __shared__ __attribute__((aligned(16))) double lds64[];
  const int t = threadIdx.x;
  const unsigned row = blockIdx.x;          // ((e*FD + fd)*B + b)
  const int b = (int)(row % (unsigned)B);
  const unsigned r2 = row / (unsigned)B;
  const int fd = (int)(r2 % (unsigned)FD);
  const long e = r2 / (unsigned)FD;
  const double f = freq[fd];
  const XSrc src = x.offset(e * epoch_stride + (size_t)b * n);
  const cd wa = ldc(tw + t), wb = ldc(tw + 16 * (t & 15));
  cd v[16];
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const int i = t + 256 * j;
    const double2 sv = ld_x(src, i);
    const double2 w = tab[nco_index(f, i)];                     // gnsstools/nco.py:6-10
    v[j] = cd{sv.x, sv.y} * cd{w.x, w.y};
  }
  fft4096<false>(v, lds64, wa, wb, t);
  double2* dst = X + (long)row * kN + t;
#pragma unroll
  for (int j = 0; j < 16; j++) stc(dst + 256 * j, conj(v[rev16(j)]));      // np.conj(fft.fft(b))  acquire-gps-l1.py:32
}

// grid: 8 x ceil(units / 8) x P; the P workgroups of an (epoch, Doppler bin) unit run on one XCD and share its B rows in that L2
__global__ __launch_bounds__(kBlock, 2) void c128_4k_correlate_kernel(const double2* __restrict__ X, const double2* __restrict__ C,
                                                                      const int* __restrict__ items, const int* __restrict__ fset,
                                                                      const double2* __restrict__ tw, RowRec64* __restrict__ rows, int E, int P, int F,
                                                                      int D, int B) {
  using namespace gacq::f64;
  extern __shared__ __attribute__((aligned(16))) double lds64[];
  __shared__ cd s_tw2[15 * 16];
  const int t = threadIdx.x;
  const unsigned xcd = blockIdx.x & 7u, jx = blockIdx.x >> 3;
  const int p = (int)(jx % (unsigned)P);
  const unsigned u = (jx / (unsigned)P) * 8u + xcd;
  if (u >= (unsigned)E * (unsigned)D) return;
  const long e = u / (unsigned)D;
  const int d = (int)(u % (unsigned)D);
  const cd wa = ldc(tw + t), wb = ldc(tw + 16 * (t & 15));
  build_tw2(s_tw2, conj(wb), t);                          // pass-2 powers of the inverse transform, as in fused4k_c128_kernel
  cd c[16];
  {
    const double2* cp = C + (long)items[p] * kN + t;
#pragma unroll
    for (int j = 0; j < 16; j++) c[j] = ldc(cp + 256 * j);
  }
  const double2* xs = X + ((((long)e * F + fset[p]) * D + d) * (long)B) * kN + t;
  const double inv_n = 1.0 / (double)kN;
  double q[16];
#pragma unroll
  for (int k = 0; k < 16; k++) q[k] = 0.0;
  __syncthreads();
  for (int b = 0; b < B; b++) {
    cd v[16];
#pragma unroll
    for (int j = 0; j < 16; j++) v[j] = ldc(xs + (long)b * kN + 256 * j);
#pragma unroll
    for (int j = 0; j < 16; j++) v[j] = c[j] * v[j];                             // C_p * np.conj(fft.fft(b))
    if (b > 0) __syncthreads();                                                  // the previous transform's exchange-2 reads are complete
    fft4096<true, true, true>(v, lds64, wa, wb, t, s_tw2 + (t & 15));
    asm volatile("s_setprio 0" ::: "memory");
#pragma unroll
    for (int k = 0; k < 16; k++) {                                               // lane t holds lags t + 256 k
      const cd r = v[rev16(k)];
      q[k] += sqrt_pos(r.x * r.x + r.y * r.y) * inv_n;                           // np.absolute(ifft(...)), summed over the blocks
    }
  }
  RowMax row = wave_reduce_lags256(q, t);
  row.block_reduce<kBlock / 64>();
  if (t == 0) rows[(e * P + p) * (long)D + d] = row.rec();
}

int nco_table64(gacq_ctx* ctx, const double2** out) {
  auto it = ctx->tables.find("nco64");
  if (it != ctx->tables.end()) { *out = (const double2*)it->second.p; return GACQ_OK; }
  std::vector<double2> h(kNcoTableSize);
  for (int k = 0; k < kNcoTableSize; k++) {
    const double a = 2.0 * M_PI * (double)k * (1.0 / kNcoTableSize);       // np.exp(2*pi*1j*np.arange(NT)*(1.0/NT))  nco.py:4
    h[k] = make_double2(std::cos(a), std::sin(a));
  }
  const void* p = nullptr;
  const int rc = table_cache(ctx, "nco64", h.data(), sizeof(double2) * kNcoTableSize, &p);
  *out = (const double2*)p;
  return rc;
}

}  // namespace

namespace gacq {

int verify_spectra(gacq_sig* s) {
  if (s->spectra64) return GACQ_OK;
  gacq_ctx* ctx = s->ctx;
  const size_t count = (size_t)s->nprn * s->N;
  std::vector<double2> host(count, make_double2(0.0, 0.0));
  for (int p = 0; p < s->nprn; p++)
    for (int i = 0; i < s->desc.n; i++) host[(size_t)p * s->N + i].x = (double)s->replica[(size_t)p * s->desc.n + i];
  // built in a local buffer and published only once the transform has run: a failure (the transform's scratch, a rocFFT plan) must not
  // leave untransformed replicas behind for the next call to take for code spectra
  double2* buf = nullptr;
  GACQ_HIP(ctx, hipMalloc((void**)&buf, sizeof(double2) * count));
  int rc = GACQ_OK;
  if (hipMemcpyAsync(buf, host.data(), sizeof(double2) * count, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
    rc = set_error(ctx, GACQ_ERR_HIP, "complex128 code spectra: upload of the replicas failed");
  // c = fft.fft(c)   acquire-gps-l1.py:24 -- with the library's own complex128 transform where it factors the length (every length of the
  // reference's scripts), so that the default path never pays for a rocFFT plan; rocFFT's double-precision transform otherwise
  if (rc == GACQ_OK) rc = tie_code_spectra64(ctx, buf, s->nprn, s->N);
  if (rc == GACQ_ERR_UNSUPPORTED) rc = fft_exec(ctx, s->N, s->nprn, false, buf, true);
  if (rc == GACQ_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = set_error(ctx, GACQ_ERR_HIP, "complex128 code spectrum transform failed");
  if (rc != GACQ_OK) {
    (void)hipStreamSynchronize(ctx->stream);      // `host` is still being read by the copy
    (void)hipFree(buf);
    return rc;
  }
  s->spectra64 = buf;
  return GACQ_OK;
}

// the code spectra in the order the R x M forms read them (c128_split_spectra_kernel), published only once the reorder has run
static int split_spectra64(gacq_sig* sig, int R, int M, const char* what) {
  if (sig->spectra64_split) return GACQ_OK;
  gacq_ctx* ctx = sig->ctx;
  double2* buf = nullptr;
  GACQ_HIP(ctx, hipMalloc((void**)&buf, sizeof(double2) * (size_t)sig->nprn * sig->N));
  hipLaunchKernelGGL(c128_split_spectra_kernel, dim3((unsigned)(sig->nprn * R)), dim3(kBlock), 0, ctx->stream, (const double2*)sig->spectra64, buf, R, M);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
    (void)hipFree(buf);
    return set_error(ctx, GACQ_ERR_HIP, "%s: code-spectrum reorder failed", what);
  }
  sig->spectra64_split = buf;
  return GACQ_OK;
}

// the split form's kernels for one outer radix (N = 4 x 4096 or 16 x 4096)
struct SplitKernels {
  decltype(&c128_split_forward_kernel<4>) forward;
  decltype(&c128_split_corr_kernel<4>) corr;
  decltype(&c128_split_reader_kernel<4>) reader;
};
template <int R> static SplitKernels split_kernels() { return {c128_split_forward_kernel<R>, c128_split_corr_kernel<R>, c128_split_reader_kernel<R>}; }

// One host path for the five forms, in the shape of launch_search: prepare, size the epoch pass, then per epoch pass the form's forward
// stage, the Z' passes of the forms with a Z' round trip (writer, inverse, reader) and one Doppler scan.
int verify_search(gacq_sig* sig, const SearchPlan& plan, XSrc d_x, size_t nsamp, int nepoch, int P, int F, int D, int B, gacq_peak* d_out,
                  float* d_qrow) {
  gacq_ctx* ctx = sig->ctx;
  hipStream_t st = ctx->stream;
  const int n = sig->desc.n, N = sig->N;
  const Form form = plan.form;
  const bool fused = form == Form::C128Fused4k, lds4k = form == Form::C128Lds4k, split = form == Form::C128Split, r31 = form == Form::C128R31;
  const bool rocfft = form == Form::C128Rocfft;
  const char* what = split ? "complex128 split engine" : r31 ? "complex128 radix-31 engine" : "verification engine";
  const auto stage = [rocfft](int s) { return rocfft ? -1 : s; };      // the rocFFT form records no stage times
  // one kernel on the search's stream under stage timer s (s < 0: inside a stage of its caller)
  const auto launch = [&](int s, auto kernel, long grid, int block, size_t lds, auto... args) {
    return timed(ctx, stage(s), [&] {
      hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(block), lds, st, args...);
      GACQ_HIP(ctx, hipGetLastError());
      return (int)GACQ_OK;
    });
  };
  int rc;
  if ((rc = verify_spectra(sig)) != GACQ_OK) return rc;
  const double2* tab;
  if ((rc = nco_table64(ctx, &tab)) != GACQ_OK) return rc;
  // N = R x M: the split form's outer radix 4 / 16 over the resident 4096-point transform; 31 x M around rocFFT's length-M transforms (M in its
  // native radices: no Bluestein); 1 x N, rocFFT's own length-N transform
  const int R = split ? N / f64::kN : r31 ? 31 : 1, M = N / R;
  const double2* tw = nullptr;      // W_4096 of the resident transform (N = 4096) / W_N of the outer stage (split, radix-31)
  if (!rocfft && (rc = twiddles64(ctx, N, &tw)) != GACQ_OK) return rc;
  if ((split || r31) && (rc = split_spectra64(sig, R, M, what)) != GACQ_OK) return rc;
  const double2* C = (const double2*)(split || r31 ? sig->spectra64_split : sig->spectra64);
  const SplitKernels sk = R == 4 ? split_kernels<4>() : split_kernels<16>();
  const void* lds_kernels[2] = {nullptr, nullptr};      // the form's kernels on the resident transform: 64 KiB of dynamic LDS
  if (fused) lds_kernels[0] = (const void*)fused4k_c128_kernel;
  if (lds4k) { lds_kernels[0] = (const void*)c128_4k_forward_kernel; lds_kernels[1] = (const void*)c128_4k_correlate_kernel; }
  if (split) { lds_kernels[0] = (const void*)sk.forward; lds_kernels[1] = (const void*)sk.corr; }
  for (const void* k : lds_kernels)
    if (k) GACQ_HIP(ctx, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, f64::kLdsBytes));

  // epochs per pass so that the forward-spectra buffer respects the workspace limit; the fused form buffers nothing but the row records
  const size_t x_epoch_bytes = sizeof(double2) * (size_t)F * D * B * N;
  const int Ec = fused ? nepoch : epochs_per_pass(ctx, nepoch, x_epoch_bytes);
  if (!fused && (rc = ensure(ctx, ctx->X, x_epoch_bytes * Ec)) != GACQ_OK) return rc;
  if ((rc = ensure(ctx, ctx->rows, sizeof(RowRec64) * (size_t)Ec * P * D)) != GACQ_OK) return rc;

  // items per workgroup.  Fused: one forward transform per workgroup, amortised over up to 32 items while >= ~1024 workgroups remain (2
  // resident per CU).  Split writer: the forward-spectrum row stays in registers over its items (one carrier); with a carrier per item
  // (GLONASS) every item has its own row and nothing is shared.
  int pch = 1;
  if (fused) {
    pch = 4;
    while (pch < 32 && (long)nepoch * D * ((P + 2 * pch - 1) / (2 * pch)) >= 1024) pch *= 2;
    pch = std::min(pch, P);
  } else if (split && F == 1) {
    pch = std::min(P, 8);
  }
  const int nchunk = (P + pch - 1) / pch;
  const unsigned cols = (unsigned)((N + kBlock - 1) / kBlock);
  const int chunksM = (M + kBlock - 1) / kBlock;
  const int* d_items = (const int*)ctx->items.p;
  const int* d_fset = (const int*)ctx->fset.p;
  const double* d_freq = (const double*)ctx->freq.p;
  for (int e0 = 0; e0 < nepoch; e0 += Ec) {
    const int ne = std::min(Ec, nepoch - e0);
    const XSrc xe = d_x.offset((size_t)e0 * nsamp);
    double2* X = (double2*)ctx->X.p;
    RowRec64* rows = (RowRec64*)ctx->rows.p;
    const long rows_x = (long)ne * F * D * B;
    switch (form) {
      case Form::C128Fused4k:      // one kernel per search: the row never leaves the workgroup
        rc = launch(6, fused4k_c128_kernel, 8 * (long)((ne + 7) / 8) * D * nchunk, kBlock, f64::kLdsBytes, xe, nsamp, C, d_items, d_freq, tab, tw, rows, ne, P, D, pch,
                    nchunk);
        break;
      case Form::C128Lds4k:      // several blocks or carriers: forward spectra once, then one workgroup per (epoch, Doppler bin, item) over its B rows
        rc = launch(0, c128_4k_forward_kernel, rows_x, kBlock, f64::kLdsBytes, xe, nsamp, X, d_freq, tab, tw, n, F * D, B);
        if (rc == GACQ_OK)
          rc = launch(6, c128_4k_correlate_kernel, 8 * (((long)ne * D + 7) / 8) * P, kBlock, f64::kLdsBytes, X, C, d_items, d_fset, tw, rows, ne, P, F, D, B);
        break;
      default: {      // the forms with a Z' round trip: carrier wipe-off, then the forward transform
        if (rows_x * cols >= (1L << 31)) return set_error(ctx, GACQ_ERR_UNSUPPORTED, "%s: too many forward rows in one pass (lower the workspace limit)", what);
        // split and radix-31: wipe-off into the correlation workspace (free until the first Z' pass), the outer DFT out of it into X
        if (!rocfft && (rc = ensure(ctx, ctx->Y, x_epoch_bytes * ne)) != GACQ_OK) return rc;
        double2* mixed = rocfft ? X : (double2*)ctx->Y.p;
        rc = timed(ctx, stage(0), [&] {
          int r = launch(-1, mix64_kernel, rows_x * cols, kBlock, 0, xe, nsamp, mixed, d_freq, tab, n, N, F * D, B, cols);
          if (r == GACQ_OK && split) r = launch(-1, sk.forward, ((rows_x + 7) / 8) * 8 * R, kBlock, f64::kLdsBytes, mixed, X, tw, (unsigned)rows_x);
          if (r == GACQ_OK && r31) r = launch(-1, c128_r31_forward_kernel, rows_x * chunksM, kBlock, 0, mixed, X, tw, M, chunksM);
          return r;
        });
        if (rc == GACQ_OK && !split) rc = timed(ctx, stage(1), [&] { return fft_exec(ctx, M, rows_x * R, false, X, true); });
      }
    }
    if (rc != GACQ_OK) return rc;
    if (split || r31 || rocfft) {
      // Z' passes of whole units of B rows each.  Split: an (epoch, Doppler bin) with its P items; radix-31 and rocFFT: an (epoch, item,
      // Doppler bin) group.  Split and radix-31: at most 4 GiB a pass (or one unit / eight items' worth where that is more), as in the fp32
      // split engines, and one unit a pass for a row dump; the rocFFT form fills the workspace.  No evening of the passes.
      const long units = (long)ne * D * (split ? 1 : P);
      const size_t unit_bytes = sizeof(double2) * (size_t)B * N * (split ? P : 1);
      const size_t floor_bytes = split ? unit_bytes : 8 * unit_bytes * (size_t)D;
      const size_t pass_cap = rocfft ? ws_budget(ctx) : std::min(ws_budget(ctx), std::max<size_t>((size_t)4 << 30, floor_bytes));
      long uc = (long)std::max<size_t>(1, std::min<size_t>((size_t)units, pass_cap / unit_bytes));
      uc = std::min<long>(uc, std::max<long>(1, ((1L << 31) - 1) / (split ? (long)B * R * nchunk : (long)B * cols)));      // the writer's grid below 2^31
      if (d_qrow && !rocfft) uc = 1;
      if ((rc = ensure(ctx, ctx->Y, unit_bytes * uc)) != GACQ_OK) return rc;
      double2* Y = (double2*)ctx->Y.p;
      for (long u0 = 0; u0 < units; u0 += uc) {
        const long nu = std::min(uc, units - u0);
        switch (form) {
          case Form::C128Split:      // K2 + inner transforms + twiddle in one kernel; then outer inverse DFT-R + |.| + reduce
            rc = launch(6, sk.corr, nu * B * nchunk * R, kBlock, f64::kLdsBytes, X, C, Y, d_items, d_fset, tw, u0, P, F, D, B, pch, nchunk);
            if (rc == GACQ_OK) rc = launch(4, sk.reader, nu * P, kBlock, 0, Y, rows, u0, P, D, B, d_qrow);
            break;
          default:      // K2, rocFFT's inverse transforms of length M; then inverse DFT-31 + |.| + reduce, or magnitudes and peaks
            rc = launch(2, conj_mul64_kernel, nu * B * cols, kBlock, 0, X, C, Y, d_items, d_fset, u0, P, F, D, B, N, cols);
            if (rc == GACQ_OK) rc = timed(ctx, stage(3), [&] { return fft_exec(ctx, M, nu * B * R, true, Y, true); });
            if (rc == GACQ_OK && r31) rc = launch(4, c128_r31_reader_kernel, nu, kBlock, 0, Y, rows, tw, u0, M, B, d_qrow);
            if (rc == GACQ_OK && rocfft) rc = launch(4, mag_peak64_kernel, nu, kBlock, 0, Y, rows, u0, B, N, d_qrow);
        }
        if (rc != GACQ_OK) return rc;
      }
    }
    const long nep = (long)ne * P;
    if ((rc = launch(5, best_doppler64_kernel, (nep + 63) / 64, 64, 0, rows, d_out + (size_t)e0 * P, nep, D, N, sig->desc.metric_mode)) != GACQ_OK) return rc;
  }
  return GACQ_OK;
}

}  // namespace gacq
