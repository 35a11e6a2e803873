// Navigation data from tracked prompts (gacq_navsym, gacq_viterbi_dev; the definitions are in include/gacq.h, restated in numpy in
// tests/navdata_oracle.py).
//
// navsym_kernel: one workgroup per channel.  S[a][m] = sum_r o[r] p[a + m R + r] is evaluated in fp64, r ascending, nothing fused
// (o[r] p is exact, so the only roundings are the R - 1 additions).  The alignments are walked one after the other, a lane taking
// every kNavBlock-th symbol of the alignment, so that a lane's running sum of an alignment is one register and consecutive lanes read
// consecutive runs of R prompts (every cache line it touches is used whole).  Pass 1 reduces the largest finite |S| as the bit pattern
// of the double (monotonic for finite non-negative values); pass 2 reduces t = llrint(ldexp(|S|, 40 - e)) per alignment as int64 and
// counts the symbols that are finite; both reductions are of integers, so no order can change them.  One lane then picks the
// alignment and forms A, and the symbols of that alignment alone are evaluated once more and quantised.
//
// viterbi_kernel: one wave per job, state s in lane s, kVitWaves jobs per workgroup.  64 steps at a time: lane i fetches the symbol
// pair of step t0 + i (through the job's gather), the pairs are handed round by v_readlane, the two predecessor metrics come by
// ds_bpermute, the 64-bit ballot of the decisions of step t0 + i is kept by lane i and the 64 survivor words are written together.
// Survivors live in LDS (kVitLdsSteps steps per wave); a job longer than that keeps them in a global workspace instead.  The
// traceback reads 64 words at a time and walks them with scalar arithmetic; lane i then writes the bit of step t0 + i.  The waves of
// a workgroup never meet: there is no barrier in the kernel.
#pragma clang fp contract(off)

#include "gacq_common.h"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace gacq;

namespace {

constexpr int kNavBlock = 256;
constexpr int kNavWaves = kNavBlock / 64;
constexpr int kNavMaxR = GACQ_NAV_MAX_R;
constexpr int kNavMaxN = 1 << 24;
constexpr unsigned long long kInfBits = 0x7ff0000000000000ull;

constexpr int kVitWaves = 4;
constexpr int kVitLdsSteps = 1536;                  // 12 KiB of survivor words per wave, 48 KiB per workgroup
constexpr int kVitMaxSteps = 1 << 20;
constexpr int kVitFloor = -(1 << 28);

struct NavChan {
  long long p_off;               // first prompt of the channel in the flat array
  long long q_off;               // first soft symbol of the channel in the flat output
  int n, R, align, pad;
  int8_t o[kNavMaxR + 4];
};

struct NavOut {
  long long E[kNavMaxR];
  double A;
  int align, nq;
};

__device__ __forceinline__ double nav_sum(const double* __restrict__ p, const double (&o)[kNavMaxR], int R) {
  double s = o[0] * p[0];
#pragma unroll
  for (int r = 1; r < kNavMaxR; r++)
    if (r < R) s = s + o[r] * p[r];
  return s;
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const unsigned long long w = __shfl_xor(v, off);
    v = w > v ? w : v;
  }
  return v;
}

__global__ __launch_bounds__(kNavBlock) void navsym_kernel(const NavChan* __restrict__ chans, const double* __restrict__ prompts,
                                                           NavOut* __restrict__ outs, int8_t* __restrict__ q_out) {
  __shared__ unsigned long long wmax[kNavWaves];
  __shared__ long long wsum[kNavMaxR][kNavWaves];
  __shared__ int wcnt[kNavMaxR][kNavWaves];
  __shared__ int s_align;
  __shared__ double s_A;
  const NavChan& c = chans[blockIdx.x];
  const double* __restrict__ p = prompts + c.p_off;
  const int n = c.n, R = c.R, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double o[kNavMaxR];
#pragma unroll
  for (int r = 0; r < kNavMaxR; r++) o[r] = r < R ? (double)c.o[r] : 0.0;

  // pass 1: the largest finite |S|
  unsigned long long mx = 0ull;
  for (int a = 0; a < R; a++) {
    const int M = (n - a) / R;
    for (int m = tid; m < M; m += kNavBlock) {
      const unsigned long long b = (unsigned long long)__double_as_longlong(fabs(nav_sum(p + a + (long long)m * R, o, R)));
      if (b < kInfBits && b > mx) mx = b;
    }
  }
  mx = wave_max(mx);
  if (lane == 0) wmax[wave] = mx;
  __syncthreads();
  mx = wmax[0];
#pragma unroll
  for (int w = 1; w < kNavWaves; w++) mx = wmax[w] > mx ? wmax[w] : mx;
  int e = 0;
  (void)frexp(__longlong_as_double((long long)mx), &e);

  // pass 2: per alignment, the sum of t and the number of symbols that are finite
  for (int a = 0; a < R; a++) {
    const int M = (n - a) / R;
    long long acc = 0, cnt = 0;
    for (int m = tid; m < M; m += kNavBlock) {
      const double s = fabs(nav_sum(p + a + (long long)m * R, o, R));
      if ((unsigned long long)__double_as_longlong(s) < kInfBits) {
        acc += llrint(ldexp(s, 40 - e));
        cnt++;
      }
    }
    acc = wave_sum(acc);
    cnt = wave_sum(cnt);
    if (lane == 0) {
      wsum[a][wave] = acc;
      wcnt[a][wave] = (int)cnt;
    }
  }
  __syncthreads();
  if (tid == 0) {
    NavOut& out = outs[blockIdx.x];
    int best = 0, mbest = 0;
    long long ebest = 0;
    for (int a = 0; a < kNavMaxR; a++) {
      long long E = 0;
      int M = 0;
      if (a < R) {
#pragma unroll
        for (int w = 0; w < kNavWaves; w++) {
          E += wsum[a][w];
          M += wcnt[a][w];
        }
      }
      out.E[a] = E;
      const bool take = a < R && (c.align >= 0 ? a == c.align : (a == 0 || E > ebest));
      if (take) {
        best = a;
        ebest = E;
        mbest = M;
      }
    }
    const double A = mbest > 0 ? ldexp((double)ebest / (double)mbest, e - 40) : 0.0;
    out.A = A;
    out.align = best;
    out.nq = (n - best) / R;
    s_align = best;
    s_A = A;
  }
  __syncthreads();

  // the soft symbols of the chosen alignment
  const int a = s_align;
  const double A = s_A;
  const int M = (n - a) / R;
  int8_t* __restrict__ q = q_out + c.q_off;
  for (int m = tid; m < M; m += kNavBlock) {
    const double s = nav_sum(p + a + (long long)m * R, o, R);
    int v = 0;
    if ((unsigned long long)__double_as_longlong(fabs(s)) < kInfBits && A > 0.0)
      v = (int)fmin(fmax(rint((s * 48.0) / A), -127.0), 127.0);
    q[m] = (int8_t)v;
  }
}

struct VitArgs {
  const gacq_vit_job* jobs;
  const int8_t* sym;
  uint8_t* bits;
  int* metric;
  unsigned long long* spill;     // survivor words of the jobs longer than kVitLdsSteps, at spill_off[job]
  const long long* spill_off;    // -1: the job's survivors fit LDS
  int J;
};

// the symbol pair of step t of the job: low 16 bits the G1 symbol, high 16 bits the G2 symbol (both sign-extended int8)
__device__ __forceinline__ int vit_pair(const gacq_vit_job& j, const int8_t* __restrict__ sym, int t) {
  if (t >= j.steps) return 0;
  int i0 = 2 * t, i1 = 2 * t + 1;
  if (j.rows > 0) {
    i0 = (i0 % j.rows) * j.cols + i0 / j.rows;
    i1 = (i1 % j.rows) * j.cols + i1 / j.rows;
  }
  const int q0 = sym[j.sym_base + i0], q1 = sym[j.sym_base + i1];
  return (q0 & 0xffff) | (q1 << 16);
}

__global__ __launch_bounds__(kVitWaves * 64) void viterbi_kernel(const VitArgs a) {
  __shared__ unsigned long long lds_surv[kVitWaves][kVitLdsSteps];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // uniform: the job is read by scalar loads
  const int job = blockIdx.x * kVitWaves + wave;
  if (job >= a.J) return;
  const gacq_vit_job j = a.jobs[job];
  const long long so = a.spill_off[job];
  const bool spilled = so >= 0;
  unsigned long long* __restrict__ gsurv = a.spill + (spilled ? so : 0);
  unsigned long long* lsurv = lds_surv[wave];

  // lane = next state ns; its predecessors p0 = (2 ns) & 63 and p1 = p0 | 1 under input b = ns >> 5.  p1 differs from p0 in r[6],
  // which both polynomials tap, so its two coded bits are the complements of p0's: bm1 = -bm0.
  const int b = lane >> 5, p0 = (2 * lane) & 63;
  const int c1 = (b ^ (p0 >> 5) ^ (p0 >> 4) ^ (p0 >> 3) ^ p0) & 1;                       // G1 = 171: r0 r1 r2 r3 r6
  const int c2 = ((b ^ (p0 >> 4) ^ (p0 >> 3) ^ (p0 >> 1) ^ p0) & 1) ^ (j.g2_inverted ? 1 : 0);   // G2 = 133: r0 r2 r3 r5 r6
  const int e0 = 1 - 2 * c1, e1 = 1 - 2 * c2;
  int pm = j.start_state < 0 ? 0 : (lane == j.start_state ? 0 : kVitFloor);

  const int steps = j.steps;
  int next = vit_pair(j, a.sym, lane);
  for (int t0 = 0; t0 < steps; t0 += 64) {
    const int pairs = next;
    next = vit_pair(j, a.sym, t0 + 64 + lane);
    const int cnt = min(64, steps - t0);
    unsigned long long mine = 0ull;
    for (int i = 0; i < cnt; i++) {
      const int w = __builtin_amdgcn_readlane(pairs, i);
      const int bm = e0 * (int)(short)(w & 0xffff) + e1 * (w >> 16);
      const int a0 = __builtin_amdgcn_ds_bpermute(4 * p0, pm) + bm;
      const int a1 = __builtin_amdgcn_ds_bpermute(4 * p0 + 4, pm) - bm;
      const bool d = a1 > a0;                                                          // a tie takes p0
      pm = d ? a1 : a0;
      const unsigned long long word = __ballot(d);
      mine = lane == i ? word : mine;
    }
    if (lane < cnt) {
      if (spilled) gsurv[t0 + lane] = mine;
      else lsurv[t0 + lane] = mine;
    }
  }
  // the wave's own survivor stores are complete and visible before its lanes read words that other lanes wrote
  __threadfence();

  // end state: fixed, or the best metric with ties to the lowest state
  int s = j.end_state;
  if (s < 0) {
    int bm = pm, bs = lane;
#pragma unroll
    for (int off = 32; off; off >>= 1) {
      const int om = __shfl_xor(bm, off), os = __shfl_xor(bs, off);
      if (om > bm || (om == bm && os < bs)) {
        bm = om;
        bs = os;
      }
    }
    s = bs;
  }
  s = __builtin_amdgcn_readfirstlane(s);
  const int final_metric = __builtin_amdgcn_readlane(pm, s);
  if (lane == 0) a.metric[job] = final_metric;

  // traceback: the bit of step t is the newest input of the state after it, s >> 5; its predecessor is ((2 s) & 63) | decision
  const int first = j.first_bit, last = j.first_bit + j.nbits;                         // bits [first, last) are written
  if (j.nbits <= 0) return;
  for (int t0 = (steps - 1) & ~63; t0 >= (first & ~63); t0 -= 64) {
    const int cnt = min(64, steps - t0);
    unsigned long long word = 0ull;
    if (lane < cnt) word = spilled ? gsurv[t0 + lane] : lsurv[t0 + lane];
    const unsigned lo = (unsigned)word, hi = (unsigned)(word >> 32);
    unsigned long long outbits = 0ull;
    for (int i = cnt - 1; i >= 0; i--) {
      const unsigned wl = __builtin_amdgcn_readlane(lo, i), wh = __builtin_amdgcn_readlane(hi, i);
      const unsigned long long w = ((unsigned long long)wh << 32) | wl;
      outbits |= (unsigned long long)(s >> 5) << i;
      s = ((2 * s) & 63) | (int)((w >> s) & 1ull);
    }
    const int t = t0 + lane;
    if (lane < cnt && t >= first && t < last) a.bits[j.bit_base + (t - first)] = (uint8_t)((outbits >> lane) & 1ull);
  }
}

}  // namespace

extern "C" int gacq_navsym_check(const double* prompts, const int* n, const int* R, const int8_t* overlay, const int* align, int K,
                                 const int* align_out, const long long* E_out, const double* A_out, const int8_t* q_out, const int* nq_out) {
  if (K < 1) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_navsym: K = %d, need at least one channel", K);
  if (!prompts || !n || !R || !overlay || !align_out || !E_out || !A_out || !q_out || !nq_out)
    return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_navsym: NULL argument");
  for (int k = 0; k < K; k++) {
    if (R[k] < 1 || R[k] > kNavMaxR) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_navsym: channel %d: R = %d outside 1..%d", k, R[k], kNavMaxR);
    if (n[k] > kNavMaxN) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_navsym: channel %d: n = %d above 2^24", k, n[k]);
    for (int r = 0; r < R[k]; r++)
      if (overlay[k * kNavMaxR + r] != 1 && overlay[k * kNavMaxR + r] != -1)
        return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_navsym: channel %d: overlay[%d] = %d is not +-1", k, r, (int)overlay[k * kNavMaxR + r]);
    if (align && (align[k] < -1 || align[k] >= R[k]))
      return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_navsym: channel %d: align = %d outside -1..%d", k, align[k], R[k] - 1);
  }
  for (int k = 0; k < K; k++)
    if (n[k] < 2 * R[k] - 1)
      return set_error(nullptr, GACQ_ERR_SHORT_INPUT, "gacq_navsym: channel %d: %d records, an alignment of R = %d needs %d", k, n[k], R[k], 2 * R[k] - 1);
  return GACQ_OK;
}

extern "C" int gacq_navsym(gacq_ctx* ctx, const double* prompts, const int* n, const int* R, const int8_t* overlay, const int* align, int K,
                           int* align_out, long long* E_out, double* A_out, int8_t* q_out, int* nq_out) {
  // everything is checked before anything is allocated or launched
  const int rc = gacq_navsym_check(prompts, n, R, overlay, align, K, align_out, E_out, A_out, q_out, nq_out);
  if (rc < 0) {
    if (ctx) set_error(ctx, rc, "%s", gacq_last_error(nullptr));
    return rc;
  }
  if (!ctx) return GACQ_ERR_BAD_ARG;
  std::vector<NavChan> chans(K);
  long long np = 0, nq = 0;
  for (int k = 0; k < K; k++) {
    NavChan& c = chans[k];
    c.p_off = np;
    c.q_off = nq;
    c.n = n[k];
    c.R = R[k];
    c.align = align ? align[k] : -1;
    c.pad = 0;
    for (int r = 0; r < kNavMaxR + 4; r++) c.o[r] = r < R[k] ? overlay[k * kNavMaxR + r] : 0;
    np += n[k];
    nq += n[k] / R[k];
  }
  GACQ_DEVICE(ctx);
  const size_t b_ch = (size_t)K * sizeof(NavChan), b_p = (size_t)np * sizeof(double), b_out = (size_t)K * sizeof(NavOut), b_q = (size_t)nq;
  const size_t o_p = (b_ch + 255) & ~(size_t)255, o_out = (o_p + b_p + 255) & ~(size_t)255, o_q = (o_out + b_out + 255) & ~(size_t)255;
  char* d = nullptr;
  GACQ_HIP(ctx, hipMalloc((void**)&d, o_q + b_q + 256));
  std::vector<NavOut> outs(K);
  hipError_t e = hipMemcpyAsync(d, chans.data(), b_ch, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d + o_p, prompts, b_p, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(navsym_kernel, dim3(K), dim3(kNavBlock), 0, ctx->stream, (const NavChan*)d, (const double*)(d + o_p), (NavOut*)(d + o_out),
                       (int8_t*)(d + o_q));
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(outs.data(), d + o_out, b_out, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && b_q) e = hipMemcpyAsync(q_out, d + o_q, b_q, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(d);
  if (e != hipSuccess) return set_error(ctx, GACQ_ERR_HIP, "gacq_navsym: %s", hipGetErrorString(e));
  for (int k = 0; k < K; k++) {
    for (int a = 0; a < kNavMaxR; a++) E_out[(size_t)k * kNavMaxR + a] = outs[k].E[a];
    A_out[k] = outs[k].A;
    align_out[k] = outs[k].align;
    nq_out[k] = outs[k].nq;
  }
  return GACQ_OK;
}

extern "C" int gacq_viterbi_check(const gacq_vit_job* jobs, int J, long long nsym, long long nbits) {
  if (J < 1) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_viterbi_dev: J = %d, need at least one job", J);
  if (!jobs) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_viterbi_dev: NULL argument");
  if (nsym < 0 || nbits < 0) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_viterbi_dev: negative buffer length");
  for (int i = 0; i < J; i++) {
    const gacq_vit_job& j = jobs[i];
    if (j.steps < 1 || j.steps > kVitMaxSteps) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_viterbi_dev: job %d: %d steps outside 1..2^20", i, j.steps);
    if (j.sym_base < 0 || j.sym_base + 2ll * j.steps > nsym)
      return set_error(nullptr, GACQ_ERR_SHORT_INPUT, "gacq_viterbi_dev: job %d: symbols %lld .. %lld of %lld", i, j.sym_base, j.sym_base + 2ll * j.steps - 1, nsym);
    if (j.rows < 0 || j.cols < 0 || (j.rows > 0 && (long long)j.rows * j.cols != 2ll * j.steps))
      return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_viterbi_dev: job %d: a %d x %d gather does not hold its %d symbols", i, j.rows, j.cols, 2 * j.steps);
    if (j.start_state < -1 || j.start_state > 63 || j.end_state < -1 || j.end_state > 63)
      return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_viterbi_dev: job %d: start / end state %d / %d outside -1..63", i, j.start_state, j.end_state);
    if (j.first_bit < 0 || j.nbits < 0 || (long long)j.first_bit + j.nbits > j.steps)
      return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_viterbi_dev: job %d: bits %d .. %d of %d steps", i, j.first_bit, j.first_bit + j.nbits - 1, j.steps);
    if (j.bit_base < 0 || j.bit_base + j.nbits > nbits)
      return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_viterbi_dev: job %d: output bits %lld .. %lld of %lld", i, j.bit_base, j.bit_base + j.nbits - 1, nbits);
  }
  return GACQ_OK;
}

extern "C" int gacq_viterbi_dev(gacq_ctx* ctx, const void* d_sym, long long nsym, const gacq_vit_job* jobs, int J, void* d_bits, long long nbits,
                                void* d_metric) {
  int rc = gacq_viterbi_check(jobs, J, nsym, nbits);
  if (rc == GACQ_OK && (!d_sym || !d_bits || !d_metric)) rc = set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_viterbi_dev: NULL argument");
  if (rc < 0) {
    if (ctx) set_error(ctx, rc, "%s", gacq_last_error(nullptr));
    return rc;
  }
  if (!ctx) return GACQ_ERR_BAD_ARG;
  std::vector<long long> spill_off(J);
  long long nspill = 0;
  for (int i = 0; i < J; i++) {
    spill_off[i] = jobs[i].steps > kVitLdsSteps ? nspill : -1;
    if (jobs[i].steps > kVitLdsSteps) nspill += jobs[i].steps;
  }
  GACQ_DEVICE(ctx);
  const size_t b_jobs = (size_t)J * sizeof(gacq_vit_job), b_off = (size_t)J * sizeof(long long), b_spill = (size_t)nspill * sizeof(unsigned long long);
  const size_t o_off = (b_jobs + 255) & ~(size_t)255, o_spill = (o_off + b_off + 255) & ~(size_t)255;
  char* d = nullptr;
  GACQ_HIP(ctx, hipMalloc((void**)&d, o_spill + b_spill + 256));
  hipError_t e = hipMemcpyAsync(d, jobs, b_jobs, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d + o_off, spill_off.data(), b_off, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    VitArgs a;
    a.jobs = (const gacq_vit_job*)d;
    a.sym = (const int8_t*)d_sym;
    a.bits = (uint8_t*)d_bits;
    a.metric = (int*)d_metric;
    a.spill = (unsigned long long*)(d + o_spill);
    a.spill_off = (const long long*)(d + o_off);
    a.J = J;
    hipLaunchKernelGGL(viterbi_kernel, dim3((J + kVitWaves - 1) / kVitWaves), dim3(kVitWaves * 64), 0, ctx->stream, a);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(d);
  if (e != hipSuccess) return set_error(ctx, GACQ_ERR_HIP, "gacq_viterbi_dev: %s", hipGetErrorString(e));
  return GACQ_OK;
}
