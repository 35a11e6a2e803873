// Cancellation of tracked signals (gacq_cancel_dev, include/gacq.h): every satellite's signal is rebuilt from per-segment parameters
//   theta(j) = (p0 + i F) mod 2^64,  pos(j) = c0 + i Cf,  i = j - s0,   r(j) = w(pos(j)) exp(2 pi i theta(j) / 2^64)
// and taken out of the recording, v(j) = x(j) - sum_k float32(A_k) r_k(j), with A_k given or estimated per segment as the projection
// A = sum x conj(r) / sum w^2 of the input on the replica.  Two kernels:
//   cancel_project_kernel   one workgroup per segment; sample i goes to lane i mod 256, a lane adds its products in ascending i in fp64,
//                           the lanes are summed by a fixed tree (DPP inside a row of 16, then LDS): no atomics, so the bits of A depend
//                           on the segment and its samples alone.
//   cancel_subtract_kernel  a workgroup owns a tile of 2048 consecutive output samples, a lane a run of 8 (one 16-byte store of int8
//                           I/Q).  Per (tile, satellite) one lane finds the first segment that ends after the tile's first sample by
//                           bisection; every lane walks on from there to its run and then over the segment boundaries inside the run.
// Nothing is carried from sample to sample: phase and code position of a sample are one 64-bit multiply-add each on i (< 2^24, so the
// whole chips since s0 fit 32 bits), and the chip index is that count mod L by a multiplication with 1 / L in fp64 and one correction
// (the count is below 2^29: the product is off only at exact multiples of L, by one, downwards).  A tile's bytes therefore cannot depend
// on the tiling, the call or the addresses.
// Chips are read as bytes from the context's cached tables ("chips:<code>:<prn>", shared with the tracking loops and the simulator)
// through the cache, reloaded only when a lane's chip index moves: 32 tables of at most 10240 bytes stay resident in L2, consecutive
// samples mostly share a chip, and no per-tile staging pass is needed.
// sin / cos: turn_sincos of gacq_turn.h, the one routine gacq_simulate.hip calls, so the replica of a simulated signal is that signal.
// The int8 output is rint / clamp of the very fp32 values the complex64 output stores.
// The replica (cancel_replica), the device tables CanSat / CanSeg and the host preparation of the segment table are
// in gacq_cancelcore.h, which gacq_aprompt.hip shares: its prompts are cancel_project_kernel's amplitudes bit for bit.
#pragma clang fp contract(off)

#include "gacq_cancelcore.h"
#include "gacq_fft64.h"

using namespace gacq;

namespace {

constexpr int kCanRun = 8;                      // samples per lane: one 16-byte store of int8 I/Q
constexpr int kCanTile = kCanBlock * kCanRun;

struct CanArgs {
  const CanSat* sats;
  const CanSeg* segs;
  const void* in;                               // the input of output sample out_first
  void* out;
  unsigned long long* clip;                     // NULL, or the count of int8 components at +-127
  long long out_first, n;
  int K;
  int in_aligned, out_aligned;                  // in / out is 16-byte aligned
};

struct CanProjArgs {
  const CanSat* sats;
  CanSeg* segs;
  double2* amps;                                // A per segment, fp64
  const void* in;                               // input sample in_first
  long long in_first;
  unsigned nseg;
};

template <bool INC>
__global__ __launch_bounds__(kCanBlock) void cancel_project_kernel(const CanProjArgs a) {
  __shared__ double s_red[3][kCanBlock / 16];
  __shared__ double s_sum[3];
  const int tid = threadIdx.x;
  for (unsigned gi = blockIdx.x; gi < a.nseg; gi += gridDim.x) {
    const CanSeg g = a.segs[gi];
    if (!(g.sat_touch >> 8)) continue;                            // the same for the whole workgroup
    const CanSat s = a.sats[g.sat_touch & 0xffu];
    const long long off = g.s0 - a.in_first;
    double acc[3] = {0.0, 0.0, 0.0};
    unsigned chip_at = ~0u, cbit = 0u;
    for (unsigned u = tid; u < g.n; u += kCanBlock) {
      float xr, xi;
      if (INC) {
        const float2 x = reinterpret_cast<const float2*>(a.in)[off + u];
        xr = x.x;
        xi = x.y;
      } else {
        const int8_t* x = reinterpret_cast<const int8_t*>(a.in) + 2 * (off + u);
        xr = (float)x[0];
        xi = (float)x[1];
      }
      float rr, ri, w;
      cancel_replica(s, g, u, chip_at, cbit, rr, ri, w);
      const float pr = xr * rr + xi * ri, pi = xi * rr - xr * ri, ww = w * w;      // x conj(r), fp32
      acc[0] = acc[0] + (double)pr;
      acc[1] = acc[1] + (double)pi;
      acc[2] = acc[2] + (double)ww;
    }
    // row sums by DPP (lanes 0, 16, 32, 48 of each wave), then through LDS in a fixed order, as track_loop_kernel has it
#pragma unroll
    for (int t = 0; t < 3; t++) {
      double v = acc[t];
      v += gacq::f64::dpp_f64(v, 0);
      v += gacq::f64::dpp_f64(v, 1);
      v += gacq::f64::dpp_f64(v, 2);
      v += gacq::f64::dpp_f64(v, 3);
      acc[t] = v;
    }
    if ((tid & 15) == 0)
      for (int t = 0; t < 3; t++) s_red[t][tid >> 4] = acc[t];
    __syncthreads();
    if (tid < 3) {
      double sum = 0.0;
      for (int w = 0; w < kCanBlock / 64; w++)
        sum = sum + ((s_red[tid][4 * w] + s_red[tid][4 * w + 1]) + (s_red[tid][4 * w + 2] + s_red[tid][4 * w + 3]));
      s_sum[tid] = sum;
    }
    __syncthreads();
    if (tid == 0) {
      const double e = s_sum[2];
      const double are = e == 0.0 ? 0.0 : s_sum[0] / e, aim = e == 0.0 ? 0.0 : s_sum[1] / e;
      a.amps[gi] = make_double2(are, aim);
      a.segs[gi].ar = (float)are;
      a.segs[gi].ai = (float)aim;
    }
    __syncthreads();                                              // s_red and s_sum are free again
  }
}

template <bool INC, bool OUTC>
__global__ __launch_bounds__(kCanBlock) void cancel_subtract_kernel(const CanArgs a) {
  __shared__ unsigned s_first[kCanMaxK];
  const int tid = threadIdx.x;
  const long long ntiles = (a.n + kCanTile - 1) / kCanTile;
  const CanSeg* __restrict__ segs = a.segs;
  unsigned nclip = 0u;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long tile_j = a.out_first + t * kCanTile;
    __syncthreads();
    if (tid < a.K) {                                              // the first segment of satellite tid that ends after the tile's first sample
      const CanSat s = a.sats[tid];
      unsigned lo = s.first, hi = s.first + s.nseg;
      while (lo < hi) {
        const unsigned mid = lo + (hi - lo) / 2u;
        if (segs[mid].s0 + (long long)segs[mid].n <= tile_j) lo = mid + 1u;
        else hi = mid;
      }
      s_first[tid] = lo;
    }
    __syncthreads();
    const long long m = t * kCanTile + (long long)tid * kCanRun;  // offset from out_first
    if (m >= a.n) continue;
    const long long left = a.n - m, j0 = a.out_first + m;
    float vr[kCanRun], vi[kCanRun];
    if (INC) {
      const float2* __restrict__ p = reinterpret_cast<const float2*>(a.in) + m;
      if (left >= kCanRun && a.in_aligned) {
#pragma unroll
        for (int i = 0; i < kCanRun; i += 2) {
          const float4 q = reinterpret_cast<const float4*>(p)[i / 2];
          vr[i] = q.x; vi[i] = q.y; vr[i + 1] = q.z; vi[i + 1] = q.w;
        }
      } else {
#pragma unroll
        for (int i = 0; i < kCanRun; i++) {
          const float2 q = i < left ? p[i] : make_float2(0.0f, 0.0f);
          vr[i] = q.x; vi[i] = q.y;
        }
      }
    } else {
      const int8_t* __restrict__ p = reinterpret_cast<const int8_t*>(a.in) + 2 * m;
      if (left >= kCanRun && a.in_aligned) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < kCanRun; i++) {
          vr[i] = (float)(int)(int8_t)(w[i / 2] >> (16 * (i & 1)));
          vi[i] = (float)(int)(int8_t)(w[i / 2] >> (16 * (i & 1) + 8));
        }
      } else {
#pragma unroll
        for (int i = 0; i < kCanRun; i++) {
          vr[i] = i < left ? (float)p[2 * i] : 0.0f;
          vi[i] = i < left ? (float)p[2 * i + 1] : 0.0f;
        }
      }
    }
    for (int k = 0; k < a.K; k++) {
      const CanSat s = a.sats[k];                                 // the same address in every lane
      unsigned g = s_first[k];
      const unsigned gend = s.first + s.nseg;
      while (g < gend && segs[g].s0 + (long long)segs[g].n <= j0) g++;      // on to the run: the tile's segments only
      if (g >= gend) continue;
      CanSeg sg = segs[g];
      if (sg.s0 >= j0 + kCanRun) continue;
      long long rel = j0 - sg.s0;                                 // i of the run's first sample; negative before the segment
      bool live = true;
      unsigned chip_at = ~0u, cbit = 0u;
#pragma unroll
      for (int i = 0; i < kCanRun; i++) {
        if (live && rel + i >= (long long)sg.n) {                 // a boundary inside the run: at most one per sample
          g++;
          live = g < gend;
          if (live) {
            sg = segs[g];
            rel = j0 - sg.s0;
          }
        }
        if (live && rel + i >= 0) {
          float rr, ri, w;
          cancel_replica(s, sg, (unsigned)(rel + i), chip_at, cbit, rr, ri, w);
          const float tr = sg.ar * rr - sg.ai * ri, ti = sg.ar * ri + sg.ai * rr;      // float32(A) r
          vr[i] = vr[i] - tr;
          vi[i] = vi[i] - ti;
        }
      }
    }
    if (OUTC) {
      float2* __restrict__ o = reinterpret_cast<float2*>(a.out) + m;
      if (left >= kCanRun && a.out_aligned) {
#pragma unroll
        for (int i = 0; i < kCanRun; i += 2) reinterpret_cast<float4*>(o)[i / 2] = make_float4(vr[i], vi[i], vr[i + 1], vi[i + 1]);
      } else {
#pragma unroll
        for (int i = 0; i < kCanRun; i++)
          if (i < left) o[i] = make_float2(vr[i], vi[i]);
      }
    } else {
      unsigned b[2 * kCanRun];
#pragma unroll
      for (int i = 0; i < kCanRun; i++) {
        const int qr = (int)fminf(fmaxf(rintf(vr[i]), -127.0f), 127.0f), qi = (int)fminf(fmaxf(rintf(vi[i]), -127.0f), 127.0f);      // rintf: half to even
        b[2 * i] = (unsigned)qr & 0xffu;
        b[2 * i + 1] = (unsigned)qi & 0xffu;
        if (i < left) nclip += (qr == 127 || qr == -127 ? 1u : 0u) + (qi == 127 || qi == -127 ? 1u : 0u);
      }
      uint8_t* __restrict__ o = reinterpret_cast<uint8_t*>(a.out) + 2 * m;
      if (left >= kCanRun && a.out_aligned) {
        uint4 w;
        w.x = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        w.y = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
        w.z = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
        w.w = b[12] | (b[13] << 8) | (b[14] << 16) | (b[15] << 24);
        *reinterpret_cast<uint4*>(o) = w;
      } else {
#pragma unroll
        for (int i = 0; i < kCanRun; i++)
          if (i < left) {
            o[2 * i] = (uint8_t)b[2 * i];
            o[2 * i + 1] = (uint8_t)b[2 * i + 1];
          }
      }
    }
  }
  if (!OUTC && a.clip) {                                          // an integer count: the order of the additions does not matter
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nclip += __shfl_down(nclip, o);
    if ((tid & 63) == 0 && nclip) atomicAdd(a.clip, (unsigned long long)nclip);
  }
}

}  // namespace

namespace {

bool can_touches(const gacq_cancel_seg& g, long long out_first, long long n_out) { return g.s0 < out_first + n_out && g.s0 + g.n > out_first; }

// every check of the call; Ls (NULL or K ints) receives the code lengths
int can_check(const gacq_cancel_sat* sats, int K, const gacq_cancel_seg* segs, double fs, int estimate, const void* d_in, int in_complex64,
              long long in_first, long long in_count, long long out_first, long long n_out, int out_complex64, const void* d_out, int* Ls) {
  if (!sats || !segs || !d_in || !d_out) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_cancel: NULL argument");
  if (const int rc = can_check_rate("gacq_cancel", K, fs)) return rc;
  if (const int rc = st_check_range(nullptr, "gacq_cancel", in_first, in_count, out_first, n_out)) return rc;
  if (in_complex64 && (uintptr_t)d_in % 8u) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_cancel: complex64 input must be 8-byte aligned");
  if (out_complex64 && (uintptr_t)d_out % 8u) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_cancel: complex64 output must be 8-byte aligned");
  long long total = 0;
  if (const int rc = can_check_table("gacq_cancel", sats, K, segs, fs, true, Ls, &total)) return rc;
  if (n_out == 0) return GACQ_OK;
  if (out_first < in_first || out_first + n_out > in_first + in_count)
    return set_error(nullptr, GACQ_ERR_SHORT_INPUT, "gacq_cancel: outputs %lld .. %lld need their inputs, present are %lld .. %lld", out_first,
                     out_first + n_out - 1, in_first, in_first + in_count - 1);
  if (estimate)
    for (long long i = 0; i < total; i++)
      if (can_touches(segs[i], out_first, n_out) && (segs[i].s0 < in_first || segs[i].s0 + segs[i].n > in_first + in_count))
        return set_error(nullptr, GACQ_ERR_SHORT_INPUT, "gacq_cancel: segment %lld (samples %lld .. %lld) is estimated on inputs that are not present (%lld .. %lld)",
                         i, segs[i].s0, segs[i].s0 + segs[i].n - 1, in_first, in_first + in_count - 1);
  return GACQ_OK;
}

}  // namespace

extern "C" int gacq_cancel_check(const gacq_cancel_sat* sats, int K, const gacq_cancel_seg* segs, double fs, int estimate, const void* d_in,
                                 int in_complex64, long long in_first, long long in_count, long long out_first, long long n_out, int out_complex64,
                                 const void* d_out) {
  return can_check(sats, K, segs, fs, estimate, d_in, in_complex64, in_first, in_count, out_first, n_out, out_complex64, d_out, nullptr);
}

extern "C" int gacq_cancel_dev(gacq_ctx* ctx, const gacq_cancel_sat* sats, int K, const gacq_cancel_seg* segs, double fs, int estimate, const void* d_in,
                               int in_complex64, long long in_first, long long in_count, long long out_first, long long n_out, int out_complex64,
                               void* d_out, double* amps_out, unsigned long long* clipped) {
  if (!ctx) return GACQ_ERR_BAD_ARG;
  // everything is checked before anything is allocated or launched
  int Ls[kCanMaxK];
  int rc = can_check(sats, K, segs, fs, estimate, d_in, in_complex64, in_first, in_count, out_first, n_out, out_complex64, d_out, Ls);
  if (rc < 0) return st_forward(ctx, rc);
  if (n_out == 0) return GACQ_OK;
  GACQ_DEVICE(ctx);
  hipStream_t stream = ctx->stream;
  CanTable tab;
  if ((rc = can_table_build(ctx, "gacq_cancel_dev", sats, K, segs, Ls, fs, [&](const gacq_cancel_seg& g) { return can_touches(g, out_first, n_out); },
                            tab)) != GACQ_OK)
    return rc;
  const size_t S = tab.S;
  const bool any = tab.any;
  const std::vector<CanSeg>& hg = tab.segs;
  DevBuf& d_amps = ctx->tables["cancel:amps"];
  if ((rc = ensure(ctx, d_amps, sizeof(double2) * hg.size() + 8)) != GACQ_OK) return rc;
  unsigned long long* d_clip = (unsigned long long*)((double2*)d_amps.p + hg.size());
  // the uploads come from pageable memory and the downloads go to it: the stream is waited for on every way out from here on
  const size_t esz = in_complex64 ? 8 : 2;
  std::vector<double2> ha(amps_out && estimate && any ? S : 0);
  unsigned long long nclip = 0;
  const auto queue = [&]() -> hipError_t {
    hipError_t e = can_table_queue(tab, stream);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(d_clip, 0, 8, stream)) != hipSuccess) return e;
    if (estimate && any) {
      CanProjArgs p;
      p.sats = tab.d_sats;
      p.segs = tab.d_segs;
      p.amps = (double2*)d_amps.p;
      p.in = d_in;
      p.in_first = in_first;
      p.nseg = (unsigned)S;
      const unsigned grid = std::min((unsigned)S, kCanMaxGrid);
      if (in_complex64) hipLaunchKernelGGL((cancel_project_kernel<true>), dim3(grid), dim3(kCanBlock), 0, stream, p);
      else hipLaunchKernelGGL((cancel_project_kernel<false>), dim3(grid), dim3(kCanBlock), 0, stream, p);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    CanArgs a;
    a.sats = tab.d_sats;
    a.segs = tab.d_segs;
    a.in = (const unsigned char*)d_in + (size_t)(out_first - in_first) * esz;
    a.out = d_out;
    a.clip = d_clip;
    a.out_first = out_first;
    a.n = n_out;
    a.K = K;
    a.in_aligned = ((uintptr_t)a.in % 16u) == 0u;
    a.out_aligned = ((uintptr_t)d_out % 16u) == 0u;
    const long long ntiles = (n_out + kCanTile - 1) / kCanTile;
    const unsigned grid = (unsigned)std::min<long long>(ntiles, (long long)kCanMaxGrid);
    if (in_complex64) {
      if (out_complex64) hipLaunchKernelGGL((cancel_subtract_kernel<true, true>), dim3(grid), dim3(kCanBlock), 0, stream, a);
      else hipLaunchKernelGGL((cancel_subtract_kernel<true, false>), dim3(grid), dim3(kCanBlock), 0, stream, a);
    } else {
      if (out_complex64) hipLaunchKernelGGL((cancel_subtract_kernel<false, true>), dim3(grid), dim3(kCanBlock), 0, stream, a);
      else hipLaunchKernelGGL((cancel_subtract_kernel<false, false>), dim3(grid), dim3(kCanBlock), 0, stream, a);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (!ha.empty() && (e = hipMemcpyAsync(ha.data(), d_amps.p, sizeof(double2) * S, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    if (clipped) e = hipMemcpyAsync(&nclip, d_clip, 8, hipMemcpyDeviceToHost, stream);
    return e;
  };
  const hipError_t eq = queue(), es = hipStreamSynchronize(stream);
  if (eq != hipSuccess || es != hipSuccess)
    return set_error(ctx, GACQ_ERR_HIP, "gacq_cancel_dev: %s", hipGetErrorString(eq != hipSuccess ? eq : es));
  if (amps_out)
    for (size_t i = 0; i < S; i++)
      if (hg[i].sat_touch >> 8) {
        amps_out[2 * i] = estimate ? ha[i].x : segs[i].amp_re;
        amps_out[2 * i + 1] = estimate ? ha[i].y : segs[i].amp_im;
      }
  if (clipped) *clipped = nclip;
  return GACQ_OK;
}
