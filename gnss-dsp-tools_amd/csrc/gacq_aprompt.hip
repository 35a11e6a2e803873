// Prompts of tracked signals across an antenna array (gacq_aprompt_dev, include/gacq.h): the projection A = sum x conj(r) / sum w^2 of
// gacq_cancel_dev's estimate, of M recordings on one sample clock at once.  The replica of a sample -- a 64-bit phase, a chip lookup, a
// sine / cosine polynomial: cancel_replica of gacq_cancelcore.h, the one gacq_cancel.hip calls -- is built once and multiplied into all
// M antennas.
//   aprompt_project_kernel<INC, M>   one workgroup of 256 per segment that lies wholly inside the input; sample i goes to lane i mod 256,
//                                    a lane adds its fp32 products in ascending i into 2 M + 1 fp64 sums held in registers (re and im
//                                    per antenna, then w^2); each sum goes through the DPP row sums and the fixed LDS tree of
//                                    cancel_project_kernel.  A sum of antenna p sees the samples of antenna p alone, in the order and
//                                    with the operations of that kernel: the bits of A_p are those gacq_cancel_dev returns on antenna
//                                    p's recording, whatever M, the other rows, the other segments and the addresses are.
// M is a compile-time parameter (the sums are indexed at compile time) in 1, 2, 4, 8; another number of antennas runs the next larger
// form with row 0 repeated in the spare places, whose sums are not written.
#pragma clang fp contract(off)

#include "gacq_cancelcore.h"
#include "gacq_fft64.h"

using namespace gacq;

namespace {

constexpr int kAprMaxM = 8;

struct AprArgs {
  const CanSat* sats;
  const CanSeg* segs;
  const void* in[kAprMaxM];                     // input sample in_first of every antenna; the spare ones repeat antenna 0
  double2* prompts;                             // [segment][m]
  double* energy;                               // [segment]
  long long in_first;
  unsigned nseg;
  int m;                                        // antennas whose results are written, <= M
};

template <bool INC, int M>
__global__ __launch_bounds__(kCanBlock) void aprompt_project_kernel(const AprArgs a) {
  constexpr int kSums = 2 * M + 1;
  __shared__ double s_red[kSums][kCanBlock / 16];
  __shared__ double s_sum[kSums];
  const int tid = threadIdx.x;
  for (unsigned gi = blockIdx.x; gi < a.nseg; gi += gridDim.x) {
    const CanSeg g = a.segs[gi];
    if (!(g.sat_touch >> 8)) continue;                            // the same for the whole workgroup
    const CanSat s = a.sats[g.sat_touch & 0xffu];
    const long long off = g.s0 - a.in_first;
    double acc[kSums];
#pragma unroll
    for (int t = 0; t < kSums; t++) acc[t] = 0.0;
    unsigned chip_at = ~0u, cbit = 0u;
    for (unsigned u = tid; u < g.n; u += kCanBlock) {
      float xr[M], xi[M];
#pragma unroll
      for (int p = 0; p < M; p++) {
        if (INC) {
          const float2 x = reinterpret_cast<const float2*>(a.in[p])[off + u];
          xr[p] = x.x;
          xi[p] = x.y;
        } else {
          const int8_t* x = reinterpret_cast<const int8_t*>(a.in[p]) + 2 * (off + u);
          xr[p] = (float)x[0];
          xi[p] = (float)x[1];
        }
      }
      float rr, ri, w;
      cancel_replica(s, g, u, chip_at, cbit, rr, ri, w);
      const float ww = w * w;
#pragma unroll
      for (int p = 0; p < M; p++) {
        const float pr = xr[p] * rr + xi[p] * ri, pi = xi[p] * rr - xr[p] * ri;      // x conj(r), fp32
        acc[2 * p] = acc[2 * p] + (double)pr;
        acc[2 * p + 1] = acc[2 * p + 1] + (double)pi;
      }
      acc[2 * M] = acc[2 * M] + (double)ww;
    }
    // cancel_project_kernel's reduction, sum by sum: DPP row sums (lanes 0, 16, 32, 48 of each wave), then LDS in a fixed order
#pragma unroll
    for (int t = 0; t < kSums; t++) {
      double v = acc[t];
      v += gacq::f64::dpp_f64(v, 0);
      v += gacq::f64::dpp_f64(v, 1);
      v += gacq::f64::dpp_f64(v, 2);
      v += gacq::f64::dpp_f64(v, 3);
      acc[t] = v;
    }
    if ((tid & 15) == 0) {
#pragma unroll
      for (int t = 0; t < kSums; t++) s_red[t][tid >> 4] = acc[t];
    }
    __syncthreads();
    if (tid < kSums) {
      double sum = 0.0;
      for (int w = 0; w < kCanBlock / 64; w++)
        sum = sum + ((s_red[tid][4 * w] + s_red[tid][4 * w + 1]) + (s_red[tid][4 * w + 2] + s_red[tid][4 * w + 3]));
      s_sum[tid] = sum;
    }
    __syncthreads();
    if (tid < a.m) {
      const double e = s_sum[2 * M];
      const double are = e == 0.0 ? 0.0 : s_sum[2 * tid] / e, aim = e == 0.0 ? 0.0 : s_sum[2 * tid + 1] / e;
      a.prompts[(size_t)gi * (size_t)a.m + (size_t)tid] = make_double2(are, aim);
      if (tid == 0) a.energy[gi] = e;
    }
    __syncthreads();                                              // s_red and s_sum are free again
  }
}

template <bool INC>
void apr_launch(int M, unsigned grid, hipStream_t stream, const AprArgs& a) {
  if (M == 1) hipLaunchKernelGGL((aprompt_project_kernel<INC, 1>), dim3(grid), dim3(kCanBlock), 0, stream, a);
  else if (M == 2) hipLaunchKernelGGL((aprompt_project_kernel<INC, 2>), dim3(grid), dim3(kCanBlock), 0, stream, a);
  else if (M <= 4) hipLaunchKernelGGL((aprompt_project_kernel<INC, 4>), dim3(grid), dim3(kCanBlock), 0, stream, a);
  else hipLaunchKernelGGL((aprompt_project_kernel<INC, 8>), dim3(grid), dim3(kCanBlock), 0, stream, a);
}

bool apr_inside(const gacq_cancel_seg& g, long long in_first, long long in_count) { return g.s0 >= in_first && g.s0 + g.n <= in_first + in_count; }

// every check of the call; Ls (NULL or K ints) receives the code lengths
int apr_check(const gacq_cancel_sat* sats, int K, const gacq_cancel_seg* segs, double fs, const void* const* d_in, int antennas, int in_complex64,
              long long in_first, long long in_count, int* Ls) {
  if (!sats || !segs || !d_in) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_aprompt: NULL argument");
  if (const int rc = can_check_rate("gacq_aprompt", K, fs)) return rc;
  if (const int rc = st_check_range(nullptr, "gacq_aprompt", in_first, in_count, 0, 0)) return rc;
  if (antennas < 1 || antennas > kAprMaxM)
    return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_aprompt: %d antennas: need 1..%d", antennas, kAprMaxM);
  for (int p = 0; p < antennas; p++) {
    if (!d_in[p]) return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_aprompt: the pointer of antenna %d is NULL", p);
    if (in_complex64 && (uintptr_t)d_in[p] % 8u)
      return set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_aprompt: complex64 input must be 8-byte aligned (antenna %d)", p);
  }
  return can_check_table("gacq_aprompt", sats, K, segs, fs, false, Ls, nullptr);
}

}  // namespace

extern "C" int gacq_aprompt_check(const gacq_cancel_sat* sats, int K, const gacq_cancel_seg* segs, double fs, const void* const* d_in, int antennas,
                                  int in_complex64, long long in_first, long long in_count) {
  return apr_check(sats, K, segs, fs, d_in, antennas, in_complex64, in_first, in_count, nullptr);
}

extern "C" int gacq_aprompt_dev(gacq_ctx* ctx, const gacq_cancel_sat* sats, int K, const gacq_cancel_seg* segs, double fs, const void* const* d_in,
                                int antennas, int in_complex64, long long in_first, long long in_count, double* prompts_out, double* energy_out) {
  if (!ctx) return GACQ_ERR_BAD_ARG;
  // everything is checked before anything is allocated or launched
  int Ls[kCanMaxK];
  int rc = apr_check(sats, K, segs, fs, d_in, antennas, in_complex64, in_first, in_count, Ls);
  if (rc < 0) return st_forward(ctx, rc);
  if (!prompts_out) return set_error(ctx, GACQ_ERR_BAD_ARG, "gacq_aprompt_dev: prompts_out is NULL");
  GACQ_DEVICE(ctx);
  hipStream_t stream = ctx->stream;
  CanTable tab;
  if ((rc = can_table_build(ctx, "gacq_aprompt_dev", sats, K, segs, Ls, fs, [&](const gacq_cancel_seg& g) { return apr_inside(g, in_first, in_count); },
                            tab)) != GACQ_OK)
    return rc;
  if (!tab.any) return GACQ_OK;                                     // no segment wholly inside the input
  const size_t S = tab.S, m = (size_t)antennas;
  DevBuf& d_res = ctx->tables["aprompt:out"];
  if ((rc = ensure(ctx, d_res, sizeof(double) * S * (2 * m + 1))) != GACQ_OK) return rc;
  std::vector<double> hr(S * (2 * m + 1));                          // prompts [S][m][2], then the energies [S]
  AprArgs a;
  a.sats = tab.d_sats;
  a.segs = tab.d_segs;
  for (int p = 0; p < kAprMaxM; p++) a.in[p] = d_in[p < antennas ? p : 0];
  a.prompts = (double2*)d_res.p;
  a.energy = (double*)d_res.p + S * 2 * m;
  a.in_first = in_first;
  a.nseg = (unsigned)S;
  a.m = antennas;
  // the uploads come from pageable memory and the download goes to it: the stream is waited for on every way out from here on
  const auto queue = [&]() -> hipError_t {
    hipError_t e = can_table_queue(tab, stream);
    if (e != hipSuccess) return e;
    const unsigned grid = std::min((unsigned)S, kCanMaxGrid);
    if (in_complex64) apr_launch<true>(antennas, grid, stream, a);
    else apr_launch<false>(antennas, grid, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return hipMemcpyAsync(hr.data(), d_res.p, sizeof(double) * hr.size(), hipMemcpyDeviceToHost, stream);
  };
  const hipError_t eq = queue(), es = hipStreamSynchronize(stream);
  if (eq != hipSuccess || es != hipSuccess)
    return set_error(ctx, GACQ_ERR_HIP, "gacq_aprompt_dev: %s", hipGetErrorString(eq != hipSuccess ? eq : es));
  for (size_t i = 0; i < S; i++)
    if (tab.segs[i].sat_touch >> 8) {
      std::memcpy(prompts_out + i * 2 * m, hr.data() + i * 2 * m, sizeof(double) * 2 * m);
      if (energy_out) energy_out[i] = hr[S * 2 * m + i];
    }
  return GACQ_OK;
}
