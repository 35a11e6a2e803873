// Bearings of interferers from array covariances (gacq_bearing_*, include/gacq.h): the minimum-variance (Capon) quadratic form
// q_g = a_g^H A^-1 a_g of every block's loaded window covariance over a grid of G directions, and the K smallest q (the strongest Capon
// powers 1 / q) among cells that lie apart.  The covariance is the exact int64 d_cov of gacq_null_run_dev and every q is one written-out
// fp64 sequence, so every output bit is a function of (configuration, tables, covariance) alone.
//
// Two launches per chunk of blocks, on one stream:
//   bearing_factor_kernel    a wave per block, lane 8 r + c holds A[r][c] as in null_weights_kernel: the loading and the elimination of
//      the matrix are that kernel's own functions (ar_load_diagonal, ar_eliminate of gacq_arraycore.h, which also holds the bounds on
//      the antennas and the shift), so the matrix factored here is the matrix nulling solves.  What a cell needs of it goes to the
//      workspace, 64 pairs of doubles a block: the multiplier m = A[r][k] / piv_k at [r][k], r > k, and (piv_k, 0) at [k][k].  None of
//      that depends on the cell.
//   bearing_spectrum_kernel  one workgroup of 256 lanes per block; lane t owns the cells g = t, t + 256, ..  The block's factor is read
//      once into 1 KB of LDS and every use is a broadcast read; a_g comes from the planar copy [p][re|im][g] of the table that
//      gacq_bearing_open made, so a wave reads 512 consecutive bytes per component; b stays in registers (the antennas are a
//      compile-time count: one body per M inside the kernel, chosen by a uniform switch).  Forward elimination of b, the M squared
//      magnitudes over the pivots, the sum left to right: the cell's q.
//      Between the K ranks a block's q live in a global row of the workspace (G doubles; 32768 of them do not fit the 20480 doubles
//      of LDS, and a row a workgroup that large would leave one workgroup a compute unit; at the sizes of a 5 or 2 degree grid the row
//      is 11 or 65 KB and stays in the cache it was written through).  A lane reads and writes only its own cells there, so the
//      rounds need no fence.  The row holds q where the cell is eligible and +inf where not; a round that excludes a cell stores
//      +inf, which no eligible q equals.  Rank 0 and the floor are reduced from registers during the evaluation; each later rank is
//      one pass over the row and the planar u table: exclude by the rank before, take the smallest of what is left.
//      Every reduction carries (q, g) and compares q first and g second: lane, wave (shuffles), workgroup (LDS) give the same pair in
//      any order.
#pragma clang fp contract(off)

#include "gacq_arraycore.h"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace gacq;

namespace {

constexpr int kBrBlock = 256;                        // threads a workgroup
constexpr int kBrMinM = 2, kBrMaxCells = 32768, kBrMaxPeaks = 4;      // at most kArMaxM antennas, load_shift at most kArMaxShift
constexpr long long kBrMaxChunk = 1ll << 14;         // blocks a pair of launches evaluates, at most
constexpr long long kBrRowDoubles = 1ll << 24;       // doubles of the q rows of a chunk, at most (128 MiB)
constexpr long long kBrMaxIndex = 1ll << 48;
constexpr int kBrNoCell = 0x7fffffff;

struct BrFactorArgs {
  const long long* cov;         // row 0 of the launch: [..][M][M][2]
  double2* F;                   // [block][8][8]
  long long stride;             // rows from one block to the next
  int nblk, M, shift;
};

__global__ __launch_bounds__(kBrBlock) void bearing_factor_kernel(const BrFactorArgs a) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (kBrBlock / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (i >= a.nblk) return;
  const int r = lane >> 3, c = lane & 7, M = a.M;
  const bool in = r < M && c < M;
  long long Rre = 0, Rim = 0;
  if (in) {
    const long long* pr = a.cov + ((i * a.stride * M + r) * M + c) * 2;
    Rre = pr[0];
    Rim = pr[1];
  }
  // ---- the loading and the elimination of nulling (gacq_arraycore.h); a lane below the diagonal is left with the numerator of its
  // multiplier
  double Are, Aim;
  ar_load_diagonal(Rre, Rim, a.shift, M, r, c, Are, Aim);
  ar_eliminate(Are, Aim, M, r, c);
  const double piv = __shfl(Are, 9 * c, 64);          // of the lane's column
  double2 f = make_double2(0.0, 0.0);
  if (in && r > c) f = make_double2(Are / piv, Aim / piv);
  if (in && r == c) f = make_double2(Are, 0.0);
  a.F[64 * (long long)i + lane] = f;
}

struct BrPeak {                 // 16 bytes on an 8-byte boundary
  int g, zero;
  double q;
};

struct BrSpecArgs {
  const double2* F;             // [block][8][8]
  const double* a;              // planar [M][2][G]
  const double* u;              // planar [3][G]
  double* row;                  // [block][G]: the q of the cells still in the running, +inf elsewhere
  double* spectrum;             // the launch's block 0, or NULL
  BrPeak* peaks;                // [block][K]
  double* floor;
  double cos_sep;
  int G, M, K;
};

__device__ __forceinline__ bool br_better(double q, int g, double q2, int g2) { return q < q2 || (q == q2 && g < g2); }

// the smallest (q, g) of the workgroup in every lane; red holds a pair per wave
__device__ __forceinline__ void br_argmin(double& q, int& g, double* red_q, int* red_g) {
  for (int off = 1; off < 64; off <<= 1) {
    const double q2 = __shfl_xor(q, off, 64);
    const int g2 = __shfl_xor(g, off, 64);
    if (br_better(q2, g2, q, g)) q = q2, g = g2;
  }
  const int wave = threadIdx.x >> 6;
  __syncthreads();                                   // the pairs of the round before have been read
  if ((threadIdx.x & 63) == 0) red_q[wave] = q, red_g[wave] = g;
  __syncthreads();
  q = red_q[0], g = red_g[0];
#pragma unroll
  for (int w = 1; w < kBrBlock / 64; w++)
    if (br_better(red_q[w], red_g[w], q, g)) q = red_q[w], g = red_g[w];
}

// The q of the lane's cells for M antennas: into the row (and the spectrum), the lane's smallest eligible (q, g) and largest eligible q
template <int M>
__device__ __forceinline__ void br_evaluate(const BrSpecArgs& a, const double2* F, double* row, double* spec, double& best_q, int& best_g,
                                            double& top) {
  const int G = a.G;
  for (int g = threadIdx.x; g < G; g += kBrBlock) {
    // the factor is read from LDS in every pass: without this the compiler lifts its 128 dwords out of the loop and spills them
    asm volatile("" ::: "memory");
    double bre[M], bim[M];
#pragma unroll
    for (int p = 0; p < M; p++) {
      bre[p] = a.a[(long long)(2 * p) * G + g];
      bim[p] = a.a[(long long)(2 * p + 1) * G + g];
    }
    double q = 0.0;
#pragma unroll
    for (int k = 0; k < M; k++) {
#pragma unroll
      for (int r = k + 1; r < M; r++) {
        const double2 m = F[8 * r + k];
        bre[r] = bre[r] - (m.x * bre[k] - m.y * bim[k]);
        bim[r] = bim[r] - (m.x * bim[k] + m.y * bre[k]);
      }
      const double tk = (bre[k] * bre[k] + bim[k] * bim[k]) / F[9 * k].x;
      q = k == 0 ? tk : q + tk;
    }
    if (spec) spec[g] = q != q ? __longlong_as_double(0x7ff8000000000000ll) : q;     // IEEE leaves a NaN's sign and payload open
    const bool ok = __builtin_isfinite(q) && q > 0.0;
    row[g] = ok ? q : __builtin_inf();
    if (ok) {
      if (q < best_q) best_q = q, best_g = g;         // g ascends: the first of equal q stays
      top = fmax(top, q);
    }
  }
}

// four workgroups a compute unit at the least: with 128 registers a wave the factor is read from LDS where it is used (with all 512 in
// reach the compiler keeps its 128 dwords in registers across the cell loop, one wave a SIMD)
__global__ __launch_bounds__(kBrBlock, 4) void bearing_spectrum_kernel(const BrSpecArgs a) {
  __shared__ double2 F[64];
  __shared__ double red_q[kBrBlock / 64];
  __shared__ int red_g[kBrBlock / 64];
  const int tid = threadIdx.x, G = a.G;
  const long long blk = blockIdx.x;
  if (tid < 64) F[tid] = a.F[64 * blk + tid];
  __syncthreads();
  double* row = a.row + blk * G;
  double* spec = a.spectrum ? a.spectrum + blk * G : nullptr;
  double best_q = __builtin_inf(), top = -__builtin_inf();
  int best_g = kBrNoCell;
  switch (a.M) {
    case 2: br_evaluate<2>(a, F, row, spec, best_q, best_g, top); break;
    case 3: br_evaluate<3>(a, F, row, spec, best_q, best_g, top); break;
    case 4: br_evaluate<4>(a, F, row, spec, best_q, best_g, top); break;
    case 5: br_evaluate<5>(a, F, row, spec, best_q, best_g, top); break;
    case 6: br_evaluate<6>(a, F, row, spec, best_q, best_g, top); break;
    case 7: br_evaluate<7>(a, F, row, spec, best_q, best_g, top); break;
    default: br_evaluate<8>(a, F, row, spec, best_q, best_g, top); break;
  }
  // ---- the floor: the largest eligible q, +inf when there is none
  for (int off = 1; off < 64; off <<= 1) top = fmax(top, __shfl_xor(top, off, 64));
  if ((tid & 63) == 0) red_q[tid >> 6] = top;
  __syncthreads();
  if (tid == 0) {
    double f = red_q[0];
    for (int w = 1; w < kBrBlock / 64; w++) f = fmax(f, red_q[w]);
    a.floor[blk] = f == -__builtin_inf() ? __builtin_inf() : f;
  }
  // ---- the ranks
  const double* ux = a.u;
  const double* uy = a.u + G;
  const double* uz = a.u + 2 * (long long)G;
  for (int k = 0; k < a.K; k++) {
    if (k > 0) {
      // best_g is rank k - 1, the same in every lane: its cells are out, and the smallest of the rest is this rank
      double q = __builtin_inf();
      int gq = kBrNoCell;
      if (best_g != kBrNoCell) {
        const double px = ux[best_g], py = uy[best_g], pz = uz[best_g];
        for (int g = tid; g < G; g += kBrBlock) {
          const double v = row[g];
          if (v == __builtin_inf()) continue;
          const double dot = (ux[g] * px + uy[g] * py) + uz[g] * pz;
          if (dot >= a.cos_sep) row[g] = __builtin_inf();
          else if (v < q) q = v, gq = g;
        }
      }
      best_q = q, best_g = gq;
    }
    br_argmin(best_q, best_g, red_q, red_g);
    if (tid == 0) {
      BrPeak* o = a.peaks + blk * a.K + k;
      *reinterpret_cast<int2*>(o) = make_int2(best_g == kBrNoCell ? -1 : best_g, 0);
      o->q = best_q;
    }
  }
}

}  // namespace

#include "gacq_streamhost.h"

struct gacq_bearing {
  gacq_ctx* ctx = nullptr;
  gacq_bearing_cfg cfg{};
  long long chunk = 0;          // blocks a pair of launches evaluates
  StDevBlock dev;               // the planar a table, the planar u table, the factors of a chunk, its q rows
  size_t at_u = 0, at_F = 0, at_row = 0;
};

static int check_cfg(const gacq_bearing_cfg* c) {
  const char* who = "gacq_bearing";
  if (!c) return gacq::set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: NULL argument", who);
  if (c->antennas < kBrMinM || c->antennas > kArMaxM)
    return gacq::set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: %d antennas: need %d..%d", who, c->antennas, kBrMinM, kArMaxM);
  if (c->load_shift < 0 || c->load_shift > kArMaxShift)
    return gacq::set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: load_shift %d lies outside 0..%d", who, c->load_shift, kArMaxShift);
  if (c->cells < 1 || c->cells > kBrMaxCells)
    return gacq::set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: %d grid cells: need 1..%d", who, c->cells, kBrMaxCells);
  if (c->peaks < 1 || c->peaks > kBrMaxPeaks)
    return gacq::set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: %d peaks: need 1..%d", who, c->peaks, kBrMaxPeaks);
  if (!std::isfinite(c->cos_sep) || c->cos_sep < -1.0 || c->cos_sep > 1.0)
    return gacq::set_error(nullptr, GACQ_ERR_BAD_ARG, "%s: cos_sep %g lies outside -1..1", who, c->cos_sep);
  return GACQ_OK;
}

extern "C" int gacq_bearing_check(const gacq_bearing_cfg* cfg, long long n, long long stride) {
  const int rc = check_cfg(cfg);
  if (rc < 0) return rc;
  // n stride <= 2^48 without forming a product that could overflow
  if (n < 0 || stride < 1 || n > kBrMaxIndex || stride > kBrMaxIndex || (n > 0 && stride > kBrMaxIndex / n))
    return gacq::set_error(nullptr, GACQ_ERR_BAD_ARG, "gacq_bearing: need 0 <= n, 1 <= stride and n stride <= 2^48 (%lld, %lld)", n, stride);
  return GACQ_OK;
}

extern "C" int gacq_bearing_open(gacq_ctx* ctx, const gacq_bearing_cfg* cfg, const double* a, const double* u, gacq_bearing** out) {
  const char* who = "gacq_bearing_open";
  if (!ctx) return GACQ_ERR_BAD_ARG;
  if (!out) return gacq::set_error(ctx, GACQ_ERR_BAD_ARG, "%s: NULL argument", who);
  *out = nullptr;
  const int rc = gacq_bearing_check(cfg, 0, 1);
  if (rc < 0) return st_forward(ctx, rc);
  if (!a || !u) return gacq::set_error(ctx, GACQ_ERR_BAD_ARG, "%s: NULL argument", who);
  const long long G = cfg->cells, M = cfg->antennas;
  for (long long i = 0; i < G * M * 2; i++)
    if (!std::isfinite(a[i])) return gacq::set_error(ctx, GACQ_ERR_BAD_ARG, "%s: entry %lld of the steering table is not finite", who, i);
  for (long long i = 0; i < G * 3; i++)
    if (!std::isfinite(u[i])) return gacq::set_error(ctx, GACQ_ERR_BAD_ARG, "%s: entry %lld of the direction table is not finite", who, i);
  // the planar copies: a [p][re|im][g], u [x|y|z][g]
  std::vector<double> tab((size_t)(G * (2 * M + 3)));
  for (long long g = 0; g < G; g++) {
    for (long long p = 0; p < 2 * M; p++) tab[(size_t)(p * G + g)] = a[g * 2 * M + p];
    for (long long x = 0; x < 3; x++) tab[(size_t)((2 * M + x) * G + g)] = u[g * 3 + x];
  }
  std::unique_ptr<gacq_bearing> h(new gacq_bearing);
  h->ctx = ctx;
  h->cfg = *cfg;
  h->chunk = std::max(1ll, std::min(kBrMaxChunk, kBrRowDoubles / G));
  h->at_u = (size_t)(2 * M * G) * sizeof(double);
  h->at_F = (h->at_u + (size_t)(3 * G) * sizeof(double) + 15) / 16 * 16;
  h->at_row = h->at_F + (size_t)h->chunk * 64 * sizeof(double2);
  {
    GACQ_DEVICE(ctx);
    hipError_t e = h->dev.alloc(ctx, h->at_row + (size_t)(h->chunk * G) * sizeof(double));
    if (e == hipSuccess) e = h->dev.upload(0, tab.data(), tab.size() * sizeof(double));
    if (e != hipSuccess) return gacq::set_error(ctx, GACQ_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
  }
  *out = h.release();
  return GACQ_OK;
}

extern "C" void gacq_bearing_close(gacq_bearing* h) { delete h; }

extern "C" int gacq_bearing_run_dev(gacq_bearing* h, const void* d_cov, long long n, long long stride, void* d_peaks, void* d_floor,
                                    void* d_spectrum) {
  const char* who = "gacq_bearing_run_dev";
  if (!h) return GACQ_ERR_BAD_ARG;
  gacq_ctx* ctx = h->ctx;
  const gacq_bearing_cfg& c = h->cfg;
  int rc = gacq_bearing_check(&c, n, stride);
  if (rc < 0) return st_forward(ctx, rc);
  if (!d_cov || !d_peaks || !d_floor) return gacq::set_error(ctx, GACQ_ERR_BAD_ARG, "%s: NULL argument", who);
  if ((uintptr_t)d_cov % 8u || (uintptr_t)d_peaks % 8u || (uintptr_t)d_floor % 8u || (uintptr_t)d_spectrum % 8u)
    return gacq::set_error(ctx, GACQ_ERR_BAD_ARG, "%s: d_cov, d_peaks, d_floor and d_spectrum must be 8-byte aligned", who);
  if (n == 0) return GACQ_OK;
  const long long G = c.cells, M = c.antennas;
  char* base = (char*)h->dev.p;
  hipStream_t stream = ctx->stream;
  GACQ_DEVICE(ctx);
  for (long long i0 = 0; i0 < n; i0 += h->chunk) {
    const long long nb = std::min(h->chunk, n - i0);
    BrFactorArgs fa;
    fa.cov = (const long long*)d_cov + i0 * stride * M * M * 2;
    fa.F = (double2*)(base + h->at_F);
    fa.stride = stride;
    fa.nblk = (int)nb;
    fa.M = c.antennas;
    fa.shift = c.load_shift;
    hipLaunchKernelGGL(bearing_factor_kernel, dim3((unsigned)((nb + kBrBlock / 64 - 1) / (kBrBlock / 64))), dim3(kBrBlock), 0, stream, fa);
    if ((rc = st_launched(ctx, who)) < 0) return rc;
    BrSpecArgs sa;
    sa.F = fa.F;
    sa.a = (const double*)base;
    sa.u = (const double*)(base + h->at_u);
    sa.row = (double*)(base + h->at_row);
    sa.spectrum = d_spectrum ? (double*)d_spectrum + i0 * G : nullptr;
    sa.peaks = (BrPeak*)d_peaks + i0 * c.peaks;
    sa.floor = (double*)d_floor + i0;
    sa.cos_sep = c.cos_sep;
    sa.G = c.cells;
    sa.M = c.antennas;
    sa.K = c.peaks;
    hipLaunchKernelGGL(bearing_spectrum_kernel, dim3((unsigned)nb), dim3(kBrBlock), 0, stream, sa);
    if ((rc = st_launched(ctx, who)) < 0) return rc;
  }
  return GACQ_OK;
}
