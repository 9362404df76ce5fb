// sets.hip -- the set-level half of mgeval (the reference's music_evaluation/music_evaluator.py with mgeval/utils.py: c_dist, kl_dist,
// overlap_area): leave-one-out and inter-set Euclidean distances of per-sample statistics, and KL divergence / overlap area of the
// Gaussian-KDE densities (Scott's factor) of two distance vectors.  Definition, quirks and measurements: docs/rounds/sets.md, include/rgm.h.
//
//   rgm_set_distances   one launch, one thread per distance.
//   rgm_set_kl_oa       four launches:
//     stats     one workgroup per vector: minimum, maximum, mean, sum of squared deviations, bandwidth;
//     density   grid (point tiles, data chunks, 2 densities): a workgroup owns a tile of evaluation points (512, two per lane in registers;
//               64, one per lane, where the grid would be small) and walks ONE chunk of CHUNK data values through LDS, a slice of it (2048 / 512) at a time;
//               every (chunk, point) partial sum has one owner and does not depend on the tile shape;
//     fold      adds the chunks of a point in chunk order and scales: the two densities at their KL points and at the Simpson points;
//     finish    one workgroup: the two normalising sums, sum p log(p / q), Simpson's rule at `panels` and at `panels / 2`.
//   rgm_kde_pdf         stats, density and fold of one vector at the caller's points.
// Everything is float64 without FMA contraction.  (x - y) / h is formed directly, per pair.  CHUNK and the workgroup shapes are
// constants of the build, every sum has one owner and a fixed order (compensated where it is long), and there are no atomics: a result
// depends on its inputs alone and repeats bit for bit.  Everything runs on the caller's stream in the caller's workspace.
#include "common.h"

#pragma clang fp contract(off)

namespace rgm {
namespace sets {
constexpr int STAT_THREADS = 1024, CHUNK = 16384, SMALL_GRID = 1024;
constexpr int MAX_N = 1 << 24, MAX_KL = 4096, MAX_PANELS = 65536, MAX_M = 1 << 20, MAX_ROWS = 32768, MAX_D = 144;
constexpr double SQRT_2PI = 2.5066282746310002;

struct Stats {                                          // what the stats launch leaves per vector: 8 doubles
  double lo, hi, mean, var, h, den, degenerate, pad;    // den = n h sqrt(2 pi); degenerate: n < 2 or a variance that is not positive and finite
};

__host__ __device__ inline int n_chunks(int n) { return (n + CHUNK - 1) / CHUNK; }
__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// s += v with Kahan's compensation c: the long sums (n values per point, 16384 values per lane at n = 2^24) stay within a few ulp
__device__ __forceinline__ void kahan(double& s, double& c, double v) {
  const double y = v - c, t = s + y;
  c = (t - s) - y;
  s = t;
}

// OP 0: sum, 1: minimum, 2: maximum.  A fixed shuffle tree per wave, then the waves in wave order: the same value in every thread
template <int OP>
__device__ __forceinline__ double combine(double a, double b) {
  return OP == 0 ? a + b : OP == 1 ? fmin(a, b) : fmax(a, b);
}
template <int OP>
__device__ __forceinline__ double block_reduce(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = combine<OP>(v, __shfl_xor(v, o, 64));
  __syncthreads();                                      // `red` may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = red[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = combine<OP>(r, red[w]);
  return r;
}

// grid Na * W / 256, block 256; W = Nb, or Nb - 1 with the diagonal skipped
__global__ __launch_bounds__(256) void distance_kernel(const double* __restrict__ a, const double* __restrict__ b, int Nb, int d, int skip,
                                                       double* __restrict__ out, size_t total) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int W = skip ? Nb - 1 : Nb;
  const int i = (int)(t / W), c = (int)(t % W);
  const int j = c + (skip && c >= i ? 1 : 0);
  const double *pa = a + (size_t)i * d, *pb = b + (size_t)j * d;
  double s = 0.0;
  for (int k = 0; k < d; ++k) {
    const double x = pa[k] - pb[k];
    s += x * x;
  }
  const double r = sqrt(s);
  out[t] = isfinite(r) ? r : 0.0;                       // music_evaluator.delete_nan
}

// grid 1 or 2 (one workgroup per vector), block 1024
__global__ __launch_bounds__(STAT_THREADS) void stats_kernel(const double* __restrict__ d0, int n0, const double* __restrict__ d1, int n1,
                                                             Stats* __restrict__ st) {
  __shared__ double red[STAT_THREADS / 64];
  const double* y = blockIdx.x ? d1 : d0;
  const int n = blockIdx.x ? n1 : n0, tid = threadIdx.x;
  double lo = __longlong_as_double(0x7ff0000000000000ll), hi = -lo, s = 0.0, c = 0.0;
  for (int i = tid; i < n; i += STAT_THREADS) {
    const double v = y[i];
    lo = fmin(lo, v);
    hi = fmax(hi, v);
    kahan(s, c, v);
  }
  lo = block_reduce<1>(lo, red);
  hi = block_reduce<2>(hi, red);
  const double mean = block_reduce<0>(s, red) / (double)n;
  s = c = 0.0;
  for (int i = tid; i < n; i += STAT_THREADS) {
    const double v = y[i] - mean;
    kahan(s, c, v * v);
  }
  const double ss = block_reduce<0>(s, red);
  if (tid == 0) {
    Stats o;
    o.lo = lo;
    o.hi = hi;
    o.mean = mean;
    o.var = n >= 2 ? ss / (double)(n - 1) : quiet_nan();
    o.h = sqrt(o.var) * pow((double)n, -0.2);           // Scott's factor n^(-1 / (d + 4)), d = 1
    o.den = (double)n * o.h * SQRT_2PI;
    o.degenerate = (n >= 2 && o.var > 0.0 && isfinite(o.var) && o.h > 0.0) ? 0.0 : 1.0;
    o.pad = 0.0;
    st[blockIdx.x] = o;
  }
}

// evaluation point p of density d: the caller's x[p], or (kl_oa) p < kl: linspace(lo_d, hi_d, kl)[p], else point p - kl of the
// panels + 1 Simpson points over [min lo, max hi].  lo + i step with the last point equal to hi, as numpy.linspace forms it.
__device__ __forceinline__ double point_of(const Stats* __restrict__ st, int d, const double* __restrict__ x, int kl, int panels, int p) {
  if (x) return x[p];
  if (p < kl) {
    const double lo = st[d].lo, hi = st[d].hi, step = (hi - lo) / (double)(kl - 1);
    return p == kl - 1 ? hi : (double)p * step + lo;
  }
  const int q = p - kl;
  const double lo = fmin(st[0].lo, st[1].lo), hi = fmax(st[0].hi, st[1].hi), step = (hi - lo) / (double)panels;
  return q == panels ? hi : (double)q * step + lo;
}

// grid (ceil(M / TILE), max chunks, densities), block THREADS, TILE = THREADS * PTS points.  part[(d * maxc + chunk) * M + p] = sum over
// the chunk's y, in y order, of exp(-((x_p - y) / h)^2 / 2): a point's sum does not depend on the tile it is in nor on
// the LDS slice SUB, so the two shapes below give the same bits.  Nothing is written for a degenerate input: fold and finish answer NaN without reading `part`.
template <int THREADS, int PTS, int SUB>
__global__ __launch_bounds__(THREADS) void density_kernel(const double* __restrict__ d0, int n0, const double* __restrict__ d1, int n1,
                                                               const double* __restrict__ x, int kl, int panels, int M, int maxc,
                                                               const Stats* __restrict__ st, double* __restrict__ part) {
  constexpr int TILE = THREADS * PTS;
  __shared__ double ys[SUB];
  const int d = blockIdx.z, chunk = blockIdx.y, tid = threadIdx.x;
  const double* y = d ? d1 : d0;
  const int n = d ? n1 : n0;
  if (chunk >= n_chunks(n)) return;                     // uniform per workgroup
  if (st[0].degenerate != 0.0 || (gridDim.z == 2 && st[1].degenerate != 0.0)) return;
  const double h = st[d].h;
  double xs[PTS], acc[PTS], comp[PTS];
#pragma unroll
  for (int i = 0; i < PTS; ++i) {
    const int p = blockIdx.x * TILE + i * THREADS + tid;
    xs[i] = p < M ? point_of(st, d, x, kl, panels, p) : 0.0;
    acc[i] = comp[i] = 0.0;
  }
  const int end = min(n, (chunk + 1) * CHUNK);
  for (int base = chunk * CHUNK; base < end; base += SUB) {
    const int cnt = min(SUB, end - base);
    __syncthreads();
    for (int k = tid; k < cnt; k += THREADS) ys[k] = y[base + k];
    __syncthreads();
    for (int k = 0; k < cnt; ++k) {
      const double yk = ys[k];                          // one address per wave: a broadcast read
#pragma unroll
      for (int i = 0; i < PTS; ++i) {
        const double t = (xs[i] - yk) / h;
        kahan(acc[i], comp[i], exp(-0.5 * t * t));
      }
    }
  }
#pragma unroll
  for (int i = 0; i < PTS; ++i) {
    const int p = blockIdx.x * TILE + i * THREADS + tid;
    if (p < M) part[((size_t)d * maxc + chunk) * M + p] = acc[i];
  }
}

// grid (ceil(M / 256), densities), block 256: pdf[d * M + p] = (chunks in chunk order) / (n h sqrt(2 pi)), NaN for a degenerate input
__global__ __launch_bounds__(256) void fold_kernel(int n0, int n1, int M, int maxc, const Stats* __restrict__ st, const double* __restrict__ part,
                                                   double* __restrict__ pdf) {
  const int d = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  if (p >= M) return;
  if (st[0].degenerate != 0.0 || (gridDim.y == 2 && st[1].degenerate != 0.0)) {
    pdf[(size_t)d * M + p] = quiet_nan();
    return;
  }
  const int chunks = n_chunks(d ? n1 : n0);
  double s = 0.0, c = 0.0;
  for (int k = 0; k < chunks; ++k) kahan(s, c, part[((size_t)d * maxc + k) * M + p]);
  pdf[(size_t)d * M + p] = s / st[d].den;
}

// scipy.special.rel_entr
__device__ __forceinline__ double rel_entr(double x, double y) {
  if (isnan(x) || isnan(y)) return quiet_nan();
  if (x > 0.0 && y > 0.0) return x * log(x / y);
  if (x == 0.0 && y >= 0.0) return 0.0;
  return __longlong_as_double(0x7ff0000000000000ll);
}

// grid 1, block 1024.  out: KL, OA, |OA(panels) - OA(panels / 2)|, h_A, h_B, lo, hi, flag
__global__ __launch_bounds__(STAT_THREADS) void finish_kernel(const Stats* __restrict__ st, const double* __restrict__ pdf, int kl, int panels, int M,
                                                              double* __restrict__ out) {
  __shared__ double red[STAT_THREADS / 64];
  const int tid = threadIdx.x;
  const double lo = fmin(st[0].lo, st[1].lo), hi = fmax(st[0].hi, st[1].hi);
  const bool bad = st[0].degenerate != 0.0 || st[1].degenerate != 0.0;
  if (tid == 0) {
    out[3] = st[0].h;
    out[4] = st[1].h;
    out[5] = lo;
    out[6] = hi;
    out[7] = bad ? 1.0 : 0.0;
    if (bad) out[0] = out[1] = out[2] = quiet_nan();
  }
  if (bad) return;
  const double *pa = pdf, *pb = pdf + M;
  double sa = 0.0, sb = 0.0;
  for (int i = tid; i < kl; i += STAT_THREADS) {
    sa += pa[i];
    sb += pb[i];
  }
  sa = block_reduce<0>(sa, red);
  sb = block_reduce<0>(sb, red);
  double e = 0.0;
  for (int i = tid; i < kl; i += STAT_THREADS) e += rel_entr(pa[i] / sa, pb[i] / sb);
  e = block_reduce<0>(e, red);
  // Simpson: the interior points by i mod 4, so that the rule at half the panels comes from the same samples
  double odd = 0.0, two = 0.0, four = 0.0;
  for (int i = tid; i <= panels; i += STAT_THREADS) {
    const double m = fmin(pa[kl + i], pb[kl + i]);
    if (i & 1) odd += m;
    else if (i == 0 || i == panels) continue;
    else if (i & 2) two += m;
    else four += m;
  }
  odd = block_reduce<0>(odd, red);
  two = block_reduce<0>(two, red);
  four = block_reduce<0>(four, red);
  if (tid == 0) {
    const double ends = fmin(pa[kl], pb[kl]) + fmin(pa[kl + panels], pb[kl + panels]);
    const double step = (hi - lo) / (double)panels;
    const double oa = step / 3.0 * (ends + 4.0 * odd + 2.0 * (two + four));
    out[0] = e;
    out[1] = oa;
    out[2] = panels % 4 == 0 ? fabs(oa - 2.0 * step / 3.0 * (ends + 4.0 * two + 2.0 * four)) : quiet_nan();
  }
}

inline size_t align64(size_t b) { return (b + 63) & ~(size_t)63; }

// 512 points per workgroup of four waves, two per lane; where that leaves fewer than SMALL_GRID workgroups (a few hundred samples per
// set: less than a wave per SIMD), one wave per workgroup, one point per lane and a 4 KiB slice (16 KiB per one-wave workgroup would
// cap a SIMD at three waves) instead -- eight times the workgroups, the same sums
inline void launch_density(hipStream_t s, const double* d0, int n0, const double* d1, int n1, int dens, const double* x, int kl, int panels, int M,
                           int maxc, const Stats* st, double* part) {
  const long long big = (long long)((M + 511) / 512) * (n_chunks(n0) + (dens == 2 ? n_chunks(n1) : 0));
  if (big >= SMALL_GRID)
    hipLaunchKernelGGL((density_kernel<256, 2, 2048>), dim3((M + 511) / 512, maxc, dens), dim3(256), 0, s, d0, n0, d1, n1, x, kl, panels, M, maxc, st, part);
  else
    hipLaunchKernelGGL((density_kernel<64, 1, 512>), dim3((M + 63) / 64, maxc, dens), dim3(64), 0, s, d0, n0, d1, n1, x, kl, panels, M, maxc, st, part);
}
}  // namespace sets
}  // namespace rgm

using namespace rgm;

extern "C" int rgm_set_distances(const double* a, int Na, const double* b, int Nb, int d, int skip_diagonal, double* out, void* stream) {
  RGM_REQUIRE(a && b && out, "set_distances: bad arguments");
  RGM_REQUIRE(Na >= 1 && Na <= sets::MAX_ROWS && Nb >= 1 && Nb <= sets::MAX_ROWS, "set_distances: %d x %d rows (1 .. %d each)", Na, Nb, sets::MAX_ROWS);
  RGM_REQUIRE(d >= 1 && d <= sets::MAX_D, "set_distances: d = %d (1 .. %d)", d, sets::MAX_D);
  RGM_REQUIRE(!skip_diagonal || (Na == Nb && Nb >= 2), "set_distances: skipping the diagonal needs Na == Nb >= 2, got %d and %d", Na, Nb);
  const size_t total = (size_t)Na * (size_t)(skip_diagonal ? Nb - 1 : Nb);
  hipLaunchKernelGGL(sets::distance_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, Nb, d,
                     skip_diagonal ? 1 : 0, out, total);
  RGM_LAUNCH_CHECK();
  return RGM_OK;
}

extern "C" size_t rgm_kde_pdf_workspace(int n, int m) {
  if (n < 1 || n > sets::MAX_N || m < 1 || m > sets::MAX_M) return 0;
  return sets::align64(sizeof(sets::Stats)) + (size_t)sets::n_chunks(n) * m * sizeof(double);
}

extern "C" int rgm_kde_pdf(const double* data, int n, const double* x, int m, double* pdf, void* ws, size_t ws_bytes, void* stream) {
  RGM_REQUIRE(data && x && pdf, "kde_pdf: bad arguments");
  RGM_REQUIRE(n >= 1 && n <= sets::MAX_N, "kde_pdf: n = %d (1 .. %d)", n, sets::MAX_N);
  RGM_REQUIRE(m >= 1 && m <= sets::MAX_M, "kde_pdf: m = %d points (1 .. %d)", m, sets::MAX_M);
  RGM_REQUIRE(ws && ws_bytes >= rgm_kde_pdf_workspace(n, m), "kde_pdf: workspace of %zu bytes, %zu needed", ws_bytes, rgm_kde_pdf_workspace(n, m));
  RGM_REQUIRE(((uintptr_t)ws & 7) == 0, "kde_pdf: the workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  sets::Stats* st = (sets::Stats*)ws;
  double* part = (double*)((char*)ws + sets::align64(sizeof(sets::Stats)));
  const int maxc = sets::n_chunks(n);
  hipLaunchKernelGGL(sets::stats_kernel, dim3(1), dim3(sets::STAT_THREADS), 0, s, data, n, data, n, st);
  RGM_LAUNCH_CHECK();
  sets::launch_density(s, data, n, data, n, 1, x, 0, 0, m, maxc, st, part);
  RGM_LAUNCH_CHECK();
  hipLaunchKernelGGL(sets::fold_kernel, dim3((m + 255) / 256, 1), dim3(256), 0, s, n, n, m, maxc, st, part, pdf);
  RGM_LAUNCH_CHECK();
  return RGM_OK;
}

extern "C" size_t rgm_set_kl_oa_workspace(int nA, int nB, int kl_points, int oa_panels) {
  if (nA < 2 || nA > sets::MAX_N || nB < 2 || nB > sets::MAX_N || kl_points < 2 || kl_points > sets::MAX_KL || oa_panels < 2 ||
      oa_panels > sets::MAX_PANELS || (oa_panels & 1))
    return 0;
  const size_t M = (size_t)kl_points + oa_panels + 1, maxc = sets::n_chunks(std::max(nA, nB));
  return sets::align64(2 * sizeof(sets::Stats)) + 2 * M * sizeof(double) + 2 * maxc * M * sizeof(double);
}

extern "C" int rgm_set_kl_oa(const double* A, int nA, const double* B, int nB, int kl_points, int oa_panels, double* out, void* ws, size_t ws_bytes,
                             void* stream) {
  RGM_REQUIRE(A && B && out, "set_kl_oa: bad arguments");
  RGM_REQUIRE(nA >= 2 && nA <= sets::MAX_N && nB >= 2 && nB <= sets::MAX_N, "set_kl_oa: %d and %d distances (2 .. %d each)", nA, nB, sets::MAX_N);
  RGM_REQUIRE(kl_points >= 2 && kl_points <= sets::MAX_KL, "set_kl_oa: %d KL points (2 .. %d)", kl_points, sets::MAX_KL);
  RGM_REQUIRE(oa_panels >= 2 && oa_panels <= sets::MAX_PANELS && !(oa_panels & 1), "set_kl_oa: %d Simpson panels (even, 2 .. %d)", oa_panels,
              sets::MAX_PANELS);
  RGM_REQUIRE(ws && ws_bytes >= rgm_set_kl_oa_workspace(nA, nB, kl_points, oa_panels), "set_kl_oa: workspace of %zu bytes, %zu needed", ws_bytes,
              rgm_set_kl_oa_workspace(nA, nB, kl_points, oa_panels));
  RGM_REQUIRE(((uintptr_t)ws & 7) == 0, "set_kl_oa: the workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int M = kl_points + oa_panels + 1, maxc = sets::n_chunks(std::max(nA, nB));
  sets::Stats* st = (sets::Stats*)ws;
  double* pdf = (double*)((char*)ws + sets::align64(2 * sizeof(sets::Stats)));
  double* part = pdf + 2 * (size_t)M;
  hipLaunchKernelGGL(sets::stats_kernel, dim3(2), dim3(sets::STAT_THREADS), 0, s, A, nA, B, nB, st);
  RGM_LAUNCH_CHECK();
  sets::launch_density(s, A, nA, B, nB, 2, nullptr, kl_points, oa_panels, M, maxc, st, part);
  RGM_LAUNCH_CHECK();
  hipLaunchKernelGGL(sets::fold_kernel, dim3((M + 255) / 256, 2), dim3(256), 0, s, nA, nB, M, maxc, st, part, pdf);
  RGM_LAUNCH_CHECK();
  hipLaunchKernelGGL(sets::finish_kernel, dim3(1), dim3(sets::STAT_THREADS), 0, s, st, pdf, kl_points, oa_panels, M, out);
  RGM_LAUNCH_CHECK();
  return RGM_OK;
}
