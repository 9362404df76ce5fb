// particles.hip -- the device primitives of particle rule guidance (sequential Monte Carlo beside SCG): weighting and systematic
// resampling of B groups of n particles with the decision taken on the device, and the ancestor gather of latent rows.
// Definition, quirks and measurements: docs/rounds/particles.md, include/rgm.h.
//
//   rgm_particle_resample   one launch, one workgroup of 256 per group: the group's n log-weights sit in LDS, thread 0 owns the three
//                           sums (normaliser, sum of squares, cumulative weights) in ascending k, every thread then finds the ancestors
//                           of its particles by bisection of the cumulative weights.
//   rgm_gather_rows         one launch, grid (rows, chunks of a row): 16-byte copies where the rows allow it.
// Float64 without FMA contraction, no atomics, nothing allocated, everything on the caller's stream: a group's result depends on its
// own inputs alone -- not on B, not on its position -- and repeats bit for bit.
#include "common.h"
#include "philox.h"

#pragma clang fp contract(off)

namespace rgm {
namespace particles {
constexpr int THREADS = 256, MAX_N = 1024, PER = MAX_N / THREADS, COPY_THREADS = 256;

__device__ __forceinline__ double neg_inf() { return __longlong_as_double(0xfff0000000000000ll); }

// grid B, block 256.  Particle k of group b is element k * B + b.
__global__ __launch_bounds__(THREADS) void resample_kernel(const float* __restrict__ reward, double* __restrict__ logw, float* __restrict__ r_prev,
                                                           double lambda, double ess_frac, const double* __restrict__ u_in, uint64_t seed,
                                                           uint64_t counter, int32_t* __restrict__ anc, double* __restrict__ ess_out,
                                                           int32_t* __restrict__ resampled, int n, int B) {
  __shared__ double a[MAX_N];          // l_k, then exp(l_k - max), then the cumulative weights c_k
  __shared__ float rp[MAX_N];          // r_prev after this step's update, before the ancestor gather
  __shared__ double red[THREADS / 64];
  __shared__ double sh_sum, sh_ess;
  __shared__ int sh_last;
  const int b = blockIdx.x, tid = threadIdx.x;
  double ell[PER];
  double m = neg_inf();
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int k = tid + i * THREADS;
    ell[i] = neg_inf();
    if (k < n) {
      const size_t at = (size_t)k * B + b;
      const float rf = reward[at], pf = r_prev[at];
      const double lw = logw[at];
      const bool dead = !(rf < __builtin_inff());                    // NaN or +inf
      const double r = dead ? neg_inf() : (double)rf;
      double l = (r == neg_inf() || lw == neg_inf()) ? neg_inf() : lw + lambda * (r - (double)pf);
      if (!(l < (double)__builtin_inff())) l = neg_inf();            // a log-weight that is NaN or +inf is a broken particle too
      ell[i] = l;
      a[k] = l;
      rp[k] = r == neg_inf() ? pf : rf;                              // a dead particle keeps its last finite reward
      m = fmax(m, l);
    }
  }
  // the maximum: a fixed shuffle tree per wave, then the waves in wave order -- the same value in every thread
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  m = red[0];
  for (int w = 1; w < THREADS / 64; ++w) m = fmax(m, red[w]);
  if (m == neg_inf()) {                                              // every weight is 0 (uniform over the workgroup)
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int k = tid + i * THREADS;
      if (k < n) {
        const size_t at = (size_t)k * B + b;
        logw[at] = 0.0;
        r_prev[at] = rp[k];
        anc[at] = k;
      }
    }
    if (tid == 0) {
      ess_out[b] = 0.0;
      resampled[b] = -1;
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int k = tid + i * THREADS;
    if (k < n) a[k] = exp(ell[i] - m);
  }
  __syncthreads();
  if (tid == 0) {                                                    // the one owner of the sums, in ascending k
    double s = 0.0;
    for (int j = 0; j < n; ++j) s += a[j];
    double c = 0.0, ss = 0.0;
    int last = 0;
    for (int j = 0; j < n; ++j) {
      const double w = a[j] / s;
      if (w > 0.0) last = j;
      ss += w * w;
      c += w;
      a[j] = c;
    }
    sh_sum = s;
    sh_ess = 1.0 / ss;
    sh_last = last;
  }
  __syncthreads();
  const double ess = sh_ess;
  const bool go = ess_frac > 1.0 || (ess_frac > 0.0 && ess < ess_frac * (double)n);
  if (tid == 0) {
    ess_out[b] = ess;
    resampled[b] = go ? 1 : 0;
  }
  if (go) {
    double u;
    if (u_in) {
      u = u_in[b];
    } else {
      uint32_t r[4];
      philox4x32_10(counter + (uint64_t)b, seed, r);
      u = ((double)r[0] + 0.5) * (1.0 / 4294967296.0);
    }
    const int last = sh_last;                                        // c_j from the last particle of non-zero weight on counts as +inf
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int k = tid + i * THREADS;
      if (k < n) {
        const double thr = ((double)k + u) / (double)n;
        int lo = 0, hi = last;                                       // min{j : c_j > thr}: c is non-decreasing
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (a[mid] > thr) hi = mid;
          else lo = mid + 1;
        }
        const size_t at = (size_t)k * B + b;
        anc[at] = lo;
        logw[at] = 0.0;
        r_prev[at] = rp[lo];
      }
    }
  } else {
    const double ls = log(sh_sum), ln = log((double)n);
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int k = tid + i * THREADS;
      if (k < n) {
        const size_t at = (size_t)k * B + b;
        anc[at] = k;
        logw[at] = ell[i] - m - ls + ln;
        r_prev[at] = rp[k];
      }
    }
  }
}

// grid (n * B rows, chunks of a row), block 256; VEC 4: float4 per thread, 1: one float
template <int VEC>
__global__ __launch_bounds__(COPY_THREADS) void gather_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                              const int32_t* __restrict__ anc, int n, int B, int E) {
  const int row = blockIdx.x, b = row % B;
  const int at = (blockIdx.y * COPY_THREADS + threadIdx.x) * VEC;
  if (at >= E) return;
  const int k = min(max(anc[row], 0), n - 1);
  const float* s = src + ((size_t)k * B + b) * E + at;
  float* d = dst + (size_t)row * E + at;
  if constexpr (VEC == 4) *reinterpret_cast<float4*>(d) = *reinterpret_cast<const float4*>(s);
  else *d = *s;
}
}  // namespace particles
}  // namespace rgm

using namespace rgm;

extern "C" int rgm_particle_resample(const float* reward, double* logw, float* r_prev, double lambda, double ess_frac, const double* u,
                                     uint64_t seed, uint64_t counter, int32_t* anc, double* ess_out, int32_t* resampled, int n, int B,
                                     void* stream) {
  RGM_REQUIRE(reward && logw && r_prev && anc && ess_out && resampled, "particle_resample: bad arguments");
  RGM_REQUIRE(n >= 1 && n <= particles::MAX_N, "particle_resample: n = %d particles per group (1 .. %d)", n, particles::MAX_N);
  RGM_REQUIRE(B >= 1 && (long long)n * B <= 0x7fffffffll, "particle_resample: B = %d groups of %d particles", B, n);
  RGM_REQUIRE(lambda == lambda && lambda - lambda == 0.0, "particle_resample: lambda = %g is not finite", lambda);
  RGM_REQUIRE(ess_frac == ess_frac, "particle_resample: the ESS fraction is NaN");
  RGM_REQUIRE(((uintptr_t)logw & 7) == 0 && ((uintptr_t)ess_out & 7) == 0 && ((uintptr_t)u & 7) == 0,
              "particle_resample: the float64 arrays must be 8-byte aligned");
  hipLaunchKernelGGL(particles::resample_kernel, dim3(B), dim3(particles::THREADS), 0, (hipStream_t)stream, reward, logw, r_prev, lambda,
                     ess_frac, u, seed, counter, anc, ess_out, resampled, n, B);
  RGM_LAUNCH_CHECK();
  return RGM_OK;
}

extern "C" int rgm_gather_rows(const float* src, float* dst, const int32_t* anc, int n, int B, int E, void* stream) {
  RGM_REQUIRE(src && dst && anc, "gather_rows: bad arguments");
  RGM_REQUIRE(n >= 1 && B >= 1 && E >= 1 && (long long)n * B <= 0x7fffffffll, "gather_rows: %d x %d rows of %d", n, B, E);
  const size_t bytes = (size_t)n * B * E * sizeof(float);
  const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst;
  RGM_REQUIRE(s0 + bytes <= d0 || d0 + bytes <= s0, "gather_rows: source and destination overlap (the gather is out of place)");
  const bool vec = E % 4 == 0 && (s0 & 15) == 0 && (d0 & 15) == 0;
  const int per = particles::COPY_THREADS * (vec ? 4 : 1), chunks = (E + per - 1) / per;
  RGM_REQUIRE(chunks <= 65535, "gather_rows: rows of %d floats (at most %d)", E, 65535 * per);
  const dim3 grid((unsigned)((long long)n * B), (unsigned)chunks);
  if (vec)
    hipLaunchKernelGGL(particles::gather_kernel<4>, grid, dim3(particles::COPY_THREADS), 0, (hipStream_t)stream, src, dst, anc, n, B, E);
  else
    hipLaunchKernelGGL(particles::gather_kernel<1>, grid, dim3(particles::COPY_THREADS), 0, (hipStream_t)stream, src, dst, anc, n, B, E);
  RGM_LAUNCH_CHECK();
  return RGM_OK;
}
