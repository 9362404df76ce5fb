// eval.hip -- what the scheduler needs to take an EXISTING latent as its input: the DDIM ODE run towards noise and the terms of
// the variational bound in bits per dimension.
//
// Reference: guided_diffusion/gaussian_diffusion.py
//   :978-1014 ddim_reverse_sample, :1145-1178 _vb_terms_bpd, :1255-1272 _prior_bpd, :1297-1318 the per-step errors of calc_bpd_loop;
//   guided_diffusion/losses.py :12-39 normal_kl, :42-77 discretized_gaussian_log_likelihood.
//
// Arithmetic.  These kernels read 12-24 bytes per element and are bound by memory, so every element is evaluated in fp64 from the
// fp32 inputs and the fp32-cast schedule tables (what _extract_into_tensor hands the reference): the re-derived eps
// (c1 x - x0) / c2 and the decoder term's difference of two nearly equal CDF values lose no digits to cancellation.
//
// Reduction (rgm_vb_terms, rgm_prior_bpd).  A sample's E elements are cut into chunks of VB_CHUNK = 2048 -- a function of E alone.
// Workgroup (chunk, sample) of the first launch sums its chunk: every thread its 8 elements in index order, a wave64 xor-shuffle
// tree, the 4 waves' sums in wave order through LDS; the fp64 partial sums go to partials[sample][chunk][3].  A second launch of one
// wave per sample adds the chunks (lane l takes chunks l, l + 64, ... in order, then the same shuffle tree) and writes the means.
// No atomics, every partial and every output owned by exactly one thread: the same inputs give the same bits on every launch, and
// a sample's numbers depend neither on N nor on its row in the batch.
#include "common.h"

namespace rgm {

constexpr int VB_THREADS = 256;
constexpr int VB_CHUNK = 2048;            // elements per workgroup: 2 x 16 bytes per thread and array
constexpr double LN2 = 0.6931471805599453;

struct EvalTables {
  const float* sqrt_recip_ac;
  const float* sqrt_recipm1_ac;
  const float* post_c1;
  const float* post_c2;
  const float* logvar;        // the FIXED_LARGE / FIXED_SMALL model log-variance
  const float* ac;
};

// x0 = c1 x - c2 eps (clip) ; eps' = (c1 x - x0) / c2 ; sample = sqrt(abar_next) x0 + sqrt(1 - abar_next) eps'
__global__ void ddim_reverse_step_kernel(const float* __restrict__ x, const float* __restrict__ eps_in, const int64_t* __restrict__ t,
                                         EvalTables tb, int clip, int T, float* __restrict__ sample, float* __restrict__ pred_xstart,
                                         long long total, int E) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int ti = (int)t[i / E];
  const double c1 = tb.sqrt_recip_ac[ti], c2 = tb.sqrt_recipm1_ac[ti];
  const double abn = ti + 1 < T ? (double)tb.ac[ti + 1] : 0.0;
  const double xv = x[i];
  double x0 = c1 * xv - c2 * (double)eps_in[i];
  if (clip) x0 = fmin(fmax(x0, -1.0), 1.0);
  const double e2 = (c1 * xv - x0) / c2;
  sample[i] = (float)(x0 * sqrt(abn) + sqrt(1.0 - abn) * e2);
  pred_xstart[i] = (float)x0;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the workgroup's sums of K values per thread -> dst[0..K) (thread 0 writes)
template <int K>
__device__ __forceinline__ void block_sum_store(double (&acc)[K], double* __restrict__ dst) {
  __shared__ double red[VB_THREADS / 64][K];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double s = wave_sum_f64(acc[k]);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      double s = red[0][k];
      for (int w = 1; w < VB_THREADS / 64; ++w) s += red[w][k];
      dst[k] = s;
    }
  }
}

// 4 consecutive elements of a sample's row starting at e (vec: E % 4 == 0 and the base 16-byte aligned)
__device__ __forceinline__ void load4(const float* __restrict__ row, int e, int E, bool vec, float (&v)[4]) {
  if (vec) {
    const float4 q = ldg16(row + e);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = e + j < E ? row[e + j] : 0.f;
  }
}

__device__ __forceinline__ double approx_cdf(double u) {
  return 0.5 * (1.0 + tanh(0.7978845608028654 * (u + 0.044715 * u * u * u)));
}

// grid (chunks, N).  partials[(b * chunks + chunk) * 3 + {0: vb term in nats, 1: (x0 - x_start)^2, 2: (eps' - noise)^2}]
__global__ void __launch_bounds__(VB_THREADS)
vb_terms_partial_kernel(const float* __restrict__ x_start, const float* __restrict__ x_t, const float* __restrict__ eps_in,
                        const float* __restrict__ noise, const int64_t* __restrict__ t, EvalTables tb,
                        const float* __restrict__ post_logvar, const float* __restrict__ vv, const float* __restrict__ min_log,
                        const float* __restrict__ max_log, const float* __restrict__ model_mean, const float* __restrict__ model_xstart,
                        int clip, double* __restrict__ partials, float* __restrict__ pred_xstart, int E, int vec) {
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int ti = (int)t[b];
  const long long row = (long long)b * E;
  const double c1 = tb.sqrt_recip_ac[ti], c2 = tb.sqrt_recipm1_ac[ti];
  const double pc1 = tb.post_c1[ti], pc2 = tb.post_c2[ti];
  const double lv1 = post_logvar[ti];
  const double lo = min_log ? (double)min_log[ti] : 0.0, hi = max_log ? (double)max_log[ti] : 0.0;
  const bool decoder = ti == 0;
  // per-sample constants: exp(lv1) always; with fixed variances exp(-lv2) (KL) or exp(-0.5 lv2) (decoder) as well
  const double e_lv1 = exp(lv1);
  double lv2 = tb.logvar[ti];
  double e_inv = vv ? 0.0 : exp(decoder ? -0.5 * lv2 : -lv2);
  double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int s = 0; s < VB_CHUNK / (4 * VB_THREADS); ++s) {
    const int e = chunk * VB_CHUNK + (s * VB_THREADS + (int)threadIdx.x) * 4;
    if (e >= E) break;
    float xs[4], xt[4], ep[4] = {0.f, 0.f, 0.f, 0.f}, nz[4], v4[4], mm[4], mx[4];
    load4(x_start + row, e, E, vec, xs);
    load4(x_t + row, e, E, vec, xt);
    if (model_xstart) load4(model_xstart + row, e, E, vec, mx);
    else load4(eps_in + row, e, E, vec, ep);
    if (noise) load4(noise + row, e, E, vec, nz);
    if (vv) load4(vv + row, e, E, vec, v4);
    if (model_mean) load4(model_mean + row, e, E, vec, mm);
    float x0f[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool live = e + j < E;
      const double xsv = xs[j], xtv = xt[j];
      double x0 = model_xstart ? (double)mx[j] : c1 * xtv - c2 * (double)ep[j];
      if (clip) x0 = fmin(fmax(x0, -1.0), 1.0);
      x0f[j] = (float)x0;
      if (vv) {
        if (min_log) {
          const double frac = ((double)v4[j] + 1.0) / 2.0;
          lv2 = frac * hi + (1.0 - frac) * lo;
        } else {
          lv2 = v4[j];
        }
        e_inv = exp(decoder ? -0.5 * lv2 : -lv2);
      }
      double term;
      if (!decoder) {
        // normal_kl(q_posterior_mean, lv1, model_mean, lv2): both means share pc2 x_t unless the network predicts the mean itself
        const double dm = model_mean ? pc1 * xsv + pc2 * xtv - (double)mm[j] : pc1 * (xsv - x0);
        term = 0.5 * (-1.0 + lv2 - lv1 + (e_lv1 + dm * dm) * e_inv);
      } else {
        const double mean = model_mean ? (double)mm[j] : pc1 * x0 + pc2 * xtv;
        const double cx = xsv - mean;
        double p;
        if (xsv < -0.999) p = approx_cdf(e_inv * (cx + 1.0 / 255.0));
        else if (xsv > 0.999) p = 1.0 - approx_cdf(e_inv * (cx - 1.0 / 255.0));
        else p = approx_cdf(e_inv * (cx + 1.0 / 255.0)) - approx_cdf(e_inv * (cx - 1.0 / 255.0));
        term = -log(fmax(p, 1e-12));
      }
      const double dx = x0 - xsv;
      if (live) {
        acc[0] += term;
        acc[1] += dx * dx;
        if (noise) {
          const double de = (c1 * xtv - x0) / c2 - (double)nz[j];
          acc[2] += de * de;
        }
      }
    }
    if (pred_xstart) {
      if (vec) {
        *reinterpret_cast<float4*>(pred_xstart + row + e) = make_float4(x0f[0], x0f[1], x0f[2], x0f[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (e + j < E) pred_xstart[row + e + j] = x0f[j];
      }
    }
  }
  block_sum_store<3>(acc, partials + ((long long)b * gridDim.x + chunk) * 3);
}

// grid (chunks, N): partials[b * chunks + chunk] = sum over the chunk of normal_kl(sqrt_ac x, lv, 0, 0)
__global__ void __launch_bounds__(VB_THREADS)
prior_partial_kernel(const float* __restrict__ x_start, float sqrt_ac, float log_one_minus_ac, double* __restrict__ partials, int E,
                     int vec) {
  const int b = blockIdx.y, chunk = blockIdx.x;
  const long long row = (long long)b * E;
  const double a = sqrt_ac, lv = log_one_minus_ac, base = -1.0 - lv + exp(lv);
  double acc[1] = {0.0};
#pragma unroll
  for (int s = 0; s < VB_CHUNK / (4 * VB_THREADS); ++s) {
    const int e = chunk * VB_CHUNK + (s * VB_THREADS + (int)threadIdx.x) * 4;
    if (e >= E) break;
    float xs[4];
    load4(x_start + row, e, E, vec, xs);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double m = a * (double)xs[j];
      if (e + j < E) acc[0] += 0.5 * (base + m * m);
    }
  }
  block_sum_store<1>(acc, partials + (long long)b * gridDim.x + chunk);
}

// one wave per sample: out_k[b] = scale_k / E * sum over the chunks, in a fixed order (out_k NULL: skipped)
template <int K>
__global__ void __launch_bounds__(64)
chunk_sum_kernel(const double* __restrict__ partials, int chunks, int E, double scale0, float* __restrict__ out0,
                 float* __restrict__ out1, float* __restrict__ out2) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const double* p = partials + (long long)b * chunks * K;
  double acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0;
  for (int c = lane; c < chunks; c += 64)
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] += p[(long long)c * K + k];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = wave_sum_f64(acc[k]);
  if (lane == 0) {
    if (out0) out0[b] = (float)(acc[0] * scale0 / (double)E);
    if constexpr (K == 3) {
      if (out1) out1[b] = (float)(acc[1] / (double)E);
      if (out2) out2[b] = (float)(acc[2] / (double)E);
    }
  }
}

static EvalTables make_eval_tables(const float* const* tabs) {
  EvalTables t;
  t.sqrt_recip_ac = tabs[0];
  t.sqrt_recipm1_ac = tabs[1];
  t.post_c1 = tabs[2];
  t.post_c2 = tabs[3];
  t.logvar = tabs[5];
  t.ac = tabs[6];
  return t;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace rgm

using namespace rgm;

extern "C" int rgm_ddim_reverse_step(const float* x, const float* eps, const int64_t* t, const float* const* tables, int num_timesteps,
                                     int clip_denoised, float* sample, float* pred_xstart, int N, int E, void* stream) {
  RGM_REQUIRE(x && eps && t && tables && sample && pred_xstart && N > 0 && E > 0 && num_timesteps > 0, "ddim_reverse_step: bad arguments");
  const long long total = (long long)N * E;
  hipLaunchKernelGGL(ddim_reverse_step_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, eps, t,
                     make_eval_tables(tables), clip_denoised, num_timesteps, sample, pred_xstart, total, E);
  RGM_LAUNCH_CHECK();
  return RGM_OK;
}

extern "C" int64_t rgm_vb_terms_partials(int N, int E) {
  if (N <= 0 || E <= 0) return 0;
  return (int64_t)N * cdiv(E, VB_CHUNK) * 3;
}

extern "C" int rgm_vb_terms(const float* x_start, const float* x_t, const float* eps, const float* noise, const int64_t* t,
                            const float* const* tables, const float* post_logvar_tab, const float* var_values, const float* min_log_tab,
                            const float* max_log_tab, const float* model_mean, const float* model_xstart, int clip_denoised,
                            double* partials, float* vb, float* xstart_mse, float* eps_mse, float* pred_xstart, int N, int E,
                            void* stream) {
  RGM_REQUIRE(x_start && x_t && (eps || model_xstart) && t && tables && post_logvar_tab && partials && vb && N > 0 && E > 0,
              "vb_terms: bad arguments");
  RGM_REQUIRE(N <= 65535, "vb_terms: N = %d samples (at most 65535 per launch)", N);
  RGM_REQUIRE((min_log_tab == nullptr) == (max_log_tab == nullptr), "vb_terms: min / max log-variance tables come together");
  RGM_REQUIRE(var_values || !min_log_tab, "vb_terms: log-variance tables without var_values");
  RGM_REQUIRE(noise || !eps_mse, "vb_terms: eps_mse needs the noise");
  const int chunks = cdiv(E, VB_CHUNK);
  const int vec = E % 4 == 0 && aligned16(x_start) && aligned16(x_t) && aligned16(eps) && aligned16(noise) && aligned16(var_values) &&
                  aligned16(model_mean) && aligned16(model_xstart) && aligned16(pred_xstart);
  hipLaunchKernelGGL(vb_terms_partial_kernel, dim3(chunks, N), dim3(VB_THREADS), 0, (hipStream_t)stream, x_start, x_t, eps, noise, t,
                     make_eval_tables(tables), post_logvar_tab, var_values, min_log_tab, max_log_tab, model_mean, model_xstart,
                     clip_denoised, partials, pred_xstart, E, vec);
  RGM_LAUNCH_CHECK();
  hipLaunchKernelGGL(chunk_sum_kernel<3>, dim3(N), dim3(64), 0, (hipStream_t)stream, (const double*)partials, chunks, E, 1.0 / LN2, vb,
                     xstart_mse, eps_mse);
  RGM_LAUNCH_CHECK();
  return RGM_OK;
}

extern "C" int rgm_prior_bpd(const float* x_start, float sqrt_alphas_cumprod_T, float log_one_minus_alphas_cumprod_T, double* partials,
                             float* out, int N, int E, void* stream) {
  RGM_REQUIRE(x_start && partials && out && N > 0 && N <= 65535 && E > 0, "prior_bpd: bad arguments");
  const int chunks = cdiv(E, VB_CHUNK);
  const int vec = E % 4 == 0 && aligned16(x_start);
  hipLaunchKernelGGL(prior_partial_kernel, dim3(chunks, N), dim3(VB_THREADS), 0, (hipStream_t)stream, x_start, sqrt_alphas_cumprod_T,
                     log_one_minus_alphas_cumprod_T, partials, E, vec);
  RGM_LAUNCH_CHECK();
  hipLaunchKernelGGL(chunk_sum_kernel<1>, dim3(N), dim3(64), 0, (hipStream_t)stream, (const double*)partials, chunks, E, 1.0 / LN2, out,
                     (float*)nullptr, (float*)nullptr);
  RGM_LAUNCH_CHECK();
  return RGM_OK;
}
