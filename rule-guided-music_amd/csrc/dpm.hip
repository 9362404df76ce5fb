// dpm.hip -- one step of DPM-Solver++(2M), the second-order multistep solver in data-prediction form
// (Lu et al. 2022, "DPM-Solver++: Fast Solver for Guided Sampling of Diffusion Probabilistic Models", Alg. 2 and its SDE
// variant), fused into ONE launch like the steps of sampler.hip: per-row int64 t, float32 device tables indexed by the chain
// index, optional pointers.
//
// With lambda_i = 1/2 log(abar_i / (1 - abar_i)), the step from chain index i (t) to i - 1 (s) has h = lambda_{i-1} - lambda_i and
//   x0 = c1 x - c2 eps (clip) ; classifier gradient as ddim_step_kernel's condition_score
//   D  = x0 + 1/2 (x0 - x0_prev) / r0,  r0 = (lambda_i - lambda_{i+1}) / h          (x0_prev: pred_xstart of the step before)
//   ODE  x_s = (sigma_s / sigma_t) x - alpha_s (e^-h - 1) D
//   SDE  x_s = (sigma_s / sigma_t) e^-h x + alpha_s (1 - e^-2h) D + sigma_s sqrt(1 - e^-2h) z
// The four coefficients (of x, of D, the extrapolation weight 1 / (2 r0), of z) come from tables the host built in float64 for
// one of the two modes -- the kernel never calls exp, and the final step (h = inf: x_s = D) is an entry of those tables too.
#include "common.h"

namespace rgm {

struct DpmTables {
  const float* c1;    // sqrt_recip_alphas_cumprod
  const float* c2;    // sqrt_recipm1_alphas_cumprod
  const float* ac;    // alphas_cumprod
  const float* cx;    // coefficient of x
  const float* cd;    // coefficient of D
  const float* w1;    // 1 / (2 r0); 0 where the step is first order by construction
  const float* cn;    // coefficient of the noise (0 in ODE mode)
};

// One thread per element; E = elements per sample.  noise == nullptr -> sample = the mean (SCG draws its own candidates).
__global__ void dpmpp_step_kernel(const float* __restrict__ x, const float* __restrict__ eps_in, const float* __restrict__ grad,
                                  const float* __restrict__ x0_prev, const float* __restrict__ noise, const int64_t* __restrict__ t,
                                  DpmTables tb, int top, int order, int clip, int t_end, float* __restrict__ sample,
                                  float* __restrict__ pred_xstart, float* __restrict__ g_out, long long total, int E) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int b = (int)(i / E);
  const int ti = (int)t[b];
  const float xv = x[i];
  const float c1 = tb.c1[ti], c2 = tb.c2[ti];
  float x0 = c1 * xv - c2 * eps_in[i];
  if (clip) x0 = fminf(fmaxf(x0, -1.f), 1.f);
  if (grad) {
    float e = (c1 * xv - x0) / c2;
    e = e - sqrtf(1.f - tb.ac[ti]) * grad[i];
    x0 = c1 * xv - c2 * e;
  }
  // first order at the chain's top index (no earlier estimate), at the last index (the target has abar = 1) and on request
  float D = x0;
  if (x0_prev && order == 2 && ti > 0 && ti < top) D = x0 + tb.w1[ti] * (x0 - x0_prev[i]);
  const float cn = tb.cn[ti];
  float s = D;                                    // the last index returns D itself
  if (ti > 0) {
    s = tb.cx[ti] * xv + tb.cd[ti] * D;
    if (noise) s = s + (ti != t_end ? 1.f : 0.f) * cn * noise[i];
  }
  sample[i] = s;
  pred_xstart[i] = x0;
  if (g_out && (i % E) == 0) g_out[b] = cn;
}

}  // namespace rgm

using namespace rgm;

extern "C" int rgm_dpmpp_step(const float* x, const float* eps, const float* grad, const float* x0_prev, const float* noise,
                              const int64_t* t, const float* const* tables, const float* const* dpm_tables, int num_timesteps,
                              int order, int clip_denoised, int t_end, float* sample, float* pred_xstart, float* g_out, int N, int E,
                              void* stream) {
  RGM_REQUIRE(x && eps && t && tables && dpm_tables && sample && pred_xstart && N > 0 && E > 0 && num_timesteps > 0,
              "dpmpp_step: bad arguments");
  RGM_REQUIRE(order == 1 || order == 2, "dpmpp_step: order %d (1 or 2)", order);
  for (int k = 0; k < 4; ++k) RGM_REQUIRE(dpm_tables[k] != nullptr, "dpmpp_step: coefficient table %d is NULL", k);
  DpmTables tb;
  tb.c1 = tables[0];
  tb.c2 = tables[1];
  tb.ac = tables[6];
  tb.cx = dpm_tables[0];
  tb.cd = dpm_tables[1];
  tb.w1 = dpm_tables[2];
  tb.cn = dpm_tables[3];
  const long long total = (long long)N * E;
  hipLaunchKernelGGL(dpmpp_step_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, eps, grad,
                     x0_prev, noise, t, tb, num_timesteps - 1, order, clip_denoised, t_end, sample, pred_xstart, g_out, total, E);
  RGM_LAUNCH_CHECK();
  return RGM_OK;
}
