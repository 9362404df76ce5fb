/* rgm.h -- C ABI of librgm_hip.so: the MI355X (gfx950) native layer under the reference's Python API.
 *
 * The reference (yjhuangcd/rule-guided-music) has no FFI: its hot path sits behind Python call
 * signatures.  The drop-in keeps those signatures in rule-guided-music_amd/ and
 * binds THIS header with ctypes (rule-guided-music_amd/rgm/native.py); INTEGRATION.md shows the stub.
 * Each entry point cites the reference interface it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; tensors are dense, row-major,
 *     float32 unless stated; all work is enqueued on the hipStream_t passed in (as void*), nothing
 *     synchronises the device, nothing allocates except *_create / *_set_param (weight arena);
 *   - return 0 (RGM_OK) or a negative rgm_status; never throws; rgm_last_error() gives the text
 *     (thread-local, valid until the next call on that thread);
 *   - handles are bound to the device current at *_create, not thread-safe (one per rank);
 *   - workspace is caller-provided memory of at least *_workspace_bytes(), 256-byte aligned.
 */
#ifndef RGM_H
#define RGM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  RGM_OK = 0,
  RGM_ERR_INVALID = -1,   /* bad argument / shape / unknown key */
  RGM_ERR_HIP = -2,       /* a HIP runtime call failed */
  RGM_ERR_WORKSPACE = -3, /* workspace too small */
  RGM_ERR_STATE = -4      /* handle not ready (missing parameters) */
} rgm_status;

int rgm_version(void);
const char* rgm_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * DiTRotary eps-network / DiTRotaryClassifier            guided_diffusion/dit.py:538-634, :735-831
 * ---------------------------------------------------------------------------------------------- */
typedef struct rgm_dit rgm_dit;

typedef struct {
  int32_t depth;        /* 28 for DiTRotary_XL_8 (dit.py:902) */
  int32_t hidden;       /* 1152 */
  int32_t heads;        /* 16 */
  int32_t patch;        /* 8  (FlattenPatchify1D, dit.py:200-227) */
  int32_t in_ch;        /* 4  */
  int32_t out_ch;       /* 4  (learn_sigma False) ; ignored for classifiers */
  int32_t width;        /* input_size[1] = 16 */
  int32_t n_embed;      /* rows of y_embedder.embedding_table (num_classes + 1), 0 = unconditional */
  int32_t kind;         /* 0 eps-net, 1 classifier (cls token + head), 2 chord classifier (key + chord heads) */
  int32_t n_out;        /* classifier: num_classes of classifier_head */
  int32_t max_tokens;   /* largest sequence length that will be used (2*H, +1 for classifiers) */
} rgm_dit_cfg;

int rgm_dit_create(const rgm_dit_cfg* cfg, rgm_dit** out);
void rgm_dit_destroy(rgm_dit* h);
/* Copy one state_dict tensor (key exactly as in the reference module's state_dict()) into
 * the library's weight arena.  dptr: device float32; the caller keeps ownership of its tensor.
 * Replaces nn.Module.load_state_dict on scripts/sample_rule.py:71-73, :100-102. */
int rgm_dit_set_param(rgm_dit* h, const char* key, const void* dptr, const int64_t* shape, int ndim);
/* number of parameters still unset (0 == ready) */
int rgm_dit_missing_params(rgm_dit* h);
size_t rgm_dit_workspace_bytes(const rgm_dit* h, int N, int H);
/* DiTRotary.forward(x, t, y) dit.py:618-634.  x (N,in_ch,H,width); t (N) int64 (already re-spaced);
 * y (N) int32 row of the label table or NULL; eps (N,out_ch,H,width). */
int rgm_dit_forward(rgm_dit* h, const float* x, const int64_t* t, const int32_t* y, float* eps,
                    int N, int H, void* ws, size_t ws_bytes, void* stream);
/* The adaLN modulation of U (t, y) pairs: rows[U][(6 depth + 2) hidden] = adaLN_modulation(SiLU(t_embedder(t) + y_embedder(y))) of every
 * block and the final layer (dit.py:621-628, :333, :374) -- exactly what rgm_dit_forward computes for a sample with that timestep and label,
 * row by row (a row's arithmetic does not depend on the batch it sits in).  One pass over the adaLN weights (0.9 GB for XL) per 32 pairs.
 * A sampler that knows its schedule (gaussian_diffusion.py:833-880: the loop visits fixed timesteps) asks for the next steps' rows at once
 * and passes them to rgm_dit_forward_cond: sample i takes rows[idx[i]] (idx: device int32, 0 <= idx[i] < U).  ws as for N = U rows. */
int rgm_dit_cond_rows(rgm_dit* h, const int64_t* t, const int32_t* y, int U, int H, float* rows, void* ws, size_t ws_bytes, void* stream);
int rgm_dit_forward_cond(rgm_dit* h, const float* x, const float* rows, const int32_t* idx, int U, float* eps,
                         int N, int H, void* ws, size_t ws_bytes, void* stream);
/* DiTRotaryClassifier.forward dit.py:803-831.  logits (N,n_out) [kind 1]  or  key (N,25) + chord
 * (N,H/width,n_out) [kind 2; key_out may be NULL]. */
int rgm_dit_classify(rgm_dit* h, const float* x, const int64_t* t, float* logits, float* key_out,
                     int N, int H, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Building blocks (exported for parity tests and for composing other callers)
 * ---------------------------------------------------------------------------------------------- */
/* C[M,N] = act(alpha * A[M,K] . B[N,K]^T + bias[N]) (* gate) (+ res); fp32 MFMA (v_mfma_f32_32x32x2_f32).
 * act: 0 none, 1 SiLU, 2 GELU(tanh).  gate (or NULL): gate[(row / rows_per_gate) * gate_ld + col].
 * res (or NULL, may alias C): res[row * ldres + col].  K % 32 == 0.  nn.Linear / 1x1 conv. */
int rgm_gemm(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K,
             const float* bias, int act, float alpha, const float* gate, int gate_ld, int rows_per_gate,
             const float* res, int ldres, void* stream);
/* out = LN(x; eps, no affine) * (1 + scale[b]) + shift[b]   (dit.py:25-26, :334-335); b = row / rows_per_batch;
 * shift/scale rows have stride mod_ld.  weight/bias (affine LN, dit.py:770) optional; shift/scale optional. */
int rgm_layernorm_modulate(const float* x, float* out, int M, int D, float eps, const float* weight,
                           const float* bias, const float* shift, const float* scale, int mod_ld,
                           int rows_per_batch, void* stream);
/* adaLN conditioning of a whole forward in one weight-streaming pass (csrc/adaln_stream.hip): mod[N, L] = cs[N, D] . W^T[L, D] + bias[L],
 * cs = SiLU(c) -- the Linear of every block's adaLN_modulation (ref guided_diffusion/dit.py:318-322, 333) and of the final layer (:366-369,
 * 374), whose weights the DiT handles keep contiguous.  Exact fp32 (v_mfma_f32_16x16x4_f32); one pass over the weights per 32 rows.  N <= 256, D in {384, 768, 1152}, L % 16 == 0,
 * 16-byte aligned pointers; RGM_ERR_INVALID for any other shape (rgm_dit_forward then runs its tiled GEMM instead). */
int rgm_adaln_stream(const float* cs, const float* W, const float* bias, float* mod, int N, int D, int L, void* stream);
/* RotaryAttention core (dit.py:263-277): qkv (N*T, 3*heads*hd) -> o (N*T, heads*hd); rotary on the first
 * 2*rot_half channels of q,k with cos/sin tables (T, rot_half); softmax scale hd^-0.5. hd in {64,72}, 1 <= T <= 8192.
 * A head's K and V stay in LDS up to T = 256 (hd 72) / 288 (hd 64); longer sequences run the streaming (flash-style) kernel,
 * csrc/attention_stream.hip, in the same arithmetic. */
int rgm_rotary_attention(const float* qkv, float* o, const float* cos_tab, const float* sin_tab,
                         int N, int T, int heads, int hd, int rot_half, void* stream);
/* the same forward, also writing lse (N*heads*T): log-sum-exp of the scaled scores of every query, the saved quantity of the backward */
int rgm_rotary_attention_lse(const float* qkv, float* o, float* lse, const float* cos_tab, const float* sin_tab,
                             int N, int T, int heads, int hd, int rot_half, void* stream);

/* Arithmetic of the GEMM family (every nn.Linear / conv of the path):
 *   0  exact fp32 products on v_mfma_f32_32x32x2_f32 (default; 157 TFLOP/s peak);
 *   1  "bf16x3": operands split hi+lo bf16 while staged to LDS, a*b ~= ah*bh + ah*bl + al*bh on
 *      v_mfma_f32_32x32x16_bf16 with fp32 accumulation (~2e-5 relative per product; 833 TFLOP/s equivalent peak).
 *   2  "bf16x3_presplit": same products, hi/lo split done once by the producer of each operand; the DiT backbone
 *      GEMMs and the VAE 3x3 convs run on the LDS-DMA kernel (rgm_gemm_split), everything else as mode 1.
 * Process-wide default used by all handles; results stay within the 1e-3 latent tolerance in every mode (tests). */
int rgm_set_gemm_precision(int prec);
int rgm_get_gemm_precision(void);
/* Element type of the hi / lo halves the bf16x3 modes split fp32 operands into -- a build constant of the library: 0 = bf16 (default
 * build), 1 = fp16 (make F16=1 -> librgm_hip_f16.so: 2^-22 instead of 2^-16 per product at the same MFMA rate, fp16's exponent range). */
int rgm_split_dtype(void);
/* Split-row format of the pre-split bf16x3 path (precision 2, "bf16x3_presplit"): a logical fp32 row of K values
 * keeps its K*4 bytes; every block of 32 values is one 128-byte line [32 bf16 hi | 32 bf16 lo] (x ~= hi + lo, both
 * round-to-nearest; K % 32 == 0).  rgm_split_rows converts (rows,K) fp32 -> split (out-of-place); rgm_gemm_split is
 * the LDS-DMA kernel (csrc/gemm2.hip) on operands already in that format (A (M,K), B (N,K) both split):
 * C = act(A . B^T + bias), optionally written split as well (N % 32 == 0).  tile: 0 auto; 1 128x128, 2 128x64,
 * 3 64x64, 5 256x128 (3-stage ring); 21 / 22 = 128x128 / 128x64 with the single-set pipeline; 43 / 44 / 45 / 46 =
 * 128x128 / 128x64 / 256x128 / 64x64 with the cross-iteration register pipeline; 51 / 52 = 128x128 / 128x64 with
 * the loader/consumer split (4 MFMA waves + 4 DMA waves, 3-stage ring). */
int rgm_split_rows(const float* x, float* out, int64_t rows, int K, void* stream);
int rgm_gemm_split(const float* A_split, const float* B_split, float* C, int M, int N, int K, const float* bias,
                   int act, int tile, int out_split, void* stream);
/* the same with explicit row strides (elements; multiples of 32 for split rows): padded rows keep one K-slice of
 * many rows from landing on a few L2 channels when K*4 is a multiple of 2 KiB */
int rgm_split_rows_ld(const float* x, int ld_in, float* out, int ld_out, int64_t rows, int K, void* stream);
int rgm_gemm_split_ld(const float* A_split, int lda, const float* B_split, int ldb, float* C, int ldc, int M, int N, int K,
                      const float* bias, int act, int tile, int out_split, void* stream);
/* The one-wave-per-SIMD kernels (tiles 71 = 256x256, 72 = 512x128; csrc/gemm2.hip PIPE 5): mode 0 keeps the heuristics off them, 1 (default)
 * lets them choose; min_tiles = tiles a VAE conv launch must have before it takes them (default 256: one round of the chip). */
int rgm_set_big_tiles(int mode, int min_tiles);
/* K-sliced fc2 of a DiT block (rgm_dit_forward, pre-split arithmetic): 1 (default) = the kernel that reduces the K slices also writes the
 * next block's adaLN-LayerNorm of each row (ref guided_diffusion/dit.py:334-336 -- same values as the separate LayerNorm launch,
 * tests/test_gpu_fullsize.py), 0 = separate launches.  rgm_fused_reduce_ln_launches: how many launches took the fused route so far. */
int rgm_set_fuse_reduce_ln(int on);
long long rgm_fused_reduce_ln_launches(void);
/* adaLN conditioning of a forward (ref guided_diffusion/dit.py:332, 372: every block's adaLN_modulation(c), 0.9 GB of weights for N rows):
 * 1 = block 0's slice in front of block 0, the rest on a side stream owned by the handle, forked from and joined to the caller's
 * stream by events (still stream-ordered for the caller; capturable) while block 0 computes; 0 (default; measured equal or better) = one
 * GEMM in front of block 0. */
int rgm_set_adaln_overlap(int on);
/* GroupNorm + swish of a ResnetBlock's conv1 output (ref taming/modules/diffusionmodules/model.py:117-126: h = conv1(.); h = norm2(h);
 * h = nonlinearity(h)) inside the conv launch of the decoder: the tiles of an image leave their partial sums, meet at an L2-resident
 * counter (bounded wait) and write normalised split rows -- the separate HBM pass over the tensor disappears.  mode 0 = never, 1 = where
 * the launch qualifies (default), 2 = every tile on the fallback path (raw rows + in-place fix-up kernel; tests).  *prev (optional)
 * receives the previous mode; rgm_gn_fused_launches() counts the launches that took the route. */
int rgm_set_gn_fuse(int mode, int* prev);
long long rgm_gn_fused_launches(void);
/* Tiles of those fused launches whose bounded wait (1 ms) for the image's other tiles ran out -- they write raw rows and a fix-up pass
 * converts them, same values -- since the last reset; synchronises the device; reset != 0 zeroes the counter.  0 on an idle device:
 * a non-zero count says another stream held CUs while a decode ran (each such tile costs up to 1 ms). */
long long rgm_gn_fallback_tiles(int reset);
/* Blocks of an eps-network forward (ref guided_diffusion/dit.py:618-634: samples are independent inside a block) as TWO half batches, the
 * second on a side stream owned by the handle, forked from and joined to the caller's stream by events (stream-ordered for the caller):
 * one half's kernels fill the CUs the other half's last round of one-workgroup-per-CU tiles leaves idle.  Batches of at least
 * min_batch samples take it; 0 = never; -1 (default) = the batch sizes where a same-box sweep found it ahead (2, 5..9, 17..39, 57..).
 * *prev (optional) receives the previous setting. */
int rgm_set_dit_halves(int min_batch, int* prev);
/* Epilogue of the 128x144 pre-split GEMM tile (tile 81: proj / fc2 of a DiT block at the samplers' batches): 0 = four consumer waves write
 * bias / activation / gate / residual straight from their accumulators; 1 = the tile passes through the (then idle) operand ring and all
 * eight waves move whole 576-byte rows.  Identical results.  Default: RGM_G144_EPI, else 1.  *prev (optional) receives the previous mode;
 * another mode is RGM_ERR_INVALID and changes nothing. */
int rgm_set_gemm144_epilogue(int mode, int* prev);
/* Short-sequence attention of the bf16x3 modes at head_dim 72 (T <= 128: C5's half windows; ref guided_diffusion/dit.py:263-288) with TWO
 * workgroups per CU (four waves and 79 KiB of LDS each) instead of the one-per-CU guard of round 3: the guard answered a hazard of the
 * interleaved Q prologue, which the two-phase prologue removed (profiles/r05_attn_hazard_two_phase_n96.txt).  1 = on,
 * 0 = guard (default).  Returns the previous setting. */
int rgm_set_attn_pairs(int on);
/* The streaming attention forward (csrc/attention_stream.hip) for EVERY sequence length of hd 64 / 72, not only where the resident
 * kernels cannot hold a head: comparisons of the two on the same inputs.  1 = on, 0 = off (default).  Returns the previous setting. */
int rgm_set_attn_stream(int on);
/* Deterministic split-K of the pre-split GEMM (csrc/gemm2.hip: K slices as a batch + one fixed-order reduce kernel, which for the fc2
 * of a DiT block also writes the next adaLN-LayerNorm): the scratch is caller memory like every other workspace,
 * rgm_gemm_scratch_bytes(M, N) bytes for GEMMs of up to M rows and N columns, 16-byte aligned, no initialisation.  tile 0 lets the
 * heuristic choose. */
size_t rgm_gemm_scratch_bytes(int M, int N);
int rgm_gemm_split_ws(const float* A_split, const float* B_split, float* C, int M, int N, int K, const float* bias, int act,
                      int tile, int out_split, void* ws, size_t ws_bytes, void* stream);
/* The general pre-split entry: C = (act(alpha * A . B^T + bias)) * gate + res with explicit row strides (elements), the per-sample
 * adaLN gate gate[(row / rows_per_gate) * gate_ld + col] and a residual that may alias C (the proj / fc2 epilogue of a DiT block,
 * guided_diffusion/dit.py:332-336), explicit tile as in rgm_gemm_split (71.. = the one-wave-per-SIMD tiles) and the
 * caller's scratch (NULL: no workspace-backed decomposition).  The tiles above 128x128 (5, 45, 71, 72, 73) take a gate only with
 * rows_per_gate >= 32 (RGM_ERR_INVALID otherwise); tile 0 keeps finer gates on the 128-row kernels. */
int rgm_gemm_split_epi(const float* A_split, int lda, const float* B_split, int ldb, float* C, int ldc, int M, int N, int K,
                       const float* bias, int act, float alpha, const float* gate, int gate_ld, int rows_per_gate,
                       const float* res, int ldres, int tile, int out_split, void* ws, size_t ws_bytes, void* stream);
/* Same as rgm_gemm without gate/residual but with an explicit tile shape in the low 4 bits (1: 128x128,
 * 2: 128x64, 3: 64x64, 4: 32x128, 0: auto) and an explicit precision in bits 4.. (0: library default,
 * 1: fp32, 2: bf16x3) -- used by the parity tests and tile-selection experiments. */
int rgm_gemm_tile(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K,
                  const float* bias, int act, int tile, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Sampler step kernels                                   guided_diffusion/gaussian_diffusion.py
 * `tables_host`: HOST array of 8 DEVICE pointers to the float32-cast schedule tables (length = number of
 * re-spaced timesteps), in this order: sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod,
 * posterior_mean_coef1, posterior_mean_coef2, model_variance (FIXED_LARGE, :316-329), model_log_variance,
 * alphas_cumprod, alphas_cumprod_prev  -- i.e. what _extract_into_tensor (:1331-1344) would upload per call.
 * t: (N) int64 indices into those tables.  E = elements per sample.
 * ---------------------------------------------------------------------------------------------- */
/* Counter-based N(0,1): element i depends only on (seed, offset+i) (Philox4x32-10 + Box-Muller).
 * Replaces th.randn / th.randn_like at :846, :699, :715, :944, :512. */
int rgm_randn(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream);
/* p_mean_variance + condition_mean + p_sample update (:252-357, :402-407, :698-703):
 *   x0 = c1 x - c2 eps (clip) ; mean = pc1 x0 + pc2 x (+ var * grad) ; sample = mean + [t > t_end] exp(.5 logvar) noise.
 * grad / noise may be NULL (noise NULL -> sample = mean).  g_out (N) or NULL receives exp(.5 logvar). */
int rgm_ddpm_step(const float* x, const float* eps, const float* grad, const float* noise, const int64_t* t,
                  const float* const* tables_host, int clip_denoised, int t_end, float* sample, float* pred_xstart,
                  float* g_out, int N, int E, void* stream);
/* The same step with LEARNED variances (learn_sigma=True checkpoints; p_mean_variance :299-313): var_values (N,E) is the second
 * half of the network's output; min_log_tab / max_log_tab (device float32 tables: posterior_log_variance_clipped, log(betas))
 * give log var = frac max + (1 - frac) min, frac = (v + 1) / 2 (LEARNED_RANGE); both NULL: var_values is the log-variance (LEARNED). */
int rgm_ddpm_step_learned(const float* x, const float* eps, const float* var_values, const float* min_log_tab,
                          const float* max_log_tab, const float* grad, const float* noise, const int64_t* t,
                          const float* const* tables_host, int clip_denoised, int t_end, float* sample, float* pred_xstart, int N,
                          int E, void* stream);
/* ... also writing the per-element noise scale g_elem (N,E) = exp(0.5 log_variance): the tensor g_coeff p_sample hands scg_sample at
 * a learned-variance step (:706-711).  Per-element candidates: rgm_scg_candidates(mean, g_elem, noise, cand, n, N*E, 1). */
int rgm_ddpm_step_learned_g(const float* x, const float* eps, const float* var_values, const float* min_log_tab,
                            const float* max_log_tab, const float* grad, const float* noise, const int64_t* t,
                            const float* const* tables_host, int clip_denoised, int t_end, float* sample, float* pred_xstart,
                            float* g_elem, int N, int E, void* stream);
/* ddim_sample (:881-952) incl. condition_score (:467-489) when grad != NULL; g_out receives sigma. */
int rgm_ddim_step(const float* x, const float* eps, const float* grad, const float* noise, const int64_t* t,
                  const float* const* tables_host, int clip_denoised, int t_end, float eta, float* sample,
                  float* pred_xstart, float* g_out, int N, int E, void* stream);
/* One step of DPM-Solver++(2M) in data-prediction form (csrc/dpm.hip; no counterpart in the reference).  With lambda_i = 1/2 log(abar_i /
 * (1 - abar_i)) and h = lambda_{i-1} - lambda_i, at chain index i = t[b]:
 *   x0 = c1 x - c2 eps (clip), then condition_score exactly as rgm_ddim_step applies it when grad != NULL;
 *   D = x0 + w1[i] (x0 - x0_prev), w1 = 1 / (2 r0), r0 = (lambda_i - lambda_{i+1}) / h; D = x0 when x0_prev is NULL, order == 1,
 *       i == num_timesteps - 1 (no earlier estimate) or i == 0 (the target has abar = 1);
 *   sample = cx[i] x + cd[i] D + [i != t_end] cn[i] noise; at i == 0 the sample is D itself, bit for bit.
 * dpm_tables_host: HOST array of 4 DEVICE float32 tables of length num_timesteps -- cx, cd, w1, cn -- built by the caller in float64:
 *   ODE: cx = sigma_s / sigma_t, cd = -alpha_s expm1(-h), cn = 0;  SDE: cx = sigma_s / sigma_t e^-h, cd = -alpha_s expm1(-2h),
 *   cn = sigma_s sqrt(-expm1(-2h));  entry 0 (h = inf) is cx = 0, cd = 1, cn = 0.  tables_host as above (entries 0, 1 and 6 are read).
 * noise NULL -> sample is the mean; pred_xstart receives x0 (the next step's x0_prev); g_out (N) or NULL receives cn[t]. */
int rgm_dpmpp_step(const float* x, const float* eps, const float* grad, const float* x0_prev, const float* noise, const int64_t* t,
                   const float* const* tables_host, const float* const* dpm_tables_host, int num_timesteps, int order,
                   int clip_denoised, int t_end, float* sample, float* pred_xstart, float* g_out, int N, int E, void* stream);
/* ddim_reverse_sample (:978-1014), the DDIM ODE towards noise (eta = 0): x0 = c1 x - c2 eps (clip); eps' = (c1 x - x0) / c2 (re-derived,
 * so a clip shows in it); sample = sqrt(abar_next) x0 + sqrt(1 - abar_next) eps', abar_next = alphas_cumprod[t + 1], 0 at the last index
 * t == num_timesteps - 1 (the chain length = the tables' length).  Evaluated in fp64 per element, stored as fp32. */
int rgm_ddim_reverse_step(const float* x, const float* eps, const int64_t* t, const float* const* tables_host, int num_timesteps,
                          int clip_denoised, float* sample, float* pred_xstart, int N, int E, void* stream);
/* _vb_terms_bpd (:1145-1178) and the two per-step errors of calc_bpd_loop (:1311-1314) in one pass.  Per sample b:
 *   vb[b]         t[b] > 0: mean of normal_kl(q_posterior_mean(x_start, x_t), post_logvar_tab[t], model_mean, model_log_variance);
 *                 t[b] == 0: mean of -discretized_gaussian_log_likelihood(x_start, model_mean, 0.5 model_log_variance); both / ln 2
 *   xstart_mse[b] mean((pred_xstart - x_start)^2)                                   (may be NULL)
 *   eps_mse[b]    mean(((c1 x_t - pred_xstart) / c2 - noise)^2), needs noise         (both may be NULL)
 *   pred_xstart   (N,E) or NULL: c1 x_t - c2 eps, clipped to [-1, 1] if asked.
 * Variances: tables_host[5] (fixed), or var_values (N,E) with min_log_tab / max_log_tab exactly as rgm_ddpm_step_learned takes them.
 * post_logvar_tab: device float32 posterior_log_variance_clipped.  model_mean (N,E) or NULL: the network's own mean (PREVIOUS_X)
 * instead of the posterior mean of pred_xstart; model_xstart (N,E) or NULL: the x0 estimate itself instead of c1 x_t - c2 eps (eps may
 * then be NULL).  partials: device scratch of rgm_vb_terms_partials(N, E) doubles.  fp64 per element; fixed partition of E into
 * chunks of 2048 and a fixed combination order, no atomics: bitwise repeatable, and a sample's outputs do not depend on N or its row. */
int64_t rgm_vb_terms_partials(int N, int E);
int rgm_vb_terms(const float* x_start, const float* x_t, const float* eps, const float* noise, const int64_t* t,
                 const float* const* tables_host, const float* post_logvar_tab, const float* var_values, const float* min_log_tab,
                 const float* max_log_tab, const float* model_mean, const float* model_xstart, int clip_denoised, double* partials,
                 float* vb, float* xstart_mse, float* eps_mse, float* pred_xstart, int N, int E, void* stream);
/* _prior_bpd (:1255-1272): out[b] = mean(normal_kl(sqrt_alphas_cumprod[T-1] x_start, log_one_minus_alphas_cumprod[T-1], 0, 0)) / ln 2;
 * the two table entries as float32 values; the same reduction (partials: rgm_vb_terms_partials(N, E) doubles suffice). */
int rgm_prior_bpd(const float* x_start, float sqrt_alphas_cumprod_T, float log_one_minus_alphas_cumprod_T, double* partials, float* out,
                  int N, int E, void* stream);
/* scg_sample candidate expansion (:509-514): cand[k][b] = mean[b] + g[b] * noise[k][b], k < n. */
int rgm_scg_candidates(const float* mean, const float* g, const float* noise, float* cand, int n, int B, int E,
                       void* stream);
/* _predict_xstart_from_eps (:359-364) times out_scale (the 1/scale_factor of _decode :1350). */
int rgm_xstart_from_eps(const float* x, const float* eps, const int64_t* t, const float* const* tables_host,
                        float out_scale, float* out, int N, int E, void* stream);
/* Replacement-based conditioning of the editing path (p_mean_variance :293-298): x0 = clip(predict_xstart(x, eps)),
 * x0r = mask*gt + (1-mask)*x0, eps_out = predict_eps_from_xstart(x, x0r).  gt, mask (N,E) like x; eps_out may alias eps. */
int rgm_edit_replace_eps(const float* x, const float* eps, const float* gt, const float* mask, const int64_t* t,
                         const float* const* tables_host, int clip_denoised, float* eps_out, int N, int E, void* stream);
/* scg_sample selection (:539-554): max_ind[b] = first argmax_k total[k][b]; out[b] = cand[max_ind[b]][b].
 * cand and out may both be NULL (index only); max_ind may be NULL. */
int rgm_scg_select(const float* cand, const float* total_logp, float* out, int64_t* max_ind, int n, int B, int E,
                   void* stream);
/* Sharded SCG (SURVEY 8e option i; replaces the gather `sample[max_ind, arange(B)]` of :553-554 / :587-589 when the winner
 * was scored on another rank): out[b] = mean[b] + g[b] * z, z = the rgm_randn stream (seed) at positions
 * base + (k*B + b)*E + e with k = max_ind[seg][b]; the latent row h of (C,H,W) belongs to segment h / seg_rows
 * (max_ind is (S,B), S = ceil(H / seg_rows); seg_rows >= H: one winner per sample).  No host read of max_ind. */
int rgm_scg_rebuild(const float* mean, const float* g, const int64_t* max_ind, uint64_t seed, uint64_t base, float* out,
                    int B, int E, int H, int W, int seg_rows, void* stream);
/* the same with a per-element noise scale g_elem (B,E) (learned variances) */
int rgm_scg_rebuild_g(const float* mean, const float* g_elem, const int64_t* max_ind, uint64_t seed, uint64_t base, float* out,
                      int B, int E, int H, int W, int seg_rows, void* stream);

/* ------------------------------------------------------------------------------------------------
 * taming KL-VAE decoder (f8-all-onset config)            taming/models/klvae_pedal.py:80-85,
 *                                                        taming/modules/diffusionmodules/model.py:436-537
 * ---------------------------------------------------------------------------------------------- */
typedef struct rgm_vae rgm_vae;
int rgm_vae_create(rgm_vae** out);
void rgm_vae_destroy(rgm_vae* h);
/* key as in the Lightning checkpoint's ["state_dict"] ("decoder.*", "post_quant_conv.*"; klvae_pedal.py:50-59).
 * 3x3 conv weights are repacked to [cout][tap][cin] on the device.  "encoder.*" / "quant_conv.*" are optional (only
 * rgm_vae_encode needs them); other prefixes (loss.) are not ours: query with rgm_vae_has_param and skip them
 * (strict=False semantics). */
int rgm_vae_set_param(rgm_vae* h, const char* key, const void* dptr, const int64_t* shape, int ndim);
int rgm_vae_has_param(rgm_vae* h, const char* key);
int rgm_vae_missing_params(rgm_vae* h);            /* decoder + post_quant_conv parameters still unset (what decode needs) */
int rgm_vae_encoder_missing_params(rgm_vae* h);    /* encoder + quant_conv parameters still unset (what encode needs) */
size_t rgm_vae_workspace_bytes(const rgm_vae* h, int M /* number of 16x16 latent squares */);
/* AutoencoderKL.decode(z): z (M,4,16,16) -> out (M,3,128,128). */
int rgm_vae_decode(rgm_vae* h, const float* z, float* out, int M, void* ws, size_t ws_bytes, void* stream);
/* _decode (gaussian_diffusion.py:1347-1358) fused: latent (N,4,H,16) * inv_scale -> H/16 squares per sample ->
 * roll (N,3,128,8H) float32 (may be NULL) and/or roll_u8 (N,128,8H,3) uint8 with the background threshold and
 * truncating cast of decode_sample_for_midi (midi_util.py:59-63) (may be NULL). */
int rgm_vae_decode_latent(rgm_vae* h, const float* latent, float inv_scale, float* roll, uint8_t* roll_u8,
                          float threshold, int N, int H, void* ws, size_t ws_bytes, void* stream);
/* AutoencoderKL.encode_save(x, range_fix=False) (klvae_pedal.py:61-68; Encoder.forward model.py:404-433 incl. the
 * stride-2 Downsample convs :56-75, then quant_conv): x (M,3,128,128) piano-roll tiles in [-1,1] -> moments
 * (M,8,16,16) = mean (channels 0..3) | logvar (4..7).  Workspace as for decode with the same M. */
int rgm_vae_encode(rgm_vae* h, const float* x, float* moments, int M, void* ws, size_t ws_bytes, void* stream);
/* Decoder input gradient -- what torch.autograd computes when the reference's dps_rule branch differentiates
 * rule(_decode(x0_hat)) w.r.t. the latent (gaussian_diffusion.py:415-433 with guidance.nn False; _decode :1347-1358;
 * Decoder.forward model.py:506-537).  Two stream-ordered calls sharing one workspace of
 * rgm_vae_grad_workspace_bytes(h, N*H/16) bytes that the caller leaves untouched in between:
 *   rgm_vae_decode_latent_save: the same roll as rgm_vae_decode_latent, keeping every ResnetBlock's input and conv1
 *     output, the attention tensors and all GroupNorm statistics (~105 MB per 16x16 square) in `ws`;
 *   rgm_vae_decode_latent_vjp:  d_latent (N,4,H,16) = (d roll / d latent)^T d_roll, d_roll (N,3,128,8H).
 * rgm_vae_enable_grad builds the mirrored/transposed weight copies the backward GEMMs read (once, after set_param;
 * ~0.2 GB); the grad calls return RGM_ERR_STATE without it.  Input gradients only -- no parameter gradients. */
int rgm_vae_enable_grad(rgm_vae* h);
size_t rgm_vae_grad_workspace_bytes(const rgm_vae* h, int M /* number of 16x16 latent squares */);
int rgm_vae_decode_latent_save(rgm_vae* h, const float* latent, float inv_scale, float* roll, int N, int H, void* ws,
                               size_t ws_bytes, void* stream);
int rgm_vae_decode_latent_vjp(rgm_vae* h, const float* d_roll, float inv_scale, float* d_latent, int N, int H, void* ws,
                              size_t ws_bytes, void* stream);
/* midi_util.py:59-63 on an existing roll: (B,3,128,T) float32 -> (B,128,T,3) uint8. */
int rgm_quantise_roll(const float* roll, uint8_t* out_u8, int B, int T, float threshold, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Rule programs (FUNC_DICT / LOSS_DICT built-ins)        music_rule_guidance/music_rules.py, rule_maps.py
 * roll (N,C,128,T) float32, channel 0 is read AND WRITTEN (piano_like mask / background threshold, like the
 * reference's in-place view writes).
 * ---------------------------------------------------------------------------------------------- */
/* total_pitch_class_histogram (:29-43): out (N,12); scratch N*128 floats. */
int rgm_rule_pitch_hist(float* roll, float* out, float* scratch, int N, int C, int T, void* stream);
/* rule_x0_mse_dummy for pitch_hist (condition_functions.py:122-126): logp (N) = -scale * ||pitch_hist(roll) - target||^2
 * and d_roll (N,C,128,T) = d logp / d roll (0.5 * d/dh on channel 0's piano rows, 0 elsewhere); hist (N,12) optional;
 * scratch N*140 floats.  Writes the piano_like mask into roll like rgm_rule_pitch_hist. */
int rgm_rule_pitch_hist_vag(float* roll, const float* target, float scale, float* hist, float* logp, float* d_roll,
                            float* scratch, int N, int C, int T, void* stream);
/* note_density (:46-83): out (N, 2*T/interval) = [vertical..., horizontal...]; interval divides 256 and T. */
int rgm_rule_note_density(float* roll, float* out, int N, int C, int T, int interval, float hscale, void* stream);
/* get_chords' preamble (music_rules.py:97-110): piano_like mask and < -0.95 -> -1 written into channel 0 of roll, then
 * clamp((x+1)/2*127, 0, 127) truncated -> out (N,128,T) uint8: the integer roll the host chord analyser (music21) reads. */
int rgm_rule_chord_quantise(float* roll, uint8_t* out, int N, int C, int T, void* stream);
/* The native chord and key analyser of the chord rules, on the integer roll q (N,128,T) uint8 of rgm_rule_chord_quantise.  Its own
 * definition (docs/rounds/chords.md), NOT a restatement of the reference's music21 analyser: agreement with music21 is unmeasured.
 *   active(p,t) = q[p,t] > 0 for the piano pitches 21..108 only; W = T / Wc windows of Wc columns (1 <= Wc <= 1024), the columns
 *   behind W*Wc count for the key only.
 *   key: D[c] = number of active (p,t) with p % 12 == c over all T columns; r_k = Pearson correlation (float64, sums in class order
 *     0..11, no FMA contraction) of D with profile[mode][(c - tonic) % 12] for k = 12*mode + tonic (mode 0 = major); the key is the
 *     first maximum, coef = r_key; sum (D - mean)^2 == 0 (silence, flat profile): key -1, coef 0, all chords 0.
 *   window chord: the longest maximal run of columns with one non-empty set of active pitches (runs cut at window boundaries, the
 *     earliest among equals); its root r maximises 8[r+7] + 4[r+4 or r+3] + 3[r+6] + 2[r+10 or r+11] over its pitch classes (membership
 *     mod 12), ties to the smallest (r - bass) % 12; roots[n][w] = r, or -1 without a sounding column.
 *   chords[n][w] = DEG[(root - tonic) % 12], DEG = 1 2 2 3 3 4 4 5 6 6 7 7, 0 for a silent window.  tonic = given_tonic[n] (0..11)
 *     where given_tonic != NULL and >= 0, else the analysed key's.  analyse_key == 0 (needs given_tonic): no key analysis, key -1 and
 *     coef 0 are written, a sample with given_tonic < 0 gets chords 0.
 * profile: 2 x 12 doubles [major | minor] on the device.  chords (N,W) int64, roots (N,W) int32, key (N) int32, coef (N) float64.
 * ws: N * (T / Wc + 1) * 12 int32.  Two launches, no atomics: bitwise repeatable, a sample's answer independent of N and its row. */
int rgm_rule_chords(const uint8_t* q, int N, int T, int Wc, const double* profile, const int32_t* given_tonic, int analyse_key,
                    int64_t* chords, int32_t* roots, int32_t* key, double* coef, void* ws, size_t ws_bytes, void* stream);
/* mgeval's note statistics on the device                music_evaluation/mgeval/core.py:32-412 (class metrics), over the object of
 * music_rule_guidance/piano_roll_to_chord.py:167-275 (piano_roll_to_pretty_midi) and the fork's pretty_midi/instrument.py:69-207
 * (get_piano_roll), :301-340 (get_pitch_class_transition_matrix), :242-259 (get_end_time).  The values are the reference's for the
 * in-memory object at fs = 100 (tests/golden/notes.npz); the full definition and its quirks are in docs/rounds/notes.md.
 * roll: uint8 cells 0..127, read only, cell (n, c, p, t) at roll + n stride_n + c stride_c + p stride_p + t stride_t (bytes): a
 *   channel-first (N,C,128,T) roll and the (N,128,T,C) tensor of decode_sample_for_midi are both read in place.  C = 1 [velocity],
 *   2 [velocity | pedal], 3 [velocity | onset | pedal]; 1 <= T <= 32768.  first_column_onsets (C = 3): the onset channel counts as 127
 *   in column 0 of every row whose raw velocity there is not 0 (guided_diffusion/midi_util.py:81-85).
 * out_int (N,148) int64: notes n, total_used_pitch, pitch_range, mean_note_velocity (sum // n), pitch_class_transition_matrix (12 x 12,
 *   normalize = 0).  out_real (N,16) float64: end_time, avg_IOI, mean_note_duration, note_density (n / end_time), the 12 values of
 *   total_pitch_class_histogram.  NaN where mgeval answers NaN (avg_IOI for n < 2, the histogram of an empty rebuilt roll).
 * ws: rgm_note_stats_workspace(N, T) bytes (0 for sizes out of range), 8-byte aligned.  Three launches on `stream`, no host sync, no
 * floating-point atomics: bitwise repeatable, a sample's answer independent of N and its row. */
size_t rgm_note_stats_workspace(int N, int T);
int rgm_note_stats(const uint8_t* roll, long long stride_n, long long stride_c, long long stride_p, long long stride_t, int N, int C,
                   int T, int first_column_onsets, int64_t* out_int, double* out_real, void* ws, size_t ws_bytes, void* stream);
/* Float roll (N,C,128,T) in [-1, 1] -> the uint8 roll rgm_note_stats reads: (uint8) clamp((x + 1) * 63.5 + 2^-10, 0, 127), the
 * quantiser of decode_sample_for_midi (midi_util.py:61) with a bias and WITHOUT its background threshold (:60): it inverts
 * u8 / 63.5 - 1, on which scripts/sample_rule.py reports rules, for all 128 levels.  Plain truncation of that round trip loses levels
 * 1..4, 9, 10, 18..21; a threshold at -0.95 would lose 1..3 (3 / 63.5 - 1 = -0.9528).  A caller who wants the decode's threshold
 * on a continuous roll applies it first (docs/rounds/notes.md). */
int rgm_roll_to_u8(const float* roll, uint8_t* out, int N, int C, int T, void* stream);
/* Standard MIDI Files on the device                      guided_diffusion/midi_util.py:67-93 (save_piano_roll_midi) over
 * music_rule_guidance/piano_roll_to_chord.py:167-275 (piano_roll_to_pretty_midi) and the fork's pretty_midi/pretty_midi.py:1341-1520 (write);
 * csrc/midi.hip, docs/rounds/midi.md.  The roll is what rgm_note_stats takes (uint8, four byte strides, C = 1 / 2 / 3, 1 <= T <= 32768,
 * first_column_onsets) and is never written.  The file is byte for byte the one the host writer (SimpleMIDI.write) makes of the same roll:
 * format 1, 220 ticks per quarter, a tempo track and one instrument on channel 0, a status byte on every message, deltas of 1 to 3 bytes.
 * ticks_host: HOST int32 table of T + 1 entries, the tick of every column boundary (time_to_tick(k / fs)); it must start at >= 0, rise by at
 *   least 2 from entry to entry (the column order is then the tick order; true for fs <= 220) and stay below 2^21: a table that does not is
 *   refused with RGM_ERR_INVALID before any launch.  It is copied to the device on `stream` and must stay unchanged until that copy has run.
 * Two calls with one host read of the sizes between them, sharing a workspace the caller leaves untouched in between:
 *   rgm_midi_measure: counts (N,4) int64 = notes, CC events, messages of the whole file (both tracks, end-of-tracks included), file bytes.
 *   rgm_midi_emit: note_off / cc_off / byte_off (N) int64: where sample n's rows and bytes begin in the packed arrays (exclusive sums of
 *     the counts); notes (rows of 4 int32: pitch, velocity, start column, end column, ordered by (pitch, start column); a run that reaches
 *     the right edge ends in column T, a note started by an onset one column behind its run has end == start), ccs (rows of 2 int32: column,
 *     value of controller 64, in column order), bytes (the files, back to back).  *_cap: rows / bytes the arrays hold; a sample that would
 *     not fit is left out whole.  notes / ccs may be NULL with a capacity of 0.  program: 0 .. 127.
 * ws: rgm_midi_workspace(N, T) bytes (0 for sizes out of range), 8-byte aligned; RGM_ERR_WORKSPACE if short.  Three + two launches, no
 * atomics, no floating point: bitwise repeatable, a sample's rows and bytes independent of N and its place in the batch. */
size_t rgm_midi_workspace(int N, int T);
int rgm_midi_measure(const uint8_t* roll, long long stride_n, long long stride_c, long long stride_p, long long stride_t, int N, int C,
                     int T, int first_column_onsets, const int32_t* ticks_host, int64_t* counts, void* ws, size_t ws_bytes, void* stream);
int rgm_midi_emit(int N, int T, int program, const int64_t* note_off, const int64_t* cc_off, const int64_t* byte_off, int32_t* notes,
                  long long notes_cap, int32_t* ccs, long long ccs_cap, uint8_t* bytes, long long bytes_cap, void* ws, size_t ws_bytes,
                  void* stream);
/* Standard MIDI Files read on the device                  music_rule_guidance/piano_roll_to_chord.py (SimpleMIDI._read, midi_to_full_piano_roll),
 * the reference's datasets/piano_roll_all.py and scripts/edit.py:170-171; csrc/midi_read.hip, docs/rounds/midi_read.md.  The definition is the
 * host reader, mirrored byte for byte; its parse step has no reference of its own (mido), its roll builder is pinned to the reference's fork.
 * blob: the N files back to back, 16-byte aligned, its allocation padded to a multiple of 16 bytes; never written.  offsets: N + 1 int64 on the
 *   device, offsets[N] == total_bytes.  total_tracks: the sum of the track counts of the headers (bytes 10..11) of all files of at least 14
 *   bytes that begin with "MThd"; a file whose tracks the total does not cover gets status 9.
 * rgm_midi_read_scan: status (N) int32, counts (N,4) int64 = notes, control changes, tempo entries (the initial one included), instruments,
 *   columns (N) int64 = the T of the host's roll at fs.  Optional: note_off / cc_off (N + 1) int64, the exclusive row offsets over the files;
 *   notes (rows of 8 int64: instrument, channel, pitch, velocity, start tick, end tick, and the BITS of two float64, start and end in
 *   seconds) in (instrument, order of the note-offs) order; ccs (rows of 5 int64: instrument, number, value, tick, bits of the float64
 *   seconds) in (instrument, event) order.  notes and ccs come together; a file whose rows do not fit the capacities is left out whole.
 * rgm_midi_read_rolls (after a scan with the same N, total_bytes, total_tracks, fs and workspace): out (N,3,128,T) = columns [start_column,
 *   start_column + T) of every accepted file's [velocity | onset | pedal] roll, zero beyond the file's own columns and for a refused file;
 *   out_u8 = 0: float32, the host's values; 1: uint8 saturating at 255 with overflow (N) int64 = the number of saturated cells.
 * status: 0 accepted, 1 not a Standard MIDI File, 2 SMPTE or zero division, 3 bad or overrunning track chunk, 4 data ending inside a message,
 *   5 a data byte >= 0x80 in a channel message, 6 more than 2048 tempo entries, 7 no note reaching the first column, 8 a tick >= 2^40 or
 *   2^31 columns, 9 total_tracks too small.  A refused file has zero counts and columns.
 * ws: rgm_midi_read_workspace(N, total_bytes, total_tracks) bytes (0 for sizes out of range: N 1 .. 65535, 1 .. 2^30 bytes, 0 .. 2^26 tracks),
 *   16-byte aligned; RGM_ERR_WORKSPACE if short; RGM_ERR_INVALID for fs <= 0, sizes or pointers, before any launch.  Float64 without
 *   contraction, integer atomics only: bitwise repeatable, a file's results independent of N and of its place in the blob. */
size_t rgm_midi_read_workspace(int N, long long total_bytes, int total_tracks);
int rgm_midi_read_scan(const uint8_t* blob, const int64_t* offsets, int N, long long total_bytes, int total_tracks, double fs, int32_t* status,
                       int64_t* counts, int64_t* columns, int64_t* note_off, int64_t* cc_off, int64_t* notes, long long notes_cap, int64_t* ccs,
                       long long ccs_cap, void* ws, size_t ws_bytes, void* stream);
int rgm_midi_read_rolls(int N, long long total_bytes, int total_tracks, double fs, long long start_column, int T, int out_u8, void* out,
                        int64_t* overflow, void* ws, size_t ws_bytes, void* stream);
/* Audio of a roll on the device: the sine voice          the fork's pretty_midi/pretty_midi.py:954-983 (PrettyMIDI.synthesize, wave = np.sin) over
 * pretty_midi/instrument.py:355-441 (Instrument.synthesize), applied to the notes and pedal events of piano_roll_to_pretty_midi
 * (music_rule_guidance/piano_roll_to_chord.py:167-275); csrc/synth.hip, docs/rounds/synth.md.  The host partner is synthesize_roll.
 * rgm_synth_render reads what rgm_midi_emit left on the device -- notes (rows of 4 int32, 16-byte aligned), ccs (rows of 2 int32), note_off /
 *   cc_off (N) int64, counts (N,4) int64 of rgm_midi_measure; notes_rows / ccs_rows: rows the arrays hold, a sample whose rows lie outside
 *   is rendered without them -- and four HOST tables, formed in float64 on the host so that every truncation is the host partner's own:
 *   samp_host[k] = int(audio_fs * (k / fs)) and len_host[k] = int(audio_fs * (k / fs + 1)), T + 1 int64 each; omega_host[p] = 2 pi f_p * 1.0 /
 *   audio_fs, 128 float64; fade_host = linspace(1, 0, F), F = int(.1 * audio_fs) <= cap / 8 + 16.  The integer tables must start at >= 0, not
 *   decrease, stay below 2^31 and satisfy samp <= len; audio_fs must be positive: otherwise RGM_ERR_INVALID before any launch.  They are
 *   copied on `stream` and must stay unchanged until those copies have run.
 *   wave (N, cap) float64, 16-byte aligned: sample i of a row is the sum over the notes sounding there, in ascending pitch order, of
 *   (((exp(-k / audio_fs) * fade) * velocity) * sin(omega[pitch] * k)), k = i - samp[start]; a note of n = samp[end] - samp[start] samples
 *   fades over its last F samples by the table (n > F) or over all of them by linspace(1, 0, n) (n <= F); zero from the sample's length on.
 *   cap: a multiple of 8, at least len_host[T].  lengths (N) int64 = len[last column holding a note end or a CC]; peak (N) float64 = the
 *   largest magnitude; silent (N) int32 = 1 for a sample without notes or with a peak of 0 (the reference divides 0 by 0 there).
 * rgm_synth_pcm: format 0: out (N, cap) float32 = (float)(wave / peak), the division in float64; format 1: out N WAV files (mono, 16 bit,
 *   `rate` in the header) at a stride of 44 + 2 cap bytes, each with its own length in both size fields, samples (int16) rint((wave / peak) *
 *   32767), zero bytes behind the file's end.  A silent sample gives zeros.  No host read between the two entries.
 * ws: rgm_synth_workspace(N, T, cap) bytes (0 for sizes out of range: N 1 .. 65535, T 1 .. 32768, cap 8 .. 2^31 - 1), 16-byte aligned;
 *   RGM_ERR_WORKSPACE if short.  Two launches + one; IEEE double without contraction, no atomics: bitwise repeatable, a sample's rows
 *   independent of N and of its place in the batch. */
size_t rgm_synth_workspace(int N, int T, long long cap);
int rgm_synth_render(int N, int T, const int32_t* notes, long long notes_rows, const int64_t* note_off, const int32_t* ccs, long long ccs_rows,
                     const int64_t* cc_off, const int64_t* counts, double audio_fs, const int64_t* samp_host, const int64_t* len_host,
                     const double* omega_host, const double* fade_host, int F, double* wave, long long cap, int64_t* lengths, double* peak,
                     int32_t* silent, void* ws, size_t ws_bytes, void* stream);
int rgm_synth_pcm(int N, const double* wave, const int64_t* lengths, const double* peak, long long cap, int format, int rate, void* out,
                  void* stream);
/* Augmented training batches                              guided_diffusion/pr_datasets_all.py (ImageDataset.__getitem__, key_shift),
 * train_util.py (get_kl_input), compute_std.py; csrc/augment.hip; definition, quirks and measurements in docs/rounds/augment.md.
 *
 * rgm_roll_augment: N uint8 excerpts (3, 128, lengths[f]) [velocity | onset | pedal] lie in `blob` at byte offsets[f] (any byte offset; the
 *   blob itself 16-byte aligned, blob_bytes the padded allocation, a multiple of 16; offsets holds N + 1 entries, the last is not read).
 *   params (B, 5) int32 rows (file, start, pr_len, k, flags), flags bit 0: time stretch, bit 1: key shift.  out (B, 3, 128, S) float32:
 *   x = u8 / 63.5f - 1 of columns [start, start + pr_len) resampled to S columns (bit 0; [0, S) otherwise) -- stretched (pr_len < S:
 *   velocity and pedal by torch's nearest map, every source onset kept once, -1 between), compressed (pr_len > S: nearest, an onset of 1.0
 *   where the resampled velocity rises) or copied; velocity and onset rows moved by new[p] = old[(p + |k|) mod 128] (bit 1; k < 0 shifts
 *   the same way as k > 0, the reference's behaviour); pitches < 21 and > 108 set to -1.  status (B) int32: 0 accepted, 1 file index out
 *   of range or the file's extent outside the blob, 2 window outside the file, 3 pr_len < 1 or above rgm_roll_augment_capacity(S) =
 *   ((S + S / 16 + 15) & ~15) + 16 source columns, 4 |k| > 127 -- checked in the order 1, 3, 2, 4; a refused row is -1 throughout, the
 *   other rows are unaffected.  1 <= S <= 16384, 1 <= B <= 2^23.  One launch of 128 B workgroups, no atomics, the blob is only read;
 *   every launch repeats bit for bit and a row's result depends neither on B nor on its position.  Size and pointer errors return a
 *   status before the launch.
 * rgm_latent_windows: moments (n_tiles * B, 8, 16, 16), tile s of sample b in row s * B + b (the encoder's output for the stacked tiles).
 *   z[b, c, 16 s + j, i] = moments[s B + b, c, i, j] (the posterior mode, c < 4);  shift_size = 0: z0 (B, 4, 16 n_tiles, 16) = z *
 *   scale_factor;  shift_size > 0 (n_tiles >= 8): z0[b W + w, c, r, i] = z[b, c, 16 shift_size w + r, i] * scale_factor, r < 128,
 *   W = rgm_latent_windows_count(n_tiles, shift_size) = (16 n_tiles - 128) / (16 shift_size) + 1.  x_t (NULL: skipped), same shape:
 *   sqrt_ac[t[row]] * z0 + sqrt_1mac[t[row]] * noise, two float32 products and a sum; t int64 per output row (clamped into the tables of
 *   num_timesteps float32 entries); noise from the caller's buffer, or (NULL) the values rgm_randn(seed, offset) writes into a tensor of
 *   z0's shape.  One launch.
 * rgm_latent_std: out[3] float64 = mean, unbiased standard deviation (torch.std) and 1 / std of n float32 values: float64 sums and
 *   sums of squares of chunks of 2048 in a fixed order, the chunks added by one wave in a fixed order.  ws: rgm_latent_std_workspace(n)
 *   bytes, 8-byte aligned.  n = 1 gives NaN.  Two launches, no atomics, bitwise repeatable. */
int rgm_roll_augment_capacity(int S);
int rgm_roll_augment(const uint8_t* blob, long long blob_bytes, const int64_t* offsets, const int32_t* lengths, int N, const int32_t* params,
                     int B, int S, float* out, int32_t* status, void* stream);
int rgm_latent_windows_count(int n_tiles, int shift_size);
int rgm_latent_windows(const float* moments, int B, int n_tiles, int shift_size, float scale_factor, float* z0, const int64_t* t,
                       const float* sqrt_ac, const float* sqrt_1mac, int num_timesteps, const float* noise, uint64_t seed, uint64_t offset,
                       float* x_t, void* stream);
size_t rgm_latent_std_workspace(long long n);
int rgm_latent_std(const float* x, long long n, double* out, void* ws, size_t ws_bytes, void* stream);
/* The set-level half of mgeval                           music_evaluation/music_evaluator.py:117-186, mgeval/utils.py (c_dist, kl_dist,
 * overlap_area), csrc/sets.hip; definition, quirks and measurements in docs/rounds/sets.md.  Everything is float64 on `stream` in the
 * caller's workspace (8-byte aligned), no host sync, no atomics, no FMA contraction; every sum has one owner and a fixed order and the
 * chunking is a constant of the build, so a result depends on its inputs alone and repeats bit for bit.  Size errors return a status
 * before any launch.
 *
 * rgm_set_distances: a (Na,d), b (Nb,d) row-major, 1 <= Na, Nb <= 32768, 1 <= d <= 144.  out[i][j] = sqrt(sum_k (a[i,k] - b[j,k])^2),
 *   summed in k order; NaN and +-inf results are written as 0 (music_evaluator.delete_nan).  skip_diagonal (needs Na == Nb >= 2): a
 *   row holds the Nb - 1 entries j != i in ascending j -- the leave-one-out loop after its transpose and reshape.
 * rgm_kde_pdf: scipy.stats.gaussian_kde(data)(x) for one-dimensional data: h = sqrt(sum (y - mean)^2 / (n - 1)) n^(-1/5),
 *   pdf(x) = sum_j exp(-((x - y_j) / h)^2 / 2) / (n h sqrt(2 pi)), (x - y) / h formed per pair.  1 <= n <= 2^24, 1 <= m <= 2^20; n < 2
 *   or a zero variance writes NaN to every output (no status: the caller cannot know without a sync).  ws: rgm_kde_pdf_workspace(n, m).
 * rgm_set_kl_oa: kl_dist(A, B, kl_points) and overlap_area(A, B) in one call.  KL = sum p log(p / q) (scipy.special.rel_entr's rules for
 *   zeros) of pdf_A on linspace(min A, max A, kl_points) and pdf_B on linspace(min B, max B, kl_points) -- two different point sets, the
 *   reference's definition -- each divided by its sum.  OA = the composite Simpson rule of min(pdf_A, pdf_B) on oa_panels + 1 equally
 *   spaced points over [min(min A, min B), max(max A, max B)], in place of QUADPACK's adaptive rule.  linspace is lo + i (hi - lo) /
 *   (points - 1) with the last point equal to hi.  2 <= nA, nB <= 2^24, 2 <= kl_points <= 4096, oa_panels even in 2 .. 65536 (the
 *   Python surface defaults to 1000 and 16384).
 *   out[8]: KL, OA, |OA(oa_panels) - OA(oa_panels / 2)| (NaN unless oa_panels is a multiple of 4), h_A, h_B, lo, hi, flag.  flag = 1 and
 *   KL = OA = NaN where a variance is 0 (the reference raises LinAlgError there).  ws: rgm_set_kl_oa_workspace(...) bytes (0 for sizes out
 *   of range): 16 (1 + chunks) (kl_points + oa_panels + 1) + 128, chunks = ceil(max(nA, nB) / 16384).  Four launches. */
int rgm_set_distances(const double* a, int Na, const double* b, int Nb, int d, int skip_diagonal, double* out, void* stream);
size_t rgm_kde_pdf_workspace(int n, int m);
int rgm_kde_pdf(const double* data, int n, const double* x, int m, double* pdf, void* ws, size_t ws_bytes, void* stream);
size_t rgm_set_kl_oa_workspace(int nA, int nB, int kl_points, int oa_panels);
int rgm_set_kl_oa(const double* A, int nA, const double* B, int nB, int kl_points, int oa_panels, double* out, void* ws, size_t ws_bytes,
                  void* stream);
/* torch.bucketize(v, bounds) as used by note_density_class (:86-94): out int64. */
int rgm_bucketize(const float* v, const float* bounds, int nb, int64_t* out, int n, void* stream);
/* mse_loss_mean / zero_one_loss_mean (rule_maps.py:17-22) over the last dim: a,b (rows,K) -> out (rows). */
int rgm_row_loss(const float* a, const float* b, float* out, int rows, int K, int zero_one, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Classifier guidance backward                            guided_diffusion/condition_functions.py:58-85
 * ---------------------------------------------------------------------------------------------- */
/* Value and input-gradient of a DiTRotaryClassifier log-probability in one call (replaces
 * th.autograd.grad(log_probs.sum(), x_in) * classifier_scale; weights are frozen, so only dgrad runs):
 *   loss_kind 0 (kind-1 handle): log p = -sum_k (logits - target)^2, target float32 (N, n_out)    [grad_nn_zt_mse]
 *   loss_kind 1 (kind-2 handle): log p = -sum_w CE(chord_logits[w], target[w]), target int64 (N, H/width)
 *                                                                                 [grad_nn_zt_chord, both=False]
 *   loss_kind 1 (kind-1 handle): log p = log softmax(logits)[target], target int64 (N,)             [grad_nn_zt_xentropy :46-56]
 * grad_x (N,in_ch,H,width) = d(sum log p)/dx * scale;  logits_out (N[,H/width], n_out) or NULL.
 * Any H the handle's max_tokens allows (classifiers: H*width/patch + 1 tokens): beyond 256 (hd 72) / 288 (hd 64) tokens the attention
 * backward streams (csrc/attention_bwd_stream.hip).  The workspace keeps every block's activations: 40 * hidden bytes per token and block. */
size_t rgm_dit_grad_workspace_bytes(const rgm_dit* h, int N, int H);
int rgm_dit_cls_value_and_grad(rgm_dit* h, const float* x, const int64_t* t, const void* target, int loss_kind,
                               float scale, float* logits_out, float* grad_x, int N, int H, void* ws,
                               size_t ws_bytes, void* stream);
/* Input gradient of the eps-network -- the autograd step of DPS guidance (condition_mean, gaussian_diffusion.py:415-465:
 * th.autograd.grad(log_probs.sum(), xt) through pred_xstart(xt, model(xt))): eps_out = model(x, t, y) (optional) and
 * grad_x = (d eps / d x)^T g_eps, via the saved-activation forward and the same dgrad chain as the classifiers.
 * rgm_dit_enable_grad(h) first: it keeps W^T copies of the eps-network's Linear weights (1.8 GB at XL); workspace =
 * rgm_dit_grad_workspace_bytes(h, N, H).  Two phases that may be separate calls on the same workspace: forward
 * (x, t [, y] given; g_eps/grad_x NULL) saves the activations and writes eps_out; backward (x NULL; g_eps, grad_x given)
 * consumes them -- DPS forms g_eps from the classifier's gradient at x0(eps) in between.  Any H the handle's max_tokens allows. */
int rgm_dit_enable_grad(rgm_dit* h);
int rgm_dit_vjp(rgm_dit* h, const float* x, const int64_t* t, const int32_t* y, const float* g_eps, float* eps_out,
                float* grad_x, int N, int H, void* ws, size_t ws_bytes, void* stream);
/* Attention launches of the classifier path (DiTRotary-S/8-cls: 257 tokens = 9 tiles of 32 on 8 waves, 6 heads x the sampler's batch of
 * (sample, head) pairs on 256 CUs; ref guided_diffusion/dit.py:803-831 + condition_functions.py:58-64): -1 (default) = per-tile workgroups
 * (backward: one per query / key tile, partial sums through LDS in a fixed order; forward: two per (sample, head)) whenever the
 * (sample, head) grid would leave CUs idle, 0 = never, 1 = always.  Same values to the last bit of the summation order. */
int rgm_set_attn_split(int mode);
/* The streaming attention backward (csrc/attention_bwd_stream.hip) for EVERY sequence length of hd 64 / 72, not only where the resident
 * kernels cannot hold a head: comparisons of the two on the same inputs, tests.  1 = on, 0 = off (default).  Returns the previous
 * setting.  rgm_attn_bwd_stream_launches: how many backward launches took the streaming pair so far in this process. */
int rgm_set_attn_bwd_stream(int on);
long long rgm_attn_bwd_stream_launches(void);
/* d(qkv) (N*T, 3*heads*hd) of the RotaryAttention core from dO, the saved qkv, O and per-query log-sum-exp (N, heads, T); hd in {64, 72},
 * 1 <= T <= 8192.  Q / dO resp. K / V of a head stay in LDS up to T = 256 (hd 72) / 288 (hd 64) -- the resident kernels,
 * csrc/attention_bwd.hip; longer sequences run the streaming (flash-style) pair, csrc/attention_bwd_stream.hip, in the same arithmetic:
 * deterministic, no atomics. */
int rgm_rotary_attention_bwd(const float* qkv, const float* o, const float* d_o, const float* lse, float* dqkv,
                             const float* cos_tab, const float* sin_tab, int N, int T, int heads, int hd,
                             int rot_half, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Measurement hooks (bench.py roofline leg): with profiling on, every GEMM launch is bracketed by two
 * hipEvents recorded on the launch stream.  kernel ids: gemm.hip = tile (1..5: 128x128 / 128x64 / 64x64 /
 * 32x128 / 256x128) + 10 with the implicit 3x3-conv loader + 20 in bf16x3; gemm2.hip = 40 + tile (as in
 * rgm_gemm_split) + 10 with the conv loader.
 * rgm_gemm2_dbg: s_memtime stamps of the gemm2 K loop (tools/gemm_stamp.py; library built with
 * -DRGM_GEMM2_STAMPS): mode 1 arm, 2 copy 64 counters to out64, 0 off.
 * ---------------------------------------------------------------------------------------------- */
int rgm_prof_enable(int on);
int rgm_prof_reset(void);
int rgm_prof_report(int kernel, int* launches, double* total_ms, double* total_flops);
/* algorithmic HBM bytes (every operand read once, the output written once) summed over the recorded launches of a pre-split kernel id */
double rgm_prof_bytes(int kernel);
/* per-launch records of the pre-split GEMM kernels in launch order (kernel id, milliseconds, algorithmic FLOPs); returns the count */
int rgm_prof_dump(int cap, int* ids, double* ms, double* flops);
int rgm_gemm2_dbg(int mode, long long* out64);
/* the same for the 128x144 kernel (gemm144.hip, tools/g144_stamp.py): always built; 8 waves x 8 slots (cycles of the middle workgroup).
 * mode 1 arms, 2 copies the 64 slots out, 3 copies 64 + 8 x 4096 values (per workgroup of the stamped launch: entry / exit in shader cycles,
 * entry / exit on the 100 MHz wall clock, K loop, epilogue, prologue cycles, raster id -- tools/g144_insitu_stamp.py ALLWG=1), 0 disarms */
int rgm_gemm144_dbg(int mode, long long* out64);

/* ------------------------------------------------------------------------------------------------
 * DiffCollage long-sequence composition                   diff_collage/w_img.py, condind_long.py, condind_circle.py
 * ---------------------------------------------------------------------------------------------- */
/* split_wimg (:8-24): img (B,C,h,W) -> wins (B*n,C,h,128), window i at columns [i*(128-overlap), +128), read
 * circularly (column >= W wraps) so the circular variant needs no concatenated copy.  halves (B*n,C,h,overlap)
 * or NULL receives the right `overlap` columns of every window (input of the half-window eps call). */
int rgm_collage_split(const float* img, float* wins, float* halves, int B, int C, int h, int W, int n, int overlap,
                      void* stream);
/* get_eps_t_fn tail (condind_long.py:36-50 / condind_circle.py:57-82): out = fold-sum of full_i minus half_i
 * (i < n-1) on the right overlaps; circle != 0 averages the wrapped seam; is_avg divides by the coverage
 * count (avg_merge_wimg is_avg=True).  half may be NULL (plain merge). */
int rgm_collage_merge(const float* full, const float* half, float* out, int B, int C, int h, int n, int overlap,
                      int circle, int is_avg, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Particle rule guidance (sequential Monte Carlo)          csrc/particles.hip, docs/rounds/particles.md
 * ---------------------------------------------------------------------------------------------- */
/* One weighting-and-resampling step for B groups of n particles, particle k of group b at index k*B + b (SCG's candidate layout).
 * Per group, in float64:
 *   r_k   = reward[k], with NaN and +inf counted as -inf (a broken particle dies; rgm_scg_select keeps argmax's NaN-as-max instead)
 *   l_k   = logw[k] + lambda (r_k - r_prev[k]); -inf where r_k or logw[k] is -inf.  r_prev[k] <- r_k where r_k is finite.
 *   w_k   = exp(l_k - max l) / sum, ESS = 1 / sum w_k^2 -> ess_out[b]
 *   resample iff ESS < ess_frac n (ess_frac <= 0: never, > 1: always).  Every weight 0: no resampling, logw <- 0, resampled[b] = -1,
 *   ess_out[b] = 0, anc[k] = k.
 *   resampling is systematic: c_j = w_0 + ... + w_j in ascending j, c_{n-1} counted as +inf, anc[k] = min{j : c_j > (k + u) / n}
 *   (strict: a zero-weight particle is never chosen); then logw <- 0, r_prev[k] <- r_prev[anc[k]], resampled[b] = 1.
 *   otherwise anc[k] = k, logw[k] <- l_k - logsumexp(l) + log n (uniform weights are 0), resampled[b] = 0.
 * u: B float64 on the device in [0, 1), or NULL: u_b = (w0 + 0.5) 2^-32 with w0 the first word of Philox4x32-10 block
 * (seed, counter + b) -- the generator of rgm_randn.  logw (float64) and r_prev (float32) are updated in place; anc int32 (n, B),
 * ess_out float64 (B), resampled int32 (B).  1 <= n <= 1024.  One workgroup per group, every sum with one owner in ascending k: a
 * group's result depends neither on B nor on its position, and launches repeat bit for bit. */
int rgm_particle_resample(const float* reward, double* logw, float* r_prev, double lambda, double ess_frac, const double* u,
                          uint64_t seed, uint64_t counter, int32_t* anc, double* ess_out, int32_t* resampled, int n, int B, void* stream);
/* dst[(k, b), :] = src[(anc[k, b], b), :] for n x B rows of E floats, out of place (the ranges must not overlap); an ancestor outside
 * [0, n) is clamped into it.  16-byte copies where E % 4 == 0 and both bases are 16-byte aligned, 4-byte ones otherwise. */
int rgm_gather_rows(const float* src, float* dst, const int32_t* anc, int n, int B, int E, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RGM_H */
