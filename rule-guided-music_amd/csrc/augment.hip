// Augmented training batches built on the device: time stretch, key shift, latent windows, noised latents and the latent scale
// (docs/rounds/augment.md).
//
// The definition is the reference's data path: ImageDataset.__getitem__ and key_shift (guided_diffusion/pr_datasets_all.py), get_kl_input
// (guided_diffusion/train_util.py), q_sample and compute_std.py.  The host partner guided_diffusion/pr_datasets_all.augment_excerpt restates
// __getitem__ in closed form and is pinned to it bit for bit; the kernels are compared with the host partner.
//
//   rgm_roll_augment     one launch, one workgroup per (output row, output pitch): uint8 excerpts in a blob -> the float32 batch (B, 3, 128, S).
//     scale      x = float(u8) / 63.5f - 1, a true division: the 256 possible values are divided once per workgroup into an LDS table;
//     window     columns [start, start + pr_len) with the stretch flag, [0, S) without it: the three source rows of the workgroup (velocity
//                and onset at pitch (p + |k|) & 127, pedal at pitch p) are staged in LDS with aligned 16-byte loads;
//     stretch    pr_len < S: velocity and pedal by torch's `nearest` map src(j) = min(int(floorf(j * (float(pr_len) / float(S)))), pr_len - 1);
//                onsets by a(j) = int((float(j) / float(S)) * float(pr_len)): a column whose a differs from its left neighbour's (and column
//                0) takes source onset column rank(j) = the number of such columns before it, every other column is -1.  The ranks come from
//                a scan: firsts per group of 4 columns, an exclusive prefix over the groups in LDS;
//     compress   pr_len > S: all three by src(j), then onset = 1 where the resampled velocity exceeds its left neighbour (column 0 never);
//     key shift  new[p] = old[(p + |k|) mod 128] for velocity and onset -- the reference shifts k < 0 the same way as k > 0;
//     piano_like pitches < 21 and > 108 are -1 in all three channels: those workgroups write without reading.
//     Every thread writes 4 consecutive columns with one 16-byte store (S % 4 == 0; 4-byte stores otherwise).  A refused row is -1 throughout.
//   rgm_latent_windows   VAE moments of the S/128 tiles (tile-major) -> the posterior mode re-assembled along time, cut into windows of 128
//                latent rows, times scale_factor, and optionally x_t = sqrt_ac[t] z + sqrt_1mac[t] noise in the same launch.
//   rgm_latent_std       mean, unbiased standard deviation and its reciprocal of n float32 values, in float64.
//
// Floating point: IEEE, no contraction (the index maps are float32 products and quotients whose truncation decides a column).  No atomics:
// every output element has one owner, every sum one order that depends on n alone.  Launches repeat bit for bit, and a row's result depends
// neither on B nor on its position.  The blob is only read.  All stores are ordinary vector stores.
#include "philox.h"
#include "roll_bits.h"

#pragma clang fp contract(off)

namespace rgm {
namespace augment {
using rollbits::MAX_PIANO;
using rollbits::MIN_PIANO;

constexpr int THREADS = 256;
constexpr int MAX_S = 16384;
constexpr int MAX_B = 1 << 23;                            // 128 workgroups per row in a one-dimensional grid
constexpr int ST_OK = 0, ST_FILE = 1, ST_WINDOW = 2, ST_LENGTH = 3, ST_SHIFT = 4;
constexpr int FLAG_STRETCH = 1, FLAG_SHIFT = 2;
constexpr int LUT_BYTES = 1024, SCAN_BYTES = 1024;

// source columns a row may ask for: 1.0625 S rounded up to 16, plus 16 (int(1.05 S) fits for every S)
__host__ __device__ inline int capacity(int S) { return ((S + S / 16 + 15) & ~15) + 16; }
__host__ __device__ inline int groups(int S) { return (S + 3) >> 2; }
__host__ __device__ inline int pre_bytes(int S) { return (2 * groups(S) + 15) & ~15; }
__host__ __device__ inline int row_bytes(int S) { return capacity(S) + 32; }   // up to 15 bytes in front of an unaligned row, the last load whole
__host__ __device__ inline size_t lds_bytes(int S) { return (size_t)LUT_BYTES + SCAN_BYTES + pre_bytes(S) + 3 * (size_t)row_bytes(S); }

__device__ __forceinline__ int onset_map(int j, float fS, float fL) { return (int)(((float)j / fS) * fL); }
__device__ __forceinline__ bool is_first(int j, float fS, float fL) { return j == 0 || onset_map(j, fS, fL) != onset_map(j - 1, fS, fL); }
__device__ __forceinline__ int nearest(int j, float scale, int L) { return min((int)floorf((float)j * scale), L - 1); }

__device__ __forceinline__ void put4(float* __restrict__ row, int g, int S, bool vec, float a, float b, float c, float d) {
  if (vec) {
    *reinterpret_cast<float4*>(row + 4 * g) = make_float4(a, b, c, d);
  } else {
    const int j = 4 * g;
    if (j < S) row[j] = a;
    if (j + 1 < S) row[j + 1] = b;
    if (j + 2 < S) row[j + 2] = c;
    if (j + 3 < S) row[j + 3] = d;
  }
}

// grid: 128 B workgroups, workgroup x = row (x >> 7), output pitch (x & 127).  params: (B, 5) int32 rows (file, start, pr_len, k, flags).
__global__ void __launch_bounds__(THREADS)
roll_augment_kernel(const uint8_t* __restrict__ blob, const int64_t* __restrict__ offsets, const int32_t* __restrict__ lengths,
                    const int32_t* __restrict__ params, int N, long long blob_bytes, int S, int vec_i, float* __restrict__ out,
                    int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int b = blockIdx.x >> 7, p = blockIdx.x & 127, tid = threadIdx.x;
  const bool vec = vec_i != 0;
  const int cap = capacity(S), G = groups(S), rb = row_bytes(S);
  float* lut = reinterpret_cast<float*>(smem);
  int* scan = reinterpret_cast<int*>(smem + LUT_BYTES);
  uint16_t* pre = reinterpret_cast<uint16_t*>(smem + LUT_BYTES + SCAN_BYTES);
  uint8_t* stage = smem + LUT_BYTES + SCAN_BYTES + pre_bytes(S);

  const int32_t* pr = params + 5 * (size_t)b;
  const int f = pr[0], start = pr[1], pr_len = pr[2], k = pr[3], flags = pr[4];
  const bool stretch = (flags & FLAG_STRETCH) != 0, shift = (flags & FLAG_SHIFT) != 0;
  const int L = stretch ? pr_len : S;
  const long long w0 = stretch ? (long long)start : 0ll;
  int st = ST_OK;
  long long off = 0;
  int T = 0;
  if (f < 0 || f >= N) {
    st = ST_FILE;
  } else {
    off = offsets[f];
    T = lengths[f];
    if (T < 1 || off < 0 || off > blob_bytes || 384ll * T > blob_bytes - off) st = ST_FILE;      // the file's own extent leaves the blob
  }
  if (!st && stretch && (pr_len < 1 || pr_len > cap)) st = ST_LENGTH;
  if (!st && !stretch && S > cap) st = ST_LENGTH;
  if (!st && (w0 < 0 || w0 + L > T)) st = ST_WINDOW;
  if (!st && shift && (k < -127 || k > 127)) st = ST_SHIFT;
  if (p == 0 && tid == 0) status[b] = st;

  float* row0 = out + (((size_t)b * 3 + 0) * 128 + p) * (size_t)S;
  float* row1 = out + (((size_t)b * 3 + 1) * 128 + p) * (size_t)S;
  float* row2 = out + (((size_t)b * 3 + 2) * 128 + p) * (size_t)S;
  if (st || p < MIN_PIANO || p > MAX_PIANO) {              // refused, or outside the piano: -1 without reading
    for (int g = tid; g < G; g += THREADS) {
      put4(row0, g, S, vec, -1.f, -1.f, -1.f, -1.f);
      put4(row1, g, S, vec, -1.f, -1.f, -1.f, -1.f);
      put4(row2, g, S, vec, -1.f, -1.f, -1.f, -1.f);
    }
    return;
  }

  const int ak = shift ? (k < 0 ? -k : k) : 0;
  const int q = (p + ak) & 127;
  int lead[3];
  {
    const long long src[3] = {off + (long long)q * T + w0, off + (128ll + q) * T + w0, off + (256ll + p) * T + w0};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const long long a0 = src[c] & ~15ll;
      lead[c] = (int)(src[c] - a0);
      const int nvec = (lead[c] + L + 15) >> 4;           // 16 nvec <= cap + 16 < row_bytes
      uint4* dst = reinterpret_cast<uint4*>(stage + c * rb);
      for (int i = tid; i < nvec; i += THREADS) {
        const long long pa = a0 + 16ll * i;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (pa + 16 <= blob_bytes) v = *reinterpret_cast<const uint4*>(blob + pa);
        dst[i] = v;
      }
    }
  }
  lut[tid] = (float)tid / 63.5f - 1.0f;
  const uint8_t* s0 = stage + lead[0];
  const uint8_t* s1 = stage + rb + lead[1];
  const uint8_t* s2 = stage + 2 * rb + lead[2];
  const float fS = (float)S, fL = (float)L;
  const float scale = fL / fS;

  if (L < S) {
    // firsts per group of 4 columns, then their exclusive prefix: every thread sums a run of consecutive groups, the 256 sums are scanned
    for (int g = tid; g < G; g += THREADS) {
      int n = 0;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int j = 4 * g + jj;
        n += (j < S && is_first(j, fS, fL)) ? 1 : 0;
      }
      pre[g] = (uint16_t)n;
    }
    __syncthreads();
    const int per = (G + THREADS - 1) / THREADS;
    const int g0 = min(tid * per, G), g1 = min(g0 + per, G);
    int sum = 0;
    for (int g = g0; g < g1; ++g) sum += pre[g];
    scan[tid] = sum;
    __syncthreads();
    for (int d = 1; d < THREADS; d <<= 1) {
      const int v = tid >= d ? scan[tid - d] : 0;
      __syncthreads();
      scan[tid] += v;
      __syncthreads();
    }
    int run = scan[tid] - sum;
    for (int g = g0; g < g1; ++g) {
      const int n = pre[g];
      pre[g] = (uint16_t)run;
      run += n;
    }
  }
  __syncthreads();

  for (int g = tid; g < G; g += THREADS) {
    float v0[4], v1[4], v2[4];
    int rank = L < S ? (int)pre[g] : 0;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int j = 4 * g + jj;
      v0[jj] = v1[jj] = v2[jj] = -1.f;
      if (j >= S) continue;
      if (L < S) {
        const int s = nearest(j, scale, L);
        v0[jj] = lut[s0[s]];
        v2[jj] = lut[s2[s]];
        if (is_first(j, fS, fL)) {
          v1[jj] = lut[s1[min(rank, L - 1)]];
          ++rank;
        }
      } else if (L > S) {
        const int s = nearest(j, scale, L);
        v0[jj] = lut[s0[s]];
        v1[jj] = lut[s1[s]];
        v2[jj] = lut[s2[s]];
        if (j > 0 && v0[jj] > lut[s0[nearest(j - 1, scale, L)]]) v1[jj] = 1.0f;
      } else {
        v0[jj] = lut[s0[j]];
        v1[jj] = lut[s1[j]];
        v2[jj] = lut[s2[j]];
      }
    }
    put4(row0, g, S, vec, v0[0], v0[1], v0[2], v0[3]);
    put4(row1, g, S, vec, v1[0], v1[1], v1[2], v1[3]);
    put4(row2, g, S, vec, v2[0], v2[1], v2[2], v2[3]);
  }
}

// ---- latent windows and noised latents -----------------------------------------------------------------------------------------------------
// the 4 normals of Philox block `ctr`: Box-Muller on (0,1] x [0,1) -- the arithmetic of rgm_randn (sampler.hip), operation for operation
__device__ __forceinline__ void normals4(uint64_t ctr, uint64_t seed, float (&z)[4]) {
  uint32_t r[4];
  philox4x32_10(ctr, seed, r);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float u1 = ((float)(r[2 * h] >> 8) + 1.0f) * (1.0f / 16777216.0f);
    const float u2 = (float)(r[2 * h + 1] >> 8) * (1.0f / 16777216.0f);
    const float rad = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincosf(6.283185307179586f * u2, &sn, &cs);
    z[2 * h] = rad * cs;
    z[2 * h + 1] = rad * sn;
  }
}

// one thread per 4 consecutive elements of z0 (rows, 4, R, 16): out[b W + w, c, r, i] = scale * mean[s B + b, c, i, j], 16 s + j = step w + r
__global__ void __launch_bounds__(THREADS)
latent_windows_kernel(const float* __restrict__ moments, int B, int W, int R, int step, float scale_factor, float* __restrict__ z0,
                      const int64_t* __restrict__ t, const float* __restrict__ sqrt_ac, const float* __restrict__ sqrt_1mac, int num_timesteps,
                      const float* __restrict__ noise, uint64_t seed, uint64_t offset, float* __restrict__ x_t, long long quads) {
  const long long qd = blockIdx.x * (long long)THREADS + threadIdx.x;
  if (qd >= quads) return;
  const long long e = qd * 4;
  const int i = (int)(e & 15);
  const long long rr = e >> 4;
  const int r = (int)(rr % R);
  const long long cc = rr / R;
  const int c = (int)(cc & 3);
  const long long row = cc >> 2;
  const int w = (int)(row % W), b = (int)(row / W);
  const int lat = step * w + r, s = lat >> 4, j = lat & 15;
  const float* m = moments + (((size_t)s * B + b) * 8 + c) * 256 + (size_t)i * 16 + j;
  float z[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) z[u] = m[16 * u] * scale_factor;
  *reinterpret_cast<float4*>(z0 + e) = make_float4(z[0], z[1], z[2], z[3]);
  if (!x_t) return;
  long long ti = t[row];
  ti = ti < 0 ? 0 : (ti >= num_timesteps ? num_timesteps - 1 : ti);          // a step outside the schedule is clamped: no read leaves the tables
  const float a = sqrt_ac[ti], sd = sqrt_1mac[ti];
  float n[4];
  if (noise) {
    const float4 v = *reinterpret_cast<const float4*>(noise + e);
    n[0] = v.x; n[1] = v.y; n[2] = v.z; n[3] = v.w;
  } else {
    const uint64_t pos = offset + (uint64_t)e;
    const int lane = (int)(pos & 3);
    float za[4], zb[4] = {0.f, 0.f, 0.f, 0.f};
    normals4(pos >> 2, seed, za);
    if (lane) normals4((pos >> 2) + 1, seed, zb);
#pragma unroll
    for (int u = 0; u < 4; ++u) {                         // element u is normal lane + u of the two blocks: static indices only
      const float c0 = za[u], c1 = u + 1 < 4 ? za[(u + 1) & 3] : zb[(u + 1) & 3], c2 = u + 2 < 4 ? za[(u + 2) & 3] : zb[(u + 2) & 3],
                  c3 = u + 3 < 4 ? za[(u + 3) & 3] : zb[(u + 3) & 3];
      n[u] = lane == 0 ? c0 : (lane == 1 ? c1 : (lane == 2 ? c2 : c3));
    }
  }
  float o[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const float p0 = a * z[u], p1 = sd * n[u];
    o[u] = p0 + p1;
  }
  *reinterpret_cast<float4*>(x_t + e) = make_float4(o[0], o[1], o[2], o[3]);
}

// ---- latent scale ------------------------------------------------------------------------------------------------------------------------------
constexpr int STD_CHUNK = 2048;                           // elements per workgroup: a function of nothing but the build

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// workgroup `chunk` sums its 2048 elements: every thread its 8 in index order, a wave64 xor tree, the 4 waves in wave order
__global__ void __launch_bounds__(THREADS) std_partial_kernel(const float* __restrict__ x, long long n, double* __restrict__ partials) {
  __shared__ double red[THREADS / 64][2];
  const long long base = (long long)blockIdx.x * STD_CHUNK;
  double s = 0.0, ss = 0.0;
#pragma unroll
  for (int h = 0; h < STD_CHUNK / (4 * THREADS); ++h) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long e = base + (h * THREADS + (int)threadIdx.x) * 4 + u;
      if (e < n) {
        const double v = (double)x[e];
        s += v;
        ss += v * v;
      }
    }
  }
  s = wave_sum(s);
  ss = wave_sum(ss);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) { red[wave][0] = s; red[wave][1] = ss; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = red[0][0], c = red[0][1];
    for (int w = 1; w < THREADS / 64; ++w) { a += red[w][0]; c += red[w][1]; }
    partials[2 * (long long)blockIdx.x] = a;
    partials[2 * (long long)blockIdx.x + 1] = c;
  }
}

// one wave: lane l adds chunks l, l + 64, ... in order, then the same tree.  out: mean, unbiased std, 1 / std
__global__ void __launch_bounds__(64) std_final_kernel(const double* __restrict__ partials, long long chunks, long long n, double* __restrict__ out) {
  double s = 0.0, ss = 0.0;
  for (long long c = threadIdx.x; c < chunks; c += 64) {
    s += partials[2 * c];
    ss += partials[2 * c + 1];
  }
  s = wave_sum(s);
  ss = wave_sum(ss);
  if (threadIdx.x == 0) {
    const double dn = (double)n, mean = s / dn;
    const double m2 = ss - s * mean;                      // sum (x - mean)^2
    const double var = n > 1 ? fmax(m2, 0.0) / (dn - 1.0) : __longlong_as_double(0x7ff8000000000000ll);
    const double sd = sqrt(var);
    out[0] = mean;
    out[1] = sd;
    out[2] = 1.0 / sd;
  }
}
}  // namespace augment
}  // namespace rgm

using namespace rgm;

extern "C" int rgm_roll_augment_capacity(int S) { return S >= 1 && S <= augment::MAX_S ? augment::capacity(S) : 0; }

extern "C" int rgm_roll_augment(const uint8_t* blob, long long blob_bytes, const int64_t* offsets, const int32_t* lengths, int N,
                                const int32_t* params, int B, int S, float* out, int32_t* status, void* stream) {
  RGM_REQUIRE(blob && offsets && lengths && params && out && status, "roll_augment: bad arguments");
  RGM_REQUIRE(N >= 1 && N <= (1 << 24), "roll_augment: N = %d excerpts (1 .. 2^24)", N);
  RGM_REQUIRE(B >= 1 && B <= augment::MAX_B, "roll_augment: B = %d rows (1 .. 2^23 per launch)", B);
  RGM_REQUIRE(S >= 1 && S <= augment::MAX_S, "roll_augment: S = %d columns (1 .. %d)", S, augment::MAX_S);
  RGM_REQUIRE(blob_bytes >= 16 && blob_bytes % 16 == 0, "roll_augment: a blob of %lld bytes (a positive multiple of 16: the allocation is padded)",
              blob_bytes);
  RGM_REQUIRE(((uintptr_t)blob & 15) == 0, "roll_augment: the blob must be 16-byte aligned");
  RGM_REQUIRE(((uintptr_t)out & 3) == 0 && ((uintptr_t)status & 3) == 0 && ((uintptr_t)params & 3) == 0 && ((uintptr_t)lengths & 3) == 0 &&
                  ((uintptr_t)offsets & 7) == 0, "roll_augment: misaligned array");
  const size_t lds = augment::lds_bytes(S);
  RGM_REQUIRE(lds <= 65536, "roll_augment: S = %d needs %zu bytes of LDS", S, lds);
  const int vec = S % 4 == 0 && ((uintptr_t)out & 15) == 0;
  hipLaunchKernelGGL(augment::roll_augment_kernel, dim3((unsigned)B * 128u), dim3(augment::THREADS), lds, (hipStream_t)stream, blob, offsets,
                     lengths, params, N, blob_bytes, S, vec, out, status);
  RGM_LAUNCH_CHECK();
  return RGM_OK;
}

extern "C" int rgm_latent_windows_count(int n_tiles, int shift_size) {
  if (n_tiles < 1 || n_tiles > 4096 || shift_size < 0 || shift_size > 4096) return 0;
  if (shift_size == 0) return 1;
  if (n_tiles < 8) return 0;
  return (16 * n_tiles - 128) / (16 * shift_size) + 1;
}

extern "C" int rgm_latent_windows(const float* moments, int B, int n_tiles, int shift_size, float scale_factor, float* z0, const int64_t* t,
                                  const float* sqrt_ac, const float* sqrt_1mac, int num_timesteps, const float* noise, uint64_t seed,
                                  uint64_t offset, float* x_t, void* stream) {
  RGM_REQUIRE(moments && z0, "latent_windows: bad arguments");
  RGM_REQUIRE(B >= 1 && B <= (1 << 20), "latent_windows: B = %d (1 .. 2^20)", B);
  RGM_REQUIRE(n_tiles >= 1 && n_tiles <= 4096, "latent_windows: %d tiles (1 .. 4096)", n_tiles);
  const int W = rgm_latent_windows_count(n_tiles, shift_size);
  RGM_REQUIRE(W >= 1, "latent_windows: shift_size = %d with %d tiles (0, or 1 .. 4096 with at least 8 tiles: a window is 128 latent rows)",
              shift_size, n_tiles);
  RGM_REQUIRE(!x_t || (t && sqrt_ac && sqrt_1mac && num_timesteps >= 1), "latent_windows: x_t needs t and the two schedule tables");
  RGM_REQUIRE(((uintptr_t)moments & 3) == 0 && ((uintptr_t)z0 & 15) == 0 && ((uintptr_t)x_t & 15) == 0 && ((uintptr_t)noise & 15) == 0 &&
                  ((uintptr_t)t & 7) == 0, "latent_windows: z0, x_t and the noise must be 16-byte aligned");
  const int R = shift_size ? 128 : 16 * n_tiles;
  const long long quads = (long long)B * W * 4 * R * 4;
  RGM_REQUIRE(quads <= (1ll << 38), "latent_windows: %lld output elements", quads * 4);
  hipLaunchKernelGGL(augment::latent_windows_kernel, dim3((unsigned)((quads + augment::THREADS - 1) / augment::THREADS)), dim3(augment::THREADS),
                     0, (hipStream_t)stream, moments, B, W, R, 16 * shift_size, scale_factor, z0, t, sqrt_ac, sqrt_1mac, num_timesteps, noise, seed,
                     offset, x_t, quads);
  RGM_LAUNCH_CHECK();
  return RGM_OK;
}

extern "C" size_t rgm_latent_std_workspace(long long n) {
  if (n < 1 || n > (1ll << 40)) return 0;
  return (size_t)((n + augment::STD_CHUNK - 1) / augment::STD_CHUNK) * 16;
}

extern "C" int rgm_latent_std(const float* x, long long n, double* out, void* ws, size_t ws_bytes, void* stream) {
  RGM_REQUIRE(x && out, "latent_std: bad arguments");
  RGM_REQUIRE(n >= 1 && n <= (1ll << 40), "latent_std: n = %lld (1 .. 2^40)", n);
  const size_t need = rgm_latent_std_workspace(n);
  if (!ws || ws_bytes < need) {
    set_error("latent_std: workspace of %zu bytes, %zu needed", ws ? ws_bytes : (size_t)0, need);
    return RGM_ERR_WORKSPACE;
  }
  RGM_REQUIRE(((uintptr_t)ws & 7) == 0 && ((uintptr_t)out & 7) == 0 && ((uintptr_t)x & 3) == 0, "latent_std: misaligned array");
  const long long chunks = (n + augment::STD_CHUNK - 1) / augment::STD_CHUNK;
  hipLaunchKernelGGL(augment::std_partial_kernel, dim3((unsigned)chunks), dim3(augment::THREADS), 0, (hipStream_t)stream, x, n, (double*)ws);
  RGM_LAUNCH_CHECK();
  hipLaunchKernelGGL(augment::std_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)ws, chunks, n, out);
  RGM_LAUNCH_CHECK();
  return RGM_OK;
}
