// attention_bwd_body.h -- pieces shared by the resident (attention_bwd.hip) and the streaming (attention_bwd_stream.hip) attention backward:
// the exponential, the hi + lo operand split and its MFMA triple, the pre-split LDS row format, the rotation and the d(qkv) stores.
#pragma once
#include "common.h"

namespace rgm {

__device__ __forceinline__ float exp_le0(float x) {
  const float L2E_HI = 1.44269502162933349609375f, L2E_LO = 1.925963033500011e-8f;
  x = fmaxf(x, -104.0f);
  const float t = x * L2E_HI;
  float r = fmaf(x, L2E_HI, -t);
  r = fmaf(x, L2E_LO, r);
  const float e = __builtin_amdgcn_exp2f(t);
  return fmaf(e, r * 0.693147182464599609375f, e);
}

// ---- bf16x3 arithmetic of the backward (round 6; the bf16x3 / bf16x3_presplit modes): the same five contractions on v_mfma_f32_32x32x16_bf16,
// every operand split hi + lo when it is fetched (a*b ~= al*bh + ah*bl + ah*bh, fp32 accumulate -- the forward's and the GEMMs' arithmetic),
// with the register layouts of the fp32 kernels: 16 channels (or 16 keys / queries) per MFMA instead of 2 -- 36 (dq) / 48 (dkv) MFMAs of 32
// cycles per tile pair where the fp32 path issues 96 / 128 of 64.  The LDS images are pre-split rows (PsImg below); only the registers that
// become B operands (Q / dO resp. K / V fragments once per tile, P and dS per tile pair) are split by the wave that holds them.
typedef split_t bsplit8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ void bwd_split8(const float* v, bsplit8& hi, bsplit8& lo) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    hi[i] = (split_t)v[i];
    lo[i] = (split_t)(v[i] - (float)hi[i]);
  }
}
#ifdef RGM_SPLIT_F16
#define RGM_BWD_MFMA __builtin_amdgcn_mfma_f32_32x32x16_f16
#else
#define RGM_BWD_MFMA __builtin_amdgcn_mfma_f32_32x32x16_bf16
#endif
// acc += A . B with both operands split: term order al*bh, ah*bl, ah*bh (as everywhere)
__device__ __forceinline__ void mfma_x3(f32x16& acc, const bsplit8& ah, const bsplit8& al, const bsplit8& bh, const bsplit8& bl) {
  acc = RGM_BWD_MFMA(al, bh, acc, 0, 0, 0);
  acc = RGM_BWD_MFMA(ah, bl, acc, 0, 0, 0);
  acc = RGM_BWD_MFMA(ah, bh, acc, 0, 0, 0);
}
// ---- LDS images of the x3 kernels: a row keeps its (HD + 4) * 4 bytes but holds [HD hi halves | HD lo halves | 16 bytes of pad] -- split ONCE
// by the thread that stages the element (the on-the-fly split of round 6's first version was repeated by each of the eight waves for the tile
// it read: the kernels were VALU-bound).  Row stride in 16-byte slots: 17 (hd 64) / 19 (hd 72), odd -> conflict-free ds_read_b128 groups.
template <int HD>
struct PsImg {
  static constexpr int RS = (HD + 4) * 4;                    // bytes per row (the fp32 image's HDP floats)
  static __device__ __forceinline__ void st4(float* img, int row, int d0, const float4& v) {
    typedef split_t h4 __attribute__((ext_vector_type(4)));
    h4 hi, lo;
    hi[0] = (split_t)v.x; hi[1] = (split_t)v.y; hi[2] = (split_t)v.z; hi[3] = (split_t)v.w;
    lo[0] = (split_t)(v.x - (float)hi[0]); lo[1] = (split_t)(v.y - (float)hi[1]);
    lo[2] = (split_t)(v.z - (float)hi[2]); lo[3] = (split_t)(v.w - (float)hi[3]);
    char* rp = reinterpret_cast<char*>(img) + row * RS + 2 * d0;
    *reinterpret_cast<h4*>(rp) = hi;
    *reinterpret_cast<h4*>(rp + 2 * HD) = lo;
  }
  // channels d0 .. d0 + 7 of `row` (d0 a multiple of 8) as the split fragment; zero = the chunk lies beyond the row's channels
  static __device__ __forceinline__ void row8(const float* img, int row, int d0, bool zero, bsplit8& hi, bsplit8& lo) {
    const char* rp = reinterpret_cast<const char*>(img) + row * RS + 2 * d0;
    hi = *reinterpret_cast<const bsplit8*>(rp);
    lo = *reinterpret_cast<const bsplit8*>(rp + 2 * HD);
    if (zero) {
#pragma unroll
      for (int i = 0; i < 8; ++i) { hi[i] = (split_t)0.f; lo[i] = (split_t)0.f; }
    }
  }
  // the transposed fragment: channel `col` of the 8 rows a lane's C/D registers 8 h2 .. 8 h2 + 7 stand for -- row (j & 3) + 8 (2 h2 + (j >> 2))
  // + 4 hh of the 32-row tile starting at row `r0`: slot j of the B operand built from those registers meets slot j here
  static __device__ __forceinline__ void col8(const float* img, int r0, int col, int h2, int hh, bsplit8& hi, bsplit8& lo) {
    const char* cp = reinterpret_cast<const char*>(img) + (long long)r0 * RS + 2 * col;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const char* ep = cp + ((j & 3) + 8 * (2 * h2 + (j >> 2)) + 4 * hh) * RS;
      hi[j] = *reinterpret_cast<const split_t*>(ep);
      lo[j] = *reinterpret_cast<const split_t*>(ep + 2 * HD);
    }
  }
  // the element / four elements as floats again (hi + lo: 2^-17 of the fp32 value; the lone-token paths' plain sums)
  static __device__ __forceinline__ float ld1(const float* img, int row, int d) {
    const char* ep = reinterpret_cast<const char*>(img) + row * RS + 2 * d;
    return (float)*reinterpret_cast<const split_t*>(ep) + (float)*reinterpret_cast<const split_t*>(ep + 2 * HD);
  }
  static __device__ __forceinline__ float4 ld4(const float* img, int row, int d0) {
    typedef split_t h4 __attribute__((ext_vector_type(4)));
    const char* rp = reinterpret_cast<const char*>(img) + row * RS + 2 * d0;
    const h4 hi = *reinterpret_cast<const h4*>(rp), lo = *reinterpret_cast<const h4*>(rp + 2 * HD);
    return make_float4((float)hi[0] + (float)lo[0], (float)hi[1] + (float)lo[1], (float)hi[2] + (float)lo[2], (float)hi[3] + (float)lo[3]);
  }
};
// one accessor for both image formats (X3: pre-split rows; else fp32 rows of HDP floats)
template <int HD, bool X3>
__device__ __forceinline__ float4 img_ld4(const float* img, int row, int d0) {
  if constexpr (X3) return PsImg<HD>::ld4(img, row, d0);
  else return *reinterpret_cast<const float4*>(img + row * (HD + 4) + d0);
}
template <int HD, bool X3>
__device__ __forceinline__ float img_ld1(const float* img, int row, int d) {
  if constexpr (X3) return PsImg<HD>::ld1(img, row, d);
  else return img[row * (HD + 4) + d];
}

__device__ __forceinline__ float4 rotate4(float4 v, const float* __restrict__ ct, const float* __restrict__ st, int pi, bool inverse) {
  const float c0 = ct[pi], c1 = ct[pi + 1];
  float s0 = st[pi], s1 = st[pi + 1];
  if (inverse) { s0 = -s0; s1 = -s1; }
  return make_float4(v.x * c0 - v.y * s0, v.y * c0 + v.x * s0, v.z * c1 - v.w * s1, v.w * c1 + v.z * s1);
}

// d(qkv) rows go out as fp32 or -- for a pre-split dgrad GEMM right behind (dit.hip grad chain) -- as split rows (common.h split_idx);
// col = column of the value's first channel inside the 3 D wide row, a multiple of 4 (the four channels share a 32-block)
__device__ __forceinline__ void dqkv_store4(float* __restrict__ dqkv, long long row, int D3, int col, const float4& v, int osplit) {
  if (osplit) {
    typedef split_t bf16x4 __attribute__((ext_vector_type(4)));
    bf16x4 hi, lo;
    hi[0] = (split_t)v.x; hi[1] = (split_t)v.y; hi[2] = (split_t)v.z; hi[3] = (split_t)v.w;
    lo[0] = (split_t)(v.x - (float)hi[0]); lo[1] = (split_t)(v.y - (float)hi[1]);
    lo[2] = (split_t)(v.z - (float)hi[2]); lo[3] = (split_t)(v.w - (float)hi[3]);
    split_t* rp = reinterpret_cast<split_t*>(dqkv + row * D3);
    *reinterpret_cast<bf16x4*>(rp + split_idx(col)) = hi;
    *reinterpret_cast<bf16x4*>(rp + split_idx(col) + 32) = lo;
  } else {
    *reinterpret_cast<float4*>(dqkv + row * D3 + col) = v;
  }
}
__device__ __forceinline__ void dqkv_store1(float* __restrict__ dqkv, long long row, int D3, int col, float v, int osplit) {
  if (osplit) {
    split_t* rp = reinterpret_cast<split_t*>(dqkv + row * D3);
    const split_t hi = (split_t)v;
    rp[split_idx(col)] = hi;
    rp[split_idx(col) + 32] = (split_t)(v - (float)hi);
  } else {
    dqkv[row * D3 + col] = v;
  }
}

}  // namespace rgm
