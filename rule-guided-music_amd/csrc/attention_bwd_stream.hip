// attention_bwd_stream.hip -- the attention backward of attention_bwd.hip for sequences too long to keep a head's K / V (resp. Q / dO) in
// LDS: hd 72 at T > 256, hd 64 at T > 288, up to ATTN_STREAM_MAX_T tokens.  Classifier guidance, DPS and guided editing of long excerpts
// (the reference's autograd through guided_diffusion/dit.py:263-277 does not depend on the length).
//
// Same maths as the resident pair (header of attention_bwd.hip), same two-kernel shape, so every output element is owned by exactly one
// wave -- no atomics, deterministic -- and no T x T matrix exists anywhere:
//   * dq kernel : a workgroup owns 256 queries of one (sample, head), 32 per wave; Q (rotated, scaled), dO, lse and D = rowsum(dO * O) of
//                 its queries live in registers; K (rotated) and V stream through two LDS buffers in blocks of 64 keys;
//   * dkv kernel: a workgroup owns 256 keys; their K (rotated) and V fragments live in registers; Q (rotated, pre-scaled), dO, lse and D
//                 stream through two LDS buffers in blocks of 64 queries; dK / dV accumulate over the whole query range, written once.
// D is computed inside both kernels: the dq kernel sums its own queries' dO * O in the prologue (as the resident kernel does); the dkv
// kernel sums a query's row while staging it (the eight threads that stage a row hold its dO chunks and load the matching O chunks; three
// shuffles in a fixed order).  No pre-pass, no workspace.
// The per-tile products are those of the resident kernels (transposed scores, P^T / dS^T stay in the register file as B operands; LDS rows
// in the fp32 or the PsImg pre-split format), in both arithmetics: X3 = 0 exact fp32 on v_mfma_f32_32x32x2_f32, X3 = 1 hi + lo split
// operands on v_mfma_f32_32x32x16_bf16 (term order al*bh, ah*bl, ah*bh).
// Streaming follows the forward (header of attention_stream.hip).  dq kernel: block b + 2 is requested into registers before block b + 1's
// products and written to LDS after them.  dkv kernel: the K / V fragments and the dK / dV accumulators (168 .. 176 registers at hd 72) leave
// no room for a block held in registers THROUGH the products (tried: 302 .. 375 spilled registers), so block b + 1 is loaded and written to
// the other buffer in front of block b's products, in two passes (Q, then dO with O) -- its load latency is exposed twice per block.  Both: one barrier per block; retire_loads() before any staged register is read, lds_written() before the next
// block's loads issue; one workgroup per CU; EVERY wave runs EVERY block -- a wave without queries / keys (partial last tile) works on the
// clamped row and stores nothing.
#include <stdlib.h>
#include "common.h"
#include "attention_bwd_body.h"

namespace rgm {

namespace {
// every outstanding load retired, then 32 idle cycles before the first read of a destination register (attention_stream.hip)
__device__ __forceinline__ void retire_loads() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_waitcnt vmcnt(0)\n\ts_nop 7\n\ts_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}
// the block's LDS writes done before the next block's loads are issued
__device__ __forceinline__ void lds_written() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}
constexpr int BOWN = 256;   // queries (dq) / keys (dkv) per workgroup: 8 waves x 32
constexpr int BSTR = 64;    // rows per streamed block: thread (row = tid / 8, sub = tid % 8) stages the float4 chunks sub, sub + 8, sub + 16
int g_bwd_stream_force = 0;
long long g_bwd_stream_launches = 0;

__device__ __forceinline__ float4 rot_fwd(const float4& x, const float4& f) {   // f = (c0, s0, c1, s1); (1, 0, 1, 0) outside the rotary channels
  return make_float4(x.x * f.x - x.y * f.y, x.y * f.x + x.x * f.y, x.z * f.z - x.w * f.w, x.w * f.z + x.z * f.w);
}
__device__ __forceinline__ float4 rot_inv(const float4& x, const float4& f) {   // the inverse rotation (rotate4 with the sines negated)
  return make_float4(x.x * f.x + x.y * f.y, x.y * f.x - x.x * f.y, x.z * f.z + x.w * f.w, x.w * f.z - x.z * f.w);
}
// rotary factors of the epilogue's un-rotation for the channels this lane stores (tile dt, group g: channels dt*32 + 8g + 4hh ..+3) of
// token `row`: all requested, then ONE wait (retire_loads) in front of the first use.  With the factors loaded where they are used
// (rotate4, a global_load_dwordx2 used right behind its counted wait) the hd 64 bf16x3 dkv instance returned, in a few workgroups per
// launch, dK rows whose third channel of a group was wrong by ~0.1 in lanes 48-63 -- the signature of DESIGN 4h.
template <int HD, int DT>
__device__ __forceinline__ void epilogue_factors(float4 (&fac)[DT * 4], const float* __restrict__ cos_tab, const float* __restrict__ sin_tab,
                                                 int row, int rot_half, int hh) {
#pragma unroll
  for (int i = 0; i < DT * 4; ++i) {
    const int d = (i >> 2) * 32 + 8 * (i & 3) + 4 * hh;
    fac[i] = make_float4(1.f, 0.f, 1.f, 0.f);
    if (d < HD && d < 2 * rot_half) {
      const unsigned pi = (unsigned)(row * rot_half + (d >> 1));
      const float2 cc = ldg8(cos_tab + pi), ss = ldg8(sin_tab + pi);
      fac[i] = make_float4(cc.x, ss.x, cc.y, ss.y);
    }
  }
  retire_loads();
}
}  // namespace

template <int HD>
struct BwdStreamGeom {
  static constexpr int HDP = HD + 4;
  static constexpr int IMG = BSTR * HDP;                               // floats per 64-row image (fp32 rows or PsImg rows: the same bytes)
  static constexpr size_t BYTES = (size_t)(4 * IMG + 4 * BSTR) * 4;    // two buffers x two images, then lse / D of both buffers (dkv)
};

// ------------------------------------------------------------------------------------------- dQ
template <int HD, bool X3>
__global__ __launch_bounds__(512) void attn_bwd_stream_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ o,
                                                                 const float* __restrict__ d_o, const float* __restrict__ lse,
                                                                 float* __restrict__ dqkv, const float* __restrict__ cos_tab,
                                                                 const float* __restrict__ sin_tab, int T, int heads, int rot_half, int osplit,
                                                                 int qblocks) {
  constexpr int HDP = HD + 4, KB = HD / 8, DT = (HD + 31) / 32, KS = (HD + 15) / 16, CPR = HD / 4, NIT = (CPR + 7) / 8;
  constexpr int IMG = BwdStreamGeom<HD>::IMG;
  // (hd = 72, fp32: the third channel tile's operand reads run past a K row into the next row / the V image: finite or never-stored rows)
  extern __shared__ __attribute__((aligned(16))) float smem[];   // [buffer][K image | V image]
  const int pair = blockIdx.x / qblocks, qb = blockIdx.x - pair * qblocks;
  const int n = pair / heads, head = pair - n * heads;
  const int D = heads * HD, D3 = 3 * D, R = 2 * rot_half;
  const float* base = qkv + (long long)n * T * D3 + head * HD;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hh = lane >> 5;
  const int srow = tid >> 3, sub = tid & 7;
  const int nb = (T + BSTR - 1) / BSTR;
  const float scale = rsqrtf((float)HD);

  constexpr int NRT = 2;                                      // chunks sub, sub + 8 can rotate; sub + 16 (channels >= 64) never does (launcher)
  float4 kst[NIT], vst[NIT], cst[NRT];                        // one block's K / V chunks and the K chunks' rotary factors
  auto request = [&](int b) {
    const int key = b * BSTR + srow;
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int c = sub + 8 * i, d0 = 4 * c;
      kst[i] = vst[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (i < NRT) cst[i] = make_float4(1.f, 0.f, 1.f, 0.f);
      if (c < CPR && key < T) {
        const unsigned off = (unsigned)key * (unsigned)D3 + (unsigned)d0;   // (uniform base + 32-bit lane offset: < 2^27 floats per sample)
        kst[i] = ldg16(base + D + off);
        vst[i] = ldg16(base + 2 * D + off);
        if (i < NRT && d0 < R) {
          const unsigned pi = (unsigned)(key * rot_half + (d0 >> 1));
          const float2 cc = ldg8(cos_tab + pi), ss = ldg8(sin_tab + pi);
          cst[i < NRT ? i : 0] = make_float4(cc.x, ss.x, cc.y, ss.y);
        }
      }
    }
  };
  auto deposit = [&](float* buf) {
    retire_loads();
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int c = sub + 8 * i, d0 = 4 * c;
      if (c >= CPR) continue;
      const float4 kv = i < NRT ? rot_fwd(kst[i], cst[i < NRT ? i : 0]) : kst[i];
      if constexpr (X3) {
        PsImg<HD>::st4(buf, srow, d0, kv);
        PsImg<HD>::st4(buf + IMG, srow, d0, vst[i]);
      } else {
        *reinterpret_cast<float4*>(buf + srow * HDP + d0) = kv;
        *reinterpret_cast<float4*>(buf + IMG + srow * HDP + d0) = vst[i];
      }
    }
  };

  // ---- prologue: this lane's query (clamped in the partial last tile), two phases each: loads, ONE wait, first use
  const int q = qb * BOWN + wave * 32 + l31, qc = min(q, T - 1);
  const long long orow = ((long long)n * T + qc) * D + head * HD;
  constexpr int NQ = X3 ? 2 * KS : KB;                          // float4 chunks of a row this lane holds
  // x3: lane (query l31, half hh) holds channels 16 j + 8 hh + 4 u (i = 2 j + u); fp32: 8 i + 4 hh
  auto chunk_d0 = [&](int i) { return X3 ? 16 * (i >> 1) + 8 * hh + 4 * (i & 1) : 8 * i + 4 * hh; };
  float qv[NQ][4], gv[NQ][4];
  float dsum = 0.f, lq;
  {
    float4 raw[NQ], fac[NQ];
    const float* qp = base + (long long)qc * D3;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int d0 = chunk_d0(i);
      raw[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      fac[i] = make_float4(1.f, 0.f, 1.f, 0.f);
      if (d0 < HD) {
        raw[i] = ldg16(qp + d0);
        if (d0 < R) {
          const int pi = qc * rot_half + (d0 >> 1);
          const float2 cc = ldg8(cos_tab + pi), ss = ldg8(sin_tab + pi);
          fac[i] = make_float4(cc.x, ss.x, cc.y, ss.y);
        }
      }
    }
    retire_loads();
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const float4 v = rot_fwd(raw[i], fac[i]);
      qv[i][0] = v.x * scale; qv[i][1] = v.y * scale; qv[i][2] = v.z * scale; qv[i][3] = v.w * scale;
    }
  }
  {
    float4 graw[NQ], oraw[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int d0 = chunk_d0(i);
      graw[i] = oraw[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (d0 < HD) {
        graw[i] = ldg16(d_o + orow + d0);
        oraw[i] = ldg16(o + orow + d0);
      }
    }
    lq = ldg4(lse + ((long long)n * heads + head) * T + qc);
    retire_loads();
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const float4 g = graw[i], ov = oraw[i];
      gv[i][0] = g.x; gv[i][1] = g.y; gv[i][2] = g.z; gv[i][3] = g.w;
      dsum += (g.x * ov.x + g.y * ov.y) + (g.z * ov.z + g.w * ov.w);
    }
  }
  dsum += __shfl_xor(dsum, 32, 64);                             // D[q] = sum_d dO[q][d] O[q][d]
  f32x4 qf[X3 ? 1 : KB], dof[X3 ? 1 : KB];
  bsplit8 qh[X3 ? KS : 1], ql[X3 ? KS : 1], gh[X3 ? KS : 1], gl[X3 ? KS : 1];
  if constexpr (X3) {
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      float q8[8], g8[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        q8[e] = qv[2 * j + (e >> 2)][e & 3];
        g8[e] = gv[2 * j + (e >> 2)][e & 3];
      }
      bwd_split8(q8, qh[j], ql[j]);
      bwd_split8(g8, gh[j], gl[j]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < KB; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        qf[j][e] = qv[j][e];
        dof[j][e] = gv[j][e];
      }
  }

  request(0);
  deposit(smem);
  lds_written();
  if (nb > 1) request(1);
  __builtin_amdgcn_sched_barrier(0);
  __syncthreads();

  f32x16 dq[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) dq[dt][e] = 0.f;

  for (int b = 0; b < nb; ++b) {
    const float* Ks = smem + (b & 1) * 2 * IMG;
    const float* Vs = Ks + IMG;
#pragma unroll 1
    for (int kt = 0; kt < 2; ++kt) {
      const int k0 = b * BSTR + kt * 32;                        // first key of the tile; row kt * 32 of the images
      if (k0 >= T) break;                                       // (the same for every wave of the grid)
      f32x16 s, dp;
#pragma unroll
      for (int e = 0; e < 16; ++e) { s[e] = 0.f; dp[e] = 0.f; }
      if constexpr (X3) {
#pragma unroll
        for (int j = 0; j < KS; ++j) {
          const bool past = 16 * j + 8 * hh >= HD;
          bsplit8 kh, kl, vh, vl;
          PsImg<HD>::row8(Ks, kt * 32 + l31, 16 * j + 8 * hh, past, kh, kl);
          PsImg<HD>::row8(Vs, kt * 32 + l31, 16 * j + 8 * hh, past, vh, vl);
          mfma_x3(s, kh, kl, qh[j], ql[j]);                     // S^T[key][query]
          mfma_x3(dp, vh, vl, gh[j], gl[j]);                    // dP^T[key][query]
        }
      } else {
        const float* kp = Ks + (kt * 32 + l31) * HDP + 4 * hh;
        const float* vp = Vs + (kt * 32 + l31) * HDP + 4 * hh;
#pragma unroll
        for (int j = 0; j < KB; ++j) {
          const f32x4 kf = *reinterpret_cast<const f32x4*>(kp + 8 * j);
          const f32x4 vf = *reinterpret_cast<const f32x4*>(vp + 8 * j);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[u], qf[j][u], s, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[u], dof[j][u], dp, 0, 0, 0);
          }
        }
      }
      f32x16 ds;
      const bool ragged = k0 + 32 > T;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        float p = exp_le0(s[e] - lq);
        if (ragged && k0 + (e & 3) + 8 * (e >> 2) + 4 * hh >= T) p = 0.f;   // keys past the sequence (staged as zero rows)
        ds[e] = p * (dp[e] - dsum);
      }
      if constexpr (X3) {   // dQ^T[d][query] += K^T[d][key] dS^T[key][query]
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
          float d8[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) d8[j] = ds[8 * h2 + j];
          bsplit8 dsh, dsl;
          bwd_split8(d8, dsh, dsl);
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            bsplit8 ah, al;
            PsImg<HD>::col8(Ks, kt * 32, min(dt * 32 + l31, HD - 1), h2, hh, ah, al);   // (channels past hd: rows of dQ^T nobody stores)
            mfma_x3(dq[dt], ah, al, dsh, dsl);
          }
        }
      } else {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const float* kr = Ks + (kt * 32 + (u & 3) + 8 * (u >> 2) + 4 * hh) * HDP + l31;
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) dq[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kr[dt * 32], ds[u], dq[dt], 0, 0, 0);
          if ((u & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    // the next block (requested one iteration ago) goes to the other buffer -- last read in iteration b - 1, behind a barrier; the one
    // after it is requested now and flies through the next iteration's MFMAs
    if (b + 1 < nb) {
      deposit(smem + ((b + 1) & 1) * 2 * IMG);
      lds_written();
      if (b + 2 < nb) request(b + 2);
      __builtin_amdgcn_sched_barrier(0);
      __syncthreads();
    }
  }

  float4 efac[DT * 4];
  epilogue_factors<HD, DT>(efac, cos_tab, sin_tab, qc, rot_half, hh);
  if (q >= T) return;
  // dQ^T[d][query]: lane = query row, registers 4g..4g+3 = channels dt*32 + 8g + 4hh ..+3
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = dt * 32 + 8 * g + 4 * hh;
      if (d >= HD) continue;
      float4 v = make_float4(dq[dt][4 * g] * scale, dq[dt][4 * g + 1] * scale, dq[dt][4 * g + 2] * scale, dq[dt][4 * g + 3] * scale);
      v = rot_inv(v, efac[dt * 4 + g]);
      dqkv_store4(dqkv, (long long)n * T + q, D3, head * HD + d, v, osplit);
    }
}

// ------------------------------------------------------------------------------------------- dK, dV
template <int HD, bool X3>
__global__ __launch_bounds__(512) void attn_bwd_stream_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ o,
                                                                  const float* __restrict__ d_o, const float* __restrict__ lse,
                                                                  float* __restrict__ dqkv, const float* __restrict__ cos_tab,
                                                                  const float* __restrict__ sin_tab, int T, int heads, int rot_half, int osplit,
                                                                  int kblocks) {
  constexpr int HDP = HD + 4, KB = HD / 8, DT = (HD + 31) / 32, KS = (HD + 15) / 16, CPR = HD / 4, NIT = (CPR + 7) / 8;
  constexpr int IMG = BwdStreamGeom<HD>::IMG;
  // (hd = 72, fp32: the third channel tile's operand reads run past a row into the next row / image / the lse rows: never-stored rows)
  extern __shared__ __attribute__((aligned(16))) float smem[];   // [buffer][Q image | dO image], then [buffer][lse 64 | D 64]
  float* LD = smem + 4 * IMG;
  const int pair = blockIdx.x / kblocks, kb = blockIdx.x - pair * kblocks;
  const int n = pair / heads, head = pair - n * heads;
  const int D = heads * HD, D3 = 3 * D, R = 2 * rot_half;
  const float* base = qkv + (long long)n * T * D3 + head * HD;
  const float* gbase = d_o + (long long)n * T * D + head * HD;
  const float* obase = o + (long long)n * T * D + head * HD;
  const float* lbase = lse + ((long long)n * heads + head) * T;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hh = lane >> 5;
  const int srow = tid >> 3, sub = tid & 7;
  const int nb = (T + BSTR - 1) / BSTR;
  const float scale = rsqrtf((float)HD);

  // one block's staging in two passes (Q with its rotary factors, then dO with O), each: loads, ONE wait, LDS writes -- 25 staged
  // registers at a time beside the fragments and accumulators
  auto stage_q = [&](int b, int which) {
    float* buf = smem + which * 2 * IMG;
    const int qi = b * BSTR + srow;
    float4 qst[NIT], cst[NIT];
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int c = sub + 8 * i, d0 = 4 * c;
      qst[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      cst[i] = make_float4(1.f, 0.f, 1.f, 0.f);
      if (c < CPR && qi < T) {
        qst[i] = ldg16(base + ((unsigned)qi * (unsigned)D3 + (unsigned)d0));   // (uniform base + 32-bit lane offset: < 2^27 floats per sample)
        if (d0 < R) {
          const int pi = qi * rot_half + (d0 >> 1);
          const float2 cc = ldg8(cos_tab + (unsigned)pi), ss = ldg8(sin_tab + (unsigned)pi);
          cst[i] = make_float4(cc.x, ss.x, cc.y, ss.y);
        }
      }
    }
    retire_loads();
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int c = sub + 8 * i, d0 = 4 * c;
      if (c >= CPR) continue;
      float4 qv = rot_fwd(qst[i], cst[i]);
      qv = make_float4(qv.x * scale, qv.y * scale, qv.z * scale, qv.w * scale);
      if constexpr (X3) PsImg<HD>::st4(buf, srow, d0, qv);
      else *reinterpret_cast<float4*>(buf + srow * HDP + d0) = qv;
    }
    lds_written();
  };
  auto stage_g = [&](int b, int which) {
    float* buf = smem + which * 2 * IMG + IMG;
    const int qi = b * BSTR + srow;
    float4 gst[NIT], ost[NIT];
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int c = sub + 8 * i, d0 = 4 * c;
      gst[i] = ost[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < CPR && qi < T) {
        gst[i] = ldg16(gbase + ((unsigned)qi * (unsigned)D + (unsigned)d0));
        ost[i] = ldg16(obase + ((unsigned)qi * (unsigned)D + (unsigned)d0));
      }
    }
    const float lst = qi < T ? ldg4(lbase + (unsigned)qi) : 0.f;
    retire_loads();
    float dd = 0.f;
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int c = sub + 8 * i, d0 = 4 * c;
      if (c >= CPR) continue;
      const float4 g = gst[i], ov = ost[i];
      dd += (g.x * ov.x + g.y * ov.y) + (g.z * ov.z + g.w * ov.w);
      if constexpr (X3) PsImg<HD>::st4(buf, srow, d0, g);
      else *reinterpret_cast<float4*>(buf + srow * HDP + d0) = g;
    }
    dd += __shfl_xor(dd, 1, 64);                                // the row's eight threads are neighbouring lanes
    dd += __shfl_xor(dd, 2, 64);
    dd += __shfl_xor(dd, 4, 64);
    if (sub == 0) {
      LD[which * 2 * BSTR + srow] = lst;
      LD[which * 2 * BSTR + BSTR + srow] = dd;                  // D = rowsum(dO * O); 0 for rows past the sequence
    }
    lds_written();
  };

  // ---- prologue: this lane's key (clamped in the partial last tile): loads, ONE wait, first use
  const int key = kb * BOWN + wave * 32 + l31, kc = min(key, T - 1);
  const bool key_ok = key < T;
  constexpr int NQ = X3 ? 2 * KS : KB;
  auto chunk_d0 = [&](int i) { return X3 ? 16 * (i >> 1) + 8 * hh + 4 * (i & 1) : 8 * i + 4 * hh; };
  f32x4 kf[X3 ? 1 : KB], vf[X3 ? 1 : KB];
  bsplit8 kh[X3 ? KS : 1], kl[X3 ? KS : 1], vh[X3 ? KS : 1], vl[X3 ? KS : 1];
  {
    float4 kraw[NQ], vraw[NQ], fac[NQ];
    const float* rowp = base + (long long)kc * D3;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int d0 = chunk_d0(i);
      kraw[i] = vraw[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      fac[i] = make_float4(1.f, 0.f, 1.f, 0.f);
      if (d0 < HD) {
        kraw[i] = ldg16(rowp + D + d0);
        vraw[i] = ldg16(rowp + 2 * D + d0);
        if (d0 < R) {
          const int pi = kc * rot_half + (d0 >> 1);
          const float2 cc = ldg8(cos_tab + pi), ss = ldg8(sin_tab + pi);
          fac[i] = make_float4(cc.x, ss.x, cc.y, ss.y);
        }
      }
    }
    retire_loads();
    if constexpr (X3) {
#pragma unroll
      for (int j = 0; j < KS; ++j) {
        float k8[8], v8[8];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const float4 kv = rot_fwd(kraw[2 * j + u], fac[2 * j + u]), vv = vraw[2 * j + u];
          k8[4 * u] = kv.x; k8[4 * u + 1] = kv.y; k8[4 * u + 2] = kv.z; k8[4 * u + 3] = kv.w;
          v8[4 * u] = vv.x; v8[4 * u + 1] = vv.y; v8[4 * u + 2] = vv.z; v8[4 * u + 3] = vv.w;
        }
        bwd_split8(k8, kh[j], kl[j]);
        bwd_split8(v8, vh[j], vl[j]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        const float4 kv = rot_fwd(kraw[j], fac[j]), vv = vraw[j];
        kf[j][0] = kv.x; kf[j][1] = kv.y; kf[j][2] = kv.z; kf[j][3] = kv.w;
        vf[j][0] = vv.x; vf[j][1] = vv.y; vf[j][2] = vv.z; vf[j][3] = vv.w;
      }
    }
  }

  stage_q(0, 0);
  stage_g(0, 0);
  __builtin_amdgcn_sched_barrier(0);
  __syncthreads();

  f32x16 dk[DT], dv[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) { dk[dt][e] = 0.f; dv[dt][e] = 0.f; }

  for (int b = 0; b < nb; ++b) {
    // the next block goes to the other buffer -- last read in iteration b - 1, behind a barrier -- BEFORE this block's products: the staged
    // registers are dead while the products run (see the header)
    if (b + 1 < nb) {
      stage_q(b + 1, (b + 1) & 1);
      stage_g(b + 1, (b + 1) & 1);
      __builtin_amdgcn_sched_barrier(0);
    }
    const float* Qs = smem + (b & 1) * 2 * IMG;
    const float* Gs = Qs + IMG;
    const float* Ls = LD + (b & 1) * 2 * BSTR;
    const float* Ds = Ls + BSTR;
#pragma unroll 1
    for (int qt = 0; qt < 2; ++qt) {
      const int q0 = b * BSTR + qt * 32;                        // first query of the tile; row qt * 32 of the images
      if (q0 >= T) break;                                       // (the same for every wave of the grid)
      f32x16 s, dp;
#pragma unroll
      for (int e = 0; e < 16; ++e) { s[e] = 0.f; dp[e] = 0.f; }
      if constexpr (X3) {
#pragma unroll
        for (int j = 0; j < KS; ++j) {
          const bool past = 16 * j + 8 * hh >= HD;
          bsplit8 qfh, qfl, gfh, gfl;
          PsImg<HD>::row8(Qs, qt * 32 + l31, 16 * j + 8 * hh, past, qfh, qfl);
          PsImg<HD>::row8(Gs, qt * 32 + l31, 16 * j + 8 * hh, past, gfh, gfl);
          mfma_x3(s, qfh, qfl, kh[j], kl[j]);                   // S[query][key]
          mfma_x3(dp, gfh, gfl, vh[j], vl[j]);                  // dP[query][key]
        }
      } else {
        const float* qp = Qs + (qt * 32 + l31) * HDP + 4 * hh;
        const float* gp = Gs + (qt * 32 + l31) * HDP + 4 * hh;
#pragma unroll
        for (int j = 0; j < KB; ++j) {
          const f32x4 qf = *reinterpret_cast<const f32x4*>(qp + 8 * j);
          const f32x4 gf = *reinterpret_cast<const f32x4*>(gp + 8 * j);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[u], kf[j][u], s, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x2f32(gf[u], vf[j][u], dp, 0, 0, 0);
          }
        }
      }
      f32x16 p, ds;
      const bool ragged = q0 + 32 > T;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int qrow = (e & 3) + 8 * (e >> 2) + 4 * hh;
        float pv = exp_le0(s[e] - Ls[qt * 32 + qrow]);
        if (!key_ok || (ragged && q0 + qrow >= T)) pv = 0.f;     // clamped key column / queries past the sequence (zero rows)
        p[e] = pv;
        ds[e] = pv * (dp[e] - Ds[qt * 32 + qrow]);
      }
      if constexpr (X3) {   // dV^T[d][key] += dO^T[d][query] P[query][key], dK^T[d][key] += Q^T[d][query] dS[query][key]
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
          float p8[8], d8[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            p8[j] = p[8 * h2 + j];
            d8[j] = ds[8 * h2 + j];
          }
          bsplit8 ph, pl, dsh, dsl;
          bwd_split8(p8, ph, pl);
          bwd_split8(d8, dsh, dsl);
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            bsplit8 ah, al;
            const int dcol = min(dt * 32 + l31, HD - 1);        // (channels past hd: accumulator rows nobody stores)
            PsImg<HD>::col8(Gs, qt * 32, dcol, h2, hh, ah, al);
            mfma_x3(dv[dt], ah, al, ph, pl);
            PsImg<HD>::col8(Qs, qt * 32, dcol, h2, hh, ah, al);
            mfma_x3(dk[dt], ah, al, dsh, dsl);
          }
        }
      } else {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const int qrow = qt * 32 + (u & 3) + 8 * (u >> 2) + 4 * hh;
          const float* gr = Gs + qrow * HDP + l31;
          const float* qr = Qs + qrow * HDP + l31;
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            dv[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(gr[dt * 32], p[u], dv[dt], 0, 0, 0);    // dV^T[d][key]
            dk[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(qr[dt * 32], ds[u], dk[dt], 0, 0, 0);   // dK_rot^T[d][key]
          }
          if ((u & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (b + 1 < nb) __syncthreads();
  }

  float4 efac[DT * 4];
  epilogue_factors<HD, DT>(efac, cos_tab, sin_tab, kc, rot_half, hh);
  if (!key_ok) return;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = dt * 32 + 8 * g + 4 * hh;
      if (d >= HD) continue;
      float4 kv = make_float4(dk[dt][4 * g], dk[dt][4 * g + 1], dk[dt][4 * g + 2], dk[dt][4 * g + 3]);
      kv = rot_inv(kv, efac[dt * 4 + g]);
      dqkv_store4(dqkv, (long long)n * T + key, D3, head * HD + D + d, kv, osplit);
      dqkv_store4(dqkv, (long long)n * T + key, D3, head * HD + 2 * D + d,
                  make_float4(dv[dt][4 * g], dv[dt][4 * g + 1], dv[dt][4 * g + 2], dv[dt][4 * g + 3]), osplit);
    }
}

template <int HD, bool X3>
static int launch_bwd_stream(const float* qkv, const float* o, const float* d_o, const float* lse, float* dqkv, const float* ct,
                             const float* st, int N, int T, int heads, int rot_half, hipStream_t s, int osplit) {
  const size_t lds = attn_lds_one_per_cu(BwdStreamGeom<HD>::BYTES);   // one workgroup per CU (common.h attn_prepare_kernel)
  const int blocks = (T + BOWN - 1) / BOWN;
  auto kq = attn_bwd_stream_dq_kernel<HD, X3>;
  auto kkv = attn_bwd_stream_dkv_kernel<HD, X3>;
  static bool prepared = false;
  if (!prepared) {
    RGM_TRY(attn_prepare_kernel(kq, 512, lds, "attn_bwd_stream_dq_kernel"));
    RGM_TRY(attn_prepare_kernel(kkv, 512, lds, "attn_bwd_stream_dkv_kernel"));
    prepared = true;
  }
  hipLaunchKernelGGL(kq, dim3(N * heads * blocks), dim3(512), lds, s, qkv, o, d_o, lse, dqkv, ct, st, T, heads, rot_half, osplit, blocks);
  RGM_LAUNCH_CHECK();
  hipLaunchKernelGGL(kkv, dim3(N * heads * blocks), dim3(512), lds, s, qkv, o, d_o, lse, dqkv, ct, st, T, heads, rot_half, osplit, blocks);
  RGM_LAUNCH_CHECK();
  ++g_bwd_stream_launches;
  return RGM_OK;
}

bool attn_bwd_stream_wanted(int T, int hd) {
  if (hd != 64 && hd != 72) return false;
  return g_bwd_stream_force || (hd == 72 && T > 256) || T > 288;
}

int rotary_attention_bwd_stream_launch(const float* qkv, const float* o, const float* d_o, const float* lse, float* dqkv,
                                       const float* cos_tab, const float* sin_tab, int N, int T, int heads, int hd, int rot_half,
                                       hipStream_t s, int osplit, int x3) {
  RGM_REQUIRE(N > 0 && T > 0 && T <= ATTN_STREAM_MAX_T, "attention backward: T=%d out of range (1..%d)", T, ATTN_STREAM_MAX_T);
  RGM_REQUIRE((2 * rot_half) % 4 == 0 && 2 * rot_half <= 64, "attention backward: rotary dim %d (a multiple of 4, at most 64)", 2 * rot_half);
  RGM_REQUIRE((long long)N * heads * ((T + BOWN - 1) / BOWN) <= 0x7fffffff, "attention backward: grid of N=%d heads=%d T=%d", N, heads, T);
  if (hd == 72) return x3 ? launch_bwd_stream<72, true>(qkv, o, d_o, lse, dqkv, cos_tab, sin_tab, N, T, heads, rot_half, s, osplit)
                          : launch_bwd_stream<72, false>(qkv, o, d_o, lse, dqkv, cos_tab, sin_tab, N, T, heads, rot_half, s, osplit);
  if (hd == 64) return x3 ? launch_bwd_stream<64, true>(qkv, o, d_o, lse, dqkv, cos_tab, sin_tab, N, T, heads, rot_half, s, osplit)
                          : launch_bwd_stream<64, false>(qkv, o, d_o, lse, dqkv, cos_tab, sin_tab, N, T, heads, rot_half, s, osplit);
  set_error("attention backward: head_dim %d not supported (64, 72)", hd);
  return RGM_ERR_INVALID;
}

int attn_bwd_stream_force_set(int on) {
  const int prev = g_bwd_stream_force;
  g_bwd_stream_force = on;
  return prev;
}

}  // namespace rgm

// 1 = the streaming attention backward for every sequence length (comparisons against the resident kernels, tests), 0 = only where the
// resident kernels cannot hold a head (default).  Returns the previous setting.
extern "C" int rgm_set_attn_bwd_stream(int on) { return rgm::attn_bwd_stream_force_set(on != 0); }
// launches of the streaming backward (dq + dkv pair) so far in this process
extern "C" long long rgm_attn_bwd_stream_launches(void) { return rgm::g_bwd_stream_launches; }
