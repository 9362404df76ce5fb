// attention_stream.hip -- the RotaryAttention core of attention.hip / attention_x3.hip for sequences too long to keep a head's K and V
// in LDS (hd 72 at T > 256, hd 64 at T > 288; up to ATTN_STREAM_MAX_T tokens): long excerpts, the reference's `--image_size H 16`
// with H > 128 (guided_diffusion/dit.py:538-634 does not depend on the length; rotary positions).
//
// Flash-style forward.  A workgroup (8 waves) owns 256 queries of one (sample, head), 32 per wave; the keys stream through two LDS
// buffers in blocks of 64 with the running-maximum softmax (m, l per query in fp32; the output accumulators are rescaled once per
// block), so no T x T score matrix exists anywhere.  The structure is the key-blocked kernel of attention_x3.hip grown to any length:
//   * block b+2's rows are requested into registers before block b+1's products start and written to LDS (rotated, split / transposed)
//     after them, one barrier per block (register staging, the STAGE_LOAD / STAGE_WRITE split);
//   * scores are TRANSPOSED, S^T = K . Q^T: the probabilities come out in the B-operand layout of O^T = V^T . P^T and never leave the
//     register file;
//   * the rotary factors of a key come from the global cos / sin tables with its K chunk (the table of a whole sequence no longer fits
//     beside the blocks), those of a query in the two-phase Q prologue -- every prologue load retired before the first use.
// Both arithmetics of the resident pair:
//   X3 = 0 (precision 0): exact fp32 products on v_mfma_f32_32x32x2_f32, scores in the natural-log domain (exp_neg), K rows padded to
//          hd + 4 floats (odd 16-byte slot stride), V rows plain -- the LDS images of attention.hip per block;
//   X3 = 1 (precisions 1 / 2): hi + lo split operands on v_mfma_f32_32x32x16_bf16, three MFMAs per product, scores in the log2 domain;
//          K [key][hi KP | lo KP | pad] and V^T [d][hi 64 | lo 64 | pad] with the keys of every 32-group permuted so that a lane's
//          probabilities of one k16 step are 16 contiguous bytes -- the images of attention_x3_body.h per block.
// One workgroup per CU (attn_prepare_kernel), and two explicit waits around the register staging, found by repeat runs (the same launch
// N times on fixed inputs, rows compared bitwise):
//   * retire_loads(): every load retired by ONE wait, then 32 idle cycles, before any destination register is read (the Q prologue and
//     each block's deposit).  With the compiler's counted waits in deposit() -- uses right behind them -- the hd 64 bf16x3 instance
//     returned wrong rows in about one launch of four even ALONE on its CU (the DESIGN 4h pattern inside one workgroup);
//   * lds_written(): a block's LDS writes complete before the next block's loads are issued.  Without it one workgroup in ~10^5 produced
//     slightly different rows (2 of 200 launches of 1024 workgroups): the loads may land in registers that still hold the data of writes
//     just issued.  With both, 0 of 1200 launches differed (hd 72 N 16 T 1024, hd 64 N 8 T 576).
#include "common.h"
#include "attention_x3_body.h"

namespace rgm {

namespace {
// every outstanding load retired, then 32 idle cycles before the first read of a destination register (see the header)
__device__ __forceinline__ void retire_loads() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_waitcnt vmcnt(0)\n\ts_nop 7\n\ts_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}
// the block's LDS writes done before the next block's loads are issued: those loads land in registers the register allocator may have
// given to the data of the writes just issued
__device__ __forceinline__ void lds_written() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}
constexpr int SQ = 256;   // queries per workgroup: 8 waves x 32
constexpr int SKB = 64;   // keys per streamed block
int g_attn_stream_force = 0;   // rgm_set_attn_stream: 1 = every shape of hd 64 / 72 takes this kernel (comparisons against the resident kernels)
}  // namespace

template <int HD, int X3>
struct StreamGeom {
  static constexpr int KP = X3 ? (HD + 15) / 16 * 16 : HD;   // K row length in LDS (x3: the k16 contraction, zero-padded)
  static constexpr int KROW = X3 ? KP * 4 + 16 : (HD + 4) * 4;  // bytes per K row: odd number of 16-byte slots
  static constexpr int VROW = X3 ? SKB * 4 + 16 : HD * 4;       // bytes per V^T row (x3, 17 slots) / V row (fp32)
  static constexpr int VBYTES = X3 ? HD * VROW : SKB * VROW;
  static constexpr int BUF = VBYTES + SKB * KROW;              // V first: the fp32 kernel's reads of the last 32-wide channel tile run
                                                               // past the last V row into the block's K rows (finite, discarded outputs)
  static_assert(!X3 || ((KROW / 16) % 2 == 1 && (VROW / 16) % 2 == 1), "slot strides must be odd");
  static_assert(X3 || (KROW / 16) % 2 == 1, "K slot stride must be odd");
};

// TAIL = 1: the last, partial query tile of every (sample, head), launched on its own (qb = qb0): there ALL eight waves run every
// block, a wave without a query (q0 >= T) on the clamped query qc, storing nothing.  When such waves skipped the block's products,
// the other waves of that workgroup returned wrong rows that differed from launch to launch (hd 64 bf16x3, T = 6001: 37 of 40
// launches; hd 72: 1 of 40); running them gave 0 of 40.  The full tiles keep the TAIL = 0 instance, whose waves all have queries.
template <int HD, int X3, int TAIL>
__global__ __launch_bounds__(512) void rotary_attention_stream_kernel(const float* __restrict__ qkv, float* __restrict__ o,
                                                                      const float* __restrict__ cos_tab, const float* __restrict__ sin_tab,
                                                                      int T, int heads, int rot_half, float* __restrict__ lse, int out_split,
                                                                      int qblocks, int qb0) {
  using G = StreamGeom<HD, X3>;
  constexpr int KP = G::KP, KROW = G::KROW, VROW = G::VROW, VBYTES = G::VBYTES, BUF = G::BUF;
  constexpr int KS = (HD + 15) / 16;        // x3: k16 steps of QK^T
  constexpr int KB8 = HD / 8;               // fp32: k-blocks of 8 channels in QK^T
  constexpr int DT = (HD + 31) / 32;        // 32-wide output-channel tiles
  constexpr int CPR = KP / 4;               // float4 chunks per K row
  constexpr int KCH = SKB * CPR;
  constexpr int KSLOTS = (KCH + 511) / 512;
  // V chunks.  x3: indexed so that ONE transposing ds_write_b16 of a wave covers 32 keys x 2 channel chunks of opposite parity (32
  // different banks; attention_x3.hip, blocked kernel).  fp32: row-major like K.
  constexpr int VCH = HD / 4;
  constexpr int VPAIRS = (VCH + 1) / 2;
  constexpr int VITEMS = X3 ? (SKB / 32) * VPAIRS * 64 : SKB * VCH;
  constexpr int VSLOTS = (VITEMS + 511) / 512;
  typedef split_t bf16x4 __attribute__((ext_vector_type(4)));
  extern __shared__ __attribute__((aligned(16))) char smem_s[];

  const int pair = blockIdx.x / qblocks, qb = TAIL ? qb0 : blockIdx.x - pair * qblocks;
  const int n = pair / heads, head = pair - n * heads;
  const int D = heads * HD, D3 = 3 * D;
  const float* base = qkv + (long long)n * T * D3 + head * HD;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hh = lane >> 5;
  const int R = 2 * rot_half;
  const int nb = (T + SKB - 1) / SKB;
  const int q0 = qb * SQ + wave * 32;
  const bool active = TAIL || q0 < T;                          // wave-uniform: this wave runs the blocks (see TAIL)
  const int q = q0 + l31;
  const int qc = min(q, T - 1);

  float4 kq[KSLOTS], kf[KSLOTS], vq[VSLOTS];                  // one block's K chunks, their rotary factors (c0, s0, c1, s1), V chunks
  auto v_item = [&](int sl, int& key, int& d0) {               // false: no chunk in this slot
    const int w = tid + sl * 512;
    if constexpr (X3) {
      const int wv = w >> 6, ln = w & 63;
      const int g32 = wv % (SKB / 32), it = wv / (SKB / 32);
      key = g32 * 32 + (ln & 31);
      d0 = (2 * it + (ln >> 5)) * 4;
      return w < VITEMS && d0 < HD;
    } else {
      key = w / VCH;
      d0 = (w - key * VCH) * 4;
      return w < VITEMS;
    }
  };
  auto request = [&](int b) {
#pragma unroll
    for (int sl = 0; sl < KSLOTS; ++sl) {
      const int c = tid + sl * 512;
      const int key = c / CPR, d0 = (c - key * CPR) * 4, kg = b * SKB + key;
      kq[sl] = make_float4(0.f, 0.f, 0.f, 0.f);
      kf[sl] = make_float4(1.f, 0.f, 1.f, 0.f);
      if (c < KCH && kg < T && d0 < HD) {
        kq[sl] = ldg16(base + (long long)kg * D3 + D + d0);
        if (d0 < R) {
          const int pi = kg * rot_half + (d0 >> 1);
          const float2 cc = ldg8(cos_tab + pi), ss = ldg8(sin_tab + pi);
          kf[sl] = make_float4(cc.x, ss.x, cc.y, ss.y);
        }
      }
    }
#pragma unroll
    for (int sl = 0; sl < VSLOTS; ++sl) {
      int key, d0;
      vq[sl] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (v_item(sl, key, d0) && b * SKB + key < T) vq[sl] = ldg16(base + (long long)(b * SKB + key) * D3 + 2 * D + d0);
    }
  };
  auto deposit = [&](char* buf) {        // rotate (and split) K, write K rows and the V image of the block held in registers
    char* Vs = buf;
    char* Ks = buf + VBYTES;
    // every load of the block retired in front of all uses (see the header); they were issued a whole block of MFMAs ago
    retire_loads();
#pragma unroll
    for (int sl = 0; sl < KSLOTS; ++sl) {
      const int c = tid + sl * 512;
      if (c >= KCH) continue;
      const int key = c / CPR, d0 = (c - key * CPR) * 4;
      const float4 x = kq[sl], f = kf[sl];
      const float kr[4] = {x.x * f.x - x.y * f.y, x.y * f.x + x.x * f.y, x.z * f.z - x.w * f.w, x.w * f.z + x.z * f.w};
      if constexpr (X3) {
        bf16x4 hi, lo;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          hi[i] = (split_t)kr[i];
          lo[i] = (split_t)(kr[i] - (float)hi[i]);
        }
        char* krp = Ks + key * KROW + d0 * 2;
        *reinterpret_cast<bf16x4*>(krp) = hi;
        *reinterpret_cast<bf16x4*>(krp + KP * 2) = lo;
      } else {
        *reinterpret_cast<float4*>(Ks + key * KROW + d0 * 4) = make_float4(kr[0], kr[1], kr[2], kr[3]);
      }
    }
#pragma unroll
    for (int sl = 0; sl < VSLOTS; ++sl) {
      int key, d0;
      if (!v_item(sl, key, d0)) continue;
      if constexpr (X3) {
        // key -> position inside its 32-group: key = (j&3) + 8*(2*h2 + (j>>2)) + 4*half  <->  pos = 16*h2 + 8*half + j
        const int k32 = key & 31;
        const int half = (k32 >> 2) & 1, blk = k32 >> 3;
        const int pos = (key & ~31) + 16 * (blk >> 1) + 8 * half + 4 * (blk & 1) + (k32 & 3);
        const float vs[4] = {vq[sl].x, vq[sl].y, vq[sl].z, vq[sl].w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const split_t vh = (split_t)vs[i];
          char* vr = Vs + (d0 + i) * VROW + pos * 2;
          *reinterpret_cast<split_t*>(vr) = vh;
          *reinterpret_cast<split_t*>(vr + SKB * 2) = (split_t)(vs[i] - (float)vh);
        }
      } else {
        *reinterpret_cast<float4*>(Vs + key * VROW + d0 * 4) = vq[sl];
      }
    }
  };

  request(0);
  // ---- Q prologue, two-phase: every load issued, then ONE wait that retires them all (block 0's included), then the first use
  float4 qraw[KS * 2];
  float4 qfac[KS * 2];
  {
    const float* qp = base + (long long)qc * D3;
#pragma unroll
    for (int i = 0; i < KS * 2; ++i) {
      // x3: lane (query l31, half hh) holds channels 16j + 8hh + 4u (i = 2j + u); fp32: 8j + 4hh (i = j < HD / 8)
      const int d0 = X3 ? 16 * (i >> 1) + 8 * hh + 4 * (i & 1) : 8 * i + 4 * hh;
      qraw[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      qfac[i] = make_float4(1.f, 0.f, 1.f, 0.f);
      if ((X3 || i < KB8) && d0 < HD) {
        qraw[i] = ldg16(qp + d0);
        if (d0 < R) {
          const int pi = qc * rot_half + (d0 >> 1);
          const float2 cc = ldg8(cos_tab + pi), ss = ldg8(sin_tab + pi);
          qfac[i] = make_float4(cc.x, ss.x, cc.y, ss.y);
        }
      }
    }
  }
  retire_loads();
  // scores: x3 in the log2 domain (log2(e) folded into the query scale, p = one v_exp_f32), fp32 in the natural domain (exp_neg)
  const float scale = X3 ? rsqrtf((float)HD) * 1.44269504088896340736f : rsqrtf((float)HD);
  float qs[KS * 2][4];
#pragma unroll
  for (int i = 0; i < KS * 2; ++i) {
    const float4 v = qraw[i], f = qfac[i];
    qs[i][0] = (v.x * f.x - v.y * f.y) * scale;
    qs[i][1] = (v.y * f.x + v.x * f.y) * scale;
    qs[i][2] = (v.z * f.z - v.w * f.w) * scale;
    qs[i][3] = (v.w * f.z + v.z * f.w) * scale;
  }
  bf16x8 qh[X3 ? KS : 1], ql[X3 ? KS : 1];
  f32x4 qf[X3 ? 1 : KB8];
  if constexpr (X3) {
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      float v8[8];
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) v8[4 * u + e] = qs[2 * j + u][e];
      split8(v8, qh[j], ql[j]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < KB8; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) qf[j][e] = qs[j][e];
  }

  deposit(smem_s);
  lds_written();
  if (nb > 1) request(1);
  __builtin_amdgcn_sched_barrier(0);
  __syncthreads();

  f32x16 oacc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) oacc[dt][e] = 0.f;
  int vrow[DT];                                                 // x3: V^T rows >= hd feed discarded outputs
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) vrow[dt] = min(dt * 32 + l31, HD - 1) * VROW + 16 * hh;
  float m_run = -INFINITY, l_run = 0.f;

  for (int b = 0; b < nb; ++b) {
    const char* Vs = smem_s + (b & 1) * BUF;
    const char* Ks = Vs + VBYTES;
    if (active) {
      // ---- S^T of the block's two key tiles
      f32x16 sacc[2];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
        for (int e = 0; e < 16; ++e) sacc[kt][e] = 0.f;
        if constexpr (X3) {
          const char* kp = Ks + (kt * 32 + l31) * KROW + 16 * hh;
#pragma unroll
          for (int j = 0; j < KS; ++j) {
            const bf16x8 kh = *reinterpret_cast<const bf16x8*>(kp + 32 * j);
            const bf16x8 kl = *reinterpret_cast<const bf16x8*>(kp + 32 * j + KP * 2);
            sacc[kt] = RGM_MFMA_SPLIT_32x32x16(kl, qh[j], sacc[kt], 0, 0, 0);
            sacc[kt] = RGM_MFMA_SPLIT_32x32x16(kh, ql[j], sacc[kt], 0, 0, 0);
            sacc[kt] = RGM_MFMA_SPLIT_32x32x16(kh, qh[j], sacc[kt], 0, 0, 0);
          }
        } else {
          const float* kp = reinterpret_cast<const float*>(Ks + (kt * 32 + l31) * KROW) + 4 * hh;
#pragma unroll
          for (int j = 0; j < KB8; ++j) {
            const f32x4 kv = *reinterpret_cast<const f32x4*>(kp + 8 * j);
#pragma unroll
            for (int s = 0; s < 4; ++s) sacc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kv[s], qf[j][s], sacc[kt], 0, 0, 0);
          }
        }
      }
      // ---- running softmax: register e of tile kt is key b*64 + kt*32 + (e&3) + 8*(e>>2) + 4*hh
      float mx = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        const int k0 = b * SKB + kt * 32;
        if (k0 + 32 > T) {                   // ragged or empty tile (wave-uniform)
#pragma unroll
          for (int e = 0; e < 16; ++e)
            if (k0 + (e & 3) + 8 * (e >> 2) + 4 * hh >= T) sacc[kt][e] = -INFINITY;
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) mx = fmaxf(mx, sacc[kt][e]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx);                     // finite from block 0 on (key 0 is never masked)
      // 0 for the first block (m_run = -inf), 1 when nothing grew
      const float alpha = X3 ? __builtin_amdgcn_exp2f(m_run - m_new) : exp_neg(m_run - m_new);
      float sum = 0.f;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float pv = X3 ? __builtin_amdgcn_exp2f(sacc[kt][e] - m_new) : exp_neg(sacc[kt][e] - m_new);   // masked: 0
          sacc[kt][e] = pv;
          sum += pv;
        }
      sum += __shfl_xor(sum, 32, 64);
      l_run = l_run * alpha + sum;
      m_run = m_new;
      if (b > 0) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
          for (int e = 0; e < 16; ++e) oacc[dt][e] *= alpha;
      }
      // ---- O^T += V^T . P^T over the block's 64 keys
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        if constexpr (X3) {
#pragma unroll
          for (int h2 = 0; h2 < 2; ++h2) {
            float p8[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) p8[j] = sacc[kt][8 * h2 + j];
            bf16x8 ph, pl;
            split8(p8, ph, pl);
            const int koff = (kt * 32 + 16 * h2) * 2;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
              const bf16x8 vh = *reinterpret_cast<const bf16x8*>(Vs + vrow[dt] + koff);
              const bf16x8 vl = *reinterpret_cast<const bf16x8*>(Vs + vrow[dt] + koff + SKB * 2);
              oacc[dt] = RGM_MFMA_SPLIT_32x32x16(vl, ph, oacc[dt], 0, 0, 0);
              oacc[dt] = RGM_MFMA_SPLIT_32x32x16(vh, pl, oacc[dt], 0, 0, 0);
              oacc[dt] = RGM_MFMA_SPLIT_32x32x16(vh, ph, oacc[dt], 0, 0, 0);
            }
          }
        } else {
#pragma unroll
          for (int s = 0; s < 16; ++s) {
            const float* vp = reinterpret_cast<const float*>(Vs + (kt * 32 + (s & 3) + 8 * (s >> 2) + 4 * hh) * VROW) + l31;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
              oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[dt * 32], sacc[kt][s], oacc[dt], 0, 0, 0);
            if ((s & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // keep the V reads from being hoisted (spills)
          }
        }
      }
    }   // active
    __builtin_amdgcn_sched_barrier(0);
    // ---- the next block (requested one iteration ago) goes to the other buffer -- last read in iteration b-1, behind a barrier;
    // the one after it is requested now and flies through the next iteration's MFMAs
    if (b + 1 < nb) {
      deposit(smem_s + ((b + 1) & 1) * BUF);
      lds_written();
      if (b + 2 < nb) request(b + 2);
      __builtin_amdgcn_sched_barrier(0);
      __syncthreads();
    }
  }

  if (!active || q >= T) return;   // (q >= T covers the waves TAIL runs without queries)
  const float inv = 1.0f / l_run;
  if (lse && hh == 0)   // natural-log sum-exp of the scaled scores, saved for the backward
    lse[((long long)n * heads + head) * T + q] = X3 ? (m_run + log2f(l_run)) * 0.693147180559945309417f : m_run + logf(l_run);
  float* op = o + ((long long)n * T + q) * D + head * HD;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = dt * 32 + 8 * g + 4 * hh;
      if (d < HD) {
        const float4 ov = make_float4(oacc[dt][4 * g] * inv, oacc[dt][4 * g + 1] * inv, oacc[dt][4 * g + 2] * inv, oacc[dt][4 * g + 3] * inv);
        if (out_split) {   // split-row format (common.h split_idx): A operand of the pre-split proj GEMM
          bf16x4 hi, lo;
          hi[0] = (split_t)ov.x; hi[1] = (split_t)ov.y; hi[2] = (split_t)ov.z; hi[3] = (split_t)ov.w;
          lo[0] = (split_t)(ov.x - (float)hi[0]); lo[1] = (split_t)(ov.y - (float)hi[1]);
          lo[2] = (split_t)(ov.z - (float)hi[2]); lo[3] = (split_t)(ov.w - (float)hi[3]);
          split_t* rp = reinterpret_cast<split_t*>(o + ((long long)n * T + q) * D);
          store_split4_maybe_pair<32>(rp, head * HD + d, hi, lo);   // lanes l / l + 32 (hh = 0 / 1) hold one 8-aligned group of the same row
        } else {
          *reinterpret_cast<float4*>(op + d) = ov;
        }
      }
    }
}

template <int HD, int X3, int TAIL>
static int launch_stream_part(const float* qkv, float* o, const float* ct, const float* st, int N, int T, int heads, int rot_half, float* lse,
                              int out_split, int qblocks, int qb0, hipStream_t s) {
  const size_t lds = attn_lds_one_per_cu(2 * (size_t)StreamGeom<HD, X3>::BUF);   // two block buffers; one workgroup per CU
  auto kern = rotary_attention_stream_kernel<HD, X3, TAIL>;
  static bool prepared = false;
  if (!prepared) RGM_TRY(attn_prepare_kernel(kern, 512, lds, "rotary_attention_stream_kernel"));
  prepared = true;
  hipLaunchKernelGGL(kern, dim3(N * heads * qblocks), dim3(512), lds, s, qkv, o, ct, st, T, heads, rot_half, lse, out_split, qblocks, qb0);
  RGM_LAUNCH_CHECK();
  return RGM_OK;
}

// the full query tiles, then (T % 256 != 0) the partial last tile of every (sample, head) with the TAIL instance
template <int HD, int X3>
static int launch_stream(const float* qkv, float* o, const float* ct, const float* st, int N, int T, int heads, int rot_half, float* lse,
                         int out_split, hipStream_t s) {
  const int full = T / SQ;
  if (full > 0) RGM_TRY((launch_stream_part<HD, X3, 0>(qkv, o, ct, st, N, T, heads, rot_half, lse, out_split, full, 0, s)));
  if (T % SQ) RGM_TRY((launch_stream_part<HD, X3, 1>(qkv, o, ct, st, N, T, heads, rot_half, lse, out_split, 1, full, s)));
  return RGM_OK;
}

bool attn_stream_wanted(int T, int hd) {
  if (hd != 64 && hd != 72) return false;
  return g_attn_stream_force || (hd == 72 && T > 256) || T > 288;
}

int rotary_attention_stream_launch(const float* qkv, float* o, const float* cos_tab, const float* sin_tab, int N, int T, int heads, int hd,
                                   int rot_half, hipStream_t s, float* lse, int out_split, int x3) {
  RGM_REQUIRE(N > 0 && T > 0 && T <= ATTN_STREAM_MAX_T, "attention: T=%d out of range (1..%d)", T, ATTN_STREAM_MAX_T);
  RGM_REQUIRE((2 * rot_half) % 4 == 0 && 2 * rot_half <= hd, "attention: rotary dim %d", 2 * rot_half);
  RGM_REQUIRE((long long)N * heads * ((T + SQ - 1) / SQ) <= 0x7fffffff, "attention: grid of N=%d heads=%d T=%d", N, heads, T);
  if (hd == 72) return x3 ? launch_stream<72, 1>(qkv, o, cos_tab, sin_tab, N, T, heads, rot_half, lse, out_split, s)
                          : launch_stream<72, 0>(qkv, o, cos_tab, sin_tab, N, T, heads, rot_half, lse, out_split, s);
  if (hd == 64) return x3 ? launch_stream<64, 1>(qkv, o, cos_tab, sin_tab, N, T, heads, rot_half, lse, out_split, s)
                          : launch_stream<64, 0>(qkv, o, cos_tab, sin_tab, N, T, heads, rot_half, lse, out_split, s);
  set_error("attention: head_dim %d not supported (64, 72)", hd);
  return RGM_ERR_INVALID;
}

int attn_stream_force_set(int on) {
  const int prev = g_attn_stream_force;
  g_attn_stream_force = on;
  return prev;
}

}  // namespace rgm

// 1 = the streaming attention forward for every sequence length (comparisons against the resident kernels), 0 = only where they cannot
// hold a head (default).  Returns the previous setting.
extern "C" int rgm_set_attn_stream(int on) { return rgm::attn_stream_force_set(on != 0); }
