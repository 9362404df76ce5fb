// chords.hip -- the native chord and key analyser of the chord rules (FUNC_DICT chord_progression*), on the integer roll
// (N,128,T) uint8 that rgm_rule_chord_quantise leaves on the device.  HBM-bound byte work: the roll is read once.
//
// The reference's analyser is music21 code (piano_roll_to_chord.py:307-359: chordify, Krumhansl-Schmuckler key, Roman numerals); this
// is NOT a restatement of it but an analyser with its own written definition (docs/rounds/chords.md, include/rgm.h) -- agreement with
// music21 has not been measured.
//
//   launch 1, one workgroup per (window, sample): column masks of the 88 piano pitches, the window's pitch-class counts, the run
//             boundaries, the longest sounding run (earliest on a tie) and the root of its pitch set;
//   launch 2, one wave per sample: the counts added in window order (+ the columns behind the last whole window), the 24 Pearson
//             correlations in float64 (fixed order, no FMA contraction: the host analyser does the same IEEE operations), the first
//             maximum, and the scale degree of every window's root.
// No atomics: every partial result has one owner, so the answer is bitwise repeatable and a sample's answer does not depend on N or
// on its position in the batch.
#include "common.h"

#pragma clang fp contract(off)

namespace rgm {
namespace chords {
constexpr int MIN_PIANO = 21, MAX_PIANO = 108, N_LO = 64;      // mask word lo: pitches 21..84, hi: pitches 85..108 (24 bits)
constexpr int THREADS = 256, MAX_WC = 1024;

// bits of the lo / hi word whose pitch has class c
constexpr uint64_t class_lo(int c) {
  uint64_t m = 0;
  for (int i = 0; i < N_LO; ++i)
    if ((MIN_PIANO + i) % 12 == c) m |= 1ull << i;
  return m;
}
constexpr uint32_t class_hi(int c) {
  uint32_t m = 0;
  for (int i = 0; MIN_PIANO + N_LO + i <= MAX_PIANO; ++i)
    if ((MIN_PIANO + N_LO + i) % 12 == c) m |= 1u << i;
  return m;
}
template <int C> struct ClassMask {
  static constexpr uint64_t lo = class_lo(C);
  static constexpr uint32_t hi = class_hi(C);
};

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// root of a sounding column mask: best score over the members of its pitch-class set, ties to the class nearest above the bass
__device__ __forceinline__ int root_of(uint64_t lo, uint32_t hi) {
  unsigned S = 0;
  static_for<0, 12>([&](auto c) {
    if ((lo & ClassMask<decltype(c)::value>::lo) | (uint64_t)(hi & ClassMask<decltype(c)::value>::hi)) S |= 1u << decltype(c)::value;
  });
  const int lowest = lo ? MIN_PIANO + __builtin_ctzll(lo) : MIN_PIANO + N_LO + __builtin_ctz(hi);
  const int bass = lowest % 12;
  int best = -1, root = bass;
  for (int k = 0; k < 12; ++k) {
    const int r = (bass + k) % 12;
    if (!((S >> r) & 1u)) continue;
    auto has = [&](int d) { return (int)((S >> ((r + d) % 12)) & 1u); };
    const int s = 8 * has(7) + 4 * (has(4) | has(3)) + 3 * has(6) + 2 * (has(10) | has(11));
    if (s > best) { best = s; root = r; }
  }
  return root;
}

// grid (W + (T % Wc != 0), N), block 256.  Window w < W: columns [w Wc, (w + 1) Wc) -> counts + root; block W: the columns behind the
// last whole window -> counts only.  counts (N, gridDim.x, 12) int32, roots (N, W) int32 (-1: no sounding column).
__global__ __launch_bounds__(THREADS) void window_kernel(const uint8_t* __restrict__ q, int T, int Wc, int W,
                                                         int* __restrict__ counts, int* __restrict__ roots) {
  __shared__ uint64_t m_lo[MAX_WC];
  __shared__ uint32_t m_hi[MAX_WC];
  __shared__ uint64_t starts[MAX_WC / 64];            // bit t: column t begins a run (columns >= ncol: set, they end the last run)
  __shared__ int red[THREADS / 64][13];
  const int w = blockIdx.x, n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t0 = w * Wc;
  const int ncol = w < W ? Wc : T - W * Wc;           // <= MAX_WC
  const uint8_t* base = q + (long long)n * 128 * T + t0;

  int cnt[12];
#pragma unroll
  for (int c = 0; c < 12; ++c) cnt[c] = 0;
  for (int t = tid; t < ncol; t += THREADS) {          // a wave reads 64 consecutive bytes of one pitch row per load
    uint64_t lo = 0;
    uint32_t hi = 0;
#pragma unroll 8
    for (int i = 0; i < N_LO; ++i) lo |= (uint64_t)(base[(long long)(MIN_PIANO + i) * T + t] > 0) << i;
#pragma unroll 8
    for (int i = 0; MIN_PIANO + N_LO + i <= MAX_PIANO; ++i) hi |= (uint32_t)(base[(long long)(MIN_PIANO + N_LO + i) * T + t] > 0) << i;
    m_lo[t] = lo;
    m_hi[t] = hi;
    static_for<0, 12>([&](auto c) {
      cnt[decltype(c)::value] += __popcll(lo & ClassMask<decltype(c)::value>::lo) + __popc(hi & ClassMask<decltype(c)::value>::hi);
    });
  }
#pragma unroll
  for (int c = 0; c < 12; ++c) {
    const int s = wave_sum_i(cnt[c]);
    if (lane == 0) red[wave][c] = s;
  }
  __syncthreads();                                     // masks and the waves' counts are in LDS
  if (tid < 12) counts[((long long)n * gridDim.x + w) * 12 + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
  if (w >= W) return;                                  // whole block: the leftover columns have no chord

  // run starts, one ballot word per 64 columns (uniform trip count: every lane votes)
  for (int tb = 0; tb < MAX_WC; tb += THREADS) {
    const int t = tb + tid;
    bool st = true;
    if (t > 0 && t < ncol) st = m_lo[t] != m_lo[t - 1] || m_hi[t] != m_hi[t - 1];
    const uint64_t word = __ballot(st);
    if (lane == 0) starts[t >> 6] = word;
  }
  __syncthreads();
  // every sounding run start finds its end (the next start) and bids length * 1024 + (1023 - start): the maximum is the longest run,
  // the earliest among equals
  int bid = 0;
  for (int t = tid; t < ncol; t += THREADS) {
    if (!((starts[t >> 6] >> (t & 63)) & 1ull) || (m_lo[t] == 0 && m_hi[t] == 0)) continue;
    int end = ncol;
    const int u = t + 1;                               // first candidate column of the next run
    if (u < MAX_WC) {
      int wd = u >> 6;
      uint64_t bits = starts[wd] & (~0ull << (u & 63));
      while (bits == 0 && ++wd < MAX_WC / 64) bits = starts[wd];
      if (bits) end = min(ncol, wd * 64 + __builtin_ctzll(bits));
    }
    bid = max(bid, (end - t) * MAX_WC + (MAX_WC - 1 - t));
  }
  bid = wave_max_i(bid);
  if (lane == 0) red[wave][12] = bid;
  __syncthreads();
  if (tid == 0) {
    const int b = max(max(red[0][12], red[1][12]), max(red[2][12], red[3][12]));
    int root = -1;
    if (b > 0) {
      const int t = MAX_WC - 1 - (b & (MAX_WC - 1));
      root = root_of(m_lo[t], m_hi[t]);
    }
    roots[(long long)n * W + w] = root;
  }
}

__constant__ int DEG[12] = {1, 2, 2, 3, 3, 4, 4, 5, 6, 6, 7, 7};

// grid N, block 64 (one wave per sample).  nblk = window blocks per sample in `counts`.
__global__ __launch_bounds__(64) void key_kernel(const int* __restrict__ counts, const int* __restrict__ roots, int nblk, int W,
                                                 const double* __restrict__ profile, const int* __restrict__ given, int analyse,
                                                 int64_t* __restrict__ chords, int* __restrict__ key_out, double* __restrict__ coef_out) {
  __shared__ double D[12];
  __shared__ double r[24];
  __shared__ int key_sh;
  const int n = blockIdx.x, lane = threadIdx.x;
  int key = -1;
  if (analyse) {
    if (lane < 12) {
      long long s = 0;
      for (int b = 0; b < nblk; ++b) s += counts[((long long)n * nblk + b) * 12 + lane];
      D[lane] = (double)s;
    }
    __syncthreads();
    double sxx = 0.0;
    {
      double sx = 0.0;
      for (int c = 0; c < 12; ++c) sx += D[c];
      const double mx = sx / 12.0;
      for (int c = 0; c < 12; ++c) sxx += (D[c] - mx) * (D[c] - mx);
      if (lane < 24) {
        const double* P = profile + (lane / 12) * 12;
        const int tonic = lane % 12;
        double sy = 0.0;
        for (int c = 0; c < 12; ++c) sy += P[(c - tonic + 12) % 12];
        const double my = sy / 12.0;
        double sxy = 0.0, syy = 0.0;
        for (int c = 0; c < 12; ++c) {
          const double dx = D[c] - mx, dy = P[(c - tonic + 12) % 12] - my;
          sxy += dx * dy;
          syy += dy * dy;
        }
        r[lane] = sxx == 0.0 ? 0.0 : sxy / sqrt(sxx * syy);
      }
    }
    __syncthreads();
    if (lane == 0) {
      int k = -1;
      if (sxx != 0.0) {
        k = 0;
        for (int j = 1; j < 24; ++j)
          if (r[j] > r[k]) k = j;
      }
      key_sh = k;
      key_out[n] = k;
      coef_out[n] = k < 0 ? 0.0 : r[k];
    }
    __syncthreads();
    key = key_sh;
  } else if (lane == 0) {
    key_out[n] = -1;
    coef_out[n] = 0.0;
  }
  const int g = given ? given[n] : -1;
  const bool none = analyse ? key < 0 : g < 0;
  const int tonic = g >= 0 ? g % 12 : (key >= 0 ? key % 12 : 0);
  for (int w = lane; w < W; w += 64) {
    const int root = roots[(long long)n * W + w];
    chords[(long long)n * W + w] = (none || root < 0) ? 0 : DEG[(root - tonic + 12) % 12];
  }
}
}  // namespace chords
}  // namespace rgm

using namespace rgm;

// window blocks per sample (the whole windows + one for the columns behind them) x 12 int32 counts
static size_t chords_workspace_bytes(int N, int T, int Wc) { return (size_t)N * (size_t)(T / Wc + 1) * 12 * sizeof(int); }

extern "C" int rgm_rule_chords(const uint8_t* q, int N, int T, int Wc, const double* profile, const int32_t* given_tonic,
                               int analyse_key, int64_t* chords_out, int32_t* roots_out, int32_t* key_out, double* coef_out,
                               void* ws, size_t ws_bytes, void* stream) {
  RGM_REQUIRE(q && profile && key_out && coef_out && N > 0 && T > 0, "rule_chords: bad arguments");
  RGM_REQUIRE(Wc >= 1 && Wc <= chords::MAX_WC, "rule_chords: window of %d columns (1 .. %d)", Wc, chords::MAX_WC);
  RGM_REQUIRE(N <= 65535, "rule_chords: N = %d (at most 65535 samples per call)", N);
  RGM_REQUIRE(analyse_key || given_tonic, "rule_chords: without key analysis a given tonic is needed");
  const int W = T / Wc;
  const int nblk = W + (T % Wc != 0 ? 1 : 0);
  RGM_REQUIRE(W == 0 || (chords_out && roots_out), "rule_chords: chords / roots outputs missing");
  RGM_REQUIRE(ws && ws_bytes >= chords_workspace_bytes(N, T, Wc), "rule_chords: workspace of %zu bytes, %zu needed", ws_bytes,
              chords_workspace_bytes(N, T, Wc));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(chords::window_kernel, dim3(nblk, N), dim3(chords::THREADS), 0, s, q, T, Wc, W, (int*)ws, roots_out);
  RGM_LAUNCH_CHECK();
  hipLaunchKernelGGL(chords::key_kernel, dim3(N), dim3(64), 0, s, (const int*)ws, roots_out, nblk, W, profile, given_tonic,
                     analyse_key ? 1 : 0, chords_out, key_out, coef_out);
  RGM_LAUNCH_CHECK();
  return RGM_OK;
}
