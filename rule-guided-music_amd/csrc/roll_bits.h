// roll_bits.h -- what the kernels that walk an integer piano roll column by column share (notes.hip, midi.hip): the piano range, the
// limits of a roll, and the two per-column levels of the reference's piano_roll_to_pretty_midi (music_rule_guidance/piano_roll_to_chord.py:
// 167-275) that every pitch row depends on -- the background maximum and the pedal sum.
#pragma once
#include "common.h"

namespace rgm {
namespace rollbits {
constexpr int MIN_PIANO = 21, MAX_PIANO = 108, MAX_T = 32768, MAX_WORDS = MAX_T / 64 + 1;

__host__ __device__ inline int n_words(int T) { return T / 64 + 1; }                    // words of 64 columns 0..T
__device__ __forceinline__ int top_bit(uint64_t m) { return 63 - __builtin_clzll(m); }

// Column t of one sample (vel, ped: its velocity and pedal channels; sp, st: byte strides of a pitch and a column): raises bg to the largest
// velocity of rows 0..20 and returns the sum of the pedal cells >= 4 of rows 21..108 (0 without a pedal channel, C < 2).  The pedal value of
// the column is that sum floor-divided by 88.
__device__ __forceinline__ int column_levels(const uint8_t* vel, const uint8_t* ped, long long sp, long long st, int C,
                                             int t, int& bg) {
  int sum = 0;
#pragma unroll 7
  for (int p = 0; p < MIN_PIANO; ++p) bg = max(bg, (int)vel[p * sp + t * st]);
  if (C >= 2) {
#pragma unroll 8
    for (int p = MIN_PIANO; p <= MAX_PIANO; ++p) {
      const int x = ped[p * sp + t * st];
      sum += x >= 4 ? x : 0;
    }
  }
  return sum;
}
}  // namespace rollbits
}  // namespace rgm
