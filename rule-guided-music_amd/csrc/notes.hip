// notes.hip -- mgeval's note statistics (the reference's music_evaluation/mgeval/core.py `metrics`, driven by music_evaluator.py) of
// the object the reference's piano_roll_to_pretty_midi (music_rule_guidance/piano_roll_to_chord.py:167-275) builds from an integer
// roll, without a note list: per pitch row the runs, onsets and note edges are ballot words, the rebuilt roll of the fork's
// get_piano_roll(fs = 100) (pretty_midi/instrument.py:69-207) is summed column by column, and the pitch-class transition matrix comes
// from per-column start / end counts.  Definition, quirks and measurements: docs/rounds/notes.md, include/rgm.h.
//
//   launch 1, one workgroup per sample: the background maximum (rows 0..20), the pedal vector (rows 21..108, floor mean), its press /
//             release latch and the pedal-down columns of the rebuilt roll, and the columns k with int((k / 100) * 100) == k - 1;
//   launch 2, one wave per (pitch row, sample): walks the row 64 columns at a time carrying the run state, the covering note's
//             velocity and the pedal's running maximum; leaves the row's note count, velocity sum, duration sum, first / last start,
//             last end, the row sum of the rebuilt roll, and the note starts / ends as bit rows;
//   launch 3, one workgroup per sample: folds the 128 rows in row order and forms the 144 transition counts from the +-5-column
//             neighbourhood of every end column.
// Times are k / 100 in float64 exactly as the reference forms them; the comparison |end / 100 - start / 100| < 0.05 at a distance of
// five columns is evaluated, not tabulated.  No floating-point atomics: every float has one owner and a fixed summation order (lane
// partial sums, a fixed shuffle tree, rows in order), so the answer is bitwise repeatable and a sample's numbers depend neither on N nor
// on its row.  The input is read-only; everything runs on the caller's stream in the caller's workspace.
#include "roll_bits.h"

#pragma clang fp contract(off)

namespace rgm {
namespace notes {
using rollbits::MAX_PIANO;
using rollbits::MAX_T;
using rollbits::MAX_WORDS;
using rollbits::MIN_PIANO;
using rollbits::n_words;
using rollbits::top_bit;
constexpr int N_INT = 148, N_REAL = 16, TILE = 256, HALO = 5, PEDAL_THREADS = 1024;

struct RowStats {                                       // what launch 2 leaves per pitch row
  int n, vel_sum, first_start, last_start, last_end, pad;
  long long roll_sum;
  double dur_sum;
};
struct Head {                                           // what launch 1 leaves per sample
  int background, last_pedal, down_cut, pad;
};

// workspace of one sample: Head | down[nw] head[nw] shift[nw] | RowStats[128] | bits[128][3][nw]   (nw words of 64 columns 0..T)
__host__ __device__ inline size_t sample_bytes(int T) {
  return sizeof(Head) + (size_t)3 * n_words(T) * 8 + 128 * sizeof(RowStats) + (size_t)128 * 3 * n_words(T) * 8;
}
struct View {
  Head* head;
  uint64_t *down, *seg, *shift, *bits;
  RowStats* rows;
};
__device__ __forceinline__ View view(void* ws, int n, int T) {
  char* b = (char*)ws + (size_t)n * sample_bytes(T);
  const int nw = n_words(T);
  View v;
  v.head = (Head*)b;
  v.down = (uint64_t*)(b + sizeof(Head));
  v.seg = v.down + nw;
  v.shift = v.seg + nw;
  v.rows = (RowStats*)(v.shift + nw);
  v.bits = (uint64_t*)(v.rows + 128);
  return v;
}

__device__ __forceinline__ int column_of(int k) { return (int)(((double)k / 100.0) * 100.0); }   // int(fs * (k / fs)): k or k - 1

// grid N, block 1024.  Pedal value of column t: sum of the cells >= 4 of rows 21..108, floor-divided by 88; an event where it is not 0,
// pressing at >= 64 (16..112 keep their value, > 112 is 127) and releasing below.  In the words written, bit k stands for the rebuilt
// column k - 1: `down` = inside a press .. release span, `seg` = a span begins there.
__global__ __launch_bounds__(PEDAL_THREADS) void pedal_kernel(const uint8_t* __restrict__ roll, long long sn, long long sc, long long sp, long long st,
                                                    int C, int T, void* ws) {
  __shared__ uint64_t hi_w[MAX_WORDS + 3], lo_w[MAX_WORDS + 3], sh_w[MAX_WORDS + 3];
  __shared__ int red[2][PEDAL_THREADS / 64];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nw = n_words(T);
  const uint8_t* vel = roll + (long long)n * sn;
  const uint8_t* ped = vel + (long long)(C - 1) * sc;
  const View v = view(ws, n, T);
  int bg = 0, last = -1;
  for (int tb = 0; tb < nw * 64; tb += PEDAL_THREADS) {  // uniform trip count: every lane votes
    const int t = tb + tid;
    int sum = 0;
    if (t < T) sum = rollbits::column_levels(vel, ped, sp, st, C, t, bg);
    const int val = sum / (MAX_PIANO - MIN_PIANO + 1);
    if (val != 0) last = t;
    const uint64_t hi = __ballot(val >= 64), lo = __ballot(val != 0 && val < 64), sh = __ballot(column_of(t) != t);
    if (lane == 0 && (t >> 6) < nw) {
      hi_w[t >> 6] = hi;
      lo_w[t >> 6] = lo;
      sh_w[t >> 6] = sh;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    bg = max(bg, __shfl_xor(bg, o, 64));
    last = max(last, __shfl_xor(last, o, 64));
  }
  if (lane == 0) {
    red[0][wave] = bg;
    red[1][wave] = last;
  }
  __syncthreads();
  if (wave != 0) return;
  // the press / release latch, 64 columns per step: a column's state is that of the last event at or before it
  int state = 0, prev_state = 0, prev_plain = 0, last_press = -1;
  for (int w = 0; w < nw; ++w) {
    const uint64_t H = hi_w[w], L = lo_w[w], S = sh_w[w];
    const uint64_t ev = (H | L) & (~0ull >> (63 - lane));
    const int mine = ev ? (int)((H >> top_bit(ev)) & 1ull) : state;
    const uint64_t ST = __ballot(mine != 0);
    const uint64_t before = (ST << 1) | (uint64_t)prev_state;
    const uint64_t press = ST & ~before;
    const uint64_t plain = press & ~S;                  // pressed in a column that keeps its index: the span begins one bit further
    if (lane == 0) {
      v.down[w] = (S & ST) | (~S & before);             // rebuilt column k - 1 is column k where k maps to k - 1, else column k - 1
      v.seg[w] = (plain << 1) | (uint64_t)prev_plain | (press & S);
      v.shift[w] = S;
    }
    if (press) last_press = w * 64 + top_bit(press);
    state = prev_state = (int)(ST >> 63);
    prev_plain = (int)(plain >> 63);
  }
  if (lane == 0) {
    Head h;
    h.background = 0;
    h.last_pedal = -1;
    for (int i = 0; i < PEDAL_THREADS / 64; ++i) {
      h.background = max(h.background, red[0][i]);
      h.last_pedal = max(h.last_pedal, red[1][i]);
    }
    h.down_cut = state ? column_of(last_press) + 1 : 0x7fffffff;     // a pedal still down at the end changes nothing
    h.pad = 0;
    *v.head = h;
  }
}

// grid (128, N), block 64: one wave walks pitch row p of sample n.
__global__ __launch_bounds__(64) void row_kernel(const uint8_t* __restrict__ roll, long long sn, long long sc, long long sp, long long st,
                                                 int C, int T, int first_column_onsets, void* ws) {
  const int p = blockIdx.x, n = blockIdx.y, lane = threadIdx.x;
  const int nw = n_words(T);
  const View v = view(ws, n, T);
  const uint8_t* vel = roll + (long long)n * sn + (long long)p * sp;
  const uint8_t* ons = vel + sc;
  const int bg = v.head->background, down_cut = v.head->down_cut;
  const uint64_t le = ~0ull >> (63 - lane), lt = le >> 1;            // bits <= lane, bits < lane
  uint64_t* bits = v.bits + (size_t)p * 3 * nw;

  int prev_active = 0, carry_noted = 0, carry_vel = 0, open_start = -1, prev_cover = 0, carry_max = 0;
  int count = 0, first_start = -1, last_start = -1, last_end = -1;
  int vel_sum = 0, roll_sum = 0;                        // per lane: at most 513 columns of at most 127
  double dur = 0.0;
  for (int w = 0; w < nw; ++w) {
    const int k = w * 64 + lane;
    int x = 0, o = 0;
    if (k < T) {
      x = vel[k * st];
      if (C == 3) o = ons[k * st] >= 64 || (first_column_onsets && k == 0 && x != 0);
      x = x > bg ? x : 0;
    }
    const uint64_t A = __ballot(x != 0);
    const uint64_t before = (A << 1) | (uint64_t)prev_active;
    const uint64_t Rs = A & ~before, Re = ~A & before;  // a run's first column, the column just behind a run
    const uint64_t S = C == 3 ? (__ballot(o != 0) & (A | Re)) : Rs;   // note starts
    const uint64_t rsm = Rs & le;
    const int rs = rsm ? top_bit(rsm) : -1;             // where this column's run began, -1: before this word
    const bool noted = rs >= 0 ? ((S & le) >> rs) != 0 : ((S & le) != 0 || carry_noted);     // a start in the run up to here
    const bool noted_before = rs >= 0 ? ((S & lt) >> rs) != 0 : ((S & lt) != 0 || carry_noted);
    const int start_vel = __shfl(x, max(rs, 0), 64);
    const int run_vel = rs >= 0 ? start_vel : carry_vel;
    const bool is_a = (A >> lane) & 1ull, is_s = (S >> lane) & 1ull, is_re = (Re >> lane) & 1ull;
    const int cover = is_a && noted ? run_vel : 0;      // velocity of the note over this column
    const uint64_t EA = __ballot(is_s && noted_before); // a note ends where the next one of its run starts ...
    const uint64_t EB = __ballot(is_re && noted);       // ... and the last one behind the run
    if (lane == 0) {
      bits[w] = S;
      bits[nw + w] = EA;
      bits[2 * nw + w] = EB;
    }
    count += __popcll(S);
    if (S) {
      if (first_start < 0) first_start = w * 64 + __builtin_ctzll(S);
      last_start = w * 64 + top_bit(S);
    }
    if (EB) last_end = w * 64 + top_bit(EB);
    // durations: a note ends at the next start or the next run end, whichever comes first
    const uint64_t edges = S | Re;
    if (open_start >= 0 && edges) {
      if (lane == 0) dur += (double)(w * 64 + __builtin_ctzll(edges)) / 100.0 - (double)open_start / 100.0;
      open_start = -1;
    }
    bool open = false;
    if (is_s) {
      vel_sum += run_vel;
      const uint64_t nxt = (S & ~le) | (Re & ~lt);
      if (nxt) dur += (double)(w * 64 + __builtin_ctzll(nxt)) / 100.0 - (double)k / 100.0;
      else open = true;
    }
    const uint64_t open_m = __ballot(open);
    if (open_m) open_start = w * 64 + __builtin_ctzll(open_m);
    // the rebuilt roll: bit k stands for its column k - 1, which shows column k where k maps to k - 1 and column k - 1 otherwise
    const uint64_t SH = v.shift[w], SEG = v.seg[w];
    uint64_t DOWN = v.down[w];
    if (w * 64 + 63 >= down_cut) DOWN &= w * 64 >= down_cut ? 0ull : ~(~0ull << (down_cut - w * 64));
    int up = __shfl_up(cover, 1, 64);
    if (lane == 0) up = prev_cover;
    int r = ((SH >> lane) & 1ull) ? cover : up;
    if (k == 0) r = 0;
    int f = (int)(((SEG | ~DOWN) >> lane) & 1ull);      // a pedal span begins here, or no pedal: the running maximum starts afresh
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int ru = __shfl_up(r, d, 64), fu = __shfl_up(f, d, 64);
      if (lane >= d && !f) {
        r = max(r, ru);
        f = fu;
      }
    }
    if (!f) r = max(r, carry_max);
    roll_sum += r;
    carry_max = __shfl(r, 63, 64);
    prev_cover = __shfl(cover, 63, 64);
    prev_active = (int)(A >> 63);
    carry_noted = prev_active && __shfl((int)noted, 63, 64);
    carry_vel = __shfl(run_vel, 63, 64);
  }
  long long rsum = roll_sum;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    vel_sum += __shfl_xor(vel_sum, o, 64);
    rsum += __shfl_xor(rsum, o, 64);
    dur += __shfl_xor(dur, o, 64);                      // a fixed tree: the same sum on every launch
  }
  if (lane == 0) {
    RowStats s;
    s.n = count;
    s.vel_sum = vel_sum;
    s.first_start = first_start;
    s.last_start = last_start;
    s.last_end = last_end;
    s.pad = 0;
    s.roll_sum = rsum;
    s.dur_sum = dur;
    v.rows[p] = s;
  }
}

// grid N, block 256
__global__ __launch_bounds__(TILE) void fold_kernel(int T, void* ws, int64_t* __restrict__ out_int, double* __restrict__ out_real) {
  __shared__ unsigned long long M[144];
  __shared__ uint8_t starts[12][TILE + 2 * HALO + 2];
  __shared__ int n_sh;
  __shared__ RowStats rows[128];
  __shared__ uint64_t wS[128][6], wE[128][8];           // a tile's words: starts with one word on either side, the two kinds of ends
  const int n = blockIdx.x, tid = threadIdx.x;
  const int nw = n_words(T);
  const View v = view(ws, n, T);
  if (tid < 128) rows[tid] = v.rows[tid];
  __syncthreads();
  int64_t* oi = out_int + (size_t)n * N_INT;
  double* orl = out_real + (size_t)n * N_REAL;
  if (tid < 144) M[tid] = 0ull;
  if (tid == 0) {
    long long notes = 0, vel_sum = 0, total = 0, cls[12];
    int first = 0x7fffffff, last_start = -1, last = v.head->last_pedal, used = 0, lo = -1, hi = -1;
    double dur = 0.0;
    for (int c = 0; c < 12; ++c) cls[c] = 0;
    for (int p = 0; p < 128; ++p) {
      const RowStats s = rows[p];
      notes += s.n;
      vel_sum += s.vel_sum;
      dur += s.dur_sum;
      if (s.n > 0) {
        first = min(first, s.first_start);
        last_start = max(last_start, s.last_start);
        last = max(last, s.last_end);
      }
      cls[p % 12] += s.roll_sum;
      total += s.roll_sum;
      if (s.roll_sum > 0) {
        ++used;
        if (lo < 0) lo = p;
        hi = p;
      }
    }
    const double end_time = last > 0 ? (double)last / 100.0 : 0.0;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    oi[0] = notes;
    oi[1] = used;
    oi[2] = used ? hi - lo : 0;
    oi[3] = notes ? vel_sum / notes : 0;
    orl[0] = end_time;
    orl[1] = notes >= 2 ? ((double)last_start / 100.0 - (double)first / 100.0) / (double)(notes - 1) : nan;
    orl[2] = notes ? dur / (double)notes : 0.0;
    orl[3] = end_time > 0.0 ? (double)notes / end_time : 0.0;
    for (int c = 0; c < 12; ++c) orl[4 + c] = total ? (double)cls[c] / (double)total : nan;
    n_sh = (int)min(notes, 2ll);
  }
  __syncthreads();
  if (n_sh > 1) {                                       // the fork answers zeros for a single note
    const uint64_t* bits = v.bits;
    for (int k0 = 0; k0 <= T; k0 += TILE) {
      for (int i = tid; i < 128 * 14; i += TILE) {                    // the tile's words, coalesced; words outside the roll are empty
        const int p = i / 14, j = i % 14;
        const int kind = j < 6 ? 0 : 1 + (j - 6) / 4;
        const int w = k0 / 64 + (j < 6 ? j - 1 : (j - 6) % 4);
        const uint64_t word = w >= 0 && w < nw ? bits[((size_t)p * 3 + kind) * nw + w] : 0ull;
        if (j < 6) wS[p][j] = word;
        else wE[p][j - 6] = word;
      }
      __syncthreads();
      for (int i = tid; i < TILE + 2 * HALO; i += TILE) {             // starts per pitch class of the columns k0 - 5 .. k0 + 260
        const int c = k0 - HALO + i;
        int cnt[12];
#pragma unroll
        for (int b = 0; b < 12; ++b) cnt[b] = 0;
        if (c >= 0 && c <= T) {
#pragma unroll
          for (int b = 0; b < 12; ++b)
            for (int p = b; p < 128; p += 12) cnt[b] += (int)((wS[p][(c >> 6) - k0 / 64 + 1] >> (c & 63)) & 1ull);
        }
#pragma unroll
        for (int b = 0; b < 12; ++b) starts[b][i] = (uint8_t)cnt[b];
      }
      __syncthreads();
      const int k = k0 + tid;
      if (k <= T) {
        int ends[12], any = 0;
#pragma unroll
        for (int a = 0; a < 12; ++a) {
          ends[a] = 0;
          for (int p = a; p < 128; p += 12)
            ends[a] += (int)((wE[p][tid >> 6] >> (k & 63)) & 1ull) + (int)((wE[p][4 + (tid >> 6)] >> (k & 63)) & 1ull);
          any |= ends[a];
        }
        if (any) {
          const double te = (double)k / 100.0;
          const bool below = fabs(te - (double)(k - HALO) / 100.0) < 0.05, above = fabs(te - (double)(k + HALO) / 100.0) < 0.05;
#pragma unroll
          for (int b = 0; b < 12; ++b) {
            int near = (below ? starts[b][tid] : 0) + (above ? starts[b][tid + 2 * HALO] : 0);
            for (int d = 1; d < 2 * HALO; ++d) near += starts[b][tid + d];
            if (near) {
#pragma unroll
              for (int a = 0; a < 12; ++a)
                if (ends[a]) atomicAdd(&M[a * 12 + b], (unsigned long long)(ends[a] * near));   // integer adds: any order gives the same sum
            }
          }
        }
      }
      __syncthreads();
    }
  }
  __syncthreads();
  if (tid < 144) oi[4 + tid] = (int64_t)M[tid];
}

// grid-stride over the cells
__global__ __launch_bounds__(256) void to_u8_kernel(const float* __restrict__ x, uint8_t* __restrict__ out, size_t count) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) {
    const float y = x[i];
    out[i] = (uint8_t)fminf(fmaxf((y + 1.0f) * 63.5f + 0.0009765625f, 0.0f), 127.0f);     // fmaxf(NaN, 0) = 0
  }
}
}  // namespace notes
}  // namespace rgm

using namespace rgm;

extern "C" size_t rgm_note_stats_workspace(int N, int T) {
  if (N <= 0 || T < 1 || T > notes::MAX_T) return 0;
  return (size_t)N * notes::sample_bytes(T);
}

extern "C" int rgm_note_stats(const uint8_t* roll, long long stride_n, long long stride_c, long long stride_p, long long stride_t, int N, int C,
                              int T, int first_column_onsets, int64_t* out_int, double* out_real, void* ws, size_t ws_bytes, void* stream) {
  RGM_REQUIRE(roll && out_int && out_real, "note_stats: bad arguments");
  RGM_REQUIRE(N > 0 && N <= 65535, "note_stats: N = %d (1 .. 65535 samples per call)", N);
  RGM_REQUIRE(C >= 1 && C <= 3, "note_stats: %d channels (1: velocity, 2: + pedal, 3: velocity, onset, pedal)", C);
  RGM_REQUIRE(T >= 1 && T <= notes::MAX_T, "note_stats: T = %d columns (1 .. %d)", T, notes::MAX_T);
  RGM_REQUIRE(stride_n > 0 && stride_p > 0 && stride_t > 0 && (C == 1 || stride_c > 0), "note_stats: strides must be positive byte counts");
  RGM_REQUIRE(ws && ws_bytes >= rgm_note_stats_workspace(N, T), "note_stats: workspace of %zu bytes, %zu needed", ws_bytes,
              rgm_note_stats_workspace(N, T));
  RGM_REQUIRE(((uintptr_t)ws & 7) == 0, "note_stats: the workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(notes::pedal_kernel, dim3(N), dim3(notes::PEDAL_THREADS), 0, s, roll, stride_n, stride_c, stride_p, stride_t, C, T, ws);
  RGM_LAUNCH_CHECK();
  hipLaunchKernelGGL(notes::row_kernel, dim3(128, N), dim3(64), 0, s, roll, stride_n, stride_c, stride_p, stride_t, C, T,
                     first_column_onsets ? 1 : 0, ws);
  RGM_LAUNCH_CHECK();
  hipLaunchKernelGGL(notes::fold_kernel, dim3(N), dim3(notes::TILE), 0, s, T, ws, out_int, out_real);
  RGM_LAUNCH_CHECK();
  return RGM_OK;
}

extern "C" int rgm_roll_to_u8(const float* roll, uint8_t* out, int N, int C, int T, void* stream) {
  RGM_REQUIRE(roll && out && N > 0 && C >= 1 && T >= 1, "roll_to_u8: bad arguments");
  const size_t count = (size_t)N * C * 128 * T;
  const unsigned blocks = (unsigned)std::min<size_t>((count + 1023) / 1024, 65535);
  hipLaunchKernelGGL(notes::to_u8_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, roll, out, count);
  RGM_LAUNCH_CHECK();
  return RGM_OK;
}
