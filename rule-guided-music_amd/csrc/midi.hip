// midi.hip -- a uint8 piano roll on the device becomes a finished Standard MIDI File: the notes and sustain-pedal events of the reference's
// piano_roll_to_pretty_midi (music_rule_guidance/piano_roll_to_chord.py:167-275), the message order of its pretty_midi fork's write()
// (pretty_midi/pretty_midi.py:1341-1520) and the bytes of SMF 1.0, format 1.  The host writer (SimpleMIDI.messages / write) is the oracle:
// byte equality.  Definition, quirks and measurements: docs/rounds/midi.md, include/rgm.h.
//
//   rgm_midi_measure
//     launch 1, one workgroup per sample: the background maximum (rows 0..20) and the pedal value of every column (rows 21..108, floor mean);
//     launch 2, one wave per (pitch row, sample): walks the row 64 columns at a time carrying the run state and the run's first velocity;
//               leaves three bit rows -- a note starts / a note of non-zero length ends / a zero-length note sits in this column -- the
//               velocity of every start and the row's note count;
//     launch 3, one workgroup per sample: per column the message count (popcounts down the 128 rows of a 64-column tile held in LDS), the
//               tick of the last message before it (a running maximum), its byte count, and the exclusive scans that give every column its
//               own place in the track, in the CC array, and every row its place in the note array; writes the four sizes of the sample.
//   rgm_midi_emit
//     launch 4, one thread per column: writes the column's messages at the column's offset, its CC row, and (one thread per sample) the
//               file header, the tempo track, the track header with its length, the program change and the end-of-track;
//     launch 5, one wave per (pitch row, sample): the note rows (pitch, velocity, start column, end column).
//
// Order inside a track: the column order is the tick order because the tick table rises by at least 2 per column (checked on the host before
// any launch); inside a column the writer's key (class, data) puts the CC first, then the notes by pitch, an off (velocity 0) before the
// re-strike of its pitch; the extra off of a zero-length note, one tick later, falls strictly before the next column.
// Delta times are 1 to 3 VLQ bytes: 4 would need a gap of 2^21 ticks, and a table whose last entry reaches 2^21 is refused -- at fs = 100 column
// 32768 is tick 144179.  No atomics, no floating point: every count has one owner and every offset comes from a scan, so the result repeats
// bit for bit and a sample's bytes depend neither on N nor on its row.  The roll is read-only; all stores are ordinary vector / byte stores.
#include "roll_bits.h"

namespace rgm {
namespace midi {
using rollbits::MAX_T;
using rollbits::n_words;
using rollbits::top_bit;
constexpr int HEAD_THREADS = 1024, COL_THREADS = 256, COL_WORDS = COL_THREADS / 64;
constexpr int FILE_FIXED = 56;                          // MThd 14 | tempo track 8 + 19 | MTrk 8 | program change 3 | end of track 4
constexpr int EVENTS_AT = 52;                           // first byte behind the program change
constexpr int MAX_TICK = 1 << 21;

struct Head {                                           // per sample
  int background, n_notes, n_ccs, n_events, ev_bytes, pad[3];
};

// workspace: ticks[nc] | per sample: Head | row_off[128] | bits[128][3][nw] | off[nc] delta[nc] cc_idx[nc] | ped[nc] | vel[128][nc]
// nw words of 64 columns 0..T, nc = 64 nw
__host__ __device__ inline size_t ticks_bytes(int T) { return (size_t)n_words(T) * 64 * 4; }
__host__ __device__ inline size_t sample_bytes(int T) {
  const size_t nw = n_words(T), nc = nw * 64;
  return sizeof(Head) + 128 * 4 + 128 * 3 * nw * 8 + 3 * nc * 4 + nc + 128 * nc;
}
struct View {
  Head* head;
  int *row_off, *off, *delta, *cc_idx;
  uint64_t* bits;
  uint8_t *ped, *vel;
};
__device__ __forceinline__ View view(void* ws, int n, int T) {
  const size_t nw = n_words(T), nc = nw * 64;
  char* b = (char*)ws + ticks_bytes(T) + (size_t)n * sample_bytes(T);
  View v;
  v.head = (Head*)b;
  v.row_off = (int*)(b + sizeof(Head));
  v.bits = (uint64_t*)(v.row_off + 128);
  v.off = (int*)(v.bits + 128 * 3 * nw);
  v.delta = v.off + nc;
  v.cc_idx = v.delta + nc;
  v.ped = (uint8_t*)(v.cc_idx + nc);
  v.vel = v.ped + nc;
  return v;
}

__device__ __forceinline__ int vlq_len(int d) { return d < 128 ? 1 : d < 16384 ? 2 : 3; }
__device__ __forceinline__ int cc_value(int v) { return v < 16 ? 0 : v > 112 ? 127 : v; }

// grid N, block 1024
__global__ __launch_bounds__(HEAD_THREADS) void head_kernel(const uint8_t* __restrict__ roll, long long sn, long long sc, long long sp, long long st,
                                                            int C, int T, void* ws) {
  __shared__ int red[HEAD_THREADS / 64];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int nc = n_words(T) * 64;
  const uint8_t* vel = roll + (long long)n * sn;
  const uint8_t* ped = vel + (long long)(C - 1) * sc;
  const View v = view(ws, n, T);
  int bg = 0;
  for (int t = tid; t < nc; t += HEAD_THREADS) {
    int sum = 0;
    if (t < T) sum = rollbits::column_levels(vel, ped, sp, st, C, t, bg);
    v.ped[t] = (uint8_t)(sum / (rollbits::MAX_PIANO - rollbits::MIN_PIANO + 1));        // at most 255
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bg = max(bg, __shfl_xor(bg, o, 64));
  if ((tid & 63) == 0) red[tid >> 6] = bg;
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < HEAD_THREADS / 64; ++i) bg = max(bg, red[i]);
    v.head->background = bg;
  }
}

// grid (128, N), block 64: one wave walks pitch row p of sample n.
__global__ __launch_bounds__(64) void row_kernel(const uint8_t* __restrict__ roll, long long sn, long long sc, long long sp, long long st, int C,
                                                 int T, int first_column_onsets, void* ws) {
  const int p = blockIdx.x, n = blockIdx.y, lane = threadIdx.x;
  const int nw = n_words(T), nc = nw * 64;
  const View v = view(ws, n, T);
  const uint8_t* vel = roll + (long long)n * sn + (long long)p * sp;
  const uint8_t* ons = vel + sc;
  const int bg = v.head->background;
  const uint64_t le = ~0ull >> (63 - lane), lt = le >> 1;            // bits <= lane, bits < lane
  uint64_t* bits = v.bits + (size_t)p * 3 * nw;
  uint8_t* start_vel = v.vel + (size_t)p * nc;

  int prev_active = 0, carry_noted = 0, carry_vel = 0, count = 0;
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
    const uint64_t Rs = A & ~before, Re = ~A & before;  // a run's first column, the column just behind a run (column T included)
    const uint64_t S = C == 3 ? (__ballot(o != 0) & (A | Re)) : Rs;   // note starts: the onsets of [s, e], or the run's first column
    const uint64_t rsm = Rs & le;
    const int rs = rsm ? top_bit(rsm) : -1;             // where this column's run began, -1: before this word
    const bool noted = rs >= 0 ? ((S & le) >> rs) != 0 : ((S & le) != 0 || carry_noted);     // a start in the run up to here
    const bool noted_before = rs >= 0 ? ((S & lt) >> rs) != 0 : ((S & lt) != 0 || carry_noted);
    const int first_vel = __shfl(x, max(rs, 0), 64);
    const int run_vel = rs >= 0 ? first_vel : carry_vel;
    const bool is_s = (S >> lane) & 1ull, is_re = (Re >> lane) & 1ull;
    const uint64_t E = __ballot((is_s || is_re) && noted_before);    // a note of the run ends where the next one starts, the last behind the run
    if (lane == 0) {
      bits[w] = S;
      bits[nw + w] = E;
      bits[2 * nw + w] = S & Re;                        // an onset one column past the run: a note (e, e)
    }
    if (is_s) start_vel[k] = (uint8_t)run_vel;
    count += __popcll(S);
    prev_active = (int)(A >> 63);
    carry_noted = prev_active && __shfl((int)noted, 63, 64);
    carry_vel = __shfl(run_vel, 63, 64);
  }
  if (lane == 0) v.row_off[p] = count;
}

// exclusive scan of one int per thread over the workgroup (sum, or maximum of non-negative values); *total: the whole workgroup's.  Two
// barriers; `part` is COL_WORDS ints of LDS that the caller does not touch in between.
template <bool MAX>
__device__ __forceinline__ int block_exclusive(int x, int* part, int* total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int inc = x;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(inc, d, 64);
    if (lane >= d) inc = MAX ? max(inc, u) : inc + u;
  }
  int exc = __shfl_up(inc, 1, 64);
  if (lane == 0) exc = 0;
  __syncthreads();
  if (lane == 63) part[wave] = inc;
  __syncthreads();
  int base = 0, all = 0;
#pragma unroll
  for (int i = 0; i < COL_WORDS; ++i) {
    const int q = part[i];
    if (i < wave) base = MAX ? max(base, q) : base + q;
    all = MAX ? max(all, q) : all + q;
  }
  *total = all;
  return MAX ? max(base, exc) : base + exc;
}

// the 64-column tiles of the three bit rows of all 128 pitches, COL_WORDS words from word w0 on; words outside the roll are empty
__device__ __forceinline__ void load_tiles(uint64_t (*W)[128][COL_WORDS], const uint64_t* __restrict__ bits, int w0, int nw) {
  for (int i = threadIdx.x; i < 128 * 3 * COL_WORDS; i += COL_THREADS) {
    const int p = i / (3 * COL_WORDS), kind = (i / COL_WORDS) % 3, j = i % COL_WORDS;
    W[kind][p][j] = w0 + j < nw ? bits[((size_t)p * 3 + kind) * nw + w0 + j] : 0ull;
  }
}

// grid N, block 256
__global__ __launch_bounds__(COL_THREADS) void column_kernel(int T, void* ws, int64_t* __restrict__ counts) {
  __shared__ uint64_t W[3][128][COL_WORDS];
  __shared__ int part[COL_WORDS];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int nw = n_words(T);
  const View v = view(ws, n, T);
  const int* ticks = (const int*)ws;
  int total;
  const int notes_before = block_exclusive<false>(tid < 128 ? v.row_off[tid] : 0, part, &total);
  const int n_notes = total;
  __syncthreads();                                      // every count is read before its place is written
  if (tid < 128) v.row_off[tid] = notes_before;
  int last_tick = 0, bytes = 0, ccs = 0, events = 0;    // of the columns before this tile
  for (int w0 = 0; w0 < nw; w0 += COL_WORDS) {
    __syncthreads();
    load_tiles(W, v.bits, w0, nw);
    __syncthreads();
    const int k = w0 * 64 + tid, j = tid >> 6, b = tid & 63;
    int s = 0, e = 0, z = 0;
#pragma unroll 8
    for (int p = 0; p < 128; ++p) {
      s += (int)((W[0][p][j] >> b) & 1ull);
      e += (int)((W[1][p][j] >> b) & 1ull);
      z += (int)((W[2][p][j] >> b) & 1ull);
    }
    const int cc = k < T && v.ped[k] != 0;
    const int cnt = cc + s + e + z;                     // no bit is set behind column T
    const int tick = k <= T ? ticks[k] : 0;
    const int before = max(last_tick, block_exclusive<true>(cnt ? tick + (z > 0) : 0, part, &total));
    last_tick = max(last_tick, total);
    const int delta = tick - before;
    const int nb = cnt ? 4 * cnt - 1 + vlq_len(delta) : 0;           // a status byte on every message; every delta but the first is 0 or 1
    const int off = bytes + block_exclusive<false>(nb, part, &total);
    bytes += total;
    const int cc_idx = ccs + block_exclusive<false>(cc, part, &total);
    ccs += total;
    block_exclusive<false>(cnt, part, &total);
    events += total;
    if (k <= T) {
      v.off[k] = off;
      v.delta[k] = delta;
      v.cc_idx[k] = cc_idx;
    }
  }
  if (tid == 0) {
    Head* h = v.head;
    h->n_notes = n_notes;
    h->n_ccs = ccs;
    h->n_events = events;
    h->ev_bytes = bytes;
    counts[n * 4 + 0] = n_notes;
    counts[n * 4 + 1] = ccs;
    counts[n * 4 + 2] = events + 5;                     // tempo, time signature, end of track | program change, end of track
    counts[n * 4 + 3] = bytes + FILE_FIXED;
  }
}

__device__ __forceinline__ uint8_t* put_vlq(uint8_t* q, int d) {
  if (d >= 16384) *q++ = (uint8_t)(0x80 | (d >> 14));
  if (d >= 128) *q++ = (uint8_t)(0x80 | ((d >> 7) & 0x7f));
  *q++ = (uint8_t)(d & 0x7f);
  return q;
}
__device__ __forceinline__ uint8_t* put_msg(uint8_t* q, int delta, int status, int a, int b) {
  q = put_vlq(q, delta);
  *q++ = (uint8_t)status;
  *q++ = (uint8_t)a;
  *q++ = (uint8_t)b;
  return q;
}
__device__ __forceinline__ void put_be32(uint8_t* q, unsigned x) {
  q[0] = (uint8_t)(x >> 24);
  q[1] = (uint8_t)(x >> 16);
  q[2] = (uint8_t)(x >> 8);
  q[3] = (uint8_t)x;
}

// grid (ceil(nw / 4), N), block 256: one thread per column.  A sample whose rows or bytes would not fit the arrays is left out whole.
__global__ __launch_bounds__(COL_THREADS) void emit_columns_kernel(int T, int program, void* ws, const int64_t* __restrict__ cc_off,
                                                                   const int64_t* __restrict__ byte_off, int32_t* __restrict__ ccs,
                                                                   long long ccs_cap, uint8_t* __restrict__ out, long long out_cap) {
  __shared__ uint64_t W[3][128][COL_WORDS];
  const int n = blockIdx.y, tid = threadIdx.x, w0 = blockIdx.x * COL_WORDS;
  const int nw = n_words(T), nc = nw * 64;
  const View v = view(ws, n, T);
  const Head h = *v.head;
  const long long co = cc_off[n], bo = byte_off[n];
  if (co < 0 || co + h.n_ccs > ccs_cap || bo < 0 || bo + h.ev_bytes + FILE_FIXED > out_cap) return;
  load_tiles(W, v.bits, w0, nw);
  __syncthreads();
  uint8_t* file = out + bo;
  if (blockIdx.x == 0 && tid == 0) {
    const uint8_t fixed[EVENTS_AT] = {'M', 'T', 'h', 'd', 0, 0, 0, 6, 0, 1, 0, 2, 0, 220,                           // format 1, 2 tracks, 220 ticks / quarter
                                      'M', 'T', 'r', 'k', 0, 0, 0, 19, 0, 0xff, 0x51, 3, 0x07, 0xa1, 0x20,          // tempo 500000
                                      0, 0xff, 0x58, 4, 4, 2, 24, 8, 1, 0xff, 0x2f, 0,                              // 4/4, end of track at delta 1
                                      'M', 'T', 'r', 'k', 0, 0, 0, 0, 0, 0xc0, 0};
    for (int i = 0; i < EVENTS_AT; ++i) file[i] = fixed[i];
    put_be32(file + 45, (unsigned)(h.ev_bytes + 7));
    file[51] = (uint8_t)(program & 0x7f);
    uint8_t* q = file + EVENTS_AT + h.ev_bytes;
    q[0] = 1;
    q[1] = 0xff;
    q[2] = 0x2f;
    q[3] = 0;
  }
  const int k = w0 * 64 + tid, j = tid >> 6, b = tid & 63;
  if (k > T) return;
  uint8_t* q = file + EVENTS_AT + v.off[k];
  int delta = v.delta[k];                               // of the column's first message; 0 behind it
  const int ped = k < T ? v.ped[k] : 0;
  if (ped) {
    const int val = cc_value(ped);
    q = put_msg(q, delta, 0xb0, 64, val);
    delta = 0;
    int32_t* row = ccs + 2 * (co + v.cc_idx[k]);
    row[0] = k;
    row[1] = val;
  }
  int zl = 0;
  for (int p = 0; p < 128; ++p) {
    if ((W[1][p][j] >> b) & 1ull) {                     // a note-off is a note-on of velocity 0: it sorts before the re-strike
      q = put_msg(q, delta, 0x90, p, 0);
      delta = 0;
    }
    if ((W[0][p][j] >> b) & 1ull) {
      q = put_msg(q, delta, 0x90, p, max(1, (int)v.vel[(size_t)p * nc + k]) & 0x7f);
      delta = 0;
    }
    zl |= (int)((W[2][p][j] >> b) & 1ull);
  }
  if (zl) {
    delta = 1;                                          // a zero-length note ends one tick after it starts
    for (int p = 0; p < 128; ++p)
      if ((W[2][p][j] >> b) & 1ull) {
        q = put_msg(q, delta, 0x90, p, 0);
        delta = 0;
      }
  }
}

// grid (128, N), block 64: the note rows of pitch p in start order.  A note ends at the next end bit behind its start, a zero-length one where
// it starts; at most one note per row is open across a word boundary.
__global__ __launch_bounds__(64) void emit_notes_kernel(int T, void* ws, const int64_t* __restrict__ note_off, int32_t* __restrict__ notes,
                                                        long long notes_cap) {
  const int p = blockIdx.x, n = blockIdx.y, lane = threadIdx.x;
  const int nw = n_words(T), nc = nw * 64;
  const View v = view(ws, n, T);
  const long long no = note_off[n];
  if (no < 0 || no + v.head->n_notes > notes_cap) return;
  const uint64_t* bits = v.bits + (size_t)p * 3 * nw;
  const uint8_t* start_vel = v.vel + (size_t)p * nc;
  const uint64_t le = ~0ull >> (63 - lane), lt = le >> 1;
  int32_t* rows = notes + 4 * (no + v.row_off[p]);
  int done = 0, open = -1;                              // notes written so far; the row index of the note still waiting for its end
  for (int w = 0; w < nw; ++w) {
    const uint64_t S = bits[w], E = bits[nw + w], Z = bits[2 * nw + w];
    if (open >= 0 && E) {
      if (lane == 0) rows[4 * open + 3] = w * 64 + __builtin_ctzll(E);
      open = -1;
    }
    const int k = w * 64 + lane;
    bool waits = false;
    if ((S >> lane) & 1ull) {
      int32_t* r = rows + 4 * (done + __popcll(S & lt));
      r[0] = p;
      r[1] = start_vel[k];
      r[2] = k;
      const uint64_t nxt = E & ~le;
      if ((Z >> lane) & 1ull) r[3] = k;
      else if (nxt) r[3] = w * 64 + __builtin_ctzll(nxt);
      else waits = true;
    }
    const uint64_t wm = __ballot(waits);
    if (wm) open = done + __popcll(S & ((1ull << top_bit(wm)) - 1ull));
    done += __popcll(S);
  }
}
}  // namespace midi
}  // namespace rgm

using namespace rgm;

extern "C" size_t rgm_midi_workspace(int N, int T) {
  if (N <= 0 || N > 65535 || T < 1 || T > midi::MAX_T) return 0;
  return midi::ticks_bytes(T) + (size_t)N * midi::sample_bytes(T);
}

static int midi_check_sizes(const char* what, int N, int T, void* ws, size_t ws_bytes) {
  RGM_REQUIRE(N > 0 && N <= 65535, "%s: N = %d (1 .. 65535 samples per call)", what, N);
  RGM_REQUIRE(T >= 1 && T <= midi::MAX_T, "%s: T = %d columns (1 .. %d)", what, T, midi::MAX_T);
  if (!ws || ws_bytes < rgm_midi_workspace(N, T)) {
    set_error("%s: workspace of %zu bytes, %zu needed", what, ws ? ws_bytes : (size_t)0, rgm_midi_workspace(N, T));
    return RGM_ERR_WORKSPACE;
  }
  RGM_REQUIRE(((uintptr_t)ws & 7) == 0, "%s: the workspace must be 8-byte aligned", what);
  return RGM_OK;
}

extern "C" int rgm_midi_measure(const uint8_t* roll, long long stride_n, long long stride_c, long long stride_p, long long stride_t, int N, int C,
                                int T, int first_column_onsets, const int32_t* ticks_host, int64_t* counts, void* ws, size_t ws_bytes,
                                void* stream) {
  RGM_REQUIRE(roll && ticks_host && counts, "midi_measure: bad arguments");
  RGM_REQUIRE(C >= 1 && C <= 3, "midi_measure: %d channels (1: velocity, 2: + pedal, 3: velocity, onset, pedal)", C);
  RGM_TRY(midi_check_sizes("midi_measure", N, T, ws, ws_bytes));
  RGM_REQUIRE(stride_n > 0 && stride_p > 0 && stride_t > 0 && (C == 1 || stride_c > 0), "midi_measure: strides must be positive byte counts");
  RGM_REQUIRE(ticks_host[0] >= 0 && ticks_host[T] < midi::MAX_TICK, "midi_measure: tick table runs from %d to %d (0 .. 2^21 - 1: deltas of 1 to 3 bytes)",
              ticks_host[0], ticks_host[T]);
  for (int k = 0; k < T; ++k)
    RGM_REQUIRE(ticks_host[k + 1] - ticks_host[k] >= 2, "midi_measure: tick table rises by %d from column %d to %d; the device path needs 2 (fs <= 220)",
                ticks_host[k + 1] - ticks_host[k], k, k + 1);
  hipStream_t s = (hipStream_t)stream;
  RGM_CHECK_HIP(hipMemcpyAsync(ws, ticks_host, (size_t)(T + 1) * 4, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(midi::head_kernel, dim3(N), dim3(midi::HEAD_THREADS), 0, s, roll, stride_n, stride_c, stride_p, stride_t, C, T, ws);
  RGM_LAUNCH_CHECK();
  hipLaunchKernelGGL(midi::row_kernel, dim3(128, N), dim3(64), 0, s, roll, stride_n, stride_c, stride_p, stride_t, C, T,
                     first_column_onsets ? 1 : 0, ws);
  RGM_LAUNCH_CHECK();
  hipLaunchKernelGGL(midi::column_kernel, dim3(N), dim3(midi::COL_THREADS), 0, s, T, ws, counts);
  RGM_LAUNCH_CHECK();
  return RGM_OK;
}

extern "C" int rgm_midi_emit(int N, int T, int program, const int64_t* note_off, const int64_t* cc_off, const int64_t* byte_off, int32_t* notes,
                             long long notes_cap, int32_t* ccs, long long ccs_cap, uint8_t* bytes, long long bytes_cap, void* ws, size_t ws_bytes,
                             void* stream) {
  RGM_REQUIRE(note_off && cc_off && byte_off && bytes, "midi_emit: bad arguments");
  RGM_REQUIRE(notes_cap >= 0 && ccs_cap >= 0 && bytes_cap >= 0 && (notes || notes_cap == 0) && (ccs || ccs_cap == 0),
              "midi_emit: an array of %lld note rows / %lld CC rows / %lld bytes needs its pointer", notes_cap, ccs_cap, bytes_cap);
  RGM_REQUIRE(program >= 0 && program <= 127, "midi_emit: program %d (0 .. 127)", program);
  RGM_TRY(midi_check_sizes("midi_emit", N, T, ws, ws_bytes));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(midi::emit_columns_kernel, dim3((midi::n_words(T) + midi::COL_WORDS - 1) / midi::COL_WORDS, N), dim3(midi::COL_THREADS), 0, s, T,
                     program, ws, cc_off, byte_off, ccs, ccs_cap, bytes, bytes_cap);
  RGM_LAUNCH_CHECK();
  hipLaunchKernelGGL(midi::emit_notes_kernel, dim3(128, N), dim3(64), 0, s, T, ws, note_off, notes, notes_cap);
  RGM_LAUNCH_CHECK();
  return RGM_OK;
}
