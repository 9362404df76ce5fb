// Standard MIDI Files read on the device: events, seconds and piano rolls (docs/rounds/midi_read.md).
//
// The definition is the host reader: SimpleMIDI._read followed by midi_to_full_piano_roll (music_rule_guidance/piano_roll_to_chord.py),
// mirrored step for step -- the header with its length honoured, the MTrk walk, the per-track byte loop (deltas of any length, FF 51 03 as the
// only meta that is kept, F0 / F7 with a variable-length size, running status with a status of 0 before any status byte and the other Fx bytes
// taken as two-argument statuses, one argument for Cx / Dx), the tempo map sorted by (tick, value) with a sequential float64 sum, seconds() with
// the host's operations in the host's order, one instrument per (track, channel) that has a note or a control change, notes matched first in
// first out per (track, channel, pitch) -- and the roll builder's columns, velocity sums, onsets and sequential pedal loop.
//
//   rgm_midi_read_scan
//     launch 1, one workgroup: the track count every header claims, summed exclusively: where a file's tracks sit in the track table;
//     launch 2, one thread per file: header checks and the MTrk walk; fills the track table;
//     launch 3, one wave per track: every lane runs the same byte loop on the same values (LDS reads are broadcasts), the wave refills a 1 KB
//               window of the track with one 16-byte load per lane, lane 0 alone stores.  Note-ons wait in 16 x 128 queues whose heads and tails
//               live in LDS and whose links run through the on-records in the workspace;
//     launch 4, one workgroup per file: track prefix sums, the instruments, the tempo keys tick * 2^24 + value sorted in LDS, t_sec, then every
//               raw record placed in (track, channel, event) order with its seconds; the per-instrument end time is an integer maximum;
//     launch 5 / 6 (only with output arrays): exclusive row offsets over the files, the copy of the rows of every file that fits.
//   rgm_midi_read_rolls
//     a memset of the output, then
//     launch 1, one workgroup per (64 columns, file): velocity sums and onset marks of the tile in LDS with integer adds, written as float32 or
//               saturating uint8;
//     launch 2, one workgroup per file: the pedal loop, sequential over the file's control changes in instrument, then event order, 32768
//               columns of state at a time.
//
// Record capacities are bounded by bytes (a note needs an on and an off of at least 3 bytes each, a control change 3, a kept tempo 7), and a
// track's records start at (byte position of its chunk) / 6, 3 or 7: no count has to reach the host between the launches.  Floating point: IEEE
// double, no contraction.  Integer atomics only (a maximum and sums of integers): every launch repeats bit for bit, and a file's results depend
// neither on N nor on where the file lies in the blob.  All stores are ordinary vector stores.
#include "roll_bits.h"

#pragma clang fp contract(off)

namespace rgm {
namespace midiread {
using rollbits::MAX_PIANO;
using rollbits::MIN_PIANO;

constexpr int ST_OK = 0, ST_NOT_SMF = 1, ST_DIVISION = 2, ST_BAD_TRACK = 3, ST_TRUNCATED = 4, ST_DATA_BYTE = 5, ST_TEMPO_CAP = 6, ST_NO_NOTES = 7,
              ST_RANGE = 8, ST_CAPACITY = 9;
constexpr int TEMPO_CAP = 2048;                          // entries of a file's tempo map, the initial (0, 500000) included
constexpr long long MAX_TICK = 1ll << 40;                // a tick and a tempo value share one 64-bit sort key
constexpr long long MAX_COLUMNS = (1ll << 31) - 1;
constexpr int MAX_N = 65535, MAX_TRACKS = 1 << 26;
constexpr long long MAX_BYTES = 1ll << 30;
constexpr int WINDOW = 1024;                             // bytes of a track staged in LDS: 64 lanes x 16
constexpr int TILE = 64;                                 // columns of a velocity tile
constexpr int PEDAL_TILE = 32768;                        // columns of pedal state in LDS
constexpr int NOTE_WORDS = 8, CC_WORDS = 5;              // int64 words of a placed row

struct FileInfo {
  long long off, size, trk0, n_notes, n_ccs, n_tempo, columns;
  int status, ntrk, div, n_inst;
};
struct Trk {
  long long start, end;                                  // the track's bytes, relative to the file
  long long note0, cc0;                                  // where its rows begin among the file's
  int status, n_tempo, tempo0, inst0;
  int notes_ch[16], ccs_ch[16];
  signed char prog[16];
};
struct RawNote {
  long long t0, t1;
  int rank;                                              // among the notes of its (track, channel), in the order of their offs
  uint8_t ch, pitch, vel, pad;
};
struct OnRec {
  long long tick;
  int next, vel;
};
struct RawCC {
  long long tick;
  int rank;
  uint8_t ch, num, val, pad;
};
struct Inst {
  int track, ch, program, drum;
  long long n_notes, n_ccs, cols;
  unsigned long long maxend;                             // bits of the largest end / control-change time (non-negative doubles order as integers)
};

struct Layout {
  size_t files, trk_base, trks, raw_notes, ons, raw_ccs, raw_tempo, tempo_key, tempo_sec, notes, ccs, cc_flag, insts, note_off, cc_off, total;
};

__host__ __device__ inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

__host__ __device__ inline Layout layout(int N, long long B, int K) {
  Layout L;
  size_t at = 0;
  auto take = [&](size_t bytes) { size_t r = at; at += up16(bytes); return r; };
  const size_t n6 = (size_t)(B / 6) + 1, n3 = (size_t)(B / 3) + 1, n7 = (size_t)(B / 7) + 1;
  L.files = take((size_t)N * sizeof(FileInfo));
  L.trk_base = take((size_t)(N + 1) * 8);
  L.trks = take((size_t)(K + 1) * sizeof(Trk));
  L.raw_notes = take(n6 * sizeof(RawNote));
  L.ons = take(n3 * sizeof(OnRec));
  L.raw_ccs = take(n3 * sizeof(RawCC));
  L.raw_tempo = take(n7 * 8);
  L.tempo_key = take((n7 + N) * 8);
  L.tempo_sec = take((n7 + N) * 8);
  L.notes = take(n6 * NOTE_WORDS * 8);
  L.ccs = take(n3 * CC_WORDS * 8);
  L.cc_flag = take(n3 * 4);
  L.insts = take(((size_t)K * 16 + 1) * sizeof(Inst));
  L.note_off = take((size_t)(N + 1) * 8);
  L.cc_off = take((size_t)(N + 1) * 8);
  L.total = at;
  return L;
}

template <typename T>
__device__ __forceinline__ T* at(void* ws, size_t off) { return (T*)((char*)ws + off); }

__device__ __forceinline__ int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }
__device__ __forceinline__ long long be32(const uint8_t* p) { return ((long long)p[0] << 24) | (p[1] << 16) | (p[2] << 8) | p[3]; }

// ---- launch 1: track claims, summed over the files -------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) claims_kernel(const uint8_t* blob, const int64_t* offsets, int N, long long B, int K, void* ws, Layout L) {
  __shared__ long long part[256];
  __shared__ long long carry;
  FileInfo* files = at<FileInfo>(ws, L.files);
  long long* trk_base = at<long long>(ws, L.trk_base);
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int f0 = 0; f0 < N; f0 += 256) {
    const int f = f0 + threadIdx.x;
    long long claim = 0, off = 0, size = 0;
    int st = ST_OK;
    if (f < N) {
      off = offsets[f];
      const long long nxt = offsets[f + 1];
      if (off < 0 || nxt < off || nxt > B) { st = ST_NOT_SMF; off = 0; }
      else size = nxt - off;
      if (st == ST_OK && size >= 14) {
        const uint8_t* p = blob + off;
        if (p[0] == 'M' && p[1] == 'T' && p[2] == 'h' && p[3] == 'd') claim = be16(p + 10);
      }
    }
    part[threadIdx.x] = claim;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const long long v = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
      __syncthreads();
      part[threadIdx.x] += v;
      __syncthreads();
    }
    const long long base = carry + part[threadIdx.x] - claim;
    if (f < N) {
      if (base + claim > K) { st = st ? st : ST_CAPACITY; }   // the caller's total_tracks does not cover what the headers claim
      FileInfo fi = {};
      fi.off = off; fi.size = size; fi.trk0 = base; fi.status = st; fi.ntrk = (int)claim;
      files[f] = fi;
      trk_base[f] = base;
    }
    __syncthreads();
    if (threadIdx.x == 255) carry += part[255];
    __syncthreads();
  }
  if (threadIdx.x == 0) trk_base[N] = carry;
}

// ---- launch 2: header and chunk walk -----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) chunks_kernel(const uint8_t* blob, int N, void* ws, Layout L) {
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= N) return;
  FileInfo* fi = at<FileInfo>(ws, L.files) + f;
  Trk* trks = at<Trk>(ws, L.trks);
  if (fi->status) return;
  const long long size = fi->size;
  const uint8_t* p = blob + fi->off;
  if (size < 14 || p[0] != 'M' || p[1] != 'T' || p[2] != 'h' || p[3] != 'd') { fi->status = ST_NOT_SMF; return; }
  const long long hlen = be32(p + 4);
  const int ntrk = be16(p + 10), div = be16(p + 12);
  if ((div & 0x8000) || div == 0) { fi->status = ST_DIVISION; return; }
  fi->div = div;
  long long pos = 8 + hlen;
  for (int t = 0; t < ntrk; ++t) {
    if (pos + 8 > size || p[pos] != 'M' || p[pos + 1] != 'T' || p[pos + 2] != 'r' || p[pos + 3] != 'k') { fi->status = ST_BAD_TRACK; return; }
    const long long end = pos + 8 + be32(p + pos + 4);
    if (end > size) { fi->status = ST_BAD_TRACK; return; }
    Trk* tr = trks + fi->trk0 + t;
    tr->start = pos + 8;
    tr->end = end;
    pos = end;
  }
}

// ---- launch 3: the byte loop, one wave per track ----------------------------------------------------------------------------------------------
__device__ __forceinline__ long long first_lane(long long v) {
  const int lo = __builtin_amdgcn_readfirstlane((int)(v & 0xffffffffll)), hi = __builtin_amdgcn_readfirstlane((int)(v >> 32));
  return ((long long)hi << 32) | (unsigned int)lo;
}

struct Reader {
  const uint8_t* blob;
  long long foff, fsize, total, wbase;
  uint8_t* stage;
  // byte p of the file, or -1 behind its end.  Every lane asks for the same p, so the refill is taken by the whole wave: lane l loads the
  // 16 aligned bytes at wbase + 16 l when they hold a byte of the blob (the allocation is padded to a multiple of 16).
  __device__ __forceinline__ int get(long long p) {
    if (p < 0 || p >= fsize) return -1;
    const long long a = foff + p;
    if (a < wbase || a >= wbase + WINDOW) {
      wbase = a & ~15ll;
      __syncthreads();
      const long long pa = wbase + 16 * (int)threadIdx.x;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (pa < total) v = *(const uint4*)(blob + pa);
      ((uint4*)stage)[threadIdx.x] = v;
      __syncthreads();
    }
    return stage[a - wbase];
  }
};

__global__ void __launch_bounds__(64) parse_kernel(const uint8_t* blob, int N, long long B, void* ws, Layout L) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[WINDOW];
  __shared__ int qhead[16 * 128], qtail[16 * 128];
  __shared__ int notes_ch[16], ccs_ch[16], prog[16];
  const long long* trk_base = at<long long>(ws, L.trk_base);
  const long long slot = blockIdx.x;
  if (slot >= trk_base[N]) return;
  int lo = 0, hi = N;                                    // the last file whose base is <= slot
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (trk_base[mid] <= slot) lo = mid; else hi = mid;
  }
  const FileInfo fi = at<FileInfo>(ws, L.files)[lo];
  if (fi.status) return;
  Trk* tr = at<Trk>(ws, L.trks) + slot;
  const int lane = threadIdx.x;
  for (int i = lane; i < 16 * 128; i += 64) { qhead[i] = -1; qtail[i] = -1; }
  if (lane < 16) { notes_ch[lane] = 0; ccs_ch[lane] = 0; prog[lane] = 0; }
  __syncthreads();

  const long long start = tr->start, end = tr->end;
  const long long chunk = fi.off + start - 8, chunk_end = fi.off + end;      // absolute bytes of the chunk: its records' address space
  RawNote* rnotes = at<RawNote>(ws, L.raw_notes) + chunk / 6;
  OnRec* ons = at<OnRec>(ws, L.ons) + chunk / 3;
  RawCC* rccs = at<RawCC>(ws, L.raw_ccs) + chunk / 3;
  unsigned long long* rtempo = at<unsigned long long>(ws, L.raw_tempo) + chunk / 7;
  const long long cap6 = chunk_end / 6 - chunk / 6, cap3 = chunk_end / 3 - chunk / 3, cap7 = chunk_end / 7 - chunk / 7;

  Reader rd = {blob, fi.off, fi.size, B, -(long long)WINDOW - 16, stage};
  long long p = start, tick = 0;
  int status = 0, err = ST_OK, n_notes = 0, n_ons = 0, n_ccs = 0, n_tempo = 0;
  while (p < end && !err) {
    long long d = 0;
    int b;
    do {                                                 // the delta: any number of bytes
      b = rd.get(p++);
      if (b < 0) { err = ST_TRUNCATED; break; }
      d = (d << 7) | (b & 0x7f);
      if (d >= MAX_TICK) { err = ST_RANGE; break; }
    } while (b & 0x80);
    if (err) break;
    tick += d;
    if (tick >= MAX_TICK) { err = ST_RANGE; break; }
    b = rd.get(p);
    if (b < 0) { err = ST_TRUNCATED; break; }
    if (b == 0xff || b == 0xf0 || b == 0xf7) {
      int kind = -1;
      if (b == 0xff) {
        kind = rd.get(p + 1);
        if (kind < 0) { err = ST_TRUNCATED; break; }
        p += 2;
      } else {
        p += 1;
      }
      long long ln = 0;
      int c;
      do {
        c = rd.get(p++);
        if (c < 0) { err = ST_TRUNCATED; break; }
        ln = (ln << 7) | (c & 0x7f);
        if (ln > MAX_TICK) ln = MAX_TICK;                // longer than any file: the skip below leaves the track either way
      } while (c & 0x80);
      if (err) break;
      if (kind == 0x51 && ln == 3) {
        const int v0 = rd.get(p), v1 = rd.get(p + 1), v2 = rd.get(p + 2);
        if (v0 < 0 || v1 < 0 || v2 < 0) { err = ST_TRUNCATED; break; }
        if (n_tempo >= cap7) { err = ST_CAPACITY; break; }
        if (lane == 0) rtempo[n_tempo] = ((unsigned long long)tick << 24) | (unsigned)((v0 << 16) | (v1 << 8) | v2);
        ++n_tempo;
      }
      p += ln;
      continue;
    }
    if (b & 0x80) { status = b; ++p; }
    const int hi4 = status & 0xf0, ch = status & 0x0f;
    const int nargs = (hi4 == 0xc0 || hi4 == 0xd0) ? 1 : 2;
    const int a0 = rd.get(p), a1 = nargs == 2 ? rd.get(p + 1) : 0;
    if (a0 < 0 || a1 < 0) { err = ST_TRUNCATED; break; }
    p += nargs;
    if ((a0 | a1) & 0x80) { err = ST_DATA_BYTE; break; }
    if (hi4 == 0xc0) {
      prog[ch] = a0;
    } else if (hi4 == 0xb0) {
      if (n_ccs >= cap3) { err = ST_CAPACITY; break; }
      const int rank = ccs_ch[ch];
      ccs_ch[ch] = rank + 1;
      if (lane == 0) rccs[n_ccs] = RawCC{tick, rank, (uint8_t)ch, (uint8_t)a0, (uint8_t)a1, 0};
      ++n_ccs;
    } else if (hi4 == 0x90 && a1 > 0) {
      if (n_ons >= cap3) { err = ST_CAPACITY; break; }
      const int q = ch * 128 + a0, tail = qtail[q];
      if (lane == 0) {
        ons[n_ons] = OnRec{tick, -1, a1};
        if (tail >= 0) ons[tail].next = n_ons;
      }
      if (tail < 0) qhead[q] = n_ons;
      qtail[q] = n_ons;
      ++n_ons;
    } else if (hi4 == 0x80 || hi4 == 0x90) {
      const int q = ch * 128 + a0, head = qhead[q];
      if (head >= 0) {
        long long t0 = 0;
        int next = 0, vel = 0;
        if (lane == 0) { const OnRec o = ons[head]; t0 = o.tick; next = o.next; vel = o.vel; }
        t0 = first_lane(t0);
        next = __builtin_amdgcn_readfirstlane(next);
        vel = __builtin_amdgcn_readfirstlane(vel);
        qhead[q] = next;
        if (next < 0) qtail[q] = -1;
        if (n_notes >= cap6) { err = ST_CAPACITY; break; }
        const int rank = notes_ch[ch];
        notes_ch[ch] = rank + 1;
        if (lane == 0) rnotes[n_notes] = RawNote{t0, tick, rank, (uint8_t)ch, (uint8_t)a0, (uint8_t)vel, 0};
        ++n_notes;
      }
    }
  }
  __syncthreads();
  if (lane == 0) { tr->status = err; tr->n_tempo = n_tempo; }
  if (lane < 16) { tr->notes_ch[lane] = notes_ch[lane]; tr->ccs_ch[lane] = ccs_ch[lane]; tr->prog[lane] = (signed char)prog[lane]; }
}

// ---- launch 4: per file -- instruments, tempo map, seconds, placement -------------------------------------------------------------------
__device__ __forceinline__ double seconds_of(long long tick, const unsigned long long* keys, const double* sec, int n, double den) {
  int lo = 0, hi = n;                                    // the last entry at or before the tick (entry 0 is at tick 0)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((long long)(keys[mid] >> 24) <= tick) lo = mid; else hi = mid;
  }
  const double dt = (double)(tick - (long long)(keys[lo] >> 24)), us = (double)(keys[lo] & 0xffffff);
  return sec[lo] + (dt * us) / den;
}

__global__ void __launch_bounds__(256) place_kernel(double fs, void* ws, Layout L, int32_t* status_out, int64_t* counts_out, int64_t* columns_out) {
  __shared__ unsigned long long keys[TEMPO_CAP];
  __shared__ double sec[TEMPO_CAP];
  __shared__ int s_status, s_inst, s_tempo, s_cols;
  __shared__ long long s_notes, s_ccs;
  const int f = blockIdx.x, tid = threadIdx.x;
  FileInfo* fi = at<FileInfo>(ws, L.files) + f;
  Trk* trks = at<Trk>(ws, L.trks) + fi->trk0;
  Inst* insts = at<Inst>(ws, L.insts) + fi->trk0 * 16;
  const int ntrk = fi->ntrk;
  if (tid == 0) {
    int st = fi->status, n_inst = 0, n_tempo = 1;
    long long n_notes = 0, n_ccs = 0;
    for (int t = 0; t < ntrk && !st; ++t) {
      Trk* tr = trks + t;
      if (tr->status) { st = tr->status; break; }
      tr->inst0 = n_inst; tr->note0 = n_notes; tr->cc0 = n_ccs; tr->tempo0 = n_tempo;
      for (int c = 0; c < 16; ++c) {
        if (tr->notes_ch[c] == 0 && tr->ccs_ch[c] == 0) continue;
        Inst in = {t, c, tr->prog[c], c == 9, tr->notes_ch[c], tr->ccs_ch[c], 0, 0ull};
        insts[n_inst++] = in;
        n_notes += tr->notes_ch[c];
        n_ccs += tr->ccs_ch[c];
      }
      n_tempo += tr->n_tempo;
      if (n_tempo > TEMPO_CAP) st = ST_TEMPO_CAP;
    }
    s_status = st; s_inst = n_inst; s_tempo = n_tempo; s_notes = n_notes; s_ccs = n_ccs; s_cols = 0;
    __threadfence();
  }
  __syncthreads();
  int st = s_status;
  if (!st) {
    const int n_tempo = s_tempo, div = fi->div;
    const long long foff = fi->off;
    int n2 = 1;
    while (n2 < n_tempo) n2 <<= 1;
    for (int i = tid; i < n2; i += 256) keys[i] = i == 0 ? 500000ull : ~0ull;
    __syncthreads();
    for (int t = 0; t < ntrk; ++t) {
      const Trk* tr = trks + t;
      const unsigned long long* raw = at<unsigned long long>(ws, L.raw_tempo) + (foff + tr->start - 8) / 7;
      for (int i = tid; i < tr->n_tempo; i += 256) keys[tr->tempo0 + i] = raw[i];
    }
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)                    // bitonic sort: equal ticks order by value, as the host's tuples do
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < n2; i += 256) {
          const int x = i ^ j;
          if (x > i) {
            const unsigned long long a = keys[i], b = keys[x];
            if (((i & k) == 0) == (a > b)) { keys[i] = b; keys[x] = a; }
          }
        }
        __syncthreads();
      }
    const double den = 1e6 * (double)div;
    if (tid == 0) {
      double s = 0.0;
      sec[0] = 0.0;
      for (int k = 1; k < n_tempo; ++k) {
        const double dt = (double)((long long)(keys[k] >> 24) - (long long)(keys[k - 1] >> 24)), us = (double)(keys[k - 1] & 0xffffff);
        const double term = (dt * us) / den;
        s = k == 1 ? term : s + term;
        sec[k] = s;
      }
    }
    __syncthreads();
    unsigned long long* gkey = at<unsigned long long>(ws, L.tempo_key) + foff / 7 + f;
    double* gsec = at<double>(ws, L.tempo_sec) + foff / 7 + f;
    for (int i = tid; i < n_tempo; i += 256) { gkey[i] = keys[i]; gsec[i] = sec[i]; }

    long long* notes = at<long long>(ws, L.notes) + (foff / 6) * NOTE_WORDS;
    long long* ccs = at<long long>(ws, L.ccs) + (foff / 3) * CC_WORDS;
    for (int t = 0; t < ntrk; ++t) {
      const Trk* tr = trks + t;
      const long long chunk = foff + tr->start - 8;
      const RawNote* rn = at<RawNote>(ws, L.raw_notes) + chunk / 6;
      const RawCC* rc = at<RawCC>(ws, L.raw_ccs) + chunk / 3;
      int tn = 0, tc = 0;
      for (int c = 0; c < 16; ++c) { tn += tr->notes_ch[c]; tc += tr->ccs_ch[c]; }
      for (int i = tid; i < tn; i += 256) {
        const RawNote r = rn[i];
        long long pre = 0;
        int ir = 0;
        for (int c = 0; c < r.ch; ++c) { pre += tr->notes_ch[c]; ir += (tr->notes_ch[c] || tr->ccs_ch[c]) ? 1 : 0; }
        const int inst = tr->inst0 + ir;
        const double s0 = seconds_of(r.t0, keys, sec, n_tempo, den), s1 = seconds_of(r.t1, keys, sec, n_tempo, den);
        long long* row = notes + (tr->note0 + pre + r.rank) * NOTE_WORDS;
        row[0] = inst; row[1] = r.ch; row[2] = r.pitch; row[3] = r.vel; row[4] = r.t0; row[5] = r.t1;
        row[6] = __double_as_longlong(s0); row[7] = __double_as_longlong(s1);
        atomicMax(&insts[inst].maxend, (unsigned long long)__double_as_longlong(s1));
      }
      for (int i = tid; i < tc; i += 256) {
        const RawCC r = rc[i];
        long long pre = 0;
        int ir = 0;
        for (int c = 0; c < r.ch; ++c) { pre += tr->ccs_ch[c]; ir += (tr->notes_ch[c] || tr->ccs_ch[c]) ? 1 : 0; }
        const int inst = tr->inst0 + ir;
        const double s = seconds_of(r.tick, keys, sec, n_tempo, den);
        long long* row = ccs + (tr->cc0 + pre + r.rank) * CC_WORDS;
        row[0] = inst; row[1] = r.num; row[2] = r.val; row[3] = r.tick; row[4] = __double_as_longlong(s);
        atomicMax(&insts[inst].maxend, (unsigned long long)__double_as_longlong(s));
      }
    }
    __threadfence();
    __syncthreads();
    for (int i = tid; i < s_inst; i += 256) {            // columns of every instrument that has notes: int(fs * end time)
      if (insts[i].n_notes == 0) continue;
      const double e = __longlong_as_double((long long)atomicMax(&insts[i].maxend, 0ull));
      const double c = fs * e;
      if (!(c < (double)MAX_COLUMNS)) { atomicMax(&s_status, ST_RANGE); continue; }
      insts[i].cols = (long long)c;
      atomicMax(&s_cols, (int)(long long)c);
    }
    __syncthreads();
    st = s_status;
    if (!st && s_cols == 0) st = ST_NO_NOTES;
  }
  if (tid == 0) {
    const bool ok = st == ST_OK;
    fi->status = st;
    fi->n_notes = ok ? s_notes : 0; fi->n_ccs = ok ? s_ccs : 0; fi->n_tempo = ok ? s_tempo : 0; fi->n_inst = ok ? s_inst : 0;
    fi->columns = ok ? s_cols : 0;
    status_out[f] = st;
    counts_out[4 * f + 0] = fi->n_notes; counts_out[4 * f + 1] = fi->n_ccs; counts_out[4 * f + 2] = fi->n_tempo; counts_out[4 * f + 3] = fi->n_inst;
    columns_out[f] = fi->columns;
  }
}

// ---- launches 5 and 6: row offsets over the files and the copy of every file that fits ----------------------------------------------------
__global__ void __launch_bounds__(256) offsets_kernel(int N, void* ws, Layout L, int64_t* note_off_out, int64_t* cc_off_out) {
  __shared__ long long pa[256], pb[256];
  __shared__ long long ca, cb;
  const FileInfo* files = at<FileInfo>(ws, L.files);
  long long* note_off = at<long long>(ws, L.note_off);
  long long* cc_off = at<long long>(ws, L.cc_off);
  if (threadIdx.x == 0) { ca = 0; cb = 0; }
  __syncthreads();
  for (int f0 = 0; f0 < N; f0 += 256) {
    const int f = f0 + threadIdx.x;
    const long long a = f < N ? files[f].n_notes : 0, b = f < N ? files[f].n_ccs : 0;
    pa[threadIdx.x] = a; pb[threadIdx.x] = b;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const long long va = threadIdx.x >= d ? pa[threadIdx.x - d] : 0, vb = threadIdx.x >= d ? pb[threadIdx.x - d] : 0;
      __syncthreads();
      pa[threadIdx.x] += va; pb[threadIdx.x] += vb;
      __syncthreads();
    }
    if (f < N) {
      const long long oa = ca + pa[threadIdx.x] - a, ob = cb + pb[threadIdx.x] - b;
      note_off[f] = oa; cc_off[f] = ob;
      if (note_off_out) note_off_out[f] = oa;
      if (cc_off_out) cc_off_out[f] = ob;
    }
    __syncthreads();
    if (threadIdx.x == 255) { ca += pa[255]; cb += pb[255]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    note_off[N] = ca; cc_off[N] = cb;
    if (note_off_out) note_off_out[N] = ca;
    if (cc_off_out) cc_off_out[N] = cb;
  }
}

__global__ void __launch_bounds__(256) copy_kernel(void* ws, Layout L, int64_t* notes_out, long long notes_cap, int64_t* ccs_out, long long ccs_cap) {
  const int f = blockIdx.y;
  const FileInfo fi = at<FileInfo>(ws, L.files)[f];
  const long long no = at<long long>(ws, L.note_off)[f], co = at<long long>(ws, L.cc_off)[f];
  if (no + fi.n_notes > notes_cap || co + fi.n_ccs > ccs_cap) return;        // a file that does not fit is left out whole
  const long long* notes = at<long long>(ws, L.notes) + (fi.off / 6) * NOTE_WORDS;
  const long long* ccs = at<long long>(ws, L.ccs) + (fi.off / 3) * CC_WORDS;
  const long long step = (long long)gridDim.x * 256, first = (long long)blockIdx.x * 256 + threadIdx.x;
  for (long long i = first; i < fi.n_notes * NOTE_WORDS; i += step) notes_out[no * NOTE_WORDS + i] = notes[i];
  for (long long i = first; i < fi.n_ccs * CC_WORDS; i += step) ccs_out[co * CC_WORDS + i] = ccs[i];
}

// ---- rolls ------------------------------------------------------------------------------------------------------------------------------------
template <bool U8>
__global__ void __launch_bounds__(256) velocity_kernel(double fs, long long start_column, int T, void* out, unsigned long long* overflow, void* ws, Layout L) {
  __shared__ unsigned int vel[128][TILE];
  __shared__ uint8_t ons[128][TILE];
  __shared__ int s_over;
  const int f = blockIdx.y, tid = threadIdx.x;
  const FileInfo fi = at<FileInfo>(ws, L.files)[f];
  const long long lo = start_column + (long long)blockIdx.x * TILE;          // the tile's first column in the file
  if (fi.status || lo >= fi.columns) return;                                  // the output is zero already
  for (int i = tid; i < 128 * TILE; i += 256) { (&vel[0][0])[i] = 0; (&ons[0][0])[i] = 0; }
  if (tid == 0) s_over = 0;
  __syncthreads();
  const long long* notes = at<long long>(ws, L.notes) + (fi.off / 6) * NOTE_WORDS;
  const Inst* insts = at<Inst>(ws, L.insts) + fi.trk0 * 16;
  for (long long i = tid; i < fi.n_notes; i += 256) {
    const long long* row = notes + i * NOTE_WORDS;
    const Inst* in = insts + row[0];
    if (in->drum) continue;
    const int pitch = (int)row[2];
    const unsigned int v = (unsigned int)row[3];
    const long long c0 = (long long)(__longlong_as_double(row[6]) * fs), c1 = (long long)(__longlong_as_double(row[7]) * fs);
    const long long a = max(c0, lo), b = min(c1, lo + TILE);
    for (long long c = a; c < b; ++c) atomicAdd(&vel[pitch][c - lo], v);
    if (in->cols > 0) {
      const long long oc = min(c0, in->cols - 1);
      if (oc >= lo && oc < lo + TILE) ons[pitch][oc - lo] = 127;
    }
  }
  __syncthreads();
  const int width = (int)min((long long)TILE, (long long)T - (long long)blockIdx.x * TILE);
  int over = 0;
  for (int i = tid; i < 128 * TILE; i += 256) {
    const int p = i / TILE, c = i % TILE;
    if (c >= width) continue;
    const unsigned int v = vel[p][c];
    const size_t o0 = (((size_t)f * 3 + 0) * 128 + p) * (size_t)T + (size_t)blockIdx.x * TILE + c;
    const size_t o1 = o0 + (size_t)128 * T;
    if (U8) {
      over += v > 255u;
      ((uint8_t*)out)[o0] = (uint8_t)min(v, 255u);
      ((uint8_t*)out)[o1] = ons[p][c];
    } else {
      ((float*)out)[o0] = (float)v;
      ((float*)out)[o1] = (float)ons[p][c];
    }
  }
  if (U8) {
    if (over) atomicAdd(&s_over, over);
    __syncthreads();
    if (tid == 0 && s_over) atomicAdd(overflow + f, (unsigned long long)s_over);
  }
}

template <bool U8>
__global__ void __launch_bounds__(256) pedal_kernel(double fs, long long start_column, int T, void* out, void* ws, Layout L) {
  __shared__ uint8_t state[PEDAL_TILE];
  const int f = blockIdx.x, tid = threadIdx.x;
  const FileInfo fi = at<FileInfo>(ws, L.files)[f];
  if (fi.status) return;
  const long long Tf = fi.columns, stop = min(Tf, start_column + (long long)T);
  const long long* ccs = at<long long>(ws, L.ccs) + (fi.off / 3) * CC_WORDS;
  int* flags = at<int>(ws, L.cc_flag) + fi.off / 3;
  for (long long lo = 0; lo < stop; lo += PEDAL_TILE) {
    for (int i = tid; i < PEDAL_TILE; i += 256) state[i] = 0;
    __syncthreads();
    if (tid < 64) {
      // the wave loads 64 control changes at a time and then takes them one after the other, every lane on the same values
      for (long long base = 0; base < fi.n_ccs; base += 64) {
        const long long i = base + tid;
        int num = -1, val = 0, flag = 0;
        long long t = 0;
        if (i < fi.n_ccs) {
          const long long* row = ccs + i * CC_WORDS;
          num = (int)row[1]; val = (int)row[2];
          t = (long long)(__longlong_as_double(row[4]) * fs);
          if (num == 64 && t >= lo - 2 && t < lo) flag = __hip_atomic_load(flags + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const unsigned long long live = __ballot(num == 64 && t < Tf && t >= lo - 2 && t < lo + PEDAL_TILE);
        for (unsigned long long m = live; m; m &= m - 1) {
          const int j = __builtin_ctzll(m);
          const long long tj = ((long long)__shfl((int)(t >> 32), j) << 32) | (unsigned int)__shfl((int)t, j);
          const int vj = __shfl(val, j), fj = __shfl(flag, j);
          const int q = min(vj / 16 * 16 + 8, 127);
          bool shift;
          if (tj >= lo) {
            const int cur = state[tj - lo];
            shift = cur != 0 && abs(cur - vj) > 64;
            if (tid == 0) __hip_atomic_store(flags + base + j, shift ? 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          } else {
            shift = fj != 0;
            if (!shift) continue;
          }
          const long long tgt = shift ? min(tj + 2, Tf - 1) : tj;
          if (tgt >= lo && tgt < lo + PEDAL_TILE && tid == 0) state[tgt - lo] = (uint8_t)q;
          __builtin_amdgcn_wave_barrier();
        }
      }
    }
    __syncthreads();
    const long long a = max(lo, start_column), b = min(lo + PEDAL_TILE, stop);
    for (long long c = a + tid; c < b; c += 256) {
      const int v = state[c - lo];
      if (!v) continue;
      for (int p = MIN_PIANO; p <= MAX_PIANO; ++p) {
        const size_t o = (((size_t)f * 3 + 2) * 128 + p) * (size_t)T + (size_t)(c - start_column);
        if (U8) ((uint8_t*)out)[o] = (uint8_t)v; else ((float*)out)[o] = (float)v;
      }
    }
    __syncthreads();
  }
}
}  // namespace midiread
}  // namespace rgm

using namespace rgm;

extern "C" size_t rgm_midi_read_workspace(int N, long long total_bytes, int total_tracks) {
  if (N <= 0 || N > midiread::MAX_N || total_bytes <= 0 || total_bytes > midiread::MAX_BYTES || total_tracks < 0 || total_tracks > midiread::MAX_TRACKS)
    return 0;
  return midiread::layout(N, total_bytes, total_tracks).total;
}

static int midi_read_check(const char* what, int N, long long total_bytes, int total_tracks, double fs, const void* ws, size_t ws_bytes) {
  RGM_REQUIRE(N > 0 && N <= midiread::MAX_N, "%s: N = %d (1 .. %d files per call)", what, N, midiread::MAX_N);
  RGM_REQUIRE(total_bytes > 0 && total_bytes <= midiread::MAX_BYTES, "%s: %lld bytes (1 .. 2^30 per call)", what, total_bytes);
  RGM_REQUIRE(total_tracks >= 0 && total_tracks <= midiread::MAX_TRACKS, "%s: %d tracks (0 .. 2^26 per call)", what, total_tracks);
  RGM_REQUIRE(fs > 0.0 && fs <= 1e6, "%s: fs = %g columns per second (0 < fs <= 1e6)", what, fs);
  const size_t need = rgm_midi_read_workspace(N, total_bytes, total_tracks);
  if (!ws || ws_bytes < need) {
    set_error("%s: workspace of %zu bytes, %zu needed", what, ws ? ws_bytes : (size_t)0, need);
    return RGM_ERR_WORKSPACE;
  }
  RGM_REQUIRE(((uintptr_t)ws & 15) == 0, "%s: the workspace must be 16-byte aligned", what);
  return RGM_OK;
}

extern "C" int rgm_midi_read_scan(const uint8_t* blob, const int64_t* offsets, int N, long long total_bytes, int total_tracks, double fs,
                                  int32_t* status, int64_t* counts, int64_t* columns, int64_t* note_off, int64_t* cc_off, int64_t* notes,
                                  long long notes_cap, int64_t* ccs, long long ccs_cap, void* ws, size_t ws_bytes, void* stream) {
  RGM_REQUIRE(blob && offsets && status && counts && columns, "midi_read_scan: bad arguments");
  RGM_REQUIRE(((uintptr_t)blob & 15) == 0, "midi_read_scan: the blob must be 16-byte aligned (and its allocation padded to a multiple of 16 bytes)");
  RGM_REQUIRE(notes_cap >= 0 && ccs_cap >= 0 && (notes || notes_cap == 0) && (ccs || ccs_cap == 0),
              "midi_read_scan: an array of %lld note rows / %lld control-change rows needs its pointer", notes_cap, ccs_cap);
  RGM_REQUIRE((notes == nullptr) == (ccs == nullptr), "midi_read_scan: the note and control-change arrays come together or not at all");
  RGM_TRY(midi_read_check("midi_read_scan", N, total_bytes, total_tracks, fs, ws, ws_bytes));
  const midiread::Layout L = midiread::layout(N, total_bytes, total_tracks);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(midiread::claims_kernel, dim3(1), dim3(256), 0, s, blob, offsets, N, total_bytes, total_tracks, ws, L);
  RGM_LAUNCH_CHECK();
  hipLaunchKernelGGL(midiread::chunks_kernel, dim3((N + 63) / 64), dim3(64), 0, s, blob, N, ws, L);
  RGM_LAUNCH_CHECK();
  if (total_tracks > 0) {
    hipLaunchKernelGGL(midiread::parse_kernel, dim3(total_tracks), dim3(64), 0, s, blob, N, total_bytes, ws, L);
    RGM_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(midiread::place_kernel, dim3(N), dim3(256), 0, s, fs, ws, L, status, counts, columns);
  RGM_LAUNCH_CHECK();
  if (notes || note_off || cc_off) {
    hipLaunchKernelGGL(midiread::offsets_kernel, dim3(1), dim3(256), 0, s, N, ws, L, note_off, cc_off);
    RGM_LAUNCH_CHECK();
  }
  if (notes) {
    const long long per_file = total_bytes / N / 4096 + 1;
    const int g = per_file < 64 ? (int)per_file : 64;
    hipLaunchKernelGGL(midiread::copy_kernel, dim3(g, N), dim3(256), 0, s, ws, L, notes, notes_cap, ccs, ccs_cap);
    RGM_LAUNCH_CHECK();
  }
  return RGM_OK;
}

extern "C" int rgm_midi_read_rolls(int N, long long total_bytes, int total_tracks, double fs, long long start_column, int T, int out_u8, void* out,
                                   int64_t* overflow, void* ws, size_t ws_bytes, void* stream) {
  RGM_REQUIRE(out, "midi_read_rolls: bad arguments");
  RGM_REQUIRE(out_u8 == 0 || out_u8 == 1, "midi_read_rolls: out_u8 = %d (0: float32, 1: uint8 with an overflow count)", out_u8);
  RGM_REQUIRE(!out_u8 || overflow, "midi_read_rolls: the uint8 output needs the overflow array");
  RGM_REQUIRE(T >= 1 && T <= (1 << 24), "midi_read_rolls: T = %d columns (1 .. 2^24)", T);
  RGM_REQUIRE(start_column >= 0 && start_column < midiread::MAX_COLUMNS, "midi_read_rolls: start_column = %lld", start_column);
  RGM_TRY(midi_read_check("midi_read_rolls", N, total_bytes, total_tracks, fs, ws, ws_bytes));
  const midiread::Layout L = midiread::layout(N, total_bytes, total_tracks);
  hipStream_t s = (hipStream_t)stream;
  RGM_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)N * 3 * 128 * T * (out_u8 ? 1 : 4), s));
  if (overflow) RGM_CHECK_HIP(hipMemsetAsync(overflow, 0, (size_t)N * 8, s));
  const dim3 grid((T + midiread::TILE - 1) / midiread::TILE, N);
  if (out_u8) {
    hipLaunchKernelGGL(midiread::velocity_kernel<true>, grid, dim3(256), 0, s, fs, start_column, T, out, (unsigned long long*)overflow, ws, L);
    RGM_LAUNCH_CHECK();
    hipLaunchKernelGGL(midiread::pedal_kernel<true>, dim3(N), dim3(256), 0, s, fs, start_column, T, out, ws, L);
  } else {
    hipLaunchKernelGGL(midiread::velocity_kernel<false>, grid, dim3(256), 0, s, fs, start_column, T, out, (unsigned long long*)overflow, ws, L);
    RGM_LAUNCH_CHECK();
    hipLaunchKernelGGL(midiread::pedal_kernel<false>, dim3(N), dim3(256), 0, s, fs, start_column, T, out, ws, L);
  }
  RGM_LAUNCH_CHECK();
  return RGM_OK;
}
