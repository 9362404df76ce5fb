// synth.hip -- the note rows of a batch of piano rolls become audio on the device: the sine voice of the reference's vendored pretty_midi
// fork, PrettyMIDI.synthesize(fs, wave=np.sin) (pretty_midi/pretty_midi.py:954-983) over Instrument.synthesize (pretty_midi/instrument.py:355-441),
// applied to what piano_roll_to_pretty_midi (music_rule_guidance/piano_roll_to_chord.py:167-275) finds.  The host partner (synthesize_roll) is
// the oracle.  Definition, the one departure (an all-zero waveform stays zero instead of 0 / 0) and measurements: docs/rounds/synth.md, include/rgm.h.
//
//   rgm_synth_render
//     launch 1, grid (chunks of 512 audio samples, N), block 256: a thread owns two neighbouring audio samples.  The workgroup walks the
//               sample's note rows 256 at a time (they lie in (pitch, start column) order), keeps those whose audio interval
//               [samp[start], samp[end]) meets the chunk, packs them in order into LDS with a workgroup scan -- a batch holds at most 256,
//               however many notes meet the chunk -- and every thread adds the staged notes that cover its samples, in the staged order:
//               ascending pitch, and within a pitch the intervals are disjoint.  Along the way it finds the largest end column; with the
//               last CC row that gives the sample's length, beyond which zeros are written.  One 16-byte store per thread, and the
//               chunk's largest magnitude into the workspace.
//     launch 2, grid N, block 256: the maximum of the chunk maxima; writes peak, lengths and silent.
//   rgm_synth_pcm
//     one launch, grid (chunks of 2048 audio samples, N), block 256: a thread owns eight neighbouring samples; format 0 writes float32
//               (double division, one rounding to float), format 1 the int16 of rint((wave / peak) * 32767) behind a 44-byte RIFF header
//               per sample, at a uniform stride.
//
// Arithmetic: each term is (((exp(-k / audio_fs) * fade) * vel) * sin(omega[p] * k)) in IEEE double without contraction; k / audio_fs, the
// phase increment omega, the fade table and the integer truncations samp / len come from the host's own float64 arithmetic, so sin and
// exp are the only places where the device can differ from numpy.  No atomics: a chunk has one owner, the maximum is exact and free of
// order, so every launch repeats bit for bit and a sample's rows depend neither on N, nor on the chunk size, nor on its place in the batch.
// The note rows are only read; columns are clamped to [0, T] and pitches to 0 .. 127 before they index a table.
#include "common.h"

#pragma clang fp contract(off)

namespace rgm {
namespace synth {
constexpr int MAX_T = 32768, MAX_N = 65535;
constexpr long long MAX_LEN = (1ll << 31) - 1;
constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int CHUNK = 2 * THREADS;                      // audio samples of a render workgroup
constexpr int PCM_CHUNK = 8 * THREADS;

__host__ __device__ inline long long n_chunks(long long cap) { return (cap + CHUNK - 1) / CHUNK; }
__host__ __device__ inline long long fade_cap(long long cap) { return cap / 8 + 16; }         // F = int(.1 audio_fs) <= (cap + 1) / 10

// workspace: samp[T + 1] int64 | len[T + 1] int64 | omega[128] double | fade[fade_cap] double | chunk maxima [N][n_chunks] double
struct View {
  const long long *samp, *len;
  const double *omega, *fade;
  double* part;
};
__host__ __device__ inline size_t table_bytes(int T, long long cap) { return ((size_t)2 * (T + 1) + 128 + (size_t)fade_cap(cap)) * 8; }
__host__ __device__ inline View view(void* ws, int T, long long cap) {
  View v;
  long long* b = (long long*)ws;
  v.samp = b;
  v.len = b + (T + 1);
  v.omega = (const double*)(b + 2 * (T + 1));
  v.fade = v.omega + 128;
  v.part = (double*)(v.fade + fade_cap(cap));
  return v;
}

struct Staged {
  int a, b;                                             // audio samples [a, b)
  int pitch, vel;
};

// grid (n_chunks, N), block 256
__global__ __launch_bounds__(THREADS) void render_kernel(int T, const int32_t* __restrict__ notes, long long notes_rows,
                                                         const int64_t* __restrict__ note_off, const int32_t* __restrict__ ccs,
                                                         long long ccs_rows, const int64_t* __restrict__ cc_off,
                                                         const int64_t* __restrict__ counts, double audio_fs, int F, double* __restrict__ wave,
                                                         long long cap, void* ws) {
  __shared__ Staged staged[THREADS];
  __shared__ int wave_cnt[WAVES];
  __shared__ int wave_end[WAVES];
  __shared__ double wave_max[WAVES];
  const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const View v = view(ws, T, cap);
  const long long c0 = (long long)blockIdx.x * CHUNK, c1 = c0 + CHUNK;       // the chunk's audio samples [c0, c1)
  const long long i0 = c0 + 2 * tid;
  long long n_notes = counts[4 * n], n_ccs = counts[4 * n + 1];
  const long long no = note_off[n], co = cc_off[n];
  if (n_notes < 0 || no < 0 || no + n_notes > notes_rows) n_notes = 0;       // rows outside the arrays: the sample is left silent
  if (n_ccs < 0 || co < 0 || co + n_ccs > ccs_rows) n_ccs = 0;
  const int32_t* rows = notes + 4 * no;
  double acc0 = 0.0, acc1 = 0.0;
  int max_end = 0;
  for (long long base = 0; base < n_notes; base += THREADS) {
    // every thread looks at one note row
    Staged s = {0, 0, 0, 0};
    bool hit = false;
    if (base + tid < n_notes) {
      const int4 r = *(const int4*)(rows + 4 * (base + tid));                // pitch, velocity, start column, end column
      const int sc = min(max(r.z, 0), T), ec = min(max(r.w, 0), T);
      max_end = max(max_end, ec);
      s.a = (int)v.samp[sc];
      s.b = (int)v.samp[ec];
      s.pitch = r.x & 127;
      s.vel = r.y;
      hit = s.a < c1 && s.b > c0 && s.b > s.a;
    }
    const uint64_t m = __ballot(hit);
    if (lane == 0) wave_cnt[wv] = __popcll(m);
    __syncthreads();
    int before = __popcll(m & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      const int q = wave_cnt[w];
      if (w < wv) before += q;
      total += q;
    }
    if (hit) staged[before] = s;
    __syncthreads();
    for (int j = 0; j < total; ++j) {
      const Staged e = staged[j];                       // one address for the whole wave: a broadcast
      if (i0 + 1 < e.a || i0 >= e.b) continue;
      const int len = e.b - e.a;
      const double om = v.omega[e.pitch], vel = (double)e.vel;
      const double step = len > 1 ? -1.0 / (double)(len - 1) : 0.0;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const long long i = i0 + u;
        if (i < e.a || i >= e.b) continue;
        const int k = (int)(i - e.a);
        double env = exp(-(double)k / audio_fs);
        if (len > F) {
          if (k >= len - F) env = env * v.fade[k - (len - F)];
        } else {                                        // numpy's linspace(1, 0, len): k * step + 1, its last entry set to 0; [1.0] for len = 1
          double f = len > 1 ? (double)k * step + 1.0 : 1.0;
          if (len > 1 && k == len - 1) f = 0.0;
          env = env * f;
        }
        env = env * vel;
        const double term = env * sin(om * (double)k);
        if (u == 0) acc0 = acc0 + term;
        else acc1 = acc1 + term;
      }
    }
    __syncthreads();                                    // the batch is read before the next one is staged
  }
  // the sample's length: the largest end column or the last CC row's column
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) max_end = max(max_end, __shfl_xor(max_end, o, 64));
  double mx = fmax(fabs(acc0), fabs(acc1));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) {
    wave_end[wv] = max_end;
    wave_max[wv] = mx;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    max_end = max(max_end, wave_end[w]);
    mx = fmax(mx, wave_max[w]);
  }
  if (n_ccs > 0) max_end = max(max_end, min(max(ccs[2 * (co + n_ccs - 1)], 0), T));
  const long long L = v.len[max_end];
  if (i0 >= L) acc0 = 0.0;                              // no note reaches beyond L (samp[k] <= len[k]); written as zeros all the same
  if (i0 + 1 >= L) acc1 = 0.0;
  if (i0 + 1 < cap) {                                   // cap is even: a pair is inside or outside as a whole
    double2 o;
    o.x = acc0;
    o.y = acc1;
    *(double2*)(wave + (size_t)n * cap + i0) = o;
  }
  if (tid == 0) v.part[(size_t)n * n_chunks(cap) + blockIdx.x] = mx;
  if (tid == 0 && blockIdx.x == 0) v.part[(size_t)gridDim.y * n_chunks(cap) + n] = (double)L;  // exact: L < 2^31
}

// grid N, block 256
__global__ __launch_bounds__(THREADS) void peak_kernel(int T, const int64_t* __restrict__ counts, long long cap, int64_t* __restrict__ lengths,
                                                       double* __restrict__ peak, int32_t* __restrict__ silent, void* ws) {
  __shared__ double wave_max[WAVES];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const View v = view(ws, T, cap);
  const long long nc = n_chunks(cap);
  double mx = 0.0;
  for (long long c = tid; c < nc; c += THREADS) mx = fmax(mx, v.part[(size_t)n * nc + c]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) wave_max[wv] = mx;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 0; w < WAVES; ++w) mx = fmax(mx, wave_max[w]);
    peak[n] = mx;
    lengths[n] = (int64_t)v.part[(size_t)gridDim.x * nc + n];
    silent[n] = (counts[4 * n] <= 0 || !(mx > 0.0)) ? 1 : 0;
  }
}

struct __attribute__((packed, aligned(4))) Pcm8 {
  int16_t s[8];
};

// grid (ceil(cap / 2048), N), block 256: eight samples per thread
__global__ __launch_bounds__(THREADS) void pcm_kernel(const double* __restrict__ wave, const int64_t* __restrict__ lengths,
                                                      const double* __restrict__ peak, long long cap, int format, int rate,
                                                      uint8_t* __restrict__ out) {
  const int n = blockIdx.y, tid = threadIdx.x;
  const long long i0 = (long long)blockIdx.x * PCM_CHUNK + 8 * tid;
  const long long L = min(max((long long)lengths[n], 0ll), cap);
  const double pk = peak[n];
  const bool sounding = pk > 0.0;
  const size_t stride = 44 + 2 * (size_t)cap;
  if (format == 1 && blockIdx.x == 0 && tid == 0) {     // the header the wave module writes: mono, 16 bit
    uint8_t* h = out + (size_t)n * stride;
    const unsigned data = 2u * (unsigned)L;
    const unsigned words[11] = {0x46464952u, 36u + data, 0x45564157u, 0x20746d66u, 16u, 0x00010001u, (unsigned)rate, 2u * (unsigned)rate,
                                0x00100002u, 0x61746164u, data};
    for (int i = 0; i < 11; ++i) *(unsigned*)(h + 4 * i) = words[i];
  }
  if (i0 >= cap) return;                                // cap is a multiple of 8
  const double2* src = (const double2*)(wave + (size_t)n * cap + i0);
  double x[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double2 d = src[j];
    x[2 * j] = d.x;
    x[2 * j + 1] = d.y;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = (sounding && i0 + j < L) ? x[j] / pk : 0.0;
  if (format == 0) {
    float4* dst = (float4*)((float*)out + (size_t)n * cap + i0);
    dst[0] = make_float4((float)x[0], (float)x[1], (float)x[2], (float)x[3]);
    dst[1] = make_float4((float)x[4], (float)x[5], (float)x[6], (float)x[7]);
  } else {
    Pcm8 p;
#pragma unroll
    for (int j = 0; j < 8; ++j) p.s[j] = (int16_t)(int)rint(x[j] * 32767.0);
    *(Pcm8*)(out + (size_t)n * stride + 44 + 2 * (size_t)i0) = p;
  }
}
}  // namespace synth
}  // namespace rgm

using namespace rgm;

extern "C" size_t rgm_synth_workspace(int N, int T, long long cap) {
  if (N <= 0 || N > synth::MAX_N || T < 1 || T > synth::MAX_T || cap < 8 || cap > synth::MAX_LEN) return 0;
  return synth::table_bytes(T, cap) + ((size_t)N * synth::n_chunks(cap) + N) * 8;
}

static int synth_check_sizes(const char* what, int N, int T, long long cap, const void* ws, size_t ws_bytes) {
  RGM_REQUIRE(N > 0 && N <= synth::MAX_N, "%s: N = %d (1 .. 65535 samples per call)", what, N);
  RGM_REQUIRE(T >= 1 && T <= synth::MAX_T, "%s: T = %d columns (1 .. %d)", what, T, synth::MAX_T);
  RGM_REQUIRE(cap >= 8 && cap <= synth::MAX_LEN && cap % 8 == 0, "%s: cap = %lld audio samples per row (a multiple of 8 below 2^31)", what, cap);
  if (ws_bytes != (size_t)-1) {
    const size_t need = rgm_synth_workspace(N, T, cap);
    if (!ws || ws_bytes < need) {
      set_error("%s: workspace of %zu bytes, %zu needed", what, ws ? ws_bytes : (size_t)0, need);
      return RGM_ERR_WORKSPACE;
    }
    RGM_REQUIRE(((uintptr_t)ws & 15) == 0, "%s: the workspace must be 16-byte aligned", what);
  }
  return RGM_OK;
}

extern "C" int rgm_synth_render(int N, int T, const int32_t* notes, long long notes_rows, const int64_t* note_off, const int32_t* ccs,
                                long long ccs_rows, const int64_t* cc_off, const int64_t* counts, double audio_fs, const int64_t* samp_host, const int64_t* len_host,
                                const double* omega_host, const double* fade_host, int F, double* wave, long long cap, int64_t* lengths,
                                double* peak, int32_t* silent, void* ws, size_t ws_bytes, void* stream) {
  RGM_REQUIRE(note_off && cc_off && counts && samp_host && len_host && omega_host && wave && lengths && peak && silent, "synth_render: bad arguments");
  RGM_REQUIRE(notes_rows >= 0 && ccs_rows >= 0 && (notes || notes_rows == 0) && (ccs || ccs_rows == 0),
              "synth_render: an array of %lld note rows / %lld CC rows needs its pointer", notes_rows, ccs_rows);
  RGM_REQUIRE(((uintptr_t)notes & 15) == 0 && ((uintptr_t)ccs & 7) == 0, "synth_render: note rows must be 16-byte aligned, CC rows 8-byte");
  RGM_REQUIRE(audio_fs > 0.0 && audio_fs < 2147483648.0, "synth_render: audio_fs = %g (positive, below 2^31)", audio_fs);
  RGM_REQUIRE(N > 0 && N <= synth::MAX_N, "synth_render: N = %d (1 .. 65535 samples per call)", N);
  RGM_REQUIRE(T >= 1 && T <= synth::MAX_T, "synth_render: T = %d columns (1 .. %d)", T, synth::MAX_T);
  RGM_REQUIRE(samp_host[0] >= 0 && len_host[0] >= 0, "synth_render: the tables start at %lld and %lld (not below 0)", (long long)samp_host[0],
              (long long)len_host[0]);
  for (int k = 0; k < T; ++k)
    RGM_REQUIRE(samp_host[k + 1] >= samp_host[k] && len_host[k + 1] >= len_host[k], "synth_render: a table decreases from column %d to %d", k, k + 1);
  RGM_REQUIRE(len_host[T] <= synth::MAX_LEN && samp_host[T] <= synth::MAX_LEN, "synth_render: a waveform of %lld samples (below 2^31)",
              (long long)len_host[T]);
  for (int k = 0; k <= T; ++k)
    RGM_REQUIRE(samp_host[k] <= len_host[k], "synth_render: column %d starts at sample %lld, behind the length %lld of a waveform ending there", k,
                (long long)samp_host[k], (long long)len_host[k]);
  RGM_REQUIRE(cap >= len_host[T], "synth_render: cap = %lld audio samples per row, the tables need %lld", cap, (long long)len_host[T]);
  RGM_TRY(synth_check_sizes("synth_render", N, T, cap, ws, ws_bytes));
  RGM_REQUIRE(F >= 0 && F <= synth::fade_cap(cap) && (F == 0 || fade_host), "synth_render: a fade of %d samples (0 .. %lld for this cap)", F,
              synth::fade_cap(cap));
  RGM_REQUIRE(((uintptr_t)wave & 15) == 0, "synth_render: the waveform rows must be 16-byte aligned");
  RGM_REQUIRE(synth::n_chunks(cap) <= 0x7fffffffll, "synth_render: too many chunks");
  hipStream_t s = (hipStream_t)stream;
  long long* tab = (long long*)ws;
  RGM_CHECK_HIP(hipMemcpyAsync(tab, samp_host, (size_t)(T + 1) * 8, hipMemcpyHostToDevice, s));
  RGM_CHECK_HIP(hipMemcpyAsync(tab + (T + 1), len_host, (size_t)(T + 1) * 8, hipMemcpyHostToDevice, s));
  RGM_CHECK_HIP(hipMemcpyAsync(tab + 2 * (T + 1), omega_host, 128 * 8, hipMemcpyHostToDevice, s));
  if (F > 0) RGM_CHECK_HIP(hipMemcpyAsync(tab + 2 * (T + 1) + 128, fade_host, (size_t)F * 8, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(synth::render_kernel, dim3((unsigned)synth::n_chunks(cap), N), dim3(synth::THREADS), 0, s, T, notes, notes_rows, note_off, ccs,
                     ccs_rows, cc_off, counts, audio_fs, F, wave, cap, ws);
  RGM_LAUNCH_CHECK();
  hipLaunchKernelGGL(synth::peak_kernel, dim3(N), dim3(synth::THREADS), 0, s, T, counts, cap, lengths, peak, silent, ws);
  RGM_LAUNCH_CHECK();
  return RGM_OK;
}

extern "C" int rgm_synth_pcm(int N, const double* wave, const int64_t* lengths, const double* peak, long long cap, int format, int rate, void* out,
                             void* stream) {
  RGM_REQUIRE(wave && lengths && peak && out, "synth_pcm: bad arguments");
  RGM_REQUIRE(format == 0 || format == 1, "synth_pcm: format %d (0: float32 rows, 1: 16-bit WAV files)", format);
  RGM_REQUIRE(format == 0 || rate > 0, "synth_pcm: a WAV header needs a positive integer rate, got %d", rate);
  RGM_TRY(synth_check_sizes("synth_pcm", N, 1, cap, nullptr, (size_t)-1));
  RGM_REQUIRE(format == 0 || 44 + 2 * cap <= 0xffffffffll, "synth_pcm: a WAV file of %lld samples", cap);
  RGM_REQUIRE(((uintptr_t)wave & 15) == 0 && ((uintptr_t)out & 15) == 0, "synth_pcm: the rows must be 16-byte aligned");
  hipLaunchKernelGGL(synth::pcm_kernel, dim3((unsigned)((cap + synth::PCM_CHUNK - 1) / synth::PCM_CHUNK), N), dim3(synth::THREADS), 0,
                     (hipStream_t)stream, wave, lengths, peak, cap, format, rate, (uint8_t*)out);
  RGM_LAUNCH_CHECK();
  return RGM_OK;
}
