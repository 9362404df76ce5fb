"""Config loading, final decode to the uint8 piano roll and rule-loss reporting -- reference API
(guided_diffusion/midi_util.py:26-64, :96-124).  MIDI writing / plotting of the reference need mido +
the vendored pretty_midi fork (pure I/O, out of scope); save_piano_roll_midi stores .npy rolls instead and
hands over to an optional user hook."""
import os
from types import SimpleNamespace

import numpy as np
import pandas as pd
import torch
import yaml

from music_rule_guidance.rule_maps import FUNC_DICT, LOSS_DICT
from music_rule_guidance.music_rules import IND2KEY, KEY_DICT, MAX_PIANO, MIN_PIANO  # noqa: F401  (re-exported like the reference)
from rgm import native as _rgm


def dict_to_obj(d):
    """Nested dicts -> attribute namespaces (lists keep their element types)."""
    if isinstance(d, list):
        return [dict_to_obj(x) if isinstance(x, dict) else x for x in d]
    if isinstance(d, dict):
        return SimpleNamespace(**{k: dict_to_obj(v) for k, v in d.items()})
    return d


def load_config(filename):
    with open(filename, "r") as f:
        return dict_to_obj(yaml.safe_load(f))


# The final decode is the one place where a float becomes an INTEGER (truncating cast + background threshold): a roll value within the
# decoder's arithmetic error of a boundary flips.  It runs once per sample, outside the step loop, so it always takes the exact-fp32
# MFMA decoder (v_mfma_f32_32x32x2_f32: the reference's own arithmetic up to summation order), whatever the sampling loop ran in --
# measured on the reference's 50-step golden: 250 -> the fp32 level of mismatching entries of 786 432 (docs/rounds/r06.md).
# RGM_FINAL_DECODE_EXACT=0 / exact=False: the process-wide arithmetic instead (A/B runs).
FINAL_DECODE_EXACT = os.environ.get("RGM_FINAL_DECODE_EXACT", "1") != "0"


@torch.no_grad()
def decode_sample_for_midi(sample, embed_model=None, scale_factor=1., threshold=-0.95, exact=None):
    """Latent batch -> uint8 piano roll (B, 128, T, 3) in [0, 127].

    With the native AutoencoderKL the whole chain (1/scale_factor, square gather, decoder, background
    threshold, (x+1)*63.5 clamp, truncating cast, layout change) is one decode call; other embed models are
    driven through tensor views and only the final quantisation runs in the HIP kernel.
    exact (default FINAL_DECODE_EXACT = True): run this decode in exact-fp32 arithmetic (reference midi_util.py:42-64 is fp32)."""
    if exact is None:
        exact = FINAL_DECODE_EXACT
    if embed_model is not None and hasattr(embed_model, "decode_latent") and sample.shape[-2] > sample.shape[-1]:
        with _rgm.gemm_precision_scope("fp32" if exact else None):
            return embed_model.decode_latent(sample, scale_factor, want_u8=True, threshold=threshold, want_float=False)
    sample = sample / scale_factor
    if embed_model is not None:
        h, w = sample.shape[-2:]
        if h > w:
            sample = sample.permute(0, 1, 3, 2)
        n_lat = sample.shape[-1] // sample.shape[-2]
        if h >= w:
            sample = torch.cat(torch.chunk(sample, n_lat, dim=-1), dim=0)
        sample = embed_model.decode(sample)
        if h >= w:
            sample = torch.cat(torch.chunk(sample, n_lat, dim=0), dim=-1)
    _rgm.require_cuda(sample)
    roll = sample.to(torch.float32).contiguous()
    B, Cc, P, T = roll.shape
    assert Cc == 3 and P == 128, "quantise kernel expects (B,3,128,T)"
    out = torch.empty((B, 128, T, 3), dtype=torch.uint8, device=roll.device)
    with torch.cuda.device(roll.device):
        _rgm.check(_rgm.lib.rgm_quantise_roll(_rgm.ptr(roll), _rgm.ptr(out), B, T, float(threshold), _rgm.current_stream()))
    return out


# note-density class boundaries / centres used to shift an extracted density by whole classes (reference midi_util.py:20-23)
VERTICAL_ND_BOUNDS = [1.29, 2.7578125, 3.61, 4.4921875, 5.28125, 6.1171875, 7.22]
VERTICAL_ND_CENTER = [0.56, 2.0239, 3.1839, 4.0511, 4.8867, 5.6992, 6.6686, 7.77]
HORIZONTAL_ND_BOUNDS = [1.8, 2.6, 3.2, 3.6, 4.4, 4.8, 5.8]
HORIZONTAL_ND_CENTER = [1.4, 2.2000, 2.9, 3.4, 4.0, 4.6, 5.3, 6.3]

_MIDI_WRITER = None
_MIDI_READER = None


def register_midi_reader(fn):
    """fn(path, fs) -> piano roll (3,128,T) with values in [0,127] (the reference: pretty_midi + get_full_piano_roll,
    scripts/edit.py:170-171) -- plug in a MIDI reader for the editing CLI."""
    global _MIDI_READER
    _MIDI_READER = fn


def read_midi_piano_roll(path, fs=100):
    """MIDI file -> (3,128,T) [velocity | onset | pedal] roll.  Default: the built-in SMF reader + get_full_piano_roll's logic
    (music_rule_guidance.piano_roll_to_chord; all three channels pinned to the reference's pretty_midi fork, tests/golden/midi_rolls.npz);
    register_midi_reader replaces it, e.g. with the fork itself."""
    if _MIDI_READER is not None:
        return np.asarray(_MIDI_READER(path, fs), dtype=np.float32)
    from music_rule_guidance.piano_roll_to_chord import SimpleMIDI, midi_to_full_piano_roll
    return midi_to_full_piano_roll(SimpleMIDI(path), fs=fs)


def register_midi_writer(fn):
    """fn(piano_roll_uint8 (C,128,T), path, fs) -- plug in a MIDI writer (the reference uses its pretty_midi fork)."""
    global _MIDI_WRITER
    _MIDI_WRITER = fn


MIDI_BACKENDS = ("host", "device")
MIDI_MAX_T = 32768
_TICK_TABLES = {}


def midi_tick_table(T, fs=100):
    """The MIDI tick of every column boundary 0 .. T of a roll at fs columns per second: int32 (T + 1,), entry k =
    SimpleMIDI.time_to_tick(k / fs) -- the host writer's own conversion, Python's half-to-even round included, so the kernels of
    csrc/midi.hip never form a time.  Cached per (T, fs), read-only.  The device path needs a table that rises by at least 2 from entry to
    entry (the column order is then the tick order, and the extra off of a zero-length note, one tick behind its on, falls before the next
    column): 440 / fs >= 2, i.e. fs <= 220.  Any other fs raises ValueError.  Runs on the host."""
    from music_rule_guidance.piano_roll_to_chord import SimpleMIDI
    T = int(T)
    if not 1 <= T <= MIDI_MAX_T:
        raise ValueError(f"MIDI tick tables cover 1 .. {MIDI_MAX_T} columns, got {T}")
    if not fs > 0:
        raise ValueError(f"fs must be positive, got {fs}")
    key = (T, fs)
    tab = _TICK_TABLES.get(key)
    if tab is None:
        pm = SimpleMIDI()
        tab = np.array([pm.time_to_tick(k / fs) for k in range(T + 1)], dtype=np.int64)
        if int(np.diff(tab).min()) < 2 or int(tab[-1]) >= 1 << 21:
            raise ValueError(f"the device MIDI writer needs ticks that rise by at least 2 per column and stay below 2^21: fs = {fs} gives a "
                             f"smallest step of {int(np.diff(tab).min())} and a last tick of {int(tab[-1])} (fs <= 220 serves); use the host writer")
        tab = np.ascontiguousarray(tab.astype(np.int32))
        tab.setflags(write=False)
        _TICK_TABLES[key] = tab
    return tab


def rolls_to_midi_bytes(roll_u8, fs=100, first_column_onsets=True, program=0):
    """uint8 device rolls, channel-first (N, C, 128, T) or the (N, 128, T, C) tensor of decode_sample_for_midi -> a list of N `bytes`, each
    the Standard MIDI File piano_roll_to_pretty_midi(roll).write() makes of that roll (first_column_onsets: with save_piano_roll_midi's forced
    onsets in column 0), built by csrc/midi.hip and fetched with one device-to-host copy.  The rolls are not written to.  ValueError for an
    fs the device path does not serve (midi_tick_table)."""
    from music_rule_guidance import music_rules
    ev = music_rules.midi_events_raw(roll_u8, fs=fs, first_column_onsets=first_column_onsets, program=program)
    blob = ev["bytes"].cpu().numpy().tobytes()
    ends = np.cumsum(ev["sizes_host"][:, 3])
    return [blob[int(e - s):int(e)] for s, e in zip(ev["sizes_host"][:, 3], ends)]


WAV_BACKENDS = ("off", "device")
_SYNTH_TABLES = {}


def synth_host_tables(T, fs=100, audio_fs=44100):
    """piano_roll_to_chord.synth_tables(T, fs, audio_fs), contiguous, read-only and cached per (T, fs, audio_fs): the host tables
    rgm_synth_render copies on the caller's stream (they must outlive that copy, which the cache sees to).  ValueError for an fs /
    audio_fs the tables refuse."""
    from music_rule_guidance.piano_roll_to_chord import synth_tables
    key = (int(T), fs, audio_fs)
    tabs = _SYNTH_TABLES.get(key)
    if tabs is None:
        tabs = tuple(np.ascontiguousarray(t) for t in synth_tables(T, fs, audio_fs))
        for t in tabs:
            t.setflags(write=False)
        if len(_SYNTH_TABLES) >= 64:
            _SYNTH_TABLES.clear()
        _SYNTH_TABLES[key] = tabs
    return tabs


def _synth_render(roll_u8, fs, audio_fs, first_column_onsets):
    """-> (wave (N, cap) float64, lengths (N,) int64, peak (N,) float64, silent (N,) int32, cap): the render launches of csrc/synth.hip over
    the note and CC rows csrc/midi.hip leaves on the device"""
    from music_rule_guidance import music_rules
    if not audio_fs > 0:
        raise ValueError(f"audio_fs must be positive, got {audio_fs}")
    ev = music_rules.midi_events_raw(roll_u8, fs=fs, first_column_onsets=first_column_onsets)
    N = ev["counts"].shape[0]
    T = music_rules._note_stats_layout(roll_u8)[3]
    samp, length, omega, fade = synth_host_tables(T, fs, audio_fs)
    cap = (int(length[T]) + 7) // 8 * 8
    dev = ev["counts"].device
    wave = torch.empty((N, cap), dtype=torch.float64, device=dev)
    lengths = torch.empty(N, dtype=torch.int64, device=dev)
    peak = torch.empty(N, dtype=torch.float64, device=dev)
    silent = torch.empty(N, dtype=torch.int32, device=dev)
    notes, ccs = ev["notes"], ev["ccs"]
    with torch.cuda.device(dev):
        nbytes = _rgm.lib.rgm_synth_workspace(N, T, cap)
        if nbytes == 0:
            raise ValueError(f"the device synthesiser does not serve {N} rolls of {T} columns with {cap} audio samples each")
        ws = torch.empty((nbytes + 15) // 16 * 2, dtype=torch.int64, device=dev)
        _rgm.check(_rgm.lib.rgm_synth_render(
            N, T, _rgm.ptr(notes) if notes.numel() else None, notes.shape[0], _rgm.ptr(ev["note_offsets"]),
            _rgm.ptr(ccs) if ccs.numel() else None, ccs.shape[0], _rgm.ptr(ev["cc_offsets"]), _rgm.ptr(ev["counts"]), float(audio_fs),
            samp.ctypes.data, length.ctypes.data, omega.ctypes.data, fade.ctypes.data if len(fade) else None, len(fade), _rgm.ptr(wave), cap,
            _rgm.ptr(lengths), _rgm.ptr(peak), _rgm.ptr(silent), _rgm.ptr(ws), ws.numel() * 8, _rgm.current_stream()))
    return wave, lengths, peak, silent, cap


def rolls_to_audio(roll_u8, fs=100, audio_fs=44100, first_column_onsets=True, normalize=True, dtype=torch.float32):
    """uint8 device rolls in either layout rolls_to_midi_bytes takes -> (audio (N, cap) device tensor, lengths (N,) int64, silent (N,) bool):
    row n holds, in its first lengths[n] entries, what the reference's piano_roll_to_pretty_midi(roll, fs) followed by its pretty_midi
    fork's .synthesize(fs=audio_fs) returns for that roll -- every note one sine under exp(-t) with a 0.1 s linear fade-out, scaled by its
    velocity, the sum divided by its largest magnitude -- and zeros behind; cap is the length a roll with an event in its last column
    would have, rounded up to a multiple of 8.  Built by csrc/synth.hip; the host partner is piano_roll_to_chord.synthesize_roll.
    normalize=False: the raw sum (Instrument.synthesize); dtype torch.float64 with normalize=False hands out the kernel's own rows.
    ONE departure from the reference: a roll whose waveform is zero throughout (no notes, or none long enough to sound) gives zeros and
    silent = True where the reference divides 0 by 0 and returns NaNs.  The rolls are not written to.  ValueError for an fs / audio_fs
    the tables refuse (midi_tick_table, synth_host_tables)."""
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"audio comes as torch.float32 or torch.float64, got {dtype}")
    wave, lengths, peak, silent, cap = _synth_render(roll_u8, fs, audio_fs, first_column_onsets)
    if not normalize:
        audio = wave if dtype == torch.float64 else wave.to(dtype)
    elif dtype == torch.float32:
        audio = torch.empty((wave.shape[0], cap), dtype=torch.float32, device=wave.device)
        with torch.cuda.device(wave.device):
            _rgm.check(_rgm.lib.rgm_synth_pcm(wave.shape[0], _rgm.ptr(wave), _rgm.ptr(lengths), _rgm.ptr(peak), cap, 0, 0, _rgm.ptr(audio),
                                              _rgm.current_stream()))
    else:
        audio = torch.where((peak > 0)[:, None], wave / peak.clamp_min(torch.finfo(torch.float64).tiny)[:, None], torch.zeros_like(wave))
    return audio, lengths, silent.bool()


def rolls_to_wav_bytes(roll_u8, fs=100, audio_fs=44100, first_column_onsets=True):
    """uint8 device rolls -> a list of N `bytes`, each a mono 16-bit PCM WAV file of rolls_to_audio's normalised waveform: samples
    rint(x * 32767) behind the 44-byte header the standard library's wave module writes (piano_roll_to_chord.wav_bytes of the same
    waveform).  Rendered and quantised on the device without a host read in between, fetched with one device-to-host copy.  audio_fs
    must be a whole number: it goes into the header."""
    if int(audio_fs) != audio_fs:
        raise ValueError(f"a WAV header holds a whole sample rate, got {audio_fs}")
    wave, lengths, peak, silent, cap = _synth_render(roll_u8, fs, audio_fs, first_column_onsets)
    N, stride = wave.shape[0], 44 + 2 * cap
    out = torch.empty(N * stride, dtype=torch.uint8, device=wave.device)
    with torch.cuda.device(wave.device):
        _rgm.check(_rgm.lib.rgm_synth_pcm(N, _rgm.ptr(wave), _rgm.ptr(lengths), _rgm.ptr(peak), cap, 1, int(audio_fs), _rgm.ptr(out),
                                          _rgm.current_stream()))
    blob = out.cpu().numpy().tobytes()                  # the one copy out
    files = []
    for n in range(N):
        size = 44 + int.from_bytes(blob[n * stride + 40:n * stride + 44], "little")      # 2 * lengths[n], from the file's own header
        files.append(blob[n * stride:n * stride + size])
    return files


MIDI_READERS = ("host", "device")
MIDI_READ_STATUS = {0: "accepted", 1: "not a Standard MIDI File", 2: "SMPTE or zero time division", 3: "bad or overrunning track chunk",
                    4: "data ends inside a message", 5: "data byte >= 0x80 in a channel message", 6: "more than 2048 tempo entries",
                    7: "no note reaches the first column", 8: "a tick beyond 2^40 or more than 2^31 columns", 9: "track table too small"}
MIDI_READ_MAX_FILES = 65535
MIDI_READ_MAX_BYTES = 1 << 30


def pack_midi_files(files):
    """Paths or `bytes` -> (blob, offsets, total_tracks) on the host: the files back to back in a uint8 array whose length is padded with
    zeros to a multiple of 16 (plus 16) so that a 16-byte load of any file byte stays inside it, N + 1 int64 offsets, and the sum of the
    track counts of the 14-byte headers that begin with MThd -- what sizes the workspace of csrc/midi_read.hip.  Runs on the host."""
    datas = []
    for f in files:
        if isinstance(f, (bytes, bytearray, memoryview)):
            datas.append(bytes(f))
        else:
            with open(f, "rb") as fh:
                datas.append(fh.read())
    if not 1 <= len(datas) <= MIDI_READ_MAX_FILES:
        raise ValueError(f"the device MIDI reader takes 1 .. {MIDI_READ_MAX_FILES} files per call, got {len(datas)}")
    offsets = np.zeros(len(datas) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(d) for d in datas])
    total = int(offsets[-1])
    if not 1 <= total <= MIDI_READ_MAX_BYTES:
        raise ValueError(f"the device MIDI reader takes 1 .. 2^30 bytes per call, got {total}")
    blob = np.zeros((total + 15) // 16 * 16 + 16, dtype=np.uint8)
    blob[:total] = np.frombuffer(b"".join(datas), dtype=np.uint8)
    tracks = sum(int.from_bytes(d[10:12], "big") for d in datas if len(d) >= 14 and d[:4] == b"MThd")
    return blob, offsets, tracks


def _midi_read_scan(files, fs, want_events):
    """Pack, upload and scan: the tensors both public readers share.  One host-to-device copy of the blob, one of the offsets."""
    if not fs > 0:
        raise ValueError(f"fs must be positive, got {fs}")
    blob_h, offsets_h, tracks = pack_midi_files(files)
    N, total = len(offsets_h) - 1, int(offsets_h[-1])
    dev = torch.device("cuda", torch.cuda.current_device())
    blob = torch.from_numpy(blob_h).to(dev)
    offsets = torch.from_numpy(offsets_h).to(dev)
    r = {"N": N, "total": total, "tracks": tracks, "blob": blob, "offsets": offsets,
         "status": torch.empty(N, dtype=torch.int32, device=dev), "counts": torch.empty((N, 4), dtype=torch.int64, device=dev),
         "columns": torch.empty(N, dtype=torch.int64, device=dev)}
    notes = ccs = note_off = cc_off = None
    if want_events:                                      # rows bounded by bytes: no host read before the arrays exist
        notes = torch.zeros((total // 6 + 1, 8), dtype=torch.int64, device=dev)
        ccs = torch.zeros((total // 3 + 1, 5), dtype=torch.int64, device=dev)
        note_off = torch.empty(N + 1, dtype=torch.int64, device=dev)
        cc_off = torch.empty(N + 1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        nbytes = _rgm.lib.rgm_midi_read_workspace(N, total, tracks)
        if nbytes == 0:
            raise ValueError(f"the device MIDI reader does not serve {N} files of {total} bytes with {tracks} tracks")
        ws = torch.empty((nbytes + 15) // 16 * 2, dtype=torch.int64, device=dev)
        _rgm.check(_rgm.lib.rgm_midi_read_scan(_rgm.ptr(blob), _rgm.ptr(offsets), N, total, tracks, float(fs), _rgm.ptr(r["status"]),
                                               _rgm.ptr(r["counts"]), _rgm.ptr(r["columns"]), _rgm.ptr(note_off), _rgm.ptr(cc_off),
                                               _rgm.ptr(notes), 0 if notes is None else notes.shape[0], _rgm.ptr(ccs),
                                               0 if ccs is None else ccs.shape[0], _rgm.ptr(ws), ws.numel() * 8, _rgm.current_stream()))
    r.update(ws=ws, notes=notes, ccs=ccs, note_offsets=note_off, cc_offsets=cc_off)
    return r


def _midi_file_name(files, i):
    return f"file {i}" if isinstance(files[i], (bytes, bytearray, memoryview)) else str(files[i])


def midi_files_to_rolls(files, fs=100, columns=None, start_column=0, dtype=torch.uint8, strict=True):
    """A batch of Standard MIDI Files (paths or `bytes`) -> device tensors {"roll" (N, 3, 128, T) [velocity | onset | pedal], "columns" (N,)
    int64: every file's own length in columns, "status" (N,) int32 (MIDI_READ_STATUS), "overflow" (N,) int64}: what
    midi_to_full_piano_roll(SimpleMIDI(file), fs) gives, cut to columns [start_column, start_column + T) and zero beyond the file's own end,
    built by csrc/midi_read.hip.  dtype torch.float32: the host's values exactly; torch.uint8: saturating at 255 (the host's velocity sum of
    overlapping notes is unclipped), `overflow` counting the saturated cells.  columns=None: T is the batch maximum (at least 1) -- the one
    host read, of N sizes.  strict: ValueError naming the first refused file and its status; otherwise a refused file has a zero roll."""
    if dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"rolls come as torch.uint8 or torch.float32, got {dtype}")
    if start_column < 0 or (columns is not None and columns < 1):
        raise ValueError(f"a window needs start_column >= 0 and columns >= 1, got {start_column} and {columns}")
    files = list(files)
    r = _midi_read_scan(files, fs, False)
    if strict:
        bad = torch.nonzero(r["status"]).flatten().cpu().numpy()
        if len(bad):
            code = int(r["status"][int(bad[0])])
            raise ValueError(f"{_midi_file_name(files, int(bad[0]))}: refused by the device MIDI reader, status {code} ({MIDI_READ_STATUS[code]})")
    T = int(columns) if columns is not None else max(1, int(r["columns"].max()) - int(start_column))
    dev = r["blob"].device
    roll = torch.empty((r["N"], 3, 128, T), dtype=dtype, device=dev)
    overflow = torch.zeros(r["N"], dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _rgm.check(_rgm.lib.rgm_midi_read_rolls(r["N"], r["total"], r["tracks"], float(fs), int(start_column), T, int(dtype == torch.uint8),
                                                _rgm.ptr(roll), _rgm.ptr(overflow), _rgm.ptr(r["ws"]), r["ws"].numel() * 8, _rgm.current_stream()))
    return {"roll": roll, "columns": r["columns"], "status": r["status"], "overflow": overflow}


def midi_files_to_events(files, fs=100):
    """A batch of Standard MIDI Files -> device tensors: status (N,) int32, counts (N, 4) int64 [notes, control changes, tempo entries,
    instruments], columns (N,) int64; notes (sum, 6) int64 rows (instrument, channel, pitch, velocity, start tick, end tick) with note_times
    (sum, 2) float64 (start, end in seconds), in (instrument, order of the note-offs) order; ccs (sum, 4) int64 rows (instrument, number, value,
    tick) with cc_times (sum,) float64, in (instrument, event) order; note_offsets, cc_offsets (N + 1,) int64.  What SimpleMIDI(file) holds;
    a refused file has no rows.  One host read of the two totals trims the arrays."""
    files = list(files)
    r = _midi_read_scan(files, fs, True)
    n, c = int(r["note_offsets"][-1]), int(r["cc_offsets"][-1])
    notes, ccs = r["notes"][:n], r["ccs"][:c]
    return {"status": r["status"], "counts": r["counts"], "columns": r["columns"], "notes": notes[:, :6].contiguous(),
            "note_times": notes[:, 6:8].contiguous().view(torch.float64), "ccs": ccs[:, :4].contiguous(),
            "cc_times": ccs[:, 4].contiguous().view(torch.float64), "note_offsets": r["note_offsets"], "cc_offsets": r["cc_offsets"]}


def read_midi_piano_roll_device(path, fs=100, columns=None):
    """read_midi_piano_roll's device counterpart for one file: the float32 (3, 128, T) roll as a device tensor (T = the file's own length, or
    the first `columns` columns, zero-padded); a registered reader still wins, as everywhere."""
    if _MIDI_READER is not None:
        roll = torch.from_numpy(np.asarray(_MIDI_READER(path, fs), dtype=np.float32)).cuda()
        if columns is not None:
            roll = torch.nn.functional.pad(roll[:, :, :columns], (0, max(0, columns - roll.shape[2])))
        return roll
    return midi_files_to_rolls([path], fs=fs, columns=columns, dtype=torch.float32)["roll"][0]


def save_piano_roll_midi(sample, save_dir, fs=100, y=None, save_piano_roll=False, save_ind=0, midi_bytes=None, wav_bytes=None):
    """sample: (B, 3, 128, T) uint8 array (or (B,128,T) / (B,2,128,T)).  Writes sample_<i>[_y_<label>].midi per sample (names
    and event extraction as in the reference :67-93, incl. the forced onsets in the first column) plus the raw roll as
    .npy; register_midi_writer replaces the built-in SMF writer.  save_piano_roll (PNG plots) is not provided.
    midi_bytes: a list of B finished files (rolls_to_midi_bytes of the same rolls while they were on the device) to write instead of running
    the host extraction; a registered writer still takes precedence.
    wav_bytes: a list of B finished WAV files (rolls_to_wav_bytes of the same rolls) written as sample_<i>[_y_<label>].wav beside the .midi."""
    from music_rule_guidance.piano_roll_to_chord import piano_roll_to_pretty_midi
    if midi_bytes is not None and len(midi_bytes) != sample.shape[0]:
        raise ValueError(f"midi_bytes holds {len(midi_bytes)} files for {sample.shape[0]} rolls")
    if wav_bytes is not None and len(wav_bytes) != sample.shape[0]:
        raise ValueError(f"wav_bytes holds {len(wav_bytes)} files for {sample.shape[0]} rolls")
    os.makedirs(save_dir, exist_ok=True)
    for i in range(sample.shape[0]):
        stem = f"sample_{i + save_ind}" + (f"_y_{int(y[i])}" if y is not None else "")
        np.save(os.path.join(save_dir, stem + ".npy"), sample[i])
        if wav_bytes is not None:
            with open(os.path.join(save_dir, stem + ".wav"), "wb") as f:
                f.write(wav_bytes[i])
        if _MIDI_WRITER is not None:
            _MIDI_WRITER(sample[i], os.path.join(save_dir, stem + ".midi"), fs)
            continue
        if midi_bytes is not None:
            with open(os.path.join(save_dir, stem + ".midi"), "wb") as f:
                f.write(midi_bytes[i])
            continue
        cur = np.array(sample[i])
        if cur.ndim == 3 and cur.shape[0] == 3:            # a note sounding in the first column starts there
            cur[1, np.nonzero(cur[0, :, 0])[0], 0] = 127
        piano_roll_to_pretty_midi(cur.astype(np.float32), fs=fs).write(os.path.join(save_dir, stem + ".midi"))


def eval_rule_loss(generated_samples, target_rules):
    """DataFrame with <rule>.target_rule / .gen_rule / .loss columns, one row per sample."""
    results = {}
    B = generated_samples.shape[0]
    for name, target in target_rules.items():
        tl = target.tolist()
        results[name + ".target_rule"] = [tl] if B == 1 else tl
        target = target.to(generated_samples.device)
        if "chord" in name:
            gen, key, corr = FUNC_DICT[name](generated_samples, return_key=True)
            results[name + ".key_str"] = [IND2KEY.get(k, k) for k in key]
            results[name + ".key_corr"] = corr
        else:
            gen = FUNC_DICT[name](generated_samples)
        loss = LOSS_DICT[name](gen, target)
        gl = gen.tolist()
        results[name + ".gen_rule"] = [gl] if B == 1 else gl
        results[name + ".loss"] = loss.tolist() if loss.dim() else [loss.item()]
    return pd.DataFrame(results)
