"""Built-in rule programs on a piano roll in [-1, 1] (N, C, 128, T) -- reference API
(music_rule_guidance/music_rules.py:23-94), arithmetic in librgm_hip.so (csrc/rules.hip).

Semantics kept from the reference, including the surprising ones:
  * only channel 0 is read; rows outside the piano range [21, 108] are set to -1 IN the caller's tensor
    (the reference's piano_like writes through a view), note_density also snaps values < -0.95 to -1 there;
  * batch size 1 squeezes the batch dimension of the result;
  * note_density returns [vertical windows..., horizontal windows...] with horizontal / horizontal_scale.
CPU tensors are accepted (the CLI evaluates final rolls from numpy): they are staged to the HIP device,
processed there, and the in-place writes are copied back -- the computation never runs on the CPU.
"""
import ctypes

import numpy as np
import torch

from rgm import native as _rgm

VERTICAL_ND_BOUNDS = [1.29, 2.7578125, 3.61, 4.4921875, 5.28125, 6.1171875, 7.22]
VERTICAL_ND_CENTER = [0.56, 2.0239, 3.1839, 4.0511, 4.8867, 5.6992, 6.6686, 7.77]
HORIZONTAL_ND_BOUNDS = [1.8, 2.6, 3.2, 3.6, 4.4, 4.8, 5.8]
HORIZONTAL_ND_CENTER = [1.4, 2.2000, 2.9, 3.4, 4.0, 4.6, 5.3, 6.3]
MIN_PIANO, MAX_PIANO, OFF = 21, 108, -1


def _stage(piano_roll):
    """-> (device tensor the kernels may write, write-back callable)."""
    if piano_roll.dim() != 4 or piano_roll.shape[2] != 128:
        raise ValueError(f"piano roll must be (N, C, 128, T), got {tuple(piano_roll.shape)}")
    if piano_roll.is_cuda and piano_roll.is_contiguous() and piano_roll.dtype == torch.float32:
        return piano_roll, (lambda d: None)
    if not torch.cuda.is_available():
        raise _rgm.RgmError("rule kernels need a HIP device (no CPU fallback in the product path)")
    dev = piano_roll.device if piano_roll.is_cuda else torch.device("cuda", torch.cuda.current_device())
    d = piano_roll.detach().to(device=dev, dtype=torch.float32).contiguous()

    def back(dd):
        with torch.no_grad():
            piano_roll[:, :1].copy_(dd[:, :1].to(piano_roll.device, piano_roll.dtype))
    return d, back


def piano_like(x):
    x[:, :, :MIN_PIANO, :] = OFF
    x[:, :, MAX_PIANO + 1:, :] = OFF
    return x


def total_pitch_class_histogram(piano_roll):
    d, back = _stage(piano_roll)
    N, Cc, _, T = d.shape
    out = torch.empty((N, 12), dtype=torch.float32, device=d.device)
    scratch = torch.empty((N, 128), dtype=torch.float32, device=d.device)
    with torch.cuda.device(d.device):
        _rgm.check(_rgm.lib.rgm_rule_pitch_hist(_rgm.ptr(d), _rgm.ptr(out), _rgm.ptr(scratch), N, Cc, T, _rgm.current_stream()))
    back(d)
    out = out.to(piano_roll.device)
    return out.squeeze(0) if N == 1 else out


def note_density(piano_roll, interval=128, quantize_factor=1, horizontal_scale=5):
    if quantize_factor != 1:
        raise NotImplementedError("quantize_factor != 1 is unused by the sampling configs")
    d, back = _stage(piano_roll)
    N, Cc, _, T = d.shape
    out = torch.empty((N, 2 * (T // interval)), dtype=torch.float32, device=d.device)
    with torch.cuda.device(d.device):
        _rgm.check(_rgm.lib.rgm_rule_note_density(_rgm.ptr(d), _rgm.ptr(out), N, Cc, T, int(interval), float(horizontal_scale),
                                                  _rgm.current_stream()))
    back(d)
    out = out.to(piano_roll.device)
    return out.squeeze() if N == 1 else out


_BOUNDS = {}


def note_density_class(piano_roll, interval=128, quantize_factor=1, horizontal_scale=1):
    nd = note_density(piano_roll, interval=interval, quantize_factor=quantize_factor, horizontal_scale=horizontal_scale)
    dev = nd.device if nd.is_cuda else torch.device("cuda", torch.cuda.current_device())
    key = (str(dev), float(horizontal_scale))
    if key not in _BOUNDS:
        _BOUNDS[key] = (torch.tensor(VERTICAL_ND_BOUNDS, device=dev),
                        torch.tensor(HORIZONTAL_ND_BOUNDS, device=dev) / horizontal_scale)
    vb, hb = _BOUNDS[key]
    half = nd.shape[-1] // 2
    ndd = nd.to(dev)
    out = torch.empty(ndd.shape, dtype=torch.int64, device=dev)
    for lo, bounds in ((0, vb), (half, hb)):
        part = ndd[:, lo:lo + half].contiguous()
        res = torch.empty(part.shape, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            _rgm.check(_rgm.lib.rgm_bucketize(_rgm.ptr(part), _rgm.ptr(bounds), bounds.numel(), _rgm.ptr(res), part.numel(),
                                              _rgm.current_stream()))
        out[:, lo:lo + half] = res
    return out.to(piano_roll.device)


# ---- chord rule (a11): device-side preamble + an analyser.  The reference's analyser is symbolic-music code on music21
# (piano_roll_to_chord.py:307-359), which is not vendored and cannot be restated: it stays a plug-in with the reference's own
# per-excerpt signature, so `register_chord_backend(piano_roll_to_chords)` with the reference's function is all a user with
# music21 needs.  What IS arithmetic on the roll -- mask, background snap, 0..127 quantisation -- runs on the GPU.  Opt-in beside it:
# `register_chord_backend("native")`, an analyser with its own definition that scores the integer roll on the device (csrc/chords.hip).
KEY_DICT = {"D major": 0, "g minor": 1, "B- major": 2, "G major": 3, "d minor": 4, "c# minor": 5, "F major": 6, "E- major": 7,
            "e minor": 8, "f# minor": 9, "C major": 10, "F# major": 11, "g# minor": 12, "A major": 13, "a minor": 14,
            "B major": 15, "A- major": 16, "b- minor": 17, "E major": 18, "c minor": 19, "b minor": 20, "e- minor": 21,
            "f minor": 22, "C# major": 23, "no key": 24}      # the chord classifier's key classes (piano_roll_to_chord.py:15-18)
IND2KEY = {v: k for k, v in KEY_DICT.items()}

# ---- the native analyser's tables (docs/rounds/chords.md: its own definition, agreement with music21 unmeasured).  Key number
# k = 12 * mode + tonic, mode 0 = major, tonic 0 = C; the device kernel (csrc/chords.hip) and the host analyser
# (piano_roll_to_chord.piano_roll_to_chords_native) both read these.
CHORD_KEY_NAMES = [t + " major" for t in ("C", "C#", "D", "E-", "E", "F", "F#", "G", "A-", "A", "B-", "B")] + \
                  [t + " minor" for t in ("c", "c#", "d", "e-", "e", "f", "f#", "g", "g#", "a", "b-", "b")]
CHORD_PROFILES = {
    "krumhansl": ((6.35, 2.23, 3.48, 2.33, 4.38, 4.09, 2.52, 5.19, 2.39, 3.66, 2.29, 2.88),                 # Krumhansl & Kessler 1982
                  (6.33, 2.68, 3.52, 5.38, 2.60, 3.53, 2.54, 4.75, 3.98, 2.69, 3.34, 3.17)),
    "aarden": ((17.7661, 0.145624, 14.9265, 0.160186, 19.8049, 11.3587, 0.291248, 22.062, 0.145624, 8.15494, 0.232998, 4.95122),
               (18.2648, 0.737619, 14.0499, 16.8599, 0.702494, 14.4362, 0.702494, 18.6161, 4.56621, 1.93186, 7.37619, 1.75623)),
}
CHORD_DEGREES = (1, 2, 2, 3, 3, 4, 4, 5, 6, 6, 7, 7)      # scale degree of (root - tonic) % 12: an altered degree carries its numeral's number
CHORD_MAX_WINDOW = 1024                                    # columns per window the kernel holds in LDS


def chord_profile(name):
    if name not in CHORD_PROFILES:
        raise ValueError(f"chord profile {name!r}: one of {sorted(CHORD_PROFILES)}")
    return CHORD_PROFILES[name]


def chord_window_columns(fs, window_size):
    """columns per chord window, window_size * fs: an integer (within 1e-9) in 1 .. 1024, else ValueError"""
    wc = float(window_size) * float(fs)
    n = int(round(wc))
    if abs(wc - n) > 1e-9 or not 1 <= n <= CHORD_MAX_WINDOW:
        raise ValueError(f"chord window of window_size * fs = {window_size} * {fs} = {wc} columns: must be an integer in 1 .. {CHORD_MAX_WINDOW}")
    return n


def parse_key(key):
    """'C major', 'b- minor', 'c#', 'Bb' ... -> tonic pitch class 0..11: a letter, an optional '#' or '-' / 'b', an optional mode word
    (the degree table is the same for both modes, so only the tonic matters).  Anything else: ValueError."""
    import re
    m = re.fullmatch(r"\s*([A-Ga-g])([#\-b]?)(?:\s+([A-Za-z]+))?\s*", key) if isinstance(key, str) else None
    if m is None or (m.group(3) is not None and m.group(3).lower() not in ("major", "minor")):
        raise ValueError(f"key {key!r}: expected a letter, an optional '#' or '-' / 'b' and an optional 'major' / 'minor'")
    pc = {"c": 0, "d": 2, "e": 4, "f": 5, "g": 7, "a": 9, "b": 11}[m.group(1).lower()]
    return (pc + {"": 0, "#": 1, "-": -1, "b": -1}[m.group(2)]) % 12


def key_class(k):
    """key number of the native analyser (-1: none) -> the chord classifier's key class (KEY_DICT)"""
    return KEY_DICT["no key"] if k < 0 else KEY_DICT[CHORD_KEY_NAMES[k]]


_CHORD_BACKEND = None
_CHORD_WORKERS = 4          # the reference chunks the batch over a 4-process pool (gaussian_diffusion.py:1365-1371)
_CHORD_POOL = None
_CHORD_PROFILE = "krumhansl"   # key profiles of the "native" backend
_PROFILE_DEV = {}           # (device, profile) -> (2,12) float64 tensor


def register_chord_backend(fn, workers=4, profile="krumhansl"):
    """fn(piano_roll (128,T) int array in [0,127], given_key=None, return_key=False, fs=100., window_size=1.28) ->
    {"chords": LongTensor (T/fs/window_size,), ["key": int, "correlationCoefficient": float]} -- the signature of the reference's
    piano_roll_to_chords (music21).  workers > 1 evaluates the excerpts of a batch in a persistent spawn-context process pool
    (fn must be picklable, i.e. a module-level function); 0/1 = in this process.

    fn = "native": the analyser on the device (chords_native below; `profile` = "krumhansl" | "aarden" picks its key profiles; no
    workers, no host round trip).  It follows its own definition (docs/rounds/chords.md), as does its host partner
    piano_roll_to_chord.piano_roll_to_chords_native, which registers like any other function; agreement of either with music21 has
    not been measured."""
    global _CHORD_BACKEND, _CHORD_WORKERS, _CHORD_POOL, _CHORD_PROFILE
    if isinstance(fn, str) and fn != "native":
        raise ValueError(f"chord backend {fn!r}: a function, or 'native' for the device analyser")
    chord_profile(profile)
    _CHORD_PROFILE = profile
    if _CHORD_POOL is not None:
        _CHORD_POOL.terminate()
        _CHORD_POOL = None
    _CHORD_BACKEND, _CHORD_WORKERS = fn, int(workers)


def chord_quantise(piano_roll_batch):
    """(N,C,128,T) roll -> (N,128,T) uint8 integer roll of channel 0 (get_chords' preamble, music_rules.py:100-110); writes the
    piano_like mask and the < -0.95 -> -1 snap into the caller's roll like the reference."""
    d, back = _stage(piano_roll_batch)
    N, Cc, _, T = d.shape
    q = torch.empty((N, 128, T), dtype=torch.uint8, device=d.device)
    with torch.cuda.device(d.device):
        _rgm.check(_rgm.lib.rgm_rule_chord_quantise(_rgm.ptr(d), _rgm.ptr(q), N, Cc, T, _rgm.current_stream()))
    back(d)
    return q


def native_chord_backend():
    return isinstance(_CHORD_BACKEND, str)


def chords_native(q, wc, profile="krumhansl", given_tonic=None, analyse_key=True):
    """rgm_rule_chords on the current stream: integer roll q (N,128,T) uint8 on the device, wc columns per window -> device tensors
    chords (N,W) int64, roots (N,W) int32 (-1: silent window), key (N) int32 (12 * mode + tonic, -1: none), coefficient (N) float64.
    given_tonic: None or 0..11 (one tonic for the batch); analyse_key=False needs it."""
    _rgm.require_cuda(q)
    if q.dim() != 3 or q.shape[1] != 128 or q.dtype != torch.uint8:
        raise ValueError(f"integer roll must be (N, 128, T) uint8, got {tuple(q.shape)} {q.dtype}")
    wc = int(wc)
    if not 1 <= wc <= CHORD_MAX_WINDOW:
        raise ValueError(f"chord window of {wc} columns: must be in 1 .. {CHORD_MAX_WINDOW}")
    if given_tonic is None and not analyse_key:
        raise ValueError("without key analysis a given tonic is needed")
    prof = chord_profile(profile)
    N, _, T = q.shape
    W, dev = T // wc, q.device
    if (dev, profile) not in _PROFILE_DEV:
        _PROFILE_DEV[(dev, profile)] = torch.tensor(prof, dtype=torch.float64, device=dev)
    given = None if given_tonic is None else torch.full((N,), int(given_tonic) % 12, dtype=torch.int32, device=dev)
    chords = torch.empty((N, W), dtype=torch.int64, device=dev)
    roots = torch.empty((N, W), dtype=torch.int32, device=dev)
    key = torch.empty((N,), dtype=torch.int32, device=dev)
    coef = torch.empty((N,), dtype=torch.float64, device=dev)
    ws = torch.empty((N * (W + 1) * 12,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _rgm.check(_rgm.lib.rgm_rule_chords(_rgm.ptr(q.contiguous()), N, T, wc, _rgm.ptr(_PROFILE_DEV[(dev, profile)]), _rgm.ptr(given),
                                            int(bool(analyse_key)), _rgm.ptr(chords), _rgm.ptr(roots), _rgm.ptr(key), _rgm.ptr(coef),
                                            _rgm.ptr(ws), ws.numel() * 4, _rgm.current_stream()))
    return chords, roots, key, coef


def _get_chords_native(piano_roll_batch, given_key, fs, window_size, return_key):
    """get_chords under the "native" backend: the preamble's writes into the caller's roll, then the analyser on the same stream.  The
    chords stay on the roll's device; only return_key reads back (the keys and coefficients are Python lists, like the host path's)."""
    wc = chord_window_columns(fs, window_size)                      # ValueError before any launch
    tonic = None if given_key is None else parse_key(given_key)
    q = chord_quantise(piano_roll_batch)
    chords, _, key, coef = chords_native(q, wc, _CHORD_PROFILE, tonic, analyse_key=return_key or tonic is None)
    chords = chords.to(piano_roll_batch.device)
    if chords.shape[0] == 1:
        chords = chords.squeeze(0)
    if return_key:
        return chords, [key_class(k) for k in key.tolist()], coef.tolist()
    return chords


def _chord_job(args):
    fn, roll, kw = args
    return fn(roll, **kw)


def _chord_pool():
    """the persistent spawn-context worker pool (None: evaluate in the calling thread)"""
    global _CHORD_POOL
    if _CHORD_WORKERS <= 1:
        return None
    if _CHORD_POOL is None:
        import multiprocessing
        _CHORD_POOL = multiprocessing.get_context("spawn").Pool(_CHORD_WORKERS)
    return _CHORD_POOL


def _run_chord_jobs(jobs):
    outs = None
    if _CHORD_WORKERS > 1 and len(jobs) > 1:
        try:
            outs = _chord_pool().map(_chord_job, jobs)
        except (AttributeError, TypeError, ImportError) as e:      # an unpicklable backend (lambda / closure): run it here
            if "pickle" not in str(e).lower() and "local object" not in str(e).lower():
                raise
            outs = None
    if outs is None:
        outs = [_chord_job(j) for j in jobs]
    return outs


def _pack_chords(outs, return_key):
    chords = torch.stack([torch.as_tensor(o["chords"], dtype=torch.long) for o in outs], dim=0)
    if chords.shape[0] == 1:
        chords = chords.squeeze(0)
    if return_key:
        return chords, [o["key"] for o in outs], [o["correlationCoefficient"] for o in outs]
    return chords


# ---- the analyser OVERLAPPED with the GPU.  The reference blocks the step on pool.map (gaussian_diffusion.py:1363-1375);
# here get_chords_async enqueues the device preamble on the caller's stream, copies the uint8 rolls to pinned host memory on a side
# stream and hands the analysis to a driver thread (which waits for THAT copy only, then feeds the worker pool) -- the caller goes on
# enqueueing GPU work (the next chunk's decode, the other rules) and joins the answer where it needs it (ChordFuture.result()).
_CHORD_SIDE = {}            # device index -> side stream of the D2H copies
_CHORD_DRIVER = None        # one driver thread: futures complete in submission order


class ChordFuture:
    """result() -> what get_chords returns for the same roll (chords [, keys, correlation coefficients])."""

    def __init__(self, fut, return_key):
        self._fut, self._return_key = fut, return_key

    def done(self):
        return self._fut.done()

    def result(self):
        return _pack_chords(self._fut.result(), self._return_key)


class _ReadyChords(ChordFuture):
    """the "native" backend's answer: device tensors behind the kernels already enqueued on the caller's stream -- nothing to wait for"""

    def __init__(self, value):
        self._value = value

    def done(self):
        return True

    def result(self):
        return self._value


def get_chords_async(piano_roll_batch, given_key=None, fs=100, window_size=1.28, return_key=False):
    """get_chords without the wait: (N,C,128,T) DEVICE roll -> ChordFuture.  The roll is read (and, like get_chords, written: mask +
    background snap) by a kernel on the current stream; the caller may go on using it on that stream at once."""
    global _CHORD_DRIVER
    if _CHORD_BACKEND is None:
        raise ImportError("chord rules need a host analyser (the reference's is music21-based and not vendored): "
                          "music_rule_guidance.music_rules.register_chord_backend(piano_roll_to_chords)")
    _rgm.require_cuda(piano_roll_batch)
    if native_chord_backend():                                            # no pinned copy, no side stream, no driver thread
        return _ReadyChords(_get_chords_native(piano_roll_batch, given_key, fs, window_size, return_key))
    q = chord_quantise(piano_roll_batch)                                  # (N,128,T) uint8, current stream
    dev = q.device
    cur = torch.cuda.current_stream(dev)
    side = _CHORD_SIDE.get(dev.index)
    if side is None:
        side = _CHORD_SIDE[dev.index] = torch.cuda.Stream(device=dev)
    host = torch.empty(q.shape, dtype=torch.uint8, pin_memory=True)
    ready = torch.cuda.Event()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        host.copy_(q, non_blocking=True)
        ready.record(side)
    q.record_stream(side)                                                 # the allocator must not hand q out again before the copy ran
    kw = dict(given_key=given_key, fs=fs, window_size=window_size, return_key=return_key)
    fn = _CHORD_BACKEND

    def work():
        ready.synchronize()                                               # this copy only -- not the device
        rolls = host.numpy().astype(np.intc)
        return _run_chord_jobs([(fn, rolls[i], kw) for i in range(rolls.shape[0])])
    if _CHORD_DRIVER is None:
        from concurrent.futures import ThreadPoolExecutor
        _CHORD_DRIVER = ThreadPoolExecutor(max_workers=1, thread_name_prefix="rgm-chord")
    return ChordFuture(_CHORD_DRIVER.submit(work), return_key)


def get_chords(piano_roll_batch, given_key=None, fs=100, window_size=1.28, return_key=False):
    """FUNC_DICT['chord_progression']: (N,C,128,T) roll -> chords (N, windows) LongTensor [(windows,) when N == 1]
    (+ keys, correlation coefficients with return_key) -- reference music_rules.py:97-130.  Blocking, like the reference; the
    samplers' search step uses get_chords_async."""
    if _CHORD_BACKEND is None:
        raise ImportError("chord rules need a host analyser (the reference's is music21-based and not vendored): "
                          "music_rule_guidance.music_rules.register_chord_backend(piano_roll_to_chords)")
    if native_chord_backend():
        return _get_chords_native(piano_roll_batch, given_key, fs, window_size, return_key)
    rolls = chord_quantise(piano_roll_batch).cpu().numpy().astype(np.intc)
    kw = dict(given_key=given_key, fs=fs, window_size=window_size, return_key=return_key)
    return _pack_chords(_run_chord_jobs([(_CHORD_BACKEND, rolls[i], kw) for i in range(rolls.shape[0])]), return_key)


# ---- mgeval's note statistics (docs/rounds/notes.md): what the reference's music_evaluation/mgeval/core.py `metrics` returns for the
# object its piano_roll_to_pretty_midi builds from a roll, on the device (csrc/notes.hip).  The host partner in numpy is
# piano_roll_to_chord.piano_roll_note_stats; both are pinned to the reference by tests/golden/notes.npz.
NOTE_STATS_FS = 100
NOTE_STATS_MAX_T = 32768
NOTE_STATS_INT = ("n_notes", "total_used_pitch", "pitch_range", "mean_note_velocity")
NOTE_STATS_REAL = ("end_time", "avg_IOI", "mean_note_duration", "note_density_mgeval")


def roll_to_u8(piano_roll):
    """float device roll (N, C, 128, T) in [-1, 1] -> a new uint8 roll: (x + 1) 63.5 + 2^-10, clamped to 0 .. 127 and truncated, so that a
    uint8 roll sent through u8 / 63.5 - 1 comes back in all 128 levels.  decode_sample_for_midi's background threshold (<= -0.95 -> 0) is
    NOT applied: it would take levels 1 .. 3 away; on a continuous roll apply it first if the decode's roll is wanted
    (docs/rounds/notes.md).  The input is not written to."""
    _rgm.require_cuda(piano_roll)
    if piano_roll.dim() != 4 or piano_roll.shape[2] != 128:
        raise ValueError(f"piano roll must be (N, C, 128, T), got {tuple(piano_roll.shape)}")
    d = piano_roll.detach().to(torch.float32).contiguous()
    N, Cc, _, T = d.shape
    out = torch.empty(d.shape, dtype=torch.uint8, device=d.device)
    with torch.cuda.device(d.device):
        _rgm.check(_rgm.lib.rgm_roll_to_u8(_rgm.ptr(d), _rgm.ptr(out), N, Cc, T, _rgm.current_stream()))
    return out


def _note_stats_layout(roll):
    """-> (N, C, T, byte strides of sample / channel / pitch / column) of a channel-first (N, C, 128, T) or channel-last (N, 128, T, C)
    uint8 roll; a shape that reads both ways ((N, 3, 128, 3) cannot occur: 128 pitches) is taken channel-first."""
    if roll.dim() == 3 and roll.shape[1] == 128:
        roll = roll.unsqueeze(1)
    if roll.dim() != 4:
        raise ValueError(f"roll must be (N, C, 128, T) or (N, 128, T, C), got {tuple(roll.shape)}")
    s = roll.stride()
    if roll.shape[2] == 128 and roll.shape[1] in (1, 2, 3):
        return roll, roll.shape[0], roll.shape[1], roll.shape[3], (s[0], s[1], s[2], s[3])
    if roll.shape[1] == 128 and roll.shape[3] in (1, 2, 3):
        return roll, roll.shape[0], roll.shape[3], roll.shape[2], (s[0], s[3], s[1], s[2])
    raise ValueError(f"roll must be (N, C, 128, T) or (N, 128, T, C) with C in 1..3, got {tuple(roll.shape)}")


def note_stats_raw(roll, first_column_onsets=False):
    """uint8 device roll in either layout -> (out_int (N, 148) int64, out_real (N, 16) float64) of rgm_note_stats, read in place"""
    _rgm.require_cuda(roll)
    if roll.dtype != torch.uint8:
        raise ValueError(f"note_stats_raw reads uint8 rolls, got {roll.dtype}")
    roll, N, Cc, T, strides = _note_stats_layout(roll)
    if not 1 <= T <= NOTE_STATS_MAX_T:
        raise ValueError(f"note statistics take 1 .. {NOTE_STATS_MAX_T} columns, got {T}")
    if N == 0 or min(strides) <= 0:
        raise ValueError("note statistics need a non-empty roll with positive strides")
    dev = roll.device
    out_int = torch.empty((N, 148), dtype=torch.int64, device=dev)
    out_real = torch.empty((N, 16), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        nbytes = _rgm.lib.rgm_note_stats_workspace(N, T)
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
        _rgm.check(_rgm.lib.rgm_note_stats(ctypes.c_void_p(roll.data_ptr()), *[int(x) for x in strides], N, Cc, T, int(bool(first_column_onsets)),
                                           _rgm.ptr(out_int), _rgm.ptr(out_real), _rgm.ptr(ws), ws.numel() * 8, _rgm.current_stream()))
    return out_int, out_real


def note_stats(roll, fs=100, first_column_onsets=False):
    """mgeval's eight note statistics of a batch of rolls, on the device.  roll: a uint8 device tensor, channel-first (N, C, 128, T) or the
    (N, 128, T, C) tensor of decode_sample_for_midi (read in place), or a float roll (N, C, 128, T) in [-1, 1], which goes through
    roll_to_u8; C = 1 [velocity], 2 [velocity | pedal] or 3 [velocity | onset | pedal].  -> dict of device tensors with the reference's raw
    values, NaN included: n_notes, total_used_pitch, pitch_range, mean_note_velocity (N,) int64; end_time, avg_IOI, mean_note_duration,
    note_density_mgeval (N,) float64; total_pitch_class_histogram (N, 12) float64; pitch_class_transition_matrix (N, 12, 12) int64.
    The roll is not written to.  fs must be 100: mgeval hard-codes get_piano_roll(fs=100)."""
    if fs != NOTE_STATS_FS:
        raise ValueError(f"note statistics are defined at fs = 100 (mgeval hard-codes get_piano_roll(fs=100)), got fs = {fs}")
    if roll.is_floating_point():
        roll = roll_to_u8(roll)
    oi, orl = note_stats_raw(roll, first_column_onsets)
    out = {k: oi[:, i] for i, k in enumerate(NOTE_STATS_INT)}
    out.update({k: orl[:, i] for i, k in enumerate(NOTE_STATS_REAL)})
    out["total_pitch_class_histogram"] = orl[:, 4:16]
    out["pitch_class_transition_matrix"] = oi[:, 4:148].reshape(-1, 12, 12)
    return out


# ---- note events and Standard MIDI Files of a roll on the device (docs/rounds/midi.md, csrc/midi.hip): the notes and pedal events of
# piano_roll_to_chord.piano_roll_to_pretty_midi and the file SimpleMIDI.write makes of them, byte for byte.
def midi_events_raw(roll, fs=100, first_column_onsets=False, program=0):
    """uint8 device roll in either layout -> dict: counts (N, 4) int64 on the device [notes, CCs, messages, file bytes], sizes_host (the same
    as numpy: the one host read between the two entries), note_offsets / cc_offsets / byte_offsets (N,) int64, notes (sum, 4) int32, ccs
    (sum, 2) int32 and bytes (sum,) uint8 -- the files back to back."""
    from guided_diffusion.midi_util import midi_tick_table
    _rgm.require_cuda(roll)
    if roll.dtype != torch.uint8:
        raise ValueError(f"the MIDI kernels read uint8 rolls, got {roll.dtype}")
    roll, N, Cc, T, strides = _note_stats_layout(roll)
    if not 1 <= T <= NOTE_STATS_MAX_T:
        raise ValueError(f"the MIDI kernels take 1 .. {NOTE_STATS_MAX_T} columns, got {T}")
    if N == 0 or min(strides) <= 0:
        raise ValueError("the MIDI kernels need a non-empty roll with positive strides")
    ticks = midi_tick_table(T, fs)                      # ValueError for an fs the device path does not serve
    dev = roll.device
    counts = torch.empty((N, 4), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        nbytes = _rgm.lib.rgm_midi_workspace(N, T)
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
        stream = _rgm.current_stream()
        _rgm.check(_rgm.lib.rgm_midi_measure(ctypes.c_void_p(roll.data_ptr()), *[int(x) for x in strides], N, Cc, T, int(bool(first_column_onsets)),
                                             ctypes.c_void_p(ticks.ctypes.data), _rgm.ptr(counts), _rgm.ptr(ws), ws.numel() * 8, stream))
        offsets = (torch.cumsum(counts, 0) - counts).t().contiguous()          # exclusive, on the device: (4, N)
        sizes = counts.cpu().numpy()                                            # the one host read: N sizes
        total = sizes.sum(0)
        notes = torch.empty((int(total[0]), 4), dtype=torch.int32, device=dev)
        ccs = torch.empty((int(total[1]), 2), dtype=torch.int32, device=dev)
        blob = torch.empty(int(total[3]), dtype=torch.uint8, device=dev)
        _rgm.check(_rgm.lib.rgm_midi_emit(N, T, int(program), _rgm.ptr(offsets[0]), _rgm.ptr(offsets[1]), _rgm.ptr(offsets[3]),
                                          _rgm.ptr(notes) if notes.numel() else None, notes.shape[0], _rgm.ptr(ccs) if ccs.numel() else None,
                                          ccs.shape[0], _rgm.ptr(blob), blob.numel(), _rgm.ptr(ws), ws.numel() * 8, stream))
    return {"counts": counts, "sizes_host": sizes, "note_offsets": offsets[0], "cc_offsets": offsets[1], "byte_offsets": offsets[3],
            "notes": notes, "ccs": ccs, "bytes": blob}


def note_events(roll, fs=100, first_column_onsets=False):
    """The notes and sustain-pedal events piano_roll_to_pretty_midi finds in a batch of uint8 device rolls (channel-first (N, C, 128, T) or
    the (N, 128, T, C) tensor of decode_sample_for_midi, read in place and not written to), as device tensors: n_notes, n_ccs (N,) int64;
    notes (sum, 4) int32 rows (pitch, velocity, start column, end column) per sample in (pitch, start column) order; ccs (sum, 2) int32 rows
    (column, value of controller 64) in column order; note_offsets, cc_offsets (N,) int64: where each sample's rows begin.  Times are
    column / fs; fs only has to be one the device path serves (midi_util.midi_tick_table)."""
    ev = midi_events_raw(roll, fs=fs, first_column_onsets=first_column_onsets)
    return {"n_notes": ev["counts"][:, 0], "n_ccs": ev["counts"][:, 1], "notes": ev["notes"], "ccs": ev["ccs"],
            "note_offsets": ev["note_offsets"], "cc_offsets": ev["cc_offsets"]}


NOTE_STAT_RULES = {"mg_used_pitch": "total_used_pitch", "mg_pitch_range": "pitch_range", "mg_avg_ioi": "avg_IOI",
                   "mg_mean_velocity": "mean_note_velocity", "mg_mean_duration": "mean_note_duration",
                   "mg_notes_per_second": "note_density_mgeval", "mg_pitch_class_hist": "total_pitch_class_histogram",
                   "mg_transition": "pitch_class_transition_matrix"}


def note_stat_rule(piano_roll, stat="total_used_pitch"):
    """FUNC_DICT entry of one statistic: float roll (N, C, 128, T) -> (N, K) float32 on the roll's device, K = 1, 12
    (total_pitch_class_histogram) or 144 (the transition matrix divided by its sum, mgeval's normalize = 2), NaN and inf replaced by 0 as
    music_evaluator.delete_nan does; batch size 1 squeezes the batch dimension like the other rules.  Nothing is written into the roll."""
    if not piano_roll.is_cuda:
        if not torch.cuda.is_available():
            raise _rgm.RgmError("rule kernels need a HIP device (no CPU fallback in the product path)")
        src = piano_roll.detach().to(torch.device("cuda", torch.cuda.current_device()))
    else:
        src = piano_roll
    v = note_stats(src)[stat]
    N = v.shape[0]
    v = v.reshape(N, -1).to(torch.float64)
    if stat == "pitch_class_transition_matrix":
        v = v / v.sum(dim=1, keepdim=True)
    out = torch.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0).to(torch.float32).to(piano_roll.device)
    return out.squeeze(0) if N == 1 else out
