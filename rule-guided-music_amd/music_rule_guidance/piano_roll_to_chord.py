"""Piano roll -> note events -> Standard MIDI File, without pretty_midi / mido (neither is vendored).

Reference: music_rule_guidance/piano_roll_to_chord.py:167-275 (piano_roll_to_pretty_midi: which notes and sustain-pedal
events a generated (3,128,T) roll [velocity | onset | pedal] turns into) and guided_diffusion/midi_util.py:67-93
(save_piano_roll_midi).  The event extraction is restated here and pinned to the reference's output
(tests/golden/midi_events.npz).  The container classes mirror the pretty_midi attributes the reference touches
(`.instruments[0].notes`, `.control_changes`, `.write(path)`).  The writer's whole MESSAGE STREAM -- tick conversion, the order of
events at equal ticks, channels, track layout, delta ticks -- is pinned to what the reference's vendored pretty_midi fork hands to
mido (tests/golden/midi_writer.npz, tests/test_host_logic.py); only mido's byte serialisation of those messages is this module's own,
following the SMF 1.0 specification (format 1, 220 ticks per quarter note at 120 bpm -- pretty_midi's defaults).  Chord analysis
(music21) stays a host plug-in: music_rules.register_chord_backend (blocking get_chords, or get_chords_async beside the GPU in the
samplers' search step).  piano_roll_to_chords_native at the end is such a plug-in in numpy: the host partner of the device analyser
(csrc/chords.hip), following the same written definition (docs/rounds/chords.md), not music21's -- agreement with music21 has not been
measured.  Host-side I/O only -- nothing here is on the sampling hot path.
"""
import math
import struct

import numpy as np

from .music_rules import (CHORD_DEGREES, MAX_PIANO, MIN_PIANO, chord_profile, chord_window_columns, key_class, parse_key)

RESOLUTION = 220            # ticks per quarter note
TEMPO_US = 500000           # 120 bpm
TICKS_PER_SECOND = RESOLUTION * 1e6 / TEMPO_US


class Note:
    __slots__ = ("velocity", "pitch", "start", "end")

    def __init__(self, velocity, pitch, start, end):
        self.velocity, self.pitch, self.start, self.end = int(velocity), int(pitch), float(start), float(end)

    def __repr__(self):
        return f"Note(start={self.start:f}, end={self.end:f}, pitch={self.pitch}, velocity={self.velocity})"


class ControlChange:
    __slots__ = ("number", "value", "time")

    def __init__(self, number, value, time):
        self.number, self.value, self.time = int(number), int(value), float(time)


class Instrument:
    def __init__(self, program=0, is_drum=False, name=""):
        self.program, self.is_drum, self.name = int(program), bool(is_drum), name
        self.notes, self.control_changes = [], []


def _vlq(n):
    out = [n & 0x7F]
    n >>= 7
    while n:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    return bytes(reversed(out))


def _track(events):
    """events: (tick, order, bytes) -> MTrk chunk with delta times and the end-of-track meta event."""
    body, last = bytearray(), 0
    for tick, _, data in sorted(events, key=lambda e: (e[0], e[1])):
        body += _vlq(tick - last) + data
        last = tick
    body += _vlq(1 if events else 0) + b"\xff\x2f\x00"
    return b"MTrk" + struct.pack(">I", len(body)) + bytes(body)


class SimpleMIDI:
    """The slice of pretty_midi.PrettyMIDI the sampling scripts use: a list of instruments, write(), and a reader."""

    def __init__(self, midi_file=None):
        self.instruments = []
        self.resolution = RESOLUTION
        if midi_file is not None:
            self._read(midi_file)

    def get_end_time(self):
        ends = [n.end for i in self.instruments for n in i.notes] + [c.time for i in self.instruments for c in i.control_changes]
        return max(ends) if ends else 0.0

    # ------------------------------------------------------------------ writer
    # Message stream = what the reference's vendored pretty_midi fork hands to mido (pretty_midi/pretty_midi.py:1341-1520), pinned by
    # tests/golden/midi_writer.npz (a recording stand-in for mido around the fork's own write()): tick conversion, event order, channels,
    # track layout, delta ticks.  Only mido's byte serialisation (the SMF standard: _vlq and write() below) is this module's own.
    MSG_TIME_SIGNATURE, MSG_SET_TEMPO, MSG_PROGRAM, MSG_CONTROL, MSG_NOTE_ON, MSG_END = 0, 1, 2, 3, 4, 5

    def time_to_tick(self, t):
        """pretty_midi.time_to_tick (:1077-1109) of a freshly built PrettyMIDI: one tempo, so tick = round(t / seconds per tick) with
        Python's round (halves to even), the division written as the fork writes it."""
        if t <= 0.0:
            return 0
        return int(round(t / (60.0 / (120.0 * self.resolution))))

    def messages(self):
        """[(track, type, channel, data1, data2, delta_ticks)] in file order (types: MSG_*).  Track 0 = tempo + 4/4; one track per
        instrument: program change, then all events sorted by (tick, class, data) as the fork's comparator does (:1350-1394) -- at equal
        ticks control changes by (control, value), then note-ons by (pitch, velocity), a note-off being a note-on of velocity 0 -- and an
        end-of-track one tick behind the last event.  One deviation, outside what the samplers produce (their notes last >= 1 column =
        4.4 ticks): a note shorter than a tick ends one tick after it starts (the fork would emit its off BEFORE its on: a stuck note)."""
        tempo = int(6e7 / (60. / ((60.0 / (120.0 * self.resolution)) * self.resolution)))
        out = [(0, self.MSG_SET_TEMPO, 0, tempo, 0, 0), (0, self.MSG_TIME_SIGNATURE, 0, 4, 4, 0), (0, self.MSG_END, 0, 0, 0, 1)]
        for k, ins in enumerate(self.instruments):
            ch = 9 if ins.is_drum else (k % 15 if k % 15 < 9 else k % 15 + 1)
            ev = [(0, 6 << 16, self.MSG_PROGRAM, ins.program & 0x7F, 0)]
            for n in ins.notes:
                t0 = self.time_to_tick(n.start)
                t1 = max(self.time_to_tick(n.end), t0 + 1)
                vel = max(1, n.velocity) & 0x7F
                ev.append((t0, (10 << 16) + ((n.pitch & 0x7F) << 8) + vel, self.MSG_NOTE_ON, n.pitch & 0x7F, vel))
                ev.append((t1, (10 << 16) + ((n.pitch & 0x7F) << 8), self.MSG_NOTE_ON, n.pitch & 0x7F, 0))
            for c in ins.control_changes:
                ev.append((self.time_to_tick(c.time), (8 << 16) + ((c.number & 0x7F) << 8) + (c.value & 0x7F), self.MSG_CONTROL, c.number & 0x7F, c.value & 0x7F))
            ev.sort(key=lambda e: (e[0], e[1]))              # stable, like sorted(cmp_to_key(event_compare))
            last = 0
            for tick, _, kind, a, b in ev:
                out.append((k + 1, kind, ch, a, b, tick - last))
                last = tick
            out.append((k + 1, self.MSG_END, 0, 0, 0, 1))
        return out

    def write(self, filename):
        tracks = {}
        for trk, kind, ch, a, b, delta in self.messages():
            body = tracks.setdefault(trk, bytearray())
            body += _vlq(delta)
            if kind == self.MSG_SET_TEMPO:
                body += b"\xff\x51\x03" + struct.pack(">I", a)[1:]
            elif kind == self.MSG_TIME_SIGNATURE:
                body += bytes([0xFF, 0x58, 0x04, a, {1: 0, 2: 1, 4: 2, 8: 3, 16: 4}[b], 24, 8])
            elif kind == self.MSG_PROGRAM:
                body += bytes([0xC0 | ch, a])
            elif kind == self.MSG_CONTROL:
                body += bytes([0xB0 | ch, a, b])
            elif kind == self.MSG_NOTE_ON:
                body += bytes([0x90 | ch, a, b])
            else:
                body += b"\xff\x2f\x00"
        with open(filename, "wb") as f:
            f.write(b"MThd" + struct.pack(">IHHH", 6, 1, len(tracks), self.resolution))
            for trk in sorted(tracks):
                f.write(b"MTrk" + struct.pack(">I", len(tracks[trk])) + bytes(tracks[trk]))

    # ------------------------------------------------------------------ reader (format 0 / 1, tempo map, running status)
    def _read(self, filename):
        with open(filename, "rb") as f:
            data = f.read()
        if data[:4] != b"MThd":
            raise ValueError(f"{filename}: not a Standard MIDI File")
        hlen, _fmt, ntrk, div = struct.unpack(">IHHH", data[4:14])
        if div & 0x8000:
            raise NotImplementedError("SMPTE time division")
        self.resolution = div
        pos = 8 + hlen
        tracks, tempos = [], [(0, TEMPO_US)]
        for _ in range(ntrk):
            if data[pos:pos + 4] != b"MTrk":
                raise ValueError(f"{filename}: bad track chunk")
            tlen = struct.unpack(">I", data[pos + 4:pos + 8])[0]
            tr, p, end, tick, status = [], pos + 8, pos + 8 + tlen, 0, 0
            while p < end:
                d = 0
                while True:
                    b = data[p]
                    p += 1
                    d = (d << 7) | (b & 0x7F)
                    if not b & 0x80:
                        break
                tick += d
                b = data[p]
                if b == 0xFF:
                    kind = data[p + 1]
                    p += 2
                    ln = 0
                    while True:
                        c = data[p]
                        p += 1
                        ln = (ln << 7) | (c & 0x7F)
                        if not c & 0x80:
                            break
                    if kind == 0x51 and ln == 3:
                        tempos.append((tick, int.from_bytes(data[p:p + 3], "big")))
                    p += ln
                elif b in (0xF0, 0xF7):
                    p += 1
                    ln = 0
                    while True:
                        c = data[p]
                        p += 1
                        ln = (ln << 7) | (c & 0x7F)
                        if not c & 0x80:
                            break
                    p += ln
                else:
                    if b & 0x80:
                        status = b
                        p += 1
                    hi = status & 0xF0
                    nargs = 1 if hi in (0xC0, 0xD0) else 2
                    a = data[p:p + nargs]
                    p += nargs
                    tr.append((tick, status, a[0], a[1] if nargs == 2 else 0))
            tracks.append(tr)
            pos = end
        tempos.sort()
        t_ticks = np.array([t for t, _ in tempos], dtype=np.float64)
        t_us = np.array([u for _, u in tempos], dtype=np.float64)
        t_sec = np.concatenate(([0.0], np.cumsum(np.diff(t_ticks) * t_us[:-1] / (1e6 * div))))

        def seconds(tick):
            i = int(np.searchsorted(t_ticks, tick, side="right") - 1)
            return float(t_sec[i] + (tick - t_ticks[i]) * t_us[i] / (1e6 * div))

        for tr in tracks:
            by_ch = {}
            for tick, status, a, b in tr:
                ch, hi = status & 0x0F, status & 0xF0
                ins, on = by_ch.setdefault(ch, (Instrument(0, ch == 9), {}))
                if hi == 0xC0:
                    ins.program = a
                elif hi == 0xB0:
                    ins.control_changes.append(ControlChange(a, b, seconds(tick)))
                elif hi == 0x90 and b > 0:
                    on.setdefault(a, []).append((tick, b))
                elif hi == 0x80 or (hi == 0x90 and b == 0):
                    if on.get(a):
                        t0, vel = on[a].pop(0)
                        ins.notes.append(Note(vel, a, seconds(t0), seconds(tick)))
            for ch in sorted(by_ch):
                ins = by_ch[ch][0]
                if ins.notes or ins.control_changes:
                    ins.notes.sort(key=lambda n: (n.start, n.pitch))
                    self.instruments.append(ins)


def piano_roll_to_pretty_midi(full_roll, fs=100, program=0):
    """(128,T), (2,128,T) [velocity | pedal] or (3,128,T) [velocity | onset | pedal] roll in [0,127] -> SimpleMIDI with
    one instrument (reference :167-275).  Like the reference this WRITES into full_roll: onsets < 64 and pedal < 4
    are zeroed, velocities <= the loudest value below the piano range become 0.

    A note spans a maximal run of non-zero velocity in a pitch row and takes the run's first velocity; with an onset
    channel the run is cut at every onset inside it (+1 column) and dropped when it has none.  Pedal: the piano rows'
    mean per column (truncated), emitted as CC 64 where non-zero, < 16 -> 0 and > 112 -> 127."""
    full_roll = np.asarray(full_roll)
    onset_roll = None
    if full_roll.ndim == 3:
        piano_roll = full_roll[0]
        if full_roll.shape[0] == 2:
            pedal_roll = full_roll[1]
        else:
            onset_roll = full_roll[1]
            onset_roll[onset_roll < 64] = 0
            pedal_roll = full_roll[2]
        pedal_roll[pedal_roll < 4] = 0
        pedal = pedal_roll[MIN_PIANO:MAX_PIANO + 1].mean(axis=0).astype(np.intc)
        has_pedal = not math.isclose(pedal.max(), 0)
    else:
        piano_roll, pedal, has_pedal = full_roll, None, False
    piano_roll[piano_roll <= piano_roll[:MIN_PIANO, :].max()] = 0
    ins = Instrument(program=program)
    T = piano_roll.shape[1]
    active = np.zeros((128, T + 2), dtype=np.int8)
    active[:, 1:-1] = piano_roll != 0
    edges = np.diff(active, axis=1)                        # +1 at the first column of a run, -1 one past its last column
    off_t, off_p = np.nonzero(edges.T == -1)               # note-offs in (time, pitch) order: the order the reference appends in
    starts = {}
    on_t, on_p = np.nonzero(edges.T == 1)
    for t, p in zip(on_t, on_p):
        starts.setdefault(int(p), []).append(int(t))
    taken = {p: 0 for p in starts}
    for t, p in zip(off_t, off_p):
        t, p = int(t), int(p)
        s = starts[p][taken[p]]
        taken[p] += 1
        vel = int(piano_roll[p, s])
        if onset_roll is None:
            ins.notes.append(Note(vel, p, s / fs, t / fs))
            continue
        s_ind, e_ind = round((s / fs) * fs), round((t / fs) * fs)
        ons = np.nonzero(onset_roll[p, s_ind:e_ind + 1])[0]
        if len(ons) == 0:
            continue
        st = (ons + s_ind) / fs
        en = np.concatenate((st[1:], np.array([t / fs])))
        for a, b in zip(st, en):
            ins.notes.append(Note(vel, p, a, b))
    if has_pedal:
        for t in np.nonzero(pedal)[0]:
            v = int(pedal[t])
            v = 0 if v < 16 else (127 if v > 112 else v)
            ins.control_changes.append(ControlChange(64, v, t / fs))
    pm = SimpleMIDI()
    pm.instruments.append(ins)
    return pm


# ---- sine synthesis of a roll: the host partner of csrc/synth.hip (docs/rounds/synth.md).  A restatement of the reference's vendored
# pretty_midi fork -- PrettyMIDI.synthesize(fs, wave=np.sin) (pretty_midi/pretty_midi.py:954-983) over Instrument.synthesize
# (pretty_midi/instrument.py:355-441), one instrument, no pitch bends, not a drum -- pinned to it bit for bit (tests/golden/synth.npz).
def synth_tables(T, fs=100, audio_fs=44100):
    """The four host tables the device renderer takes, all in float64 arithmetic so that every integer truncation and the phase increment
    are synthesize_events' own bits: samp (T + 1,) int64 = int(audio_fs * (k / fs)), the first audio sample of column k; length (T + 1,)
    int64 = int(audio_fs * (k / fs + 1)), the length of a waveform whose last event lies in column k; omega (128,) float64 =
    2 pi f_p * 1.0 / audio_fs; fade = linspace(1, 0, int(.1 * audio_fs)).  ValueError unless fs and audio_fs are positive and every
    entry stays below 2^31."""
    T = int(T)
    if T < 1:
        raise ValueError(f"synthesis tables cover at least one column, got T = {T}")
    if not fs > 0 or not audio_fs > 0 or not math.isfinite(audio_fs) or not math.isfinite(fs):
        raise ValueError(f"fs and audio_fs must be positive, got {fs} and {audio_fs}")
    if audio_fs * (T / fs + 1) >= 2.0 ** 31:
        raise ValueError(f"a waveform of {T} columns at fs = {fs}, audio_fs = {audio_fs} would reach 2^31 samples")
    t = np.arange(T + 1) / float(fs)                    # k / fs, the time of a note or event in column k
    samp = (float(audio_fs) * t).astype(np.int64)       # int(): truncation of a non-negative float64
    length = (float(audio_fs) * (t + 1)).astype(np.int64)
    omega = np.array([2 * np.pi * (440.0 * (2.0 ** ((p - 69) / 12.0))) * 1.0 / audio_fs for p in range(128)], dtype=np.float64)
    fade = np.linspace(1, 0, int(.1 * audio_fs))
    return samp, length, omega, fade


def synthesize_events(pm, audio_fs=44100):
    """Instrument.synthesize(fs=audio_fs) of pm's one instrument: the un-normalised float64 sum of its notes' sines, L = int(audio_fs *
    (end_time + 1)) samples, end_time counting the control changes.  Each note is wave = sin((2 pi f * 1.0 / audio_fs) * k + 0.0) for
    k = 0 .. n - 1 under exp(-k / (1.0 * audio_fs)), the last int(.1 * audio_fs) samples (all of them for a note no longer than that)
    under a linear fade to 0, times the velocity; notes are added in list order."""
    ins = pm.instruments[0]
    out = np.zeros(int(audio_fs * (pm.get_end_time() + 1)))
    fade_out = np.linspace(1, 0, int(.1 * audio_fs))
    for note in ins.notes:
        start, end = int(audio_fs * note.start), int(audio_fs * note.end)
        frequency = 440.0 * (2.0 ** ((note.pitch - 69) / 12.0))
        k = np.arange(end - start)
        wave = np.sin((2 * np.pi * frequency * 1.0 / audio_fs) * k + 0.0)
        envelope = np.exp(-k / (1.0 * audio_fs))
        if envelope.shape[0] > fade_out.shape[0]:
            envelope[-fade_out.shape[0]:] *= fade_out
        else:
            envelope *= np.linspace(1, 0, envelope.shape[0])
        envelope *= note.velocity
        out[start:end] += envelope * wave
    return out


def synthesize_roll(full_roll, fs=100, audio_fs=44100, normalize=True, return_silent=False):
    """(128,T), (2,128,T) or (3,128,T) roll -> float64 (L,): what the reference's piano_roll_to_pretty_midi(roll, fs) followed by its
    fork's .synthesize(fs=audio_fs) returns (normalize=True: divided by its largest magnitude; False: Instrument.synthesize's raw sum).
    Like piano_roll_to_pretty_midi this writes into full_roll.  ONE departure from the reference: a waveform that is zero throughout (a
    roll without notes, or with notes too short to sound) is returned as zeros and reported silent, where the reference divides 0 by 0
    and returns L NaNs.  return_silent: -> (waveform, silent)."""
    out = synthesize_events(piano_roll_to_pretty_midi(full_roll, fs=fs), audio_fs)
    peak = np.abs(out).max() if out.shape[0] else 0.0
    silent = not peak > 0
    if normalize and not silent:
        out /= peak
    return (out, silent) if return_silent else out


def wav_bytes(x, audio_fs):
    """A waveform in [-1, 1] -> the bytes of a mono 16-bit PCM RIFF file: samples rint(x * 32767) (halves to even) as int16 behind the
    44-byte header the standard library's wave module writes."""
    import io
    import wave
    pcm = np.rint(np.asarray(x, dtype=np.float64) * 32767).astype("<i2")
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(audio_fs))
        w.writeframes(pcm.tobytes())
    return buf.getvalue()


def quantize_pedal(value, num_bins=8):
    """pedal CC value 0..127 -> centre of its bin (reference midi_util.py:252-264: 0..15 -> 8, ..., 112..127 -> 120)."""
    if value < 0 or value > 127:
        raise ValueError("Value should be between 0 and 127")
    width = 128 // num_bins
    return min(int(value) // width * width + width // 2, 127)


def midi_to_full_piano_roll(pm, fs=100):
    """SimpleMIDI (or anything with .instruments of notes / control_changes) -> (3,128,T) [velocity | onset | pedal] float32 roll:
    the reference's get_full_piano_roll (midi_util.py:267-291) over its vendored pretty_midi FORK's
    get_piano_roll(fs, pedal_threshold=None, onset=True) (/root/reference/pretty_midi/instrument.py:70-205, pretty_midi.py:797-852),
    restated and pinned to both (tests/golden/midi_rolls.npz):
      * per instrument: no notes -> nothing (the fork's onset=True path cannot unpack such an instrument and raises); int(fs * end_time) columns, end_time = last note end / control change of THAT instrument;
        drums -> zeros; velocity += over [int(start*fs), int(end*fs)) (overlaps add up, nothing is clipped; a note shorter than a
        column leaves no velocity); onset = 127 (a binary mark, not the velocity) at min(int(start*fs), columns - 1);
      * instruments are summed into max-columns rolls, the onset roll clipped to 127;
      * pedal: the reference's own loop (quantised CC 64 values on the piano rows, a 0 -> 127 jump in one column shifted by two)."""
    rolls = []
    for ins in pm.instruments:
        if not ins.notes:
            continue
        ends = [n.end for n in ins.notes] + [c.time for c in ins.control_changes] + [b.time for b in getattr(ins, "pitch_bends", [])]
        cols = int(fs * max(ends))
        vel, on = np.zeros((128, cols)), np.zeros((128, cols))
        if not ins.is_drum:
            for n in ins.notes:
                vel[n.pitch, int(n.start * fs):int(n.end * fs)] += n.velocity
                if cols > 0:
                    on[n.pitch, min(int(n.start * fs), cols - 1)] = 127
        rolls.append((vel, on))
    T = max([v.shape[1] for v, _ in rolls], default=0)
    if T == 0:   # no instrument has a note that reaches the first column: the reference's fork raises here; a (3,128,0) roll would fail far from its cause
        raise ValueError("midi_to_full_piano_roll: no notes (or none lasting one column of 1/fs s) -- the reference cannot build a roll from this file either")
    roll = np.zeros((3, 128, T), dtype=np.float64)
    for v, o in rolls:
        roll[0, :, :v.shape[1]] += v
        roll[1, :, :o.shape[1]] += o
    np.clip(roll[1], 0, 127, out=roll[1])
    for ins in pm.instruments:
        for cc in ins.control_changes:
            if cc.number != 64:
                continue
            t = int(cc.time * fs)
            if t < T:
                if roll[2, MIN_PIANO, t] != 0.0 and abs(roll[2, MIN_PIANO, t] - cc.value) > 64:
                    roll[2, MIN_PIANO:MAX_PIANO + 1, min(t + 2, T - 1)] = quantize_pedal(cc.value)
                else:
                    roll[2, MIN_PIANO:MAX_PIANO + 1, t] = quantize_pedal(cc.value)
    return roll.astype(np.float32)


# ---- the native chord and key analyser on the host (docs/rounds/chords.md).  Same definition and the same IEEE operations in the
# same order as csrc/chords.hip, so the two agree bit for bit; registered like any analyser (register_chord_backend(
# piano_roll_to_chords_native)) it runs through the worker pool and is the A/B partner of register_chord_backend("native").
ROMAN = ("", "I", "II", "III", "IV", "V", "VI", "VII")


def _native_key(D, prof):
    """pitch-class durations D (12 ints) -> (key number 12 * mode + tonic or -1, Pearson r of the key).  Plain Python floats, sums in
    class order: what the kernel computes with FMA contraction off."""
    sx = 0.0
    for c in range(12):
        sx += D[c]
    mx = sx / 12.0
    sxx = 0.0
    for c in range(12):
        sxx += (D[c] - mx) * (D[c] - mx)
    if sxx == 0.0:
        return -1, 0.0
    key, best = -1, 0.0
    for mode in (0, 1):
        P = prof[mode]
        for tonic in range(12):
            sy = 0.0
            for c in range(12):
                sy += P[(c - tonic) % 12]
            my = sy / 12.0
            sxy = syy = 0.0
            for c in range(12):
                dx, dy = D[c] - mx, P[(c - tonic) % 12] - my
                sxy += dx * dy
                syy += dy * dy
            r = sxy / math.sqrt(sxx * syy)
            if key < 0 or r > best:                       # the first maximum
                key, best = 12 * mode + tonic, r
    return key, best


def _native_root(pitches):
    """sounding pitches of a slice (ascending) -> root pitch class"""
    S = {int(p) % 12 for p in pitches}
    bass = int(pitches[0]) % 12
    root, best = bass, -1
    for k in range(12):
        r = (bass + k) % 12
        if r not in S:
            continue
        score = (8 * ((r + 7) % 12 in S) + 4 * ((r + 4) % 12 in S or (r + 3) % 12 in S) + 3 * ((r + 6) % 12 in S)
                 + 2 * ((r + 10) % 12 in S or (r + 11) % 12 in S))
        if score > best:
            root, best = r, score
    return root


def native_roots(act, wc):
    """act (88, T) bool, pitches 21..108 -> root pitch class per whole window of wc columns (-1: no sounding column): the longest run of
    columns with one non-empty pitch set inside the window, the earliest among equals."""
    W = act.shape[1] // wc
    roots = np.full(W, -1, dtype=np.int64)
    if W == 0:
        return roots
    cols = np.packbits(act[:, :W * wc], axis=0)                             # (11, W wc): one key per column
    start = np.ones(W * wc, dtype=bool)
    start[1:] = (cols[:, 1:] != cols[:, :-1]).any(axis=0)
    start[::wc] = True                                                      # runs are cut at window boundaries
    idx = np.nonzero(start)[0]
    length = np.diff(np.append(idx, W * wc))
    keep = cols[:, idx].any(axis=0)                                         # silent slices are not chords
    idx, length = idx[keep], length[keep]
    order = np.lexsort((idx, -length))                                      # longest first, earliest among equals
    win, first = np.unique(idx[order] // wc, return_index=True)
    for w, t in zip(win, idx[order][first]):
        roots[w] = _native_root(np.nonzero(act[:, t])[0] + MIN_PIANO)
    return roots


def piano_roll_to_chords_native(piano_roll_excerpt, given_key=None, return_key=False, tagging_func=None, fs=100., window_size=1.28,
                                profile="krumhansl"):
    """The reference's per-excerpt analyser interface (piano_roll_to_chord.py:307-359) over the native definition: (128, T) integer roll
    -> {"chords": int64 array (T // (window_size fs),), ["key": KEY_DICT class, "correlationCoefficient": float]}.  With given_key and not
    return_key the key is not analysed; otherwise it is, an excerpt without a key (silence, flat pitch-class profile) answers zeros,
    "no key" and 0.0, and the degrees use the given tonic when there is one.  tagging_func (default: the degree numbers themselves)
    is called with the degree's Roman numeral ("" for a silent window)."""
    wc = chord_window_columns(fs, window_size)
    prof = chord_profile(profile)
    tonic = None if given_key is None else parse_key(given_key)
    roll = np.asarray(piano_roll_excerpt)
    if roll.ndim != 2 or roll.shape[0] != 128:
        raise ValueError(f"piano roll excerpt must be (128, T), got {roll.shape}")
    act = roll[MIN_PIANO:MAX_PIANO + 1] > 0
    W = act.shape[1] // wc
    out = {}
    if tonic is None or return_key:
        per_pitch = act.sum(axis=1)
        key, coef = _native_key([int(per_pitch[(c - MIN_PIANO) % 12::12].sum()) for c in range(12)], prof)
        out = {"key": key_class(key), "correlationCoefficient": coef}
        if key < 0:
            return dict(out, chords=np.zeros(W, dtype=np.int64))
        if tonic is None:
            tonic = key % 12
    roots = native_roots(act, wc)
    chords = np.array([0 if r < 0 else CHORD_DEGREES[(r - tonic) % 12] for r in roots], dtype=np.int64)
    if tagging_func is not None:
        chords = np.array([tagging_func(ROMAN[d]) for d in chords], dtype=np.int64)
    return dict(out, chords=chords)


# ---- mgeval's note statistics on the host (docs/rounds/notes.md): what the reference's music_evaluation/mgeval/core.py `metrics`
# returns for the object its piano_roll_to_pretty_midi (:167-275) builds from a roll, written from the definition -- a note list, the
# rebuilt roll of the fork's get_piano_roll(fs=100), the pair matrix -- without a MIDI object.  Pinned to the reference by
# tests/golden/notes.npz; the A/B partner of the device analyser (csrc/notes.hip, music_rules.note_stats), which never builds a note list.
NOTE_STATS_FS = 100


def _col(k):
    """the column the fork's get_piano_roll gives the time k / 100: int((k / 100) * 100) in float64, k or k - 1"""
    return int((k / 100) * 100)


def piano_roll_note_stats(full_roll, fs=100, first_column_onsets=False):
    """(128, T) or (C, 128, T) integer roll, C = 1 [velocity], 2 [velocity | pedal] or 3 [velocity | onset | pedal] -> dict of the
    eight statistics plus n_notes and end_time (numpy scalars / arrays, NaN where mgeval answers NaN).  The input is not written to.
    first_column_onsets: the onset channel counts as 127 in column 0 of every row that sounds there (what save_piano_roll_midi does
    before it writes a file)."""
    if fs != NOTE_STATS_FS:
        raise ValueError(f"note statistics are defined at fs = 100 (mgeval hard-codes get_piano_roll(fs=100)), got fs = {fs}")
    roll = np.array(full_roll, dtype=np.int64)                  # a copy: the reference's function writes into its input, this one does not
    if roll.ndim == 2:
        roll = roll[None]
    if roll.ndim != 3 or roll.shape[0] not in (1, 2, 3) or roll.shape[1] != 128 or roll.shape[2] < 1:
        raise ValueError(f"roll must be (128, T) or (C, 128, T) with C in 1..3 and T >= 1, got {np.shape(full_roll)}")
    C, _, T = roll.shape
    vel = roll[0]
    onset = None
    if C == 3:
        onset = roll[1]
        if first_column_onsets:
            onset[vel[:, 0] != 0, 0] = 127
        onset = onset >= 64
    vel = np.where(vel > vel[:MIN_PIANO].max(), vel, 0)
    # notes (pitch, start column, end column, velocity)
    notes = []
    for p in np.nonzero(vel.any(axis=1))[0]:
        a = np.zeros(T + 2, dtype=np.int8)
        a[1:-1] = vel[p] != 0
        d = np.diff(a)
        for s, e in zip(np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]):
            v = int(vel[p, s])
            if onset is None:
                notes.append((int(p), int(s), int(e), v))
                continue
            ons = s + np.nonzero(onset[p, s:e + 1])[0]           # the slice stops at T - 1
            for o, nxt in zip(ons, list(ons[1:]) + [e]):
                notes.append((int(p), int(o), int(nxt), v))
    # pedal events (column, value)
    events = []
    if C >= 2:
        ped = roll[C - 1]
        ped = np.where(ped >= 4, ped, 0)[MIN_PIANO:MAX_PIANO + 1].sum(axis=0) // (MAX_PIANO - MIN_PIANO + 1)
        events = [(int(t), 0 if ped[t] < 16 else (127 if ped[t] > 112 else int(ped[t]))) for t in np.nonzero(ped)[0]]
    n = len(notes)
    last = max([e for _, _, e, _ in notes] + [t for t, _ in events], default=0)
    end_time = last / 100
    out = {"n_notes": np.int64(n), "end_time": np.float64(end_time)}
    # the rebuilt roll
    W = _col(last) if n else 0
    re = np.zeros((128, W), dtype=np.int64)
    for p, s, e, v in notes:
        re[p, _col(s):_col(e)] += v
    down, press = False, 0
    for t, v in events if n else []:
        if v >= 64 and not down:
            down, press = True, _col(t)
        elif v < 64 and down:
            down = False
            re[:, press:_col(t)] = np.maximum.accumulate(re[:, press:_col(t)], axis=1)
    rows = re.sum(axis=1)
    used = np.nonzero(rows > 0)[0]
    out["total_used_pitch"] = np.int64(len(used))
    out["pitch_range"] = np.int64(used[-1] - used[0]) if len(used) else np.int64(0)
    folded = np.array([rows[c::12].sum() for c in range(12)], dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        out["total_pitch_class_histogram"] = folded / folded.sum()
    out["mean_note_velocity"] = np.int64(sum(v for _, _, _, v in notes) // n) if n else np.int64(0)
    dur = 0.0
    for _, s, e, _ in notes:
        dur += e / 100 - s / 100
    out["mean_note_duration"] = np.float64(dur / n) if n else np.float64(0.0)
    out["note_density_mgeval"] = np.float64(n / end_time) if end_time > 0 else np.float64(0.0)
    starts = sorted(s for _, s, _, _ in notes)
    out["avg_IOI"] = np.float64((starts[-1] / 100 - starts[0] / 100) / (n - 1)) if n >= 2 else np.float64(np.nan)
    M = np.zeros((12, 12), dtype=np.int64)
    if n > 1:
        pc = np.array([p % 12 for p, _, _, _ in notes])
        st = np.array([s for _, s, _, _ in notes], dtype=np.float64) / 100
        en = np.array([e for _, _, e, _ in notes], dtype=np.float64) / 100
        for i0 in range(0, n, 1024):                                # ends in blocks: the pair matrix never holds more than 1024 n cells
            src, dst = np.nonzero(np.abs(np.subtract.outer(en[i0:i0 + 1024], st)) < 0.05)
            np.add.at(M, (pc[i0:i0 + 1024][src], pc[dst]), 1)
    out["pitch_class_transition_matrix"] = M
    return out
