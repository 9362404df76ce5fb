"""Standard MIDI Files and host answers shared by the MIDI-reading tests (tests/test_midiread_host.py, tests/test_gpu_midiread.py): a small
SMF byte assembler and the named cases.  The oracle is always the product's host reader on the same bytes -- SimpleMIDI._read followed by
midi_to_full_piano_roll -- never a kernel (docs/rounds/midi_read.md)."""
import os
import struct
import tempfile

import numpy as np


# ------------------------------------------------------------------------------------------------------------------------- the assembler
def vlq(n, pad=0):
    """variable-length quantity; pad: extra leading 0x80 bytes (a longer encoding of the same number)"""
    out = [n & 0x7F]
    n >>= 7
    while n:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    return bytes([0x80] * pad) + bytes(reversed(out))


def ev(delta, *data):
    return vlq(delta) + bytes(data)


def meta(delta, kind, payload=b"", pad=0):
    return vlq(delta) + bytes([0xFF, kind]) + vlq(len(payload), pad) + bytes(payload)


def tempo(delta, us):
    return meta(delta, 0x51, struct.pack(">I", us)[1:])


END = meta(0, 0x2F)


def track(*events, length=None):
    body = b"".join(events)
    return b"MTrk" + struct.pack(">I", len(body) if length is None else length) + body


def smf(*tracks, div=220, fmt=1, ntrk=None, header_extra=b""):
    return b"MThd" + struct.pack(">IHHH", 6 + len(header_extra), fmt, len(tracks) if ntrk is None else ntrk, div) + header_extra + b"".join(tracks)


def note(ch, pitch, vel, start, length):
    """[(tick, bytes)] of one note with a status byte on both messages"""
    return [(start, bytes([0x90 | ch, pitch, vel])), (start + length, bytes([0x90 | ch, pitch, 0]))]


def timed(pairs):
    """[(absolute tick, message bytes)] -> the track's events with deltas, in a stable tick order"""
    out, last = [], 0
    for tick, data in sorted(pairs, key=lambda p: p[0]):
        out.append(vlq(tick - last) + data)
        last = tick
    return out


# ------------------------------------------------------------------------------------------------------------------------- the host oracle
def host_read(data, fs=100):
    """file bytes -> dict of the host reader's answers (raises what the host raises): roll (3,128,T) float32, notes (n, 5) float64 rows
    [instrument, pitch, velocity, start s, end s] sorted, ccs (m, 4) float64 rows [instrument, number, value, time s] in (instrument, event)
    order, n_inst"""
    from music_rule_guidance.piano_roll_to_chord import SimpleMIDI, midi_to_full_piano_roll
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "a.mid")
        with open(path, "wb") as f:
            f.write(data)
        pm = SimpleMIDI(path)
    roll = midi_to_full_piano_roll(pm, fs=fs)
    notes = [(k, n.pitch, n.velocity, n.start, n.end) for k, ins in enumerate(pm.instruments) for n in ins.notes]
    ccs = [(k, c.number, c.value, c.time) for k, ins in enumerate(pm.instruments) for c in ins.control_changes]
    return {"roll": roll, "notes": sort_notes(np.array(notes, dtype=np.float64).reshape(-1, 5)), "ccs": np.array(ccs, dtype=np.float64).reshape(-1, 4),
            "n_inst": len(pm.instruments)}


def sort_notes(rows):
    """rows [instrument, pitch, velocity, start, end] sorted by (instrument, start, pitch, end, velocity)"""
    return rows[np.lexsort((rows[:, 2], rows[:, 4], rows[:, 1], rows[:, 3], rows[:, 0]))] if len(rows) else rows


def host_refuses(data, fs=100):
    try:
        host_read(data, fs)
    except Exception:                                   # ValueError, IndexError, struct.error, NotImplementedError: whatever the host raises
        return True
    return False


# ------------------------------------------------------------------------------------------------------------------------- the cases
TEMPO_TRACK = track(tempo(0, 500000), meta(0, 0x58, bytes([4, 2, 24, 8])), meta(1, 0x2F))


def simple_file(div=220, text=0, pad=0):
    """two tracks, a few notes and pedal events; text: a text meta of that length in front of the second track"""
    body = timed(note(0, 60, 80, 0, 200) + note(0, 64, 70, 110, 330) + note(0, 67, 90, 440, 100) +
                 [(50, bytes([0xB0, 64, 100])), (300, bytes([0xB0, 64, 0])), (500, bytes([0xB0, 64, 127]))])
    head = [meta(0, 0x01, bytes((i * 7 + 3) & 0x7F for i in range(text)), pad)] if text or pad else []
    return smf(TEMPO_TRACK, track(*head, ev(0, 0xC0, 5), *body, meta(1, 0x2F)), div=div)


def _running_status():
    return smf(TEMPO_TRACK, track(ev(0, 0x90, 60, 64), ev(10, 62, 70), ev(100, 60, 0), ev(5, 62, 0), ev(0, 0xB0, 64, 127), ev(30, 64, 0),
                                  ev(40, 0x90, 72, 33), ev(100, 72, 0), END))


def _status_zero_and_fx():
    # data bytes before any status byte (a status of 0), F1 / F3 / FE taken as two-argument statuses, a padded delta, a longer header
    return smf(track(ev(0, 0x3C, 0x40), ev(3, 0xF1, 0x10, 0x20), ev(0, 0x11, 0x22), vlq(5, pad=3) + bytes([0xFE, 1, 2]), ev(0, 0x90, 60, 64),
                     ev(0, 0xF3, 0x05, 0x06), ev(220, 0x80, 60, 0), ev(0, 0xA0, 60, 9), ev(0, 0xE0, 0, 64), ev(0, 0xD0, 7), ev(1, 0xC0, 9), ev(0, 11),
                     ev(110, 0x90, 61, 1), ev(110, 61, 0), END), header_extra=b"\x00\x07")


def _offs_8x():
    return smf(TEMPO_TRACK, track(ev(0, 0x90, 60, 64), ev(100, 0x80, 60, 0), ev(0, 0x90, 60, 65), ev(50, 0x80, 60, 127), ev(10, 0x91, 30, 5),
                                  ev(300, 0x81, 30, 64), END))


def _format0():
    return smf(track(tempo(0, 400000), ev(0, 0xC0, 3), *timed(note(0, 50, 60, 10, 400) + note(0, 55, 61, 200, 400)), tempo(0, 800000),
                     ev(100, 0xB0, 64, 90), END), fmt=0)


def _three_tracks():
    t1 = timed(note(0, 60, 80, 0, 300) + note(3, 62, 81, 100, 300) + note(9, 36, 99, 0, 50) + [(0, bytes([0xC3, 40])), (20, bytes([0xB3, 64, 70]))])
    t2 = timed(note(3, 70, 50, 500, 200) + note(1, 71, 51, 0, 900) + note(15, 72, 52, 30, 60) + [(700, bytes([0xB1, 64, 50])), (5, bytes([0xCF, 99]))])
    t3 = timed(note(2, 30, 10, 1000, 10))
    return smf(TEMPO_TRACK, track(*t1, END), track(*t2, END), track(*t3, END))


def _drum():
    return smf(TEMPO_TRACK, track(*timed(note(9, 40, 100, 0, 2000) + note(9, 42, 100, 100, 50) + note(0, 60, 64, 0, 300) +
                                         [(1500, bytes([0xB9, 64, 127]))]), END))


def _cc_only_instrument():
    return smf(TEMPO_TRACK, track(*timed(note(0, 60, 64, 0, 800) + [(100, bytes([0xB1, 64, 20])), (300, bytes([0xB1, 64, 100])), (301, bytes([0xB1, 7, 3]))]),
                                  END))


def _cc_extends():
    return smf(TEMPO_TRACK, track(*timed(note(0, 60, 64, 0, 200) + [(1200, bytes([0xB0, 7, 100]))]), END),
               track(*timed(note(0, 61, 64, 0, 100) + [(900, bytes([0xB0, 64, 64]))]), END))


def _overlap_fifo():
    p = [(0, bytes([0x90, 60, 100])), (50, bytes([0x90, 60, 90])), (100, bytes([0x90, 60, 110])), (400, bytes([0x90, 60, 0])),
         (500, bytes([0x80, 60, 0])), (600, bytes([0x90, 60, 0])), (0, bytes([0x90, 61, 127])), (10, bytes([0x90, 61, 127])), (20, bytes([0x90, 61, 127])),
         (300, bytes([0x80, 61, 0])), (300, bytes([0x80, 61, 0])), (300, bytes([0x80, 61, 0]))]
    return smf(TEMPO_TRACK, track(*timed(p), END))


def _unmatched():
    return smf(TEMPO_TRACK, track(ev(0, 0x80, 60, 0), ev(0, 0x90, 61, 0), ev(10, 0x90, 62, 50), ev(100, 0x90, 63, 60), ev(100, 0x80, 63, 0),
                                  ev(5, 0x80, 63, 0), ev(0, 0x90, 64, 70), END))


def _short_note():
    return smf(TEMPO_TRACK, track(*timed(note(0, 60, 64, 0, 1) + note(0, 61, 64, 440, 3) + note(0, 62, 64, 100, 500)), END))


def _sysex_and_long_metas():
    return smf(TEMPO_TRACK, track(vlq(0) + b"\xF0" + vlq(200) + bytes(range(100, 127)) * 7 + bytes(10) + b"\xF7", meta(0, 0x01, bytes(300)),
                                  ev(0, 0x90, 60, 64), vlq(10) + b"\xF7" + vlq(130) + bytes(130), meta(5, 0x7F, bytes(129), pad=1),
                                  meta(0, 0x51, b"\x01\x02"), meta(0, 0x51, b"\x01\x02\x03\x04"), ev(205, 0x80, 60, 0), END))


def _tempo_mid_note():
    return smf(track(tempo(0, 500000), tempo(150, 250000), tempo(150, 1000000), END), track(*timed(note(0, 60, 64, 100, 400) + note(0, 62, 64, 290, 20)), END))


def _tempo_same_tick():
    # two tracks set a tempo at tick 100: the map orders them by value, so 300000 is overwritten by 700000 whatever the track order
    return smf(track(tempo(100, 700000), END), track(tempo(100, 300000), tempo(0, 300000), END),
               track(*timed(note(0, 60, 64, 0, 100) + note(0, 61, 64, 100, 100) + note(0, 62, 64, 200, 300)), END), div=96)


def _tempo_thousand():
    return smf(track(*[tempo(1 if i else 0, 300000 + (i * 7919) % 400000) for i in range(1000)], END),
               track(*timed([m for i in range(12) for m in note(0, 40 + i, 30 + i, 90 * i, 170)]), END), div=96)


def _pedal_shift_middle():
    # 0 then 127 inside one column (5): the second lands two columns on; a later event in column 7 sees it
    return smf(TEMPO_TRACK, track(*timed(note(0, 60, 64, 0, 440) + [(22, bytes([0xB0, 64, 0])), (23, bytes([0xB0, 64, 127])), (31, bytes([0xB0, 64, 10])),
                                                                   (32, bytes([0xB0, 64, 120])), (40, bytes([0xB0, 64, 30]))]), END))


def _pedal_shift_end():
    # the same jump in the last two columns of a 100-column roll: clamped to column T - 1
    return smf(TEMPO_TRACK, track(*timed(note(0, 60, 64, 0, 440) + [(432, bytes([0xB0, 64, 0])), (433, bytes([0xB0, 64, 127])), (437, bytes([0xB0, 64, 0])),
                                                                   (438, bytes([0xB0, 64, 100]))]), END),
               track(*timed([(433, bytes([0xB5, 64, 127])), (438, bytes([0xB5, 64, 1]))]), END))


ACCEPTED = {                                            # name -> (file bytes, fs)
    "running_status": (_running_status(), 100), "status_zero_and_fx": (_status_zero_and_fx(), 100), "offs_8x": (_offs_8x(), 100),
    "format0": (_format0(), 100), "three_tracks": (_three_tracks(), 100), "drum": (_drum(), 100), "cc_only_instrument": (_cc_only_instrument(), 100),
    "cc_extends": (_cc_extends(), 100), "overlap_fifo": (_overlap_fifo(), 100), "unmatched": (_unmatched(), 100), "short_note": (_short_note(), 100),
    "sysex_and_long_metas": (_sysex_and_long_metas(), 100), "tempo_mid_note": (_tempo_mid_note(), 100), "tempo_same_tick": (_tempo_same_tick(), 100),
    "tempo_thousand": (_tempo_thousand(), 100), "pedal_shift_middle": (_pedal_shift_middle(), 100), "pedal_shift_end": (_pedal_shift_end(), 100),
    "div_1": (smf(track(*timed(note(0, 60, 64, 0, 3) + note(0, 62, 65, 1, 1)), END), div=1), 100),
    "div_96": (simple_file(96), 100), "div_220": (simple_file(220), 100), "div_480": (simple_file(480), 100),
    "fs_12.5": (simple_file(220), 12.5), "fs_220": (simple_file(220), 220),
}

NOT_SMF, DIVISION, BAD_TRACK, TRUNCATED, DATA_BYTE, TEMPO_CAP, NO_NOTES = 1, 2, 3, 4, 5, 6, 7
_GOOD = simple_file()
REFUSED = {                                             # name -> (file bytes, the device's status); the host raises on every one
    "bad_magic": (b"RIFF" + _GOOD[4:], NOT_SMF), "short_header": (_GOOD[:13], NOT_SMF), "empty": (b"", NOT_SMF),
    "smpte": (_GOOD[:12] + b"\xE7\x28" + _GOOD[14:], DIVISION),
    "bad_track_magic": (_GOOD.replace(b"MTrk", b"MTrX"), BAD_TRACK), "track_past_end": (smf(TEMPO_TRACK, track(ev(0, 0x90, 60, 64), ev(9, 60, 0), END, length=99)), BAD_TRACK),
    "missing_track": (smf(TEMPO_TRACK, ntrk=2), BAD_TRACK),
    "ends_in_message": (smf(TEMPO_TRACK, track(ev(0, 0x90, 60, 64), ev(220, 0x90, 60))), TRUNCATED),
    "ends_in_delta": (smf(TEMPO_TRACK, track(ev(0, 0x90, 60, 64), b"\x81")), TRUNCATED),
    "ends_in_meta": (smf(TEMPO_TRACK, track(ev(0, 0x90, 60, 64), ev(9, 60, 0), b"\x00\xFF")), TRUNCATED),
    "pitch_144": (smf(TEMPO_TRACK, track(ev(0, 0x90, 0x90, 64), ev(220, 0x80, 0x90, 0), END)), DATA_BYTE),
    "tempo_cap_and_no_notes": (smf(track(*[tempo(1, 400000 + i) for i in range(2048)], END)), TEMPO_CAP),
    "no_notes": (smf(TEMPO_TRACK, track(ev(0, 0xB0, 64, 127), ev(500, 64, 0), END)), NO_NOTES),
    "note_too_short": (smf(TEMPO_TRACK, track(ev(0, 0x90, 60, 64), ev(1, 60, 0), END)), NO_NOTES),
}
