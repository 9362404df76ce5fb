"""Rolls and host answers shared by the MIDI tests (tests/test_gpu_midi.py): the oracle is always the product's host path --
piano_roll_to_pretty_midi(...).write() on a COPY of the roll (the host function writes into its argument)."""
import os
import tempfile

import numpy as np


def host_file(roll, first_column_onsets=True, fs=100, program=0):
    """one roll (C, 128, T) or (128, T) uint8 -> (file bytes, notes (n, 4) int64 [pitch, velocity, start column, end column] sorted by
    (pitch, start column), ccs (m, 2) int64 [column, value], number of messages) of the host writer; the forced onsets of column 0 are
    applied as save_piano_roll_midi applies them"""
    from music_rule_guidance.piano_roll_to_chord import piano_roll_to_pretty_midi
    cur = np.array(roll)
    if cur.ndim == 3 and cur.shape[0] == 1:             # the host function takes a velocity-only roll as (128, T)
        cur = cur[0]
    if first_column_onsets and cur.ndim == 3 and cur.shape[0] == 3:
        cur[1, np.nonzero(cur[0, :, 0])[0], 0] = 127
    pm = piano_roll_to_pretty_midi(cur.astype(np.float32), fs=fs, program=program)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "a.midi")
        pm.write(path)
        with open(path, "rb") as f:
            data = f.read()
    ins = pm.instruments[0]
    notes = sorted((n.pitch, n.velocity, int(round(n.start * fs)), int(round(n.end * fs))) for n in ins.notes)
    notes.sort(key=lambda r: (r[0], r[2]))
    ccs = [(int(round(c.time * fs)), c.value) for c in ins.control_changes]
    return data, np.array(notes, dtype=np.int64).reshape(-1, 4), np.array(ccs, dtype=np.int64).reshape(-1, 2), len(pm.messages())


def random_roll(seed, C, T, density):
    """(C, 128, T) uint8: runs of mean length ~30 columns (they cross the 64-column words) started with probability ~density / 10 per cell,
    a low background in rows 0 .. 20, onsets of 0 / 63 / 64 / 127 and pedal columns on both sides of every threshold; density 0 is the empty
    roll, density >= 1 sets every cell and every onset"""
    rng = np.random.default_rng(seed)
    roll = np.zeros((C, 128, T), dtype=np.uint8)
    if density <= 0:
        return roll
    if density >= 1:
        roll[0] = rng.integers(1, 128, (128, T))
        roll[0, :21] = 0
        if C == 3:
            roll[1] = 127
        if C >= 2:
            roll[C - 1] = rng.integers(0, 128, (128, T))
        return roll
    state = rng.random(128) < density
    on = np.zeros((128, T), dtype=bool)
    for t in range(T):
        state = np.where(state, rng.random(128) < 0.97, rng.random(128) < density * 0.1)
        on[:, t] = state
    vel = on * rng.integers(1, 128, (128, T))
    vel[:21] = (vel[:21] > 0) * rng.integers(0, 9, (21, T))
    roll[0] = vel
    if C == 3:
        roll[1] = rng.choice(np.array([0, 63, 64, 127], dtype=np.uint8), (128, T), p=[0.8, 0.05, 0.05, 0.1])
    if C >= 2:
        level = rng.choice(np.array([0, 3, 5, 15, 17, 60, 70, 110, 127]), T)                   # per column, then noise around it
        roll[C - 1] = np.clip(level[None, :] + rng.integers(-3, 4, (128, T)), 0, 127) * (rng.random((128, T)) < 0.95)
    return roll


def pedal_column(total):
    """88 pedal cells (rows 21 .. 108) whose kept cells (>= 4) sum to `total`, only some rows set, plus cells of 3 that do not count"""
    col = np.zeros(128, dtype=np.uint8)
    p = 21
    while total >= 127 + 4:
        col[p] = 127
        total -= 127
        p += 1
    if total > 127:
        col[p], total = 64, total - 64
        p += 1
    if total:
        assert 4 <= total <= 127
        col[p] = total
        p += 1
    assert p <= 109
    col[p + 1:min(p + 4, 109)] = 3
    return col


def quirk_roll():
    """(3, 128, 16): one case per quirk of piano_roll_to_pretty_midi -- see test_the_quirk_roll"""
    r = np.zeros((3, 128, 16), dtype=np.uint8)
    r[0, 5, 3] = 10                                     # the background level: 10
    r[0, 30, 2:5], r[1, 30, 2] = 10, 127                # a velocity equal to the background: no run
    r[0, 31, 2:5], r[1, 31, 2] = 11, 127                # one above it: a note
    r[0, 40, 2:6], r[1, 40, 6] = 50, 127                # an onset one column past the run only: a note (6, 6)
    r[0, 41, 2:6], r[1, 41, 2], r[1, 41, 6] = 51, 127, 127              # ... and one at its start: (2, 6) and (6, 6)
    r[0, 42, 2:6], r[1, 42, 2], r[0, 42, 7:9], r[1, 42, 7] = 52, 127, 53, 90   # a re-strike right behind the column after a run
    r[0, 45, 3:8] = 60                                  # a run without an onset: nothing
    r[0, 50, 10:16], r[1, 50, 10] = 70, 127             # a run reaching column T
    r[0, 51, 10:16], r[1, 51, 10], r[1, 51, 13] = 71, 127, 127          # ... with a re-strike
    r[0, 52, 12:16], r[1, 52, 15] = [72, 30, 30, 90], 127               # ... started in its last column: the run's FIRST velocity
    r[0, 55, 4:7], r[1, 55, 4] = 80, 63                 # an onset of 63: none
    r[0, 56, 4:7], r[1, 56, 4] = 81, 64                 # an onset of 64
    r[0, 60, 0], r[0, 60, 1:4] = 5, 0                   # column 0 below the background: the forced onset finds no run
    r[0, 61, 0], r[0, 61, 1:4] = 5, 90                  # ... and does not start the run beside it either
    r[0, 62, 0:3] = 91                                  # a run from column 0 without an onset: a note only with first_column_onsets
    for col, total in enumerate((351, 352, 1407, 1408, 5631, 5632, 9943, 9944, 9856, 88 * 127, 87, 88)):
        r[2, :, col] = pedal_column(total)              # floor means 3 | 4, 15 | 16, 63 | 64, 112 | 113 (-> 127), 112, 127, 0 | 1
    r[2, 21:109, 12] = 3                                # cells below 4 only: no event
    r[2, 21:109, 13] = 4                                # cells of 4: value 4 -> CC value 0
    return r
