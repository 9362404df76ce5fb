"""Inputs of the note-statistics tests (docs/rounds/notes.md), shared by tests/golden/make_golden_notes.py, which asks the reference,
and by tests/test_notes_host.py / tests/test_rule_notes_gpu.py, which compare the host partner and the kernel with its answers.

cases() -> {name: (C, 128, T) uint8 roll}, in a fixed order: random note-event rolls rebuilt from their seeds (20 seeds x C in
{1, 2, 3} x T in {64, 384, 1064}) and small hand-built rolls (T = HAND_T), one per quirk of the definition.  Only seeds and the
reference's answers are stored in tests/golden/notes.npz; the rolls are rebuilt here."""
import numpy as np

SEED = 7100
N_SEEDS = 20
RANDOM_T = (64, 384, 1064)          # 1064: no multiple of 64 or 256, past column 803 where col(k) = k - 1 again
HAND_T = 80
INT_FIELDS = ("n_notes", "total_used_pitch", "pitch_range", "mean_note_velocity")     # then the 144 transition counts
REAL_FIELDS = ("end_time", "avg_IOI", "mean_note_duration", "note_density_mgeval")    # then the 12 histogram values


def random_roll(seed, C, T):
    """note events in rows 21..108 (so that most survive the background rule): velocity plateaus, onsets of 127 at most note starts and a
    few re-strikes, weak onsets (< 64) and stray onsets in silence; pedal plateaus over the piano rows; a little low noise everywhere"""
    rng = np.random.RandomState(seed)
    roll = np.zeros((C, 128, T), dtype=np.uint8)
    for _ in range(6 + T // 12):
        p, s = int(rng.randint(21, 109)), int(rng.randint(0, T))
        d = int(rng.choice([1, 2, 5, 6, 12, 40])) + int(rng.randint(0, 4))
        v = int(rng.randint(20, 128))
        roll[0, p, s:s + d] = v
        if rng.rand() < 0.3:
            roll[0, p, s + d // 2:s + d] = max(1, v - 9)               # a velocity step inside the run: the note keeps the first one
        if C == 3:
            if rng.rand() < 0.85:
                roll[1, p, s] = 127
            if d > 3 and rng.rand() < 0.3:
                roll[1, p, min(T - 1, s + int(rng.randint(1, d)))] = int(rng.choice([64, 100, 127]))
            if rng.rand() < 0.15:
                roll[1, p, min(T - 1, s + d)] = 127                   # an onset just behind the run: a note of length zero
            if rng.rand() < 0.2:
                roll[1, p, int(rng.randint(0, T))] = int(rng.choice([30, 63, 127]))
    if rng.rand() < 0.5:
        roll[0, int(rng.randint(0, 21)), int(rng.randint(0, T))] = int(rng.randint(1, 30))   # raises the background
    if C >= 2:
        t = 0
        while t < T:
            w = int(rng.randint(3, 60))
            roll[C - 1, 21:109, t:t + w] = int(rng.choice([0, 0, 2, 10, 40, 72, 100, 120, 127]))
            t += w
        roll[C - 1][rng.rand(128, T) < 0.01] = 3
    return roll


def _blank(C, T=HAND_T):
    return np.zeros((C, 128, T), dtype=np.uint8)


def _note(roll, p, s, e, v=90, onset=True):
    roll[0, p, s:e] = v
    if roll.shape[0] == 3 and onset:
        roll[1, p, s] = 127


def hand_built():
    out = {}
    for C in (1, 2, 3):
        out[f"silence.c{C}"] = _blank(C)
        r = _blank(C)
        _note(r, 60, 10, 30)
        out[f"one_note.c{C}"] = r
        r = _blank(C)
        _note(r, 50, 40, HAND_T, 70)
        _note(r, 77, 5, 9, 33)
        out[f"to_the_end.c{C}"] = r
        r = _blank(C)
        _note(r, 64, 28, 29, 80)
        _note(r, 65, 57, 59, 81)
        _note(r, 66, 56, 58, 82)
        out[f"col_shift.c{C}"] = r
        r = _blank(C)
        r[0, 5, 3:8] = 40
        r[0, 20, 50] = 55
        _note(r, 60, 10, 30, 55)
        _note(r, 62, 12, 33, 56)
        _note(r, 70, 20, 25, 100)
        out[f"background.c{C}"] = r
        r = _blank(C)
        _note(r, 109, 4, 40, 60)
        _note(r, 127, 10, 70, 61)
        _note(r, 108, 11, 12, 62)
        out[f"above_piano.c{C}"] = r
        for a, (e, s) in {"a": (6, 1), "b": (5, 0), "c": (35, 40), "d": (47, 52), "e": (68, 63)}.items():
            r = _blank(C)                                            # a note ending at e and another starting at s, five columns apart
            _note(r, 60, max(0, e - 3), e, 90)
            _note(r, 67, s, s + 2, 91)
            out[f"five_apart_{a}.c{C}"] = r
    r = _blank(3)
    r[0, 60, 10:20] = 90
    r[1, 60, 20] = 127
    out["zero_length_only.c3"] = r
    r = _blank(3)
    r[0, 60, 0:20] = 90                                               # sounds in column 0, no onset: dropped, kept with first_column_onsets
    _note(r, 72, 30, 40)
    _note(r, 74, 33, 44)
    out["column0_no_onset.c3"] = r
    r = _blank(3)
    _note(r, 60, 10, 20, onset=False)
    r[1, 60, 10] = 63
    _note(r, 61, 10, 20, onset=False)
    r[1, 61, 10] = 64
    _note(r, 62, 30, 50)
    out["onset_63_64.c3"] = r
    r = _blank(3)
    _note(r, 60, 10, 50)
    r[1, 60, 25] = 127
    r[1, 60, 26] = 100
    r[1, 60, 50] = 127                                                # ... and a zero-length note behind a re-struck run
    _note(r, 64, 49, 60)
    out["restruck.c3"] = r
    for C in (2, 3):
        r = _blank(C)
        _note(r, 60, 2, 8)
        _note(r, 64, 30, 34)
        for k, v in enumerate((2, 10, 40, 100, 120, 127)):
            r[C - 1, 21:109, 12 * k:12 * k + 9] = v
        out[f"pedal_plateaus.c{C}"] = r
        r = _blank(C)
        _note(r, 60, 10, 20)
        _note(r, 62, 40, 45, 50)
        r[C - 1, 21:109, 15:70] = 127
        out[f"pedal_never_released.c{C}"] = r
        r = _blank(C)
        _note(r, 60, 10, 20, 100)
        _note(r, 60, 30, 36, 40)
        _note(r, 64, 22, 26, 70)
        _note(r, 70, 58, 60, 20)
        r[C - 1, 21:109, 12:14] = 127                                 # pressed, a gap of zeros, released at 57..58 over notes that ended inside
        r[C - 1, 21:109, 57:59] = 20
        r[C - 1, 21:109, 59:61] = 100                                 # pressed again in the column the release maps to
        r[C - 1, 21:109, 75] = 40
        out[f"pedal_running_max.c{C}"] = r
        r = _blank(C)
        r[C - 1, 21:109, 5:9] = 127                                   # pedal events but no note
        out[f"pedal_only.c{C}"] = r
    return out


def cases():
    out = {}
    k = 0
    for T in RANDOM_T:
        for C in (1, 2, 3):
            for i in range(N_SEEDS):
                out[f"random.t{T}.c{C}.s{i}"] = random_roll(SEED + k, C, T)
                k += 1
    out.update(hand_built())
    return out


def pack(stats):
    """a note-statistics dict (numpy values) -> (148 int64, 16 float64) in the layout of the kernel's outputs"""
    ints = np.concatenate([[int(stats[k]) for k in INT_FIELDS], np.asarray(stats["pitch_class_transition_matrix"]).reshape(-1)]).astype(np.int64)
    real = np.concatenate([[float(stats[k]) for k in REAL_FIELDS], np.asarray(stats["total_pitch_class_histogram"], dtype=np.float64)])
    return ints, real


def check(ints, real, gi, gr, what):
    """the comparison rules of the issue, against the golden (gi, gr) of one case: integers and the NaN pattern exact, histogram and
    notes per second within one ulp, mean duration and average IOI within 4 n 2^-53 end_time.  Returns the largest differences."""
    assert np.array_equal(ints, gi), f"{what}: integers {ints[:4]} != {gi[:4]} or transition counts differ ({int((ints[4:] != gi[4:]).sum())} cells)"
    assert np.array_equal(np.isnan(real), np.isnan(gr)), f"{what}: NaN pattern {real} != {gr}"
    n, end_time = int(gi[0]), float(gr[0])
    assert real[0] == gr[0], f"{what}: end_time {real[0]!r} != {gr[0]!r}"
    ok = ~np.isnan(gr)
    ulp = np.zeros(16)
    ulp[ok] = np.abs(real[ok] - gr[ok]) / np.maximum(np.abs(gr[ok]), 1e-300)
    one = [3] + list(range(4, 16))
    assert (ulp[one] <= 2.0 ** -52).all(), f"{what}: histogram / notes per second off by {ulp[one].max():.3e} relative"
    bound = 4 * n * 2.0 ** -53 * end_time
    d = np.zeros(16)
    d[ok] = np.abs(real[ok] - gr[ok])
    assert d[1] <= bound and d[2] <= bound, f"{what}: avg_IOI off by {d[1]:.3e}, mean duration by {d[2]:.3e}, bound {bound:.3e}"
    return float(ulp[one].max()), float(max(d[1], d[2]))
