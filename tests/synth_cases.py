"""Rolls and host answers shared by the synthesis tests (tests/test_synth_host.py, tests/test_gpu_synth.py) and the fixture generator
(tests/golden/make_golden_synth.py).  The oracle of every GPU test is the product's host partner, synthesize_roll on a COPY of the roll
(it writes into its argument), which tests/golden/synth.npz pins to the reference's fork bit for bit."""
import numpy as np

SEED = 7300                                             # pinned by name: tests/golden/synth.npz stores it
FS = 100
SMALL_RATES = (50, 100, 8000)
BIG_RATES = (22050, 44100)


def _note(r, p, a, b, vel, onset=True):
    r[0, p, a:b] = vel
    if r.shape[0] == 3 and onset:
        r[1, p, a] = 127


def feature_roll(C, T):
    """(C, 128, T) uint8 with, as far as C allows: onset cuts inside a run, a zero-length note (an onset one column past its run), notes
    of 1, 2, 3, 4, 10, 11 and 12 columns (0, 1 and 2 audio samples at 50 / 100 Hz; F and F + 1 samples at 50, 100 and 8000 Hz where the
    truncations allow), two notes contiguous at a cut, a chord, a low background, a pedal event after the last note, and seeded random
    notes on top"""
    rng = np.random.RandomState(SEED + 10 * C + T)
    r = np.zeros((C, 128, T), dtype=np.uint8)
    r[0, 5, 1] = 6                                      # the background level
    for j, n in enumerate((1, 2, 3, 4, 10, 11, 12)):
        for rep, a in enumerate((0, 3, 7)):
            if a + n <= T - 2:
                _note(r, 30 + 3 * j + rep, a, a + n, 40 + 5 * j + rep)
    if T >= 24:
        _note(r, 60, 2, 20, 90)
        if C == 3:
            r[1, 60, 9], r[1, 60, 14] = 127, 64         # onset cuts: (2, 9), (9, 14), (14, 20)
            _note(r, 62, 4, 8, 70)
            r[1, 62, 8] = 127                           # a zero-length note (8, 8) behind (4, 8)
            _note(r, 63, 5, 12, 75, onset=False)        # a run without an onset: no note
        _note(r, 64, 2, 20, 80)
        _note(r, 67, 2, 20, 85)
    for _ in range(6 if T >= 24 else 2):
        p, a = int(rng.randint(70, 109)), int(rng.randint(0, T - 3))
        b = min(T - 2, a + int(rng.randint(1, 30)))
        if b > a and not r[0, p, max(0, a - 1):b + 1].any():
            _note(r, p, a, b, int(rng.randint(20, 128)))
    if C >= 2:
        r[C - 1, 21:109, 1:4] = 100
        r[C - 1, 21:109, T - 1] = 90                    # a pedal event after the last note: it sets the length
    return r


def fixture_rolls():
    """name -> roll of the fixture: 3-, 2- and 1-channel rolls of T <= 64, rendered at SMALL_RATES, and one of T = 8 at BIG_RATES"""
    big = np.zeros((3, 128, 8), dtype=np.uint8)
    _note(big, 57, 0, 5, 100)
    _note(big, 61, 1, 2, 64)
    _note(big, 64, 2, 7, 80)
    big[1, 64, 4] = 127
    big[2, 21:109, 7] = 50
    return {"c3": feature_roll(3, 64), "c2": feature_roll(2, 48), "c1": feature_roll(1, 33), "big": big,
            "empty": np.zeros((3, 128, 16), dtype=np.uint8)}


def fixture_cases():
    """[(case name, roll name, audio_fs)]"""
    out = [(f"{n}.{r}", n, r) for n in ("c3", "c2", "c1", "empty") for r in SMALL_RATES]
    return out + [(f"big.{r}", "big", r) for r in BIG_RATES]


def host_input(roll, first_column_onsets=False):
    """a float32 copy in the form the host functions take: (128, T) for one channel, the forced onsets of column 0 applied on request"""
    cur = np.array(roll)
    if cur.ndim == 3 and cur.shape[0] == 1:
        cur = cur[0]
    if first_column_onsets and cur.ndim == 3 and cur.shape[0] == 3:
        cur[1, np.nonzero(cur[0, :, 0])[0], 0] = 127
    return cur.astype(np.float32)


def host_render(roll, fs=FS, audio_fs=44100, first_column_onsets=True):
    """one uint8 roll -> dict of the host partner's answers: raw (L,) float64 un-normalised, silent, peak, and per audio sample m (the
    number of notes sounding) and V (the sum of their velocities), from the host's own note list"""
    from music_rule_guidance.piano_roll_to_chord import piano_roll_to_pretty_midi, synthesize_events
    pm = piano_roll_to_pretty_midi(host_input(roll, first_column_onsets), fs=fs)
    raw = synthesize_events(pm, audio_fs)
    m, V = np.zeros(raw.shape[0], dtype=np.int64), np.zeros(raw.shape[0], dtype=np.int64)
    spans = []
    for n in pm.instruments[0].notes:
        a, b = int(audio_fs * n.start), int(audio_fs * n.end)
        m[a:b] += 1
        V[a:b] += n.velocity
        spans.append((n.pitch, a, b))
    peak = float(np.abs(raw).max()) if raw.shape[0] else 0.0
    return {"raw": raw, "silent": not peak > 0, "peak": peak, "m": m, "V": V, "spans": spans, "n_notes": len(spans)}


def dense_roll(seed, C, T, density=0.3):
    """tests/midi_cases.py's random roll: runs of ~30 columns, onsets, pedal, a background"""
    import midi_cases as mc
    return mc.random_roll(seed, C, T, density)
