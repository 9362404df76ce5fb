"""Yardstick of the native chord and key analyser: a float64 / integer numpy restatement written from the definition in
docs/rounds/chords.md, plus the inputs the chord tests share.  It imports nothing from the product: tables, root scoring, slicing and
key finding are all spelled out again here, column by column, the slow and obvious way."""
import numpy as np

LOW, HIGH = 21, 108
PROFILES = {
    "krumhansl": ([6.35, 2.23, 3.48, 2.33, 4.38, 4.09, 2.52, 5.19, 2.39, 3.66, 2.29, 2.88],
                  [6.33, 2.68, 3.52, 5.38, 2.60, 3.53, 2.54, 4.75, 3.98, 2.69, 3.34, 3.17]),
    "aarden": ([17.7661, 0.145624, 14.9265, 0.160186, 19.8049, 11.3587, 0.291248, 22.062, 0.145624, 8.15494, 0.232998, 4.95122],
               [18.2648, 0.737619, 14.0499, 16.8599, 0.702494, 14.4362, 0.702494, 18.6161, 4.56621, 1.93186, 7.37619, 1.75623]),
}
DEGREE = [1, 2, 2, 3, 3, 4, 4, 5, 6, 6, 7, 7]
MAJOR_NAMES = ["C", "C#", "D", "E-", "E", "F", "F#", "G", "A-", "A", "B-", "B"]
MINOR_NAMES = ["c", "c#", "d", "e-", "e", "f", "f#", "g", "g#", "a", "b-", "b"]
KEY_CLASS = {"D major": 0, "g minor": 1, "B- major": 2, "G major": 3, "d minor": 4, "c# minor": 5, "F major": 6, "E- major": 7,
             "e minor": 8, "f# minor": 9, "C major": 10, "F# major": 11, "g# minor": 12, "A major": 13, "a minor": 14, "B major": 15,
             "A- major": 16, "b- minor": 17, "E major": 18, "c minor": 19, "b minor": 20, "e- minor": 21, "f minor": 22, "C# major": 23,
             "no key": 24}


def key_name(k):
    return "no key" if k < 0 else (MAJOR_NAMES[k] + " major" if k < 12 else MINOR_NAMES[k - 12] + " minor")


def key_class(k):
    return KEY_CLASS[key_name(k)]


def root_of(pitches):
    classes = set(p % 12 for p in pitches)
    bass = min(pitches) % 12
    ranked = []
    for r in classes:
        score = 0
        if (r + 7) % 12 in classes:
            score += 8
        if (r + 4) % 12 in classes or (r + 3) % 12 in classes:
            score += 4
        if (r + 6) % 12 in classes:
            score += 3
        if (r + 10) % 12 in classes or (r + 11) % 12 in classes:
            score += 2
        ranked.append((-score, (r - bass) % 12, r))
    return min(ranked)[2]


def correlations(q, profile="krumhansl"):
    """-> (r (24,) float64 or None when the duration profile has no variance, D (12,) ints)"""
    on = np.asarray(q)[LOW:HIGH + 1] > 0
    D = np.zeros(12, dtype=np.int64)
    for i in range(on.shape[0]):
        D[(LOW + i) % 12] += int(on[i].sum())
    d = D.astype(np.float64) - D.astype(np.float64).mean()
    if float((d * d).sum()) == 0.0:
        return None, D
    r = np.zeros(24)
    for mode in range(2):
        P = np.array(PROFILES[profile][mode], dtype=np.float64)
        for tonic in range(12):
            y = np.array([P[(c - tonic) % 12] for c in range(12)])
            y = y - y.mean()
            r[12 * mode + tonic] = (d * y).sum() / np.sqrt((d * d).sum() * (y * y).sum())
    return r, D


def window_roots(q, wc):
    on = np.asarray(q)[LOW:HIGH + 1] > 0
    roots = []
    for w in range(on.shape[1] // wc):
        cols = on[:, w * wc:(w + 1) * wc]
        best_len, best_t, t = 0, None, 0
        while t < wc:
            u = t + 1
            while u < wc and np.array_equal(cols[:, u], cols[:, t]):
                u += 1
            if cols[:, t].any() and u - t > best_len:
                best_len, best_t = u - t, t
            t = u
        roots.append(-1 if best_t is None else root_of([LOW + int(i) for i in np.nonzero(cols[:, best_t])[0]]))
    return roots


def analyse(q, wc, profile="krumhansl", given_tonic=None, analyse_key=True):
    """-> dict(chords, roots, key (-1: none), coef, gap = best minus second-best r_k, inf without a key analysis / a key)"""
    roots = window_roots(q, wc)
    key, coef, gap = -1, 0.0, float("inf")
    if analyse_key:
        r, _ = correlations(q, profile)
        if r is None:
            return dict(chords=[0] * len(roots), roots=roots, key=-1, coef=0.0, gap=gap)
        key = int(np.argmax(r))
        coef = float(r[key])
        top = np.sort(r)
        gap = float(top[-1] - top[-2])
    tonic = given_tonic if given_tonic is not None else key % 12
    chords = [0 if x < 0 else DEGREE[(x - tonic) % 12] for x in roots]
    return dict(chords=chords, roots=roots, key=key, coef=coef, gap=gap)


# ---------------------------------------------------------------------------------------------------------------- shared inputs
def random_roll(seed, T):
    """(128, T) uint8 of note events: block chords held for a while (long slices), melody notes over them (short slices), rests, velocity
    changes inside held notes, and junk outside the piano range."""
    rng = np.random.default_rng(1000 + seed)
    q = np.zeros((128, T), dtype=np.uint8)
    t = 0
    while t < T:
        dur = int(rng.integers(3, 90))
        kind = rng.random()
        if kind < 0.15:
            t += dur                                   # a rest
            continue
        base = int(rng.integers(30, 80))
        for iv in rng.choice([0, 3, 4, 7, 10, 11, 12, 15, 16], size=int(rng.integers(1, 5)), replace=False):
            p = base + int(iv)
            q[p, t:t + dur] = rng.integers(1, 128)
            if rng.random() < 0.3:                     # velocity change inside the held note
                q[p, t + dur // 2:t + dur] = rng.integers(1, 128)
        t += dur
    for _ in range(int(rng.integers(0, 12))):          # melody / pedal notes across the chord changes, the extreme pitches included
        p = int(rng.choice([21, 22, 84, 85, 86, 107, 108, int(rng.integers(21, 109))]))
        s = int(rng.integers(0, T))
        q[p, s:s + int(rng.integers(1, 200))] = rng.integers(1, 128)
    q[:LOW, :] = rng.integers(0, 128, size=(LOW, T))   # junk below and above the piano range: must be ignored
    q[HIGH + 1:, :] = rng.integers(0, 128, size=(127 - HIGH, T))
    return q


PROGRESSION = [1, 4, 5, 1, 6, 2, 5, 1]


def progression_roll(tonic, minor, T=1024, wc=128, seed=0):
    """I-IV-V-I-vi-ii-V-I (one triad per window) in random inversions, with a 3-column pickup note and a lone bass tail in every window
    -> (roll (128, T) uint8, the degrees)."""
    rng = np.random.default_rng(seed)
    q = np.zeros((128, T), dtype=np.uint8)
    scale = [0, 2, 3, 5, 7, 8, 10] if minor else [0, 2, 4, 5, 7, 9, 11]
    degs = [PROGRESSION[w % 8] for w in range(T // wc)]
    pick, tail = max(1, wc * 3 // 128), max(2, wc * 20 // 128)
    for w, d in enumerate(degs):
        tri = [scale[(d - 1 + j) % 7] + (12 if d - 1 + j >= 7 else 0) for j in (0, 2, 4)]
        inv = int(rng.integers(0, 3))
        ps = [48 + tonic + x for x in tri]
        ps = ps[inv:] + [p + 12 for p in ps[:inv]]
        q[ps, w * wc + pick:(w + 1) * wc - tail] = rng.integers(1, 128)
        q[72 + tonic + scale[int(rng.integers(0, 7))], w * wc:w * wc + pick] = 90          # the pickup: a slice of its own
        q[ps[0], (w + 1) * wc - tail:(w + 1) * wc - tail // 4] = 50                        # a lone bass note, shorter than the chord
    return q, degs


def float_roll(q, channels=3, seed=0):
    """integer roll(s) (..., 128, T) -> float roll (N, channels, 128, T) in [-1, 1] whose chord quantisation has the same active piano cells
    as q: (v + 0.5) / 63.5 - 1 lies strictly inside quantisation cell v, and velocities 1 and 2 are raised to 3 (the preamble snaps
    everything below -0.95, i.e. below 3.175 / 127, to silence).  Silent piano cells lie anywhere in [-1, -0.951] and the rows outside the
    piano range and the other channels hold noise, so the preamble has something to write."""
    q = np.asarray(q)
    q = q[None] if q.ndim == 2 else q
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, size=(q.shape[0], channels, 128, q.shape[-1])).astype(np.float32)
    sound = (np.maximum(q, 3).astype(np.float32) + 0.5) / 63.5 - 1.0
    x[:, 0, LOW:HIGH + 1] = np.where(q > 0, sound, rng.uniform(-1, -0.951, size=q.shape).astype(np.float32))[:, LOW:HIGH + 1]
    return x


C_MAJ, D_MIN, E_MIN = [60, 64, 67], [62, 65, 69], [64, 67, 71]          # roots 0, 2, 4


def hand_cases():
    """Rolls built by hand where a kernel can go wrong -> [(name, roll (128, T) uint8, wc, expected roots)].  Every roll carries junk
    that changes from column to column in rows 0..20 and 109..127: read, it would cut every slice to one column."""
    rng = np.random.default_rng(77)
    cases = []

    def roll(T):
        q = np.zeros((128, T), dtype=np.uint8)
        q[:LOW] = rng.integers(0, 128, size=(LOW, T))
        q[HIGH + 1:] = rng.integers(0, 128, size=(127 - HIGH, T))
        return q

    # slices that differ in one pitch only: found, the C major run is cut into 10 + 10 and D minor (12) wins; missed, C major (20) wins
    for p in (21, 108, 90, 85, 84):
        q = roll(32)
        q[C_MAJ, 0:20] = 70
        q[p, 0:10] = 33
        q[D_MIN, 20:32] = 70
        cases.append((f"one pitch apart at {p}", q, 32, [2]))
    # a slice across the window boundary (12 + 12 columns) loses in both windows to shorter slices inside them
    q = roll(64)
    q[D_MIN, 0:14] = 50
    q[C_MAJ, 20:44] = 50
    q[E_MIN, 44:59] = 50
    cases.append(("crossing slice loses", q, 32, [2, 4]))
    # two slices of equal length: the earlier one
    q = roll(64)
    q[C_MAJ, 0:10] = 50
    q[D_MIN, 10:20] = 50
    q[E_MIN, 32 + 5:32 + 14] = 50
    q[D_MIN, 32 + 14:32 + 23] = 50
    cases.append(("equal lengths, the earlier", q, 32, [0, 4]))
    # a silent run longer than any chord
    q = roll(32)
    q[E_MIN, 25:32] = 50
    cases.append(("long silence", q, 32, [4]))
    # a velocity change inside a held chord does not cut it (cut, D minor's 12 columns would win over 10 + 10)
    q = roll(32)
    q[C_MAJ, 0:10] = 40
    q[C_MAJ, 10:20] = 90
    q[D_MIN, 20:32] = 60
    cases.append(("velocity change", q, 32, [0]))
    # the only sound is the window's last column; the next window is silent
    q = roll(64)
    q[62, 31] = 1
    cases.append(("last column only", q, 32, [2, -1]))
    # root ties go to the bass: augmented triad on E, tritone on F#; and a clear root that is not the bass (C major, first inversion)
    q = roll(96)
    q[[64, 68, 72], 0:32] = 50
    q[[66, 72], 32:64] = 50
    q[[64, 67, 72], 64:96] = 50
    cases.append(("root ties", q, 32, [4, 6, 0]))
    # the largest window, each filled by one slice; the second holds the two extreme pitches only (A0 and C8: the root is A, by its third)
    q = roll(2048)
    q[[21, 108], 1024:2048] = 9
    q[C_MAJ, 0:1024] = 9
    cases.append(("widest window", q, 1024, [0, 9]))
    return cases
