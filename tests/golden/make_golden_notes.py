#!/usr/bin/env python3
"""Generate tests/golden/notes.npz by IMPORTING the reference:  `python tests/golden/make_golden_notes.py`.

Runs only in the build container, like the other generators; no test imports this file or the reference.  For every roll of
tests/notes_cases.py it calls the reference's piano_roll_to_pretty_midi (music_rule_guidance/piano_roll_to_chord.py:167-275) on a copy,
with the reference's vendored pretty_midi fork under the name `pretty_midi` (it imports with `mido` stubbed: only file I/O needs mido),
and the eight methods of music_evaluation/mgeval/core.py's `metrics` on the object, once as it is and once with the onset channel's
first column set as save_piano_roll_midi (guided_diffusion/midi_util.py:81-85) sets it before it writes a file.

    notes.npz
        seed, n_seeds               tests/notes_cases.py rebuilds every roll from these
        names                       the cases, in order
        ints  (cases, 2, 148)       n, used pitches, pitch range, mean velocity, 144 transition counts; [:, 1] with first-column onsets
        real  (cases, 2, 16)        end_time, avg_IOI, mean duration, notes per second, 12 histogram values
        reference_raises            what the fork's get_pitch_class_transition_matrix raises as shipped under this numpy
The reference's own time per T = 1064, C = 3 excerpt is printed (docs/rounds/notes.md reports it), not stored: the file regenerates bit for bit.

As shipped the fork's transition matrix dies in np.histogram2d(normed=...) (instrument.py:336-339); for that one call `normed` is mapped
to `density` and the unshimmed exception text is recorded.  Asserted here: every random roll has at least two notes, and the
reference counts at least one pair of a note end and a note start five columns apart and rejects at least one."""
import importlib.util
import io
import os
import sys
import time
import types
import warnings
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_shims  # noqa: E402
import notes_cases as nc  # noqa: E402  (tests/notes_cases.py)

REF = ref_shims.REF_ROOT


def load_reference():
    ref_shims.install()
    sys.modules.setdefault("matplotlib", types.ModuleType("matplotlib"))
    spec = importlib.util.spec_from_file_location("pretty_midi", os.path.join(REF, "pretty_midi", "__init__.py"),
                                                  submodule_search_locations=[os.path.join(REF, "pretty_midi")])
    rpm = importlib.util.module_from_spec(spec)
    sys.modules["pretty_midi"] = rpm                      # replaces ref_shims' inert stand-in: mgeval and the reference import this name
    spec.loader.exec_module(rpm)
    from music_rule_guidance import piano_roll_to_chord as rp2c
    rp2c.pretty_midi = rpm
    spec = importlib.util.spec_from_file_location("ref_mgeval_core", os.path.join(REF, "music_evaluation", "mgeval", "core.py"))
    core = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(core)
    return rpm, rp2c, core


def reference_stats(rp2c, core, roll, first_column_onsets, pairs):
    cur = roll.astype(np.int64)                           # a copy: the reference writes into its input
    if first_column_onsets and cur.shape[0] == 3:
        cur[1, cur[0, :, 0].nonzero()[0], 0] = 127        # midi_util.py:81-85
    pm = rp2c.piano_roll_to_pretty_midi(cur[0] if cur.shape[0] == 1 else cur, fs=100)
    f = {"pretty_midi": pm}
    m = core.metrics()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        s = {"n_notes": len(pm.instruments[0].notes), "end_time": pm.get_end_time(),
             "total_used_pitch": m.total_used_pitch(f), "pitch_range": m.pitch_range(f), "avg_IOI": m.avg_IOI(f),
             "total_pitch_class_histogram": m.total_pitch_class_histogram(f), "mean_note_velocity": m.mean_note_velocity(f),
             "mean_note_duration": m.mean_note_duration(f), "note_density_mgeval": m.note_density(f),
             "pitch_class_transition_matrix": m.pitch_class_transition_matrix(f, normalize=0)}
    M = np.asarray(s["pitch_class_transition_matrix"])
    assert np.array_equal(M, np.round(M))
    for a in pm.instruments[0].notes if pairs is not None and len(pm.instruments[0].notes) > 1 else []:
        for b in pm.instruments[0].notes:
            if round(abs(a.end - b.start) * 100) == 5:
                pairs[bool(abs(a.end - b.start) < 0.05)] += 1
    return s


def save(path, arrs):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:       # np.savez's layout with a fixed time stamp: regenerates bit for bit
        for k, v in arrs.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), compress_type=zipfile.ZIP_DEFLATED)
    assert os.path.getsize(path) < 1024 * 1024
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


def main():
    rpm, rp2c, core = load_reference()
    # the fork's transition matrix as shipped
    ins = rpm.Instrument(program=0)
    ins.notes += [rpm.Note(velocity=90, pitch=60, start=0.0, end=0.5), rpm.Note(velocity=90, pitch=62, start=0.5, end=1.0)]
    try:
        ins.get_pitch_class_transition_matrix()
        raises = ""
    except Exception as e:                                # noqa: BLE001
        raises = f"{type(e).__name__}: {e}"
    print("as shipped:", raises or "no exception")
    if raises:
        h2d = np.histogram2d
        import pretty_midi.instrument as rinst

        def histogram2d(x, y, bins=10, range=None, normed=None, weights=None, density=None):
            return h2d(x, y, bins=bins, range=range, density=normed if density is None else density, weights=weights)
        rinst.np = types.SimpleNamespace(**{k: getattr(np, k) for k in dir(np) if not k.startswith("__")})
        rinst.np.histogram2d = histogram2d
    cases = nc.cases()
    names = list(cases)
    ints, real = np.zeros((len(names), 2, 148), dtype=np.int64), np.zeros((len(names), 2, 16))
    pairs = {True: 0, False: 0}
    for i, name in enumerate(names):
        for fco in (0, 1):
            s = reference_stats(rp2c, core, cases[name], bool(fco), pairs)
            ints[i, fco], real[i, fco] = nc.pack(s)
        if name.startswith("random."):
            assert ints[i, 0, 0] >= 2, (name, ints[i, 0, :4])
    print(f"{len(names)} cases; pairs five columns apart: {pairs[True]} counted, {pairs[False]} rejected")
    assert pairs[True] >= 1 and pairs[False] >= 1
    big = [cases[n] for n in names if n.startswith("random.t1064.c3.")]
    t0 = time.perf_counter()
    for r in big:
        reference_stats(rp2c, core, r, False, None)
    per = (time.perf_counter() - t0) / len(big)
    print(f"reference: {per * 1e3:.2f} ms per T = 1064, C = 3 excerpt")
    save(os.path.join(HERE, "notes.npz"), {
        "seed": np.array([nc.SEED], dtype=np.int64), "n_seeds": np.array([nc.N_SEEDS], dtype=np.int64), "names": np.array(names),
        "ints": ints, "real": real, "reference_raises": np.array(raises)})


if __name__ == "__main__":
    main()
