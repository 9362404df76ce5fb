#!/usr/bin/env python3
"""Generate tests/golden/synth.npz by IMPORTING the reference:  `python tests/golden/make_golden_synth.py`.

Runs only in the build container, like the other generators; no test imports this file or the reference.  For every case of
tests/synth_cases.py (fixture_cases) it calls the reference's piano_roll_to_pretty_midi (music_rule_guidance/piano_roll_to_chord.py:167-275)
on a float copy of the roll, with the reference's vendored pretty_midi fork under the name `pretty_midi` (it imports with `mido` stubbed:
only file I/O needs mido), then the fork's Instrument.synthesize(fs=audio_fs) (pretty_midi/instrument.py:355-441) and
PrettyMIDI.synthesize(fs=audio_fs) (pretty_midi/pretty_midi.py:954-983).

    synth.npz
        seed                        tests/synth_cases.py SEED: the rolls are stored too, the seed says how they were made
        roll.<name>                 the uint8 rolls
        names, roll_names, rates    the cases, in order
        end_time, length            per case: get_end_time() and the number of samples
        n_notes                     per case
        raw.<case>                  Instrument.synthesize: the un-normalised float64 sum
        norm_sha256                 per case: sha256 of the bytes of PrettyMIDI.synthesize's float64 result (bit-for-bit without its size)
        norm_nan                    per case: 1 where the reference's normalised result is NaN throughout (a roll without notes: 0 / 0)
The zero tails compress; the file stays under 1 MiB (asserted)."""
import hashlib
import importlib.util
import io
import os
import sys
import types
import warnings
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_shims  # noqa: E402
import synth_cases as sc  # noqa: E402  (tests/synth_cases.py)

REF = ref_shims.REF_ROOT


def load_reference():
    ref_shims.install()
    sys.modules.setdefault("matplotlib", types.ModuleType("matplotlib"))
    spec = importlib.util.spec_from_file_location("pretty_midi", os.path.join(REF, "pretty_midi", "__init__.py"),
                                                  submodule_search_locations=[os.path.join(REF, "pretty_midi")])
    rpm = importlib.util.module_from_spec(spec)
    sys.modules["pretty_midi"] = rpm
    spec.loader.exec_module(rpm)
    from music_rule_guidance import piano_roll_to_chord as rp2c
    rp2c.pretty_midi = rpm
    return rpm, rp2c


def save(path, arrs):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:       # np.savez's layout with a fixed time stamp: regenerates bit for bit
        for k, v in arrs.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), compress_type=zipfile.ZIP_DEFLATED)
    assert os.path.getsize(path) < 1024 * 1024
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


def main():
    rpm, rp2c = load_reference()
    rolls, cases = sc.fixture_rolls(), sc.fixture_cases()
    out = {"seed": np.array([sc.SEED], dtype=np.int64)}
    out.update({f"roll.{k}": v for k, v in rolls.items()})
    end_time, length, n_notes, sha, nan = [], [], [], [], []
    for case, rname, rate in cases:
        pm = rp2c.piano_roll_to_pretty_midi(sc.host_input(rolls[rname]), fs=sc.FS)
        ins = pm.instruments[0]
        raw = ins.synthesize(fs=rate)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with np.errstate(all="ignore"):
                norm = pm.synthesize(fs=rate)
        assert raw.dtype == np.float64 and norm.dtype == np.float64 and raw.shape == norm.shape
        out[f"raw.{case}"] = raw
        end_time.append(pm.get_end_time())
        length.append(raw.shape[0])
        n_notes.append(len(ins.notes))
        nan.append(int(np.isnan(norm).all()))
        sha.append(hashlib.sha256(np.ascontiguousarray(norm).tobytes()).hexdigest())
        print(f"    {case}: {len(ins.notes)} notes, end {end_time[-1]:.2f} s, {raw.shape[0]} samples, peak {np.abs(raw).max():.3f}, NaN {nan[-1]}")
    assert any(nan) and not all(nan)
    out.update({"names": np.array([c[0] for c in cases]), "roll_names": np.array([c[1] for c in cases]),
                "rates": np.array([c[2] for c in cases], dtype=np.int64), "end_time": np.array(end_time), "length": np.array(length, dtype=np.int64),
                "n_notes": np.array(n_notes, dtype=np.int64), "norm_sha256": np.array(sha), "norm_nan": np.array(nan, dtype=np.int64)})
    save(os.path.join(HERE, "synth.npz"), out)


if __name__ == "__main__":
    main()
