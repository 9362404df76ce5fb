"""CPU: the host partner of csrc/synth.hip -- synthesize_roll, wav_bytes and the four host tables -- against the reference's vendored
pretty_midi fork (tests/golden/synth.npz, written by tests/golden/make_golden_synth.py), bit for bit (docs/rounds/synth.md)."""
import hashlib
import io
import wave

import numpy as np
import pytest

import synth_cases as sc
from conftest import load_golden


@pytest.fixture(scope="module")
def fixture():
    return load_golden("synth")


def test_the_fixture_holds_the_rolls_of_synth_cases(fixture):
    assert int(fixture["seed"][0]) == sc.SEED
    rolls = sc.fixture_rolls()
    for name, roll in rolls.items():
        assert np.array_equal(fixture[f"roll.{name}"], roll), name
    assert [tuple(c) for c in sc.fixture_cases()] == [(str(a), str(b), int(c)) for a, b, c in
                                                      zip(fixture["names"], fixture["roll_names"], fixture["rates"])]


def test_synthesize_roll_equals_the_reference_bit_for_bit(fixture):
    """the raw Instrument.synthesize sum, the normalised PrettyMIDI.synthesize result (by its sha256) and the lengths, on every case; the
    one departure: where the reference returns NaN throughout (no notes), zeros and the silent flag"""
    from music_rule_guidance.piano_roll_to_chord import synthesize_roll
    seen_nan = 0
    for i, (case, rname, rate) in enumerate(sc.fixture_cases()):
        roll = fixture[f"roll.{rname}"]
        raw = synthesize_roll(sc.host_input(roll), fs=sc.FS, audio_fs=rate, normalize=False)
        want = fixture[f"raw.{case}"]
        assert raw.dtype == np.float64 and raw.shape == want.shape == (int(fixture["length"][i]),), case
        assert raw.shape[0] == int(rate * (float(fixture["end_time"][i]) + 1)), case
        assert raw.tobytes() == want.tobytes(), f"{case}: raw sum differs, max |d| = {np.abs(raw - want).max():.3e}"
        norm, silent = synthesize_roll(sc.host_input(roll), fs=sc.FS, audio_fs=rate, return_silent=True)
        if int(fixture["norm_nan"][i]):
            seen_nan += 1
            assert int(fixture["n_notes"][i]) == 0 and silent and norm.shape == want.shape and not norm.any(), case
        else:
            assert not silent and hashlib.sha256(norm.tobytes()).hexdigest() == str(fixture["norm_sha256"][i]), case
            assert np.abs(norm).max() == 1.0
    assert seen_nan == len(sc.SMALL_RATES)


def test_the_fixture_rolls_hold_the_note_lengths_that_matter():
    """notes of 0, 1, 2, F and F + 1 audio samples, a zero-length note, two notes contiguous at a cut, a length set by a late pedal event"""
    seen = set()
    for rate in sc.SMALL_RATES:
        F = int(.1 * rate)
        for name in ("c3", "c2", "c1"):
            h = sc.host_render(sc.fixture_rolls()[name], audio_fs=rate, first_column_onsets=False)
            ns = {b - a for _, a, b in h["spans"]}
            seen |= {("n", n) for n in ns if n <= 2} | {("F", n - F) for n in ns if n in (F, F + 1)}
            ends = {(p, b) for p, a, b in h["spans"] if b > a}
            if any((p, a) in ends for p, a, b in h["spans"] if b > a):
                seen.add("contiguous")
            if h["raw"].shape[0] > max(b for _, _, b in h["spans"]) + rate:
                seen.add("late cc")
    assert seen >= {("n", 0), ("n", 1), ("n", 2), ("F", 0), ("F", 1), "contiguous", "late cc"}, seen
    from music_rule_guidance.piano_roll_to_chord import piano_roll_to_pretty_midi
    notes = piano_roll_to_pretty_midi(sc.host_input(sc.fixture_rolls()["c3"]), fs=sc.FS).instruments[0].notes
    assert any(n.start == n.end for n in notes)


def test_wav_bytes_round_trips_through_the_wave_module():
    from music_rule_guidance.piano_roll_to_chord import wav_bytes
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(-1, 1, 1000), [1.0, -1.0, 0.0, 0.5 / 32767, 1.5 / 32767, 2.5 / 32767, -0.5 / 32767]])
    for rate in (8000, 44100):
        data = wav_bytes(x, rate)
        assert len(data) == 44 + 2 * len(x) and data[:4] == b"RIFF" and data[8:16] == b"WAVEfmt "
        with wave.open(io.BytesIO(data), "rb") as w:
            assert (w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()) == (rate, 1, 2, len(x))
            pcm = np.frombuffer(w.readframes(len(x)), dtype="<i2")
        assert np.array_equal(pcm, np.rint(x * 32767).astype(np.int16))
        assert pcm[1000:].tolist() == [32767, -32767, 0, 0, 2, 2, 0]        # halves to even


@pytest.mark.parametrize("rate", [50, 100, 8000, 22050, 44100])
def test_the_host_tables_hold_the_host_partners_own_integers(rate):
    """every column k of T = 1 .. 1000: samp[k] and length[k] are the truncations synthesize_events forms of a note or event at k / fs,
    omega the phase increment it multiplies k by, fade its fade-out"""
    from music_rule_guidance.piano_roll_to_chord import synth_tables
    full = synth_tables(1000, sc.FS, rate)
    want_samp = np.array([int(rate * (k / sc.FS)) for k in range(1001)])
    want_len = np.array([int(rate * (k / sc.FS + 1)) for k in range(1001)])
    for T in range(1, 1001):
        samp, length, omega, fade = synth_tables(T, sc.FS, rate)
        assert samp.dtype == length.dtype == np.int64 and omega.dtype == fade.dtype == np.float64
        assert samp.shape == length.shape == (T + 1,) and omega.shape == (128,) and fade.shape == (int(.1 * rate),)
        assert np.array_equal(samp, want_samp[:T + 1]) and np.array_equal(length, want_len[:T + 1]), T
    assert (np.diff(full[0]) >= 0).all() and (np.diff(full[1]) >= 0).all() and (full[0] <= full[1]).all()
    for p in (0, 21, 60, 69, 108, 127):
        f = 440.0 * 2.0 ** ((p - 69) / 12.0)
        assert full[2][p] == 2 * np.pi * f * 1.0 / rate
        assert full[2][p] == (2 * np.pi * f * np.ones(1) / rate)[0]
    assert full[3].tobytes() == np.linspace(1, 0, int(.1 * rate)).tobytes()


def test_tables_refuse_what_the_device_cannot_serve():
    from music_rule_guidance.piano_roll_to_chord import synth_tables
    for bad in ((10, 100, 0), (10, 100, -8000), (10, 0, 8000), (32768, 1, 70000), (0, 100, 8000)):
        with pytest.raises(ValueError):
            synth_tables(*bad)


def _script(name):
    import importlib.util
    import os
    from conftest import PKG
    spec = importlib.util.spec_from_file_location(name + "_cli", os.path.join(PKG, "scripts", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_wav_flags_parse_and_leave_the_other_flag_sets_alone():
    cli = _script("sample_rule")
    before = set(vars(cli.create_argparser().parse_args([])))
    midi = set(vars(cli.add_midi_arguments(cli.create_argparser()).parse_args([])))
    parser = cli.add_wav_arguments(cli.create_argparser())
    a = parser.parse_args([])
    assert a.wav == "off" and a.wav_fs == 44100
    a = parser.parse_args(["--wav", "device", "--wav_fs", "16000"])
    assert a.wav == "device" and a.wav_fs == 16000
    with pytest.raises(SystemExit):
        parser.parse_args(["--wav", "host"])
    assert set(vars(parser.parse_args([]))) == before | {"wav", "wav_fs"} and not {"wav", "wav_fs"} & (before | midi)
    from types import SimpleNamespace
    assert cli.device_wav_bytes(None, SimpleNamespace(wav="off", fs=100, wav_fs=44100)) is None       # off touches nothing
    assert _script("rolls_to_wav").create_argparser().parse_args(["--roll_dir", "a", "--outdir", "b"]).wav_fs == 44100


def test_save_piano_roll_midi_writes_given_wav_bytes_beside_the_midi(tmp_path):
    import os
    from guided_diffusion import midi_util
    rolls = np.stack([sc.fixture_rolls()["c3"], sc.fixture_rolls()["empty"].repeat(4, axis=2)])
    midi_util.save_piano_roll_midi(rolls, str(tmp_path / "a"), fs=100, y=np.array([2, 2]), save_ind=5, midi_bytes=[b"MThd-0", b"MThd-1"],
                                   wav_bytes=[b"RIFF-0", b"RIFF-1"])
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f"sample_{i}_y_2.{e}" for i in (5, 6) for e in ("midi", "npy", "wav"))
    assert open(tmp_path / "a" / "sample_6_y_2.wav", "rb").read() == b"RIFF-1"
    with pytest.raises(ValueError, match="wav_bytes holds 1 files for 2 rolls"):
        midi_util.save_piano_roll_midi(rolls, str(tmp_path / "b"), wav_bytes=[b""])
    midi_util.save_piano_roll_midi(rolls, str(tmp_path / "c"), fs=100)      # the default: no .wav
    assert not [f for f in os.listdir(tmp_path / "c") if f.endswith(".wav")]
