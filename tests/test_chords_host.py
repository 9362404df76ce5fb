"""CPU: the native chord analyser's host side -- piano_roll_to_chords_native against the restatement (tests/chords_ref.py), key-string
parsing, window validation, backend registration and the CLI switch.  Comparison rules (docs/rounds/chords.md): chords, roots, key
and the "no key" cases equal exactly, every input with a gap >= 1e-9 between the best and second-best key correlation in the
restatement (asserted, never skipped), the coefficient within 1e-12 absolute."""
import importlib.util
import os
from types import SimpleNamespace

import numpy as np
import pytest

import chords_ref as ref
from conftest import PKG
from music_rule_guidance import music_rules
from music_rule_guidance import piano_roll_to_chord as p2c

SEEDS = range(40)
MIN_GAP, COEF_TOL = 1e-9, 1e-12


@pytest.fixture
def no_backend():
    music_rules.register_chord_backend(None)
    yield
    music_rules.register_chord_backend(None)


def check_against_ref(q, wc, profile="krumhansl"):
    want = ref.analyse(q, wc, profile)
    assert want["gap"] >= MIN_GAP, want["gap"]
    got = p2c.piano_roll_to_chords_native(q.astype(np.intc), return_key=True, fs=100., window_size=wc / 100., profile=profile)
    assert got["chords"].dtype == np.int64 and got["chords"].tolist() == want["chords"]
    assert got["key"] == ref.key_class(want["key"])
    assert abs(got["correlationCoefficient"] - want["coef"]) <= COEF_TOL
    assert p2c.native_roots(q[21:109] > 0, wc).tolist() == want["roots"]
    return want


@pytest.mark.parametrize("T", [128, 1024, 1064])
@pytest.mark.parametrize("wc", [16, 100, 128])
def test_host_analyser_matches_the_restatement_on_random_rolls(T, wc):
    keys = set()
    for seed in SEEDS:
        want = check_against_ref(ref.random_roll(seed, T), wc, "krumhansl" if seed % 2 == 0 else "aarden")
        assert len(want["chords"]) == T // wc
        keys.add(want["key"])
    assert len(keys) > 3                                       # the inputs do not all land in one key


@pytest.mark.parametrize("profile", ["krumhansl", "aarden"])
def test_progression_is_recovered_in_all_24_keys(profile):
    for minor in (0, 1):
        for tonic in range(12):
            q, degs = ref.progression_roll(tonic, minor, seed=tonic + 12 * minor)
            want = check_against_ref(q, 128, profile)
            name = ref.key_name(12 * minor + tonic)
            got = p2c.piano_roll_to_chords_native(q, return_key=True, profile=profile)
            assert got["chords"].tolist() == degs and want["chords"] == degs
            assert got["key"] == music_rules.KEY_DICT[name] and music_rules.IND2KEY[got["key"]] == name
            assert got["correlationCoefficient"] > 0.5


def test_pixel_window_progression():
    """fs 12.5 (chord_progression_pixel): 16 columns per window"""
    q, degs = ref.progression_roll(7, 0, T=128, wc=16, seed=3)
    assert ref.analyse(q, 16)["gap"] >= MIN_GAP
    got = p2c.piano_roll_to_chords_native(q, return_key=True, fs=12.5)
    assert got["chords"].tolist() == degs == ref.analyse(q, 16)["chords"] and got["key"] == music_rules.KEY_DICT["G major"]


def test_given_key_and_return_key_combinations():
    q, degs = ref.progression_roll(2, 0, seed=5)                # D major
    assert ref.analyse(q, 128)["gap"] >= MIN_GAP
    # given and not return_key: no key analysis, degrees relative to the given tonic
    out = p2c.piano_roll_to_chords_native(q, given_key="G major")
    assert set(out) == {"chords"}
    assert out["chords"].tolist() == ref.analyse(q, 128, given_tonic=7, analyse_key=False)["chords"] != degs
    # given and return_key: the given tonic for the degrees, the ANALYSED key and coefficient reported
    out = p2c.piano_roll_to_chords_native(q, given_key="G major", return_key=True)
    want = ref.analyse(q, 128, given_tonic=7)
    assert out["chords"].tolist() == want["chords"] and out["key"] == music_rules.KEY_DICT["D major"]
    assert abs(out["correlationCoefficient"] - want["coef"]) <= COEF_TOL
    # neither: analysed, and the dict still carries key and coefficient like the reference's
    out = p2c.piano_roll_to_chords_native(q)
    assert out["chords"].tolist() == degs and out["key"] == music_rules.KEY_DICT["D major"]
    # the mode word does not matter to the degrees
    assert p2c.piano_roll_to_chords_native(q, given_key="d")["chords"].tolist() == degs
    # silence: "no key" even with a given key when the key is analysed; with the key given and not analysed, silent windows are 0
    z = np.zeros((128, 1024), dtype=np.uint8)
    out = p2c.piano_roll_to_chords_native(z, given_key="C major", return_key=True)
    assert out["chords"].tolist() == [0] * 8 and out["key"] == music_rules.KEY_DICT["no key"] and out["correlationCoefficient"] == 0.0
    assert p2c.piano_roll_to_chords_native(z, given_key="C major")["chords"].tolist() == [0] * 8
    # tagging_func sees Roman numerals
    tagged = p2c.piano_roll_to_chords_native(q, tagging_func=lambda s: {"": 0, "I": 10, "IV": 40, "V": 50, "VI": 60, "II": 20}[s])
    assert tagged["chords"].tolist() == [10 * d for d in degs]


def test_silence_flat_profile_and_one_held_note():
    z = np.zeros((128, 1024), dtype=np.uint8)
    z[:21] = 99                                                 # junk outside the piano range is not sound
    z[109:] = 99
    flat = np.zeros((128, 256), dtype=np.uint8)
    flat[60:72, :] = 64                                         # every pitch class equally long: no variance, no key
    for q, W in ((z, 8), (flat, 2)):
        want = ref.analyse(q, 128)
        assert want["key"] == -1 and want["chords"] == [0] * W
        got = p2c.piano_roll_to_chords_native(q, return_key=True)
        assert got["chords"].tolist() == [0] * W and got["key"] == music_rules.KEY_DICT["no key"] == 24
        assert got["correlationCoefficient"] == 0.0
    assert ref.window_roots(flat, 128) == [0, 0] == p2c.native_roots(flat[21:109] > 0, 128).tolist()
    one = np.zeros((128, 1024), dtype=np.uint8)
    one[60] = 5
    assert check_against_ref(one, 128)["chords"] == [1] * 8
    assert p2c.piano_roll_to_chords_native(one)["chords"].tolist() == [1] * 8


def test_key_string_parsing_and_rejection():
    good = {"C major": 0, "c": 0, "c#": 1, "C# minor": 1, "D": 2, "e-": 3, "E- major": 3, "Eb": 3, "e minor": 4, "F": 5, "f# minor": 6,
            "G major": 7, "g#": 8, "A- major": 8, "a minor": 9, "b- minor": 10, "B- major": 10, "Bb": 10, "bb minor": 10, "B": 11,
            "b minor": 11, " b  MAJOR ": 11, "c-": 11}
    for s, pc in good.items():
        assert music_rules.parse_key(s) == pc, s
    for name in music_rules.CHORD_KEY_NAMES:
        assert music_rules.parse_key(name) == music_rules.CHORD_KEY_NAMES.index(name) % 12
        assert ref.key_name(music_rules.CHORD_KEY_NAMES.index(name)) == name and name in music_rules.KEY_DICT
    for bad in ("", "H major", "C## major", "C dorian", "major", "C major minor", "Cmajor", "1", None, 3, "c #"):
        with pytest.raises(ValueError):
            music_rules.parse_key(bad)
    with pytest.raises(ValueError):
        p2c.piano_roll_to_chords_native(np.zeros((128, 128), dtype=np.uint8), given_key="H")


def test_window_validation():
    assert music_rules.chord_window_columns(100, 1.28) == 128 and music_rules.chord_window_columns(12.5, 1.28) == 16
    assert music_rules.chord_window_columns(100., 1.) == 100 and music_rules.chord_window_columns(100, 10.24) == 1024
    assert music_rules.chord_window_columns(1, 1) == 1
    for fs, ws in ((100, 1.285), (100, 0.001), (100, 10.25), (0, 1.28), (100, 0.0), (12.5, 1.0), (100, -1.28)):
        with pytest.raises(ValueError):
            music_rules.chord_window_columns(fs, ws)
        with pytest.raises(ValueError):
            p2c.piano_roll_to_chords_native(np.zeros((128, 128), dtype=np.uint8), fs=fs, window_size=ws)
    with pytest.raises(ValueError):
        p2c.piano_roll_to_chords_native(np.zeros((128, 128), dtype=np.uint8), profile="temperley")
    with pytest.raises(ValueError):
        p2c.piano_roll_to_chords_native(np.zeros((64, 128), dtype=np.uint8))
    assert p2c.piano_roll_to_chords_native(np.ones((128, 64), dtype=np.uint8))["chords"].shape == (0,)     # shorter than a window


def test_backend_registration(no_backend):
    with pytest.raises(ImportError, match="register_chord_backend"):
        music_rules.get_chords(None)
    for bad in ("Native", "music21", ""):
        with pytest.raises(ValueError):
            music_rules.register_chord_backend(bad)
    with pytest.raises(ValueError):
        music_rules.register_chord_backend("native", profile="temperley")
    assert music_rules._CHORD_BACKEND is None and not music_rules.native_chord_backend()
    music_rules.register_chord_backend("native", profile="aarden")
    assert music_rules.native_chord_backend() and music_rules._CHORD_PROFILE == "aarden"
    music_rules.register_chord_backend(p2c.piano_roll_to_chords_native, workers=0)
    assert not music_rules.native_chord_backend() and music_rules._CHORD_PROFILE == "krumhansl"
    # the host analyser through the existing job path, in this process
    q, degs = ref.progression_roll(4, 1, seed=1)
    outs = music_rules._run_chord_jobs([(music_rules._CHORD_BACKEND, q.astype(np.intc), dict(return_key=True))] * 2)
    chords, keys, coefs = music_rules._pack_chords(outs, True)
    assert chords.tolist() == [degs, degs] and keys == [music_rules.KEY_DICT["e minor"]] * 2 and coefs[0] == coefs[1] > 0.5


def _load_cli():
    spec = importlib.util.spec_from_file_location("sample_rule_cli_chords", os.path.join(PKG, "scripts", "sample_rule.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_cli_native_backend_leaves_a_chord_config_intact(no_backend):
    from guided_diffusion.midi_util import load_config
    cli = _load_cli()
    path = os.path.join(PKG, "scripts", "configs", "cond_table", "all", "scg_classifier_all.yml")
    args = cli.add_sampler_arguments(cli.create_argparser()).parse_args(
        ["--config_path", path, "--chord_backend", "native", "--chord_profile", "aarden"])
    assert args.chord_backend == "native" and args.chord_profile == "aarden"
    before = load_config(path)
    cfg = cli.setup_chord_backend(args, load_config(path))
    assert music_rules.native_chord_backend() and music_rules._CHORD_PROFILE == "aarden" and cli.DROPPED_RULES == []
    assert vars(cfg.target_rules) == vars(before.target_rules) and "chord_progression" in vars(cfg.target_rules)
    assert vars(cfg.scg) == vars(before.scg) and cfg.guidance.cond_fn.rule_names == before.guidance.cond_fn.rule_names
    assert "chord_progression" in cfg.guidance.cond_fn.rule_names
    # the defaults are unchanged: no backend, same error
    music_rules.register_chord_backend(None)
    default = cli.add_sampler_arguments(cli.create_argparser()).parse_args([])
    assert default.chord_backend == "" and default.chord_profile == "krumhansl"
    with pytest.raises(SystemExit):                            # argparse: not one of the profiles
        cli.add_sampler_arguments(cli.create_argparser()).parse_args(["--chord_profile", "temperley"])
    with pytest.raises(RuntimeError, match="skip_chord_rules"):
        cli.setup_chord_backend(SimpleNamespace(chord_backend="", chord_workers=0, skip_chord_rules=False), load_config(path))
    with pytest.raises(ValueError):
        cli.setup_chord_backend(SimpleNamespace(chord_backend="native", chord_profile="temperley", chord_workers=0), load_config(path))


def test_run_metadata_names_the_backend(tmp_path, no_backend):
    import json
    cli = _load_cli()
    args = cli.add_sampler_arguments(cli.create_argparser()).parse_args(["--config_path", "x.yml", "--chord_backend", "native"])
    cli.write_run_metadata(str(tmp_path), args)
    meta = json.load(open(tmp_path / "run_metadata.json"))
    assert meta["chord_backend"] == "native" and meta["chord_profile"] == "krumhansl"
    args = cli.add_sampler_arguments(cli.create_argparser()).parse_args(["--config_path", "x.yml"])
    cli.write_run_metadata(str(tmp_path), args)
    meta = json.load(open(tmp_path / "run_metadata.json"))
    assert meta["chord_backend"] is None and meta["chord_profile"] is None


def test_hand_built_rolls():
    """the rolls of tests/chords_ref.hand_cases: the restatement and the host analyser both give the roots worked out by hand"""
    for name, q, wc, roots in ref.hand_cases():
        want = check_against_ref(q, wc)
        assert want["roots"] == roots, name
