"""CPU: the host partner of the note statistics (piano_roll_to_chord.piano_roll_note_stats) against the reference's answers in
tests/golden/notes.npz, on every roll of tests/notes_cases.py with first-column onsets both ways, under the comparison rules of
docs/rounds/notes.md (notes_cases.check): integers, transition counts and the NaN pattern exact, histogram and notes per second within
one ulp, mean duration and average IOI within 4 n 2^-53 end_time.  Plus the fixture's own records and the --note_stats flag."""
import importlib.util
import os

import numpy as np
import pytest

import notes_cases as nc
from conftest import PKG, load_golden


@pytest.fixture(scope="module")
def gold():
    return load_golden("notes")


@pytest.fixture(scope="module")
def cases():
    return nc.cases()


def test_fixture_names_seeds_and_the_reference_failure(gold, cases):
    assert list(gold["names"]) == list(cases) and int(gold["seed"][0]) == nc.SEED and int(gold["n_seeds"][0]) == nc.N_SEEDS
    assert gold["ints"].shape == (len(cases), 2, 148) and gold["real"].shape == (len(cases), 2, 16)
    # the fork's transition matrix raises as shipped under the generator's numpy: the fixture says so in the reference's own words
    assert "histogram2d" in str(gold["reference_raises"]) and "normed" in str(gold["reference_raises"])
    # a fixture the reference answers with zeros and NaN everywhere proves nothing: every random roll has notes, the NaN cases are there too
    random = [i for i, n in enumerate(cases) if n.startswith("random.")]
    assert len(random) == 180 and (gold["ints"][random, :, 0] >= 2).all()
    assert np.isnan(gold["real"][:, :, 1]).any() and np.isnan(gold["real"][:, :, 4]).any()
    assert (gold["ints"][:, :, 4:].sum(axis=2) > 0).sum() > 300


def test_host_partner_matches_the_reference_on_every_case(gold, cases):
    from music_rule_guidance.piano_roll_to_chord import piano_roll_note_stats
    worst_ulp = worst_abs = 0.0
    for i, (name, roll) in enumerate(cases.items()):
        for fco in (0, 1):
            ints, real = nc.pack(piano_roll_note_stats(roll, first_column_onsets=bool(fco)))
            u, d = nc.check(ints, real, gold["ints"][i, fco], gold["real"][i, fco], f"{name} first_column_onsets={fco}")
            worst_ulp, worst_abs = max(worst_ulp, u), max(worst_abs, d)
    print(f"host partner: histogram / notes per second off by at most {worst_ulp:.3e} relative, mean duration / IOI by {worst_abs:.3e}")


def test_first_column_onsets_matter_only_with_an_onset_channel(gold, cases):
    names = list(cases)
    for i, name in enumerate(names):
        if not name.endswith(".c3") and ".c3." not in name:
            assert np.array_equal(gold["ints"][i, 0], gold["ints"][i, 1]), name
    i = names.index("column0_no_onset.c3")
    assert gold["ints"][i, 0, 0] == 2 and gold["ints"][i, 1, 0] == 3


def test_host_partner_leaves_its_input_alone_and_takes_a_single_channel(cases):
    from music_rule_guidance.piano_roll_to_chord import piano_roll_note_stats
    roll = cases["random.t64.c3.s0"].copy()
    roll[0, 3, 5] = 30                                   # a background the reference's function would write through
    twin = roll.copy()
    piano_roll_note_stats(roll, first_column_onsets=True)
    assert np.array_equal(roll, twin)
    one = cases["random.t64.c1.s0"]
    a, b = nc.pack(piano_roll_note_stats(one)), nc.pack(piano_roll_note_stats(one[0]))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True)


def test_fs_other_than_100_is_refused_before_anything_runs(cases):
    import torch
    from music_rule_guidance import music_rules
    from music_rule_guidance.piano_roll_to_chord import piano_roll_note_stats
    with pytest.raises(ValueError, match="fs = 100"):
        piano_roll_note_stats(cases["one_note.c1"], fs=12.5)
    with pytest.raises(ValueError, match="fs = 100"):
        music_rules.note_stats(torch.zeros((1, 3, 128, 64), dtype=torch.uint8), fs=12.5)      # a CPU tensor: the check comes first
    with pytest.raises(ValueError):
        piano_roll_note_stats(np.zeros((4, 128, 8), dtype=np.uint8))


def test_rule_entries_are_registered():
    from guided_diffusion.gaussian_diffusion import _CHORD_NEUTRAL_RULES
    from music_rule_guidance import rule_maps
    keys = ["mg_used_pitch", "mg_pitch_range", "mg_avg_ioi", "mg_mean_velocity", "mg_mean_duration", "mg_notes_per_second",
            "mg_pitch_class_hist", "mg_transition"]
    for k in keys:
        assert k in rule_maps.FUNC_DICT and rule_maps.LOSS_DICT[k] is rule_maps.mse_loss_mean and k in _CHORD_NEUTRAL_RULES
    assert "note_density" in rule_maps.FUNC_DICT and "note_density" in _CHORD_NEUTRAL_RULES


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_cli_notes", os.path.join(PKG, "scripts", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_note_stats_flag_parses_in_both_clis_and_stays_out_of_the_reference_flags():
    cli = _load("sample_rule")
    mine = {a.dest for a in cli.create_argparser()._actions}
    assert "note_stats" not in mine                      # tests/test_host_logic.py pins this parser's extra flags as an exact set
    full = cli.add_note_stats_arguments(cli.add_sampler_arguments(cli.create_argparser()))
    assert full.parse_args([]).note_stats is False
    assert full.parse_args(["--note_stats", "True"]).note_stats is True
    edit = _load("edit")
    assert edit.create_argparser().parse_args([]).note_stats is False
    assert edit.create_argparser().parse_args(["--note_stats", "True"]).note_stats is True
