"""CPU: the host side of the device MIDI writer (docs/rounds/midi.md) -- the tick table, the --midi_backend flag, and
save_piano_roll_midi(midi_bytes=...).  The kernels themselves: tests/test_gpu_midi.py."""
import importlib.util
import os

import numpy as np
import pytest

import midi_cases as mc
from conftest import PKG, ROOT, load_golden


def _script(name):
    spec = importlib.util.spec_from_file_location(name + "_cli", os.path.join(PKG, "scripts", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("fs", [50, 100, 200, 220])
def test_tick_table_is_time_to_tick_entry_for_entry(fs):
    from guided_diffusion import midi_util
    from music_rule_guidance.piano_roll_to_chord import SimpleMIDI
    pm = SimpleMIDI()
    for T in (1, 384, 4096):
        tab = midi_util.midi_tick_table(T, fs)
        assert tab.dtype == np.int32 and tab.shape == (T + 1,) and tab.flags.c_contiguous and not tab.flags.writeable
        assert tab.tolist() == [pm.time_to_tick(k / fs) for k in range(T + 1)]
        assert np.diff(tab).min() >= 2 and tab[0] == 0
        assert midi_util.midi_tick_table(T, fs) is tab                          # cached per (T, fs)
    if fs == 100:
        full = midi_util.midi_tick_table(32768, 100)
        assert set(np.diff(full).tolist()) == {4, 5} and int(full[-1]) == 144179 and int(full[-1]) < 1 << 21


def test_tick_table_refuses_what_the_device_path_does_not_serve():
    from guided_diffusion import midi_util
    for fs in (250, 441):
        with pytest.raises(ValueError, match="rise by at least 2"):
            midi_util.midi_tick_table(384, fs)
    with pytest.raises(ValueError, match="2\\^21"):                             # a step of 4400 ticks: column 477 is past 2^21
        midi_util.midi_tick_table(1000, 0.1)
    for T in (0, 32769):
        with pytest.raises(ValueError, match="columns"):
            midi_util.midi_tick_table(T, 100)
    with pytest.raises(ValueError):
        midi_util.midi_tick_table(64, 0)


def test_midi_backend_flag_parses_and_leaves_the_reference_flag_set_alone():
    cli = _script("sample_rule")
    before = set(vars(cli.create_argparser().parse_args([])))
    parser = cli.add_midi_arguments(cli.create_argparser())
    assert parser.parse_args([]).midi_backend == "host"
    assert parser.parse_args(["--midi_backend", "device"]).midi_backend == "device"
    with pytest.raises(SystemExit):
        parser.parse_args(["--midi_backend", "gpu"])
    assert set(vars(cli.create_argparser().parse_args([]))) == before and "midi_backend" not in before
    assert set(vars(parser.parse_args([]))) == before | {"midi_backend"}
    from types import SimpleNamespace
    assert cli.device_midi_bytes(None, SimpleNamespace(midi_backend="host", fs=100)) is None      # the host backend touches nothing


def test_save_piano_roll_midi_writes_given_bytes_under_the_reference_names(tmp_path):
    from guided_diffusion import midi_util
    rolls = np.stack([load_golden("midi_events")["r3.roll"], mc.quirk_roll().repeat(24, axis=2)])
    given = [b"MThd-first", b"MThd-second"]
    twin = rolls.copy()
    midi_util.save_piano_roll_midi(rolls, str(tmp_path / "a"), fs=100, y=np.array([2, 2]), save_ind=5, midi_bytes=given)
    assert np.array_equal(rolls, twin)
    assert sorted(os.listdir(tmp_path / "a")) == ["sample_5_y_2.midi", "sample_5_y_2.npy", "sample_6_y_2.midi", "sample_6_y_2.npy"]
    for i in range(2):
        assert open(tmp_path / "a" / f"sample_{5 + i}_y_2.midi", "rb").read() == given[i]
        assert np.array_equal(np.load(tmp_path / "a" / f"sample_{5 + i}_y_2.npy"), rolls[i])
    midi_util.save_piano_roll_midi(rolls, str(tmp_path / "b"), fs=100, midi_bytes=given)
    assert sorted(os.listdir(tmp_path / "b")) == ["sample_0.midi", "sample_0.npy", "sample_1.midi", "sample_1.npy"]
    with pytest.raises(ValueError, match="1 files for 2 rolls"):
        midi_util.save_piano_roll_midi(rolls, str(tmp_path / "c"), fs=100, midi_bytes=given[:1])
    # without the argument nothing changes: the host extraction, forced onsets included
    midi_util.save_piano_roll_midi(rolls, str(tmp_path / "d"), fs=100)
    for i in range(2):
        assert open(tmp_path / "d" / f"sample_{i}.midi", "rb").read() == mc.host_file(rolls[i], True)[0]


def test_a_registered_writer_still_takes_precedence(tmp_path):
    from guided_diffusion import midi_util
    rolls = load_golden("midi_events")["r3.roll"][None]
    seen = []
    midi_util.register_midi_writer(lambda r, p, fs: seen.append((r.shape, os.path.basename(p), fs)))
    try:
        midi_util.save_piano_roll_midi(rolls, str(tmp_path), fs=50, midi_bytes=[b"unused"])
    finally:
        midi_util.register_midi_writer(None)
    assert seen == [((3, 128, 384), "sample_0.midi", 50)]
    assert sorted(os.listdir(tmp_path)) == ["sample_0.npy"]


def test_the_header_declares_the_entries_and_the_bindings_know_them():
    src = open(os.path.join(ROOT, "include", "rgm.h")).read()
    from rgm import native
    for name in ("rgm_midi_workspace", "rgm_midi_measure", "rgm_midi_emit"):
        assert name + "(" in src
        assert hasattr(native.lib, name) and getattr(native.lib, name).argtypes is not None
