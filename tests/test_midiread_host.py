"""CPU: the host side of the device MIDI reader (docs/rounds/midi_read.md) -- the case set against the host reader, blob packing, the
--midi_reader flag and scripts/midi_to_rolls.py driven by the host reader.  The kernels themselves: tests/test_gpu_midiread.py."""
import importlib.util
import json
import os

import numpy as np
import pytest

import midiread_cases as rc
from conftest import PKG, ROOT


def _script(name):
    spec = importlib.util.spec_from_file_location(name + "_cli", os.path.join(PKG, "scripts", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("name", sorted(rc.ACCEPTED))
def test_the_host_reader_accepts_every_accepting_case(name):
    data, fs = rc.ACCEPTED[name]
    h = rc.host_read(data, fs)
    assert h["roll"].shape[:2] == (3, 128) and h["roll"].shape[2] >= 1 and h["roll"].dtype == np.float32 and len(h["notes"]) >= 1


def test_the_cases_hold_what_their_names_say():
    h = {k: rc.host_read(*v) for k, v in rc.ACCEPTED.items()}
    assert h["overlap_fifo"]["roll"][0].max() == 381 and (h["overlap_fifo"]["roll"][0] > 255).sum() > 0
    c60 = h["overlap_fifo"]["notes"][h["overlap_fifo"]["notes"][:, 1] == 60]
    assert c60[:, 2].tolist() == [100, 90, 110] and (np.diff(c60[:, 4]) > 0).all()    # first in, first out: the first on takes the first off
    assert h["unmatched"]["notes"].shape[0] == 1 and h["drum"]["n_inst"] == 2 and h["drum"]["roll"].shape[2] == 454
    assert h["cc_only_instrument"]["n_inst"] == 2 and h["three_tracks"]["n_inst"] == 7
    assert h["cc_extends"]["roll"].shape[2] == 272                             # controller 7 at tick 1200 sets the length
    assert h["short_note"]["roll"][0, 60].max() == 0 and h["short_note"]["roll"][1, 60, 0] == 127
    assert h["status_zero_and_fx"]["notes"].shape[0] == 2 and h["sysex_and_long_metas"]["notes"].shape[0] == 1
    assert abs(h["tempo_same_tick"]["notes"][2, 3] - 200 * 600000 / (1e6 * 96)) < 1e-12      # 700000 holds from tick 100 on, not 300000
    p = h["pedal_shift_middle"]["roll"][2, 21]
    assert (p[5], p[7]) == (8.0, 120.0) and h["pedal_shift_middle"]["roll"][2, 20].max() == 0
    q = h["pedal_shift_end"]["roll"][2, 21]
    assert q.shape == (100,) and np.nonzero(q)[0].tolist() == [98, 99] and q[98] == 8.0 and q[99] == 8.0    # every jump lands in column 99
    assert h["div_1"]["roll"].shape[2] == 150 and h["fs_12.5"]["roll"].shape[2] * 8 <= h["div_220"]["roll"].shape[2]


@pytest.mark.parametrize("name", sorted(rc.REFUSED))
def test_the_host_reader_raises_on_every_refusal_case(name):
    with pytest.raises(Exception):
        rc.host_read(rc.REFUSED[name][0])


def test_the_host_reader_raises_on_every_truncation_of_a_small_file():
    data = rc.simple_file()
    assert not rc.host_refuses(data)
    assert all(rc.host_refuses(data[:k]) for k in range(len(data)))


def test_packing_pads_the_blob_and_counts_the_tracks(tmp_path):
    from guided_diffusion import midi_util
    a, b, c = rc.ACCEPTED["three_tracks"][0], rc.REFUSED["bad_magic"][0], rc.ACCEPTED["div_1"][0]
    path = tmp_path / "c.mid"
    path.write_bytes(c)
    blob, offsets, tracks = midi_util.pack_midi_files([a, bytearray(b), str(path), b"MThd"])
    assert offsets.dtype == np.int64 and offsets.tolist() == [0, len(a), len(a) + len(b), len(a) + len(b) + len(c), len(a) + len(b) + len(c) + 4]
    assert blob.dtype == np.uint8 and len(blob) % 16 == 0 and offsets[-1] + 16 <= len(blob) < offsets[-1] + 48
    assert blob[:offsets[-1]].tobytes() == a + b + c + b"MThd" and not blob[offsets[-1]:].any()
    assert tracks == 4 + 1                                                      # the refused and the short file claim none
    with pytest.raises(ValueError):
        midi_util.pack_midi_files([])
    with pytest.raises(ValueError):
        midi_util.pack_midi_files([b""])
    assert set(midi_util.MIDI_READ_STATUS) == set(range(10)) and midi_util.MIDI_READERS == ("host", "device")


def test_midi_reader_flag_parses_and_leaves_the_other_flag_sets_alone():
    cli = _script("sample_rule")
    before = set(vars(cli.create_argparser().parse_args([])))
    midi = set(vars(cli.add_midi_arguments(cli.create_argparser()).parse_args([])))
    parser = cli.add_midi_reader_arguments(cli.create_argparser())
    assert parser.parse_args([]).midi_reader == "host"
    assert parser.parse_args(["--midi_reader", "device"]).midi_reader == "device"
    with pytest.raises(SystemExit):
        parser.parse_args(["--midi_reader", "gpu"])
    assert set(vars(cli.create_argparser().parse_args([]))) == before and "midi_reader" not in before
    assert midi == before | {"midi_backend"} and set(vars(parser.parse_args([]))) == before | {"midi_reader"}
    edit = _script("edit")
    assert "midi_reader" not in vars(edit.create_argparser().parse_args([]))


def test_midi_to_rolls_with_the_host_reader_writes_the_reference_names(tmp_path, capsys):
    cli = _script("midi_to_rolls")
    src, out = tmp_path / "src", tmp_path / "out"
    src.mkdir()
    (src / "piece.mid").write_bytes(rc.ACCEPTED["cc_extends"][0])               # 272 columns, silent from column 90 but for the pedal in 204
    (src / "Drum.MIDI").write_bytes(rc.ACCEPTED["drum"][0])
    (src / "loud.mid").write_bytes(rc.ACCEPTED["overlap_fifo"][0])
    (src / "broken.mid").write_bytes(rc.REFUSED["ends_in_message"][0])
    (src / "notes.txt").write_bytes(b"not a MIDI file")
    meta = cli.main(["--midi_dir", str(src), "--outdir", str(out), "--image_size", "64", "--overlap", "True", "--midi_reader", "host"])
    names = sorted(f for f in os.listdir(out) if f.endswith(".npy"))
    roll = rc.host_read(rc.ACCEPTED["cc_extends"][0])["roll"]
    want = [f"piece_{k}.npy" for k in range(5) if roll[:, :, 64 * k:64 * k + 64].max() > 0]
    want += [f"shift_piece_{k}.npy" for k in range(5) if roll[:, :, 32 + 64 * k:96 + 64 * k].size and roll[:, :, 32 + 64 * k:96 + 64 * k].max() > 0]
    assert [n for n in names if "piece" in n] == sorted(want) and "piece_1.npy" not in names and "piece_3.npy" in names
    for n in names:
        a = np.load(out / n)
        assert a.shape == (3, 128, 64) and a.dtype == np.uint8 and a.max() > 0
    assert np.array_equal(np.load(out / "shift_piece_0.npy"), roll[:, :, 32:96].astype(np.uint8))
    loud = rc.host_read(rc.ACCEPTED["overlap_fifo"][0])["roll"]
    assert np.array_equal(np.load(out / "loud_0.npy"), np.minimum(loud[:, :, :64], 255).astype(np.uint8))
    last = np.load(out / "loud_2.npy")                                          # 136 columns: the last piece holds 8 and is zero-padded
    assert np.array_equal(last[:, :, :8], np.minimum(loud[:, :, 128:], 255).astype(np.uint8)) and last[:, :, :8].any() and not last[:, :, 8:].any()
    assert meta == json.load(open(out / "run_metadata.json"))
    assert meta["files"] == 4 and meta["converted"] == 3 and meta["pieces"] == len(names) and meta["midi_reader"] == "host"
    assert [r["file"] for r in meta["refused"]] == ["broken.mid"] and meta["overflow_files"] == ["loud.mid"]
    assert meta["overflow_cells"] == int((loud > 255).sum()) > 0
    assert "broken.mid" in capsys.readouterr().err
    seen = []
    cli.main(["--midi_dir", str(src), "--outdir", str(tmp_path / "o2"), "--batch_size", "3"], reader_fn=lambda paths, fs: seen.append((len(paths), fs)) or
             cli.host_reader(paths, fs))
    assert seen == [(3, 100), (1, 100)] and not any(f.startswith("shift_") for f in os.listdir(tmp_path / "o2"))


def test_the_header_declares_the_reader_entries_and_the_bindings_know_them():
    src = open(os.path.join(ROOT, "include", "rgm.h")).read()
    from rgm import native
    for name in ("rgm_midi_read_workspace", "rgm_midi_read_scan", "rgm_midi_read_rolls"):
        assert name + "(" in src
        assert hasattr(native.lib, name) and getattr(native.lib, name).argtypes is not None
