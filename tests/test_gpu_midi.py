"""-m gpu: Standard MIDI Files written on the device (csrc/midi.hip: rgm_midi_measure, rgm_midi_emit) against the host writer --
piano_roll_to_pretty_midi(...).write() on a copy of the same roll -- byte for byte, against the reference's own message stream
(tests/golden/midi_writer.npz) and event lists (midi_events.npz), through the ABI, the Python surface and the three CLIs.  Every comparison
is exact (docs/rounds/midi.md)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import midi_cases as mc
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fp32_behind_every_test():
    """the CLIs set the process-wide GEMM arithmetic (--gemm_precision); the modules behind this one expect the library's start-up value"""
    yield
    from rgm import native as R
    R.set_gemm_precision("fp32")


def _tensor(rolls, layout):
    """(N, C, 128, T) uint8 numpy -> device tensor: layout 0 channel-first, 1 the (N, 128, T, C) tensor of decode_sample_for_midi"""
    t = torch.from_numpy(np.array(rolls, dtype=np.uint8, order="C", copy=True)).cuda()    # a copy: fresh strides for a [None] axis too
    return t.permute(0, 2, 3, 1).contiguous() if layout else t


def _device(rolls, fco, layout=1, fs=100, program=0):
    """-> per sample (file bytes, notes, ccs, messages) of the device path, from ONE pair of launches: the files of rolls_to_midi_bytes'
    own route (midi_events_raw) and the rows of note_events' -- and the roll is checked to be unchanged"""
    from music_rule_guidance import music_rules
    t = _tensor(rolls, layout)
    twin = t.clone()
    ev = music_rules.midi_events_raw(t, fs=fs, first_column_onsets=fco, program=program)
    assert torch.equal(t, twin), "the roll was written to"
    sizes = ev["sizes_host"]
    assert sizes.shape == (rolls.shape[0], 4) and ev["notes"].dtype == torch.int32 and ev["ccs"].dtype == torch.int32
    blob, notes, ccs = ev["bytes"].cpu().numpy().tobytes(), ev["notes"].cpu().numpy(), ev["ccs"].cpu().numpy()
    assert notes.shape == (sizes[:, 0].sum(), 4) and ccs.shape == (sizes[:, 1].sum(), 2) and len(blob) == sizes[:, 3].sum()
    out, n0, c0, b0 = [], 0, 0, 0
    for nn, nc_, nm, nb in sizes:
        out.append((blob[b0:b0 + nb], notes[n0:n0 + nn].astype(np.int64), ccs[c0:c0 + nc_].astype(np.int64), int(nm)))
        n0, c0, b0 = n0 + nn, c0 + nc_, b0 + nb
    return out


def _check(rolls, fco, layout=1, what="", fs=100, program=0):
    """device == host for every sample of the batch: file bytes, note rows, CC rows, message count; returns the device's answers"""
    got = _device(rolls, fco, layout, fs, program)
    for i, (g, roll) in enumerate(zip(got, rolls)):
        want = mc.host_file(roll, first_column_onsets=fco, fs=fs, program=program)
        tag = f"{what} sample {i} of {len(rolls)} layout {layout} first_column_onsets={fco}"
        assert np.array_equal(g[1], want[1]), f"{tag}: notes"
        assert np.array_equal(g[2], want[2]), f"{tag}: ccs"
        assert g[3] == want[3], f"{tag}: {g[3]} messages, host {want[3]}"
        assert g[0] == want[0], f"{tag}: {len(g[0])} bytes, host {len(want[0])}"
    return got


@pytest.mark.parametrize("tag", ["r3", "r2", "r1"])
def test_the_three_reference_rolls(tag, tmp_path):
    """file bytes == the host's file; messages decoded from the device bytes == the reference fork's own stream; notes and CCs == the
    reference's event lists after the sort -- in both memory layouts"""
    from test_host_logic import _smf_messages
    ev, wr = load_golden("midi_events"), load_golden("midi_writer")
    roll = ev[f"{tag}.roll"]
    roll = roll[None] if roll.ndim == 2 else roll
    for layout in (0, 1):
        (data, notes, ccs, n_msgs), = _check(roll[None], False, layout, tag)
        path = str(tmp_path / f"{tag}{layout}.midi")
        with open(path, "wb") as f:
            f.write(data)
        fmt, div, rows = _smf_messages(path)
        assert (fmt, div) == (1, 220) and np.array_equal(rows, wr[f"{tag}.msgs"]) and n_msgs == len(rows)
        gn = ev[f"{tag}.notes"]                          # (velocity, pitch, start, end) in seconds
        want = np.stack([gn[:, 1], gn[:, 0], np.round(gn[:, 2] * 100), np.round(gn[:, 3] * 100)], axis=1).astype(np.int64)
        want = want[np.lexsort((want[:, 2], want[:, 0]))]
        assert np.array_equal(notes, want) and len(notes) > 10
        gc = ev[f"{tag}.ccs"]                            # (number, value, time)
        assert np.array_equal(ccs, np.stack([np.round(gc[:, 2] * 100), gc[:, 1]], axis=1).astype(np.int64).reshape(-1, 2))
        assert (gc[:, 0] == 64).all()


def test_the_quirk_roll():
    """one case per quirk of piano_roll_to_pretty_midi at T = 16, with and without the forced onsets of column 0; the rows named here say
    that the roll really holds each case"""
    roll = mc.quirk_roll()
    for fco in (False, True):
        for layout in (0, 1):
            (data, notes, ccs, _), = _check(roll[None], fco, layout, "quirks")
        rows = {tuple(r) for r in notes.tolist()}
        assert not [r for r in rows if r[0] in (30, 45, 55, 60, 61)]                            # == background, no onset, onset 63, column 0 below it
        assert {(31, 11, 2, 5), (40, 50, 6, 6), (41, 51, 2, 6), (41, 51, 6, 6), (42, 52, 2, 6), (42, 53, 7, 9), (50, 70, 10, 16),
                (51, 71, 10, 13), (51, 71, 13, 16), (52, 72, 15, 16), (56, 81, 4, 7)} <= rows
        assert ((62, 91, 0, 3) in rows) == fco and len(rows) == 11 + fco
        assert ccs.tolist() == [[0, 0], [1, 0], [2, 0], [3, 16], [4, 63], [5, 64], [6, 112], [7, 127], [8, 112], [9, 127], [11, 0], [13, 0]]


T_CASES = (1, 2, 63, 64, 65, 129, 384, 1000)


@pytest.mark.parametrize("T", T_CASES)
def test_random_rolls(T):
    """densities from the empty roll to every cell set, runs across the 64-column word boundaries, C = 1 / 2 / 3 and N = 1 / 3 / 17 in turn"""
    k = T_CASES.index(T)
    for C in (1, 2, 3):
        N = (1, 3, 17)[(k + C) % 3]
        dens = [(0.0, 0.02, 0.3, 0.08, 0.6)[(i + k) % 5] for i in range(N)]
        if T <= 129:
            dens[0] = 1.0                               # every cell set, an onset everywhere
            if N > 1:
                dens[1] = 0.0                           # the empty roll
        rolls = np.stack([mc.random_roll(1000 * T + 10 * C + i, C, T, d) for i, d in enumerate(dens)])
        fco = bool((k + C) % 2)
        got = _check(rolls, fco, layout=(k + C) % 2, what=f"T={T} C={C} N={N}")
        if N > 1 and T <= 129:
            assert got[1][0][-4:] == bytes([1, 0xFF, 0x2F, 0]) and len(got[1][0]) == 56 and got[1][3] == 5


def test_every_cell_set_at_eight_columns():
    """an onset everywhere: T = 8 gives 856 notes and 1725 messages on the host"""
    roll = np.zeros((3, 128, 8), dtype=np.uint8)
    roll[0, 21:], roll[1], roll[2] = 100, 127, 100
    (data, notes, ccs, n_msgs), = _check(roll[None], True, 1, "full")
    assert len(notes) == 856 and n_msgs == 1725


def test_long_deltas_and_long_tracks():
    """one late note at T = 4096: deltas of two (tick 440) and three (tick 17600) VLQ bytes; a dense T = 384 roll whose track is longer
    than 65535 bytes"""
    late = np.zeros((2, 1, 128, 4096), dtype=np.uint8)
    late[0, 0, 60, 100:110], late[1, 0, 60, 4000:4010] = 90, 90
    got = _check(late, False, 0, "late")
    assert got[0][0][52:55] == bytes([0x83, 0x38, 0x90]) and got[1][0][52:56] == bytes([0x81, 0x89, 0x40, 0x90])
    dense = np.zeros((1, 3, 128, 384), dtype=np.uint8)
    dense[0, 0, 40:80], dense[0, 1, 40:80] = 99, 127
    (data, notes, _, _), = _check(dense, True, 1, "dense")
    assert int.from_bytes(data[45:49], "big") > 65535 and len(notes) == 40 * 384


def test_launches_repeat_and_a_sample_does_not_depend_on_its_batch():
    rolls = np.stack([mc.random_roll(77 + i, 3, 384, 0.3) for i in range(17)])
    first = _device(rolls, True)
    assert min(len(f[1]) for f in first) > 10
    for _ in range(19):
        again = _device(rolls, True)
        for a, b in zip(first, again):
            assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    alone = _device(rolls[11:12], True)
    five = _device(rolls[9:14], True)
    assert alone[0][0] == first[11][0] == five[2][0]                            # the file, alone / row 2 of 5 / row 11 of 17
    for j in (1, 2):
        assert np.array_equal(alone[0][j], first[11][j]) and np.array_equal(five[2][j], first[11][j])


def test_python_surface():
    """note_events' dict, rolls_to_midi_bytes' list, program numbers, other sampling rates, and the refusal of an fs beyond 220"""
    from guided_diffusion import midi_util
    from music_rule_guidance import music_rules
    rolls = np.stack([mc.random_roll(5 + i, 3, 129, 0.3) for i in range(3)])
    t = _tensor(rolls, 1)
    ev = music_rules.note_events(t, first_column_onsets=True)
    assert set(ev) == {"n_notes", "n_ccs", "notes", "ccs", "note_offsets", "cc_offsets"} and all(v.is_cuda for v in ev.values())
    files = midi_util.rolls_to_midi_bytes(t, program=5)
    assert isinstance(files, list) and len(files) == 3 and all(isinstance(f, bytes) for f in files)
    for i in range(3):
        want = mc.host_file(rolls[i], True, program=5)
        assert files[i] == want[0] and files[i][49:52] == bytes([0, 0xC0, 5])
        lo, n = int(ev["note_offsets"][i]), int(ev["n_notes"][i])
        assert np.array_equal(ev["notes"][lo:lo + n].cpu().numpy(), want[1])
        lo, n = int(ev["cc_offsets"][i]), int(ev["n_ccs"][i])
        assert np.array_equal(ev["ccs"][lo:lo + n].cpu().numpy(), want[2])
    for fs in (50, 200, 220):
        _check(rolls[:1], True, 1, f"fs={fs}", fs=fs)
    for fs in (250, 441):
        with pytest.raises(ValueError, match="fs"):
            midi_util.rolls_to_midi_bytes(t, fs=fs)
    with pytest.raises(ValueError):
        midi_util.rolls_to_midi_bytes(torch.zeros((1, 4, 128, 64), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        midi_util.rolls_to_midi_bytes(torch.zeros((1, 3, 128, 64), dtype=torch.float32, device="cuda"))


def test_arguments_are_checked_before_any_launch():
    """T = 0, T = 32769, C = 4, N = 0, NULL pointers, a short workspace, a tick table that does not rise by 2: a status, and nothing written"""
    from guided_diffusion import midi_util
    from rgm import native as R
    L = R.lib
    assert L.rgm_midi_workspace(1, 32768) > 0 and L.rgm_midi_workspace(17, 1000) > 0
    assert L.rgm_midi_workspace(1, 32769) == 0 and L.rgm_midi_workspace(1, 0) == 0 and L.rgm_midi_workspace(0, 64) == 0
    T = 64
    roll = torch.zeros((1, 3, 128, T), dtype=torch.uint8, device="cuda")
    roll[0, 0, 21:], roll[0, 1, :, 0] = 90, 127                                 # 107 notes, no pedal
    counts = torch.full((1, 4), -7, dtype=torch.int64, device="cuda")
    nbytes = L.rgm_midi_workspace(1, T)
    ws = torch.full(((nbytes + 7) // 8,), -7, dtype=torch.int64, device="cuda")
    ticks = midi_util.midi_tick_table(T, 100)
    tp = ctypes.c_void_p(ticks.ctypes.data)
    st = (3 * 128 * T, 128 * T, T, 1)
    s = R.current_stream()

    def measure(roll_p=R.ptr(roll), N=1, C=3, T_=T, ticks_p=tp, counts_p=R.ptr(counts), ws_p=R.ptr(ws), ws_b=ws.numel() * 8):
        return L.rgm_midi_measure(roll_p, *st, N, C, T_, 1, ticks_p, counts_p, ws_p, ws_b, s)
    bad = np.array(ticks)
    bad[10] = bad[9] + 1
    long_ = np.array(ticks)
    long_[-1] = 1 << 21
    for name, status, kw in (("T = 0", -1, dict(T_=0)), ("T = 32769", -1, dict(T_=32769)), ("C = 4", -1, dict(C=4)), ("C = 0", -1, dict(C=0)),
                             ("N = 0", -1, dict(N=0)), ("roll", -1, dict(roll_p=None)), ("ticks", -1, dict(ticks_p=None)),
                             ("counts", -1, dict(counts_p=None)), ("ws", -3, dict(ws_p=None)), ("short ws", -3, dict(ws_b=nbytes - 8)),
                             ("table step", -1, dict(ticks_p=ctypes.c_void_p(bad.ctypes.data))),
                             ("table end", -1, dict(ticks_p=ctypes.c_void_p(long_.ctypes.data)))):
        assert measure(**kw) == status, name
        assert L.rgm_last_error(), name
    assert measure(ticks_p=ctypes.c_void_p(bad.ctypes.data)) == -1 and b"tick table rises by 1 from column 9 to 10" in L.rgm_last_error()
    torch.cuda.synchronize()
    assert (counts == -7).all() and (ws == -7).all()
    assert measure() == 0
    sizes = counts.cpu().numpy()
    assert sizes[0, 0] == 128 - 21 and (ws != -7).any()
    off = torch.zeros(3, dtype=torch.int64, device="cuda")
    notes = torch.full((int(sizes[0, 0]), 4), -7, dtype=torch.int32, device="cuda")
    blob = torch.full((int(sizes[0, 3]),), 7, dtype=torch.uint8, device="cuda")

    def emit(N=1, T_=T, program=0, off_p=R.ptr(off), notes_p=R.ptr(notes), notes_cap=notes.shape[0], blob_p=R.ptr(blob), blob_cap=blob.numel(),
             ws_p=R.ptr(ws), ws_b=ws.numel() * 8):
        return L.rgm_midi_emit(N, T_, program, off_p, off_p, off_p, notes_p, notes_cap, None, 0, blob_p, blob_cap, ws_p, ws_b, s)
    for name, status, kw in (("T = 0", -1, dict(T_=0)), ("T = 32769", -1, dict(T_=32769)), ("N = 0", -1, dict(N=0)), ("offsets", -1, dict(off_p=None)),
                             ("bytes", -1, dict(blob_p=None)), ("notes", -1, dict(notes_p=None)), ("program", -1, dict(program=128)),
                             ("ws", -3, dict(ws_p=None)), ("short ws", -3, dict(ws_b=nbytes - 8))):
        assert emit(**kw) == status, name
    torch.cuda.synchronize()
    assert (notes == -7).all() and (blob == 7).all()
    assert emit(notes_cap=notes.shape[0] - 1, blob_cap=blob.numel() - 1) == 0           # arrays one short: the sample is left out whole
    torch.cuda.synchronize()
    assert (notes == -7).all() and (blob == 7).all()
    assert emit() == 0
    torch.cuda.synchronize()
    assert bytes(blob.cpu().numpy().tobytes()) == mc.host_file(roll[0].cpu().numpy(), True)[0] and (notes != -7).all()
    with pytest.raises(ValueError):
        midi_util.rolls_to_midi_bytes(torch.zeros((0, 3, 128, 64), dtype=torch.uint8, device="cuda"))


# ------------------------------------------------------------------------------------------------ the three CLIs, synthetic weights
def _script(name):
    import importlib.util
    from conftest import PKG
    spec = importlib.util.spec_from_file_location(name + "_cli", os.path.join(PKG, "scripts", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _files_are_the_host_writers(out_dir, stems):
    """file names as ever; every .midi is byte for byte the host writer's file of the .npy beside it (first-column onsets as
    save_piano_roll_midi applies them)"""
    names = sorted(f for f in os.listdir(out_dir) if f.startswith("sample_"))
    assert names == sorted(s + ext for s in stems for ext in (".midi", ".npy")), names
    for s in stems:
        roll = np.load(os.path.join(out_dir, s + ".npy"))
        assert roll.shape[:2] == (3, 128) and roll.dtype == np.uint8
        with open(os.path.join(out_dir, s + ".midi"), "rb") as f:
            assert f.read() == mc.host_file(roll, True)[0], s


def test_sample_rule_cli_writes_the_same_files_from_the_device(tmp_path, monkeypatch):
    from test_gpu_cli import CFG, COMMON
    monkeypatch.chdir(tmp_path)
    cli = _script("sample_rule")
    cfg = os.path.join(CFG, "cond_table/single/scg/nd.yml")
    argv = ["--config_path", cfg, "--batch_size", "2", "--num_samples", "2", "--diffusion_steps", "24", "--sampler", "dpmpp", "--dpmpp_steps", "2"] + COMMON
    out_dir = os.path.join("loggings", cli.output_dir_for(cfg, 1))
    res = cli.main(argv + ["--midi_backend", "device"])
    assert len(res) == 2 and json.load(open(os.path.join(out_dir, "run_metadata.json")))["midi_backend"] == "device"
    _files_are_the_host_writers(out_dir, ["sample_0_y_1", "sample_1_y_1"])
    device = [open(os.path.join(out_dir, f"sample_{i}_y_1.midi"), "rb").read() for i in range(2)]
    assert min(len(d) for d in device) > 56                                    # not the empty file
    cli.main(argv)                                                              # the default run: the host loop, the same files as ever
    assert json.load(open(os.path.join(out_dir, "run_metadata.json")))["midi_backend"] == "host"
    _files_are_the_host_writers(out_dir, ["sample_0_y_1", "sample_1_y_1"])
    assert device == [open(os.path.join(out_dir, f"sample_{i}_y_1.midi"), "rb").read() for i in range(2)]    # same seed, same rolls, same bytes


def test_edit_cli_writes_the_generated_rolls_from_the_device(tmp_path, monkeypatch):
    from test_gpu_cli import CFG, COMMON
    monkeypatch.chdir(tmp_path)
    cli = _script("edit")
    cfg = os.path.join(str(tmp_path), "configs", "edit", "nd_short.yml")
    os.makedirs(os.path.dirname(cfg))
    open(cfg, "w").write(open(os.path.join(CFG, "edit", "nd_scg_given_target.yml")).read().replace("noise_level: 500", "noise_level: 3"))
    res, sample = cli.main(["--config_path", cfg, "--batch_size", "2", "--num_samples", "2", "--diffusion_steps", "24",
                            "--allow_synthetic_source", "True", "--midi_backend", "device"] + COMMON)
    out_dir = os.path.join("loggings", "edit_demo", "edit", "nd_short_cls_1_synthsrc")
    assert len(res) == 2 and json.load(open(os.path.join(out_dir, "run_metadata.json")))["midi_backend"] == "device"
    _files_are_the_host_writers(out_dir, ["sample_0_y_1", "sample_1_y_1"])
    _files_are_the_host_writers(os.path.join(out_dir, "gt"), ["sample_0_y_1"])  # the source roll: the host path


def test_cfg_sample_cli_writes_the_same_files_from_the_device(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("OPENAI_LOGDIR", str(tmp_path / "log"))
    cli = _script("cfg_sample")
    argv = ["--model", "DiTRotary_B_8", "--image_size", "128", "16", "--in_channels", "4", "--scale_factor", "1.2465", "--num_classes", "3",
            "--class_label", "2", "--synthetic_weights", "True", "--progress", "False", "--batch_size", "2", "--num_samples", "3",
            "--diffusion_steps", "24", "--class_cond", "False", "--use_dpmpp", "True", "--dpmpp_steps", "2"]
    arr = cli.main(argv + ["--midi_backend", "device", "--save_name", "_dev"])
    assert arr.shape == (3, 3, 128, 1024)                                      # two rounds of two, the first three kept
    out_dir, = [dp for dp, _, fs in os.walk(str(tmp_path)) if "run_metadata.json" in fs]
    meta = json.load(open(os.path.join(out_dir, "run_metadata.json")))
    assert meta["midi_backend"] == "device" and meta["sampler"]["name"] == "dpmpp" and out_dir.endswith("gen_cls_2_dev")
    _files_are_the_host_writers(out_dir, ["sample_0", "sample_1", "sample_2"])
    cli.main(argv + ["--save_name", "_host"])
    host_dir, = [dp for dp, _, fs in os.walk(str(tmp_path)) if "run_metadata.json" in fs and dp.endswith("_host")]
    assert "midi_backend" not in json.load(open(os.path.join(host_dir, "run_metadata.json")))
    _files_are_the_host_writers(host_dir, ["sample_0", "sample_1", "sample_2"])
    for i in range(3):
        assert open(os.path.join(out_dir, f"sample_{i}.midi"), "rb").read() == open(os.path.join(host_dir, f"sample_{i}.midi"), "rb").read()
