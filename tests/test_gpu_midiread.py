"""-m gpu: Standard MIDI Files read on the device (csrc/midi_read.hip: rgm_midi_read_scan, rgm_midi_read_rolls) against the host reader --
SimpleMIDI._read followed by midi_to_full_piano_roll on the same bytes -- events, seconds as float64 ==, rolls in both output types,
through the ABI, the Python surface and the two CLIs.  Every comparison is exact (docs/rounds/midi_read.md)."""
import json
import os

import numpy as np
import pytest
import torch

import midi_cases as mc
import midiread_cases as rc
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fp32_behind_every_test():
    """the CLIs set the process-wide GEMM arithmetic (--gemm_precision); the modules behind this one expect the library's start-up value"""
    yield
    from rgm import native as R
    R.set_gemm_precision("fp32")


_HOST = {}


def _host(data, fs):
    """the host reader's answer for these bytes, computed once per (bytes, fs); None where the host raises"""
    key = (data, fs)
    if key not in _HOST:
        try:
            _HOST[key] = rc.host_read(data, fs)
        except Exception:
            _HOST[key] = None
    return _HOST[key]


def _device_events(files, fs):
    from guided_diffusion import midi_util
    ev = midi_util.midi_files_to_events(files, fs=fs)
    no, co = ev["note_offsets"].cpu().numpy(), ev["cc_offsets"].cpu().numpy()
    notes, nt = ev["notes"].cpu().numpy(), ev["note_times"].cpu().numpy()
    ccs, ct = ev["ccs"].cpu().numpy(), ev["cc_times"].cpu().numpy()
    assert notes.shape == (no[-1], 6) and nt.shape == (no[-1], 2) and nt.dtype == np.float64 and ccs.shape == (co[-1], 4) and ct.shape == (co[-1],)
    out = []
    for i in range(len(files)):
        n, t = notes[no[i]:no[i + 1]], nt[no[i]:no[i + 1]]
        c, u = ccs[co[i]:co[i + 1]], ct[co[i]:co[i + 1]]
        assert (n[:, 5] >= n[:, 4]).all() and (n[:, 1] >= 0).all() and (n[:, 1] < 16).all()
        out.append({"notes": rc.sort_notes(np.column_stack([n[:, 0], n[:, 2], n[:, 3], t[:, 0], t[:, 1]]).astype(np.float64).reshape(-1, 5)),
                    "ccs": np.column_stack([c[:, 0], c[:, 1], c[:, 2], u]).astype(np.float64).reshape(-1, 4)})
    return out, ev["status"].cpu().numpy(), ev["counts"].cpu().numpy(), ev["columns"].cpu().numpy()


def _check(files, fs=100, what="", statuses=None):
    """device == host for every file of the batch: acceptance, counts, note rows, control changes, columns, the float32 and the uint8 roll"""
    from guided_diffusion import midi_util
    files = list(files)
    hosts = [_host(f, fs) for f in files]
    events, status, counts, columns = _device_events(files, fs)
    rf = midi_util.midi_files_to_rolls(files, fs=fs, dtype=torch.float32, strict=False)
    ru = midi_util.midi_files_to_rolls(files, fs=fs, dtype=torch.uint8, strict=False)
    T = max([h["roll"].shape[2] for h in hosts if h is not None] + [1])
    assert rf["roll"].shape == (len(files), 3, 128, T) and rf["roll"].dtype == torch.float32 and ru["roll"].dtype == torch.uint8
    assert np.array_equal(rf["status"].cpu().numpy(), status) and np.array_equal(ru["columns"].cpu().numpy(), columns)
    rolls_f, rolls_u, over = rf["roll"].cpu().numpy(), ru["roll"].cpu().numpy(), ru["overflow"].cpu().numpy()
    assert not rf["overflow"].any()
    for i, h in enumerate(hosts):
        tag = f"{what} file {i} of {len(files)} fs {fs}"
        if h is None:
            assert status[i] != 0 and not counts[i].any() and columns[i] == 0, f"{tag}: the host raises, status {status[i]}"
            assert len(events[i]["notes"]) == 0 and len(events[i]["ccs"]) == 0 and not rolls_f[i].any() and not rolls_u[i].any() and over[i] == 0, tag
            if statuses is not None:
                assert status[i] == statuses[i], f"{tag}: status {status[i]}, expected {statuses[i]}"
            continue
        assert status[i] == 0, f"{tag}: status {status[i]}"
        assert counts[i, 0] == len(h["notes"]) and counts[i, 1] == len(h["ccs"]) and counts[i, 3] == h["n_inst"] and counts[i, 2] >= 1, f"{tag}: {counts[i]}"
        assert np.array_equal(events[i]["notes"], h["notes"]), f"{tag}: notes"
        assert np.array_equal(events[i]["ccs"], h["ccs"]), f"{tag}: control changes"
        t = h["roll"].shape[2]
        assert columns[i] == t, f"{tag}: {columns[i]} columns, host {t}"
        assert np.array_equal(rolls_f[i, :, :, :t], h["roll"]) and not rolls_f[i, :, :, t:].any(), f"{tag}: float32 roll"
        assert np.array_equal(rolls_u[i, :, :, :t], np.minimum(h["roll"], 255).astype(np.uint8)) and not rolls_u[i, :, :, t:].any(), f"{tag}: uint8 roll"
        assert over[i] == (h["roll"] > 255).sum(), f"{tag}: overflow {over[i]}"
    return status, rolls_f


# ------------------------------------------------------------------------------------------------ round trips through both writers
def _written(rolls, writer):
    from guided_diffusion import midi_util
    if writer == "host":
        return [mc.host_file(r, True)[0] for r in rolls]
    return midi_util.rolls_to_midi_bytes(torch.from_numpy(np.array(rolls, dtype=np.uint8, order="C", copy=True)).cuda())   # a copy: fresh strides


@pytest.mark.parametrize("tag", ["r3", "r2", "r1"])
def test_the_reference_rolls_round_trip(tag):
    roll = load_golden("midi_events")[f"{tag}.roll"]
    roll = roll[None] if roll.ndim == 2 else roll
    host, dev = _written(roll[None], "host"), _written(roll[None], "device")
    assert host == dev
    status, _ = _check(host + dev, what=tag)
    assert not status.any()


@pytest.mark.parametrize("T,C,N,density", [(1, 1, 1, 0.5), (2, 2, 3, 0.5), (63, 3, 17, 0.2), (64, 1, 3, 1.0), (65, 2, 1, 0.3), (384, 3, 3, 0.2),
                                           (1000, 3, 1, 0.1), (64, 3, 3, 0.0)])
def test_random_rolls_round_trip(T, C, N, density):
    rolls = np.stack([mc.random_roll(100 * T + 10 * C + n, C, T, density) for n in range(N)])
    files = _written(rolls, "device")
    assert files == _written(rolls, "host")
    status, _ = _check(files, what=f"T {T} C {C} N {N}")
    assert (status != 0).all() if density == 0 else True                        # the empty roll's file holds no note: refused by both


# ------------------------------------------------------------------------------------------------ the hand-assembled cases
def test_the_named_cases_in_one_batch_per_fs():
    for fs in (100, 12.5, 220):
        names = sorted(k for k, v in rc.ACCEPTED.items() if v[1] == fs)
        status, _ = _check([rc.ACCEPTED[k][0] for k in names], fs=fs, what=f"cases {names}")
        assert not status.any(), dict(zip(names, status))


@pytest.mark.parametrize("name", sorted(rc.ACCEPTED))
def test_a_named_case_alone(name):
    data, fs = rc.ACCEPTED[name]
    status, _ = _check([data], fs=fs, what=name)
    assert status[0] == 0


def test_the_overflow_case_saturates_and_counts():
    from guided_diffusion import midi_util
    data = rc.ACCEPTED["overlap_fifo"][0]
    h = _host(data, 100)
    r = midi_util.midi_files_to_rolls([data], dtype=torch.uint8)
    assert int(r["overflow"][0]) == int((h["roll"] > 255).sum()) > 0 and int(r["roll"][0, 0].max()) == 255
    f = midi_util.midi_files_to_rolls([data], dtype=torch.float32)
    assert float(f["roll"][0, 0].max()) == 381.0 and int(f["overflow"][0]) == 0


# ------------------------------------------------------------------------------------------------ alignment
def test_a_text_meta_of_every_length_moves_every_message_over_every_boundary():
    files = [rc.simple_file(text=L) for L in range(0, 301)] + [rc.simple_file(pad=3)]
    want = _host(rc.simple_file(), 100)
    for f in files[::37]:
        assert np.array_equal(_host(f, 100)["roll"], want["roll"])              # the host reads the same music from every one of them
    for f in files:
        _HOST[(f, 100)] = want
    status, rolls = _check(files, what="text metas")
    assert not status.any() and all(np.array_equal(rolls[i], rolls[0]) for i in range(len(files)))


def test_files_at_odd_offsets_and_a_long_track():
    from guided_diffusion import midi_util
    odd = [rc.ACCEPTED["div_1"][0] + b"\x00" * k for k in (1, 2, 0)]             # trailing bytes behind the last chunk: ignored, and they shift what follows
    status, _ = _check(odd + [rc.ACCEPTED["running_status"][0], rc.ACCEPTED["three_tracks"][0]], what="odd offsets")
    assert not status.any()
    rng = np.random.default_rng(5)
    pairs = []
    for i in range(22000):                                                      # ~200 KB: 22000 notes over 3 channels, overlapping, with pedal events
        t = int(i * 37 + rng.integers(0, 30))
        pairs += rc.note(int(rng.integers(0, 3)), int(rng.integers(21, 109)), int(rng.integers(1, 128)), t, int(rng.integers(1, 900)))
        if i % 9 == 0:
            pairs.append((t, bytes([0xB0 | int(rng.integers(0, 3)), 64, int(rng.integers(0, 128))])))
    big = rc.smf(rc.track(rc.tempo(0, 90000), rc.tempo(400000, 60000), rc.END), rc.track(*rc.timed(pairs), rc.END), div=480)
    assert 150000 < len(big) < 300000
    h = _host(big, 100)
    ev, status, counts, columns = _device_events([big], 100)
    assert status[0] == 0 and counts[0, 0] == len(h["notes"]) == 22000 and columns[0] == h["roll"].shape[2] > 10000
    assert np.array_equal(ev[0]["notes"], h["notes"]) and np.array_equal(ev[0]["ccs"], h["ccs"])
    for start, T in ((0, 512), (h["roll"].shape[2] - 300, 512), (7001, 255)):
        r = midi_util.midi_files_to_rolls([big], columns=T, start_column=start, dtype=torch.float32)["roll"][0].cpu().numpy()
        want = np.zeros((3, 128, T), dtype=np.float32)
        piece = h["roll"][:, :, start:start + T]
        want[:, :, :piece.shape[2]] = piece
        assert np.array_equal(r, want), (start, T)


def test_the_pedal_walk_crosses_its_state_tile():
    """more than 32768 columns: pedal events on both sides of the boundary of the walk's state, a 0 -> 127 jump in columns 32766 and 32767 whose
    shifted value lands in the next tile, and a second instrument that comes back to those columns later in the walk"""
    from guided_diffusion import midi_util
    cc = lambda ch, col, v, sub=0: (col * 4 + sub, bytes([0xB0 | ch, 64, v]))          # 4 ticks per column at 400 ticks per second
    one = rc.note(0, 60, 64, 0, 4 * 33000) + [cc(0, 10, 0), cc(0, 10, 127, 1), cc(0, 32766, 0), cc(0, 32766, 127, 1), cc(0, 32767, 5), cc(0, 32767, 120, 1),
                                            cc(0, 32769, 60), cc(0, 32999, 0), cc(0, 32999, 127, 1)]
    two = [cc(1, 32765, 127), cc(1, 32767, 127), cc(1, 32768, 0), cc(1, 32769, 127), cc(1, 32770, 1)]
    data = rc.smf(rc.track(rc.tempo(0, 500000), rc.END), rc.track(*rc.timed(one), rc.END), rc.track(*rc.timed(two), rc.END), div=200)
    h = _host(data, 100)["roll"]
    assert h.shape[2] == 33000 and np.count_nonzero(h[2, 21, 32760:32780]) >= 5
    for start, T in ((32700, 300), (32767, 4), (0, 64), (32768, 232)):
        r = midi_util.midi_files_to_rolls([data], columns=T, start_column=start, dtype=torch.uint8)["roll"][0].cpu().numpy()
        assert np.array_equal(r, h[:, :, start:start + T].astype(np.uint8)), (start, T)


# ------------------------------------------------------------------------------------------------ windows
def test_windows():
    from guided_diffusion import midi_util
    files = [rc.ACCEPTED[k][0] for k in ("three_tracks", "pedal_shift_end", "drum", "pedal_shift_middle")]
    hosts = [_host(f, 100)["roll"] for f in files]
    longest = max(h.shape[2] for h in hosts)
    for start, T, dtype in ((0, None, torch.float32), (0, 64, torch.uint8), (3, 64, torch.float32), (97, 5, torch.float32), (98, 1, torch.uint8),
                            (100, 700, torch.float32), (1000, 3, torch.uint8), (453, None, torch.float32)):
        r = midi_util.midi_files_to_rolls(files, columns=T, start_column=start, dtype=dtype)
        got = r["roll"].cpu().numpy()
        width = T if T is not None else max(1, longest - start)
        assert got.shape == (4, 3, 128, width) and r["columns"].cpu().tolist() == [h.shape[2] for h in hosts]
        for i, h in enumerate(hosts):
            want = np.zeros((3, 128, width), dtype=np.float32)
            piece = h[:, :, start:start + width]
            want[:, :, :piece.shape[2]] = piece
            assert np.array_equal(got[i], want.astype(got.dtype)), (start, T, i)


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_case_has_its_status_and_leaves_its_neighbours_alone():
    from guided_diffusion import midi_util
    good = [rc.ACCEPTED["three_tracks"][0], rc.ACCEPTED["tempo_thousand"][0]]
    names = sorted(rc.REFUSED)
    files, want = [good[0]], [0]
    for k in names:                                                             # every refused file between two good ones
        files += [rc.REFUSED[k][0], good[len(files) % 4 == 1]]
        want += [rc.REFUSED[k][1], 0]
    status, _ = _check(files, what="refusals", statuses=want)
    assert status.tolist() == want
    with pytest.raises(ValueError, match="file 1.*status"):
        midi_util.midi_files_to_rolls(files[:3])
    assert midi_util.midi_files_to_rolls(files[:3], strict=False)["status"].tolist() == want[:3]


def test_every_truncation_of_a_small_file_is_refused():
    data = rc.simple_file()
    files = [data[:k] for k in range(1, len(data))] + [data]
    for f in files[:-1]:
        _HOST[(f, 100)] = None                                                  # the host raises on every one: tests/test_midiread_host.py
    status, _ = _check(files, what="truncations")
    assert (status[:-1] != 0).all() and status[-1] == 0 and set(status[:-1].tolist()) <= {rc.NOT_SMF, rc.BAD_TRACK}
    body = rc.smf(rc.TEMPO_TRACK, rc.track(rc.ev(0, 0x90, 60, 64), rc.ev(220, 0x80, 60, 0), rc.meta(0, 0x01, b"abc"), rc.END))
    at = body.index(b"MTrk", 20)                                                # the second chunk; its length follows every cut, so the track ends with the file
    cut = [body[:at + 4] + (len(body) - at - 8 - k).to_bytes(4, "big") + body[at + 8:len(body) - k] for k in range(1, 12)]
    status, _ = _check(cut, what="cut inside a message")                       # the host skips past the end of a cut payload and accepts: so does the device
    refused = [rc.host_refuses(c) for c in cut]
    assert sum(refused) >= 6 and [st == rc.TRUNCATED for st in status.tolist()] == refused


# ------------------------------------------------------------------------------------------------ robustness
def test_launches_repeat_and_a_file_does_not_depend_on_its_batch():
    from guided_diffusion import midi_util
    names = sorted(rc.ACCEPTED)
    pool = [rc.ACCEPTED[k][0] for k in names if rc.ACCEPTED[k][1] == 100]
    mine = rc.ACCEPTED["three_tracks"][0]
    alone = midi_util.midi_files_to_rolls([mine], dtype=torch.float32)["roll"][0]
    ev_alone = midi_util.midi_files_to_events([mine])
    first = None
    for N, at in ((17, 11), (5, 2)):
        files = (pool * 2)[:N]
        files[at] = mine
        for _ in range(10):
            r = midi_util.midi_files_to_rolls(files, dtype=torch.float32)
            ev = midi_util.midi_files_to_events(files)
            key = (N, r["roll"], ev["notes"], ev["note_times"], ev["ccs"], ev["cc_times"])
            if first is None or first[0] != N:
                first = key
            assert all(torch.equal(a, b) for a, b in zip(key[1:], first[1:]))
            t = alone.shape[2]
            assert torch.equal(r["roll"][at, :, :, :t], alone) and not r["roll"][at, :, :, t:].any()
            a, b = int(ev["note_offsets"][at]), int(ev["note_offsets"][at + 1])
            assert torch.equal(ev["notes"][a:b], ev_alone["notes"]) and torch.equal(ev["note_times"][a:b], ev_alone["note_times"])
            a, b = int(ev["cc_offsets"][at]), int(ev["cc_offsets"][at + 1])
            assert torch.equal(ev["ccs"][a:b], ev_alone["ccs"]) and torch.equal(ev["cc_times"][a:b], ev_alone["cc_times"])


def test_the_abi_refuses_bad_arguments_and_writes_nothing():
    from guided_diffusion import midi_util
    from rgm import native as R
    L, s = R.lib, R.current_stream()
    files = [rc.ACCEPTED["three_tracks"][0], rc.ACCEPTED["overlap_fifo"][0]]
    blob_h, off_h, tracks = midi_util.pack_midi_files(files)
    N, total = 2, int(off_h[-1])
    blob, off = torch.from_numpy(blob_h).cuda(), torch.from_numpy(off_h).cuda()
    twin = blob.clone()
    nbytes = L.rgm_midi_read_workspace(N, total, tracks)
    assert nbytes > 0 and nbytes % 16 == 0 and nbytes == L.rgm_midi_read_workspace(N, total, tracks)
    for bad in ((0, total, tracks), (65536, total, tracks), (N, 0, tracks), (N, (1 << 30) + 1, tracks), (N, total, -1), (N, total, (1 << 26) + 1)):
        assert L.rgm_midi_read_workspace(*bad) == 0
    ws = torch.full((nbytes // 8,), -7, dtype=torch.int64, device="cuda")
    status = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    counts = torch.full((N, 4), -7, dtype=torch.int64, device="cuda")
    columns = torch.full((N,), -7, dtype=torch.int64, device="cuda")
    noff, coff = torch.full((N + 1,), -7, dtype=torch.int64, device="cuda"), torch.full((N + 1,), -7, dtype=torch.int64, device="cuda")
    notes, ccs = torch.full((64, 8), -7, dtype=torch.int64, device="cuda"), torch.full((64, 5), -7, dtype=torch.int64, device="cuda")
    out = torch.full((N, 3, 128, 70), 7, dtype=torch.uint8, device="cuda")
    over = torch.full((N,), -7, dtype=torch.int64, device="cuda")

    def scan(N_=N, total_=total, tracks_=tracks, fs=100.0, blob_p=R.ptr(blob), off_p=R.ptr(off), st_p=R.ptr(status), notes_p=R.ptr(notes), notes_cap=64,
             ccs_p=R.ptr(ccs), ccs_cap=64, ws_p=R.ptr(ws), ws_b=nbytes):
        return L.rgm_midi_read_scan(blob_p, off_p, N_, total_, tracks_, fs, st_p, R.ptr(counts), R.ptr(columns), R.ptr(noff), R.ptr(coff), notes_p,
                                    notes_cap, ccs_p, ccs_cap, ws_p, ws_b, s)

    def rolls(N_=N, fs=100.0, start=0, T=70, u8=1, out_p=R.ptr(out), over_p=R.ptr(over), ws_p=R.ptr(ws), ws_b=nbytes):
        return L.rgm_midi_read_rolls(N_, total, tracks, fs, start, T, u8, out_p, over_p, ws_p, ws_b, s)
    odd = torch.zeros(blob.numel() + 16, dtype=torch.uint8, device="cuda")[1:]
    for name, code, kw in (("N = 0", -1, dict(N_=0)), ("bytes = 0", -1, dict(total_=0)), ("tracks < 0", -1, dict(tracks_=-1)), ("fs = 0", -1, dict(fs=0.0)),
                           ("fs < 0", -1, dict(fs=-100.0)), ("fs nan", -1, dict(fs=float("nan"))), ("blob", -1, dict(blob_p=None)),
                           ("unaligned blob", -1, dict(blob_p=R.ptr(odd))), ("offsets", -1, dict(off_p=None)), ("status", -1, dict(st_p=None)),
                           ("notes without pointer", -1, dict(notes_p=None)), ("notes without ccs", -1, dict(ccs_p=None, ccs_cap=0)),
                           ("negative capacity", -1, dict(notes_cap=-1)), ("ws", -3, dict(ws_p=None)), ("short ws", -3, dict(ws_b=nbytes - 16))):
        assert scan(**kw) == code, name
    for name, code, kw in (("N = 0", -1, dict(N_=0)), ("fs = 0", -1, dict(fs=0.0)), ("T = 0", -1, dict(T=0)), ("start < 0", -1, dict(start=-1)), ("flag", -1, dict(u8=2)),
                           ("out", -1, dict(out_p=None)), ("overflow", -1, dict(over_p=None)), ("ws", -3, dict(ws_p=None)), ("short ws", -3, dict(ws_b=nbytes - 16))):
        assert rolls(**kw) == code, name
    torch.cuda.synchronize()
    for t in (ws, status, counts, columns, noff, coff, notes, ccs, over):
        assert (t == -7).all()
    assert (out == 7).all() and torch.equal(blob, twin)
    assert scan() == 0                                                          # 64 rows: the first file (7 notes, 2 control changes) fits, the second too
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0] and counts[:, 0].tolist() == [7, 6] and noff.tolist() == [0, 7, 13] and coff.tolist() == [0, 2, 2]
    assert (notes[:13] != -7).all() and (notes[13:] == -7).all() and (ccs[:2] != -7).all() and (ccs[2:] == -7).all()
    notes.fill_(-7)
    ccs.fill_(-7)
    assert scan(notes_cap=12) == 0                                              # one row short for the second file: left out whole
    torch.cuda.synchronize()
    assert (notes[:7] != -7).all() and (notes[7:] == -7).all() and counts[:, 0].tolist() == [7, 6]
    assert scan(notes_p=None, notes_cap=0, ccs_p=None, ccs_cap=0) == 0 and rolls() == 0
    torch.cuda.synchronize()
    h = [_host(f, 100)["roll"] for f in files]
    for i in range(2):
        want = np.zeros((3, 128, 70), dtype=np.float32)
        want[:, :, :min(70, h[i].shape[2])] = h[i][:, :, :70]
        assert np.array_equal(out[i].cpu().numpy(), np.minimum(want, 255).astype(np.uint8))
    assert over.tolist() == [0, int((h[1][:, :, :70] > 255).sum())] and torch.equal(blob, twin)
    short = L.rgm_midi_read_scan(R.ptr(blob), R.ptr(off), N, total, 4, 100.0, R.ptr(status), R.ptr(counts), R.ptr(columns), None, None, None, 0, None, 0,
                                 R.ptr(ws), nbytes, s)                          # fewer tracks than the headers claim: the second file has no room
    torch.cuda.synchronize()
    assert short == 0 and status.tolist() == [0, 9] and counts[1].tolist() == [0, 0, 0, 0]
    for bad in ([], [b""]):
        with pytest.raises(ValueError):
            midi_util.midi_files_to_rolls(bad)
    with pytest.raises(ValueError):
        midi_util.midi_files_to_rolls(files, fs=0)
    with pytest.raises(ValueError):
        midi_util.midi_files_to_rolls(files, dtype=torch.int32)


# ------------------------------------------------------------------------------------------------ the two CLIs
def _script(name):
    import importlib.util
    from conftest import PKG
    spec = importlib.util.spec_from_file_location(name + "_cli", os.path.join(PKG, "scripts", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_edit_cli_builds_the_source_roll_on_the_device(tmp_path, monkeypatch):
    from test_gpu_cli import CFG, COMMON
    from music_rule_guidance.piano_roll_to_chord import piano_roll_to_pretty_midi
    monkeypatch.chdir(tmp_path)
    cli = _script("edit")
    src = os.path.join(str(tmp_path), "source.midi")
    piano_roll_to_pretty_midi(load_golden("midi_events")["r3.roll"].astype(np.float32), fs=100).write(src)
    text = open(os.path.join(CFG, "edit", "nd_scg_given_target.yml")).read().replace("noise_level: 500", "noise_level: 3").replace("source: dataset", f"source: {src}")
    runs = {}
    for name, extra in (("dev", ["--midi_reader", "device"]), ("plain", [])):
        cfg = os.path.join(str(tmp_path), "configs", "edit", f"nd_{name}.yml")
        os.makedirs(os.path.dirname(cfg), exist_ok=True)
        open(cfg, "w").write(text)
        res, sample = cli.main(["--config_path", cfg, "--batch_size", "1", "--num_samples", "1", "--diffusion_steps", "24"] + COMMON + extra)
        out_dir = os.path.join("loggings", "edit_demo", "edit", f"nd_{name}_cls_1")
        assert json.load(open(os.path.join(out_dir, "run_metadata.json")))["midi_reader"] == ("device" if name == "dev" else "host")
        runs[name] = {os.path.relpath(os.path.join(dp, f), out_dir): open(os.path.join(dp, f), "rb").read()
                      for dp, _, fs in os.walk(out_dir) for f in fs if f.endswith((".midi", ".npy"))}
        runs[name]["gt"] = np.load(os.path.join(out_dir, "gt", "sample_0_y_1.npy"))
        runs[name]["sample"] = sample.cpu().numpy() if torch.is_tensor(sample) else np.array(sample)
    gt = runs["dev"].pop("gt")
    assert gt.shape == (3, 128, 1024) and gt[0, :, :384].max() > 0 and not gt[0, :, 384:].any()
    assert np.array_equal(runs["plain"].pop("gt"), gt) and np.array_equal(runs["plain"].pop("sample"), runs["dev"].pop("sample"))
    assert runs["dev"].keys() == runs["plain"].keys() and len(runs["dev"]) >= 4      # the generated roll and the source, .midi and .npy each
    assert all(runs["dev"][k] == runs["plain"][k] for k in runs["dev"])


def test_midi_to_rolls_cli_writes_what_its_host_run_writes(tmp_path):
    cli = _script("midi_to_rolls")
    src = tmp_path / "src"
    src.mkdir()
    for k in ("three_tracks", "overlap_fifo", "cc_extends", "tempo_thousand"):
        (src / f"{k}.mid").write_bytes(rc.ACCEPTED[k][0])
    (src / "broken.mid").write_bytes(rc.REFUSED["ends_in_message"][0])
    metas = {}
    for reader in ("device", "host"):
        metas[reader] = cli.main(["--midi_dir", str(src), "--outdir", str(tmp_path / reader), "--image_size", "64", "--overlap", "True", "--batch_size", "3",
                                  "--midi_reader", reader])
    names = sorted(f for f in os.listdir(tmp_path / "host") if f.endswith(".npy"))
    assert names == sorted(f for f in os.listdir(tmp_path / "device") if f.endswith(".npy")) and len(names) > 10
    assert all((tmp_path / "host" / n).read_bytes() == (tmp_path / "device" / n).read_bytes() for n in names)
    d, h = metas["device"], metas["host"]
    assert [r["file"] for r in d["refused"]] == ["broken.mid"] == [r["file"] for r in h["refused"]] and "status 4" in d["refused"][0]["reason"]
    assert all(d[k] == h[k] for k in ("files", "converted", "pieces", "overflow_cells", "overflow_files")) and d["overflow_cells"] > 0
