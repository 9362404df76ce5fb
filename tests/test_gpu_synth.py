"""-m gpu: audio rendered on the device (csrc/synth.hip: rgm_synth_render, rgm_synth_pcm) against the host partner -- synthesize_events over
piano_roll_to_pretty_midi on a copy of the same roll, which tests/test_synth_host.py pins to the reference's fork bit for bit -- through
rolls_to_audio(dtype=float64, normalize=False), the C ABI, rolls_to_wav_bytes and the CLIs (docs/rounds/synth.md).

Lengths, silent flags and the zero tails are exact.  The raw waveform is held to |dev - host|[i] <= (C_ULP + m_i) * 2^-53 * V_i, m_i the
number of notes sounding at audio sample i and V_i the sum of their velocities, both from the host's own note list: the phase, the
exponent, the fade and the order of the multiplications are the host's bits, so the two libraries' sin and exp and the order of the sum
are the whole difference.  ROCm's documentation at hand states no error bound for the device's double sin and exp, so C_ULP was set as the issue
prescribes: the worst |dev - host| / (2^-53 V_i) - m_i over these cases, measured on an MI355X against the host partner, doubled, rounded
up and not below 8 (the measured value: docs/rounds/synth.md).  Every check prints its own worst value before it asserts."""
import ctypes
import io
import json
import os
import wave as wave_mod

import numpy as np
import pytest
import torch

import synth_cases as sc
from conftest import load_golden

pytestmark = pytest.mark.gpu

C_ULP = 8
EPS = 2.0 ** -53
CHUNK = 512                                              # audio samples of a render workgroup (csrc/synth.hip)
BATCH = 256                                              # notes of one LDS batch


@pytest.fixture(autouse=True)
def _fp32_behind_every_test():
    """the CLIs set the process-wide GEMM arithmetic (--gemm_precision); the modules behind this one expect the library's start-up value"""
    yield
    from rgm import native as R
    R.set_gemm_precision("fp32")


def _tensor(rolls, layout):
    t = torch.from_numpy(np.array(rolls, dtype=np.uint8, order="C", copy=True)).cuda()
    return t.permute(0, 2, 3, 1).contiguous() if layout else t


_HOST = {}


def _host(roll, audio_fs, fco, fs=sc.FS):
    """the host partner's answers for one roll, computed once per (roll, rate) and left unchanged"""
    key = (roll.tobytes(), roll.shape, audio_fs, fco, fs)
    if key not in _HOST:
        h = sc.host_render(roll, fs=fs, audio_fs=audio_fs, first_column_onsets=fco)
        for v in h.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _HOST[key] = h
    return _HOST[key]


def _raw(rolls, audio_fs, fco=True, layout=0, fs=sc.FS):
    """the device's raw rows, and the roll is checked to be unchanged"""
    from guided_diffusion import midi_util
    t = _tensor(rolls, layout)
    twin = t.clone()
    audio, lengths, silent = midi_util.rolls_to_audio(t, fs=fs, audio_fs=audio_fs, first_column_onsets=fco, normalize=False, dtype=torch.float64)
    assert torch.equal(t, twin), "the roll was written to"
    assert audio.dtype == torch.float64 and audio.shape[0] == len(rolls) and lengths.dtype == torch.int64 and silent.dtype == torch.bool
    return audio.cpu().numpy(), lengths.cpu().numpy(), silent.cpu().numpy()


WORST = {"c": -np.inf}


def _check(rolls, audio_fs, fco=True, layout=0, what="", fs=sc.FS):
    """device == host within the per-sample bound for every roll of the batch; lengths, silent and tails exact; -> the device's rows"""
    audio, lengths, silent = _raw(rolls, audio_fs, fco, layout, fs)
    worst = -np.inf
    for i, roll in enumerate(rolls):
        h = _host(roll, audio_fs, fco, fs)
        tag = f"{what} sample {i} of {len(rolls)} rate {audio_fs} layout {layout} first_column_onsets={fco}"
        L = h["raw"].shape[0]
        assert int(lengths[i]) == L, f"{tag}: length {int(lengths[i])}, host {L}"
        assert bool(silent[i]) == h["silent"], f"{tag}: silent"
        assert audio.shape[1] >= L and not audio[i, L:].any(), f"{tag}: the tail behind the length is not zero"
        d = np.abs(audio[i, :L] - h["raw"])
        quiet = h["V"] == 0
        assert not d[quiet].any(), f"{tag}: a sample where no note sounds is not equal"
        if (~quiet).any():
            c = d[~quiet] / (EPS * h["V"][~quiet]) - h["m"][~quiet]
            worst = max(worst, float(c.max()))
            k = int(np.argmax(c))
            print(f"{tag}: worst |dev - host| / (2^-53 V) - m = {c.max():.3f} (m = {h['m'][~quiet][k]}, V = {h['V'][~quiet][k]})")
            assert c.max() <= C_ULP, f"{tag}: {c.max():.3f} > {C_ULP}"
    WORST["c"] = max(WORST["c"], worst)
    return audio, lengths, silent


def _rolls(T, C, N):
    """N rolls whose first ones are shared by every N: densities from the empty roll to 0.6"""
    dens = [(0.3, 0.0, 0.08, 0.6, 0.02)[i % 5] for i in range(N)]
    return np.stack([sc.dense_roll(9000 * T + 10 * C + i, C, T, d) for i, d in enumerate(dens)])


@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("audio_fs", [50, 100, 8000])
@pytest.mark.parametrize("T", [1, 7, 64, 1000])
def test_random_rolls(T, audio_fs, C):
    """T x N in {1, 3, 17} x C x both layouts x three rates; the largest is N = 3 at T = 1000 and 8000 Hz.  Sample 1 of a batch is the
    empty roll: a silent sample between two sounding ones"""
    for N in (1, 3, 17):
        if N == 17 and T == 1000 and audio_fs == 8000:
            continue
        rolls = _rolls(T, C, N)
        for layout in (0, 1):
            _, _, silent = _check(rolls, audio_fs, fco=bool((T + C) % 2), layout=layout, what=f"T={T} C={C} N={N}")
            if N > 1:
                assert silent[1]


@pytest.mark.parametrize("case", [c[0] for c in sc.fixture_cases()])
def test_the_fixture_rolls_against_the_reference_waveforms(case):
    """the reference's own bits: Instrument.synthesize's raw sum of tests/golden/synth.npz, notes of 0, 1, 2, F and F + 1 audio samples,
    onset cuts, a zero-length note and a late pedal event included (tests/test_synth_host.py says that the rolls hold them), T = 8 at
    22050 and 44100 Hz"""
    g = load_golden("synth")
    i = [c[0] for c in sc.fixture_cases()].index(case)
    _, rname, rate = sc.fixture_cases()[i]
    roll = g[f"roll.{rname}"]
    audio, lengths, silent = _check(roll[None], rate, fco=False, layout=i % 2, what=case)
    want = g[f"raw.{case}"]
    assert int(lengths[0]) == int(g["length"][i]) == want.shape[0] and bool(silent[0]) == bool(g["norm_nan"][i])
    h = _host(roll, rate, False)
    assert h["raw"].tobytes() == want.tobytes()
    if rname == "c3" or rname == "c2":                  # the length is set by the pedal event in the last column, not by a note
        assert float(g["end_time"][i]) == (roll.shape[-1] - 1) / sc.FS and want.shape[0] == int(rate * (float(g["end_time"][i]) + 1))


def _edge_roll():
    """(3, 128, 64) for 8000 Hz, a column = 80 audio samples, a chunk = 512: column 32 is audio sample 2560, the start of chunk 5"""
    r = np.zeros((3, 128, 64), dtype=np.uint8)
    r[0, 30, 32:40], r[1, 30, 32] = 90, 127             # starts exactly on a chunk boundary
    r[0, 31, 20:32], r[1, 31, 20] = 80, 127             # ends exactly on it
    r[0, 32, 2:60], r[1, 32, 2] = 70, 127               # spans nine chunks
    r[0, 33, 10:50], r[1, 33, 10], r[1, 33, 32] = 60, 127, 127          # two notes contiguous at an onset cut on the boundary
    r[2, 21:109, 63] = 80                               # a length set by a late CC
    return r


def test_chunk_boundaries_and_contiguous_notes():
    from music_rule_guidance.piano_roll_to_chord import synth_tables
    samp = synth_tables(64, sc.FS, 8000)[0]
    assert samp[32] == 5 * CHUNK and samp[60] - samp[2] > 3 * CHUNK
    roll = _edge_roll()
    h = _host(roll, 8000, True)
    spans = set(h["spans"])
    assert {(30, 2560, int(samp[40])), (31, int(samp[20]), 2560), (33, int(samp[10]), 2560), (33, 2560, int(samp[50]))} <= spans
    assert h["raw"].shape[0] == int(8000 * (0.63 + 1)) > max(b for _, _, b in spans) + 8000
    for layout in (0, 1):
        _check(roll[None], 8000, True, layout, "edges")


def test_88_pitches_at_once():
    roll = np.zeros((1, 128, 64), dtype=np.uint8)
    roll[0, 21:109, 2:40] = np.arange(21, 109)[:, None]
    h = _host(roll, 8000, True)
    assert h["m"].max() == 88 and h["V"].max() == sum(range(21, 109))
    _check(roll[None], 8000, True, 0, "88 pitches")


def test_more_notes_in_a_chunk_than_one_lds_batch_holds():
    """50 Hz at T = 1000 on a dense roll: the whole roll lies in two chunks, thousands of notes meet the first"""
    roll = sc.dense_roll(4242, 3, 1000, 0.6)
    h = _host(roll, 50, True)
    in_first = sum(1 for _, a, b in h["spans"] if b > a and a < CHUNK)
    assert in_first > 4 * BATCH and h["raw"].shape[0] > CHUNK, in_first
    _check(roll[None], 50, True, 1, "LDS batches")


def test_peak_and_the_normalised_outputs():
    """the peak within the largest per-sample bound of the host's; the float32 rows == float32(dev_wave / dev_peak) and every int16 ==
    rint(dev_wave / dev_peak * 32767), both formed on the host from the device's own float64 rows: exactly; the headers == the wave module's"""
    from guided_diffusion import midi_util
    from music_rule_guidance.piano_roll_to_chord import wav_bytes
    rolls = np.stack([_edge_roll(), np.zeros((3, 128, 64), dtype=np.uint8), sc.dense_roll(31, 3, 64, 0.3)])
    rate = 8000
    for layout in (0, 1):
        t = _tensor(rolls, layout)
        raw, lengths, silent = _check(rolls, rate, True, layout, "normalised")
        peak = np.abs(raw).max(axis=1)
        for i, roll in enumerate(rolls):
            h = _host(roll, rate, True)
            bound = float(((C_ULP + h["m"]) * EPS * h["V"]).max()) if h["V"].any() else 0.0
            print(f"peak {i}: device {peak[i]!r} host {h['peak']!r} bound {bound:.3e}")
            assert abs(peak[i] - h["peak"]) <= bound
        audio, l32, s32 = midi_util.rolls_to_audio(t, audio_fs=rate)
        assert audio.dtype == torch.float32 and audio.shape == raw.shape and np.array_equal(l32.cpu().numpy(), lengths)
        assert np.array_equal(s32.cpu().numpy(), silent) and silent.tolist() == [False, True, False]
        norm = np.zeros_like(raw)
        norm[~silent] = raw[~silent] / peak[~silent, None]
        assert audio.cpu().numpy().tobytes() == norm.astype(np.float32).tobytes()
        a64, _, _ = midi_util.rolls_to_audio(t, audio_fs=rate, dtype=torch.float64)
        assert a64.cpu().numpy().tobytes() == norm.tobytes()
        files = midi_util.rolls_to_wav_bytes(t, audio_fs=rate)
        assert isinstance(files, list) and len(files) == 3 and all(isinstance(f, bytes) for f in files)
        for i, data in enumerate(files):
            L = int(lengths[i])
            assert len(data) == 44 + 2 * L and data[:44] == wav_bytes(np.zeros(L), rate)[:44]
            with wave_mod.open(io.BytesIO(data), "rb") as w:
                assert (w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()) == (rate, 1, 2, L)
                pcm = np.frombuffer(w.readframes(L), dtype="<i2")
            assert np.array_equal(pcm, np.rint(norm[i, :L] * 32767).astype(np.int16))
            assert (np.abs(pcm).max() == 32767) == (not silent[i])


def test_launches_repeat_and_a_sample_does_not_depend_on_its_batch():
    rolls = np.stack([sc.dense_roll(77 + i, 3, 64, 0.3) for i in range(17)])
    first = _raw(rolls, 8000)
    assert np.abs(first[0]).max(axis=1).min() > 0
    for _ in range(19):
        again = _raw(rolls, 8000)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
    alone, five = _raw(rolls[11:12], 8000), _raw(rolls[9:14], 8000)
    assert alone[0][0].tobytes() == first[0][11].tobytes() == five[0][2].tobytes()       # alone / row 2 of 5 / row 11 of 17
    assert alone[1][0] == first[1][11] == five[1][2]


def test_python_surface():
    """other column rates, both dtypes, and the refusals"""
    from guided_diffusion import midi_util
    rolls = np.stack([sc.dense_roll(5 + i, 3, 129, 0.3) for i in range(2)])
    for fs in (50, 200):
        _check(rolls, 8000, True, 1, f"fs={fs}", fs=fs)
    t = _tensor(rolls, 1)
    r32, _, _ = midi_util.rolls_to_audio(t, audio_fs=8000, normalize=False)
    r64, _, _ = midi_util.rolls_to_audio(t, audio_fs=8000, normalize=False, dtype=torch.float64)
    assert r32.dtype == torch.float32 and torch.equal(r32, r64.float())
    for bad in (0, -8000):
        with pytest.raises(ValueError, match="audio_fs"):
            midi_util.rolls_to_audio(t, audio_fs=bad)
    with pytest.raises(ValueError):
        midi_util.rolls_to_audio(t, audio_fs=1e9)       # 2^31 samples and more
    with pytest.raises(ValueError, match="fs"):
        midi_util.rolls_to_audio(t, fs=250)
    with pytest.raises(ValueError):
        midi_util.rolls_to_wav_bytes(t, audio_fs=8000.5)
    with pytest.raises(ValueError):
        midi_util.rolls_to_audio(t, dtype=torch.float16)
    with pytest.raises(ValueError):
        midi_util.rolls_to_audio(torch.zeros((1, 3, 128, 64), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="wav_bytes"):
        midi_util.save_piano_roll_midi(rolls, "unused", wav_bytes=[b""])


def test_arguments_are_checked_before_any_launch():
    """audio_fs <= 0, a length of 2^31, a table that decreases, a short cap, a short workspace, NULL pointers: a status, nothing written"""
    from guided_diffusion import midi_util
    from music_rule_guidance import music_rules
    from rgm import native as R
    L = R.lib
    T, N, rate = 64, 2, 8000
    assert L.rgm_synth_workspace(1, 32768, 1 << 20) > 0 and L.rgm_synth_workspace(65535, 1, 8) > 0
    assert L.rgm_synth_workspace(0, 64, 4096) == 0 and L.rgm_synth_workspace(1, 0, 4096) == 0 and L.rgm_synth_workspace(1, 32769, 4096) == 0
    assert L.rgm_synth_workspace(1, 64, 0) == 0 and L.rgm_synth_workspace(1, 64, 1 << 31) == 0
    rolls = np.stack([_edge_roll(), sc.dense_roll(31, 3, 64, 0.3)])
    ev = music_rules.midi_events_raw(_tensor(rolls, 0), first_column_onsets=True)
    samp, length, omega, fade = midi_util.synth_host_tables(T, sc.FS, rate)
    cap = (int(length[T]) + 7) // 8 * 8
    wave = torch.full((N, cap), -7.0, dtype=torch.float64, device="cuda")
    lengths = torch.full((N,), -7, dtype=torch.int64, device="cuda")
    peak = torch.full((N,), -7.0, dtype=torch.float64, device="cuda")
    silent = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    nbytes = L.rgm_synth_workspace(N, T, cap)
    ws = torch.full(((nbytes + 15) // 16 * 2,), -7, dtype=torch.int64, device="cuda")
    s = R.current_stream()
    P = lambda a: ctypes.c_void_p(a.ctypes.data)        # noqa: E731

    def render(N_=N, T_=T, rate_=float(rate), samp_p=P(samp), len_p=P(length), omega_p=P(omega), fade_p=P(fade), F=len(fade), wave_p=R.ptr(wave),
               cap_=cap, ws_p=R.ptr(ws), ws_b=ws.numel() * 8, counts_p=R.ptr(ev["counts"])):
        return L.rgm_synth_render(N_, T_, R.ptr(ev["notes"]), ev["notes"].shape[0], R.ptr(ev["note_offsets"]), R.ptr(ev["ccs"]), ev["ccs"].shape[0],
                                  R.ptr(ev["cc_offsets"]), counts_p, rate_, samp_p, len_p, omega_p, fade_p, F, wave_p, cap_, R.ptr(lengths),
                                  R.ptr(peak), R.ptr(silent), ws_p, ws_b, s)
    down, far, behind = np.array(samp), np.array(length), np.array(samp)
    down[10] = down[9] - 1
    far[-1] = 1 << 31
    behind[5] = length[5] + 1
    behind[6:] = np.maximum(behind[6:], behind[5])
    for name, status, kw in (("audio_fs = 0", -1, dict(rate_=0.0)), ("audio_fs < 0", -1, dict(rate_=-8000.0)), ("2^31 samples", -1, dict(len_p=P(far))),
                             ("a table decreases", -1, dict(samp_p=P(down))), ("samp behind len", -1, dict(samp_p=P(behind))),
                             ("short cap", -1, dict(cap_=cap - 8)), ("odd cap", -1, dict(cap_=cap + 4)), ("T = 0", -1, dict(T_=0)),
                             ("N = 0", -1, dict(N_=0)), ("tables", -1, dict(samp_p=None)), ("wave", -1, dict(wave_p=None)),
                             ("counts", -1, dict(counts_p=None)), ("fade", -1, dict(fade_p=None)), ("long fade", -1, dict(F=cap)),
                             ("ws", -3, dict(ws_p=None)), ("short ws", -3, dict(ws_b=nbytes - 8))):
        assert render(**kw) == status, name
        assert L.rgm_last_error(), name
    assert render(samp_p=P(down)) == -1 and b"decreases from column 9 to 10" in L.rgm_last_error()
    out = torch.full((N * (44 + 2 * cap),), 7, dtype=torch.uint8, device="cuda")
    for name, kw in (("format", dict(fmt=2)), ("rate", dict(rate_=0)), ("cap", dict(cap_=cap + 4)), ("out", dict(out_p=None)), ("N", dict(N_=0))):
        a = dict(N_=N, cap_=cap, fmt=1, rate_=rate, out_p=R.ptr(out))
        a.update(kw)
        assert L.rgm_synth_pcm(a["N_"], R.ptr(wave), R.ptr(lengths), R.ptr(peak), a["cap_"], a["fmt"], a["rate_"], a["out_p"], s) == -1, name
    torch.cuda.synchronize()
    assert (wave == -7).all() and (lengths == -7).all() and (peak == -7).all() and (silent == -7).all() and (ws == -7).all() and (out == 7).all()
    assert render() == 0
    torch.cuda.synchronize()
    for i, roll in enumerate(rolls):
        h = _host(roll, rate, True)
        assert int(lengths[i]) == h["raw"].shape[0] and int(silent[i]) == 0
        d = np.abs(wave[i, :h["raw"].shape[0]].cpu().numpy() - h["raw"])
        assert (d <= (C_ULP + h["m"]) * EPS * h["V"]).all() and not wave[i, h["raw"].shape[0]:].any()
    with pytest.raises(ValueError):
        midi_util.rolls_to_audio(torch.zeros((0, 3, 128, 64), dtype=torch.uint8, device="cuda"))


# ------------------------------------------------------------------------------------------------ the CLIs, synthetic weights
def _script(name):
    import importlib.util
    from conftest import PKG
    spec = importlib.util.spec_from_file_location(name + "_cli", os.path.join(PKG, "scripts", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_sample_rule_cli_writes_a_wav_beside_every_midi_and_rolls_to_wav_repeats_them(tmp_path, monkeypatch):
    from guided_diffusion import midi_util
    from test_gpu_cli import CFG, COMMON
    monkeypatch.chdir(tmp_path)
    cli = _script("sample_rule")
    cfg = os.path.join(CFG, "cond_table/single/scg/nd.yml")
    argv = ["--config_path", cfg, "--batch_size", "2", "--num_samples", "2", "--diffusion_steps", "24", "--sampler", "dpmpp", "--dpmpp_steps", "2"] + COMMON
    out_dir = os.path.join("loggings", cli.output_dir_for(cfg, 1))
    res = cli.main(argv + ["--wav", "device", "--wav_fs", "8000"])
    meta = json.load(open(os.path.join(out_dir, "run_metadata.json")))
    assert len(res) == 2 and meta["wav"] == "device" and meta["wav_fs"] == 8000 and meta["midi_backend"] == "host"
    stems = ["sample_0_y_1", "sample_1_y_1"]
    names = sorted(f for f in os.listdir(out_dir) if f.startswith("sample_"))
    assert names == sorted(s + ext for s in stems for ext in (".midi", ".npy", ".wav")), names
    for s_ in stems:
        roll = np.load(os.path.join(out_dir, s_ + ".npy"))
        data = open(os.path.join(out_dir, s_ + ".wav"), "rb").read()
        with wave_mod.open(io.BytesIO(data), "rb") as w:
            assert (w.getframerate(), w.getnchannels(), w.getsampwidth()) == (8000, 1, 2) and w.getnframes() == (len(data) - 44) // 2 >= 8000
        assert data == midi_util.rolls_to_wav_bytes(_tensor(roll[None], 0), audio_fs=8000)[0], s_
    conv = _script("rolls_to_wav")
    wav_dir = str(tmp_path / "wavs")
    m = conv.main(["--roll_dir", out_dir, "--outdir", wav_dir, "--wav_fs", "8000", "--batch", "1"])
    assert m["written"] == 2 and not m["skipped"]
    for s_ in stems:
        assert open(os.path.join(wav_dir, s_ + ".wav"), "rb").read() == open(os.path.join(out_dir, s_ + ".wav"), "rb").read()
