"""-m gpu: mgeval's note statistics on the device (csrc/notes.hip: rgm_note_stats, rgm_roll_to_u8) against the reference's answers in
tests/golden/notes.npz and against the host partner, through the ABI, through FUNC_DICT, inside an SCG search step and from the CLI.
Comparison rules (docs/rounds/notes.md, notes_cases.check): integers, transition counts and the NaN pattern exact, histogram and notes
per second within one ulp, mean duration and average IOI within 4 n 2^-53 end_time.

The file name puts these tests behind the test_gpu_* files, like tests/test_rule_chords_gpu.py: the search step and the CLI runs build
models, and the suite's wall-clock tests are sensitive to what the process has created before them."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import notes_cases as nc
from conftest import load_golden

pytestmark = pytest.mark.gpu
MG_RULES = {"mg_used_pitch": 1, "mg_pitch_range": 1, "mg_avg_ioi": 1, "mg_mean_velocity": 1, "mg_mean_duration": 1,
            "mg_notes_per_second": 1, "mg_pitch_class_hist": 12, "mg_transition": 144}


@pytest.fixture(scope="module")
def gold():
    return load_golden("notes")


@pytest.fixture(scope="module")
def cases():
    return nc.cases()


def _raw(rolls, fco, layout):
    """(N, C, 128, T) uint8 numpy -> the kernel's two outputs; layout 1 hands over the (N, 128, T, C) tensor decode_sample_for_midi
    returns, layout 2 a channel-first VIEW of it (the strides of that tensor, no copy)"""
    from music_rule_guidance import music_rules
    t = torch.from_numpy(np.ascontiguousarray(rolls)).cuda()
    if layout:
        t = t.permute(0, 2, 3, 1).contiguous()
        if layout == 2:
            t = t.permute(0, 3, 1, 2)
            assert not t.is_contiguous() or t.shape[1] == 1
    oi, orl = music_rules.note_stats_raw(t, bool(fco))
    assert oi.shape == (rolls.shape[0], 148) and oi.dtype == torch.int64 and orl.shape == (rolls.shape[0], 16) and orl.dtype == torch.float64
    return oi.cpu().numpy(), orl.cpu().numpy()


def test_kernel_matches_the_reference_on_every_case_in_batches_and_both_layouts(gold, cases):
    """every case of the fixture, in batches of 1, 3 and 5 rows of different cases with the same (C, T) -- no padding: the golden of a
    case holds for its own T only"""
    names = list(cases)
    groups = {}
    for i, n in enumerate(names):
        groups.setdefault(cases[n].shape, []).append(i)
    worst_ulp = worst_abs = 0.0
    done = 0
    for shape, idx in groups.items():
        pos, k = 0, 0
        while pos < len(idx):
            rows = idx[pos:pos + (1, 3, 5)[k % 3]]
            pos, k = pos + len(rows), k + 1
            batch = np.stack([cases[names[i]] for i in rows])
            for fco in (0, 1):
                for layout in (0, 1, 2):
                    oi, orl = _raw(batch, fco, layout)
                    for r, i in enumerate(rows):
                        u, d = nc.check(oi[r], orl[r], gold["ints"][i, fco], gold["real"][i, fco],
                                        f"{names[i]} first_column_onsets={fco} layout={layout} row {r} of {len(rows)}")
                        worst_ulp, worst_abs = max(worst_ulp, u), max(worst_abs, d)
            done += len(rows)
    assert done == len(names)
    print(f"kernel: histogram / notes per second off by at most {worst_ulp:.3e} relative, mean duration / IOI by {worst_abs:.3e}")


def test_kernel_matches_the_host_partner_beyond_the_fixture():
    """sizes the fixture does not hold: T = 1 and 63 .. 65 (one word and its edges), 2500 columns (ten transition tiles), against the
    host partner under the same rules"""
    from music_rule_guidance.piano_roll_to_chord import piano_roll_note_stats
    for T in (1, 63, 64, 65, 2500):
        for C in (1, 2, 3):
            batch = np.stack([nc.random_roll(900 + 7 * T + s, C, T) for s in range(3)])
            for fco in (0, 1):
                oi, orl = _raw(batch, fco, 1)
                for r in range(3):
                    gi, gr = nc.pack(piano_roll_note_stats(batch[r], first_column_onsets=bool(fco)))
                    nc.check(oi[r], orl[r], gi, gr, f"T={T} C={C} row {r} first_column_onsets={fco}")


def test_launches_repeat_bitwise_and_rows_do_not_depend_on_the_batch():
    rolls = np.stack([nc.random_roll(5000 + i, 3, 1024) for i in range(64)])
    first = _raw(rolls, 1, 1)
    assert first[0][:, 0].min() >= 2
    for _ in range(19):
        again = _raw(rolls, 1, 1)
        assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    five = _raw(rolls[10:15], 1, 1)
    alone = _raw(rolls[13:14], 1, 1)
    for a, b, c in zip(first, five, alone):
        assert a[13].tobytes() == b[3].tobytes() == c[0].tobytes()


def test_arguments_are_checked_before_any_launch():
    from music_rule_guidance import music_rules
    from rgm import native as R
    with pytest.raises(ValueError, match="fs = 100"):
        music_rules.note_stats(torch.zeros((1, 3, 128, 64), dtype=torch.uint8, device="cuda"), fs=12.5)
    with pytest.raises(ValueError):
        music_rules.note_stats(torch.zeros((1, 4, 128, 64), dtype=torch.uint8, device="cuda"))
    assert R.lib.rgm_note_stats_workspace(1, 32768) > 0 and R.lib.rgm_note_stats_workspace(1, 32769) == 0
    roll = torch.zeros((1, 1, 128, 64), dtype=torch.uint8, device="cuda")
    oi = torch.zeros((1, 148), dtype=torch.int64, device="cuda")
    orl = torch.zeros((1, 16), dtype=torch.float64, device="cuda")
    ws = torch.zeros(8, dtype=torch.int64, device="cuda")                      # too small
    assert R.lib.rgm_note_stats(R.ptr(roll), 128 * 64, 128 * 64, 64, 1, 1, 1, 64, 0, R.ptr(oi), R.ptr(orl), R.ptr(ws), 64, R.current_stream()) != 0
    assert b"workspace" in R.lib.rgm_last_error()
    assert R.lib.rgm_note_stats(R.ptr(roll), 128 * 64, 128 * 64, 64, 1, 1, 4, 64, 0, R.ptr(oi), R.ptr(orl), R.ptr(ws), 64, R.current_stream()) != 0


def _levels_roll():
    """(1, 3, 128, 64) uint8 holding all 128 levels in every channel: velocity and pedal rows hold their own index on columns 8 .. 39, the
    onset rows 127 minus it in column 8, so that the notes of rows 21 .. 63 (velocities 21 .. 63, above the background 20 of the rows below) start"""
    u = np.zeros((1, 3, 128, 64), dtype=np.uint8)
    u[0, 0, :, 8:40] = np.arange(128, dtype=np.uint8)[:, None]
    u[0, 1, :, 8] = 127 - np.arange(128, dtype=np.uint8)
    u[0, 2, :, 8:40] = np.arange(128, dtype=np.uint8)[:, None]
    return u


def test_roll_to_u8_returns_every_level():
    """a roll holding all 128 levels in every channel, sent through u8 / 63.5 - 1, comes back equal (plain truncation loses levels 1 .. 4,
    9, 10 and 18 .. 21; a background threshold at -0.95 would lose 1 .. 3)"""
    from music_rule_guidance import music_rules
    u = torch.from_numpy(_levels_roll()).cuda()
    x = u.float() / 63.5 - 1
    twin = x.clone()
    back = music_rules.roll_to_u8(x)
    assert torch.equal(x, twin) and back.dtype == torch.uint8 and back.shape == u.shape
    lost = sorted(set(u[back != u].tolist()))
    assert torch.equal(back, u), f"levels {lost} do not come back"
    trunc = ((x + 1) * 63.5).clamp(0, 127).to(torch.uint8)
    assert 21 in set(u[trunc != u].tolist())                                    # what the bias is for
    # out of range and the ends of the range
    edge = torch.tensor([-3.0, -1.0, -0.99, 1.0, 1.5], device="cuda").reshape(1, 1, 1, 5).expand(1, 1, 128, 5)
    assert music_rules.roll_to_u8(edge)[0, 0, 7].tolist() == [0, 0, 0, 127, 127]


def test_mean_velocity_of_the_float_roll_equals_that_of_the_uint8_roll():
    """FUNC_DICT["mg_mean_velocity"] on u8 / 63.5 - 1 equals note_stats on the uint8 roll; with plain truncation levels 18 .. 21
    come back one lower, the note of row 21 takes velocity 20 and the mean drops to 41"""
    from music_rule_guidance import music_rules
    from music_rule_guidance.rule_maps import FUNC_DICT
    u = torch.from_numpy(_levels_roll()).cuda()
    want = music_rules.note_stats(u)
    assert int(want["n_notes"][0]) == 43 and int(want["mean_note_velocity"][0]) == 42
    x = u.float() / 63.5 - 1
    assert FUNC_DICT["mg_mean_velocity"](x).tolist() == [42.0]
    trunc = ((x + 1) * 63.5).clamp(0, 127).to(torch.uint8)                      # what plain truncation would hand to the kernel
    assert 21 in set(u[trunc != u].tolist()) and int(music_rules.note_stats(trunc)["mean_note_velocity"][0]) == 41
    got = music_rules.note_stats(x)
    for k in want:
        assert torch.equal(torch.nan_to_num(got[k].double(), nan=-1.0), torch.nan_to_num(want[k].double(), nan=-1.0)), k


def test_rule_entries_shapes_squeeze_nan_and_the_untouched_roll(cases):
    from music_rule_guidance import music_rules
    from music_rule_guidance.rule_maps import FUNC_DICT, LOSS_DICT
    u = torch.from_numpy(np.stack([cases[f"random.t384.c3.s{i}"] for i in range(3)])).cuda()
    x = u.float() / 63.5 - 1
    twin = x.clone()
    st = music_rules.note_stats(u)
    for name, K in MG_RULES.items():
        out = FUNC_DICT[name](x)
        assert out.shape == (3, K) and out.dtype == torch.float32 and out.is_cuda and torch.isfinite(out).all(), name
        one = FUNC_DICT[name](x[1:2])
        assert one.shape == (K,) and torch.equal(one, out[1]), name
        assert LOSS_DICT[name](out, out).abs().max() == 0
        cpu = FUNC_DICT[name](x.cpu())
        assert not cpu.is_cuda and torch.equal(cpu, out.cpu()), name
    assert torch.equal(x, twin)                                                  # nothing is written into the caller's roll
    assert torch.equal(FUNC_DICT["mg_pitch_range"](x)[:, 0].double(), st["pitch_range"].double())
    tr = FUNC_DICT["mg_transition"](x)
    assert torch.allclose(tr.sum(dim=1), torch.ones(3, device="cuda"), atol=1e-6)
    # one note: avg_IOI is NaN and the transition matrix is all zero (0 / 0) in the raw statistics, 0 in the rules
    one = torch.from_numpy(cases["one_note.c3"]).cuda()[None]
    raw = music_rules.note_stats(one)
    assert int(raw["n_notes"][0]) == 1 and torch.isnan(raw["avg_IOI"][0]) and int(raw["pitch_class_transition_matrix"].sum()) == 0
    xf = one.float() / 63.5 - 1
    assert FUNC_DICT["mg_avg_ioi"](xf).tolist() == [0.0] and FUNC_DICT["mg_transition"](xf).abs().max() == 0
    silent = torch.full((2, 3, 128, 64), -1.0, device="cuda")
    assert FUNC_DICT["mg_pitch_class_hist"](silent).abs().max() == 0            # NaN histogram of an empty roll -> 0


def test_dps_rule_call_takes_the_zero_gradient_path(cases, monkeypatch):
    from guided_diffusion.condition_functions import _rule_x0_vag
    from music_rule_guidance.rule_maps import FUNC_DICT

    def no_autograd(*a, **k):
        raise AssertionError("autograd was invoked for a hard-count rule")
    monkeypatch.setattr(torch.autograd, "grad", no_autograd)
    u = torch.from_numpy(np.stack([cases[f"random.t384.c3.s{i}"] for i in range(2)])).cuda()
    x = u.float() / 63.5 - 1
    target = torch.tensor([[30.0], [12.0]], device="cuda")
    lp, grad = _rule_x0_vag(x, target, "mg_pitch_range", 2.0)
    assert grad is None and lp.shape == (2,)
    want = -2.0 * ((FUNC_DICT["mg_pitch_range"](x) - target) ** 2).sum(dim=1)
    assert torch.allclose(lp, want, rtol=1e-6)


def _host_rule(stat):
    """the FUNC_DICT entry of one statistic served by the host partner on .cpu() rolls (the quantiser of rgm_roll_to_u8 in numpy float32)"""
    from music_rule_guidance.piano_roll_to_chord import piano_roll_note_stats

    def fn(piano_roll):
        x = piano_roll.detach().float().cpu().numpy()
        q = np.clip((x + np.float32(1)) * np.float32(63.5) + np.float32(2.0 ** -10), 0, 127).astype(np.uint8)
        vals = np.array([[float(piano_roll_note_stats(r)[stat])] for r in q], dtype=np.float64)
        out = torch.from_numpy(np.nan_to_num(vals, nan=0.0, posinf=0.0, neginf=0.0).astype(np.float32)).to(piano_roll.device)
        return out.squeeze(0) if out.shape[0] == 1 else out
    return fn


def test_search_step_is_the_same_under_the_device_and_the_host_partner(monkeypatch):
    """one SCG step (B = 2, n = 4) of the synthetic eps-network and the real decoder path with mg_pitch_range + mg_mean_duration: scored on
    the device against the same two keys served by the host partner -- log-probability table, winners and sample bit for bit"""
    from gpu_util import dev
    from guided_diffusion.gaussian_diffusion import PhiloxNoise
    from music_rule_guidance import rule_maps
    from test_gpu_sampler import SM, _diffusion, _dit, _model_fn, _vae
    g = load_golden("steps")
    m, vae = _dit(SM, 11), _vae(2)
    rules = {"mg_pitch_range": torch.tensor([[40.0], [24.0]], device="cuda"), "mg_mean_duration": torch.tensor([[0.25], [0.5]], device="cuda")}
    scg = dict(num_samples=4, mg_pitch_range=0.01, mg_mean_duration=5.)

    def run():
        guid = SimpleNamespace(schedule=True, t_start=750, t_end=0, interval=1, method="no_guidance", dc=SimpleNamespace(base=0))
        d = _diffusion("")
        d.t_end = 0
        d.noise = PhiloxNoise(seed=99)
        out = d.p_sample(_model_fn(m), dev(g["x"]), dev(g["scg.t"]), clip_denoised=False, model_kwargs={"y": dev(g["y"]), "rule": rules},
                         embed_model=vae, scale_factor=1.2465, guidance_kwargs=guid, scg_kwargs=scg)
        return out["sample"].clone(), d.last_scg["total_log_prob"].clone(), d.last_scg["max_ind"].clone()
    device = run()
    monkeypatch.setitem(rule_maps.FUNC_DICT, "mg_pitch_range", _host_rule("pitch_range"))
    monkeypatch.setitem(rule_maps.FUNC_DICT, "mg_mean_duration", _host_rule("mean_note_duration"))
    host = run()
    assert device[1].shape == (4, 2) and torch.isfinite(device[1]).all() and device[1].unique().numel() > 1
    for a, b in zip(device, host):
        assert torch.equal(a, b)


def test_sample_rule_cli_reports_the_note_statistics_of_the_saved_rolls(tmp_path, monkeypatch):
    """scripts/sample_rule.py --note_stats True, two solver steps, synthetic weights: the notes.* columns are the host partner's answers on
    the saved .npy rolls (first-column onsets, as in the saved file), their means are in summary.csv, the metadata records the switch; a
    run without the flag has no such column"""
    import pandas as pd
    from music_rule_guidance.piano_roll_to_chord import piano_roll_note_stats
    from test_gpu_cli import CFG, COMMON, _cli
    monkeypatch.chdir(tmp_path)
    cli = _cli()
    cfg = os.path.join(CFG, "cond_table/single/scg/nd.yml")
    argv = ["--config_path", cfg, "--batch_size", "2", "--num_samples", "2", "--diffusion_steps", "24", "--sampler", "dpmpp", "--dpmpp_steps", "2"] + COMMON
    res = cli.main(argv + ["--note_stats", "True"])
    out_dir = os.path.join("loggings", cli.output_dir_for(cfg, 1))
    assert json.load(open(os.path.join(out_dir, "run_metadata.json")))["note_stats"] is True
    df = pd.read_csv(os.path.join(out_dir, "results.csv"))
    note_cols = [c for c in df.columns if c.startswith("notes.")]
    assert len(note_cols) == 10 and len(df) == 2 and set(note_cols) == {c for c in res.columns if c.startswith("notes.")}
    for i in range(2):
        roll = np.load(os.path.join(out_dir, f"sample_{i}_y_1.npy"))
        assert roll.shape[:2] == (3, 128) and roll.dtype == np.uint8
        gi, gr = nc.pack(piano_roll_note_stats(roll, first_column_onsets=True))
        row = {k: res["notes." + k][i] for k in nc.INT_FIELDS + nc.REAL_FIELDS + ("pitch_class_transition_matrix", "total_pitch_class_histogram")}
        nc.check(*nc.pack(row), gi, gr, f"sample {i}")
        assert df["notes.n_notes"][i] == gi[0]
    summary = pd.read_csv(os.path.join(out_dir, "summary.csv"))
    assert "notes.mean_note_duration" in set(summary["Attr"]) and "note_density.loss" in set(summary["Attr"])
    mean = float(summary[summary["Attr"] == "notes.n_notes"]["Mean"].iloc[0])
    assert mean == float(np.mean(res["notes.n_notes"]))
    plain = cli.main(argv)
    assert not [c for c in plain.columns if c.startswith("notes.")]
    df = pd.read_csv(os.path.join(out_dir, "results.csv"))
    assert not [c for c in df.columns if c.startswith("notes.")]
    assert json.load(open(os.path.join(out_dir, "run_metadata.json")))["note_stats"] is False
