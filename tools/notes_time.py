"""What the note statistics cost.  (1) rgm_note_stats at (N, C, T) = (64, 3, 1024) on a prepared uint8 roll in the layout
decode_sample_for_midi returns, and note_stats on the float roll (quantiser + kernel), HIP events behind a warm-up.  (2) The host partner
piano_roll_note_stats per excerpt on one core.  (3) How far the statistics move when the fixture rolls go through the project's own
SimpleMIDI write -> read round trip (times rounded to MIDI ticks): reported, not asserted.  (4) One SCG search step of XL-28
(bf16x3_presplit, synthetic weights) with B = 4 samples x n = 16 candidates: note_density alone, and note_density + mg_mean_duration --
same process, same box.  Writes profiles/notes_time.json and prints it as one line.

    python tools/notes_time.py [--out profiles/notes_time.json] [--repeats 5] [--host_only]"""
import argparse
import json
import os
import sys
import tempfile
import time
from functools import partial
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rule-guided-music_amd"), os.path.join(ROOT, "tests")]

XL28 = dict(depth=28, hidden=1152, heads=16, patch=8, in_ch=4, out_ch=4, num_classes=3)
B, N_CAND, H = 4, 16, 128


def timed(fn, iters, warmup=20):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters          # ms


def rolls(n, T=1024):
    import notes_cases as nc
    return np.stack([nc.random_roll(5000 + i, 3, T) for i in range(n)])


def kernel_alone(iters=200):
    import torch
    from music_rule_guidance import music_rules
    N, T = 64, 1024
    u = torch.from_numpy(rolls(N, T)).cuda().permute(0, 2, 3, 1).contiguous()          # (N, 128, T, 3)
    x = (u.permute(0, 3, 1, 2).float() / 63.5 - 1).contiguous()
    k = timed(lambda: music_rules.note_stats_raw(u, True), iters)
    whole = timed(lambda: music_rules.note_stats(x), iters)
    return {"shape": f"N{N}_C3_T{T}", "rgm_note_stats_call_us": round(k * 1e3, 2), "note_stats_on_float_roll_call_us": round(whole * 1e3, 2),
            "notes_per_roll_mean": float(music_rules.note_stats(u)["n_notes"].double().mean())}


def host_partner():
    from music_rule_guidance.piano_roll_to_chord import piano_roll_note_stats
    r = rolls(20)
    piano_roll_note_stats(r[0])
    t0 = time.perf_counter()
    for x in r:
        piano_roll_note_stats(x, first_column_onsets=True)
    return {"shape": "C3_T1024", "host_partner_ms_per_excerpt": round((time.perf_counter() - t0) / len(r) * 1e3, 3)}


def midi_round_trip():
    """largest change of each scalar statistic over the fixture rolls when the notes and pedal events go through SimpleMIDI.write and the
    reader: start / end times come back rounded to ticks (220 per quarter at 120 bpm: 4.4 per column)"""
    import notes_cases as nc
    from music_rule_guidance.piano_roll_to_chord import SimpleMIDI, piano_roll_note_stats, piano_roll_to_pretty_midi
    worst = {"n_notes": 0.0, "end_time": 0.0, "avg_IOI": 0.0, "mean_note_duration": 0.0, "note_density_mgeval": 0.0, "mean_note_velocity": 0.0}
    count = 0
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "x.midi")
        for name, roll in nc.cases().items():
            if not name.startswith("random.") or roll.shape[0] != 3:
                continue
            want = piano_roll_note_stats(roll)
            piano_roll_to_pretty_midi(roll.astype(np.float32).copy(), fs=100).write(path)
            back = SimpleMIDI(path)
            notes = [n for ins in back.instruments for n in ins.notes]
            if not notes:
                continue
            count += 1
            st = sorted(n.start for n in notes)
            end = back.get_end_time()
            got = {"n_notes": len(notes), "end_time": end, "avg_IOI": (st[-1] - st[0]) / (len(st) - 1) if len(st) > 1 else float("nan"),
                   "mean_note_duration": sum(n.end - n.start for n in notes) / len(notes), "note_density_mgeval": len(notes) / end if end else 0.0,
                   "mean_note_velocity": sum(n.velocity for n in notes) // len(notes)}
            for k in worst:
                d = abs(float(got[k]) - float(want[k]))
                if d == d:
                    worst[k] = max(worst[k], d)
    return {"rolls": count, "largest_change": {k: float(f"{v:.6g}") for k, v in worst.items()}}


def search_step(repeats):
    import torch
    from guided_diffusion.condition_functions import model_fn
    from guided_diffusion.dit import DiTRotary
    from guided_diffusion.gaussian_diffusion import PhiloxNoise
    from guided_diffusion.script_util import create_diffusion
    from music_rule_guidance import music_rules
    from rgm import synth
    from taming.models.klvae_pedal import AutoencoderKL
    m = DiTRotary(input_size=[H, 16], patch_size=8, in_channels=4, hidden_size=1152, depth=28, num_heads=16, num_classes=3, learn_sigma=False)
    m.load_state_dict(synth.dit_state_dict(1, final_std=0.3 / 1152 ** 0.5, device="cuda", **XL28))
    m = m.to("cuda").eval()
    vae = AutoencoderKL()
    vae.load_state_dict(synth.vae_state_dict(2, device="cuda", encoder=True))
    vae = vae.to("cuda").eval()
    mf = partial(model_fn, model=m, num_classes=3, class_cond=True, cfg=False, w=0.)
    x = torch.randn((B, 4, H, 16), device="cuda") * 0.5
    t = torch.full((B,), 400, dtype=torch.long, device="cuda")
    y = torch.arange(B, device="cuda") % 3
    seed_roll = (torch.from_numpy(rolls(B, 8 * H)).cuda().float() / 63.5 - 1).contiguous()
    nd = music_rules.note_density(seed_roll.clone())
    rules = {"note_density": nd, "mg_mean_duration": torch.full((B, 1), 0.25, device="cuda")}
    guid = SimpleNamespace(schedule=True, t_start=750, t_end=0, interval=1, method="no_guidance")

    def step(names):
        d = create_diffusion(learn_sigma=False, diffusion_steps=1000, noise_schedule="linear", timestep_respacing="", use_kl=False,
                             predict_xstart=False, rescale_timesteps=False, rescale_learned_sigmas=False)
        d.t_end = 0
        d.noise = PhiloxNoise(seed=99)
        r = {k: rules[k] for k in names}
        scg = dict(num_samples=N_CAND, **{k: 1. for k in r})

        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d.p_sample(mf, x, t, clip_denoised=False, model_kwargs={"y": y, "rule": r}, embed_model=vae, scale_factor=1.2465,
                       guidance_kwargs=guid, scg_kwargs=scg)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        for _ in range(2):
            run()
        return round(min(run() for _ in range(repeats)), 2)

    return {"shape": f"B{B}_n{N_CAND}_H{H}", "network": "XL-28 bf16x3_presplit, synthetic weights",
            "note_density_ms": step(["note_density"]), "note_density_and_mg_mean_duration_ms": step(["note_density", "mg_mean_duration"]),
            "note_density_again_ms": step(["note_density"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "notes_time.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host_only", action="store_true", help="the host partner and the MIDI round trip only (no GPU needed)")
    a = ap.parse_args()
    out = {"host_partner": host_partner(), "midi_round_trip": midi_round_trip()}
    if not a.host_only:
        import torch
        from rgm import native as R
        torch.backends.cuda.matmul.allow_tf32 = False
        R.set_gemm_precision("bf16x3_presplit")
        out.update({"kernel_alone": kernel_alone(), "search_step": search_step(a.repeats), "device": torch.cuda.get_device_name(0)})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
