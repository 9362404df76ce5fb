"""What the native chord analyser costs.  (1) The scoring alone at (N, T) = (64, 1024), 128 columns per window: rgm_rule_chords on a
prepared uint8 roll, and get_chords (preamble + analyser) on the float roll, HIP events behind a warm-up.  (2) One SCG search step of XL-28
(bf16x3_presplit, synthetic weights) with B = 4 samples x n = 16 candidates and the rules chord_progression + note_density: without the
chord rule, with the device analyser (register_chord_backend("native")), and with its host partner piano_roll_to_chords_native in the
4-worker pool -- same process, same box.  The figures are reported, not asserted.  Writes profiles/chords_time.json and prints it as one
line.

    python tools/chords_time.py [--out profiles/chords_time.json] [--repeats 5]"""
import argparse
import json
import os
import sys
import time
from functools import partial
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rule-guided-music_amd")]

XL28 = dict(depth=28, hidden=1152, heads=16, patch=8, in_ch=4, out_ch=4, num_classes=3)
B, N_CAND, H = 4, 16, 128


def timed(fn, iters, warmup=5):
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


def test_rolls(n, T):
    """float rolls (n, 3, 128, T) with held block chords (what a decoded candidate looks like to the analyser: long slices and rests)"""
    import numpy as np
    rng = np.random.default_rng(0)
    x = rng.uniform(-1.0, -0.96, size=(n, 3, 128, T)).astype(np.float32)
    for i in range(n):
        t = 0
        while t < T:
            dur = int(rng.integers(8, 96))
            base = int(rng.integers(36, 84))
            for iv in rng.choice([0, 3, 4, 7, 10, 12, 16], size=int(rng.integers(1, 5)), replace=False):
                x[i, 0, base + int(iv), t:t + dur] = rng.uniform(-0.5, 1.0)
            t += dur
    return x


def scoring_alone(iters=200):
    import torch
    from music_rule_guidance import music_rules
    N, T, wc = 64, 1024, 128
    x = torch.from_numpy(test_rolls(N, T)).cuda()
    q = music_rules.chord_quantise(x.clone())
    music_rules.register_chord_backend("native")
    try:
        kernel = timed(lambda: music_rules.chords_native(q, wc), iters, warmup=20)
        whole = timed(lambda: music_rules.get_chords(x), iters, warmup=20)
    finally:
        music_rules.register_chord_backend(None)
    read = N * 88 * T                          # bytes of the piano rows
    return {"shape": f"N{N}_T{T}_Wc{wc}", "rgm_rule_chords_call_us": round(kernel * 1e3, 2), "piano_rows_read_GBps": round(read / kernel / 1e6, 1),
            "get_chords_call_us": round(whole * 1e3, 2)}


def search_step(repeats):
    import torch
    from guided_diffusion.condition_functions import model_fn
    from guided_diffusion.dit import DiTRotary
    from guided_diffusion.gaussian_diffusion import PhiloxNoise
    from guided_diffusion.script_util import create_diffusion
    from music_rule_guidance import music_rules
    from music_rule_guidance.piano_roll_to_chord import piano_roll_to_chords_native
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
    nd = music_rules.note_density(torch.from_numpy(test_rolls(B, 8 * H)).cuda())
    rules = {"note_density": nd, "chord_progression": torch.tensor([[1, 4, 5, 1, 6, 2, 5, 1]] * B, dtype=torch.long, device="cuda")}
    guid = SimpleNamespace(schedule=True, t_start=750, t_end=0, interval=1, method="no_guidance")

    def step(with_chords):
        d = create_diffusion(learn_sigma=False, diffusion_steps=1000, noise_schedule="linear", timestep_respacing="", use_kl=False,
                             predict_xstart=False, rescale_timesteps=False, rescale_learned_sigmas=False)
        d.t_end = 0
        d.noise = PhiloxNoise(seed=99)
        r = rules if with_chords else {"note_density": nd}
        scg = dict(num_samples=N_CAND, **{k: 1. for k in r})

        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d.p_sample(mf, x, t, clip_denoised=False, model_kwargs={"y": y, "rule": r}, embed_model=vae, scale_factor=1.2465,
                       guidance_kwargs=guid, scg_kwargs=scg)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        for _ in range(2):
            run()                                       # warm-up: workspaces, the worker pool's start
        return round(min(run() for _ in range(repeats)), 2)

    out = {"shape": f"B{B}_n{N_CAND}_H{H}", "network": "XL-28 bf16x3_presplit, synthetic weights", "rules": list(rules)}
    try:
        out["no_chord_rule_ms"] = step(False)
        music_rules.register_chord_backend("native")
        out["device_analyser_ms"] = step(True)
        music_rules.register_chord_backend(piano_roll_to_chords_native, workers=4)
        out["host_analyser_pool4_ms"] = step(True)
    finally:
        music_rules.register_chord_backend(None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chords_time.json"))
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    from rgm import native as R
    torch.backends.cuda.matmul.allow_tf32 = False
    R.set_gemm_precision("bf16x3_presplit")
    out = {"scoring_alone": scoring_alone(), "search_step": search_step(a.repeats), "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
