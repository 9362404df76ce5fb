"""What particle rule guidance costs: rgm_particle_resample at (n, B) = (16, 4), (64, 16), (1024, 64) and rgm_gather_rows of the same
row counts at E = 8192 (HIP events around the launch alone, warm-up, the minimum of 5 rounds), and ONE particle step against ONE SCG
step IN ONE PROCESS (the boxes of the pool differ by a few per cent) at C4's size: XL-28, B = 4, n = 16, note_density through the VAE
decoder, bf16x3_presplit, on a "ddim50" chain at eta = 1.  A step's time is the difference of a 10-step and a 5-step chain over 5, so
that what a chain pays once (the first draw, the particle loop's final weighting) drops out.  The figures are reported, not asserted.
Writes profiles/particles_time.json and prints it as one line.

    python tools/particles_time.py [--out profiles/particles_time.json] [--repeats 3]"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from functools import partial
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rule-guided-music_amd")]

import torch  # noqa: E402

from rgm import native as R, synth  # noqa: E402

XL28 = dict(depth=28, hidden=1152, heads=16, patch=8, in_ch=4, out_ch=4, num_classes=3)
B, N_PART, H, E = 4, 16, 128, 8192


def launch_us(fn, iters=50, rounds=5, warmup=10):
    """microseconds per launch: events around `iters` back-to-back launches, the minimum of `rounds`"""
    for _ in range(warmup):
        fn()
    best = float("inf")
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / iters * 1e3)
    return round(best, 2)


def kernels():
    out = {}
    for n, b in ((16, 4), (64, 16), (1024, 64)):
        g = torch.Generator(device="cuda").manual_seed(n)
        reward = torch.randn(n * b, device="cuda", generator=g)
        logw = torch.zeros(n * b, dtype=torch.float64, device="cuda")
        rp = torch.zeros(n * b, device="cuda")
        anc = torch.empty(n * b, dtype=torch.int32, device="cuda")
        ess, flag = torch.empty(b, dtype=torch.float64, device="cuda"), torch.empty(b, dtype=torch.int32, device="cuda")
        st = R.current_stream()

        def resample(frac):
            R.check(R.lib.rgm_particle_resample(R.ptr(reward), R.ptr(logw), R.ptr(rp), 1.0, frac, None, C.c_uint64(1), C.c_uint64(0), R.ptr(anc),
                                                R.ptr(ess), R.ptr(flag), n, b, st))
        src = torch.randn(n * b, E, device="cuda", generator=g)
        dst = torch.empty_like(src)
        resample(2.0)
        out[f"n{n}_B{b}"] = {"resample_always_us": launch_us(lambda: resample(2.0)), "resample_never_us": launch_us(lambda: resample(0.0)),
                             "gather_rows_E8192_us": launch_us(lambda: R.check(R.lib.rgm_gather_rows(R.ptr(src), R.ptr(dst), R.ptr(anc), n, b, E, st))),
                             "gather_bytes_moved": 2 * n * b * E * 4}
    return out


def diffusion(rs):
    from guided_diffusion.script_util import create_diffusion
    return create_diffusion(learn_sigma=False, diffusion_steps=1000, noise_schedule="linear", timestep_respacing=rs, use_kl=False,
                            predict_xstart=False, rescale_timesteps=False, rescale_learned_sigmas=False)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def steps(repeats):
    from guided_diffusion.condition_functions import model_fn
    from guided_diffusion.dit import DiTRotary
    from taming.models.klvae_pedal import AutoencoderKL
    m = DiTRotary(input_size=[H, 16], patch_size=8, in_channels=4, hidden_size=1152, depth=28, num_heads=16, num_classes=3, learn_sigma=False)
    m.load_state_dict(synth.dit_state_dict(1, final_std=0.3 / 1152 ** 0.5, device="cuda", **XL28))
    m = m.to("cuda").eval()
    vae = AutoencoderKL()
    vae.load_state_dict(synth.vae_state_dict(2, device="cuda", encoder=True))
    vae = vae.to("cuda").eval()
    mf = partial(model_fn, model=m, num_classes=3, class_cond=True, cfg=False, w=0.)
    mk = {"y": torch.ones(B, dtype=torch.int, device="cuda"), "rule": {"note_density": torch.tensor([3.] * 16, device="cuda").repeat(B, 1)}}
    shape = (B, 4, H, 16)
    d = diffusion("ddim50")
    common = dict(clip_denoised=False, model_kwargs=mk, embed_model=vae, scale_factor=1.2465, device="cuda")
    gk = SimpleNamespace(method="no_guidance", schedule=False)

    def scg(t_end):
        return d.ddim_sample_loop(mf, shape, eta=1.0, t_end=t_end, guidance_kwargs=gk, scg_kwargs={"num_samples": N_PART, "note_density": 1.}, **common)

    def particles(t_end):
        return d.particle_sample_loop(mf, shape, N_PART, sampler="ddim", t_end=t_end, particle_kwargs={"note_density": 1.}, **common)
    out = {}
    for name, fn in (("scg", scg), ("particles", particles)):
        fn(45)                                                       # warm-up: tables, conditioning rows, workspaces
        t5 = min(wall_ms(lambda: fn(45)) for _ in range(repeats))
        t10 = min(wall_ms(lambda: fn(40)) for _ in range(repeats))
        out[name] = {"chain_5_steps_ms": round(t5, 2), "chain_10_steps_ms": round(t10, 2), "ms_per_step": round((t10 - t5) / 5, 3)}
    out["particle_step_over_scg_step"] = round(out["particles"]["ms_per_step"] / out["scg"]["ms_per_step"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "particles_time.json"))
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    torch.backends.cuda.matmul.allow_tf32 = False
    R.set_gemm_precision("bf16x3_presplit")
    out = {"precision": "bf16x3_presplit", "kernels": kernels(), "step_at_c4": dict(shape=f"XL28_B{B}_n{N_PART}_H{H}", chain="ddim50 eta 1",
                                                                                  **steps(a.repeats))}
    out["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
