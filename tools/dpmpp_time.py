"""What the DPM-Solver++(2M) sampler costs: the step kernel next to rgm_ddim_step (us per call of the Python wrapper, host side
included, at (N, E) = (16, 8192)) and whole chains of XL-28 (bf16x3_presplit) at (B, H) = (16, 128) IN ONE PROCESS (the boxes of the
pool differ by a few per cent): "logsnr20" 2M (eta 0 and 1) against "ddim50" and "ddim100" (eta 1).  The figures are reported, not
asserted; the expectation is that chain time follows the number of steps.  Writes profiles/dpmpp_time.json and prints it as one line.

    python tools/dpmpp_time.py [--out profiles/dpmpp_time.json] [--repeats 2]"""
import argparse
import json
import os
import sys
import time
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rule-guided-music_amd")]

import torch  # noqa: E402

from rgm import native as R, synth  # noqa: E402

XL28 = dict(depth=28, hidden=1152, heads=16, patch=8, in_ch=4, out_ch=4, num_classes=3)
B, H = 16, 128


def timed(fn, iters, warmup=5):
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


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def diffusion(rs):
    from guided_diffusion.script_util import create_diffusion
    return create_diffusion(learn_sigma=False, diffusion_steps=1000, noise_schedule="linear", timestep_respacing=rs, use_kl=False,
                            predict_xstart=False, rescale_timesteps=False, rescale_learned_sigmas=False)


def network():
    from guided_diffusion.dit import DiTRotary
    m = DiTRotary(input_size=[H, 16], patch_size=8, in_channels=4, hidden_size=1152, depth=28, num_heads=16, num_classes=3,
                  learn_sigma=False)
    m.load_state_dict(synth.dit_state_dict(1, final_std=0.3 / 1152 ** 0.5, device="cuda", **XL28))
    return m.to("cuda").eval()


def step_kernels(iters=200):
    d = diffusion("logsnr20")
    d.t_end = 0
    N, E = B, 4 * H * 16
    x, eps, prev, z = (torch.randn(N, E, device="cuda") * 0.5 for _ in range(4))
    t = torch.full((N,), 10, dtype=torch.long, device="cuda")
    return {"shape": f"N{N}_E{E}",
            "ddim_step_call_us": round(timed(lambda: d._step("ddim", x, eps, None, z, t, False, eta=1.0), iters) * 1e3, 2),
            "dpmpp_step_sde_2m_call_us": round(timed(lambda: d._dpm_step(x, eps, None, prev, z, t, False, order=2, eta=1.0), iters) * 1e3, 2),
            "dpmpp_step_ode_2m_call_us": round(timed(lambda: d._dpm_step(x, eps, None, prev, None, t, False, order=2, eta=0.0), iters) * 1e3, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dpmpp_time.json"))
    ap.add_argument("--repeats", type=int, default=2)
    a = ap.parse_args()
    torch.backends.cuda.matmul.allow_tf32 = False
    R.set_gemm_precision("bf16x3_presplit")
    from guided_diffusion.condition_functions import model_fn
    m = network()
    mf = partial(model_fn, model=m, num_classes=3, class_cond=True, cfg=False, w=0.)
    kw = {"y": torch.arange(B, device="cuda") % 3}
    shape = (B, 4, H, 16)
    x = torch.randn(shape, device="cuda") * 0.5
    t = torch.full((B,), 500, dtype=torch.long, device="cuda")
    out = {"precision": "bf16x3_presplit", "shape": f"B{B}_H{H}", "step_kernels": step_kernels(), "chains": {}}
    fwd = timed(lambda: m(x, t, kw["y"]), 20)
    runs = [("logsnr20_dpmpp_2m_ode", "logsnr20", lambda d: d.dpmpp_sample_loop(mf, shape, clip_denoised=False, order=2, eta=0.0, model_kwargs=kw, device="cuda")),
            ("logsnr20_dpmpp_2m_sde", "logsnr20", lambda d: d.dpmpp_sample_loop(mf, shape, clip_denoised=False, order=2, eta=1.0, model_kwargs=kw, device="cuda")),
            ("ddim50_eta1", "ddim50", lambda d: d.ddim_sample_loop(mf, shape, clip_denoised=False, eta=1.0, model_kwargs=kw, device="cuda")),
            ("ddim100_eta1", "ddim100", lambda d: d.ddim_sample_loop(mf, shape, clip_denoised=False, eta=1.0, model_kwargs=kw, device="cuda"))]
    for name, rs, fn in runs:
        d = diffusion(rs)
        fn(d)                                                   # warm-up: tables, conditioning rows, workspaces
        ms = min(wall_ms(lambda: fn(d)) for _ in range(a.repeats))
        out["chains"][name] = {"steps": d.num_timesteps, "chain_ms": round(ms, 2), "ms_per_step": round(ms / d.num_timesteps, 3)}
    fwd = min(fwd, timed(lambda: m(x, t, kw["y"]), 20))
    out["forward_ms"] = round(fwd, 3)
    ref = out["chains"]["logsnr20_dpmpp_2m_sde"]["chain_ms"]
    out["chain_time_over_logsnr20_sde"] = {k: round(v["chain_ms"] / ref, 3) for k, v in out["chains"].items()}
    out["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
