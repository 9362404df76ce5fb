"""What evaluation and inversion cost beside the forward: XL-28 (bf16x3_presplit), ms per step of calc_bpd_loop and of
ddim_reverse_sample_loop at (B, H) = (16, 128) and (8, 256) against the bare forward at the same shape IN THE SAME PROCESS (the boxes of
the pool differ by 4 %), the two kernels alone (us per launch; rgm_vb_terms' achieved bytes/s at N = 1, E = 262144 and N = 68, E = 8192),
a full 1000-step calc_bpd_loop at B = 16, and how far 20 ddim50 inversion steps followed by 20 deterministic DDIM steps return from the
source latent.  Prints one JSON line (kept as profiles/eval_time.json).

    python tools/eval_time.py [--steps 50] [--full-loop 1]
    python tools/eval_time.py --only bpd     # one short calc_bpd_loop alone (under rocprofv3 --kernel-trace --stats)
    python tools/eval_time.py --only kernels --shape 68x8192     # 200 launches of the two kernels at one shape (the same)"""
import argparse
import json
import os
import sys
import time
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rule-guided-music_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rgm import native as R, synth  # noqa: E402

XL28 = dict(depth=28, hidden=1152, heads=16, patch=8, in_ch=4, out_ch=4, num_classes=3)
SHAPES = ((16, 128), (8, 256))


def timed(fn, iters, warmup=3):
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


def network():
    from guided_diffusion.dit import DiTRotary
    m = DiTRotary(input_size=[128, 16], patch_size=8, in_channels=4, hidden_size=1152, depth=28, num_heads=16, num_classes=3,
                  learn_sigma=False)
    m.load_state_dict(synth.dit_state_dict(1, final_std=0.3 / 1152 ** 0.5, device="cuda", **XL28))
    return m.to("cuda").eval()


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


def kernels_alone(iters=200, shapes=((1, 262144), (68, 8192), (16, 8192), (8, 16384))):
    """us per CALL of the two kernels' Python wrappers (allocations and launches included: at these sizes the host side is what is
    measured -- the kernels' own times come from a rocprofv3 --kernel-trace --stats run of `--only kernels`), and the bytes/s that
    would correspond (4 arrays read, pred_xstart written: 20 B / element)"""
    d = diffusion("ddim50")
    out = {}
    for N, E in shapes:
        xs, xt, ep, nz = (torch.randn(N, E, device="cuda") * 0.5 for _ in range(4))
        t = torch.full((N,), 25, dtype=torch.long, device="cuda")
        us = timed(lambda: d._vb_terms(xs, xt, ep, nz, t, True), iters) * 1e3
        us_r = timed(lambda: d._ddim_reverse_step(xt, ep, t, True), iters) * 1e3
        out[f"N{N}_E{E}"] = {"vb_terms_call_us": round(us, 2), "vb_terms_call_GBps": round(20.0 * N * E / (us * 1e-6) / 1e9, 1),
                             "ddim_reverse_step_call_us": round(us_r, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--full-loop", type=int, default=1)
    ap.add_argument("--only", default=None, choices=["bpd", "invert", "kernels"])
    ap.add_argument("--shape", default="1x262144", metavar="NxE", help="--only kernels: the shape of the 200 launches")
    a = ap.parse_args()
    torch.backends.cuda.matmul.allow_tf32 = False
    R.set_gemm_precision("bf16x3_presplit")
    from guided_diffusion.condition_functions import model_fn
    if a.only == "kernels":
        N, E = (int(v) for v in a.shape.split("x"))
        print(json.dumps({"shape": a.shape, **kernels_alone(shapes=((N, E),))}))
        return
    m = network()
    mf = partial(model_fn, model=m, num_classes=3, class_cond=True, cfg=False, w=0.)
    if a.only:
        B, H = SHAPES[0]
        d = diffusion("ddim50" if a.only == "invert" else "8")
        x = torch.randn(B, 4, H, 16, device="cuda") * 0.5
        kw = {"y": torch.arange(B, device="cuda") % 3}
        fn = (lambda: d.calc_bpd_loop(mf, x, model_kwargs=kw)) if a.only == "bpd" else (lambda: d.ddim_reverse_sample_loop(mf, x, num_steps=9, model_kwargs=kw))
        fn()
        print(json.dumps({a.only + "_ms": round(wall_ms(fn), 3)}))
        return
    out = {"precision": "bf16x3_presplit", "steps": a.steps, "per_step_ms": {}}
    for B, H in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(B)
        x = torch.randn(B, 4, H, 16, device="cuda", generator=g) * 0.5
        t = torch.full((B,), 500, dtype=torch.long, device="cuda")
        y = torch.arange(B, device="cuda") % 3
        kw = {"y": y}
        fwd = timed(lambda: m(x, t, y), 20)
        d = diffusion(str(a.steps))
        d.calc_bpd_loop(mf, x, model_kwargs=kw)                                       # warm-up (tables, conditioning rows)
        bpd = wall_ms(lambda: d.calc_bpd_loop(mf, x, model_kwargs=kw)) / a.steps
        d.ddim_reverse_sample_loop(mf, x, model_kwargs=kw)
        inv = wall_ms(lambda: d.ddim_reverse_sample_loop(mf, x, model_kwargs=kw)) / (a.steps - 1)
        fwd2 = timed(lambda: m(x, t, y), 20)
        out["per_step_ms"][f"B{B}_H{H}"] = {"forward": round(min(fwd, fwd2), 3), "calc_bpd_loop": round(bpd, 3), "ddim_reverse_sample_loop": round(inv, 3),
                                            "bpd_minus_forward": round(bpd - min(fwd, fwd2), 3), "inversion_minus_forward": round(inv - min(fwd, fwd2), 3)}
    out["kernels"] = kernels_alone()
    if a.full_loop:
        B, H = SHAPES[0]
        x = torch.randn(B, 4, H, 16, device="cuda") * 0.5
        kw = {"y": torch.arange(B, device="cuda") % 3}
        d = diffusion("")
        res = {}
        s = wall_ms(lambda: res.update(d.calc_bpd_loop(mf, x, model_kwargs=kw))) / 1e3
        out["full_1000_step_bpd_B16"] = {"seconds": round(s, 2), "1000_x_forward_s": round(out["per_step_ms"]["B16_H128"]["forward"], 3),
                                         "total_bpd_mean": float(res["total_bpd"].mean())}
    # information: what the inversion preserves -- 20 ddim50 steps up, 20 deterministic DDIM steps down
    B, H = 4, 128
    d = diffusion("ddim50")
    x = torch.randn(B, 4, H, 16, device="cuda") * 0.5
    kw = {"y": torch.arange(B, device="cuda") % 3}
    lat = d.ddim_reverse_sample_loop(mf, x, num_steps=21, clip_denoised=False, model_kwargs=kw)
    back = d.ddim_sample_loop(mf, x.shape, noise=lat, clip_denoised=False, model_kwargs=kw, device="cuda", eta=0.0,
                              edit_kwargs={"noise_level": 21, "gt": x, "mask": torch.zeros_like(x), "l_start": 0, "l_end": H})
    diff = (back - x).abs()
    out["ddim50_invert20_then_sample20"] = {"max_abs": float(diff.max()), "mean_abs": float(diff.mean()), "source_abs_mean": float(x.abs().mean())}
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    np.random.seed(0)
    main()
