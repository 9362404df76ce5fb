"""Guided long excerpts at a fixed token count (4096 tokens per step), device-event timing, warm shapes, one process:

  * the attention backward alone at XL width (16 heads, hd 72), N x T = 4096: the streaming dq + dkv pair (csrc/attention_bwd_stream.hip)
    at T = 256 (forced), 512, 1024, 2048 and the resident pair at T = 256, in both arithmetics.  us per launch of the PAIR and the
    ALGORITHMIC rate 10 N heads T^2 hd FLOP / time (five T x T x hd contractions; the two-kernel form executes seven -- S and dP are
    formed in both kernels -- i.e. 14 N heads T^2 hd, reported as `tflops_executed`);
  * one classifier-guided DDPM step (XL-28 + DiTRotary-S/8-cls, grad_nn_zt_mse x 10, "250" chain) and one DPS-nn step (nn_z0_mse_dummy
    through the same classifier and the XL-28 VJP) at (B, H) = (16, 128) -- the resident backward -- and (8, 256), (4, 512), (2, 1024):
    equal token counts, so the ratio to the (16, 128) step is the cost of length.

Prints one JSON line (profiles/guided_long_time.json).

    python tools/guided_long_time.py [--iters 10] [--attn-iters 100]
    python tools/guided_long_time.py --only-attn 4x1024     # that backward alone (under rocprofv3 --kernel-trace --stats)"""
import argparse
import json
import os
import sys
from functools import partial
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rule-guided-music_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rgm import native as R, synth  # noqa: E402

SHAPES = ((16, 128), (8, 256), (4, 512), (2, 1024))
XL28 = dict(depth=28, hidden=1152, heads=16, patch=8, in_ch=4, out_ch=4, num_classes=3)
CLS = dict(depth=12, hidden=384, heads=6, patch=8, in_ch=4, classifier=True, cls_classes=16)


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


def attention_bwd_us(N, T, iters, stream, heads=16, hd=72):
    from oracle import dit_np as odit
    cos, sin = odit.rotary_tables(synth.rotary_freqs(hd // 2), T)
    D = heads * hd
    qkv = torch.randn(N * T, 3 * D, device="cuda")
    d_o = torch.randn(N * T, D, device="cuda")
    o = torch.empty(N * T, D, device="cuda")
    lse = torch.empty(N * heads * T, device="cuda")
    out = torch.empty(N * T, 3 * D, device="cuda")
    cd, sd = torch.from_numpy(cos).cuda(), torch.from_numpy(sin).cuda()
    st = R.current_stream()
    R.check(R.lib.rgm_rotary_attention_lse(R.ptr(qkv), R.ptr(o), R.ptr(lse), R.ptr(cd), R.ptr(sd), N, T, heads, hd, hd // 4, st))
    prev = R.lib.rgm_set_attn_bwd_stream(1 if stream else 0)
    try:
        ms = timed(lambda: R.check(R.lib.rgm_rotary_attention_bwd(R.ptr(qkv), R.ptr(o), R.ptr(d_o), R.ptr(lse), R.ptr(out), R.ptr(cd),
                                                                  R.ptr(sd), N, T, heads, hd, hd // 4, st)), iters)
    finally:
        R.lib.rgm_set_attn_bwd_stream(prev)
    us = ms * 1e3
    alg = 10.0 * N * heads * T * T * hd / (us * 1e-6) / 1e12
    return {"us": round(us, 2), "tflops_algorithmic": round(alg, 1), "tflops_executed": round(alg * 1.4, 1)}


def models():
    from guided_diffusion.dit import DiTRotary, DiTRotaryClassifier
    m = DiTRotary(input_size=[128, 16], patch_size=8, in_channels=4, hidden_size=1152, depth=28, num_heads=16, num_classes=3,
                  learn_sigma=False)
    m.load_state_dict(synth.dit_state_dict(1, final_std=0.3 / 1152 ** 0.5, device="cuda", **XL28))
    c = DiTRotaryClassifier(input_size=[128, 16], patch_size=8, in_channels=4, hidden_size=384, depth=12, num_heads=6, num_classes=16)
    c.load_state_dict({k: torch.from_numpy(v) for k, v in synth.dit_state_dict(3, **CLS).items()})
    return m.to("cuda").eval(), c.to("cuda").eval()


def step_ms(m, c, B, H, kind, iters):
    from guided_diffusion.condition_functions import composite_nn_zt, model_fn
    from guided_diffusion.script_util import create_diffusion
    d = create_diffusion(learn_sigma=False, diffusion_steps=1000, noise_schedule="linear", timestep_respacing="250", use_kl=False,
                         predict_xstart=False, rescale_timesteps=False, rescale_learned_sigmas=False)
    d.t_end = 0
    mf = partial(model_fn, model=m, num_classes=3, class_cond=True, cfg=False, w=0.)
    g = torch.Generator(device="cuda").manual_seed(B)
    x = torch.randn(B, 4, H, 16, device="cuda", generator=g)
    t = torch.full((B,), 120, dtype=torch.long, device="cuda")
    kw = {"y": torch.arange(B, device="cuda") % 3, "rule": {"note_density": torch.rand(B, 16, device="cuda", generator=g) * 4}}
    if kind == "cls":
        cond = partial(composite_nn_zt, fns=["grad_nn_zt_mse"], classifier_scales=[10.], classifiers=[c], rule_names=["note_density"])
        gk = SimpleNamespace(schedule=False, method="classifier_guidance")
    else:
        cond = partial(composite_nn_zt, fns=["nn_z0_mse_dummy"], classifier_scales=[1.], classifiers=[c], rule_names=["note_density"])
        gk = SimpleNamespace(schedule=False, method="dps", step_size=1.5, nn=True, vae=False)
    return timed(lambda: d.p_sample(mf, x, t, clip_denoised=False, cond_fn=cond, model_kwargs=kw, guidance_kwargs=gk), iters, warmup=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--attn-iters", type=int, default=100)
    ap.add_argument("--only-attn", default=None, metavar="NxT")
    a = ap.parse_args()
    from guided_diffusion.dit import set_long_backward
    set_long_backward(True)
    if a.only_attn:
        N, T = (int(v) for v in a.only_attn.split("x"))
        R.set_gemm_precision("bf16x3_presplit")
        print(json.dumps({"attention_bwd": {f"N{N}_T{T}": attention_bwd_us(N, T, a.attn_iters, stream=True)}, "precision": "bf16x3_presplit"}))
        return
    out = {"tokens": 4096, "heads": 16, "head_dim": 72, "attention_bwd_stream": {}, "attention_bwd_resident": {}}
    for prec in ("bf16x3_presplit", "fp32"):
        R.set_gemm_precision(prec)
        it = a.attn_iters if prec != "fp32" else max(a.attn_iters // 4, 5)
        out["attention_bwd_stream"][prec] = {f"N{4096 // T}_T{T}": attention_bwd_us(4096 // T, T, it, stream=True) for T in (256, 512, 1024, 2048)}
        out["attention_bwd_resident"][prec] = {"N16_T256": attention_bwd_us(16, 256, it, stream=False)}
    R.set_gemm_precision("bf16x3_presplit")
    m, c = models()
    out["step_precision"] = "bf16x3_presplit"
    for kind in ("cls", "dps"):
        ms = {f"B{B}_H{H}": round(step_ms(m, c, B, H, kind, a.iters), 3) for B, H in SHAPES}
        out[f"{kind}_step_ms"] = ms
        out[f"{kind}_step_ratio_vs_B16_H128"] = {k: round(v / ms["B16_H128"], 3) for k, v in ms.items()}
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    np.random.seed(0)
    main()
