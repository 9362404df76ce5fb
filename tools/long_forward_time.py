"""Long excerpts at a fixed token count: XL-28 eps-network forwards (bf16x3_presplit) at 4096 tokens per forward split as
(B, H) = (16, 128), (8, 256), (4, 512), (2, 1024) -- T = 2H = 256 .. 2048; every GEMM has the same shape at these points, so the
difference is the attention -- and the streaming attention kernel alone at those shapes (us per launch, TFLOP/s counting 4 N T^2 heads hd),
plus the fp32 streaming kernel at one shape.  Prints one JSON line.

    python tools/long_forward_time.py [--iters 20] [--attn-iters 200]
    python tools/long_forward_time.py --only 8x256     # that forward alone (under rocprofv3 --kernel-trace --stats)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rule-guided-music_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rgm import native as R, synth  # noqa: E402

SHAPES = ((16, 128), (8, 256), (4, 512), (2, 1024))
XL28 = dict(depth=28, hidden=1152, heads=16, patch=8, in_ch=4, out_ch=4, num_classes=3)


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


def forward_ms(B, H, iters):
    from guided_diffusion.dit import DiTRotary
    m = DiTRotary(input_size=[128, 16], patch_size=8, in_channels=4, hidden_size=1152, depth=28, num_heads=16, num_classes=3,
                  learn_sigma=False)
    m.load_state_dict(synth.dit_state_dict(1, final_std=0.3 / 1152 ** 0.5, device="cuda", **XL28))
    m = m.to("cuda").eval()
    g = torch.Generator(device="cuda").manual_seed(B)
    x = torch.randn(B, 4, H, 16, device="cuda", generator=g)
    t = torch.full((B,), 500, dtype=torch.long, device="cuda")
    y = torch.arange(B, device="cuda") % 3
    return timed(lambda: m(x, t, y), iters)


def attention_us(N, T, iters, heads=16, hd=72):
    from oracle import dit_np as odit
    cos, sin = odit.rotary_tables(synth.rotary_freqs(hd // 2), T)
    qkv = torch.randn(N * T, 3 * heads * hd, device="cuda") * 1.5
    o = torch.empty(N * T, heads * hd, device="cuda")
    cd, sd = torch.from_numpy(cos).cuda(), torch.from_numpy(sin).cuda()
    st = R.current_stream()
    prev = R.lib.rgm_set_attn_stream(1)
    try:
        ms = timed(lambda: R.check(R.lib.rgm_rotary_attention(R.ptr(qkv), R.ptr(o), R.ptr(cd), R.ptr(sd), N, T, heads, hd, hd // 4, st)),
                   iters)
    finally:
        R.lib.rgm_set_attn_stream(prev)
    us = ms * 1e3
    return us, 4.0 * N * T * T * heads * hd / (us * 1e-6) / 1e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--attn-iters", type=int, default=200)
    ap.add_argument("--only", default=None, metavar="BxH")
    a = ap.parse_args()
    torch.backends.cuda.matmul.allow_tf32 = False
    if a.only:
        B, H = (int(v) for v in a.only.split("x"))
        R.set_gemm_precision("bf16x3_presplit")
        print(json.dumps({"forward_ms": {f"B{B}_H{H}": round(forward_ms(B, H, a.iters), 3)}, "precision": "bf16x3_presplit"}))
        return
    out = {"tokens_per_forward": 4096, "precision": "bf16x3_presplit", "forward_ms": {}, "stream_attention": {}}
    R.set_gemm_precision("bf16x3_presplit")
    for B, H in SHAPES:
        out["forward_ms"][f"B{B}_H{H}"] = round(forward_ms(B, H, a.iters), 3)
        us, tf = attention_us(B, 2 * H, a.attn_iters)
        out["stream_attention"][f"N{B}_T{2 * H}"] = {"us": round(us, 2), "tflops": round(tf, 1)}
    base = out["forward_ms"]["B16_H128"]
    out["forward_ratio_vs_B16_H128"] = {k: round(v / base, 3) for k, v in out["forward_ms"].items()}
    R.set_gemm_precision("fp32")
    us, tf = attention_us(8, 512, a.attn_iters // 4)
    out["stream_attention_fp32"] = {"N8_T512": {"us": round(us, 2), "tflops": round(tf, 1)}}
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    np.random.seed(0)
    main()
