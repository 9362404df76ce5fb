#!/usr/bin/env python3
"""Is DiTRotaryClassifier.value_and_grad (depth 12, hidden 384, H = 256: 513 tokens, the long backward) a function of its inputs alone?
(1) the workspace pre-filled with different bytes, (2) repeats on one fill.  Names the buffers of the gradient workspace (gplan in
csrc/dit.hip) whose bytes differ from the reference run.  usage: race_cls_grad.py [fp32|bf16x3|bf16x3_presplit] [repeats]
Measured with it (docs/rounds/gemm_inputs.md): bf16x3_presplit, 3 of 200 calls differ -- in the backward's buffers only."""
import os, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, ROOT + "/rule-guided-music_amd", ROOT + "/tests"):
    sys.path.insert(0, p)
import numpy as np, torch
from conftest import load_golden
from gpu_util import dev, load_module
from rgm import native as R, synth
from guided_diffusion import dit
from guided_diffusion.dit import DiTRotaryClassifier

PREC = sys.argv[1] if len(sys.argv) > 1 else "bf16x3_presplit"
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 200
def say(*a):
    print(*a, flush=True)

R.set_gemm_precision(PREC)
dit.set_long_backward(True)
arch = dict(depth=12, hidden=384, heads=6, patch=8, in_ch=4, classifier=True, cls_classes=16)
g = load_golden("guidedlong_cls")
tag, H, B = "s8", 256, 2
m = DiTRotaryClassifier(input_size=[128, 16], patch_size=8, in_channels=4, hidden_size=384, depth=12, num_heads=6, num_classes=16)
m = load_module(m, synth.dit_state_dict(int(g[f"{tag}.seed"][0]), **arch))
x = dev(np.random.RandomState(int(g[f"{tag}.x{H}_seed"][0])).randn(B, 4, H, 16).astype(np.float32))
t, rule = dev(g[f"{tag}.t{H}"]), dev(g[f"{tag}.rule{H}"])

def layout():
    N, D, dep, heads = B, 384, 12, 6
    T0 = H * 16 // 8; T = T0 + 1; M0 = N * T0; M = N * T; L = 6 * dep * D; Kp = 32; Rr = N
    segs, off = [], 0
    def take(name, floats, ld=None):
        nonlocal off
        segs.append((name, off, floats * 4, ld)); off += (floats * 4 + 255) // 256 * 256
    take("tok_in", M0 * 32, 32); take("zpre", M0 * 256, 256); take("h1", M0 * 256, 256); take("temb", N * 256, 256)
    take("c1", N * D, D); take("c", N * D, D); take("cs", N * D, D); take("mod", N * L, L)
    take("xs", (dep + 1) * M * D, D); take("x1s", dep * M * D, D); take("qkvs", dep * M * 3 * D, 3 * D); take("aos", dep * M * D, D)
    take("pres", dep * M * 4 * D, 4 * D); take("lses", dep * N * heads * T, T)
    take("xm", M * D, D); take("hid", M * 4 * D, 4 * D); take("dx", M * D, D); take("dx1", M * D, D); take("t1", M * D, D)
    take("dbig", M * 4 * D, 4 * D); take("dqkv", M * 3 * D, 3 * D); take("dsmall", M * D, D)
    take("pool", Rr * D, D); take("pooln", Rr * D, D); take("z1pre", Rr * 96, 96); take("z1", Rr * 96, 96); take("logits", Rr * 16, 16)
    take("dl", Rr * Kp, Kp); take("dz1", Rr * 96, 96); take("dpooln", Rr * D, D); take("dpool", Rr * D, D)
    take("dz", M0 * 256, 256); take("dtin", M0 * 32, 32)
    return segs, off, M

SEGS, END, M = layout()

def where(a, b):
    """segments of the workspace in which byte tensors a and b differ"""
    res = []
    for name, off, nbytes, ld in SEGS + [("sk", END, a.numel() - END, None)]:
        if nbytes <= 0:
            continue
        d = (a[off:off + nbytes] != b[off:off + nbytes])
        n = int(d.sum())
        if n:
            idx = torch.nonzero(d)[:, 0] // 4
            first, last = int(idx[0]), int(idx[-1])
            if ld:
                res.append(f"{name}: {n} bytes, elems {first}..{last} = row {first // ld} col {first % ld} .. row {last // ld} col {last % ld}"
                           f" (M={M}: block {first // ld // M}, row-in-block {first // ld % M})")
            else:
                res.append(f"{name}: {n} bytes, elems {first}..{last}")
    return res

def run(fill=None):
    if fill is not None and m._ws is not None:
        if fill == "rand":
            m._ws.copy_(torch.randint(0, 256, (m._ws.numel(),), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)))
        else:
            m._ws.fill_(fill)
    lg, gr = m.value_and_grad(x, t, rule, "mse", 10.0)
    torch.cuda.synchronize()
    return lg.clone(), gr.clone(), m._ws.clone()

lg0, gr0, ws0 = run()                      # first call: workspace as torch.empty left it
say(f"{PREC}: workspace {ws0.numel()} bytes, plan without scratch {END}; finite grad {bool(torch.isfinite(gr0).all())}")
lgz, grz, wsz = run(0)
say("first call (torch.empty workspace) vs zero-filled: grad equal", torch.equal(gr0, grz), "logits equal", torch.equal(lg0, lgz))
for fill in (0xFF, 0x7F, 0xAB, "rand"):
    lg, gr, ws = run(fill)
    eq = torch.equal(gr.view(torch.int32), grz.view(torch.int32))
    say(f"fill {fill}: grad equal {eq}, logits equal {torch.equal(lg, lgz)}, finite {bool(torch.isfinite(gr).all())},"
        f" max |d| {float((gr - grz).abs().max()):.3e}")
    # written regions must not depend on the fill: compare only where this run and the zero run both wrote, i.e. where ws != fill pattern
    if not eq:
        if fill != "rand":
            wrote = ws != fill
            a, b = torch.where(wrote, ws, torch.zeros_like(ws)), torch.where(wrote, wsz, torch.zeros_like(ws))
            for line in where(a, b)[:40]:
                say("    ", line)
lgr, grr, wsr = run(0)
bad = 0
for rep in range(REPS):
    lg, gr, ws = run(0)
    if not torch.equal(ws, wsr):
        bad += 1
        say(f"rep {rep}: workspace differs; grad equal {torch.equal(gr, grr)} max |d grad| {float((gr - grr).abs().max()):.3e}")
        for line in where(ws, wsr)[:40]:
            say("    ", line)
        if bad >= 3:
            break
say(f"{REPS} repeats on a zero-filled workspace: {bad} differed")
# repeats without refilling: the workspace holds the previous call's values (what the test's second call sees)
bad = 0
for rep in range(REPS):
    lg, gr, ws = run()
    if not torch.equal(gr, grr):
        bad += 1
        say(f"rep {rep} (no refill): grad differs, max |d| {float((gr - grr).abs().max()):.3e}")
        for line in where(ws, wsr)[:40]:
            say("    ", line)
        if bad >= 3:
            break
say(f"{REPS} repeats without refill: {bad} differed")
