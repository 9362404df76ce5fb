#!/usr/bin/env python3
"""Generate the long-excerpt fixtures (DiTRotary beyond 256 tokens) under tests/golden/ by IMPORTING the reference.

Runs only in the build container, like make_golden.py, whose builders (reference modules through ref_shims, rgm.synth weights,
the teacher-forced noise queue) it reuses:  `python tests/golden/make_golden_long.py`.

    long_dit_xl2.npz    XL-2 eps-network forward at H = 136 (B 2), 256 (B 2), 512 (B 1): T = 272, 512, 1024 tokens
    long_dit_xl28.npz   XL-28 forward at H = 256, B = 2
    long_ddim.npz       one teacher-forced DDIM step (ddim50 chain, eta = 1, injected noise) at H = 256, B = 2, XL-2
    long_dit_xl2_edge.npz  XL-2 forward at H = 1040 (B 2; T = 2080: partial last query tile and key block) and H = 4096 (B 1;
                        T = 8192, the streaming kernel's ceiling).  x is NOT stored: x{H} = RandomState(x{H}_seed).randn(B, 4, H, 16);
                        t{H}, y{H} are, with the reference output at the latent rows rows{H} = edge_rows(H) only (out{H}: (B, 4, R, 16))

Seeds are pinned by name in LONG_SEEDS and stored as ONE-ELEMENT arrays (make_golden.py's FIXTURE_SEEDS check reads 0-d `*seed`
arrays only); tests/test_long_fixtures.py holds the fixtures to this table."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (installs ref_shims, imports the reference)

F32 = np.float32
LONG_SEEDS = {
    "long_dit_xl2": {"seed": 1, "x_seed": 700},
    "long_dit_xl28": {"seed": 1, "x_seed": 701},
    "long_ddim": {"seed": 11, "x_seed": 702},
    "long_dit_xl2_edge": {"seed": 1, "x1040_seed": 704, "x4096_seed": 705},
}
EDGE_SHAPES = ((1040, 2), (4096, 1))      # (H, B) of long_dit_xl2_edge
LIMIT = 1024 * 1024


def save(name, **arrs):
    stored = {k: int(np.asarray(v).reshape(-1)[0]) for k, v in arrs.items() if k.endswith("seed")}
    assert stored == LONG_SEEDS[name], f"{name}: stored seeds {stored} != LONG_SEEDS[{name!r}]"
    p = os.path.join(HERE, name + ".npz")
    np.savez_compressed(p, **arrs)
    assert os.path.getsize(p) < LIMIT, f"{p}: {os.path.getsize(p)} bytes"
    print(f"  wrote {p} ({os.path.getsize(p) / 1024:.0f} KiB)")


def seeds(name):
    return {k: np.array([v], dtype=np.int64) for k, v in LONG_SEEDS[name].items()}


def g_forward(name, arch, shapes):
    print(f"[{name}]")
    s = LONG_SEEDS[name]
    m, sd = mg.ref_dit(arch, s["seed"])
    rng = np.random.RandomState(s["x_seed"])
    out = {}
    for H, B in shapes:
        x = rng.randn(B, 4, H, 16).astype(F32)
        t = rng.randint(0, 1000, size=B).astype(np.int64)
        y = rng.randint(0, 4, size=B).astype(np.int64)                # 3 == the null label
        ref = m(torch.from_numpy(x), torch.from_numpy(t), torch.from_numpy(y)).numpy()
        if arch["depth"] <= 2:
            ora = mg.odit.dit_forward(sd, x, t, y, depth=arch["depth"], heads=arch["heads"])
            mg.err(f"forward H={H} (T={2 * H})", ora, ref)
        out.update({f"x{H}": x, f"t{H}": t, f"y{H}": y, f"out{H}": ref})
    save(name, **seeds(name), **out)


def edge_rows(H):
    """latent rows stored of an H-row output: the first and last 64, every 16th in between"""
    return np.unique(np.concatenate((np.arange(64), np.arange(64, H - 64, 16), np.arange(H - 64, H))))


def edge_input(name, H, B):
    return np.random.RandomState(LONG_SEEDS[name][f"x{H}_seed"]).randn(B, 4, H, 16).astype(F32)


def g_edge():
    name = "long_dit_xl2_edge"
    print(f"[{name}]")
    m, sd = mg.ref_dit(mg.XL2, LONG_SEEDS[name]["seed"])
    out = {}
    for H, B in EDGE_SHAPES:
        x = edge_input(name, H, B)
        t = np.array([917, 3][:B], dtype=np.int64)
        y = np.array([2, 3][:B], dtype=np.int64)                      # 3 == the null label
        with torch.no_grad():
            ref = m(torch.from_numpy(x), torch.from_numpy(t), torch.from_numpy(y)).numpy()
        rows = edge_rows(H)
        ora = mg.odit.dit_forward(sd, x, t, y, depth=2, heads=16)
        mg.err(f"forward H={H} (T={2 * H})", ora, ref)
        out.update({f"t{H}": t, f"y{H}": y, f"rows{H}": rows.astype(np.int64), f"out{H}": np.ascontiguousarray(ref[:, :, rows])})
        del ref, ora
    save(name, **seeds(name), **out)


def g_ddim():
    name = "long_ddim"
    print(f"[{name}]")
    s = LONG_SEEDS[name]
    m, sd = mg.ref_dit(mg.XL2, s["seed"])
    rng = np.random.RandomState(s["x_seed"])
    B, H = 2, 256
    x = rng.randn(B, 4, H, 16).astype(F32)
    y = np.array([1, 2], dtype=np.int64)
    t = np.full((B,), 30, dtype=np.int64)
    nz = rng.randn(B, 4, H, 16).astype(F32)
    d = mg.make_diffusion("ddim50")
    d.t_end = 0
    mg.NQ.push(nz)
    r = d.ddim_sample(mg.ref_model_fn(m, 3, True), torch.from_numpy(x), torch.from_numpy(t), clip_denoised=False, eta=1.0,
                      model_kwargs={"y": torch.from_numpy(y)})
    S = mg.odf.Schedule(1000, "linear", "ddim50")
    o = mg.odf.ddim_sample(S, mg.np_model(sd, mg.XL2), x, t, nz, eta=1.0, model_kwargs={"y": y})
    mg.err("ddim sample", o["sample"], r["sample"].numpy())
    save(name, **seeds(name), x=x, y=y, t=t, noise=nz, sample=r["sample"].numpy(), pred_xstart=r["pred_xstart"].numpy())


if __name__ == "__main__":
    which = set(sys.argv[1:]) or {"xl2", "xl28", "ddim", "edge"}
    torch.set_num_threads(8)
    if "xl2" in which:
        g_forward("long_dit_xl2", mg.XL2, [(136, 2), (256, 2), (512, 1)])
    if "xl28" in which:
        g_forward("long_dit_xl28", mg.XL28, [(256, 2)])
    if "ddim" in which:
        g_ddim()
    if "edge" in which:
        g_edge()
