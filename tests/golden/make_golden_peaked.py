#!/usr/bin/env python3
"""Generate the peaked-softmax model fixture under tests/golden/ by IMPORTING the reference:  `python tests/golden/make_golden_peaked.py`.

Runs only in the build container, like make_golden.py / make_golden_long.py / make_golden_guided_long.py, whose builders it reuses.

Every other model-level fixture runs rgm.synth weights, under which the scaled attention scores stay below 6 and no key gets more than
0.15 of a row: a nearly flat softmax.  Here the q and k rows of every attn.qkv.weight / .bias are multiplied by one factor QK_GAIN
(tests/attn_cases.peak_qk), chosen so that max |score| over the blocks lies in [30, 60] -- asserted below with the oracle -- which is
where a trained DiT lives.

    peaked.npz (+ .part2.npz, ..., joined by conftest.load_golden)
        xl2.*   XL-2 eps and th.autograd.grad((m(x, t, y) * c).sum(), x) at H = 128 (T = 256) and H = 256 (T = 512), B = 1
        cls.*   depth-2 DiTRotary-S/8-cls logits and grad_nn_zt_mse (scale 10) at H = 128 (T = 257) and H = 256 (T = 513), B = 2
    each from the reference in float32 (`...32`) and again with the reference module in float64 (`...64`).  The reference's own
    float32-against-float64 error must stay within a quarter of the tolerances the GPU tests hold the kernels to (asserted below).

No input tensor is stored: x and the cotangent c are np.random.RandomState(seed).randn(shape) of seeds pinned by name in PEAKED_SEEDS and
stored as one-element arrays, the gain likewise as `qk_gain`; tests/test_peaked_fixtures.py holds the fixture to this table."""
import glob
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (installs ref_shims, imports the reference)
import attn_cases  # noqa: E402  (tests/attn_cases.py: peak_qk, model_max_scores)

F32 = np.float32
PEAKED_SEEDS = {"peaked": {"xl2.seed": 1, "cls.seed": 4, "xl2.x128_seed": 840, "xl2.x256_seed": 841, "cls.x128_seed": 842, "cls.x256_seed": 843}}
QK_GAIN = 2.8
SCORE_RANGE = (30.0, 60.0)
TOL, GRAD_TOL = 2e-4, 5e-4                       # tests/test_gpu_dit.py: outputs, gradients
LIMIT = 1024 * 1024
PART_BYTES = 900 * 1024


def randn(seed, *shape):
    return np.random.RandomState(seed).randn(*shape).astype(F32)


def save(name, **arrs):
    stored = {k: int(np.asarray(v).reshape(-1)[0]) for k, v in arrs.items() if k.endswith("seed")}
    assert stored == PEAKED_SEEDS[name], f"{name}: stored seeds {stored} != PEAKED_SEEDS[{name!r}]"
    for old in glob.glob(os.path.join(HERE, name + ".part*.npz")):
        os.remove(old)
    parts, size = [{k: v for k, v in arrs.items() if k.endswith("seed") or k == "qk_gain"}], 0
    for k, v in arrs.items():
        if k in parts[0]:
            continue
        n = np.asarray(v).nbytes
        if size + n > PART_BYTES and size > 0:
            parts.append({})
            size = 0
        parts[-1][k] = v
        size += n
    for i, part in enumerate(parts):
        p = os.path.join(HERE, name + (".npz" if i == 0 else f".part{i + 1}.npz"))
        np.savez_compressed(p, **part)
        assert os.path.getsize(p) < LIMIT, f"{p}: {os.path.getsize(p)} bytes"
        print(f"  wrote {p} ({os.path.getsize(p) / 1024:.0f} KiB)")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def load(m, sd):
    """peaked weights into a reference module.  The reference computes the sinusoidal timestep features in float32 whatever the module's
    dtype (dit.py TimestepEmbedder.timestep_embedding); they are an input of the MLP behind them, so for the float64 run they are cast to
    the weights' dtype there and everything after them runs in float64."""
    m.load_state_dict(mg.tsd(sd), strict=True)
    m.t_embedder.mlp.register_forward_pre_hook(lambda mod, inp: (inp[0].to(mod[0].weight.dtype),))
    return m.eval()


def check_scores(tag, H, scores):
    print(f"    {tag} H={H}: max |score| per block {[round(s, 1) for s in scores]} (oracle)")
    assert all(SCORE_RANGE[0] <= s <= SCORE_RANGE[1] for s in scores), (tag, H, scores)


def own_error(tag, what, v32, v64, tol):
    e = rel(v32, v64)
    print(f"    {tag} {what}: the reference's float32 against its float64 {e:.3e} (a quarter of the tolerance: {tol / 4:.2e})")
    assert e <= tol / 4, (tag, what, e)


def main():
    name = "peaked"
    s = PEAKED_SEEDS[name]
    out = {"qk_gain": np.array([QK_GAIN], dtype=np.float64)}
    torch.set_grad_enabled(True)

    m, sd0 = mg.ref_dit(mg.XL2, s["xl2.seed"])
    sd = attn_cases.peak_qk(sd0, QK_GAIN)
    load(m, sd)
    for H in (128, 256):
        x, c = randn(s[f"xl2.x{H}_seed"], 1, 4, H, 16), randn(s[f"xl2.x{H}_seed"] + 1000, 1, 4, H, 16)
        t, y = np.array([37], dtype=np.int64), np.array([2], dtype=np.int64)
        check_scores("xl2", H, attn_cases.model_max_scores(sd, 16, lambda: mg.odit.dit_forward(sd, x, t, y, depth=2, heads=16)))
        res = {}
        for bits, dt in ((32, torch.float32), (64, torch.float64)):
            mm = m.double() if bits == 64 else m.float()
            xt = torch.from_numpy(x).to(dt).requires_grad_(True)
            eps = mm(xt, torch.from_numpy(t), torch.from_numpy(y))
            assert eps.dtype == dt
            gx = torch.autograd.grad((eps * torch.from_numpy(c).to(dt)).sum(), xt)[0]
            res[bits] = (eps.detach().numpy(), gx.numpy())
            out.update({f"xl2.eps{H}_{bits}": res[bits][0], f"xl2.grad{H}_{bits}": res[bits][1]})
        m.float()
        mg.err(f"xl2 H={H} eps", mg.odit.dit_forward(sd, x, t, y, depth=2, heads=16), res[32][0])
        own_error("xl2", f"eps H={H}", res[32][0], res[64][0], TOL)
        own_error("xl2", f"grad H={H}", res[32][1], res[64][1], GRAD_TOL)
        out.update({f"xl2.t{H}": t, f"xl2.y{H}": y})

    cm, csd0 = mg.ref_cls(mg.CLS2, s["cls.seed"])
    csd = attn_cases.peak_qk(csd0, QK_GAIN)
    load(cm, csd)
    for H in (128, 256):
        x = randn(s[f"cls.x{H}_seed"], 2, 4, H, 16)
        t = np.array([991, 12], dtype=np.int64)
        rule = (np.random.RandomState(s[f"cls.x{H}_seed"] + 1000).rand(2, 16) * 4).astype(F32)
        check_scores("cls", H, attn_cases.model_max_scores(csd, 6, lambda: mg.odit.grad_nn_zt_mse(csd, x, t, rule, 10., depth=2, heads=6)))
        res = {}
        for bits, dt in ((32, torch.float32), (64, torch.float64)):
            mm = cm.double() if bits == 64 else cm.float()
            xt = torch.from_numpy(x).to(dt)
            logits = mm(xt, torch.from_numpy(t)).detach()
            assert logits.dtype == dt
            g = mg.rcf.grad_nn_zt_mse(xt, torch.from_numpy(t), rule=torch.from_numpy(rule).to(dt), classifier_scale=10., classifier=mm)
            assert g.dtype == dt
            res[bits] = (logits.numpy(), g.numpy())
            out.update({f"cls.logits{H}_{bits}": res[bits][0], f"cls.grad{H}_{bits}": res[bits][1]})
        cm.float()
        og, ol = mg.odit.grad_nn_zt_mse(csd, x, t, rule, 10., depth=2, heads=6)
        mg.err(f"cls H={H} logits", ol, res[32][0])
        mg.err(f"cls H={H} grad_nn_zt_mse", og, res[32][1])
        own_error("cls", f"logits H={H}", res[32][0], res[64][0], TOL)
        own_error("cls", f"grad H={H}", res[32][1], res[64][1], GRAD_TOL)
        out.update({f"cls.t{H}": t, f"cls.rule{H}": rule})
    torch.set_grad_enabled(False)
    save(name, **{k: np.array([v], dtype=np.int64) for k, v in s.items()}, **out)


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
