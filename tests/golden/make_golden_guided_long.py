#!/usr/bin/env python3
"""Generate the guided long-excerpt fixtures (classifier guidance, DPS, guided editing beyond 256 tokens) under tests/golden/ by
IMPORTING the reference and recording its AUTOGRAD results.

Runs only in the build container, like make_golden.py and make_golden_long.py, whose builders (reference modules through ref_shims,
rgm.synth weights, the teacher-forced noise queue) it reuses:  `python tests/golden/make_golden_guided_long.py [cls] [vjp] [steps]`.

    guidedlong_cls.npz    DiTRotary-S/8-cls: logits and grad_nn_zt_mse (scale 10) of depth 2 and depth 12 at H = 256 (T = 513), B = 2,
                          and of depth 2 at H = 512 (T = 1025), B = 1; the chord classifier's grad_nn_zt_chord at H = 256;
                          grad_nn_zt_xentropy (depth 2) at H = 256
    guidedlong_vjp.npz    th.autograd.grad((m(x, t, y) * g).sum(), x) of the eps-network: XL-2 at H = 136 / 256 / 512 (T = 272 / 512 /
                          1024), XL-28 at H = 256, B = 1
    guidedlong_steps.npz  (+ .part2.npz, joined by conftest.load_golden) teacher-forced single steps at H = 256, B = 2, XL-2 + the
                          depth-2 classifier: classifier-guided p_sample ("250" chain); condition_score DDIM step (ddim50 chain,
                          eta = 1); DPS-nn p_sample (nn_z0_mse_dummy); DPS-rule p_sample with pitch_hist through the real decoder; a
                          classifier-guided edit step.  The reference REFUSES classifier guidance under a partial editable range at
                          any length (it multiplies the full-size variance by the gradient of the editable slice): the exception text
                          is stored as `edit.reference_raises` and the step recorded is the one the shipped configs run, the whole
                          latent editable (`editfull.*`).

No input tensor is stored: every x, cotangent and noise is np.random.RandomState(seed).randn(shape) of a seed pinned by name in
GUIDED_LONG_SEEDS and stored as a ONE-ELEMENT array (make_golden.py's FIXTURE_SEEDS check reads 0-d `*seed` arrays only);
tests/test_guided_long_fixtures.py holds the fixtures to this table."""
import glob
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (installs ref_shims, imports the reference)

F32 = np.float32
GUIDED_LONG_SEEDS = {
    "guidedlong_cls": {"s8d2.seed": 4, "s8.seed": 3, "chord.seed": 5, "s8d2.x256_seed": 810, "s8.x256_seed": 811, "s8d2.x512_seed": 812,
                       "chord.x256_seed": 813, "xent.x256_seed": 814},
    "guidedlong_vjp": {"xl2.seed": 1, "xl28.seed": 1, "xl2.x136_seed": 820, "xl2.x256_seed": 821, "xl2.x512_seed": 822,
                       "xl28.x256_seed": 823},
    "guidedlong_steps": {"dit.seed": 1, "cls.seed": 4, "vae.seed": 2, "x_seed": 830, "cg.noise_seed": 831, "dcg.noise_seed": 832,
                         "dps.noise_seed": 833, "dpsr.noise_seed": 834, "editfull.noise_seed": 835, "gt_seed": 836},
}
LIMIT = 1024 * 1024
PART_BYTES = 900 * 1024


def randn(seed, *shape):
    """THE rule every input of these fixtures is rebuilt by (tests restate it)."""
    return np.random.RandomState(seed).randn(*shape).astype(F32)


def seeds(name):
    return {k: np.array([v], dtype=np.int64) for k, v in GUIDED_LONG_SEEDS[name].items()}


def save(name, **arrs):
    stored = {k: int(np.asarray(v).reshape(-1)[0]) for k, v in arrs.items() if k.endswith("seed")}
    assert stored == GUIDED_LONG_SEEDS[name], f"{name}: stored seeds {stored} != GUIDED_LONG_SEEDS[{name!r}]"
    for old in glob.glob(os.path.join(HERE, name + ".part*.npz")):
        os.remove(old)
    # the seeds and the first arrays in name.npz, the rest in name.part2.npz, ... (conftest.load_golden joins them), no file over 1 MiB
    parts, size = [{k: v for k, v in arrs.items() if k.endswith("seed")}], 0
    for k, v in arrs.items():
        if k.endswith("seed"):
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


def g_cls():
    name = "guidedlong_cls"
    print(f"[{name}]")
    s = GUIDED_LONG_SEEDS[name]
    out = {}
    torch.set_grad_enabled(True)
    for tag, arch, H, B in (("s8d2", mg.CLS2, 256, 2), ("s8", mg.CLS, 256, 2), ("s8d2", mg.CLS2, 512, 1)):
        m, sd = mg.ref_cls(arch, s[f"{tag}.seed"])
        x = randn(s[f"{tag}.x{H}_seed"], B, 4, H, 16)
        t = np.array([991, 12][:B], dtype=np.int64)
        rule = (np.random.RandomState(s[f"{tag}.x{H}_seed"] + 1000).rand(B, 16) * 4).astype(F32)
        logits = m(torch.from_numpy(x), torch.from_numpy(t)).detach().numpy()
        g = mg.rcf.grad_nn_zt_mse(torch.from_numpy(x), torch.from_numpy(t), rule=torch.from_numpy(rule), classifier_scale=10.,
                                  classifier=m).numpy()
        og, ol = mg.odit.grad_nn_zt_mse(sd, x, t, rule, 10., depth=arch["depth"], heads=arch["heads"])
        mg.err(f"{tag} H={H} logits", ol, logits)
        mg.err(f"{tag} H={H} grad_nn_zt_mse", og, g)
        out.update({f"{tag}.t{H}": t, f"{tag}.rule{H}": rule, f"{tag}.logits{H}": logits, f"{tag}.grad{H}": g})
    m, sd = mg.ref_cls(mg.CHD, s["chord.seed"])
    x = randn(s["chord.x256_seed"], 2, 4, 256, 16)
    t = np.array([500, 3], dtype=np.int64)
    rule = np.random.RandomState(s["chord.x256_seed"] + 1000).randint(0, 8, size=(2, 256 // 16)).astype(np.int64)      # one chord per 16 latent rows
    key, ch = m(torch.from_numpy(x), torch.from_numpy(t))
    g = mg.rcf.grad_nn_zt_chord(torch.from_numpy(x), torch.from_numpy(t), rule=torch.from_numpy(rule), classifier_scale=10.,
                                classifier=m).numpy()
    og, (ok, oc) = mg.odit.grad_nn_zt_chord(sd, x, t, rule, 10., depth=2, heads=6)
    mg.err("chord logits", oc, ch.detach().numpy())
    mg.err("grad_nn_zt_chord", og, g)
    out.update({"chord.t256": t, "chord.rule256": rule, "chord.key256": key.detach().numpy(), "chord.logits256": ch.detach().numpy(),
                "chord.grad256": g})
    # grad_nn_zt_xentropy (condition_functions.py:46-56): d log softmax(classifier(x, 0))[rule] / dx, the depth-2 classifier
    m, sd = mg.ref_cls(mg.CLS2, s["s8d2.seed"])
    x = randn(s["xent.x256_seed"], 2, 4, 256, 16)
    lab = np.array([3, 11], dtype=np.int64)
    gx = mg.rcf.grad_nn_zt_xentropy(torch.from_numpy(x), rule=torch.from_numpy(lab), classifier=m).numpy()
    print(f"    xentropy |grad| {np.abs(gx).max():.3e}")
    out.update({"xent.rule256": lab, "xent.grad256": gx})
    torch.set_grad_enabled(False)
    save(name, **seeds(name), **out)


def g_vjp():
    name = "guidedlong_vjp"
    print(f"[{name}]")
    s = GUIDED_LONG_SEEDS[name]
    out = {}
    torch.set_grad_enabled(True)
    for tag, arch, shapes in (("xl2", mg.XL2, (136, 256, 512)), ("xl28", mg.XL28, (256,))):
        m, sd = mg.ref_dit(arch, s[f"{tag}.seed"])
        for H in shapes:
            x = randn(s[f"{tag}.x{H}_seed"], 1, 4, H, 16)
            g = randn(s[f"{tag}.x{H}_seed"] + 1000, 1, 4, H, 16)
            t = np.array([37], dtype=np.int64)
            y = np.array([2], dtype=np.int64)
            xt = torch.from_numpy(x).requires_grad_(True)
            eps = m(xt, torch.from_numpy(t), torch.from_numpy(y))
            gx = torch.autograd.grad((eps * torch.from_numpy(g)).sum(), xt)[0]
            out.update({f"{tag}.t{H}": t, f"{tag}.y{H}": y, f"{tag}.eps{H}": eps.detach().numpy(), f"{tag}.grad{H}": gx.numpy()})
            print(f"    {tag} H={H}: |eps| {np.abs(eps.detach().numpy()).max():.3f}  |grad_x| {np.abs(gx.numpy()).max():.3f}")
    torch.set_grad_enabled(False)
    save(name, **seeds(name), **out)


def g_steps():
    name = "guidedlong_steps"
    print(f"[{name}]")
    from functools import partial
    from types import SimpleNamespace
    s = GUIDED_LONG_SEEDS[name]
    B, H = 2, 256
    m, sd = mg.ref_dit(mg.XL2, s["dit.seed"])
    cm, csd = mg.ref_cls(mg.CLS2, s["cls.seed"])
    mf = mg.ref_model_fn(m, 3, True)
    x = randn(s["x_seed"], B, 4, H, 16)
    y = np.array([1, 2], dtype=np.int64)
    rule = (np.random.RandomState(s["x_seed"] + 1000).rand(B, 16) * 4).astype(F32)
    trule = {"note_density": torch.from_numpy(rule)}
    tx, ty = torch.from_numpy(x), torch.from_numpy(y)
    out = {"y": y, "rule": rule}
    cg = SimpleNamespace(schedule=False, method="classifier_guidance")
    cond = partial(mg.rcf.composite_nn_zt, fns=["grad_nn_zt_mse"], classifier_scales=[10.], classifiers=[cm], rule_names=["note_density"])
    torch.set_grad_enabled(True)

    def unguided(rs, t, nz, ddim=False):
        d = mg.make_diffusion(rs)
        d.t_end = 0
        mg.NQ.push(nz)
        with torch.no_grad():
            if ddim:
                return d.ddim_sample(mf, tx, torch.from_numpy(t), clip_denoised=False, eta=1.0, model_kwargs={"y": ty})
            return d.p_sample(mf, tx, torch.from_numpy(t), clip_denoised=False, model_kwargs={"y": ty})

    # ---- classifier-guided DDPM step, "250" chain (condition_mean)
    d = mg.make_diffusion("250")
    d.t_end = 0
    t = np.full((B,), 200, dtype=np.int64)
    nz = randn(s["cg.noise_seed"], B, 4, H, 16)
    mg.NQ.push(nz)
    r = d.p_sample(mf, tx, torch.from_numpy(t), clip_denoised=False, cond_fn=cond, model_kwargs={"y": ty, "rule": trule}, guidance_kwargs=cg)
    u = unguided("250", t, nz)
    shift = (r["sample"] - u["sample"]).detach().numpy()
    print(f"    cg: guidance shift |max| {np.abs(shift).max():.3e}")
    out.update({"cg.t": t, "cg.sample": r["sample"].detach().numpy(), "cg.shift": shift})

    # ---- DDIM (eta = 1) + classifier guidance in eps space (condition_score), ddim50 chain
    d = mg.make_diffusion("ddim50")
    d.t_end = 0
    t = np.full((B,), 30, dtype=np.int64)
    nz = randn(s["dcg.noise_seed"], B, 4, H, 16)
    mg.NQ.push(nz)
    r = d.ddim_sample(mf, tx, torch.from_numpy(t), clip_denoised=False, cond_fn=cond, eta=1.0, model_kwargs={"y": ty, "rule": trule},
                      guidance_kwargs=cg)
    u = unguided("ddim50", t, nz, ddim=True)
    shift = (r["sample"] - u["sample"]).detach().numpy()
    print(f"    dcg: guidance shift |max| {np.abs(shift).max():.3e}")
    out.update({"dcg.t": t, "dcg.sample": r["sample"].detach().numpy(), "dcg.shift": shift})

    # ---- DPS through the classifier on x0 (nn_z0_mse_dummy), "250" chain
    d = mg.make_diffusion("250")
    d.t_end = 0
    t = np.full((B,), 130, dtype=np.int64)
    nz = randn(s["dps.noise_seed"], B, 4, H, 16)
    mg.NQ.push(nz)
    dcond = partial(mg.rcf.composite_nn_zt, fns=["nn_z0_mse_dummy"], classifier_scales=[1.], classifiers=[cm], rule_names=["note_density"])
    gk = SimpleNamespace(schedule=False, method="dps", step_size=1.5, nn=True, vae=False)
    r = d.p_sample(mf, tx, torch.from_numpy(t), clip_denoised=False, cond_fn=dcond, model_kwargs={"y": ty, "rule": trule},
                   guidance_kwargs=gk, embed_model=None)
    out.update({"dps.t": t, "dps.sample": r["sample"].detach().numpy(), "dps.pred_xstart": r["pred_xstart"].detach().numpy()})
    print(f"    dps: sample range {r['sample'].min().item():.3f} .. {r['sample'].max().item():.3f}")

    # ---- DPS through pitch_hist(decode(x0)) with the reference Decoder, "250" chain
    vae = mg.RefVAE(s["vae.seed"])
    tgt = np.random.RandomState(s["x_seed"] + 2000).rand(B, 12).astype(F32)
    tgt /= tgt.sum(-1, keepdims=True)
    d = mg.make_diffusion("250")
    d.t_end = 0
    t = np.full((B,), 90, dtype=np.int64)
    nz = randn(s["dpsr.noise_seed"], B, 4, H, 16)
    mg.NQ.push(nz)
    rcond = partial(mg.rcf.composite_rule, fns=["rule_x0_mse_dummy"], classifier_scales=[1.], rule_names=["pitch_hist"])
    gk = SimpleNamespace(schedule=False, method="dps", step_size=100.0, nn=False, vae=True)
    t0 = time.time()
    r = d.p_sample(mf, tx, torch.from_numpy(t), clip_denoised=False, cond_fn=rcond,
                   model_kwargs={"y": ty, "rule": {"pitch_hist": torch.from_numpy(tgt)}}, guidance_kwargs=gk, embed_model=vae,
                   scale_factor=1.2465)
    u = unguided("250", t, nz)
    shift = (r["sample"] - u["sample"]).detach().numpy()
    print(f"    dpsr: guidance shift |max| {np.abs(shift).max():.4e}  ({time.time() - t0:.0f} s)")
    out.update({"dpsr.t": t, "dpsr.target": tgt, "dpsr.sample": r["sample"].detach().numpy(), "dpsr.shift": shift})

    # ---- classifier-guided edit step, "250" chain: a partial editable range first (as asked of these fixtures), then the whole latent
    gt = (randn(s["gt_seed"], B, 4, H, 16) * 0.8).astype(F32)
    ls, le = 64, 192
    mask = np.ones_like(gt)
    mask[:, :, ls:le, :] = 0.
    t = np.full((B,), 120, dtype=np.int64)
    nz = randn(s["editfull.noise_seed"], B, 4, H, 16)
    out.update({"edit.l_start": np.array([ls]), "edit.l_end": np.array([le]), "editfull.t": t})
    for tag, ek in (("edit", {"gt": torch.from_numpy(gt), "mask": torch.from_numpy(mask), "l_start": ls, "l_end": le, "noise_level": 3}),
                    ("editfull", {"gt": torch.from_numpy(gt), "mask": torch.zeros(gt.shape), "l_start": 0, "l_end": H, "noise_level": 3})):
        d = mg.make_diffusion("250")
        d.t_end = 0
        mg.NQ.q.clear()
        mg.NQ.push(nz)
        try:
            with torch.no_grad():
                r = d.p_sample(mf, tx, torch.from_numpy(t), clip_denoised=False, cond_fn=cond, model_kwargs={"y": ty, "rule": trule},
                               guidance_kwargs=cg, edit_kwargs=ek)
            out[f"{tag}.sample"] = r["sample"].detach().numpy()
            print(f"    {tag}: ran, sample range {r['sample'].min().item():.3f} .. {r['sample'].max().item():.3f}")
        except Exception as e:  # noqa: BLE001  (whatever the reference raises is the record)
            out[f"{tag}.reference_raises"] = np.array(f"{type(e).__name__}: {e}")
            print(f"    {tag}: the reference raises {type(e).__name__}: {e}")
    mg.NQ.q.clear()
    torch.set_grad_enabled(False)
    save(name, **seeds(name), **out)


if __name__ == "__main__":
    which = set(sys.argv[1:]) or {"cls", "vjp", "steps"}
    torch.set_num_threads(8)
    if "cls" in which:
        g_cls()
    if "vjp" in which:
        g_vjp()
    if "steps" in which:
        g_steps()
