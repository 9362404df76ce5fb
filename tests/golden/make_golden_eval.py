#!/usr/bin/env python3
"""Generate the inversion / bits-per-dim fixtures under tests/golden/ by IMPORTING the reference.

Runs only in the build container, like make_golden.py, whose builders (reference modules through ref_shims, rgm.synth weights,
the teacher-forced noise queue) it reuses:  `python tests/golden/make_golden_eval.py`.

    eval_terms.npz    no network.  Chain "8", B = 2, E = 2048.  For every variance type (fixed_large, fixed_small, learned,
                      learned_range), every timestep pair of T_SETS and clip_denoised on / off: the reference's _vb_terms_bpd output,
                      xstart_mse and mse (the lines of calc_bpd_loop) computed in fp64 (fp64_tables below) from a frozen model output, and next to each
                      (`.d_ref`) the deviation of the reference's own fp32 result, relative to the largest fp64 magnitude.
                      pred_xstart per (timestep pair, clip); _prior_bpd.
    eval_steps.npz    the same inputs: ddim_reverse_sample (sample, per timestep pair and clip) and _predict_xstart_from_xprev in fp64,
                      with d_ref.
    eval_bpd.npz      calc_bpd_loop on chain "8": SM network (seed 11), class-conditional, injected noise -- inputs, the reference's
                      model output of every step, its five outputs (fp32) and the same five re-evaluated in fp64 from the stored model
                      outputs, with d_ref.  `ls.*`: the same on a learn_sigma=True network (dict(SM, out_ch=8), seed 21) whose final
                      layer is scaled down (`ls.final_std`) until every vb term is below 1e3.
    eval_invert.npz   SM, chain "ddim50", H = 128: x_start, the first ddim_reverse_sample step and the latent after 20 of them
                      (clip_denoised=False).
    eval_api.json     parameter names of the reference's five methods (inspect.signature).

Seeds are pinned by name in EVAL_SEEDS and stored as ONE-ELEMENT arrays; tests/test_eval_fixtures.py holds the fixtures to this table."""
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (installs ref_shims, imports the reference)

F32, F64 = np.float32, np.float64
EVAL_SEEDS = {
    "eval_terms": {"x_seed": 810},
    "eval_steps": {"x_seed": 810},
    "eval_bpd": {"seed": 11, "x_seed": 811, "ls.seed": 21, "ls.x_seed": 812},
    "eval_invert": {"seed": 11, "x_seed": 813},
}
VAR_TYPES = ("fixed_large", "fixed_small", "learned", "learned_range")
T_SETS = ((0, 0), (1, 7), (4, 0), (7, 4))       # chain "8": t in {0, 1, mid, T - 1}, equal and mixed within the batch
LIMIT = 1024 * 1024
API = ("ddim_reverse_sample", "_predict_xstart_from_xprev", "_vb_terms_bpd", "_prior_bpd", "calc_bpd_loop")


def save(name, **arrs):
    stored = {k: int(np.asarray(v).reshape(-1)[0]) for k, v in arrs.items() if k.endswith("seed")}
    assert stored == EVAL_SEEDS[name], f"{name}: stored seeds {stored} != EVAL_SEEDS[{name!r}]"
    p = os.path.join(HERE, name + ".npz")
    np.savez_compressed(p, **arrs)
    assert os.path.getsize(p) < LIMIT, f"{p}: {os.path.getsize(p)} bytes"
    print(f"  wrote {p} ({os.path.getsize(p) / 1024:.0f} KiB)")


def seeds(name):
    return {k: np.array([v], dtype=np.int64) for k, v in EVAL_SEEDS[name].items()}


def d_ref(f32, f64):
    f32, f64 = np.asarray(f32, dtype=F64), np.asarray(f64, dtype=F64)
    return np.array([np.abs(f32 - f64).max() / (np.abs(f64).max() + 1e-300)])


def diffusion(rs, var_type="fixed_large"):
    vt = {"fixed_large": mg.rgd.ModelVarType.FIXED_LARGE, "fixed_small": mg.rgd.ModelVarType.FIXED_SMALL,
          "learned": mg.rgd.ModelVarType.LEARNED, "learned_range": mg.rgd.ModelVarType.LEARNED_RANGE}[var_type]
    return mg.rrs.SpacedDiffusion(use_timesteps=mg.rrs.space_timesteps(1000, rs), betas=mg.rgd.get_named_beta_schedule("linear", 1000),
                                  model_mean_type=mg.rgd.ModelMeanType.EPSILON, model_var_type=vt, loss_type=mg.rgd.LossType.MSE,
                                  rescale_timesteps=False)


class fp64_tables:
    """The reference's _extract_into_tensor ends in .float(): with .double() inputs its table entries still arrive as float32 TENSORS,
    and what is formed from them alone (exp(logvar1 - logvar2) of fixed variances, the prior's exp(logvar)) is then evaluated in
    float32 -- a "fp64" prior_bpd 3e-5 away from its value.  Inside this context the entries keep their float32-cast VALUES (what the
    fp32 run sees) but arrive as float64 tensors, so that the fp64 results are fp64 throughout."""

    def __enter__(self):
        self.orig = orig = mg.rgd._extract_into_tensor
        mg.rgd._extract_into_tensor = lambda arr, t, shape: orig(arr, t, shape).double()

    def __exit__(self, *exc):
        mg.rgd._extract_into_tensor = self.orig


def both(fn):
    """fn(dtype) in fp64 (under fp64_tables) and in fp32 -> (r64, r32)"""
    with fp64_tables():
        r64 = fn(torch.float64)
    return r64, fn(torch.float32)


def terms_inputs():
    rng = np.random.RandomState(EVAL_SEEDS["eval_terms"]["x_seed"])
    B, H = 2, 32
    shape = (B, 4, H, 16)
    x_start = np.clip(rng.randn(*shape) * 0.8, -1, 1).astype(F32)      # data lives in [-1, 1]; a fifth of it at the two edge bins
    flat = x_start.reshape(B, -1)
    for b in range(B):          # both edge bins of the decoder term and both sides of +-0.999
        flat[b, 5:13] = np.array([-1, 1, -0.9995, 0.9995, -1, 1, -0.9995, 0.9995], dtype=F32)
        flat[b, 1000:1004] = np.array([-0.9985, 0.9985, -1, 1], dtype=F32)
    # x_t is random AROUND x_start (what q_sample gives at a small t): with an unrelated x_t the t == 0 term sits in the tails where
    # cdf_plus - cdf_min is 1e-12 .. 1e-6 and fp64 itself keeps 1e-9 of the mean (torch's and numpy's tanh differ by an ulp there);
    # tests/test_gpu_eval.py covers unrelated inputs (the 1e-12 clamps) at its own sizes
    x_t = (x_start + 0.01 * rng.randn(*shape)).astype(F32)
    eps = rng.randn(*shape).astype(F32)
    noise = rng.randn(*shape).astype(F32)
    var_values = rng.uniform(-1, 1, size=shape).astype(F32)          # LEARNED_RANGE: the interpolation fraction in [-1, 1]
    var_log = (-4.0 + 2.0 * var_values).astype(F32)                  # LEARNED: the log-variance itself
    xprev = rng.randn(*shape).astype(F32)
    return dict(x_start=x_start, x_t=x_t, eps=eps, noise=noise, var_values=var_values, var_log=var_log, xprev=xprev)


def frozen(out, dt):
    o = torch.from_numpy(out).to(dt)
    return lambda x, t, **kw: o


def model_out(inp, vt):
    if vt == "learned_range":
        return np.concatenate([inp["eps"], inp["var_values"]], axis=1)
    if vt == "learned":
        return np.concatenate([inp["eps"], inp["var_log"]], axis=1)
    return inp["eps"]


def vb_case(d, inp, vt, t, clip, dt):
    """_vb_terms_bpd and the two errors exactly as calc_bpd_loop forms them (:1300-1314), in dtype dt"""
    T = lambda a: torch.from_numpy(a).to(dt)
    x_start, x_t, noise, tt = T(inp["x_start"]), T(inp["x_t"]), T(inp["noise"]), torch.from_numpy(t)
    with torch.no_grad():
        out = d._vb_terms_bpd(frozen(model_out(inp, vt), dt), x_start=x_start, x_t=x_t, t=tt, clip_denoised=clip, model_kwargs={})
    xm = mg.rgd.mean_flat((out["pred_xstart"] - x_start) ** 2)
    e = d._predict_eps_from_xstart(x_t, tt, out["pred_xstart"])
    return {"vb": out["output"].numpy(), "xstart_mse": xm.numpy(), "mse": mg.rgd.mean_flat((e - noise) ** 2).numpy(),
            "pred_xstart": out["pred_xstart"].numpy()}


def g_terms():
    print("[eval_terms / eval_steps]")
    inp = terms_inputs()
    out = dict(inp)
    out["t_sets"] = np.array(T_SETS, dtype=np.int64)
    steps = {"t_sets": out["t_sets"]}
    worst = {}
    for vt in VAR_TYPES:
        d = diffusion("8", vt)
        for si, ts in enumerate(T_SETS):
            t = np.array(ts, dtype=np.int64)
            for clip in (0, 1):
                r64, r32 = both(lambda dt: vb_case(d, inp, vt, t, bool(clip), dt))
                tag = f"{vt}.s{si}.c{clip}"
                for k in ("vb", "xstart_mse", "mse"):
                    out[f"{tag}.{k}"] = r64[k]
                    out[f"{tag}.{k}.d_ref"] = d_ref(r32[k], r64[k])
                    worst[k] = max(worst.get(k, 0.), float(out[f"{tag}.{k}.d_ref"][0]))
                if vt == "fixed_large":       # pred_xstart does not depend on the variance type
                    out[f"s{si}.c{clip}.pred_xstart"] = r64["pred_xstart"]
                    out[f"s{si}.c{clip}.pred_xstart.d_ref"] = d_ref(r32["pred_xstart"], r64["pred_xstart"])
                    def rev(dt):
                        with torch.no_grad():
                            return d.ddim_reverse_sample(frozen(inp["eps"], dt), torch.from_numpy(inp["x_t"]).to(dt), torch.from_numpy(t),
                                                         clip_denoised=bool(clip), model_kwargs={})
                    v64, v32 = both(rev)
                    assert np.array_equal(v64["pred_xstart"].numpy(), r64["pred_xstart"])
                    steps[f"s{si}.c{clip}.sample"] = v64["sample"].numpy()
                    steps[f"s{si}.c{clip}.sample.d_ref"] = d_ref(v32["sample"].numpy(), v64["sample"].numpy())
            if vt == "fixed_large":
                tt = torch.from_numpy(t)
                x64, x32 = both(lambda dt: d._predict_xstart_from_xprev(torch.from_numpy(inp["x_t"]).to(dt), tt,
                                                                        torch.from_numpy(inp["xprev"]).to(dt)).numpy())
                steps[f"s{si}.xstart_from_xprev"] = x64
                steps[f"s{si}.xstart_from_xprev.d_ref"] = d_ref(x32, x64)
    d = diffusion("8")
    p64, p32 = both(lambda dt: d._prior_bpd(torch.from_numpy(inp["x_start"]).to(dt)).numpy())
    out["prior_bpd"], out["prior_bpd.d_ref"] = p64, d_ref(p32, p64)
    print("    worst d_ref:", {k: f"{v:.2e}" for k, v in worst.items()}, f"prior {float(out['prior_bpd.d_ref'][0]):.2e}")
    save("eval_terms", **seeds("eval_terms"), **out)
    save("eval_steps", **seeds("eval_steps"), **steps)


def ls_dit(seed, final_std):
    arch = dict(mg.SM, out_ch=8)
    sd = mg.synth.dit_state_dict(seed, final_std=final_std, **arch)
    m = mg.rdit.DiTRotary(input_size=[128, 16], patch_size=8, in_channels=4, hidden_size=384, depth=2, num_heads=6, num_classes=3,
                          learn_sigma=True)
    m.load_state_dict(mg.tsd(sd), strict=True)
    m.eval()
    return m


def bpd_entry(m, learn_sigma, x_start, y, noises):
    """calc_bpd_loop of the reference on chain "8" in fp32 (recording the model's output at every step) and again in fp64 from
    those outputs"""
    d = mg.rsu.create_diffusion(learn_sigma=learn_sigma, diffusion_steps=1000, noise_schedule="linear", timestep_respacing="8",
                                use_kl=False, predict_xstart=False, rescale_timesteps=False, rescale_learned_sigmas=False)
    mf = mg.ref_model_fn(m, 3, True)
    outs = []

    def rec(x, t, **kw):
        o = mf(x, t, **kw)
        outs.append(o.detach().numpy().copy())
        return o
    mg.NQ.push(*noises)
    with torch.no_grad():
        r32 = d.calc_bpd_loop(rec, torch.from_numpy(x_start), clip_denoised=True, model_kwargs={"y": torch.from_numpy(y)})
    assert len(outs) == 8 and not mg.NQ.q
    replay = [torch.from_numpy(o).double() for o in outs]
    mg.NQ.q += [torch.from_numpy(n).double() for n in noises]
    with torch.no_grad(), fp64_tables():
        r64 = d.calc_bpd_loop(lambda x, t, **kw: replay.pop(0), torch.from_numpy(x_start).double(), clip_denoised=True,
                              model_kwargs={"y": torch.from_numpy(y)})
    assert not replay and not mg.NQ.q
    res = {"model_out": np.stack(outs)}
    for k in ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse"):
        res[f"ref.{k}"] = r32[k].numpy()
        res[f"f64.{k}"] = r64[k].numpy()
        res[f"f64.{k}.d_ref"] = d_ref(r32[k].numpy(), r64[k].numpy())
    return res


def g_bpd():
    print("[eval_bpd]")
    s = EVAL_SEEDS["eval_bpd"]
    B, H = 2, 32
    out = {}
    for prefix, learn in (("", False), ("ls.", True)):
        rng = np.random.RandomState(s[prefix + "x_seed"])
        x_start = (rng.randn(B, 4, H, 16) * 0.8).astype(F32)
        y = np.array([1, 2], dtype=np.int64)
        noises = [rng.randn(B, 4, H, 16).astype(F32) for _ in range(8)]
        if not learn:
            m, _ = mg.ref_dit(mg.SM, s["seed"])
            res = bpd_entry(m, False, x_start, y, noises)
        else:
            std = 1.0 / 384 ** 0.5                 # rgm.synth's default final-layer scale: its variance channels overflow the KL
            while True:
                res = bpd_entry(ls_dit(s["ls.seed"], std), True, x_start, y, noises)
                top = float(np.abs(res["f64.vb"]).max())
                print(f"    learn_sigma: final_std {std:.5f} -> largest vb term {top:.3g}")
                if top < 1e3:
                    break
                std *= 0.5
            assert np.abs(res["f64.vb"]).max() < 1e3 and np.abs(res["ref.vb"]).max() < 1e3
            out["ls.final_std"] = np.array([std])
        out.update({prefix + "x_start": x_start, prefix + "y": y, prefix + "noise": np.stack(noises)})
        out.update({prefix + k: v for k, v in res.items()})
        print(f"    {prefix or 'sm.'} total_bpd {res['ref.total_bpd']}  d_ref(total) {float(res['f64.total_bpd.d_ref'][0]):.2e}"
              f"  d_ref(vb) {float(res['f64.vb.d_ref'][0]):.2e}")
    save("eval_bpd", **seeds("eval_bpd"), **out)


def g_invert():
    print("[eval_invert]")
    s = EVAL_SEEDS["eval_invert"]
    m, _ = mg.ref_dit(mg.SM, s["seed"])
    mf = mg.ref_model_fn(m, 3, True)
    rng = np.random.RandomState(s["x_seed"])
    B, H = 2, 128
    x_start = (rng.randn(B, 4, H, 16) * 0.8).astype(F32)
    y = np.array([1, 2], dtype=np.int64)
    d = mg.make_diffusion("ddim50")
    img = torch.from_numpy(x_start)
    first = None
    with torch.no_grad():
        for i in range(20):
            r = d.ddim_reverse_sample(mf, img, torch.full((B,), i, dtype=torch.int64), clip_denoised=False, model_kwargs={"y": torch.from_numpy(y)})
            first = first or r
            img = r["sample"]
    save("eval_invert", **seeds("eval_invert"), x_start=x_start, y=y, steps=np.array([20], dtype=np.int64),
         first_sample=first["sample"].numpy(), first_pred_xstart=first["pred_xstart"].numpy(), latent=img.numpy())


def g_api():
    names = {n: list(inspect.signature(getattr(mg.rgd.GaussianDiffusion, n)).parameters) for n in API}
    p = os.path.join(HERE, "eval_api.json")
    with open(p, "w") as f:
        json.dump(names, f, indent=1)
        f.write("\n")
    print(f"  wrote {p}")


if __name__ == "__main__":
    which = set(sys.argv[1:]) or {"terms", "bpd", "invert", "api"}
    torch.set_num_threads(8)
    if "terms" in which:
        g_terms()
    if "bpd" in which:
        g_bpd()
    if "invert" in which:
        g_invert()
    if "api" in which:
        g_api()
