"""-m gpu: DDIM inversion and bits-per-dim evaluation -- rgm_ddim_reverse_step / rgm_vb_terms / rgm_prior_bpd (csrc/eval.hip) and the
scheduler methods built on them (ddim_reverse_sample(_loop), _vb_terms_bpd, _prior_bpd, calc_bpd_loop, _predict_xstart_from_xprev)
against the reference's fp64 results (tests/golden/make_golden_eval.py) and the fp64 restatement of tests/eval_ref.py.

Bound of every comparison with fp64: max(4 d_ref, 1e-6) relative to the quantity's largest magnitude, d_ref = the reference's own fp32
deviation from fp64 (eval_ref.bound); where no reference result exists (the large shapes) the floor 1e-6 alone.

Measured on the MI355X (docs/rounds/eval.md): the kernels evaluate every element in fp64, so what is left is the rounding of their fp32
outputs -- largest error 5.9e-8 over all cases; largest error / d_ref: vb 1.0 (decoder and KL branch alike: our float and the
reference's float are then the same number), xstart_mse 1.0, mse 0.62, pred_xstart 0.96, ddim_reverse_sample 0.36, _prior_bpd 2e-4,
_predict_xstart_from_xprev 1.0.  No term needs the factor 4.  calc_bpd_loop on the reference's model outputs: <= 5.6e-8 on all five
outputs; with our network each step's output within 6.4e-6 (fp32) / 2.0e-5 (bf16x3) of the reference's, total_bpd 3.7e-3 from the
reference's FP32 result (= that result's own distance from fp64; printed, not asserted).  20-step inversion: 8.7e-7 / 7.1e-6.
"""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import eval_ref as er
from conftest import PKG, load_golden
from rgm import synth
from test_gpu_sampler import SM, _diffusion, _dit, _inject, _model_fn

pytestmark = pytest.mark.gpu
F32 = np.float32
TOL = 2e-4          # the forward contract (tests/test_gpu_long.py)


def _frozen(*outs):
    """a 'network' that returns stored outputs, one per call (the last one for ever)"""
    q = [torch.from_numpy(np.ascontiguousarray(o)).cuda() for o in outs]
    return lambda x, t, **kw: q.pop(0) if len(q) > 1 else q[0]


def _vb_kernel(d, var_type, x_start, x_t, eps, noise, t, clip, var_values=None):
    """rgm_vb_terms through the C ABI on numpy inputs -> dict of numpy outputs"""
    from gpu_util import dev
    from rgm import native as R
    N = x_start.shape[0]
    E = x_start.size // N
    xs, xt, ep, tt = dev(x_start), dev(x_t), dev(eps), dev(np.asarray(t, dtype=np.int64))
    nz = dev(noise) if noise is not None else None
    vv = dev(var_values) if var_values is not None else None
    lt = d._learned_tabs("cuda")
    lo, hi = (lt[0], lt[1]) if var_type == "learned_range" else (None, None)
    part = torch.empty(int(R.lib.rgm_vb_terms_partials(N, E)), dtype=torch.float64, device="cuda")
    vb, xm, em = (torch.full((N,), float("nan"), device="cuda") for _ in range(3))
    x0 = torch.full((N, E), float("nan"), device="cuda")
    R.check(R.lib.rgm_vb_terms(R.ptr(xs), R.ptr(xt), R.ptr(ep), R.ptr(nz), R.ptr(tt), d._tab("cuda").ptrs, R.ptr(lt[0]), R.ptr(vv), R.ptr(lo),
                               R.ptr(hi), None, None, int(clip), R.ptr(part), R.ptr(vb), R.ptr(xm), R.ptr(em) if nz is not None else None,
                               R.ptr(x0), N, E, R.current_stream()))
    torch.cuda.synchronize()
    return {"vb": vb.cpu().numpy(), "xstart_mse": xm.cpu().numpy(), "mse": em.cpu().numpy(), "pred_xstart": x0.cpu().numpy().reshape(x_t.shape)}


def _report(tag, got, want, d_ref):
    err, lim = er.rel_to_max(got, want), er.bound(d_ref)
    d = float(np.asarray(d_ref).reshape(-1)[0])
    print(f"EVAL {tag}: err {err:.3e}  d_ref {d:.3e}  err/d_ref {err / max(d, 1e-300):.3g}  bound {lim:.3e}")
    return err, lim


@pytest.mark.parametrize("var_type", er.VAR_TYPES)
def test_vb_terms_kernel_matches_the_fp64_reference(var_type):
    g = load_golden("eval_terms")
    d = er.diffusion("8", var_type)
    vv = {"learned": g["var_log"], "learned_range": g["var_values"]}.get(var_type)
    bad = []
    for si, ts in enumerate(g["t_sets"]):
        for clip in (0, 1):
            r = _vb_kernel(d, var_type, g["x_start"], g["x_t"], g["eps"], g["noise"], ts, clip, vv)
            tag = f"{var_type}.s{si}.c{clip}"
            for k in ("vb", "xstart_mse", "mse"):
                err, lim = _report(f"{tag}.{k}", r[k], g[f"{tag}.{k}"], g[f"{tag}.{k}.d_ref"])
                if not err <= lim:
                    bad.append((tag, k, err, lim))
            err, lim = _report(f"{tag}.pred_xstart", r["pred_xstart"], g[f"s{si}.c{clip}.pred_xstart"], g[f"s{si}.c{clip}.pred_xstart.d_ref"])
            if not err <= lim:
                bad.append((tag, "pred_xstart", err, lim))
    assert not bad, bad


@pytest.mark.parametrize("var_type", er.VAR_TYPES)
def test_methods_match_the_fp64_reference_on_a_frozen_output(var_type):
    """the same fixture through the Python methods (a model that returns the stored output; the re-spaced chain wraps it)"""
    from gpu_util import dev
    g, s = load_golden("eval_terms"), load_golden("eval_steps")
    d = er.diffusion("8", var_type)
    out = {"learned": np.concatenate([g["eps"], g["var_log"]], 1), "learned_range": np.concatenate([g["eps"], g["var_values"]], 1)}.get(var_type, g["eps"])
    bad = []

    def check(tag, got, want, d_ref):
        err, lim = _report(tag, got.cpu().numpy(), want, d_ref)
        if not err <= lim:
            bad.append((tag, err, lim))
    for si, ts in enumerate(g["t_sets"]):
        t = dev(ts)
        for clip in (0, 1):
            r = d._vb_terms_bpd(_frozen(out), dev(g["x_start"]), dev(g["x_t"]), t, clip_denoised=bool(clip), model_kwargs={})
            tag = f"{var_type}.s{si}.c{clip}"
            assert r["output"].shape == (2,) and r["pred_xstart"].shape == g["x_t"].shape
            check(f"method.{tag}.vb", r["output"], g[f"{tag}.vb"], g[f"{tag}.vb.d_ref"])
            check(f"method.{tag}.pred_xstart", r["pred_xstart"], g[f"s{si}.c{clip}.pred_xstart"], g[f"s{si}.c{clip}.pred_xstart.d_ref"])
            rv = d.ddim_reverse_sample(_frozen(out), dev(g["x_t"]), t, clip_denoised=bool(clip), model_kwargs={})
            check(f"method.{tag}.reverse.sample", rv["sample"], s[f"s{si}.c{clip}.sample"], s[f"s{si}.c{clip}.sample.d_ref"])
            check(f"method.{tag}.reverse.pred_xstart", rv["pred_xstart"], g[f"s{si}.c{clip}.pred_xstart"], g[f"s{si}.c{clip}.pred_xstart.d_ref"])
        xp = d._predict_xstart_from_xprev(dev(g["x_t"]), t, dev(g["xprev"]))
        check(f"method.s{si}.xstart_from_xprev", xp, s[f"s{si}.xstart_from_xprev"], s[f"s{si}.xstart_from_xprev.d_ref"])
    check("method.prior_bpd", d._prior_bpd(dev(g["x_start"])), g["prior_bpd"], g["prior_bpd.d_ref"])
    with pytest.raises(AssertionError):
        d.ddim_reverse_sample(_frozen(out), dev(g["x_t"]), dev(g["t_sets"][0]), eta=1.0)
    assert not bad, bad


@pytest.mark.parametrize("E,var_type,chain", [(8192, "fixed_large", "ddim50"), (8192, "learned_range", "250"), (262144, "fixed_small", "1000"),
                                              (262144, "learned", "ddim50")])
def test_vb_terms_at_large_shapes_is_exact_repeatable_and_batch_invariant(E, var_type, chain):
    """E = 8192 / 262144, N = 1, 3, 68 against the fp64 restatement (floor bound 1e-6: unrelated random inputs, so the decoder term's
    1e-12 clamps are hit); row b of N = 68 bitwise equal to the sample launched alone; 20 launches bitwise equal."""
    d = er.diffusion(chain, var_type)
    T = d.num_timesteps
    rng = np.random.RandomState(E % 1000 + len(var_type))
    N = 68
    shape = (N, 4, E // 64, 16)
    x_start = np.clip(rng.randn(*shape) * 0.8, -1, 1).astype(F32)
    x_t, eps, noise = (rng.randn(*shape).astype(F32) for _ in range(3))
    x_t[::2] = (x_start[::2] + 0.02 * x_t[::2]).astype(F32)                # every other sample near its source (a small-t q_sample)
    vv = {"learned": (-4 + 2 * rng.uniform(-1, 1, size=shape)).astype(F32), "learned_range": rng.uniform(-1, 1, size=shape).astype(F32)}.get(var_type)
    t = rng.randint(0, T, size=N).astype(np.int64)
    t[[0, 2, 5, 67]] = [0, 0, T - 1, 0]
    clip = E == 8192
    full = _vb_kernel(d, var_type, x_start, x_t, eps, noise, t, clip, vv)
    bad = []
    for n in (1, 3, 68):
        sl = slice(0, n)
        r = full if n == N else _vb_kernel(d, var_type, x_start[sl], x_t[sl], eps[sl], noise[sl], t[sl], clip, None if vv is None else vv[sl])
        ref = er.vb_terms(d, var_type, x_start[sl], x_t[sl], eps[sl], noise[sl], t[sl], clip, var_values=None if vv is None else vv[sl])
        for k in ("vb", "xstart_mse", "mse", "pred_xstart"):
            err, lim = _report(f"large.E{E}.N{n}.{var_type}.{k}", r[k], ref[k], 0.0)
            if not err <= lim:
                bad.append((n, k, err, lim))
        for k in ("vb", "xstart_mse", "mse"):
            assert np.array_equal(r[k], full[k][sl]), (n, k)                   # a sample's numbers do not depend on N
    for b in (2, 5, 41, 67):                                                   # ... nor on its row
        sl = slice(b, b + 1)
        r = _vb_kernel(d, var_type, x_start[sl], x_t[sl], eps[sl], noise[sl], t[sl], clip, None if vv is None else vv[sl])
        for k in ("vb", "xstart_mse", "mse", "pred_xstart"):
            assert np.array_equal(r[k], full[k][sl]), (b, k)
    sl = slice(0, 3 if E > 8192 else N)
    for _ in range(20):
        r = _vb_kernel(d, var_type, x_start[sl], x_t[sl], eps[sl], noise[sl], t[sl], clip, None if vv is None else vv[sl])
        assert all(np.array_equal(r[k], full[k][sl]) for k in r)
    assert not bad, bad


@pytest.mark.parametrize("mean_type", ["START_X", "PREVIOUS_X"])
def test_vb_terms_of_the_other_mean_types(mean_type):
    """a network that predicts x_0 or x_{t-1}: the KL / decoder term uses the model MEAN (for PREVIOUS_X the raw output), the errors the
    x0 estimate; against the restatement (no reference result is stored for these: floor bound 1e-6, for PREVIOUS_X see below)"""
    from gpu_util import dev
    g = load_golden("eval_terms")
    d = er.diffusion("8", "fixed_large", mean_type)
    x0_net = (g["x_start"] + 0.01 * g["eps"]).astype(F32)
    bad = []
    for ts in g["t_sets"]:
        if mean_type == "START_X":
            out, kw = x0_net, dict(model_xstart=x0_net)
        else:
            out = (er.tab(d.posterior_mean_coef1, ts, x0_net) * x0_net + er.tab(d.posterior_mean_coef2, ts, x0_net) * g["x_t"]).astype(F32)
            kw = dict(model_mean=out, model_xstart=er.xstart_from_xprev(d, g["x_t"], ts, out))
        ref = er.vb_terms(d, "fixed_large", g["x_start"], g["x_t"], None, g["noise"], ts, True, **kw)
        d_ref = dict.fromkeys(ref, 0.0)
        if mean_type == "PREVIOUS_X":
            # x0 = xprev / coef1 - coef2 / coef1 x_t is formed in fp32 like the reference forms it (_predict_xstart_from_xprev; the value
            # p_sample returns as pred_xstart), two terms up to 10x the result at the last index: d_ref is that fp32 formula's own
            # deviation, here restated in numpy float32, and the bound is the issue's max(4 d_ref, 1e-6)
            a = (1.0 / d.posterior_mean_coef1)[ts].astype(F32).reshape(-1, 1, 1, 1)
            b = (d.posterior_mean_coef2 / d.posterior_mean_coef1)[ts].astype(F32).reshape(-1, 1, 1, 1)
            ref32 = er.vb_terms(d, "fixed_large", g["x_start"], g["x_t"], None, g["noise"], ts, True, model_mean=out, model_xstart=a * out - b * g["x_t"])
            d_ref = {k: er.rel_to_max(ref32[k], ref[k]) for k in ref}
        t = dev(ts)
        r = d._vb_terms_bpd(_frozen(out), dev(g["x_start"]), dev(g["x_t"]), t, clip_denoised=True, model_kwargs={})
        eps = d.p_mean_variance(_frozen(out), dev(g["x_t"]), t, clip_denoised=True, model_kwargs={})["eps"]
        v, xm, em, x0 = d._vb_terms(dev(g["x_start"]), dev(g["x_t"]), eps, dev(g["noise"]), t, True)
        assert torch.equal(v, r["output"])
        for k, got in (("vb", v), ("xstart_mse", xm), ("mse", em), ("pred_xstart", x0)):
            err, lim = _report(f"{mean_type}.t{tuple(int(v) for v in ts)}.{k}", got.cpu().numpy(), ref[k], d_ref[k])
            if not err <= lim:
                bad.append((tuple(ts), k, err, lim))
    assert not bad, bad


def _ls_dit(seed, final_std):
    from gpu_util import load_module
    from guided_diffusion.dit import DiTRotary
    m = DiTRotary(input_size=[128, 16], patch_size=8, in_channels=4, hidden_size=384, depth=2, num_heads=6, num_classes=3, learn_sigma=True)
    return load_module(m, synth.dit_state_dict(seed, final_std=final_std, **dict(SM, out_ch=8)))


def _bpd_setup(g, prefix):
    from guided_diffusion.script_util import create_diffusion
    learn = bool(prefix)
    d = create_diffusion(learn_sigma=learn, diffusion_steps=1000, noise_schedule="linear", timestep_respacing="8", use_kl=False,
                         predict_xstart=False, rescale_timesteps=False, rescale_learned_sigmas=False)
    m = _ls_dit(int(g["ls.seed"][0]), float(g["ls.final_std"][0])) if learn else _dit(SM, int(g["seed"][0]))
    return d, m


KEYS = ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse")


@pytest.mark.parametrize("prefix", ["", "ls."])
def test_calc_bpd_loop_on_the_reference_outputs_matches_fp64(prefix):
    """(a) the reference's stored model outputs in place of the network: all five outputs within the bound of the fixture's fp64
    values; (d) shapes and column order as the reference's (column 0 = the last timestep)"""
    from gpu_util import dev
    g = load_golden("eval_bpd")
    d, _ = _bpd_setup(g, prefix)
    _inject(d, *g[prefix + "noise"])
    seen = []

    def model(x, t, **kw):
        seen.append(t.cpu().numpy().copy())
        return frozen(x, t, **kw)
    frozen = _frozen(*g[prefix + "model_out"])
    r = d.calc_bpd_loop(model, dev(g[prefix + "x_start"]), clip_denoised=True, model_kwargs={"y": dev(g[prefix + "y"])})
    tm = d.timestep_map
    assert [int(s[0]) for s in seen] == [tm[i] for i in range(8)[::-1]]                 # descending, re-spaced: the network sees timestep_map[t]
    bad = []
    for k in KEYS:
        assert tuple(r[k].shape) == g[f"{prefix}f64.{k}"].shape == ((2,) if k.endswith("bpd") else (2, 8))
        err, lim = _report(f"bpd.{prefix}{k}", r[k].cpu().numpy(), g[f"{prefix}f64.{k}"], g[f"{prefix}f64.{k}.d_ref"])
        if not err <= lim:
            bad.append((k, err, lim))
    assert not bad, bad


@pytest.mark.parametrize("prefix", ["", "ls."])
def test_calc_bpd_loop_with_our_network(prefix, precision):
    """(b) every step's network output within the forward contract of the reference's stored output; (c) the loop bitwise equal to
    _vb_terms_bpd and the error terms called by hand per step with _t_host unset; the deviation of total_bpd from the reference's is
    printed, not asserted (a quadratic function of (b))"""
    from gpu_util import dev, rel
    g = load_golden("eval_bpd")
    d, m = _bpd_setup(g, prefix)
    mf = _model_fn(m)
    outs = []

    def rec(x, t, **kw):
        o = mf(x, t, **kw)
        outs.append(o.clone())
        return o
    _inject(d, *g[prefix + "noise"])
    xs, kw = dev(g[prefix + "x_start"]), {"y": dev(g[prefix + "y"])}
    r = d.calc_bpd_loop(rec, xs, clip_denoised=True, model_kwargs=kw)
    assert len(outs) == 8
    for j, o in enumerate(outs):
        e = rel(o.cpu().numpy(), g[prefix + "model_out"][j])
        print(f"EVAL bpd.{prefix}step{j}.{precision}: network output rel {e:.3e}")
        assert e < TOL, (j, e)
    for k in KEYS:
        print(f"EVAL bpd.{prefix}{k}.{precision}: deviation from the reference's fp32 {er.rel_to_max(r[k].cpu().numpy(), g[f'{prefix}ref.{k}']):.3e}")
    # by hand, the conditioning computed ahead off (_t_host unset)
    assert d._t_host is None
    for j, i in enumerate(range(8)[::-1]):
        t = torch.full((2,), i, dtype=torch.int64, device="cuda")
        nz = dev(g[prefix + "noise"][j])
        x_t = d.q_sample(xs, t, noise=nz)
        hand = d._vb_terms_bpd(mf, xs, x_t, t, clip_denoised=True, model_kwargs=kw)
        assert torch.equal(hand["output"], r["vb"][:, j]), j
        eps = d.p_mean_variance(mf, x_t, t, clip_denoised=True, model_kwargs=kw)["eps"]
        _, xm, em, x0 = d._vb_terms(xs, x_t, eps, nz, t, True)
        assert torch.equal(xm, r["xstart_mse"][:, j]) and torch.equal(em, r["mse"][:, j]) and torch.equal(x0, hand["pred_xstart"]), j
    assert torch.equal(r["total_bpd"], r["vb"].sum(dim=1) + r["prior_bpd"]) and torch.equal(r["prior_bpd"], d._prior_bpd(xs))


def test_ddim_inversion_matches_reference(precision):
    from gpu_util import dev, rel
    g = load_golden("eval_invert")
    m = _dit(SM, int(g["seed"][0]))
    d = _diffusion("ddim50")
    mf, kw = _model_fn(m), {"y": dev(g["y"])}
    xs = dev(g["x_start"])
    first = d.ddim_reverse_sample(mf, xs, torch.zeros(2, dtype=torch.int64, device="cuda"), clip_denoised=False, model_kwargs=kw)
    e1, e2 = rel(first["sample"].cpu().numpy(), g["first_sample"]), rel(first["pred_xstart"].cpu().numpy(), g["first_pred_xstart"])
    n = int(g["steps"][0])
    lat = d.ddim_reverse_sample_loop(mf, xs, num_steps=n + 1, clip_denoised=False, model_kwargs=kw)
    e3 = rel(lat.cpu().numpy(), g["latent"])
    print(f"EVAL invert.{precision}: first sample {e1:.3e} pred_xstart {e2:.3e}; latent after {n} steps {e3:.3e}")
    assert e1 < 5e-4 and e2 < 5e-4
    assert e3 < 1e-3
    img = xs
    for i in range(n):
        img = d.ddim_reverse_sample(mf, img, torch.full((2,), i, dtype=torch.int64, device="cuda"), clip_denoised=False, model_kwargs=kw)["sample"]
    assert torch.equal(img, lat)
    # the whole chain by default: 49 steps, the latent at index 49
    assert d.ddim_reverse_sample_loop(_frozen(np.zeros((2, 4, 128, 16), F32)), xs).shape == xs.shape


def test_long_excerpt_inversion_and_vb_term(precision):
    """H = 256 (512 tokens: the streaming attention): one reverse step and one _vb_terms_bpd equal the kernels applied by hand to
    p_mean_variance(...)['eps'], bitwise"""
    m = _dit(SM, 11)
    d = _diffusion("ddim50")
    mf = _model_fn(m)
    gen = torch.Generator().manual_seed(5)
    xs = (torch.randn(2, 4, 256, 16, generator=gen) * 0.5).cuda()
    x_t = (xs + 0.3 * torch.randn(2, 4, 256, 16, generator=gen).cuda())
    t = torch.tensor([7, 0], device="cuda")
    kw = {"y": torch.tensor([1, 2], device="cuda")}
    eps = d.p_mean_variance(mf, x_t, t, clip_denoised=True, model_kwargs=kw)["eps"]
    assert eps.shape == x_t.shape and bool(torch.isfinite(eps).all())
    rv = d.ddim_reverse_sample(mf, x_t, t, clip_denoised=True, model_kwargs=kw)
    s, x0 = d._ddim_reverse_step(x_t, eps, t, True)
    assert torch.equal(rv["sample"], s) and torch.equal(rv["pred_xstart"], x0)
    vb = d._vb_terms_bpd(mf, xs, x_t, t, clip_denoised=True, model_kwargs=kw)
    v, _, _, x0v = d._vb_terms(xs, x_t, eps, None, t, True, want_mse=False)
    assert torch.equal(vb["output"], v) and torch.equal(vb["pred_xstart"], x0v) and bool(torch.isfinite(v).all())


def test_edit_cli_starts_from_the_ddim_inversion(tmp_path, monkeypatch):
    from guided_diffusion.gaussian_diffusion import GaussianDiffusion
    from test_gpu_cli import CFG, COMMON
    monkeypatch.chdir(tmp_path)
    spec = importlib.util.spec_from_file_location("edit_cli_inv", os.path.join(PKG, "scripts", "edit.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    cfg = os.path.join(str(tmp_path), "configs", "edit", "nd_short.yml")
    os.makedirs(os.path.dirname(cfg))
    open(cfg, "w").write(open(os.path.join(CFG, "edit", "nd_scg_given_target.yml")).read().replace("noise_level: 500", "noise_level: 12"))
    args = ["--config_path", cfg, "--batch_size", "2", "--num_samples", "2", "--diffusion_steps", "24", "--allow_synthetic_source", "True"] + COMMON
    seen = {}
    loop, inv = GaussianDiffusion._loop, GaussianDiffusion.ddim_reverse_sample_loop

    def spy_loop(self, step_fn, model, shape, noise, *a, **k):
        seen["noise"] = noise
        return loop(self, step_fn, model, shape, noise, *a, **k)

    def spy_inv(self, model, x_start, **k):
        seen["inv_kwargs"] = k
        seen["inv"] = inv(self, model, x_start, **k)
        # by hand: 11 reverse steps at chain indices 0 .. 10 on the same inputs
        img = x_start.float()
        for i in range(int(k["num_steps"]) - 1):
            img = self.ddim_reverse_sample(model, img, torch.full((img.shape[0],), i, dtype=torch.int64, device=img.device),
                                           clip_denoised=k["clip_denoised"], model_kwargs=k["model_kwargs"])["sample"]
        seen["hand"] = img
        return seen["inv"]
    monkeypatch.setattr(GaussianDiffusion, "_loop", spy_loop)
    monkeypatch.setattr(GaussianDiffusion, "ddim_reverse_sample_loop", spy_inv)

    def run(extra):
        torch.manual_seed(1234)
        seen.clear()
        return cli.main(args + extra)
    res_i, sample_i = run(["--edit_start", "ddim_inversion"])
    assert seen["inv_kwargs"]["num_steps"] == 12
    assert seen["noise"] is seen["inv"] and torch.equal(cli.LAST_START, seen["inv"]) and torch.equal(seen["hand"], seen["inv"])
    assert seen["inv"].shape == (2, 4, 128, 16) and bool(torch.isfinite(seen["inv"]).all())
    out_dir = os.path.join("loggings", "edit_demo", "edit", "nd_short_cls_1_synthsrc_inv")
    assert json.load(open(os.path.join(out_dir, "run_metadata.json")))["edit_start"] == "ddim_inversion"
    assert sample_i.shape == (2, 128, 1024, 3) and np.isfinite(res_i["note_density.loss"]).all()
    res_d, sample_d = run([])
    assert seen["noise"] is None and "inv" not in seen and cli.LAST_START is None
    res_n, sample_n = run(["--edit_start", "noise"])
    assert torch.equal(sample_d, sample_n) and res_d["note_density.loss"].tolist() == res_n["note_density.loss"].tolist()
    plain = os.path.join("loggings", "edit_demo", "edit", "nd_short_cls_1_synthsrc")
    assert json.load(open(os.path.join(plain, "run_metadata.json")))["edit_start"] == "noise"
