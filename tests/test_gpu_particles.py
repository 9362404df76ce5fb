"""-m gpu: particle rule guidance -- rgm_particle_resample and rgm_gather_rows (csrc/particles.hip) against the float64 restatement of
tests/particles_ref.py, and GaussianDiffusion.particle_sample_loop against the plain loops, a chain made by hand, the restatement's
run on the Gaussian data model, the synthetic network with its decoder and rule, and the CLI.

Ancestors, the resampling flag and the gathered r_prev are demanded exactly (the case builder keeps every threshold 1e-9 from every
cumulative weight and every ESS 1e-9 n from its threshold); ESS (relative) and the log-weights (absolute) within (n + 8) 2^-52 of the
restatement: two ulp per exp plus an n-term non-negative sum.  The bound comes from the restatement, never from the kernel."""
import ctypes as C
import importlib.util
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dpmpp_ref as R
import particles_ref as P
from conftest import PKG

pytestmark = pytest.mark.gpu
F32 = np.float32


def _resample(reward, logw, r_prev, lam, ess, u=None, seed=0, counter=0):
    """one launch on copies of the inputs -> (status, dict of numpy outputs)"""
    from gpu_util import dev
    from rgm import native as N
    n, B = reward.shape
    rw, lw, rp = dev(reward.astype(F32)), dev(np.asarray(logw, np.float64)), dev(np.asarray(r_prev, F32))
    uu = dev(np.asarray(u, np.float64)) if u is not None else None
    anc = torch.full((n, B), -7, dtype=torch.int32, device="cuda")
    ess_out = torch.full((B,), -7.0, dtype=torch.float64, device="cuda")
    flag = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    st = N.lib.rgm_particle_resample(N.ptr(rw), N.ptr(lw), N.ptr(rp), float(lam), float(ess), N.ptr(uu), C.c_uint64(seed),
                                     C.c_uint64(counter), N.ptr(anc), N.ptr(ess_out), N.ptr(flag), n, B, N.current_stream())
    return st, dict(anc=anc.cpu().numpy(), logw=lw.cpu().numpy(), r_prev=rp.cpu().numpy(), ess=ess_out.cpu().numpy(),
                    resampled=flag.cpu().numpy())


def _run_case(c, cols=None):
    sel = slice(None) if cols is None else cols
    st, out = _resample(c["reward"][:, sel], c["logw"][:, sel], c["r_prev"][:, sel], c["lam"], c["ess"], c["u"][sel])
    assert st == 0
    return out


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


@pytest.mark.parametrize("B", P.BS)
@pytest.mark.parametrize("n", P.NS)
def test_kernel_matches_the_restatement_on_every_case(n, B):
    tol = P.tolerance(n)
    worst_e = worst_l = 0.0
    for c in P.cases(n, B):
        out, ref = _run_case(c), c["ref"]
        tag = (c["name"], c["ess"], n, B)
        assert np.array_equal(out["resampled"], ref["resampled"]), tag
        assert np.array_equal(out["anc"], ref["anc"]), tag
        assert np.array_equal(out["r_prev"], ref["r_prev"], equal_nan=True), tag
        live = ref["ess"] > 0
        e = np.abs(out["ess"][live] - ref["ess"][live]) / ref["ess"][live] if live.any() else np.zeros(1)
        assert np.array_equal(out["ess"][~live], ref["ess"][~live]), tag
        fin = np.isfinite(ref["logw"])
        assert np.array_equal(out["logw"][~fin], ref["logw"][~fin]), tag            # the dead stay at -inf
        l = np.abs(out["logw"][fin] - ref["logw"][fin])
        worst_e, worst_l = max(worst_e, float(e.max())), max(worst_l, float(l.max()) if l.size else 0.0)
        assert e.max() <= tol, (tag, e.max(), tol)
        assert (l.max() if l.size else 0.0) <= tol, (tag, l.max(), tol)
    print(f"[particles n={n} B={B}] worst ESS error {worst_e / 2.0 ** -52:.1f}, worst log-weight error {worst_l / 2.0 ** -52:.1f} "
          f"(bound {n + 8}) x 2^-52")


def test_kernel_repeats_bitwise_and_a_group_does_not_depend_on_its_batch():
    for n in (3, 65, 1024):
        for c in P.cases(n, 257):
            first = _run_case(c)
            if c["name"] in ("utop", "dominant"):
                for _ in range(19):
                    assert _same(first, _run_case(c))
            for b in (0, 100, 256):                                                 # the group alone
                alone = _run_case(c, slice(b, b + 1))
                assert all(np.array_equal(alone[k][..., 0], first[k][..., b], equal_nan=True) for k in first), (c["name"], n, b)


def test_argument_errors_launch_nothing():
    from rgm import native as N
    n, B = 4, 3
    z = np.zeros((n, B))
    for kw in (dict(n=0), dict(n=1025), dict(B=0), dict(lam=float("nan")), dict(lam=float("inf")), dict(ess=float("nan"))):
        rw = torch.zeros(1030 * 3, device="cuda")
        lw = torch.full((1030 * 3,), 5.0, dtype=torch.float64, device="cuda")
        rp = torch.full((1030 * 3,), 5.0, device="cuda")
        anc = torch.full((1030 * 3,), -7, dtype=torch.int32, device="cuda")
        es = torch.full((B,), -7.0, dtype=torch.float64, device="cuda")
        fl = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        st = N.lib.rgm_particle_resample(N.ptr(rw), N.ptr(lw), N.ptr(rp), kw.get("lam", 1.0), kw.get("ess", 0.5), None, C.c_uint64(0), C.c_uint64(0),
                                         N.ptr(anc), N.ptr(es), N.ptr(fl), kw.get("n", n), kw.get("B", B), N.current_stream())
        torch.cuda.synchronize()
        assert st != 0 and N.lib.rgm_last_error(), kw
        assert (lw == 5.0).all() and (rp == 5.0).all() and (anc == -7).all() and (es == -7.0).all() and (fl == -7).all(), kw
    st, _ = _resample(z.astype(F32), z, z.astype(F32), 1.0, 0.5)
    assert st == 0
    assert N.lib.rgm_particle_resample(None, None, None, 1.0, 0.5, None, C.c_uint64(0), C.c_uint64(0), None, None, None, n, B, N.current_stream()) != 0
    src = torch.arange(n * B * 8, dtype=torch.float32, device="cuda")
    dst = torch.full_like(src, -7.0)
    a = torch.zeros(n * B, dtype=torch.int32, device="cuda")
    for args in ((N.ptr(src), N.ptr(src), N.ptr(a), n, B, 8), (N.ptr(src), N.ptr(dst), N.ptr(a), 0, B, 8), (N.ptr(src), N.ptr(dst), N.ptr(a), n, B, 0),
                 (N.ptr(src), C.c_void_p(src.data_ptr() + 64), N.ptr(a), n, B, 8), (None, N.ptr(dst), N.ptr(a), n, B, 8)):
        assert N.lib.rgm_gather_rows(*args, N.current_stream()) != 0
    torch.cuda.synchronize()
    assert (dst == -7.0).all() and torch.equal(src, torch.arange(n * B * 8, dtype=torch.float32, device="cuda"))


def test_philox_offsets_are_the_generators_first_word():
    """65536 groups whose weights read u back through the ancestor of particle 0 (particles_ref.ladder_rewards): every ancestor equals
    the restatement's under u = (w0 + 0.5) 2^-32 of the numpy Philox, so u lies in [0, 1); its mean is within 5 standard errors of 1/2;
    and a group's draw depends on (seed, counter + b) alone"""
    n, B, rungs, seed = 64, 65536, 32, 0x1234567890ABCDEF
    reward = P.ladder_rewards(n, B, rungs)
    z = np.zeros((n, B))
    for counter in range(1000, 20000, 1000):                                        # the builder's rule: keep the margin, else move on
        u = P.philox_u(seed, counter, B)
        ref = P.resample(reward, z, z.astype(F32), 1.0, 2.0, u)
        if ref["margin_c"].min() >= P.MARGIN:
            break
    assert ref["margin_c"].min() >= P.MARGIN and (u >= 0).all() and (u < 1).all()
    st, out = _resample(reward, z, z.astype(F32), 1.0, 2.0, None, seed, counter)
    assert st == 0 and np.array_equal(out["anc"], ref["anc"]) and (out["resampled"] == 1).all()
    back = (out["anc"][0] + 0.5) / rungs                                            # u to 1 / 32, centred
    assert np.abs(back - u).max() <= 1.0 / rungs                                    # (the float32 rewards move a rung by parts in 10^7)
    se = np.sqrt(1.0 / 12.0 / B)
    print(f"[particles philox] mean of the offsets read back {back.mean():.5f} (5 standard errors: {5 * se:.5f})")
    assert abs(back.mean() - 0.5) <= 5 * se
    # the same counters in another launch shape, and shifted by one group
    st, sub = _resample(reward[:, :300], z[:, :300], z[:, :300].astype(F32), 1.0, 2.0, None, seed, counter + 7)
    assert st == 0 and np.array_equal(sub["anc"][:, :293], out["anc"][:, 7:300])
    st, other = _resample(reward[:, :300], z[:, :300], z[:, :300].astype(F32), 1.0, 2.0, None, seed + 1, counter)
    assert not np.array_equal(other["anc"][0], out["anc"][0, :300])


@pytest.mark.parametrize("E", [4, 6, 8192, 8198])
def test_gather_rows_is_bitwise(E):
    from guided_diffusion.gaussian_diffusion import GaussianDiffusion
    n, B = 5, 3
    rng = np.random.RandomState(E)
    src = torch.from_numpy(rng.randn(n * B, E).astype(F32)).cuda()
    src.view(torch.int32)[0, :3] = torch.tensor([0x7FC00001, -8388608, -2147483648], dtype=torch.int32, device="cuda")   # NaN payload, -inf, -0
    ar = torch.arange(B, device="cuda")
    for name, anc in (("identity", np.tile(np.arange(n)[:, None], (1, B))), ("one", np.full((n, B), 3)),
                      ("permutation", np.stack([rng.permutation(n) for _ in range(B)], axis=1)), ("random", rng.randint(0, n, size=(n, B)))):
        a = torch.from_numpy(anc.astype(np.int32)).cuda()
        out = GaussianDiffusion._gather_rows(src, a)
        want = src.view(n, B, E)[a.long(), ar[None, :]].reshape(n * B, E)
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)), (name, E)
    if E == 8198:                                                                   # rows of a 4-multiple on a base that is not 16-byte aligned
        big = torch.from_numpy(rng.randn(n * B * 8 + 1).astype(F32)).cuda()
        off = big[1:].view(n * B, 8)
        out = GaussianDiffusion._gather_rows(off, a) if off.is_contiguous() else None
        assert torch.equal(out, off.view(n, B, 8)[a.long(), ar[None, :]].reshape(n * B, 8))


# ------------------------------------------------------------------------------------ the loop
def _diffusion(rs):
    from guided_diffusion.script_util import create_diffusion
    return create_diffusion(learn_sigma=False, diffusion_steps=1000, noise_schedule="linear", timestep_respacing=rs,
                            use_kl=False, predict_xstart=False, rescale_timesteps=False, rescale_learned_sigmas=False)


class _GaussianEps:
    """eps of dpmpp_ref.GaussianModel on the device (float64 inside), called with ORIGINAL timesteps"""

    def __init__(self, gm, shape):
        self.mu = torch.from_numpy(gm.mu).cuda().view(shape)
        self.s = torch.from_numpy(gm.s).cuda().view(shape)
        self.ac = torch.from_numpy(R.linear_alphas_cumprod()).cuda()

    def __call__(self, x, t, **kw):
        a = self.ac[t].view(-1, 1, 1, 1)
        return ((1 - a).sqrt() * (x.double() - a.sqrt() * self.mu) / (a * self.s ** 2 + 1 - a)).float()


SHAPE = (3, 2, 8, 16)
TARGET, TAU = -0.4, 0.35


def _reward(x0, t):
    return -(x0[:, 0, 0, 0] - TARGET) ** 2 / (2 * TAU ** 2)


def _cond(x, t, **kw):
    return -0.3 * (x - 0.1)


def _u_half(i, B):
    return torch.full((B,), 0.5, dtype=torch.float64, device="cuda")


def _plain(d, sampler, model, shape, cond):
    gk = SimpleNamespace(schedule=False, method="classifier_guidance") if cond else None
    kw = dict(clip_denoised=False, cond_fn=_cond if cond else None, guidance_kwargs=gk, model_kwargs={}, device="cuda")
    if sampler == "ddpm":
        return d.p_sample_loop(model, shape, **kw)
    if sampler == "ddim":
        return d.ddim_sample_loop(model, shape, eta=1.0, **kw)
    return d.dpmpp_sample_loop(model, shape, order=2, eta=1.0, **kw)


@pytest.mark.parametrize("cond", [False, True])
@pytest.mark.parametrize("sampler,rs", [("ddpm", "25"), ("ddim", "ddim25"), ("dpmpp", "logsnr12")])
def test_one_particle_is_the_plain_loop(sampler, rs, cond):
    from guided_diffusion.gaussian_diffusion import PhiloxNoise
    d = _diffusion(rs)
    model = _GaussianEps(R.GaussianModel(256, 0), SHAPE[1:])
    d.noise = PhiloxNoise(seed=5)
    want = _plain(d, sampler, model, SHAPE, cond)
    d.noise = PhiloxNoise(seed=5)
    got = d.particle_sample_loop(model, SHAPE, 1, sampler=sampler, clip_denoised=False, cond_fn=_cond if cond else None, reward_fn=_reward,
                                 u_fn=_u_half, device="cuda")
    assert torch.equal(got["sample"], want) and torch.equal(got["best"], want)
    assert (got["log_weights"] == 0).all() and (got["max_ind"] == 0).all()


@pytest.mark.parametrize("sampler,rs", [("ddpm", "25"), ("dpmpp", "logsnr12")])
def test_lambda_zero_is_the_plain_loop_at_batch_n_b(sampler, rs):
    from guided_diffusion.gaussian_diffusion import PhiloxNoise
    d = _diffusion(rs)
    model = _GaussianEps(R.GaussianModel(256, 0), SHAPE[1:])
    n = 4
    d.noise = PhiloxNoise(seed=6)
    want = _plain(d, sampler, model, (n * SHAPE[0],) + SHAPE[1:], False)
    d.noise = PhiloxNoise(seed=6)
    got = d.particle_sample_loop(model, SHAPE, n, sampler=sampler, particle_kwargs={"lambda": 0.0}, clip_denoised=False, reward_fn=_reward,
                                 u_fn=_u_half, device="cuda")
    assert torch.equal(got["sample"], want)
    assert (got["log_weights"] == 0).all() and (got["resampled_steps"] == 0).all()
    assert torch.equal(got["reward"].reshape(-1), _reward(want, None).float())


def test_loop_is_the_chain_made_by_hand_and_repeats():
    """6 steps of DPM-Solver++: forward, kernel, gather, step -- by hand from the public pieces, with the Philox offsets"""
    from guided_diffusion.gaussian_diffusion import PhiloxNoise
    from gpu_util import dev
    d = _diffusion("logsnr6")
    assert d.num_timesteps == 6
    model = _GaussianEps(R.GaussianModel(256, 0), SHAPE[1:])
    n, B = 4, SHAPE[0]
    rows = (n * B,) + SHAPE[1:]
    pk = {"lambda": 3.0, "ess": 0.9}
    runs = []
    for _ in range(2):
        d.noise = PhiloxNoise(seed=8)
        runs.append(d.particle_sample_loop(model, SHAPE, n, sampler="dpmpp", particle_kwargs=pk, clip_denoised=False, reward_fn=_reward, device="cuda"))
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0])
    assert runs[0]["resampled_steps"].sum().item() > 0
    d.noise = PhiloxNoise(seed=8)
    d.t_end = 0
    wm = d._wrap_model(model)
    x = d._draw(rows, "cuda")
    state = dict(n=n, B=B, logw=torch.zeros(n * B, dtype=torch.float64, device="cuda"), r_prev=torch.zeros(n * B, device="cuda"),
                 ess=torch.zeros(B, dtype=torch.float64, device="cuda"), resampled=torch.zeros(B, dtype=torch.int32, device="cuda"))
    prev, count = None, torch.zeros(B, dtype=torch.int64, device="cuda")
    for i in range(5, -1, -1):
        t = torch.full((n * B,), i, dtype=torch.int64, device="cuda")
        eps = wm(x, t)
        r = _reward(d._predict_xstart_from_eps(x, t, eps), t).float().contiguous()
        anc = d._particle_resample(state, r, 3.0, 0.9, None)
        count += state["resampled"] == 1
        ar = torch.arange(B, device="cuda")[None, :]
        take = lambda v: v.view((n, B) + SHAPE[1:])[anc.long(), ar].reshape(rows).contiguous()
        x, eps, prev = take(x), take(eps), (None if prev is None else take(prev))
        x, prev, _ = d._dpm_step(x, eps, None, prev, d._draw(rows, "cuda"), t, False, order=2, eta=1.0)
    assert torch.equal(x, runs[0]["sample"]) and torch.equal(count, runs[0]["resampled_steps"])


def test_loop_runs_without_a_host_sync():
    from guided_diffusion.gaussian_diffusion import PhiloxNoise
    d = _diffusion("logsnr6")
    model = d._wrap_model(_GaussianEps(R.GaussianModel(256, 0), SHAPE[1:]))   # wrapped once: a wrapper uploads its timestep map on first use
    kw = dict(sampler="dpmpp", particle_kwargs={"lambda": 3.0, "ess": 0.9}, clip_denoised=False, reward_fn=_reward,
              cond_fn=d._wrap_model(_cond), device="cuda")
    d.noise = PhiloxNoise(seed=9)
    d.particle_sample_loop(model, SHAPE, 4, **kw)                       # warm: the schedule tables and the timestep map reach the device
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = d.particle_sample_loop(model, SHAPE, 4, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(out["sample"]).all()


# ------------------------------------------------------------------------------------ the Gaussian data model
G_SHAPE, G_N = (512, 1, 8, 16), 16


@pytest.fixture(scope="module")
def cpu_gauss():
    """the restatement's run of the same chain (ddim100, eta = 1, 16 particles, 512 groups), its own noise: the weighted mean of
    element 0 with its standard error over the groups"""
    gm = R.GaussianModel(128, 0)
    ac = R.chain_alphas_cumprod(range(0, 1000, 10))
    rng = np.random.RandomState(21)
    reward = lambda x0: -(x0[:, 0] - TARGET) ** 2 / (2 * TAU ** 2)
    x, logw, _, count = P.particle_chain(ac, gm, rng.randn(G_N * 512, 128), G_N, 512, reward, lam=1.0, ess=0.5,
                                         noise=lambda i, s: rng.randn(*s), u=lambda i, B: rng.rand(B))
    g = (P.weights(logw) * x.reshape(G_N, 512, 128)[:, :, 0]).sum(axis=0)
    return gm, float(g.mean()), float(g.std(ddof=1) / np.sqrt(512))


def test_gaussian_model_chain_against_the_restatement(cpu_gauss):
    from guided_diffusion.gaussian_diffusion import PhiloxNoise
    gm, m_cpu, se_cpu = cpu_gauss
    d = _diffusion("ddim100")
    model = _GaussianEps(gm, G_SHAPE[1:])
    res = {}
    for lam in (1.0, 0.0):
        d.noise = PhiloxNoise(seed=31 + int(lam))
        out = d.particle_sample_loop(model, G_SHAPE, G_N, sampler="ddim", particle_kwargs={"lambda": lam}, clip_denoised=False,
                                     reward_fn=_reward, device="cuda")
        w = P.weights(out["log_weights"].cpu().numpy())
        xs = out["sample"].cpu().numpy().astype(np.float64).reshape(G_N, 512, 128)
        res[lam] = (w, xs, out["resampled_steps"].cpu().numpy())
    w, xs, count = res[1.0]
    g = (w * xs[:, :, 0]).sum(axis=0)
    m, se = float(g.mean()), float(g.std(ddof=1) / np.sqrt(512))
    tilted = P.tilted_gaussian(gm.mu[0], gm.s[0], TARGET, TAU, 1.0)[0]
    print(f"[particles gaussian gpu] weighted mean of element 0: {m:.4f} +- {se:.4f}, restatement {m_cpu:.4f} +- {se_cpu:.4f}, closed form "
          f"{tilted:.4f}, prior {gm.mu[0]:.4f}; groups that resampled {int((count > 0).sum())} of 512")
    assert abs(m - m_cpu) <= 5 * np.hypot(se, se_cpu)
    # element 1 is not rewarded: its weighted variance is the lambda = 0 run's
    var = {}
    for lam, (w_, x_, _) in res.items():
        v = (w_ * (x_[:, :, 1] - gm.mu[1]) ** 2).sum(axis=0)
        var[lam] = (float(v.mean()), float(v.std(ddof=1) / np.sqrt(512)))
    print(f"[particles gaussian gpu] variance of element 1: {var[1.0][0]:.5f} +- {var[1.0][1]:.5f} against {var[0.0][0]:.5f} +- {var[0.0][1]:.5f} "
          f"at lambda = 0 (prior {gm.s[1] ** 2:.5f})")
    assert abs(var[1.0][0] - var[0.0][0]) <= 5 * np.hypot(var[1.0][1], var[0.0][1])
    assert (count > 0).any() and (count == 0).any()
    assert (res[0.0][2] == 0).all()


# ------------------------------------------------------------------------------------ the network, the decoder, the rule
def test_synthetic_network_decoder_and_rule():
    from gpu_util import dev
    from conftest import load_golden
    from guided_diffusion.gaussian_diffusion import PhiloxNoise, _decode, _extract_rule
    from music_rule_guidance.rule_maps import LOSS_DICT
    from test_gpu_sampler import SM, _dit, _model_fn, _vae
    g = load_golden("steps2")
    d = _diffusion("logsnr6")
    net, vae = _model_fn(_dit(SM, 11)), _vae(2)
    n, B = 4, 2
    target = dev(g["target.note_density"])
    mk = {"y": dev(g["y"]), "rule": {"note_density": target}}
    d.noise = PhiloxNoise(seed=12)
    out = d.particle_sample_loop(net, (B, 4, 128, 16), n, sampler="dpmpp", particle_kwargs={"lambda": 0.5, "ess": 0.9, "note_density": 2.0},
                                 model_kwargs=mk, embed_model=vae, scale_factor=1.2465, clip_denoised=False, device="cuda")
    assert out["sample"].shape == (n * B, 4, 128, 16) and out["log_weights"].shape == (n, B) and out["log_weights"].dtype == torch.float64
    assert d.last_particles is out
    with torch.no_grad():
        roll = _decode(out["sample"], vae, scale_factor=1.2465)
        hand = (-LOSS_DICT["note_density"](_extract_rule("note_density", roll), target.repeat(n, 1)) * 2.0).float().view(n, B)
    assert torch.equal(out["reward"], hand)
    assert torch.equal(out["max_ind"], hand.argmax(dim=0))
    assert torch.equal(out["best"], out["sample"].view(n, B, 4, 128, 16)[out["max_ind"], torch.arange(B, device="cuda")])
    assert abs(torch.exp(out["log_weights"]).mean(dim=0) - 1).max().item() < 1e-12


# ------------------------------------------------------------------------------------ the CLI
COMMON = ["--model", "DiTRotary_B_8", "--image_size", "128", "16", "--in_channels", "4", "--scale_factor", "1.2465",
          "--class_cond", "True", "--num_classes", "3", "--class_label", "1", "--synthetic_weights", "True", "--progress", "False"]
CFG = os.path.join(PKG, "scripts", "configs", "cond_table", "single", "scg", "nd.yml")


def _script(name):
    spec = importlib.util.spec_from_file_location(name + "_cli_particles_gpu", os.path.join(PKG, "scripts", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("keep", ["best", "all", None])
def test_sample_rule_cli_with_particles(tmp_path, monkeypatch, keep):
    import pandas as pd
    monkeypatch.chdir(tmp_path)
    cli = _script("sample_rule")
    flags = [] if keep is None else ["--particles", "4", "--particle_keep", keep]
    res = cli.main(["--config_path", CFG, "--batch_size", "2", "--num_samples", "2", "--diffusion_steps", "24", "--sampler", "dpmpp",
                    "--dpmpp_steps", "4"] + flags + COMMON)
    out_dir = os.path.join("loggings", cli.output_dir_for(CFG, 1))
    meta = json.load(open(os.path.join(out_dir, "run_metadata.json")))
    table = pd.read_csv(os.path.join(out_dir, "results.csv"))
    rolls = sorted(f for f in os.listdir(out_dir) if f.endswith(".npy"))
    assert np.isfinite(res["note_density.loss"]).all()
    if keep is None:
        assert meta["particles"] is None and len(res) == 2 and len(rolls) == 2 and "particle" not in table.columns
        return
    assert meta["particles"] == {"num_particles": 4, "lambda": 1.0, "ess": 0.5, "every": 1, "keep": keep}
    assert meta["sampler"]["name"] == "dpmpp"
    if keep == "best":
        assert len(res) == 2 and len(rolls) == 2 and "particle" not in table.columns and "log_weight" not in table.columns
    else:
        assert len(res) == 8 and len(rolls) == 8
        assert table["particle"].tolist() == [0, 0, 1, 1, 2, 2, 3, 3] and np.isfinite(table["log_weight"]).all()
    roll = np.load(os.path.join(out_dir, rolls[0]))
    assert roll.shape == (3, 128, 1024) and roll.dtype == np.uint8 and roll.max() <= 127
