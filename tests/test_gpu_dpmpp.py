"""-m gpu: the DPM-Solver++(2M) step kernel (csrc/dpm.hip, rgm_dpmpp_step) and the sampler built on it (dpmpp_sample,
dpmpp_sample_loop) against the float64 restatement of tests/dpmpp_ref.py and the DDIM step the suite already pins to the reference.

Tolerance against float64, everywhere: max(4 d32, floor) relative to the largest magnitude, d32 = the deviation of the SAME restatement
evaluated in numpy float32 (floor 1e-6 for a step, 1e-5 for a chain).  It never comes from a kernel; err / d32 is printed."""
import importlib.util
import itertools
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dpmpp_ref as R
from conftest import PKG, load_golden

pytestmark = pytest.mark.gpu
F32 = np.float32
CHAINS = ["", "ddim50", "logsnr20", "8"]
SHAPES = [(1, 8192), (3, 1024), (5, 8192), (5, 1024)]


def _diffusion(rs, learn_sigma=False):
    from guided_diffusion.script_util import create_diffusion
    return create_diffusion(learn_sigma=learn_sigma, diffusion_steps=1000, noise_schedule="linear", timestep_respacing=rs,
                            use_kl=False, predict_xstart=False, rescale_timesteps=False, rescale_learned_sigmas=False)


def _rows(T, N, t_end):
    """distinct chain indices: the top index, 0 and t_end first"""
    pool = [T - 1, 0, t_end, T // 2, 1, T - 2, T // 3]
    seen = []
    for v in pool:
        if v not in seen:
            seen.append(v)
    return np.array(seen[:N], dtype=np.int64)


def _inputs(ac, t, E, seed):
    """x_t of a data point that leaves [-1, 1] here and there (the clip acts), a noisy eps estimate, gradient, earlier x0, noise"""
    rng = np.random.RandomState(seed)
    N = len(t)
    x0 = rng.uniform(-1.3, 1.3, size=(N, E))
    e = rng.randn(N, E)
    a = ac[t][:, None]
    x = (np.sqrt(a) * x0 + np.sqrt(1 - a) * e).astype(F32)
    eps = (e + 0.1 * rng.randn(N, E)).astype(F32)
    return dict(x=x, eps=eps, grad=(0.1 * rng.randn(N, E)).astype(F32), x0_prev=(x0 + 0.05 * rng.randn(N, E)).astype(F32),
                noise=rng.randn(N, E).astype(F32))


def _launch(d, inp, t, order, eta, clip, use_grad, use_noise, use_prev, t_end=0, want_g=True):
    from gpu_util import dev
    d.t_end = t_end
    s, x0, g = d._dpm_step(dev(inp["x"]), dev(inp["eps"]), dev(inp["grad"]) if use_grad else None,
                           dev(inp["x0_prev"]) if use_prev else None, dev(inp["noise"]) if use_noise else None, dev(t), clip,
                           order=order, eta=eta, want_g=want_g)
    return s, x0, g


def _ref(ac, inp, t, order, eta, clip, use_grad, use_noise, use_prev, t_end, dtype):
    return R.step(ac, inp["x"], inp["eps"], t, grad=inp["grad"] if use_grad else None, x0_prev=inp["x0_prev"] if use_prev else None,
                  noise=inp["noise"] if use_noise else None, order=order, sde=eta == 1, clip=clip, t_end=t_end, dtype=dtype)


@pytest.mark.parametrize("N,E", SHAPES)
@pytest.mark.parametrize("rs", CHAINS)
def test_kernel_matches_the_float64_restatement(rs, N, E):
    """every combination of order, eta, clip, gradient, noise and x0_prev, rows at distinct t (top index, 0, t_end among them)"""
    d = _diffusion(rs)
    ac, T = d.alphas_cumprod, d.num_timesteps
    t_end = 2
    worst = 0.0
    ts = [_rows(T, N, t_end)] if N > 1 else [np.array([v], dtype=np.int64) for v in _rows(T, 4, t_end)]
    for t in ts:
        inp = _inputs(ac, t, E, seed=N * 7 + E + len(rs))
        for order, eta, clip, ug, un, up in itertools.product((1, 2), (0.0, 1.0), (False, True), (False, True), (False, True), (False, True)):
            s, x0, g = _launch(d, inp, t, order, eta, clip, ug, un, up, t_end)
            r64 = _ref(ac, inp, t, order, eta, clip, ug, un, up, t_end, np.float64)
            r32 = _ref(ac, inp, t, order, eta, clip, ug, un, up, t_end, np.float32)
            for name, out, a, b in (("sample", s, r64[0], r32[0]), ("pred_xstart", x0, r64[1], r32[1])):
                d32, tol = R.bound(a, b)
                err = R.rel_err(out.cpu().numpy(), a)
                worst = max(worst, err / max(d32, 1e-12))
                assert err <= tol, (name, rs, N, E, t.tolist(), order, eta, clip, ug, un, up, err, d32)
            assert np.abs(g.cpu().numpy() - r64[2]).max() <= 2e-7              # the noise scale is the table's float32 entry (<= 1)
            last = torch.from_numpy(t == 0).to(s.device)
            if last.any():                                                       # the last index returns D (= x0 there) bit for bit
                assert torch.equal(s[last], x0[last])
    print(f"[dpmpp step {rs or 'full'} N={N} E={E}] worst err / d32 = {worst:.2f}")


@pytest.mark.parametrize("rs", CHAINS)
@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("use_grad", [False, True])
def test_order_one_is_the_ddim_step(rs, eta, use_grad):
    """order = 1 and rgm_ddim_step against the float64 DDIM step, each within the bound of its own float32 restatement"""
    from gpu_util import dev
    d = _diffusion(rs)
    ac, T = d.alphas_cumprod, d.num_timesteps
    N, E = 5, 8192
    t = _rows(T, N, 0)
    inp = _inputs(ac, t, E, seed=3)
    grad = inp["grad"] if use_grad else None
    ref = R.ddim_step(ac, inp["x"], inp["eps"], t, grad=grad, noise=inp["noise"], eta=eta)
    ddim32 = R.ddim_step(ac, inp["x"], inp["eps"], t, grad=grad, noise=inp["noise"], eta=eta, dtype=np.float32)
    dpm32 = R.step(ac, inp["x"], inp["eps"], t, grad=grad, noise=inp["noise"], order=1, sde=eta == 1, dtype=np.float32)
    d.t_end = 0
    a = d._step("ddim", dev(inp["x"]), dev(inp["eps"]), dev(grad) if use_grad else None, dev(inp["noise"]), dev(t), False, eta=eta,
                want_g=True)
    b = _launch(d, inp, t, 1, eta, False, use_grad, True, True)
    for name, i in (("sample", 0), ("pred_xstart", 1)):
        for who, out, r32 in (("ddim", a[i], ddim32[i]), ("dpmpp", b[i], dpm32[i])):
            d32, tol = R.bound(ref[i], r32)
            err = R.rel_err(out.cpu().numpy(), ref[i])
            print(f"[order 1 vs ddim {rs or 'full'} eta={eta} grad={use_grad}] {who} {name}: err {err:.2e}, d32 {d32:.2e}, err / d32 {err / max(d32, 1e-12):.2f}")
            assert err <= tol, (who, name, err, d32)
    assert np.abs(b[2].cpu().numpy() - ref[2]).max() <= 2e-7                   # the noise scale is DDIM's sigma (<= 1)


def test_launches_are_bitwise_repeatable_and_rows_independent():
    d = _diffusion("logsnr20")
    ac, T = d.alphas_cumprod, d.num_timesteps
    t = _rows(T, 5, 2)
    inp = _inputs(ac, t, 8192, seed=5)
    first = _launch(d, inp, t, 2, 1.0, True, True, True, True, 2)
    for _ in range(19):
        again = _launch(d, inp, t, 2, 1.0, True, True, True, True, 2)
        assert all(torch.equal(u, v) for u, v in zip(first, again))
    # a row alone, and the rows in another order and another batch size
    for rows in ([0], [3], [4, 2, 0], [4, 3, 2, 1, 0]):
        sub = {k: np.ascontiguousarray(v[rows]) for k, v in inp.items()}
        out = _launch(d, sub, t[rows], 2, 1.0, True, True, True, True, 2)
        idx = torch.tensor(rows, device=first[0].device)
        assert all(torch.equal(u[idx], v) for u, v in zip(first, out))


class _GaussianEps:
    """eps of dpmpp_ref.GaussianModel on the device (float64 inside, like the restatement's), called with ORIGINAL timesteps"""

    def __init__(self, gm, shape):
        self.mu = torch.from_numpy(gm.mu).cuda().view(shape)
        self.s = torch.from_numpy(gm.s).cuda().view(shape)
        self.ac = torch.from_numpy(R.linear_alphas_cumprod()).cuda()
        self.calls = 0

    def __call__(self, x, t, **kw):
        self.calls += 1
        a = self.ac[t].view(-1, 1, 1, 1)
        return ((1 - a).sqrt() * (x.double() - a.sqrt() * self.mu) / (a * self.s ** 2 + 1 - a)).float()


SHAPE = (4, 4, 128, 16)     # N E = 32768, E = 8192


@pytest.fixture(scope="module")
def gauss():
    gm = R.GaussianModel(8192, 0)
    xT = np.random.RandomState(1).randn(4, 8192).astype(F32)
    return gm, xT


def test_loop_is_the_same_steps_made_by_hand(gauss):
    from guided_diffusion.gaussian_diffusion import PhiloxNoise
    gm, xT = gauss
    d = _diffusion("logsnr20")
    model = _GaussianEps(gm, SHAPE[1:])
    x_T = torch.from_numpy(xT).cuda().view(SHAPE)
    for eta in (0.0, 1.0):
        d.noise = PhiloxNoise(seed=11)
        loop = d.dpmpp_sample_loop(model, SHAPE, noise=x_T, clip_denoised=False, order=2, eta=eta, device="cuda")
        d.noise = PhiloxNoise(seed=11)
        d.t_end = 0
        x, prev = x_T, None
        for i in range(d.num_timesteps - 1, -1, -1):
            out = d.dpmpp_sample(model, x, torch.full((4,), i, dtype=torch.int64, device="cuda"), x0_prev=prev, order=2, eta=eta,
                                 clip_denoised=False)
            x, prev = out["sample"], out["pred_xstart"]
        assert torch.equal(loop, x)
    assert model.calls == 4 * d.num_timesteps          # one network evaluation per step


def test_ode_chain_on_the_gaussian_model(gauss):
    gm, xT = gauss
    d = _diffusion("logsnr20")
    ac = d.alphas_cumprod
    np.testing.assert_allclose(ac, R.chain_alphas_cumprod(R.logsnr_steps(R.linear_alphas_cumprod(), 20)), rtol=1e-12)
    model = _GaussianEps(gm, SHAPE[1:])
    out = d.dpmpp_sample_loop(model, SHAPE, noise=torch.from_numpy(xT).cuda().view(SHAPE), clip_denoised=False, order=2, eta=0.0,
                              device="cuda").cpu().numpy().reshape(4, -1)
    r64 = R.chain(ac, gm, xT, order=2)
    r32 = R.chain(ac, gm, xT, order=2, dtype=np.float32)
    d32, tol = R.bound(r64, r32, floor=1e-5)
    err = R.rel_err(out, r64)
    exact = gm.exact(ac[-1], xT.astype(np.float64))
    e_gpu, e_ref = R.rel_rms(out, exact), R.rel_rms(r64, exact)
    print(f"[dpmpp ode chain logsnr20] err {err:.2e}, d32 {d32:.2e}, err / d32 {err / d32:.2f}; against the exact solution: "
          f"kernel {e_gpu:.4e}, restatement {e_ref:.4e}")
    assert err <= tol, (err, d32)
    assert e_gpu <= 1.5 * e_ref


@pytest.fixture(scope="module")
def cpu_sde_variance():
    """the restatement's standardised variance of a logsnr20 SDE chain over 2^20 elements (tests/test_dpmpp_host.py: 1.07)"""
    E = 1 << 20
    gm = R.GaussianModel(E, 0)
    rng = np.random.RandomState(2)
    ac = R.chain_alphas_cumprod(R.logsnr_steps(R.linear_alphas_cumprod(), 20))
    x = R.chain(ac, gm, np.random.RandomState(1).randn(1, E), order=2, sde=True, noise=lambda i, s: rng.randn(*s))
    return float(gm.standardised(x).var())


def test_sde_chain_variance(gauss, cpu_sde_variance):
    from guided_diffusion.gaussian_diffusion import PhiloxNoise
    gm, _ = gauss
    d = _diffusion("logsnr20")
    d.noise = PhiloxNoise(seed=2024)
    model = _GaussianEps(gm, SHAPE[1:])
    out = d.dpmpp_sample_loop(model, SHAPE, clip_denoised=False, order=2, eta=1.0, device="cuda").cpu().numpy().reshape(4, -1)
    assert out.size == 32768
    var = float(gm.standardised(out.astype(np.float64)).var())
    print(f"[dpmpp sde chain logsnr20] standardised variance {var:.4f}, restatement over 2^20 elements {cpu_sde_variance:.4f}")
    # 5 standard errors of a variance estimated from 32768 unit normals (sqrt(2 / 32768) = 0.0078) and of the CPU value's 2^20
    assert abs(var - cpu_sde_variance) <= 0.042


# ------------------------------------------------------------------------------------ the network, the decoder, SCG, the classifier
def _net():
    from test_gpu_sampler import SM, _dit, _model_fn
    return _model_fn(_dit(SM, 11))


def _scg_setup(rs="ddim50"):
    from gpu_util import dev
    from test_gpu_sampler import _vae
    g = load_golden("steps2")
    d = _diffusion(rs)
    d.t_end = 0
    nz = np.random.RandomState(int(g["dscg.noise_seed"])).randn(4, 2, 4, 128, 16).astype(F32)
    kw = dict(clip_denoised=False, eta=1.0, model_kwargs={"y": dev(g["y"]), "rule": {"note_density": dev(g["target.note_density"])}},
              embed_model=_vae(2), scale_factor=1.2465, guidance_kwargs=SimpleNamespace(method="no_guidance", schedule=True, t_start=750,
                                                                                         t_end=0, interval=1),
              scg_kwargs={"num_samples": 4, "note_density": 1.})
    return g, d, nz, kw


def test_scg_search_step_order_one_is_ddims():
    from gpu_util import dev, rel
    from test_gpu_sampler import _inject
    g, d, nz, kw = _scg_setup()
    net = _net()
    x, t = dev(g["x"]), dev(g["dscg.t"])
    _inject(d, nz)
    ref = d.ddim_sample(net, x, t, **kw)
    table, win = d.last_scg["total_log_prob"].cpu().numpy().astype(np.float64), d.last_scg["max_ind"].cpu().numpy()
    top2 = np.sort(table, axis=0)[-2:]
    margin, spread = float((top2[1] - top2[0]).min()), float(table.max() - table.min())
    print(f"[dpmpp scg] DDIM table: best - second {margin:.3e}, spread {spread:.3e}")
    assert margin > 1e-3 * spread                       # precondition: rounding cannot flip a winner
    _inject(d, nz)
    out = d.dpmpp_sample(net, x, t, order=1, **kw)
    assert np.array_equal(d.last_scg["max_ind"].cpu().numpy(), win)
    assert rel(out["sample"].cpu().numpy(), ref["sample"].cpu().numpy()) < 2e-4
    assert rel(out["pred_xstart"].cpu().numpy(), ref["pred_xstart"].cpu().numpy()) < 2e-4


def test_scg_search_step_order_two_selects_mean_plus_g_z():
    from gpu_util import dev, rel
    from test_gpu_sampler import _inject
    g, d, nz, kw = _scg_setup()
    net = _net()
    x, t = dev(g["x"]), dev(g["dscg.t"])
    prev = dev((0.5 * g["x"] + 0.1 * np.random.RandomState(9).randn(*g["x"].shape)).astype(F32))
    _inject(d, nz)
    seen, real = [], d._dpm_step

    def spy(*a, **k):
        seen.append((a, k, real(*a, **k)))
        return seen[-1][2]
    d._dpm_step = spy
    out = d.dpmpp_sample(net, x, t, x0_prev=prev, order=2, **kw)
    d._dpm_step = real
    assert len(seen) == 1                                                       # one launch: the mean and g of the search step
    (a, k, (mean, x0, gg)) = seen[0]
    assert k["order"] == 2 and k["eta"] == 1.0 and k["want_g"] and a[3] is prev and a[4] is None
    mean1, _, _ = real(*a, **dict(k, order=1))
    assert rel(mean.cpu().numpy(), mean1.cpu().numpy()) > 1e-3                     # the earlier estimate entered the mean
    sel = d.last_scg["max_ind"]
    z = dev(nz)[sel, torch.arange(2, device="cuda")]
    want = mean.double() + gg.double().view(2, 1, 1, 1) * z.double()
    assert rel(out["sample"].cpu().numpy(), want.cpu().numpy()) < 1e-6           # one float32 multiply-add per element
    assert torch.equal(out["pred_xstart"], x0)


def test_classifier_guided_step_order_one_is_the_guided_ddim_step():
    from gpu_util import dev
    from test_gpu_pins2 import _cls, _cond
    from test_gpu_sampler import _inject
    g = load_golden("steps2")
    d = _diffusion("ddim50")
    d.t_end = 0
    ac = d.alphas_cumprod
    net, cond = _net(), _cond(_cls())
    nz = np.random.RandomState(int(g["dcg.noise_seed"])).randn(2, 4, 128, 16).astype(F32)
    x, t = dev(g["x"]), dev(g["dcg.t"])
    mk = {"y": dev(g["y"]), "rule": {"note_density": dev(g["cg.rule"])}}
    kw = dict(clip_denoised=False, eta=1.0, cond_fn=cond, model_kwargs=mk, guidance_kwargs=SimpleNamespace(schedule=False, method="classifier_guidance"))
    _inject(d, nz, nz, nz)
    a = d.ddim_sample(net, x, t, **kw)
    b = d.dpmpp_sample(net, x, t, order=1, **kw)
    plain = d.dpmpp_sample(net, x, t, order=1, clip_denoised=False, eta=1.0, model_kwargs={"y": mk["y"]})
    assert (b["sample"] - plain["sample"]).abs().max().item() > 1e-3            # the gradient moved the step
    # the float64 DDIM step on the same eps and gradient; each kernel within the bound of its own float32 restatement
    eps = d._wrap_model(net)(x, t, y=mk["y"]).cpu().numpy().reshape(2, -1)
    grad = d._wrap_model(cond)(x, t, **mk).cpu().numpy().reshape(2, -1)
    tn, xn, zn = g["dcg.t"].astype(np.int64), g["x"].reshape(2, -1), nz.reshape(2, -1)
    ref = R.ddim_step(ac, xn, eps, tn, grad=grad, noise=zn, eta=1.0)
    ddim32 = R.ddim_step(ac, xn, eps, tn, grad=grad, noise=zn, eta=1.0, dtype=np.float32)
    dpm32 = R.step(ac, xn, eps, tn, grad=grad, noise=zn, order=1, sde=True, dtype=np.float32)
    for i, name in enumerate(("sample", "pred_xstart")):
        for who, out, r32 in (("ddim", a[name], ddim32[i]), ("dpmpp", b[name], dpm32[i])):
            d32, tol = R.bound(ref[i], r32)
            err = R.rel_err(out.cpu().numpy().reshape(2, -1), ref[i])
            print(f"[guided step] {who} {name}: err {err:.2e}, d32 {d32:.2e}")
            assert err <= tol, (who, name, err, d32)


def test_denoised_fn_edit_and_learned_sigma_go_through_the_step(gauss):
    """the options dpmpp_sample shares with ddim_sample: denoised_fn acts on x0, edit_kwargs replaces the masked x0 by the source,
    a learn_sigma network's eps half is used"""
    from gpu_util import dev
    gm, xT = gauss
    d = _diffusion("logsnr20")
    d.t_end = 0
    ac = d.alphas_cumprod
    model = _GaussianEps(gm, SHAPE[1:])
    x = torch.from_numpy(xT).cuda().view(SHAPE)
    t = torch.full((4,), 7, dtype=torch.int64, device="cuda")
    tn = np.full(4, 7, dtype=np.int64)
    base = d.dpmpp_sample(model, x, t, clip_denoised=False)
    eps = model(x, torch.full((4,), d.timestep_map[7], dtype=torch.int64, device="cuda")).cpu().numpy().reshape(4, -1)
    ref = R.step(ac, xT, eps, tn)
    assert R.rel_err(base["sample"].cpu().numpy().reshape(4, -1), ref[0]) <= R.bound(ref[0], R.step(ac, xT, eps, tn, dtype=np.float32)[0])[1]
    # denoised_fn: x0 -> 0.5 x0
    out = d.dpmpp_sample(model, x, t, clip_denoised=False, denoised_fn=lambda v: 0.5 * v)
    assert R.rel_err(out["pred_xstart"].cpu().numpy().reshape(4, -1), 0.5 * ref[1]) < 1e-5
    # edit: rows [32, 96) are generated, the rest is the source
    gt = dev(np.random.RandomState(3).uniform(-1, 1, size=(1,) + SHAPE[1:]).astype(F32))
    mask = torch.ones_like(gt)
    mask[:, :, 32:96] = 0
    out = d.dpmpp_sample(model, x, t, clip_denoised=False, edit_kwargs={"gt": gt, "mask": mask, "l_start": 32, "l_end": 96, "noise_level": 10})
    x0 = out["pred_xstart"]
    assert (x0[:, :, :32] - gt[:, :, :32]).abs().max().item() < 1e-4 and torch.allclose(x0[:, :, 32:96], base["pred_xstart"][:, :, 32:96], atol=1e-5)
    # an edit chain starts at noise_level, first order, and carries pred_xstart from there
    full = d.dpmpp_sample_loop(model, SHAPE, clip_denoised=False, eta=0.0, device="cuda",
                               edit_kwargs={"gt": gt, "mask": mask, "l_start": 32, "l_end": 96, "noise_level": 10})
    assert (full[:, :, :32] - gt[:, :, :32]).abs().max().item() < 1e-4 and torch.isfinite(full).all()
    # learn_sigma: 2C channels, the eps half drives the step
    dl = _diffusion("logsnr20", learn_sigma=True)
    dl.t_end = 0
    two = lambda x_, t_, **kw: torch.cat([model(x_, t_), torch.full_like(x_, 0.3)], dim=1)
    out = dl.dpmpp_sample(two, x, t, clip_denoised=False)
    assert torch.equal(out["sample"], base["sample"])


def test_raising_cases_raise_before_any_launch():
    from guided_diffusion import gaussian_diffusion as gd
    d = _diffusion("logsnr20")
    x, t = torch.zeros(2, 4, 128, 16, device="cuda"), torch.full((2,), 5, dtype=torch.int64, device="cuda")
    calls = []

    def model(*a, **k):
        calls.append(1)
        raise AssertionError("the model was called")
    launches = []
    real = d._dpm_step
    d._dpm_step = lambda *a, **k: launches.append(1) or real(*a, **k)
    with pytest.raises(ValueError, match="eta"):
        d.dpmpp_sample(model, x, t, eta=0.3)
    with pytest.raises(ValueError, match="order"):
        d.dpmpp_sample(model, x, t, order=3)
    with pytest.raises(ValueError, match="SCG"):
        d.dpmpp_sample(model, x, t, eta=0.0, scg_kwargs={"num_samples": 4})
    with pytest.raises(ValueError, match="SCG"):
        d.dpmpp_sample_loop(model, (2, 4, 128, 16), eta=0.0, scg_kwargs={"num_samples": 4}, device="cuda")
    with pytest.raises(NotImplementedError, match="DPS"):
        d.dpmpp_sample(model, x, t, eta=1.0, cond_fn=model, guidance_kwargs=SimpleNamespace(method="dps", schedule=False))
    d.model_mean_type = gd.ModelMeanType.PREVIOUS_X
    with pytest.raises(NotImplementedError, match="PREVIOUS_X"):
        d.dpmpp_sample(model, x, t)
    assert not calls and not launches


# ------------------------------------------------------------------------------------ CLIs
COMMON = ["--model", "DiTRotary_B_8", "--image_size", "128", "16", "--in_channels", "4", "--scale_factor", "1.2465",
          "--class_cond", "True", "--num_classes", "3", "--class_label", "1", "--synthetic_weights", "True", "--progress", "False"]
CFG = os.path.join(PKG, "scripts", "configs")


def _script(name):
    spec = importlib.util.spec_from_file_location(name + "_cli", os.path.join(PKG, "scripts", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("cfg,eta", [("cond_table/single/scg/pitch.yml", "1"), ("cond_table/no_guidance/nd.yml", "0")])
def test_sample_rule_cli_with_the_dpmpp_sampler(tmp_path, monkeypatch, cfg, eta):
    monkeypatch.chdir(tmp_path)
    cli = _script("sample_rule")
    res = cli.main(["--config_path", os.path.join(CFG, cfg), "--batch_size", "2", "--num_samples", "2", "--diffusion_steps", "24",
                    "--sampler", "dpmpp", "--dpmpp_steps", "4", "--dpmpp_eta", eta] + COMMON)
    out_dir = os.path.join("loggings", cli.output_dir_for(os.path.join(CFG, cfg), 1))
    meta = json.load(open(os.path.join(out_dir, "run_metadata.json")))
    assert meta["sampler"] == {"name": "dpmpp", "timestep_respacing": "logsnr4", "steps": 4, "order": 2, "eta": float(eta)}
    rule = "pitch_hist" if "pitch" in cfg else "note_density"
    assert len(res) == 2 and np.isfinite(res[f"{rule}.loss"]).all()
    roll = np.load(os.path.join(out_dir, "sample_0_y_1.npy"))
    assert roll.shape == (3, 128, 1024) and roll.dtype == np.uint8 and roll.max() <= 127
    with pytest.raises(SystemExit):                             # argparse: not one of the samplers
        cli.main(["--config_path", os.path.join(CFG, cfg), "--sampler", "heun"] + COMMON)


def test_edit_cli_with_the_dpmpp_sampler(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    cli = _script("edit")
    cfg = os.path.join(str(tmp_path), "configs", "edit", "nd_short.yml")
    os.makedirs(os.path.dirname(cfg))
    open(cfg, "w").write(open(os.path.join(CFG, "edit", "nd_scg_given_target.yml")).read().replace("noise_level: 500", "noise_level: 12"))
    res, sample = cli.main(["--config_path", cfg, "--batch_size", "2", "--num_samples", "2", "--diffusion_steps", "24",
                            "--allow_synthetic_source", "True", "--sampler", "dpmpp", "--dpmpp_steps", "6"] + COMMON)
    assert len(res) == 2 and np.isfinite(res["note_density.loss"]).all()
    meta = json.load(open(os.path.join("loggings", "edit_demo", "edit", "nd_short_cls_1_synthsrc", "run_metadata.json")))
    assert meta["sampler"]["name"] == "dpmpp" and meta["sampler"]["timestep_respacing"] == "logsnr6" and meta["sampler"]["eta"] == 1.0
    assert 1 <= meta["noise_level"] <= 6                       # the YAML's level, counted in steps of the solver's chain
    assert sample.shape == (2, 128, 1024, 3) and sample.dtype == torch.uint8


def test_cfg_sample_cli_with_the_dpmpp_sampler(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("OPENAI_LOGDIR", str(tmp_path / "log"))
    cli = _script("cfg_sample")
    arr = cli.main(["--model", "DiTRotary_B_8", "--image_size", "128", "16", "--in_channels", "4", "--scale_factor", "1.2465",
                    "--num_classes", "3", "--class_label", "2", "--synthetic_weights", "True", "--progress", "False", "--batch_size", "2",
                    "--num_samples", "2", "--diffusion_steps", "24", "--cfg", "True", "--w", "4.", "--class_cond", "True",
                    "--use_dpmpp", "True", "--dpmpp_steps", "4"])
    assert arr.shape == (2, 3, 128, 1024) and arr.dtype == np.uint8 and not np.array_equal(arr[0], arr[1])
    meta = [os.path.join(dp, f) for dp, _, fs in os.walk(str(tmp_path)) for f in fs if f == "run_metadata.json"]
    assert len(meta) == 1 and json.load(open(meta[0]))["sampler"]["name"] == "dpmpp"
