"""Guided sampling beyond 256 / 288 tokens: the streaming attention backward (csrc/attention_bwd_stream.hip) and everything that sits on
it -- classifier guidance, DPS, guided editing -- behind the explicit switch (guided_diffusion.dit.set_long_backward / RGM_LONG_BACKWARD).

Tolerances are the ones the same quantities are held to at T <= 256 (test_gpu_dit.py, test_gpu_sampler.py, test_gpu_dpsrule.py,
test_gpu_edit.py); none is chosen here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden, ROOT, PKG
from rgm import synth

pytestmark = pytest.mark.gpu

ATTN_TOL = {"fp32": 1e-5, "bf16x3": 4e-5, "bf16x3_presplit": 4e-5}      # test_gpu_dit.py::test_attention_backward_kernel_vs_oracle


# ------------------------------------------------------------------------------------------------ the kernels
def _attn_inputs(N, T, heads, hd, seed):
    rng = np.random.RandomState(seed)
    D = heads * hd
    return rng.randn(N * T, 3 * D).astype(np.float32), rng.randn(N * T, D).astype(np.float32)


_REF_CACHE = {}


def _attn_bwd_fp64(N, T, heads, hd, seed, chunk=1024):
    """d(qkv) (N*T, 3*D) in fp64 -- the restatement of test_gpu_dit.py::test_attention_backward_kernel_vs_oracle, one (sample, head) at a
    time and chunked over the query rows (no T x T matrix of more than `chunk` rows on the host).  Cached: the three precisions share it."""
    key = (N, T, heads, hd, seed)
    if key in _REF_CACHE:
        return _REF_CACHE[key]
    from rgm.synth import rotary_freqs
    from oracle import dit_np as odit
    qkv, d_o = _attn_inputs(N, T, heads, hd, seed)
    D = heads * hd
    cos, sin = odit.rotary_tables(rotary_freqs(hd // 2), T)
    r = qkv.reshape(N, T, 3, heads, hd)
    q, k, v = (np.ascontiguousarray(r[:, :, i].transpose(0, 2, 1, 3)) for i in range(3))
    qr, kr = odit.apply_rotary(q, cos, sin), odit.apply_rotary(k, cos, sin)
    do = d_o.reshape(N, T, heads, hd).transpose(0, 2, 1, 3)
    scale = hd ** -0.5
    dq = np.empty((N, heads, T, hd), np.float64)
    dk = np.zeros((N, heads, T, hd), np.float64)
    dv = np.zeros((N, heads, T, hd), np.float64)
    for n in range(N):
        for h in range(heads):
            k64, v64 = kr[n, h].astype(np.float64), v[n, h].astype(np.float64)
            for r0 in range(0, T, chunk):
                qc, gc = qr[n, h, r0:r0 + chunk].astype(np.float64), do[n, h, r0:r0 + chunk].astype(np.float64)
                s = (qc @ k64.T) * scale
                p = np.exp(s - s.max(-1, keepdims=True))
                p /= p.sum(-1, keepdims=True)
                dv[n, h] += p.T @ gc
                dp = gc @ v64.T
                ds = p * (dp - (dp * p).sum(-1, keepdims=True)) * scale
                dq[n, h, r0:r0 + chunk] = ds @ k64
                dk[n, h] += ds.T @ qc
    dqf = odit.apply_rotary(dq.astype(np.float32), cos, sin, inverse=True)
    dkf = odit.apply_rotary(dk.astype(np.float32), cos, sin, inverse=True)
    ref = np.stack((dqf, dkf, dv.astype(np.float32)), axis=0).transpose(1, 3, 0, 2, 4).reshape(N * T, 3 * D)
    _REF_CACHE[key] = ref
    return ref


def _attn_bwd_gpu(N, T, heads, hd, seed, launches=1):
    """rgm_rotary_attention_bwd on O and lse of rgm_rotary_attention_lse (what the product path hands it); output pre-filled with NaN."""
    from gpu_util import dev
    from rgm import native as R
    from rgm.synth import rotary_freqs
    from oracle import dit_np as odit
    qkv, d_o = _attn_inputs(N, T, heads, hd, seed)
    D = heads * hd
    cos, sin = odit.rotary_tables(rotary_freqs(hd // 2), T)
    qd, gd, cd, sd_ = dev(qkv), dev(d_o), dev(cos), dev(sin)
    od = torch.empty(N * T, D, device="cuda")
    lse = torch.empty(N * heads * T, device="cuda")
    R.check(R.lib.rgm_rotary_attention_lse(R.ptr(qd), R.ptr(od), R.ptr(lse), R.ptr(cd), R.ptr(sd_), N, T, heads, hd, hd // 4, R.current_stream()))
    outs = []
    for _ in range(launches):
        out = torch.full((N * T, 3 * D), float("nan"), device="cuda")
        R.check(R.lib.rgm_rotary_attention_bwd(R.ptr(qd), R.ptr(od), R.ptr(gd), R.ptr(lse), R.ptr(out), R.ptr(cd), R.ptr(sd_),
                                               N, T, heads, hd, hd // 4, R.current_stream()))
        outs.append(out)
    torch.cuda.synchronize()
    return outs if launches > 1 else outs[0]


LONG_SHAPES = [(2, 272, 16, 72), (2, 512, 16, 72), (1, 1000, 16, 72), (1, 2048, 16, 72), (1, 2080, 4, 72), (2, 300, 6, 64),
               (2, 513, 6, 64), (1, 1025, 6, 64), (1, 8192, 2, 72), (1, 6001, 2, 64)]


@pytest.mark.parametrize("shape", LONG_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stream_backward_kernel_vs_fp64(shape, precision):
    from gpu_util import rel
    N, T, heads, hd = shape
    out = _attn_bwd_gpu(N, T, heads, hd, seed=5).cpu().numpy()
    assert np.isfinite(out).all(), shape
    err = rel(out, _attn_bwd_fp64(N, T, heads, hd, seed=5))
    print(f"attn_bwd_stream {shape} {precision}: rel {err:.3e} (bound {ATTN_TOL[precision]:.0e})")
    assert err < ATTN_TOL[precision], (shape, err)


SHORT_SHAPES = [(2, 256, 16, 72), (3, 200, 16, 72), (2, 288, 6, 64), (2, 257, 6, 64), (1, 37, 6, 64)]


@pytest.mark.parametrize("shape", SHORT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stream_backward_matches_resident(shape, precision):
    from gpu_util import rel
    from rgm import native as R
    N, T, heads, hd = shape
    ref = _attn_bwd_fp64(N, T, heads, hd, seed=6)
    resident = _attn_bwd_gpu(N, T, heads, hd, seed=6).cpu().numpy()
    prev = R.lib.rgm_set_attn_bwd_stream(1)
    try:
        before = R.lib.rgm_attn_bwd_stream_launches()
        stream = _attn_bwd_gpu(N, T, heads, hd, seed=6).cpu().numpy()
        assert R.lib.rgm_attn_bwd_stream_launches() == before + 1
    finally:
        R.lib.rgm_set_attn_bwd_stream(prev)
    assert np.isfinite(stream).all()
    e64, eres = rel(stream, ref), rel(stream, resident)
    print(f"attn_bwd_stream forced {shape} {precision}: vs fp64 {e64:.3e}, vs resident {eres:.3e}, resident vs fp64 {rel(resident, ref):.3e}")
    assert e64 < ATTN_TOL[precision], (shape, e64)
    assert eres < 2 * ATTN_TOL[precision], (shape, eres)


def test_resident_shapes_stay_on_the_resident_kernels(precision):
    from rgm import native as R
    assert R.lib.rgm_set_attn_bwd_stream(0) == 0                 # the default
    before = R.lib.rgm_attn_bwd_stream_launches()
    for shape in ((2, 256, 16, 72), (2, 257, 6, 64)):
        _attn_bwd_gpu(*shape, seed=7)
    assert R.lib.rgm_attn_bwd_stream_launches() - before == 0
    _attn_bwd_gpu(1, 512, 6, 64, seed=7)
    assert R.lib.rgm_attn_bwd_stream_launches() - before > 0


@pytest.mark.parametrize("shape", [(8, 1024, 16, 72), (8, 577, 6, 64)], ids=lambda s: "x".join(map(str, s)))
def test_stream_backward_repeats_bitwise(shape, precision):
    """50 launches on one fixed input: every row of dq, dk, dv equal to the first launch's, bit for bit (no atomics, one owner per element)."""
    outs = _attn_bwd_gpu(*shape, seed=8, launches=50)
    first = outs[0]
    assert bool(torch.isfinite(first).all())
    differing = [i for i, o in enumerate(outs[1:], 1) if not torch.equal(o.view(torch.int32), first.view(torch.int32))]
    assert not differing, (shape, differing)


# ------------------------------------------------------------------------------------------------ the models
TOL = 2e-4                                                       # logits / eps (test_gpu_dit.py)
GRAD_TOL = 5e-4                                                  # gradients (test_gpu_dit.py, the dps.npz tests)
XL2 = dict(depth=2, hidden=1152, heads=16, patch=8, in_ch=4, out_ch=4, num_classes=3)
XL28 = dict(XL2, depth=28)
CLS2 = dict(depth=2, hidden=384, heads=6, patch=8, in_ch=4, classifier=True, cls_classes=16)
CLS12 = dict(CLS2, depth=12)
CHD = dict(depth=2, hidden=384, heads=6, patch=8, in_ch=4, classifier=True, cls_classes=8, chord=True)


def _randn(seed, *shape):
    """the rule make_golden_guided_long.py builds every input by"""
    return np.random.RandomState(int(seed)).randn(*shape).astype(np.float32)


def _seed(g, key):
    return int(g[key][0])


@pytest.fixture
def long_on():
    from guided_diffusion import dit
    dit.set_long_backward(True)
    yield
    dit.set_long_backward(None)                                  # back to following the environment (the default: off)


def _eps_model(arch, seed):
    from gpu_util import load_module
    from guided_diffusion.dit import DiTRotary
    m = DiTRotary(input_size=[128, 16], patch_size=arch["patch"], in_channels=arch["in_ch"], hidden_size=arch["hidden"],
                  depth=arch["depth"], num_heads=arch["heads"], num_classes=arch.get("num_classes", 0), learn_sigma=False)
    return load_module(m, synth.dit_state_dict(seed, device="cuda", **arch))


def _classifier(arch, seed):
    from gpu_util import load_module
    from guided_diffusion.dit import DiTRotaryClassifier
    m = DiTRotaryClassifier(input_size=[128, 16], patch_size=8, in_channels=4, hidden_size=arch["hidden"], depth=arch["depth"],
                            num_heads=arch["heads"], num_classes=arch["cls_classes"], chord=arch.get("chord", False))
    return load_module(m, synth.dit_state_dict(seed, **arch))


@pytest.mark.parametrize("tag,arch,H,B", [("s8d2", CLS2, 256, 2), ("s8", CLS12, 256, 2), ("s8d2", CLS2, 512, 1)])
def test_long_classifier_mse_gradient_matches_autograd(tag, arch, H, B, precision, long_on):
    from gpu_util import dev, rel
    from guided_diffusion.condition_functions import grad_nn_zt_mse
    g = load_golden("guidedlong_cls")
    m = _classifier(arch, _seed(g, f"{tag}.seed"))
    x, t, rule = dev(_randn(_seed(g, f"{tag}.x{H}_seed"), B, 4, H, 16)), dev(g[f"{tag}.t{H}"]), dev(g[f"{tag}.rule{H}"])
    logits, grad = m.value_and_grad(x, t, rule, "mse", 10.0)
    el, eg = rel(logits.cpu().numpy(), g[f"{tag}.logits{H}"]), rel(grad.cpu().numpy(), g[f"{tag}.grad{H}"])
    print(f"cls {tag} H={H} {precision}: logits {el:.3e}, grad {eg:.3e}")
    assert el < TOL and eg < GRAD_TOL
    assert torch.equal(grad_nn_zt_mse(x, t, rule=rule, classifier_scale=10., classifier=m), grad)


def test_long_chord_and_xentropy_gradients_match_autograd(precision, long_on):
    from gpu_util import dev, rel
    from guided_diffusion.condition_functions import grad_nn_zt_chord, grad_nn_zt_xentropy
    g = load_golden("guidedlong_cls")
    m = _classifier(CHD, _seed(g, "chord.seed"))
    x, t = dev(_randn(_seed(g, "chord.x256_seed"), 2, 4, 256, 16)), dev(g["chord.t256"])
    key, ch = m(x, t)
    assert rel(key.cpu().numpy(), g["chord.key256"]) < TOL and rel(ch.cpu().numpy(), g["chord.logits256"]) < TOL
    grad = grad_nn_zt_chord(x, t, rule=dev(g["chord.rule256"]), classifier_scale=10., classifier=m)
    eg = rel(grad.cpu().numpy(), g["chord.grad256"])
    m2 = _classifier(CLS2, _seed(g, "s8d2.seed"))
    gx = grad_nn_zt_xentropy(dev(_randn(_seed(g, "xent.x256_seed"), 2, 4, 256, 16)), rule=dev(g["xent.rule256"]), classifier=m2)
    ex = rel(gx.cpu().numpy(), g["xent.grad256"])
    print(f"chord grad {eg:.3e}, xentropy grad {ex:.3e} ({precision})")
    assert eg < GRAD_TOL and ex < GRAD_TOL


@pytest.mark.parametrize("tag,arch,shapes", [("xl2", XL2, (136, 256, 512)), ("xl28", XL28, (256,))])
def test_long_eps_network_vjp_matches_autograd(tag, arch, shapes, precision, long_on):
    from gpu_util import dev, rel
    g = load_golden("guidedlong_vjp")
    m = _eps_model(arch, _seed(g, f"{tag}.seed"))
    for H in shapes:
        s = _seed(g, f"{tag}.x{H}_seed")
        eps, grad = m.vjp(dev(_randn(s, 1, 4, H, 16)), dev(g[f"{tag}.t{H}"]), dev(g[f"{tag}.y{H}"]), dev(_randn(s + 1000, 1, 4, H, 16)))
        ee, eg = rel(eps.cpu().numpy(), g[f"{tag}.eps{H}"]), rel(grad.cpu().numpy(), g[f"{tag}.grad{H}"])
        print(f"vjp {tag} H={H} {precision}: eps {ee:.3e}, grad {eg:.3e}")
        assert ee < TOL and eg < GRAD_TOL, (tag, H)


# ------------------------------------------------------------------------------------------------ the steps
def _diffusion(rs):
    from guided_diffusion.script_util import create_diffusion
    d = create_diffusion(learn_sigma=False, diffusion_steps=1000, noise_schedule="linear", timestep_respacing=rs,
                         use_kl=False, predict_xstart=False, rescale_timesteps=False, rescale_learned_sigmas=False)
    d.t_end = 0
    return d


def _model_fn(m):
    from functools import partial
    from guided_diffusion.condition_functions import model_fn
    return partial(model_fn, model=m, num_classes=3, class_cond=True, cfg=False, w=0.)


def _inject(d, *arrays):
    q = [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays]

    def fn(shape, device):
        z = q.pop(0)
        assert tuple(z.shape) == tuple(shape), (z.shape, shape)
        return z.to(device)
    d.noise_fn = fn


class _Steps:
    """the setting of guidedlong_steps.npz: XL-2 + the depth-2 classifier, H = 256, B = 2, inputs rebuilt from their seeds"""

    def __init__(self):
        from functools import partial
        from types import SimpleNamespace
        from gpu_util import dev
        from guided_diffusion.condition_functions import composite_nn_zt
        g = self.g = load_golden("guidedlong_steps")
        self.m = _eps_model(XL2, _seed(g, "dit.seed"))
        self.cm = _classifier(CLS2, _seed(g, "cls.seed"))
        self.x = dev(_randn(_seed(g, "x_seed"), 2, 4, 256, 16))
        self.y = dev(g["y"])
        self.rule = {"note_density": dev(g["rule"])}
        self.cg = SimpleNamespace(schedule=False, method="classifier_guidance")
        self.cond = partial(composite_nn_zt, fns=["grad_nn_zt_mse"], classifier_scales=[10.], classifiers=[self.cm], rule_names=["note_density"])

    def noise(self, tag):
        return _randn(_seed(self.g, f"{tag}.noise_seed"), 2, 4, 256, 16)

    def plain(self, rs, tag, ddim=False):
        from gpu_util import dev
        d = _diffusion(rs)
        _inject(d, self.noise(tag))
        kw = dict(clip_denoised=False, model_kwargs={"y": self.y})
        t = dev(self.g[f"{tag}.t"])
        return d.ddim_sample(_model_fn(self.m), self.x, t, eta=1.0, **kw) if ddim else d.p_sample(_model_fn(self.m), self.x, t, **kw)


def test_long_classifier_guided_ddpm_step_matches_reference(precision, long_on):
    """bounds of the H = 128 twins: sample 2e-4, the guidance term on its own 5e-3 (test_gpu_pins2.py)"""
    from gpu_util import dev, rel
    s = _Steps()
    d = _diffusion("250")
    _inject(d, s.noise("cg"))
    out = d.p_sample(_model_fn(s.m), s.x, dev(s.g["cg.t"]), clip_denoised=False, cond_fn=s.cond, model_kwargs={"y": s.y, "rule": s.rule},
                     guidance_kwargs=s.cg)
    shift = (out["sample"] - s.plain("250", "cg")["sample"]).cpu().numpy()
    es, eh = rel(out["sample"].cpu().numpy(), s.g["cg.sample"]), rel(shift, s.g["cg.shift"])
    print(f"cg step {precision}: sample {es:.3e}, shift {eh:.3e}")
    assert es < 2e-4
    assert np.abs(s.g["cg.shift"]).max() > 1e-3 and eh < 5e-3


def test_long_ddim_condition_score_step_matches_reference(precision, long_on):
    from gpu_util import dev, rel
    s = _Steps()
    d = _diffusion("ddim50")
    _inject(d, s.noise("dcg"))
    out = d.ddim_sample(_model_fn(s.m), s.x, dev(s.g["dcg.t"]), clip_denoised=False, eta=1.0, cond_fn=s.cond,
                        model_kwargs={"y": s.y, "rule": s.rule}, guidance_kwargs=s.cg)
    shift = (out["sample"] - s.plain("ddim50", "dcg", ddim=True)["sample"]).cpu().numpy()
    es, eh = rel(out["sample"].cpu().numpy(), s.g["dcg.sample"]), rel(shift, s.g["dcg.shift"])
    print(f"dcg step {precision}: sample {es:.3e}, shift {eh:.3e}")
    assert es < 2e-4
    assert np.abs(s.g["dcg.shift"]).max() > 1e-3 and eh < 5e-3


def test_long_dps_nn_step_matches_reference(precision, long_on):
    """bounds of test_gpu_edit.py::test_dps_guided_step_matches_reference"""
    from functools import partial
    from types import SimpleNamespace
    from gpu_util import dev, rel
    from guided_diffusion.condition_functions import composite_nn_zt
    s = _Steps()
    d = _diffusion("250")
    _inject(d, s.noise("dps"))
    cond = partial(composite_nn_zt, fns=["nn_z0_mse_dummy"], classifier_scales=[1.], classifiers=[s.cm], rule_names=["note_density"])
    gk = SimpleNamespace(schedule=False, method="dps", step_size=1.5, nn=True, vae=False)
    out = d.p_sample(_model_fn(s.m), s.x, dev(s.g["dps.t"]), clip_denoised=False, cond_fn=cond, model_kwargs={"y": s.y, "rule": s.rule},
                     guidance_kwargs=gk)
    es, ep = rel(out["sample"].cpu().numpy(), s.g["dps.sample"]), rel(out["pred_xstart"].cpu().numpy(), s.g["dps.pred_xstart"])
    print(f"dps-nn step {precision}: sample {es:.3e}, pred_xstart {ep:.3e}")
    assert es < 5e-4 and ep < 5e-4


def test_long_dps_rule_step_matches_reference(precision, long_on):
    """bounds of test_gpu_dpsrule.py::test_dps_rule_guided_step_matches_reference"""
    from functools import partial
    from types import SimpleNamespace
    from gpu_util import dev, load_module, rel
    from guided_diffusion.condition_functions import composite_rule
    from taming.models.klvae_pedal import AutoencoderKL
    s = _Steps()
    vae = load_module(AutoencoderKL(), synth.vae_state_dict(_seed(s.g, "vae.seed"), encoder=True))
    d = _diffusion("250")
    _inject(d, s.noise("dpsr"))
    cond = partial(composite_rule, fns=["rule_x0_mse_dummy"], classifier_scales=[1.], rule_names=["pitch_hist"])
    gk = SimpleNamespace(schedule=False, method="dps", step_size=100.0, nn=False, vae=True)
    out = d.p_sample(_model_fn(s.m), s.x, dev(s.g["dpsr.t"]), clip_denoised=False, cond_fn=cond,
                     model_kwargs={"y": s.y, "rule": {"pitch_hist": dev(s.g["dpsr.target"])}}, guidance_kwargs=gk, embed_model=vae,
                     scale_factor=1.2465)
    shift = (out["sample"] - s.plain("250", "dpsr")["sample"]).cpu().numpy()
    es, eh = rel(out["sample"].cpu().numpy(), s.g["dpsr.sample"]), rel(shift, s.g["dpsr.shift"])
    print(f"dps-rule step {precision}: sample {es:.3e}, shift {eh:.3e}")
    assert es < 5e-5
    assert eh < (2e-3 if precision == "fp32" else 5e-3)


def test_long_classifier_guided_edit_step_matches_reference(precision, long_on):
    """The reference refuses classifier guidance under a PARTIAL editable range (stored text); the recorded step is the whole latent
    editable, what every shipped guided edit config runs.  Bound of test_gpu_edit.py::test_classifier_guided_edit_step_matches_reference."""
    from gpu_util import dev, rel
    s = _Steps()
    assert "must match the size" in str(s.g["edit.reference_raises"]) and "edit.sample" not in s.g
    gt = (_randn(_seed(s.g, "gt_seed"), 2, 4, 256, 16) * 0.8).astype(np.float32)
    ek = {"gt": dev(gt), "mask": dev(np.zeros_like(gt)), "l_start": 0, "l_end": 256, "noise_level": 3}
    d = _diffusion("250")
    _inject(d, s.noise("editfull"))
    out = d.p_sample(_model_fn(s.m), s.x, dev(s.g["editfull.t"]), clip_denoised=False, cond_fn=s.cond,
                     model_kwargs={"y": s.y, "rule": s.rule}, guidance_kwargs=s.cg, edit_kwargs=ek)
    es = rel(out["sample"].cpu().numpy(), s.g["editfull.sample"])
    print(f"guided edit step {precision}: sample {es:.3e}")
    assert es < 5e-4


# ------------------------------------------------------------------------------------------------ the switch
def _refusals_and_runs(expect_refusal):
    """the three calls of test_gpu_long.py::test_long_guidance_needs_the_backward_and_says_so at 512 tokens"""
    from functools import partial
    from types import SimpleNamespace
    from guided_diffusion.condition_functions import composite_nn_zt
    clf = _classifier(CLS2, 4)
    x = torch.randn(2, 4, 256, 16, device="cuda")
    t = torch.tensor([500, 20], device="cuda")
    m = _eps_model(XL2, 1)
    d = _diffusion("250")
    cond = partial(composite_nn_zt, fns=["nn_z0_mse_dummy"], classifier_scales=[1.], classifiers=[clf], rule_names=["note_density"])
    gk = SimpleNamespace(schedule=False, method="dps", step_size=1.0, nn=True, vae=False)

    def dps():
        return d.p_sample(_model_fn(m), x, torch.full((2,), 120, device="cuda"), clip_denoised=False, cond_fn=cond, guidance_kwargs=gk,
                          model_kwargs={"y": torch.tensor([1, 2], device="cuda"), "rule": {"note_density": torch.zeros(2, 16, device="cuda")}})
    if expect_refusal:
        with pytest.raises(NotImplementedError, match="288 tokens"):
            clf.value_and_grad(x, t, torch.zeros(2, 16, device="cuda"), "mse", 1.0)
        with pytest.raises(NotImplementedError, match="256 tokens"):
            dps()
        with pytest.raises(NotImplementedError, match="256 tokens"):
            m.vjp_forward(x, t, torch.tensor([1, 2], device="cuda"))
        return
    logits, grad = clf.value_and_grad(x, t, torch.zeros(2, 16, device="cuda"), "mse", 1.0)
    assert logits.shape == (2, 16) and grad.shape == x.shape and bool(torch.isfinite(grad).all())
    out = dps()
    assert out["sample"].shape == x.shape and bool(torch.isfinite(out["sample"]).all())
    eps = m.vjp_forward(x, t, torch.tensor([1, 2], device="cuda"))
    gx = m.vjp_backward(torch.ones_like(eps))
    assert eps.shape == x.shape and gx.shape == x.shape and bool(torch.isfinite(gx).all())
    with pytest.raises(NotImplementedError, match="8192 tokens"):
        m.vjp_forward(torch.zeros(1, 4, 4097, 16, device="cuda"), t[:1], torch.tensor([1], device="cuda"))     # 8194 tokens


def test_long_backward_switch_off_refuses_on_runs(precision, monkeypatch):
    from guided_diffusion import dit
    monkeypatch.delenv("RGM_LONG_BACKWARD", raising=False)
    assert dit.long_backward() is False                          # the default
    _refusals_and_runs(expect_refusal=True)
    assert dit.set_long_backward(True) is False
    try:
        _refusals_and_runs(expect_refusal=False)
        assert dit.set_long_backward(False) is True
        _refusals_and_runs(expect_refusal=True)
    finally:
        dit.set_long_backward(None)


def test_long_backward_switch_from_the_environment_in_a_fresh_process(precision):
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "import torch\n"
            "from rgm import native as R\n"
            "R.set_gemm_precision(%r)\n"
            "from guided_diffusion import dit\n"
            "assert dit.long_backward() is True\n"
            "import test_gpu_guided_long as G\n"
            "G._refusals_and_runs(expect_refusal=False)\n"
            "print('long backward from the environment: ok')\n") % (os.path.join(ROOT, "tests"), ROOT, PKG, precision)
    env = dict(os.environ, RGM_LONG_BACKWARD="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "long backward from the environment: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------------------------------------ the CLIs
CFG = os.path.join(PKG, "scripts", "configs")
CLI_COMMON = ["--model", "DiTRotary_B_8", "--image_size", "256", "16", "--in_channels", "4", "--scale_factor", "1.2465",
              "--class_cond", "True", "--num_classes", "3", "--class_label", "1", "--synthetic_weights", "True", "--progress", "False"]


def _load_cli(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(f"{name}_guided_long_cli", os.path.join(PKG, "scripts", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _write_config(tmp_path, rel_path, text):
    p = os.path.join(str(tmp_path), "configs", rel_path)
    os.makedirs(os.path.dirname(p), exist_ok=True)
    with open(p, "w") as f:
        f.write(text)
    return p


def test_sample_rule_cli_classifier_guidance_long_excerpt(tmp_path, monkeypatch, precision):
    import pandas as pd
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("RGM_LONG_BACKWARD", "1")
    cli = _load_cli("sample_rule")
    src = open(os.path.join(CFG, "cond_table", "single", "classifier", "nd.yml")).read()
    src = src.replace("[1.5, 3., 4.5, 3., 1.5, 3., 4.5, 3.]", str([1.5, 3., 4.5, 3., 1.5, 3., 4.5, 3.] * 2))       # 16 windows: 2048 frames
    src = src.replace("[10., 15., 20., 15., 10., 15., 20., 15.]", str([10., 15., 20., 15., 10., 15., 20., 15.] * 2))
    cfg = _write_config(tmp_path, os.path.join("cond_table", "single", "classifier", "nd_long.yml"), src)
    # 24 steps, like the other CLI tests: a shorter chain's rescaled linear schedule leaves (0, 1]
    args = ["--config_path", cfg, "--batch_size", "2", "--num_samples", "2", "--diffusion_steps", "24", "--gemm_precision", precision]
    res = cli.main(args + CLI_COMMON)
    out_dir = os.path.join("loggings", cli.output_dir_for(cfg, 1))
    df = pd.read_csv(os.path.join(out_dir, "results.csv"))
    assert len(df) == 2 and len(res) == 2 and np.isfinite(df["note_density.loss"]).all()
    roll = np.stack([np.load(os.path.join(out_dir, f"sample_{i}_y_1.npy")) for i in range(2)])
    assert roll.shape == (2, 3, 128, 2048) and roll.dtype == np.uint8
    assert json.load(open(os.path.join(out_dir, "run_metadata.json")))["long_backward"] is True


def test_edit_cli_guided_long_excerpt(tmp_path, monkeypatch, precision):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("RGM_LONG_BACKWARD", "1")
    cli = _load_cli("edit")
    src = open(os.path.join(CFG, "edit", "nd_500_num16.yml")).read()
    src = src.replace("noise_level: 500", "noise_level: 3").replace("l_end: 128", "l_end: 256").replace("num_samples: 16", "num_samples: 2")
    cfg = _write_config(tmp_path, os.path.join("edit", "nd_long.yml"), src)
    res, sample = cli.main(["--config_path", cfg, "--batch_size", "2", "--num_samples", "2", "--diffusion_steps", "24",
                            "--allow_synthetic_source", "True", "--gemm_precision", precision] + CLI_COMMON)
    assert len(res) == 2 and np.isfinite(res.select_dtypes("number").to_numpy()).all()
    assert sample.shape == (2, 128, 2048, 3) and sample.dtype == torch.uint8
    metas = [os.path.join(dp, f) for dp, _, fs in os.walk("loggings") for f in fs if f == "run_metadata.json"]
    assert len(metas) == 1 and json.load(open(metas[0]))["long_backward"] is True


# ------------------------------------------------------------------------------------------------ batch sharding
@pytest.mark.parametrize("kind", ["ddpm_cls", "dps"])
def test_long_batch_sharded_guided_step_reproduces_the_unsharded_rows(kind, monkeypatch, long_on):
    """test_gpu_sampler.py::test_batch_sharded_step_reproduces_the_unsharded_rows at H = 256: the guided step replayed as 'rank r of 2'
    gives the unsharded step's rows bit for bit -- the streaming backward's rows do not depend on the batch they run in.  Like its
    H = 128 twin this runs in the default (fp32) arithmetic only: in the bf16x3 modes the rows of a B = 2 and a B = 4 step differed in the
    last bits at H = 256 (3 of 4 cases; docs/rounds/guided_long.md), and no test pins bitwise batch independence there at any length."""
    H = 256
    from functools import partial
    from types import SimpleNamespace
    from gpu_util import dev
    from rgm import batch_shard
    from guided_diffusion.condition_functions import composite_nn_zt
    from guided_diffusion.gaussian_diffusion import PhiloxNoise
    m, cm = _eps_model(XL2, 1), _classifier(CLS2, 4)
    rng = np.random.RandomState(3)
    x = dev(rng.randn(4, 4, H, 16).astype(np.float32))
    y = dev(np.array([1, 2, 0, 1], dtype=np.int64))
    rule = {"note_density": dev((rng.rand(4, 16) * 4).astype(np.float32))}

    def run():
        d = _diffusion("250")
        d.noise = PhiloxNoise(seed=5)
        fn = "grad_nn_zt_mse" if kind == "ddpm_cls" else "nn_z0_mse_dummy"
        cond = partial(composite_nn_zt, fns=[fn], classifier_scales=[10. if kind == "ddpm_cls" else 1.], classifiers=[cm],
                       rule_names=["note_density"])
        gk = SimpleNamespace(schedule=False, method="classifier_guidance" if kind == "ddpm_cls" else "dps", step_size=1.5, nn=True, vae=False)
        return d.p_sample(_model_fn(m), x, dev(np.full(4, 120, dtype=np.int64)), cond_fn=cond, guidance_kwargs=gk, clip_denoised=False,
                          model_kwargs={"y": y, "rule": rule})

    ref = run()
    assert bool(torch.isfinite(ref["sample"]).all())
    for rank in (0, 1):
        monkeypatch.setattr(batch_shard, "partition", lambda B, r=rank: (r * B // 2, B // 2, True))

        def fake_gather(tensors, r=rank):
            out = []
            for mine, full in zip(tensors, (ref["sample"], ref["pred_xstart"])):
                assert mine.shape[0] == 2
                parts = [full[:2].clone(), full[2:].clone()]
                parts[r] = mine
                out.append(torch.cat(parts, dim=0))
            return out
        monkeypatch.setattr(batch_shard, "gather_rows", fake_gather)
        got = run()
        assert torch.equal(got["sample"], ref["sample"]), f"rank {rank}: rows differ from the unsharded step"
        assert torch.equal(got["pred_xstart"], ref["pred_xstart"])
