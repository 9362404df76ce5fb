"""-m gpu: long excerpts -- the streaming attention forward (csrc/attention_stream.hip) and everything that runs on it beyond 256 tokens:
rgm_rotary_attention(_lse) at T > 256 / 288, DiTRotary forwards against the reference (tests/golden/make_golden_long.py), a DDIM step
and chain, both CLIs at --image_size 256 16, repeatability, and the refusals of what needs the attention backward."""
import os

import numpy as np
import pytest
import torch

from conftest import PKG, load_golden
from oracle import dit_np as odit
from rgm import synth

pytestmark = pytest.mark.gpu
F32 = np.float32
TOL = 2e-4
XL2 = dict(depth=2, hidden=1152, heads=16, patch=8, in_ch=4, out_ch=4, num_classes=3)
XL28 = dict(XL2, depth=28)
ATTN_TOL = {"fp32": 3e-6, "bf16x3": 2e-5, "bf16x3_presplit": 2e-5}


def _qkv(N, T, heads, hd, seed):
    rng = np.random.RandomState(seed)
    return (rng.randn(N * T, 3 * heads * hd) * 1.5).astype(F32)


def _attention(qkv, N, T, heads, hd, with_lse=True):
    """(o (N*T, heads*hd), lse (N, heads, T)) through the C ABI"""
    from gpu_util import dev
    from rgm import native as R
    from rgm.synth import rotary_freqs
    rot = int(hd * 0.5)
    cos, sin = odit.rotary_tables(rotary_freqs(rot), T)
    qd, cd, sd_ = dev(qkv), dev(cos), dev(sin)
    od = torch.full((N * T, heads * hd), float("nan"), device="cuda")
    if with_lse:
        ld = torch.full((N * heads * T,), float("nan"), device="cuda")
        R.check(R.lib.rgm_rotary_attention_lse(R.ptr(qd), R.ptr(od), R.ptr(ld), R.ptr(cd), R.ptr(sd_), N, T, heads, hd, rot // 2,
                                               R.current_stream()))
    else:
        ld = None
        R.check(R.lib.rgm_rotary_attention(R.ptr(qd), R.ptr(od), R.ptr(cd), R.ptr(sd_), N, T, heads, hd, rot // 2, R.current_stream()))
    torch.cuda.synchronize()
    return od.cpu().numpy(), (ld.cpu().numpy().reshape(N, heads, T) if with_lse else None)


def _reference(qkv, N, T, heads, hd):
    """fp64 restatement, one (sample, head) at a time (a T x T score matrix per head bounds the host memory)"""
    from rgm.synth import rotary_freqs
    cos, sin = odit.rotary_tables(rotary_freqs(int(hd * 0.5)), T)
    D = heads * hd
    r = qkv.reshape(N, T, 3, heads, hd)
    o = np.zeros((N, T, heads, hd))
    lse = np.zeros((N, heads, T))
    for n in range(N):
        for h in range(heads):
            q = odit.apply_rotary(r[n, :, 0, h][None, None], cos, sin)[0, 0].astype(np.float64)
            k = odit.apply_rotary(r[n, :, 1, h][None, None], cos, sin)[0, 0].astype(np.float64)
            v = r[n, :, 2, h].astype(np.float64)
            s = q @ k.T * hd ** -0.5
            m = s.max(-1, keepdims=True)
            p = np.exp(s - m)
            l = p.sum(-1, keepdims=True)
            o[n, :, h] = (p / l) @ v
            lse[n, h] = (m + np.log(l))[:, 0]
    return o.reshape(N * T, D), lse


@pytest.mark.parametrize("N,T,heads,hd", [(2, 272, 16, 72), (2, 512, 16, 72), (1, 1000, 16, 72), (1, 2048, 16, 72), (2, 300, 6, 64),
                                          (1, 1024, 6, 64)])
def test_long_rotary_attention_matches_fp64(N, T, heads, hd, precision):
    from gpu_util import rel
    qkv = _qkv(N, T, heads, hd, T + hd)
    o, lse = _attention(qkv, N, T, heads, hd)
    o_ref, lse_ref = _reference(qkv, N, T, heads, hd)
    assert rel(o, o_ref) < ATTN_TOL[precision], (precision, rel(o, o_ref))
    assert rel(lse, lse_ref) < ATTN_TOL[precision], (precision, rel(lse, lse_ref))
    o2, _ = _attention(qkv, N, T, heads, hd, with_lse=False)
    assert np.array_equal(o, o2)                       # writing lse changes nothing else


@pytest.mark.parametrize("N,T,heads,hd", [(2, 256, 16, 72), (3, 200, 16, 72), (2, 100, 16, 72), (2, 288, 6, 64), (1, 37, 6, 64)])
def test_streaming_kernel_agrees_with_the_resident_kernel(N, T, heads, hd, precision):
    """rgm_set_attn_stream(1) sends every length to the streaming kernel: on the same inputs it must agree with the resident
    kernels (K and V of a head in LDS) within the fp64 tolerances, and with the fp64 restatement itself."""
    from gpu_util import rel
    from rgm import native as R
    qkv = _qkv(N, T, heads, hd, 7 * T + hd)
    o_res, l_res = _attention(qkv, N, T, heads, hd)
    prev = R.lib.rgm_set_attn_stream(1)
    try:
        o_str, l_str = _attention(qkv, N, T, heads, hd)
    finally:
        R.lib.rgm_set_attn_stream(prev)
    o_ref, l_ref = _reference(qkv, N, T, heads, hd)
    tol = ATTN_TOL[precision]
    assert rel(o_str, o_ref) < tol and rel(l_str, l_ref) < tol
    assert rel(o_str, o_res) < 2 * tol and rel(l_str, l_res) < 2 * tol


def test_streaming_kernel_repeats_bitwise(precision):
    """DESIGN 4h soak discipline on the new kernel: 200 launches of a grid of 1024 workgroups (four per CU of the chip) on fixed inputs give rows
    bitwise equal to the first launch.  Checks that results repeat; nothing here provokes anything."""
    from gpu_util import dev
    from rgm import native as R
    from rgm.synth import rotary_freqs
    N, T, heads, hd = 16, 1024, 16, 72
    qkv = dev(_qkv(N, T, heads, hd, 99))
    cos, sin = odit.rotary_tables(rotary_freqs(36), T)
    cd, sd_ = dev(cos), dev(sin)
    outs = [torch.full((N * T, heads * hd), float("nan"), device="cuda") for _ in range(2)]
    lses = [torch.full((N * heads * T,), float("nan"), device="cuda") for _ in range(2)]
    st = R.current_stream()

    def launch(i):
        R.check(R.lib.rgm_rotary_attention_lse(R.ptr(qkv), R.ptr(outs[i]), R.ptr(lses[i]), R.ptr(cd), R.ptr(sd_), N, T, heads, hd, 18, st))
    launch(0)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0]).all()) and bool(torch.isfinite(lses[0]).all())
    bad = []
    for i in range(200):
        launch(1)
        if not (torch.equal(outs[0], outs[1]) and torch.equal(lses[0], lses[1])):
            bad.append((i, int((outs[0] != outs[1]).sum()), int((lses[0] != lses[1]).sum())))
    torch.cuda.synchronize()
    assert not bad, bad[:5]


def _eps_model(arch):
    from guided_diffusion.dit import DiTRotary
    return DiTRotary(input_size=[128, 16], patch_size=arch["patch"], in_channels=arch["in_ch"], hidden_size=arch["hidden"],
                     depth=arch["depth"], num_heads=arch["heads"], num_classes=arch.get("num_classes", 0), learn_sigma=False)


@pytest.mark.parametrize("tag,arch,shapes", [("xl2", XL2, (136, 256, 512)), ("xl28", XL28, (256,))])
def test_long_dit_forward_matches_reference(tag, arch, shapes, precision):
    from gpu_util import dev, rel, load_module
    from guided_diffusion.dit import cond_hint
    g = load_golden(f"long_dit_{tag}")
    m = load_module(_eps_model(arch), synth.dit_state_dict(int(g["seed"][0]), device="cuda", **arch))
    for H in shapes:
        x, t, y = dev(g[f"x{H}"]), dev(g[f"t{H}"]), dev(g[f"y{H}"])
        out = m(x, t, y)
        assert out.shape == (x.shape[0], 4, H, 16)
        assert rel(out.cpu().numpy(), g[f"out{H}"]) < TOL, (tag, H, precision)
    H = shapes[-1] if tag == "xl28" else 256
    x, t, y = dev(g[f"x{H}"]), dev(g[f"t{H}"]), dev(g[f"y{H}"])
    # batch invariance: bitwise (same tiles, same arithmetic); rows of one timestep through the conditioning computed ahead: bitwise too
    a = m(x.repeat(3, 1, 1, 1), t.repeat(3), y.repeat(3))
    B = x.shape[0]
    assert torch.equal(a[:B], a[B:2 * B]) and torch.equal(a[:B], a[2 * B:])
    t0 = int(g[f"t{H}"][0])
    tt = torch.full_like(t, t0)
    plain = m(x, tt, y)
    with cond_hint((t0, [t0, max(t0 - 20, 0)])):
        ahead = m(x, tt, y)
    assert getattr(m, "_ahead", None) is not None                   # the rows-ahead path (rgm_dit_forward_cond) ran
    assert torch.equal(plain, ahead)


def test_long_dit_forward_as_two_half_batches_is_bitwise():
    """The blocks of a forward as two half batches on two streams (rgm_set_dit_halves) reach the streaming attention with half the
    samples each: the rows must not change."""
    from gpu_util import dev, load_module
    from rgm import native as R
    from ctypes import byref, c_int
    g = load_golden("long_dit_xl2")
    m = load_module(_eps_model(XL2), synth.dit_state_dict(int(g["seed"][0]), device="cuda", **XL2))
    x, t, y = dev(g["x256"]), dev(g["t256"]), dev(g["y256"])
    x4, t4, y4 = x.repeat(2, 1, 1, 1), t.repeat(2), y.repeat(2)
    prev = c_int(0)
    R.check(R.lib.rgm_set_dit_halves(0, byref(prev)))
    try:
        one = m(x4, t4, y4)
        R.check(R.lib.rgm_set_dit_halves(2, None))
        two = m(x4, t4, y4)
    finally:
        R.check(R.lib.rgm_set_dit_halves(prev.value, None))
    assert torch.equal(one, two)


def _diffusion(rs):
    from guided_diffusion.script_util import create_diffusion
    return create_diffusion(learn_sigma=False, diffusion_steps=1000, noise_schedule="linear", timestep_respacing=rs,
                            use_kl=False, predict_xstart=False, rescale_timesteps=False, rescale_learned_sigmas=False)


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


def test_long_ddim_step_and_chain(precision):
    from gpu_util import dev, load_module, rel
    from oracle import diffusion_np as odf
    g = load_golden("long_ddim")
    sd = synth.dit_state_dict(int(g["seed"][0]), **XL2)
    m = load_module(_eps_model(XL2), sd)
    d = _diffusion("ddim50")
    d.t_end = 0
    _inject(d, g["noise"])
    out = d.ddim_sample(_model_fn(m), dev(g["x"]), dev(g["t"]), clip_denoised=False, eta=1.0, model_kwargs={"y": dev(g["y"])})
    assert rel(out["sample"].cpu().numpy(), g["sample"]) < TOL
    assert rel(out["pred_xstart"].cpu().numpy(), g["pred_xstart"]) < TOL
    # a 3-step teacher-forced chain against the numpy oracle (latents within the 1e-3 contract)
    rng = np.random.RandomState(703)
    B, H = 2, 256
    xT = rng.randn(B, 4, H, 16).astype(F32)
    nz = [rng.randn(B, 4, H, 16).astype(F32) for _ in range(3)]
    d3 = _diffusion("ddim3")
    _inject(d3, xT, *nz)
    y = g["y"]
    lat = d3.ddim_sample_loop(_model_fn(m), (B, 4, H, 16), clip_denoised=False, model_kwargs={"y": dev(y)}, device="cuda", eta=1.0)

    def omodel(x, t, y=None, rule=None):
        return odit.dit_forward(sd, x, t, y, depth=2, heads=16, patch=8)
    ref = odf.sample_loop(odf.Schedule(1000, "linear", "ddim3"), omodel, xT, nz, ddim=True, eta=1.0, model_kwargs={"y": y})
    assert rel(lat.cpu().numpy(), ref) < 1e-3


def _load_cli(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(f"{name}_long_cli", os.path.join(PKG, "scripts", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _scg_pitch_config(tmp_path, nd=None):
    lines = ["target_rules:", "  pitch_hist: [0.5, 0., 0., 0., 0.25, 0., 0., 0.25, 0., 0., 0., 0.]"]
    if nd is not None:
        lines += [f"  vertical_nd: {[3.] * nd}", f"  horizontal_nd: {[15.] * nd}"]
    lines += ["guidance:", "  vae: True", "  nn: False", "  scg: True", "  method: no_guidance", "  cond_fn: Null", "  schedule: True",
              "  t_start: 1000", "  t_end: 0", "  interval: 1", "scg:", "  num_samples: 4", "  pitch_hist: 40."]
    if nd is not None:
        lines += ["  note_density: 1."]
    lines += ["sampling:", "  use_ddim: False", "  diff_collage: False", "  t_end: 0"]
    p = os.path.join(str(tmp_path), "configs", "cond_demo", "long_pitch.yml")
    os.makedirs(os.path.dirname(p), exist_ok=True)
    with open(p, "w") as f:
        f.write("\n".join(lines) + "\n")
    return p


CLI_COMMON = ["--model", "DiTRotary_B_8", "--image_size", "256", "16", "--in_channels", "4", "--scale_factor", "1.2465",
              "--class_cond", "True", "--num_classes", "3", "--class_label", "1", "--synthetic_weights", "True", "--progress", "False"]


def test_sample_rule_cli_long_excerpt(tmp_path, monkeypatch, precision):
    import pandas as pd
    monkeypatch.chdir(tmp_path)
    cli = _load_cli("sample_rule")
    cfg = _scg_pitch_config(tmp_path)
    args = ["--config_path", cfg, "--batch_size", "2", "--num_samples", "2", "--diffusion_steps", "24", "--gemm_precision", precision]
    res = cli.main(args + CLI_COMMON)
    out_dir = os.path.join("loggings", cli.output_dir_for(cfg, 1))
    df = pd.read_csv(os.path.join(out_dir, "results.csv"))
    assert len(df) == 2 and len(res) == 2
    assert {"pitch_hist.target_rule", "pitch_hist.gen_rule", "pitch_hist.loss"} <= set(df.columns)
    assert np.isfinite(df["pitch_hist.loss"]).all()
    assert os.path.exists(os.path.join(out_dir, "summary.csv"))
    roll = np.load(os.path.join(out_dir, "sample_0_y_1.npy"))
    assert roll.shape == (3, 128, 2048) and roll.dtype == np.uint8 and roll.max() <= 127
    # note_density targets made for 1024 frames do not fit 2048: refused with both lengths named
    bad = _scg_pitch_config(tmp_path, nd=8)
    with pytest.raises(ValueError, match=r"1024 frames.*2048 frames"):
        cli.main(["--config_path", bad, "--batch_size", "2", "--num_samples", "2", "--diffusion_steps", "24"] + CLI_COMMON)


def test_cfg_sample_cli_long_excerpt(tmp_path, monkeypatch, precision):
    monkeypatch.chdir(tmp_path)
    cli = _load_cli("cfg_sample")
    arr = cli.main(["--model", "DiTRotary_B_8", "--image_size", "256", "16", "--in_channels", "4", "--scale_factor", "1.2465",
                    "--class_cond", "True", "--num_classes", "3", "--class_label", "1", "--cfg", "True", "--w", "2.0",
                    "--synthetic_weights", "True", "--progress", "False", "--batch_size", "2", "--num_samples", "2",
                    "--diffusion_steps", "24", "--gemm_precision", precision, "--dir", str(tmp_path / "out")])
    assert arr.shape == (2, 3, 128, 2048) and arr.dtype == np.uint8 and arr.max() <= 127
    u8 = np.asarray(arr)
    assert np.isfinite(u8.astype(np.float32)).all()


def test_long_guidance_needs_the_backward_and_says_so(precision):
    from functools import partial
    from types import SimpleNamespace
    from gpu_util import load_module
    from guided_diffusion.dit import DiTRotaryClassifier
    from guided_diffusion.condition_functions import composite_nn_zt
    from rgm.native import RgmError
    arch = dict(depth=2, hidden=384, heads=6, patch=8, in_ch=4, classifier=True, cls_classes=16)
    clf = DiTRotaryClassifier(input_size=[128, 16], patch_size=8, in_channels=4, hidden_size=384, depth=2, num_heads=6, num_classes=16)
    clf = load_module(clf, synth.dit_state_dict(4, **arch))
    x = torch.randn(2, 4, 256, 16, device="cuda")
    t = torch.tensor([500, 20], device="cuda")
    assert clf(x, t).shape == (2, 16)                           # the classifier FORWARD runs at the new length
    with pytest.raises(NotImplementedError, match="288 tokens"):
        clf.value_and_grad(x, t, torch.zeros(2, 16, device="cuda"), "mse", 1.0)
    # DPS through p_sample: refused before the step's first launch
    m = load_module(_eps_model(XL2), synth.dit_state_dict(1, device="cuda", **XL2))
    d = _diffusion("250")
    d.t_end = 0
    cond = partial(composite_nn_zt, fns=["nn_z0_mse_dummy"], classifier_scales=[1.], classifiers=[clf], rule_names=["note_density"])
    gk = SimpleNamespace(schedule=False, method="dps", step_size=1.0, nn=True, vae=False)
    with pytest.raises(NotImplementedError, match="256 tokens"):
        d.p_sample(_model_fn(m), x, torch.full((2,), 120, device="cuda"), clip_denoised=False, cond_fn=cond, guidance_kwargs=gk,
                   model_kwargs={"y": torch.tensor([1, 2], device="cuda"), "rule": torch.zeros(2, 32, device="cuda")})
    with pytest.raises(NotImplementedError, match="256 tokens"):
        m.vjp_forward(x, t, torch.tensor([1, 2], device="cuda"))
    # beyond the streaming kernel's ceiling: the native error
    with pytest.raises(RgmError):
        m(torch.zeros(1, 4, 4104, 16, device="cuda"), torch.zeros(1, dtype=torch.long, device="cuda"), torch.zeros(1, dtype=torch.long,
                                                                                                               device="cuda"))
