"""-m gpu: long excerpts at the edges of their range.  The streaming attention forward (csrc/attention_stream.hip) at its 8192-token
ceiling, at partial query tiles / key blocks and at the smallest lengths; the DiTRotary forward at T = 8192 and T = 2080 against the
oracle and the reference's slices (tests/golden/make_golden_long.py), with a native handle that grows and then serves shorter
requests; and what runs after the eps-network at long lengths: the VAE decode of 64 squares into one roll, the rule kernels over up
to 32768 frames and one SCG step at 2048 frames."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import dit_np as odit
from rgm import synth
from test_gpu_long import ATTN_TOL, TOL, XL2, _attention, _eps_model, _qkv

pytestmark = pytest.mark.gpu
F32 = np.float32
SM = dict(depth=2, hidden=384, heads=6, patch=8, in_ch=4, out_ch=4, num_classes=3)
SQ = 256                  # queries per workgroup of the streaming kernel
_HOST = {}                # host-side references, computed once per session (the precision fixture reruns every test)


def _cached(key, fn):
    if key not in _HOST:
        _HOST[key] = fn()
    return _HOST[key]


# ----------------------------------------------------------------------------------------------- 1. the streaming attention
def _check_rows(T):
    """query rows the fp64 reference computes: every row of the first and the last 256-query tile (and the last 256 rows), every
    7th row in between; each against ALL keys -- attention rows are independent, so no row's result depends on which are checked"""
    last = (T - 1) // SQ * SQ
    return np.unique(np.concatenate((np.arange(min(SQ, T)), np.arange(SQ, T, 7), np.arange(last, T), np.arange(max(T - SQ, 0), T))))


def _reference_rows(qkv, N, T, heads, hd, rows):
    """fp64 restatement of test_gpu_long._reference at the query rows `rows` only: (o (N, R, heads*hd), lse (N, heads, R))"""
    from rgm.synth import rotary_freqs
    cos, sin = odit.rotary_tables(rotary_freqs(int(hd * 0.5)), T)
    r = qkv.reshape(N, T, 3, heads, hd)
    o = np.zeros((N, len(rows), heads, hd))
    lse = np.zeros((N, heads, len(rows)))
    for n in range(N):
        for h in range(heads):
            q = odit.apply_rotary(r[n, rows, 0, h][None, None], cos[rows], sin[rows])[0, 0].astype(np.float64)
            k = odit.apply_rotary(r[n, :, 1, h][None, None], cos, sin)[0, 0].astype(np.float64)
            v = r[n, :, 2, h].astype(np.float64)
            s = q @ k.T * hd ** -0.5
            m = s.max(-1, keepdims=True)
            p = np.exp(s - m)
            l = p.sum(-1, keepdims=True)
            o[n, :, h] = (p / l) @ v
            lse[n, h] = (m + np.log(l))[:, 0]
    return o.reshape(N, len(rows), heads * hd), lse


def _attn_tol(precision, T):
    """ATTN_TOL holds for T <= 2048, where it was set.  The exact-fp32 path sums each query's T products p * v in fp32: the rounding
    errors of such a sum grow like sqrt(T) (the bf16x3 bound is set by the split error, which does not depend on T), so four times
    as many keys at the ceiling double the fp32 bound."""
    if precision == "fp32" and T > 2048:
        return ATTN_TOL["fp32"] * np.sqrt(8192 / 2048)
    return ATTN_TOL[precision]


def _check_attention(N, T, heads, hd, seed, precision):
    from gpu_util import rel
    qkv = _qkv(N, T, heads, hd, seed)
    o, lse = _attention(qkv, N, T, heads, hd)
    assert np.isfinite(o).all() and np.isfinite(lse).all()          # every row and every lse entry written (NaN-filled before)
    rows = _check_rows(T)
    o_ref, lse_ref = _cached(("attn", N, T, heads, hd, seed), lambda: _reference_rows(qkv, N, T, heads, hd, rows))
    o = o.reshape(N, T, heads * hd)[:, rows]
    tol = _attn_tol(precision, T)
    assert rel(o, o_ref) < tol, (precision, rel(o, o_ref))
    assert rel(lse[:, :, rows], lse_ref) < tol, (precision, rel(lse[:, :, rows], lse_ref))
    return qkv, o


@pytest.mark.parametrize("N,T,heads,hd", [(1, 8192, 16, 72), (1, 8192, 6, 64), (2, 4096, 16, 72), (1, 8160, 16, 72), (1, 6001, 6, 64)])
def test_streaming_attention_at_the_ceiling_and_partial_tiles(N, T, heads, hd, precision):
    """T = 8192: 128 key blocks of 64 into one running max and sum per query, the widest grid; 8160 = 31 * 256 + 224 = 127 * 64 + 32:
    the last query tile and the last key block are both partial; 6001: any T through the C ABI"""
    _check_attention(N, T, heads, hd, T + 3 * hd, precision)


@pytest.mark.parametrize("heads,hd", [(16, 72), (6, 64)])
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 255, 257])
def test_streaming_attention_at_the_smallest_lengths(T, heads, hd, precision):
    """rgm_set_attn_stream(1) sends short lengths to the streaming kernel: one key, the edges of one 64-key block, one query tile.
    At T = 1 the single probability is exactly 1, so o = V: bit for bit in fp32 (exp(0) = 1, 1 / 1 = 1, products by 1 and sums with
    masked zeros are exact); with the bf16x3 split o = hi(V) + lo(V), whose error is at most 2^-8 * 2^-8 |V| (two RNE bf16 roundings,
    and hi + lo spans at most 17 bits, exact in fp32)."""
    from rgm import native as R
    N = 2
    prev = R.lib.rgm_set_attn_stream(1)
    try:
        qkv, o = _check_attention(N, T, heads, hd, 11 * T + hd, precision)
    finally:
        R.lib.rgm_set_attn_stream(prev)
    if T == 1:
        D = heads * hd
        v = qkv.reshape(N, 1, 3 * D)[:, :, 2 * D:]
        if precision == "fp32":
            assert np.array_equal(o, v)
        else:
            assert (np.abs(o - v) <= 2.0 ** -16 * np.abs(v)).all(), np.abs(o - v).max()


@pytest.mark.parametrize("heads,hd", [(16, 72), (6, 64)])
def test_streaming_attention_refuses_one_token_past_the_ceiling(heads, hd, precision):
    """T = 8193: both entry points return an error status before any launch; the NaN-filled output comes back untouched"""
    from gpu_util import dev
    from rgm import native as R
    from rgm.synth import rotary_freqs
    N, T = 1, 8193
    rot = int(hd * 0.5)
    cos, sin = odit.rotary_tables(rotary_freqs(rot), T)
    qd, cd, sd_ = dev(_qkv(N, T, heads, hd, 5)), dev(cos), dev(sin)
    od = torch.full((N * T, heads * hd), float("nan"), device="cuda")
    ld = torch.full((N * heads * T,), float("nan"), device="cuda")
    st = R.current_stream()
    assert R.lib.rgm_rotary_attention(R.ptr(qd), R.ptr(od), R.ptr(cd), R.ptr(sd_), N, T, heads, hd, rot // 2, st) != 0
    assert R.lib.rgm_rotary_attention_lse(R.ptr(qd), R.ptr(od), R.ptr(ld), R.ptr(cd), R.ptr(sd_), N, T, heads, hd, rot // 2, st) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(od).all()) and bool(torch.isnan(ld).all())


# ----------------------------------------------------------------------------------------------- 2. the DiTRotary forward at the ceiling
EDGE = "long_dit_xl2_edge"


def _edge_input(g, H):
    B = len(g[f"t{H}"])
    return np.random.RandomState(int(g[f"x{H}_seed"][0])).randn(B, 4, H, 16).astype(F32)


@pytest.mark.parametrize("H", [1040, 4096])
def test_dit_forward_at_the_ceiling_matches_oracle_and_reference(H, precision):
    """XL-2 at T = 2080 (B 2: partial last query tile and key block) and T = 8192 (the ceiling): the whole output against the numpy
    oracle, the stored rows against the reference"""
    from gpu_util import dev, load_module, rel
    g = load_golden(EDGE)
    sd = synth.dit_state_dict(int(g["seed"][0]), **XL2)
    x, t, y = _edge_input(g, H), g[f"t{H}"], g[f"y{H}"]
    m = load_module(_eps_model(XL2), sd)
    out = m(dev(x), dev(t), dev(y)).cpu().numpy()
    ora = _cached(("dit", H), lambda: odit.dit_forward(sd, x, t, y, depth=2, heads=16))
    assert rel(out, ora) < TOL, (H, precision, rel(out, ora))
    assert rel(out[:, :, g[f"rows{H}"]], g[f"out{H}"]) < TOL, (H, precision)


def test_dit_handle_grows_and_serves_shorter_requests_again(precision):
    """ONE module at H = 128 -> 4096 -> 128 -> 512: the native handle is destroyed and rebuilt for T = 8192 (_ensure_native) and then
    serves the shorter lengths.  Every output is bitwise equal to a freshly built module's on the same input, the conditioning rows
    computed ahead (cond_hint) included: their cache keys on _version, which the rebuild bumps, so no row of the old handle is served."""
    from gpu_util import dev, load_module
    from guided_diffusion.dit import cond_hint
    g = load_golden(EDGE)
    sd = synth.dit_state_dict(int(g["seed"][0]), **XL2)
    m = load_module(_eps_model(XL2), sd)
    rng = np.random.RandomState(77)
    y = dev(np.array([1], dtype=np.int64))

    def fresh(x, t):
        f = load_module(_eps_model(XL2), sd)
        out = f(x, t, y)
        del f
        return out

    t0 = 640
    tt = dev(np.array([t0], dtype=np.int64))
    hint = (t0, [t0, t0 - 20])
    x128 = dev(rng.randn(1, 4, 128, 16).astype(F32))
    with cond_hint(hint):
        a = m(x128, tt, y)
    assert m._ahead is not None and m._ahead["key"][0] == m._version
    assert torch.equal(a, fresh(x128, tt))
    v0, passes0 = m._version, m.ahead_passes
    x4096 = dev(rng.randn(1, 4, 4096, 16).astype(F32))
    t4096 = dev(np.array([911], dtype=np.int64))
    assert torch.equal(m(x4096, t4096, y), fresh(x4096, t4096))
    assert m._max_tokens == 8192 and m._version > v0                # rebuilt for the long request, parameters uploaded again
    with cond_hint(hint):
        b = m(x128, tt, y)                                          # the same hint as before the rebuild: rows computed again
    assert m.ahead_passes == passes0 + 1 and m._ahead["key"][0] == m._version
    assert torch.equal(b, a)
    x512 = dev(rng.randn(1, 4, 512, 16).astype(F32))
    t512 = dev(np.array([37], dtype=np.int64))
    assert torch.equal(m(x512, t512, y), fresh(x512, t512))
    assert m._max_tokens == 8192                                    # shorter requests keep the grown handle


# ----------------------------------------------------------------------------------------------- 3. past the eps-network
def _vae(seed=2):
    from gpu_util import load_module
    from taming.models.klvae_pedal import AutoencoderKL
    return load_module(AutoencoderKL(), synth.vae_state_dict(seed, encoder=True))


def test_decode_of_64_squares_into_one_roll(precision):
    """decode_latent at H = 1024 (64 squares, 8192 frames; decode_impl with S = 64), float and uint8 at once: squares 0, 1, 31 and 63
    against the numpy decoder, the whole roll against the generic tile path, the uint8 roll against the oracle's quantiser"""
    from gpu_util import dev, rel
    from oracle import vae_np as ovae
    H, S, scale = 1024, 64, 1.2465
    lat = (np.random.RandomState(901).randn(1, 4, H, 16) * 1.2).astype(F32)
    vae = _vae(2)
    roll, u8 = vae.decode_latent(dev(lat), scale_factor=scale, want_u8=True, want_float=True)
    assert roll.shape == (1, 3, 128, 8 * H) and u8.shape == (1, 128, 8 * H, 3) and u8.dtype == torch.uint8
    roll, u8 = roll.cpu().numpy(), u8.cpu().numpy()
    z = np.ascontiguousarray((lat / F32(scale)).transpose(0, 1, 3, 2))            # (1, 4, 16 pitch, H time)
    picks = (0, 1, 31, 63)
    vsd = synth.vae_state_dict(2, encoder=True)
    ref = _cached("vae_squares", lambda: ovae.decode(vsd, np.concatenate([z[..., 16 * s:16 * s + 16] for s in picks])))
    for i, s in enumerate(picks):
        assert rel(roll[:, :, :, 128 * s:128 * s + 128], ref[i:i + 1]) < 5e-5, (s, precision)
    tiles = torch.cat(torch.chunk(dev(z), S, dim=-1), dim=0).contiguous()
    whole = torch.cat(torch.chunk(vae.decode(tiles), S, dim=0), dim=-1).cpu().numpy()
    assert rel(roll, whole) < 5e-5, precision
    assert np.array_equal(ovae.quantise_roll(roll), u8)


def _edge_roll(rng, n, T):
    """sparse (N, 3, 128, T) roll: background below the -0.95 threshold but never exactly -1 (the in-place snap shows), random notes
    that never start on a multiple of 256; at every EVEN 256-column block start a note starts (its onset needs the previous column,
    which the previous workgroup of note_density_kernel owns), across every ODD one only sustained notes run (no onset there);
    notes start in the last 16 columns and run into the last column"""
    r = (-1 + 0.04 * rng.rand(n, 3, 128, T)).astype(F32)
    for b in range(n):
        for _ in range(40 * T // 1024 + 5):
            p, s, L = rng.randint(0, 128), rng.randint(1, T - 8), rng.randint(4, 120)
            if s % 256 == 0:
                s += 1
            r[b, 0, p, s:s + L] = rng.uniform(-0.5, 1.0)
            r[b, 1, p, s] = 1.0
        for k in range(1, T // 256):
            c = 256 * k
            p = rng.randint(21, 109)
            if k % 2 == 0:
                r[b, 0, p, c:c + rng.randint(2, 40)] = rng.uniform(-0.5, 1.0)
            else:
                r[b, 0, p, c - rng.randint(1, 30):c + rng.randint(1, 30)] = rng.uniform(-0.5, 1.0)
        for p, s in ((rng.randint(21, 109), T - 7), (rng.randint(21, 109), T - 100), (rng.randint(21, 109), T - 129)):
            r[b, 0, p, s:] = rng.uniform(-0.5, 1.0)
    return r


@pytest.mark.parametrize("T", [2048, 8192, 32768])
def test_rule_kernels_over_long_rolls(T, precision):
    """FUNC_DICT's kernels and chord_quantise against oracle/rules_np.py over 2048 .. 32768 frames: counts bit-exact, pitch_hist within
    1e-6, the in-place writes into the roll equal"""
    from gpu_util import dev, rel
    from music_rule_guidance import music_rules
    from music_rule_guidance.rule_maps import FUNC_DICT
    from oracle import rules_np
    roll = _edge_roll(np.random.RandomState(T), 2, T)
    for name in ("note_density", "note_density_hr_1", "note_density_hr_2", "note_density_class", "note_density_pixel"):
        r = dev(roll)
        out = FUNC_DICT[name](r).cpu().numpy()
        ro = roll.copy()
        want = rules_np.FUNC_DICT[name](ro)
        assert out.shape == want.shape and np.array_equal(out, want), name
        assert np.array_equal(r.cpu().numpy(), ro), f"{name}: in-place writes differ"
    r = dev(roll)
    ro = roll.copy()
    assert rel(FUNC_DICT["pitch_hist"](r).cpu().numpy(), rules_np.pitch_hist(ro)) < 1e-6
    assert np.array_equal(r.cpu().numpy(), ro)
    r = dev(roll)
    ro = roll.copy()
    assert np.array_equal(music_rules.chord_quantise(r).cpu().numpy(), rules_np.chord_quantise(ro))
    assert np.array_equal(r.cpu().numpy(), ro)


def test_scg_step_at_2048_frames(precision):
    """one teacher-forced DDPM step with SCG (n = 4, B = 2) at H = 256: pitch_hist and note_density targets of 2048 frames, against
    odf.p_sample with the numpy DiT and the same noise; the oracle decodes through the GPU decoder's tile path (checked above)"""
    from types import SimpleNamespace
    from functools import partial
    from gpu_util import dev, load_module, rel
    from guided_diffusion.condition_functions import model_fn
    from guided_diffusion.script_util import create_diffusion
    from oracle import diffusion_np as odf
    from oracle import rules_np as orl
    B, n, H = 2, 4, 256
    sd = synth.dit_state_dict(11, **SM)
    m = load_module(_eps_model(SM), sd)
    vae = _vae(2)
    rng = np.random.RandomState(905)
    x = rng.randn(B, 4, H, 16).astype(F32)
    nz = rng.randn(n, B, 4, H, 16).astype(F32)
    y = np.array([1, 2], dtype=np.int64)
    t = np.full((B,), 500, dtype=np.int64)
    nd = 2 * 8 * H // 128
    tgt = {"pitch_hist": np.tile(np.array([0.5, 0, 0, 0, 0.25, 0, 0, 0.25, 0, 0, 0, 0], dtype=F32), (B, 1)),
           "note_density": np.tile(np.array([3.] * (nd // 2) + [2.] * (nd // 2), dtype=F32), (B, 1))}
    scg = {"num_samples": n, "pitch_hist": 40., "note_density": 1.}
    d = create_diffusion(learn_sigma=False, diffusion_steps=1000, noise_schedule="linear", timestep_respacing="", use_kl=False,
                         predict_xstart=False, rescale_timesteps=False, rescale_learned_sigmas=False)
    d.t_end = 0
    q = [torch.from_numpy(nz)]
    d.noise_fn = lambda shape, device: q.pop(0).to(device)
    out = d.p_sample(partial(model_fn, model=m, num_classes=3, class_cond=True, cfg=False, w=0.), dev(x), dev(t), clip_denoised=False,
                     model_kwargs={"y": dev(y), "rule": {k: dev(v) for k, v in tgt.items()}}, embed_model=vae, scale_factor=1.2465,
                     guidance_kwargs=SimpleNamespace(schedule=True, t_start=750, t_end=0, interval=1, method="no_guidance"),
                     scg_kwargs=scg)

    def omodel(x, t, y=None, rule=None):
        return odit.dit_forward(sd, x, t, y, depth=2, heads=6)

    def decode(z):
        return vae.decode(dev(z)).cpu().numpy()
    o = odf.p_sample(odf.Schedule(1000, "linear", ""), omodel, x, t, nz, model_kwargs={"y": y, "rule": tgt},
                     guidance=dict(schedule=True, t_start=750, t_end=0, interval=1), scg_kwargs=scg, decode_fn=decode,
                     scale_factor=1.2465, func_dict=orl.FUNC_DICT, loss_dict=orl.LOSS_DICT, return_aux=True)
    assert np.array_equal(d.last_scg["max_ind"].cpu().numpy(), o["aux"]["max_ind"])
    assert rel(out["sample"].cpu().numpy(), o["sample"]) < TOL
