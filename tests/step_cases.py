"""Yardsticks of the sampler, SCG, rule and collage kernel tests (csrc/sampler.hip, rules.hip, collage.hip; docs/rounds/step_inputs.md):
seeded, named case generators, float64 references, float32 restatements in the kernels' own operation order, and the error measures.
Plain helpers: no GPU, no pytest fixtures.  tests/test_step_cases_host.py shows on the CPU that the references are right and the cases
hard; tests/test_gpu_step_inputs.py holds the kernels to them.

Every bound below is 4 x the worst ratio of a float32 restatement against float64, measured on the CPU (the constants are fixed here and
re-measured by the host test); a figure of a kernel never enters one."""
import numpy as np
import torch

F32 = np.float32
U = 2.0 ** -24                                   # unit round-off of float32
FACTOR = 4.0                                     # bound = FACTOR x the restatement's worst ratio (another libm, fused multiply-adds)
NAN = float("nan")

# ------------------------------------------------------------------------------------ measured on the CPU, fixed (docs/rounds/step_inputs.md)
MEASURED = {                                     # worst ratio of the float32 restatement against float64 over every case of the kernel
    "randn": 4.5973,                             # |z32 - z64| / (2^-24 (1 + rad)) of normals32 over RANDN_CASES
    "ddpm.sample": 4.2813, "ddpm.pred_xstart": 1.5474, "ddpm.g": 1.2303,        # |out - ref64| / (2^-24 A), section 3
    "learned.sample": 4.1074, "learned.pred_xstart": 1.5474, "learned.g": 1.4952,
    "ddim.sample": 2.1919, "ddim.pred_xstart": 3.2548, "ddim.g": 0.2096,
    "xstart.out": 2.0090, "edit.out": 2.5349,
    "pitch.hist": 0.3095,                        # per-class |hist - hist64| / 2^-24
    "vag.logp": 2.7839,                          # |logp - logp64| / (2^-24 |logp64|)
    "vag.hist": 0.3095,
    "vag.dh": 6.2601,                            # |dh - dh64| / (2^-24 max_c |u_c| / d)
}
FLOOR = {"pitch.hist": 1.0, "vag.hist": 1.0}     # in units of 2^-24


def bound(name):
    """FACTOR x the restatement's worst ratio, in units of 2^-24 (times the measure's own scale)"""
    return max(FACTOR * MEASURED[name], FLOOR.get(name, 0.0))


RANDN_K = bound("randn")


# ==================================================================================== 1. Philox normals
_M = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
KAT = [  # Random123 kat_vectors, philox4x32 10 rounds: counter, key, output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(ctr, key):
    """ctr: four uint64 arrays holding 32-bit words, key: two 32-bit ints -> four uint64 arrays of 32-bit words (Salmon et al. 2011)"""
    c = [np.asarray(w, dtype=np.uint64) & _M for w in ctr]
    k0, k1 = np.uint64(key[0] & 0xFFFFFFFF), np.uint64(key[1] & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & _M, (p0 >> _S32) ^ c[3] ^ k1, p0 & _M]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M, (k1 + np.uint64(0xBB67AE85)) & _M
    return c


def stream_words(seed, offset, n):
    """the two 32-bit words behind each of the n normals at stream positions offset .. offset + n - 1, and the lane parity:
    position p lies in block p >> 2 (counter words (block & 2^32-1, block >> 32, 0, 0), key (seed & 2^32-1, seed >> 32)), lane p & 3;
    lanes 0 / 1 are the cosine / sine of words (0, 1), lanes 2 / 3 of words (2, 3)"""
    pos = np.array([offset + i for i in range(n)], dtype=np.uint64) if n < 64 else np.uint64(offset) + np.arange(n, dtype=np.uint64)
    blk, lane = pos >> np.uint64(2), (pos & np.uint64(3)).astype(np.int64)
    z = np.zeros_like(blk)
    r = philox4x32_10((blk & _M, blk >> _S32, z, z), (seed & 0xFFFFFFFF, seed >> 32))
    hi = lane >= 2
    ra, rb = np.where(hi, r[2], r[0]), np.where(hi, r[3], r[1])
    return ra, rb, (lane & 1).astype(bool)


def normals64(seed, offset, n):
    """-> (z, rad) float64: Box-Muller on u1 = ((w >> 8) + 1) 2^-24 in (0, 1], u2 = (w' >> 8) 2^-24 in [0, 1): both exact in float32"""
    ra, rb, sine = stream_words(seed, offset, n)
    u1 = ((ra >> np.uint64(8)).astype(np.float64) + 1.0) * U
    u2 = (rb >> np.uint64(8)).astype(np.float64) * U
    rad = np.sqrt(-2.0 * np.log(u1))
    ang = 2.0 * np.pi * u2
    return rad * np.where(sine, np.sin(ang), np.cos(ang)), rad


def normals32(seed, offset, n):
    """the kernel's philox_normals restated in numpy float32, operation by operation"""
    ra, rb, sine = stream_words(seed, offset, n)
    u1 = ((ra >> np.uint64(8)).astype(F32) + F32(1)) * F32(U)
    u2 = (rb >> np.uint64(8)).astype(F32) * F32(U)
    rad = np.sqrt(F32(-2) * np.log(u1))
    ang = F32(6.283185307179586) * u2
    return (rad * np.where(sine, np.sin(ang), np.cos(ang))).astype(F32)


SEEDS = (0, 1, 2 ** 63 + 12345)
P34 = 2 ** 34                                    # stream position whose block counter is 2^32: the second counter word becomes 1
RANDN_CASES = [(s, off + r, n) for s in SEEDS for r in range(4) for off, n in ((0, 1), (4, 2), (8, 3), (1000, 5), (12, 1027))] + \
              [(s, P34 - 513 + r, 1027) for s in SEEDS for r in range(4)]


def randn_ratio(z, seed, offset):
    """worst |z - z64| / (2^-24 (1 + rad)) of n normals at (seed, offset)"""
    z64, rad = normals64(seed, offset, len(z))
    return float(np.max(np.abs(np.asarray(z, np.float64) - z64) / (U * (1.0 + rad))))


# ==================================================================================== 2. SCG
def scg_candidates64(mean, g, noise):
    """(B, E), (B,) or (B, E), (n, B, E) -> value and the bound's scale |mean| + |g z|, float64"""
    m, z = mean.astype(np.float64)[None], noise.astype(np.float64)
    gg = g.astype(np.float64)
    gg = gg[None, :, None] if gg.ndim == 1 else gg[None]
    return m + gg * z, np.abs(m) + np.abs(gg * z)


def argmax_first_nan(total):
    """(n, B) -> torch.argmax's choice per column: the first NaN, else the first maximum"""
    total = np.asarray(total)
    out = np.argmax(np.where(np.isnan(total), -np.inf, total), axis=0)
    for b in range(total.shape[1]):
        nz = np.flatnonzero(np.isnan(total[:, b]))
        if nz.size:
            out[b] = nz[0]
    return out.astype(np.int64)


def select_cases():
    """name -> (n, B) float32 score tables"""
    inf = np.inf
    rng = np.random.RandomState(4101)
    return {
        "all_equal": np.full((5, 3), 2.5, F32),
        "all_neg_inf": np.full((4, 2), -inf, F32),
        "inf_then_nan": np.array([[0, inf, NAN], [inf, NAN, inf], [NAN, 1, 2], [inf, inf, -inf]], F32),
        "n1": np.array([[3.0, NAN, -inf]], F32),
        "random": rng.randn(7, 5).astype(F32),
        "last_wins": np.array([[0, 1], [1, 1], [2, 1]], F32),
        "neg_zero": np.array([[-0.0, 0.0], [0.0, -0.0]], F32),
    }


# ==================================================================================== 3. step kernels
TABLE_ORDER = ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2",
               "_model_variance", "_model_log_variance", "alphas_cumprod", "alphas_cumprod_prev")
SCHEDULES = ("", "250", "ddim50")
_TABS = {}


def tables(respacing):
    """the eight float32 schedule tables of _Tables (linear-1000, re-spaced), plus min_log / max_log of the learned range, float32"""
    if respacing not in _TABS:
        from guided_diffusion.script_util import create_diffusion
        d = create_diffusion(learn_sigma=False, diffusion_steps=1000, noise_schedule="linear", timestep_respacing=respacing, use_kl=False,
                             predict_xstart=False, rescale_timesteps=False, rescale_learned_sigmas=False)
        tb = [np.ascontiguousarray(getattr(d, n), dtype=np.float64).astype(F32) for n in TABLE_ORDER]
        _TABS[respacing] = dict(tabs=tb, min_log=d.posterior_log_variance_clipped.astype(F32), max_log=np.log(d.betas).astype(F32),
                                T=int(d.num_timesteps), diffusion=d)
    return _TABS[respacing]


N_STEP, E_STEP = 4, 321


def step_inputs(respacing, s, seed=0):
    """N = 4 samples at t = (0, 1, T' - 1, middle), E = 321; x ~ N(0, 1) s; eps = (c1 x - x0*) / c2 in float64 with x0* uniform in
    [-1.5, 1.5], rounded to float32: c1 x - c2 eps cancels (157 x - 157 eps at t = T' - 1) and a third of the x0 saturate under clip"""
    tb = tables(respacing)
    T = tb["T"]
    rng = np.random.RandomState(9000 + 17 * seed + len(respacing) + int(s))
    t = np.array([0, 1, T - 1, T // 2], dtype=np.int64)
    x = (rng.randn(N_STEP, E_STEP) * s).astype(F32)
    x0s = rng.uniform(-1.5, 1.5, size=(N_STEP, E_STEP))
    c1, c2 = tb["tabs"][0].astype(np.float64)[t][:, None], tb["tabs"][1].astype(np.float64)[t][:, None]
    eps = ((c1 * x.astype(np.float64) - x0s) / c2).astype(F32)
    return dict(t=t, x=x, eps=eps, grad=rng.randn(N_STEP, E_STEP).astype(F32), noise=rng.randn(N_STEP, E_STEP).astype(F32),
                gt=rng.uniform(-1, 1, size=(N_STEP, E_STEP)).astype(F32), mid=T // 2, T=T)


def t_ends(inp):
    return (-1, 0, inp["mid"], inp["T"])


def _cols(tb, t, dtype):
    return [a[t][:, None].astype(dtype) for a in tb["tabs"]]


def clip_margin(A_x0):
    """beyond 1 + this margin the clipped x0 is exactly +-1 in any float32 evaluation: the issue's 1e-3, or the rounding of the two
    products and their difference (3 x 2^-24 A) where the operands are so large (s = 1e3) that this exceeds 1e-3"""
    return np.maximum(1e-3, 3 * U * A_x0)


def _x0(c1, c2, x, eps, clip, dt):
    """-> x0 (clipped where asked), the scale of its error |c1 x| + |c2 eps|"""
    x0 = c1 * x - c2 * eps
    A = np.abs(c1 * x).astype(np.float64) + np.abs(c2 * eps).astype(np.float64)
    return (np.clip(x0, dt(-1), dt(1)) if clip else x0), A


def ddpm_step(tb, inp, dtype, clip=0, t_end=-1, grad=False, noise=False, vv=None, mode="fixed"):
    """rgm_ddpm_step / _learned / _learned_g in `dtype`, in the kernel's operation order -> dict name -> value, and (float64 only)
    name + '.A' -> the sum of the absolute values of the terms entering it.  mode: fixed | range (vv in frac units) | learned (vv = log var).
    A divisor or a derivative (exp) is applied to the terms it acts on; a saturated clip enters as the constant 1."""
    dt = dtype
    t = inp["t"]
    c1, c2, pc1, pc2, var, logvar, _, _ = _cols(tb, t, dt)
    x, eps = inp["x"].astype(dt), inp["eps"].astype(dt)
    x0, A_x0 = _x0(c1, c2, x, eps, clip, dt)
    x0_64 = c1.astype(np.float64) * x.astype(np.float64) - c2.astype(np.float64) * eps.astype(np.float64)
    sat = (np.abs(x0_64) > 1 + clip_margin(A_x0)) if clip else np.zeros(x0.shape, bool)
    A_x0c = np.where(sat, 1.0, A_x0)
    mean = pc1 * x0 + pc2 * x
    A_mean = np.abs(pc1) * A_x0c + np.abs(pc2 * x)
    A_lv = np.zeros(x.shape)
    var = np.broadcast_to(var, x.shape)
    logvar = np.broadcast_to(logvar, x.shape)
    if mode == "range":
        v = vv.astype(dt)
        mn, mx = tb["min_log"][t][:, None].astype(dt), tb["max_log"][t][:, None].astype(dt)
        frac = (v + dt(1)) / dt(2)
        logvar = frac * mx + (dt(1) - frac) * mn
        A_lv = (np.abs(frac * mx) + np.abs((dt(1) - frac) * mn)).astype(np.float64)
        var = np.exp(logvar)
    elif mode == "learned":
        logvar = vv.astype(dt)
        var = np.exp(logvar)
    if grad:
        mean = mean + var * inp["grad"].astype(dt)
        A_mean = A_mean + np.abs(var * inp["grad"].astype(dt)) * (1 + A_lv)
    g = np.exp(dt(0.5) * logvar)
    A_g = np.abs(g).astype(np.float64) * (1 + 0.5 * A_lv)
    sample, A_s = mean, A_mean
    if noise:
        gate = (t > t_end).astype(dt)[:, None]
        sample = mean + gate * g * inp["noise"].astype(dt)
        A_s = A_mean + gate * A_g * np.abs(inp["noise"])
    out = dict(sample=sample, pred_xstart=x0, g=np.broadcast_to(g, x.shape), mean=mean, sat=sat, x0_64=x0_64)
    out.update({"sample.A": A_s, "pred_xstart.A": A_x0c, "g.A": np.broadcast_to(A_g, x.shape)})
    return out


def ddim_step(tb, inp, dtype, clip=0, t_end=-1, grad=False, noise=False, eta=1.0):
    """rgm_ddim_step in `dtype`, the kernel's operation order; A as in ddpm_step, the coefficient sqrt(1 - abp - sigma^2) carrying the
    relative error of its cancelling radicand and sigma that of 1 - ab / abp"""
    dt = dtype
    t = inp["t"]
    c1, c2, _, _, _, _, ab, abp = _cols(tb, t, dt)
    x, eps = inp["x"].astype(dt), inp["eps"].astype(dt)
    cx = c1 * x
    x0, A_x0 = _x0(c1, c2, x, eps, clip, dt)
    x0_64 = c1.astype(np.float64) * x.astype(np.float64) - c2.astype(np.float64) * eps.astype(np.float64)
    sat = (np.abs(x0_64) > 1 + clip_margin(A_x0)) if clip else np.zeros(x0.shape, bool)
    A0 = np.where(sat, 1.0, A_x0)
    acx = np.abs(cx).astype(np.float64)
    if grad:
        e = (cx - x0) / c2
        sq = np.sqrt(dt(1) - ab)
        e = e - sq * inp["grad"].astype(dt)
        A_e = (acx + A0) / c2 + np.abs(sq * inp["grad"].astype(dt))
        x0 = cx - c2 * e
        A0 = acx + c2 * A_e
    e2 = (cx - x0) / c2
    A_e2 = (acx + A0) / c2
    r = ab / abp
    sigma = dt(eta) * np.sqrt((dt(1) - abp) / (dt(1) - ab)) * np.sqrt(dt(1) - r)
    # 1 - ab / abp cancels (ab / abp = 0.9998 at t = 1): the quotient's rounding enters sigma amplified by (1 + r) / (2 (1 - r))
    with np.errstate(divide="ignore", invalid="ignore"):
        rel_s = np.where(r < 1, 2 + 0.5 * (1 + r) / (1 - r), 0.0).astype(np.float64)
    rad = dt(1) - abp - sigma * sigma
    coef = np.sqrt(rad)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(rad > 0, ((dt(1) - abp) + 2 * rel_s * sigma * sigma) / (2 * rad), 0.0).astype(np.float64)
    mean = x0 * np.sqrt(abp) + coef * e2
    A_mean = np.sqrt(abp) * A0 + coef * (1 + rel) * A_e2
    sample, A_s = mean, A_mean
    if noise:
        gate = (t != t_end).astype(dt)[:, None]
        sample = mean + gate * sigma * inp["noise"].astype(dt)
        A_s = A_mean + gate * rel_s * np.abs(sigma * inp["noise"].astype(dt))
    sg = np.broadcast_to(sigma, x.shape)
    if grad:
        sat = np.zeros(x0.shape, bool)                                  # condition_score recomputes x0 behind the clip: no longer +-1
    return {"sample": sample, "pred_xstart": x0, "g": sg, "mean": mean, "sat": sat, "x0_64": x0_64,
            "sample.A": A_s, "pred_xstart.A": A0, "g.A": np.broadcast_to(rel_s * np.abs(sigma), x.shape)}


def xstart_from_eps(tb, inp, dtype, out_scale):
    dt = dtype
    c1, c2 = _cols(tb, inp["t"], dt)[:2]
    x, eps = inp["x"].astype(dt), inp["eps"].astype(dt)
    out = (c1 * x - c2 * eps) * dt(F32(out_scale))
    A = (np.abs(c1 * x) + np.abs(c2 * eps)).astype(np.float64) * abs(float(F32(out_scale)))
    return {"out": out, "out.A": A}


def edit_replace_eps(tb, inp, dtype, clip, mask):
    """x0 = clip(c1 x - c2 eps); x0r = m gt + (1 - m) x0; out = (c1 x - x0r) / c2: at t = 0, c2 = 0.01 amplifies the numerator's error"""
    dt = dtype
    c1, c2 = _cols(tb, inp["t"], dt)[:2]
    x, eps, gt, m = inp["x"].astype(dt), inp["eps"].astype(dt), inp["gt"].astype(dt), mask.astype(dt)
    x0, A_x0 = _x0(c1, c2, x, eps, clip, dt)
    x0_64 = c1.astype(np.float64) * x.astype(np.float64) - c2.astype(np.float64) * eps.astype(np.float64)
    sat = (np.abs(x0_64) > 1 + clip_margin(A_x0)) if clip else np.zeros(x0.shape, bool)
    A0 = np.where(sat, 1.0, A_x0)
    x0r = m * gt + (dt(1) - m) * x0
    out = (c1 * x - x0r) / c2
    A = (np.abs(c1 * x) + np.abs(m * gt) + np.abs(dt(1) - m) * A0).astype(np.float64) / c2.astype(np.float64)
    return {"out": out, "out.A": A}


def ratio(got, ref, A):
    """worst |got - ref64| / (2^-24 A) per element; an element with A = 0 has to be exact"""
    got, ref, A = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(A, np.float64)
    d = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(A > 0, d / (U * A), np.where(d == 0, 0.0, np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())


RANGE_VV = (-1.5, -1.0, 0.0, 1.0, 1.5)
LEARNED_VV = (-30.0, -5.0, 0.0, 5.0)
MASKS = (0.0, 1.0, 0.5)
OUT_SCALE = 1.0 / 1.2465


def vv_array(values, seed=0):
    """(N, E) float32 cycling through `values`, shifted per sample so that every t meets every value"""
    idx = (np.arange(E_STEP)[None, :] + np.arange(N_STEP)[:, None] + seed) % len(values)
    return np.asarray(values, F32)[idx]


def mask_array(kind):
    """0, 1, 0.5 constant, or 'mixed': the three cycling"""
    return vv_array(MASKS) if kind == "mixed" else np.full((N_STEP, E_STEP), kind, F32)


def ddpm_cases():
    """every (kernel, kwargs) of the DDPM family the tests walk"""
    out = []
    for clip in (0, 1):
        for grad in (False, True):
            out.append(("ddpm", dict(clip=clip, grad=grad, noise=False, t_end=-1)))
            for te in (-1, 0, "mid", "T"):
                out.append(("ddpm", dict(clip=clip, grad=grad, noise=True, t_end=te)))
    for mode, vals in (("range", RANGE_VV), ("learned", LEARNED_VV)):
        for clip in (0, 1):
            for grad, noise, te in ((False, False, -1), (True, False, -1), (True, True, -1), (True, True, "mid"), (False, True, 0),
                                    (False, True, "mid"), (False, True, "T")):
                out.append(("learned", dict(clip=clip, grad=grad, noise=noise, t_end=te, mode=mode, vv=vals)))
    return out


def ddim_cases():
    out = []
    for clip in (0, 1):
        for grad in (False, True):
            for te in (-1, 0, "mid", "T"):
                out.append(dict(clip=clip, grad=grad, noise=True, t_end=te))
    return out


def resolve_t_end(te, inp):
    return {"mid": inp["mid"], "T": inp["T"]}.get(te, te)


# ==================================================================================== 4. rules
MARKER = F32(0.3125)                             # channels 1, 2: must come back untouched
MIN_PIANO, MAX_PIANO = 21, 108
TH = F32(-0.95)
THRESHOLD_VALUES = np.array([TH, np.nextafter(TH, F32(-2)), np.nextafter(TH, F32(0)), -1.0, np.nextafter(F32(-1), F32(-2)), -0.0, 1.2], F32)
ND_RULES = {"note_density": dict(interval=128, horizontal_scale=5), "note_density_hr_1": dict(interval=128, horizontal_scale=1.0),
            "note_density_hr_2": dict(interval=128, horizontal_scale=2.0), "note_density_pixel": dict(interval=16, horizontal_scale=5)}
RULE_SHAPES = {"threshold": [(1, 1, 128), (3, 3, 384)], "edges": [(1, 1, 128), (3, 3, 384)], "silent": [(1, 3, 128), (3, 1, 384)],
               "full": [(3, 1, 128), (1, 3, 384)], "nonfinite": [(1, 1, 128), (3, 3, 384)]}
FINITE = ("threshold", "edges", "silent", "full")
CHORD_SHAPES = {"threshold": [(3, 3, 384)], "edges": [(3, 3, 384)], "silent": [(1, 3, 128)], "full": [(3, 1, 128)], "levels": [(1, 1, 128), (3, 3, 128)]}
RULE_SEED = 7300
LEVEL_KS = (0, 1, 63, 64, 126, 127)


def rule_cases(shapes=RULE_SHAPES):
    return [(f, s) for f in shapes for s in shapes[f]]


def case_key(fam, shape):
    return f"{fam}.n{shape[0]}c{shape[1]}t{shape[2]}"


def roll(fam, shape):
    """(N, C, 128, T) float32: channel 0 the family's roll, channels 1.. the marker"""
    N, C, T = shape
    rng = np.random.RandomState(RULE_SEED + sum(map(ord, fam)) + 131 * N + 17 * C + T)
    r = np.full((N, C, 128, T), MARKER, F32)
    a = np.full((N, 128, T), -1.0, F32)
    if fam == "threshold":
        pick = rng.rand(N, 128, T) < 0.08
        a[pick] = THRESHOLD_VALUES[rng.randint(0, len(THRESHOLD_VALUES), size=int(pick.sum()))]
    elif fam == "levels":
        lv = np.array([2.0 * k / 127.0 - 1.0 for k in LEVEL_KS]).astype(F32)
        vals = np.concatenate([lv, np.nextafter(lv, F32(-2)), np.nextafter(lv, F32(2))]).astype(F32)
        pick = rng.rand(N, 128, T) < 0.2
        a[pick] = vals[rng.randint(0, len(vals), size=int(pick.sum()))]
        for j, v in enumerate(vals):                                   # every value at least once on a piano row
            a[:, 40 + j, 3] = v
    elif fam == "edges":
        a[:, 60, 0:10] = 0.8                                            # starts at t = 0
        a[:, 62, T - 10:T] = 0.5                                        # ends at T - 1
        for p in (20, 21, 108, 109):                                    # the piano range's borders, inside and outside
            a[:, p, 30:40] = 0.9
        a[:, 0, :] = 0.7                                                # a whole row outside the range
        if T > 256:
            for n in range(N):
                if n != 1:
                    a[n, 64, 250:261] = 0.6                             # active at 255 and 256: no onset at 256
                if n != 0:
                    a[n, 66, 256:261] = 0.6                             # onset exactly at t = 256, the first column of the second block
    elif fam == "full":
        a[:] = 1.0
    elif fam == "nonfinite":
        pick = rng.rand(N, 128, T) < 0.03
        a[pick] = rng.uniform(-1, 1, size=int(pick.sum())).astype(F32)
        w = T // 3 if T >= 384 else 16                                  # three different windows (interval 128 at T = 384, 16 at T = 128)
        for n in range(N):
            if n == 2:
                a[n, 70, w + 7] = np.inf                                # this sample: +inf alone
                continue
            tn = (T - 1 if N == 1 else 5) if n == 0 else 255                # the last column; a window's inside; the last column of block 0
            a[n, 50, tn] = np.nan
            a[n, 70, (tn // w + 1) % (T // w) * w + 7] = np.inf
            a[n, 80, (tn // w + 2) % (T // w) * w + 9] = -np.inf
    else:
        assert fam == "silent", fam
    r[:, 0] = a
    return r


def binarise(ch0):
    """channel 0 -> the reference's binary roll after mask and snap (NaN stays NaN), float64"""
    a = ch0.astype(np.float64).copy()
    a[:, :MIN_PIANO] = -1
    a[:, MAX_PIANO + 1:] = -1
    a[a < float(TH)] = -1
    b = (a + 1) / 2
    return np.where(b >= 1e-2, 1.0, np.where(b < 1e-2, 0.0, b))


def pitch_hist64(rl):
    """-> hist (N, 12), class sums h (N, 12), d (N, 1) in float64 from the float32 roll (mask applied)"""
    a = rl[:, 0].astype(np.float64).copy()
    a[:, :MIN_PIANO] = -1
    a[:, MAX_PIANO + 1:] = -1
    with np.errstate(invalid="ignore"):
        rows = ((a + 1) / 2).sum(-1)
        rows[:, :MIN_PIANO] = 0
        rows[:, MAX_PIANO + 1:] = 0
        h = np.concatenate((rows, np.zeros((rows.shape[0], 4))), -1).reshape(-1, 11, 12).sum(1)
        d = h.sum(-1, keepdims=True) + float(F32(1e-12))
        return h / d, h, d


def _rowsum32(rl):
    """pitch_rowsum_kernel restated: 256 threads stride the row, a xor-butterfly per wave, (s0 + s1) + (s2 + s3)"""
    a = rl[:, 0].astype(F32)
    N, _, T = a.shape
    part = np.zeros((N, 128, 256), F32)
    with np.errstate(invalid="ignore"):
        for t0 in range(0, T, 256):
            seg = (a[:, :, t0:t0 + 256] + F32(1)) / F32(2)
            part[:, :, :seg.shape[-1]] += seg
        w = part.reshape(N, 128, 4, 64)
        o = 32
        while o:
            w = w + w[..., np.arange(64) ^ o]
            o >>= 1
        s = (w[:, :, 0, 0] + w[:, :, 1, 0]) + (w[:, :, 2, 0] + w[:, :, 3, 0])
    s[:, :MIN_PIANO] = 0
    s[:, MAX_PIANO + 1:] = 0
    return s


def _fold32(rows):
    N = rows.shape[0]
    h = np.zeros((N, 12), F32)
    tot = np.zeros(N, F32)
    with np.errstate(invalid="ignore"):
        for c in range(12):
            s = np.zeros(N, F32)
            for o in range(11):
                if o * 12 + c < 128:
                    s = s + rows[:, o * 12 + c]
            h[:, c] = s
            tot = tot + s
    return h, (tot + F32(1e-12))[:, None]


def pitch_hist32(rl):
    h, d = _fold32(_rowsum32(rl))
    with np.errstate(invalid="ignore"):
        return h / d


def vag64(rl, target, scale):
    """the closed form above pitch_fold_vag_kernel in float64 -> logp (N,), hist (N, 12), dh (N, 12), the scale max|u_c| / d (N, 1)"""
    hist, _, d = pitch_hist64(rl)
    e = hist - target.astype(np.float64)
    u = -2.0 * float(F32(scale)) * e
    dh = (u - (u * hist).sum(-1, keepdims=True)) / d
    return -float(F32(scale)) * (e * e).sum(-1), hist, dh, np.abs(u).max(-1, keepdims=True) / d


def vag32(rl, target, scale):
    h, d = _fold32(_rowsum32(rl))
    sc = F32(scale)
    N = h.shape[0]
    lp, dot = np.zeros(N, F32), np.zeros(N, F32)
    u = np.zeros((N, 12), F32)
    hist = np.zeros((N, 12), F32)
    for c in range(12):
        hc = h[:, c] / d[:, 0]
        e = hc - target[:, c]
        lp = lp + e * e
        u[:, c] = F32(-2) * sc * e
        dot = dot + u[:, c] * hc
        hist[:, c] = hc
    return -sc * lp, hist, (u - dot[:, None]) / d


def vag_target(N, seed=0):
    t = np.random.RandomState(7700 + seed).rand(N, 12)
    return (t / t.sum(-1, keepdims=True)).astype(F32)


def bucketize_values(bounds):
    b = np.asarray(bounds, F32)
    v = np.concatenate([b, np.nextafter(b, F32(-np.inf)), np.nextafter(b, F32(np.inf)),
                        np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, b.min() - 1, b.max() + 1, -1e30, 1e30], F32)])
    return v.astype(F32)


def row_loss_case(K, seed=0):
    """(rows, K) a, b float32: equal cells, near-equal cells, one row with a NaN, one with an inf"""
    rng = np.random.RandomState(7800 + K + seed)
    rows = 37
    a = rng.randn(rows, K).astype(F32)
    b = np.where(rng.rand(rows, K) < 0.4, a, a + rng.randn(rows, K).astype(F32)).astype(F32)
    b[3] = a[3]                                                        # a row with no difference
    a[5, K // 2] = np.nan
    a[9, 0] = np.inf
    a[11, K - 1], b[11, K - 1] = 0.0, -0.0                              # equal for !=
    return a, b


def row_loss64(a, b, zero_one):
    a, b = a.astype(np.float64), b.astype(np.float64)
    K = a.shape[1]
    with np.errstate(invalid="ignore"):
        if zero_one:
            return (a != b).sum(-1) / K, None
        s = ((a - b) ** 2).sum(-1)
        return s / K, s / K


# ==================================================================================== 5. collage
BASE = 128
COLLAGE_B, COLLAGE_C, COLLAGE_H, COLLAGE_N, COLLAGE_OV = (1, 3), 4, (1, 16), (2, 3, 7), (0, 32, 64, 96)


def collage_valid(n, ov, circle):
    """a circular collage of width n (128 - ov) is extended by its first ov columns: it has to be that wide.  The reference's own
    split asserts (and rgm_collage_split refuses) the others: (n, ov) = (2, 96)."""
    return not circle or n * (BASE - ov) >= ov


def collage_configs():
    """(B, h, n, ov): every n x ov, with B and h alternating so that each value meets each n and ov"""
    out = []
    for i, n in enumerate(COLLAGE_N):
        for j, ov in enumerate(COLLAGE_OV):
            out.append((COLLAGE_B[(i + j) % 2], COLLAGE_H[(i + j + 1) % 2], n, ov))
            out.append((COLLAGE_B[(i + j + 1) % 2], COLLAGE_H[(i + j) % 2], n, ov))
    return out


def collage_arrays(B, h, n, ov, seed=0):
    rng = np.random.RandomState(8100 + 1000 * B + 100 * h + 10 * n + ov + seed)
    full = rng.randn(B * n, COLLAGE_C, h, BASE).astype(F32)
    half = rng.randn(B * n, COLLAGE_C, h, ov).astype(F32)
    return full, half


def split_ref(img, n, ov, circle):
    """F.unfold on the CPU (w_img.split_wimg), the circular image extended by its first ov columns -> windows ((b n), C, h, 128), halves"""
    t = torch.from_numpy(img)
    if circle:
        t = torch.cat((t, t[..., :ov]), dim=-1)
    B, C, h, W = t.shape
    assert n * BASE - ov * (n - 1) == W
    u = torch.nn.functional.unfold(t, kernel_size=(h, BASE), stride=BASE - ov)                # (B, C h 128, n)
    wins = u.reshape(B, C, h, BASE, n).permute(0, 4, 1, 2, 3).reshape(B * n, C, h, BASE).contiguous().numpy()
    return wins, np.ascontiguousarray(wins[..., BASE - ov:])


def _fold(x, n, ov):
    bn, C, h, w = x.shape
    u = x.reshape(bn // n, n, C * h * w).permute(0, 2, 1)
    return torch.nn.functional.fold(u, (h, n * w - (n - 1) * ov), kernel_size=(h, w), stride=w - ov)


def merge_ref(full, half, n, ov, circle, is_avg, dtype):
    """condind_long.py:36-50 / condind_circle.py:57-82 on arrays, in torch `dtype` on the CPU: the last window's half zeroed, full's right
    overlap minus half, fold-sum [/ coverage], the circular seam averaged -> value, sum |terms| (divisors applied), terms per element"""
    f = torch.from_numpy(full).to(dtype).clone()
    a = f.abs()
    bn = f.shape[0]
    if half is not None and ov > 0:
        hf = torch.from_numpy(half).to(dtype).clone().reshape(bn // n, n, *half.shape[1:])
        hf[:, -1] = 0
        hf = hf.reshape(bn, *half.shape[1:])
        f[..., BASE - ov:] -= hf
        a[..., BASE - ov:] += hf.abs()
    out, A, cnt = _fold(f, n, ov), _fold(a, n, ov), _fold(torch.ones_like(f), n, ov)
    terms = cnt.clone()
    if is_avg:
        out, A = out / cnt, A / cnt
    if circle and ov > 0:
        out = torch.cat(((out[..., :ov] + out[..., -ov:]) / 2.0, out[..., ov:-ov]), dim=-1)
        A = torch.cat(((A[..., :ov] + A[..., -ov:]) / 2.0, A[..., ov:-ov]), dim=-1)
        terms = torch.cat((terms[..., :ov] + terms[..., -ov:], terms[..., ov:-ov]), dim=-1)
    return out.numpy(), A.double().numpy(), terms.double().numpy()


def merge_divides(n, ov, circle, is_avg):
    """does any element pass through a division (coverage or seam)?"""
    return bool(is_avg) or bool(circle and ov > 0)


def index_windows(B, h, n):
    """window (b, i) filled with b n + i + 1: small integers, every sum and average of them exact"""
    v = np.arange(1, B * n + 1, dtype=F32).reshape(B * n, 1, 1, 1)
    return np.ascontiguousarray(np.broadcast_to(v, (B * n, COLLAGE_C, h, BASE))).astype(F32)


COLLAGE_SEED = 8200


def golden_image(n, ov):
    """the (3, 4, 1, W) image whose reference split tests/golden/step_inputs.npz holds"""
    W = n * BASE - (n - 1) * ov
    return np.random.RandomState(COLLAGE_SEED + 10 * n + ov).randn(3, COLLAGE_C, 1, W).astype(F32)


def golden_windows(n, ov):
    """the (3 n, 4, 1, 128) windows whose reference merges the fixture holds"""
    return np.random.RandomState(COLLAGE_SEED + 500 + 10 * n + ov).randn(3 * n, COLLAGE_C, 1, BASE).astype(F32)
