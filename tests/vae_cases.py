"""Inputs, CPU references, the error measure and the bound of the VAE-kernel tests on offset, peaked, dead-group and edge inputs
(test_vae_cases_host.py, test_gpu_vae_inputs.py; fixtures from tests/golden/make_golden_vae_inputs.py).  A plain helper module: no
fixtures of pytest, nothing here touches a GPU.

Weight families are deterministic edits of rgm.synth.vae_state_dict(SEED, encoder=True); the same edit applies to encoder and decoder
keys; nothing is stored but the seeds.  Latent families and the encoder's roll families run on `base` weights (the roll families also
under `offset` and `gain`).

Layout: latent (N, 4, H, 16) as decode_latent takes it (scale factor 1), one 16 x 16 square per 16 latent rows; roll (N, 3, 128, 8 H);
encoder tiles (M, 3, 128, 128) -> moments (M, 8, 16, 16).

References: oracle/vae_torch.py in float64 (ref64), in float32, and its twin of the bf16x3 modes with attn_cases.split_parts as the split."""
import numpy as np
import torch

import attn_cases

F32 = np.float32
SEED, GAIN_SEED, Z_SEED, COT_SEED = 2, 17, 5, 9
WEIGHT_FAMILIES = ("base", "offset", "gain", "peaked3", "dead")
LATENT_FAMILIES = ("zlat0", "zlat4", "impulse")
DECODE_FAMILIES = WEIGHT_FAMILIES + LATENT_FAMILIES
TWO_SQUARE_FAMILIES = ("offset", "impulse")                 # decode_latent at N = 1, H = 32 (`base` there calibrates R_p)
ROLL_FAMILIES = ("silence", "corners", "sparse")
ENCODE_WEIGHTS = ("base", "offset", "gain")
DEAD_GROUP = 3
CONDITIONING_LIMIT = 1e-4                                   # worst block of the float32 reference against float64, any family
_OFFSET_KEYS = ("conv_in", "conv1", "conv2", "nin_shortcut", "proj_out", "upsample", "downsample")


# ------------------------------------------------------------------------------------------------ weights
def base_weights():
    from rgm import synth
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in synth.vae_state_dict(SEED, encoder=True).items()}


def weights(name, base=None):
    """state dict (numpy float32) of a weight family; latent and roll families run on `base`"""
    sd = {k: np.array(v, copy=True) for k, v in (base or base_weights()).items()}
    if name in ("base",) + LATENT_FAMILIES:
        return sd
    assert name in WEIGHT_FAMILIES, name
    rng = np.random.RandomState(GAIN_SEED)
    for k in list(sd):
        norm = "norm" in k
        if name == "offset" and k.endswith(".bias") and not norm and any(s in k for s in _OFFSET_KEYS):
            C = sd[k].shape[0]
            g = np.arange(C) // max(1, C // 32)                  # the GroupNorm group of the output channel
            sd[k] = (sd[k] + np.where(g % 2 == 0, 1.0, -1.0) * (20.0 + 40.0 * g / 32)).astype(F32)
        elif name == "gain" and norm and k.endswith(".weight"):
            sd[k] = (sd[k] * np.exp(rng.uniform(-2.0, 2.0, size=sd[k].shape))).astype(F32)
        elif name == "gain" and norm and k.endswith(".bias"):
            sd[k] = (sd[k] + 2.0 * rng.randn(*sd[k].shape)).astype(F32)
        elif name == "peaked3" and ("attn_1.q." in k or "attn_1.k." in k):
            sd[k] = (sd[k] * F32(3.0)).astype(F32)
        elif name == "dead" and k.endswith("conv1.weight"):
            gw = sd[k].shape[0] // 32
            sd[k][DEAD_GROUP * gw:(DEAD_GROUP + 1) * gw] = 0
            sd[k[:-len("weight")] + "bias"][DEAD_GROUP * gw:(DEAD_GROUP + 1) * gw] = 0.75
    return sd


# ------------------------------------------------------------------------------------------------ inputs
def latent(name, H=16):
    """(1, 4, H, 16) float32.  H = 16: one square; H = 32: two squares, the second a draw of its own."""
    z = np.random.RandomState(Z_SEED + (H - 16)).randn(1, 4, H, 16).astype(F32)
    if name == "zlat0":
        z[:] = 0
    elif name == "zlat4":
        z *= F32(4.0)
    elif name == "impulse":
        z[:] = 0
        z[0, :, 0, 0] = 3.0                                      # a corner pixel of square 0
        if H > 16:
            z[0, :, 16, 7] = -3.0                                # square 1, first column after the seam
    return z


def cotangent(H=16):
    return np.random.RandomState(COT_SEED + (H - 16)).randn(1, 3, 128, 8 * H).astype(F32)


def rolls():
    """(3, 3, 128, 128) float32 encoder tiles: ROLL_FAMILIES in order"""
    from test_gpu_sampler import _sparse_roll
    sil = -np.ones((3, 128, 128), F32)
    cor = sil.copy()
    for p in (0, 127):
        for s, e in ((0, 20), (100, 128)):                       # a note starting at time 0 and one ending at time 127, lowest and highest pitch
            cor[0, p, s:e] = 0.8
            cor[1, p, s] = 1.0
    return np.stack((sil, cor, _sparse_roll(np.random.RandomState(400), 1, 128)[0])).astype(F32)


def tiles_of(lat):
    """latent (N, 4, H, 16) -> the squares (N * H / 16, 4, 16, 16) AutoencoderKL.decode consumes (square-major)"""
    lat = np.asarray(lat)
    k = lat.shape[2] // 16
    return np.ascontiguousarray(np.concatenate(np.split(lat.transpose(0, 1, 3, 2), k, axis=-1), axis=0))


# ------------------------------------------------------------------------------------------------ references
def model(sd, kind, hooks=None, probe=None):
    """kind: 'ref64' | 'fp32' | 'bf16x3' (the twin; both bf16x3 modes share it)"""
    from oracle import vae_torch
    if kind == "ref64":
        return vae_torch.VAE(sd, torch.float64, hooks=hooks, probe=probe)
    if kind == "fp32":
        return vae_torch.VAE(sd, torch.float32, hooks=hooks, probe=probe)
    assert kind == "bf16x3", kind
    return vae_torch.VAE(sd, torch.float64, split=attn_cases.split_parts, hooks=hooks, probe=probe)


def arith(precision):
    return "fp32" if precision == "fp32" else "bf16x3"


def run_decode(m, lat, cot=None):
    """-> {'roll': (N, 3, 128, 8H) float64 ndarray[, 'dlat': (N, 4, H, 16)]}"""
    lt = torch.from_numpy(np.ascontiguousarray(lat))
    if cot is None:
        with torch.no_grad():
            return {"roll": m.decode_latent(lt).double().numpy()}
    roll, g = m.decode_latent_vjp(lt, torch.from_numpy(np.ascontiguousarray(cot)))
    return {"roll": roll.double().numpy(), "dlat": g.double().numpy()}


def run_encode(m, x):
    with torch.no_grad():
        return m.encode_moments(torch.from_numpy(np.ascontiguousarray(x))).double().numpy()


# ------------------------------------------------------------------------------------------------ the measure
def block_err(a, b, quantity):
    """max |a - b| over a block / max |b| over the same block.  Blocks: roll (N, 3, 128, 8H) -> (N, square, channel); moments
    (M, 8, 16, 16) -> (tile, channel); d(latent) (N, 4, H, 16) -> (sample, channel, square).  NaN or inf in a block of `a` gives inf;
    a block whose reference is all zero passes only when `a` is all zero there."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    if quantity == "roll":
        N, C, P, T = b.shape
        a, b = (x.reshape(N, C, P, T // 128, 128).transpose(0, 3, 1, 2, 4).reshape(N, T // 128, C, -1) for x in (a, b))
    elif quantity == "moments":
        a, b = (x.reshape(x.shape[0], x.shape[1], -1) for x in (a, b))
    elif quantity == "dlat":
        N, C, H, W = b.shape
        a, b = (x.reshape(N, C, H // 16, 16 * W) for x in (a, b))
    else:
        raise KeyError(quantity)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(a - b).max(axis=-1)
        d = np.where(np.isfinite(d), d, np.inf)
        s = np.abs(b).max(axis=-1)
        return np.where(s > 0, d / s, np.where(d == 0, 0.0, np.inf))


def rel(a, b):
    """the suite's norm-wise measure (gpu_util.rel), for the comparisons with it"""
    return attn_cases.rel(a, b)


def tolerances():
    """TOL_p per quantity: the constants of the existing VAE tests, imported (never copied)"""
    import test_gpu_dpsrule
    import test_gpu_edit
    import test_gpu_sampler
    return {"roll": test_gpu_sampler.VAE_DECODE_TOL, "moments": test_gpu_edit.VAE_ENCODE_TOL, "dlat": test_gpu_dpsrule.VAE_VJP_TOL}


# ------------------------------------------------------------------------------------------------ fixtures and the bound
_CACHE = {}


def fixtures():
    if "fx" not in _CACHE:
        from conftest import load_golden
        _CACHE["fx"] = load_golden("vae_inputs")
    return _CACHE["fx"]


def case_key(family, quantity, H=16):
    """fixture prefix of a case: '<family>' (one square), '<family>.h32' (two squares), 'enc.<weights>' (moments of the three rolls)"""
    if quantity == "moments":
        return "enc." + family
    return family if H == 16 else f"{family}.h{H}"


def reference(family, quantity, H=16):
    """the stored float64 result of the reference"""
    return fixtures()[f"{case_key(family, quantity, H)}.{ {'roll': 'roll64', 'dlat': 'dlat64', 'moments': 'mom64'}[quantity]}"]


def comparator_errors(precision, family, quantity, H=16):
    """stored block errors, against float64, of the comparator of `precision`: the float32 reference for fp32, the twin for both bf16x3 modes"""
    return fixtures()[f"{case_key(family, quantity, H)}.err_{arith(precision)}.{quantity}"]


def headroom(precision, quantity, H=16):
    """R_p = max(1, TOL_p / worst block of the comparator on `base` at the same shape) -> (R_p, that worst block)"""
    worst = float(comparator_errors(precision, "base", quantity, H).max())
    return max(1.0, tolerances()[quantity][precision] / worst), worst


def bound(precision, family, quantity, H=16):
    """max(TOL_p, 2 R_p x worst block of the comparator on this family): one number for every block of the case"""
    R, _ = headroom(precision, quantity, H)
    return max(tolerances()[quantity][precision], 2.0 * R * float(comparator_errors(precision, family, quantity, H).max()))


def within(err, bnd):
    """every block within the bound; NaN fails"""
    return bool(np.all(np.asarray(err) <= bnd))


# ------------------------------------------------------------------------------------------------ family properties (float64 oracle)
def properties(probe, roll=None):
    """numbers the family table is asserted on, from a probe dict filled by one float64 decode"""
    out = {}
    ratios, dead = [], []
    for key, g in probe.get("gn_in", []):
        mu, sd_ = g.mean(-1), g.std(-1)
        ratios.append(float(torch.where(sd_ > 0, mu.abs() / sd_, torch.zeros_like(sd_)).max()))      # a constant group has no ratio
        if key.endswith("norm2"):
            dead.append(float(g[:, DEAD_GROUP].std(-1).max()))
    out["gn_ratio"] = max(ratios)
    out["dead_std"] = max(dead)
    (_, s), (_, p) = probe["scores"][0], probe["probs"][0]
    out["max_score"] = float(s.abs().max())
    out["mean_row_max"] = float(p.amax(-1).mean())
    if roll is not None:
        out["roll_range"] = float(np.abs(roll).max())
    return out


# ------------------------------------------------------------------------------------------------ mutants of the float64 oracle
def mutant_hooks(name):
    """deliberately wrong arithmetic for the sensitivity tests (hooks of oracle.vae_torch.VAE):
      'var32'      GroupNorm variance as E[x^2] - mean^2 in float32, every GroupNorm
      'tiles15'    the statistics of decoder.up.0.block.0.norm1 (128 x 128) taken over 15 of its 16 tiles of 8 rows
      'edge_pad'   the zero column left of decoder.up.1.upsample.conv's input replaced by edge replication
      'keys255_last' / 'keys255_top'   softmax normalised by the sum over 255 of 256 keys: without the last key / without the key that
                   collects the most probability over all rows (found by the hook itself)"""
    import torch.nn.functional as F
    if name == "var32":
        def stats(g, key):
            g32 = g.to(torch.float32)
            mu = g32.mean(-1, keepdim=True)
            var = (g32 * g32).mean(-1, keepdim=True) - mu * mu
            return mu.to(g.dtype), var.to(g.dtype)
        return {"gn_stats": stats}
    if name == "tiles15":
        def stats(g, key):
            if key == "decoder.up.0.block.0.norm1":
                m, G, n = g.shape
                part = g.reshape(m, G, n // (128 * 128), 128, 128)[:, :, :, :120].reshape(m, G, -1)
            else:
                part = g
            mu = part.mean(-1, keepdim=True)
            return mu, ((part - mu) ** 2).mean(-1, keepdim=True)
        return {"gn_stats": stats}
    if name == "edge_pad":
        def pad(x, p, key):
            y = F.pad(x, p)
            if key == "decoder.up.1.upsample.conv":
                y = y.clone()
                y[:, :, :, 0] = y[:, :, :, 1]
            return y
        return {"pad": pad}
    if name in ("keys255_last", "keys255_top"):
        def softmax(s):
            e = torch.exp(s - s.amax(-1, keepdim=True))
            keep = torch.ones(s.shape[-1], dtype=torch.bool)
            keep[-1 if name == "keys255_last" else int((e / e.sum(-1, keepdim=True)).sum(dim=(0, 1)).argmax())] = False
            return e / e[..., keep].sum(-1, keepdim=True)
        return {"softmax": softmax}
    raise KeyError(name)


# mutant -> the families it is run on; the first is the one it has to be caught on (test_vae_cases_host.py)
MUTANTS = {"var32": ("offset", "base"), "tiles15": ("base",), "edge_pad": ("base",), "keys255_top": ("peaked3",), "keys255_last": ("gain", "peaked3")}
