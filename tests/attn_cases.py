"""Inputs, CPU references and the error measure of the attention-kernel tests on peaked, shifted and uneven-scale inputs
(test_attn_cases_host.py, test_gpu_attn_inputs.py).  A plain helper module: no fixtures, nothing here touches a GPU.

Layout everywhere: qkv (N*T, 3*D) = (N, T, 3, heads, hd) like the output of the qkv GEMM, d_o and o (N*T, D), lse (N, heads, T),
d(qkv) like qkv.  Rotary covers the first hd/2 channels, so channel hd-1 is not rotated and carries an exact, chosen score term.

References, all one (sample, head) at a time and chunked over the query rows:
  ref64  float64 throughout (rotary included);
  ref32  the arithmetic of the reference's non-fused path (guided_diffusion/dit.py RotaryAttention: q * scale @ k^T, softmax, @ v) in
         float32 with torch on the CPU, autograd for the backward;
  twin   'fp32': ref32.  'bf16x3' / 'bf16x3_presplit': ref64 with both operands of every matrix product passed through the three-term split
         of csrc/common.h (hi = split_t(x), lo = split_t(x - hi), products hi*hi + hi*lo + lo*hi, wide accumulation), the query scale (and
         log2 e in the forward) folded into q before the split, P / dS rounded to float32 before their split, lse and D rounded to
         float32.  It restates the documented arithmetic, not the kernels."""
import math

import numpy as np
import torch

F32 = np.float32
KEY_BLOCK = 64                      # keys per streamed block of csrc/attention_stream.hip (SKB)
FAMILIES = ("randn", "peaked3", "peaked6", "headscale", "ramp_up", "ramp_down", "rowshift", "lastkey", "firstkey")
FORWARD_ONLY = ("jump",)
# max |scaled score| a family is built to reach (T = 1000, hd 72); the host test holds every shape within a factor 1.5 of it
MAX_SCORE = {"peaked3": 50.0, "peaked6": 200.0, "rowshift": 147.0, "jump": 176.0}


# ------------------------------------------------------------------------------------------------ inputs
def family(name, N, T, heads, hd, seed):
    """(qkv (N*T, 3*D), d_o (N*T, D)) float32, rebuilt from the seed.  'randn15' is 'randn' x 1.5: what the forward tests of the suite feed."""
    rng = np.random.RandomState(seed)
    D = heads * hd
    qkv = rng.randn(N * T, 3 * D).astype(F32)
    d_o = rng.randn(N * T, D).astype(F32)
    r = qkv.reshape(N, T, 3, heads, hd)
    g = d_o.reshape(N, T, heads, hd)
    q, k, v = r[:, :, 0], r[:, :, 1], r[:, :, 2]                 # views (N, T, heads, hd)
    if name == "randn":
        pass
    elif name == "randn15":
        qkv *= F32(1.5)
    elif name in ("peaked3", "peaked6"):
        f = F32(3.0 if name == "peaked3" else 6.0)
        q *= f
        k *= f
    elif name == "headscale":
        s = (10.0 ** np.linspace(-2, 1, heads)).astype(F32)[None, None, :, None]
        v *= s
        g *= s
    elif name in ("ramp_up", "ramp_down"):
        q[..., hd - 1] = 8.0
        ramp = np.linspace(0, 40, T).astype(F32)
        k[..., hd - 1] = (ramp if name == "ramp_up" else -ramp)[None, :, None]
    elif name == "rowshift":
        q[..., hd - 1] = np.where(np.arange(T) % 2 == 0, 30.0, -30.0).astype(F32)[None, :, None]
        k[..., hd - 1] = 40.0
    elif name in ("lastkey", "firstkey"):
        q[..., hd - 1] = 3.0
        k[:, T - 1 if name == "lastkey" else 0, :, hd - 1] = 25.0
    elif name == "jump":
        q[..., hd - 1] = 6.0
        k[:, T - 1, :, hd - 1] = 250.0
    elif name == "zeroq":                                        # every score exactly 0: lse = ln T, o = the column mean of v
        q[...] = 0.0
    else:
        raise KeyError(name)
    return qkv, d_o


def rotary_tables(hd, T):
    from oracle import dit_np as odit
    from rgm.synth import rotary_freqs
    return odit.rotary_tables(rotary_freqs(hd // 2), T)          # (T, hd/4) each, float32


def _rot(x, cos, sin, inverse=False):
    """rotate interleaved pairs of the first 2*cos.shape[1] channels of x (T, hd) in x's own dtype"""
    c, s = cos.astype(x.dtype), (-sin if inverse else sin).astype(x.dtype)
    r = 2 * cos.shape[1]
    a, b = x[:, 0:r:2], x[:, 1:r:2]
    out = x.copy()
    out[:, 0:r:2] = a * c - b * s
    out[:, 1:r:2] = b * c + a * s
    return out


# ------------------------------------------------------------------------------------------------ the split
def split_parts(x32, split=torch.bfloat16):
    """float32 array -> (hi, lo) as float64 arrays: hi = split_t(x), lo = split_t(x - hi), round to nearest even (csrc/common.h)"""
    x32 = np.ascontiguousarray(x32, dtype=F32)
    hi = _round_to(x32, split)
    lo = _round_to(x32 - hi, split)
    return hi.astype(np.float64), lo.astype(np.float64)


def _round_to(x32, split):
    if split == torch.float16:
        return x32.astype(np.float16).astype(F32)
    assert split == torch.bfloat16, split
    u = x32.view(np.uint32)                                      # finite inputs only: round to nearest even on the upper 16 bits
    u = (u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)
    return u.view(F32)


def _t(parts):
    return parts[0].T, parts[1].T


def _x3(a, b):
    """a (m, k) . b (n, k)^T from their (hi, lo) parts: hi*hi + hi*lo + lo*hi in float64"""
    return a[0] @ (b[0] + b[1]).T + a[1] @ b[0].T


# ------------------------------------------------------------------------------------------------ float64 and the bf16x3 twin
WORKERS = 6                         # threads of the references (numpy and torch release the GIL in their kernels)


def _pmap(fn, items):
    items = list(items)
    if len(items) < 2:
        return [fn(i) for i in items]
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(min(WORKERS, len(items))) as ex:
        return list(ex.map(fn, items))


def _pair(q, k, v, g, cos, sin, split, backward, chunk):
    """one (sample, head): q, k, v, g (T, hd) float32 -> o, lse, dq, dk, dv.  split None: float64; else the twin of the bf16x3 kernels."""
    T, hd = q.shape
    scale = hd ** -0.5
    if split is None:
        qr, kr = _rot(q.astype(np.float64), cos, sin), _rot(k.astype(np.float64), cos, sin)
        v64 = v.astype(np.float64)
        g64 = None if g is None else g.astype(np.float64)
    else:
        qr, kr = _rot(q, cos, sin), _rot(k, cos, sin)          # float32, like the kernels' staging
        kp, vp = split_parts(kr, split), split_parts(v, split)
        vtp, ktp = _t(vp), _t(kp)

    def rows(r0):
        sl = slice(r0, r0 + chunk)
        dq = dk = dv = None
        if split is None:
            qs = qr[sl] * scale
            s = qs @ kr.T
            m = s.max(-1, keepdims=True)
            p = np.exp(s - m)
            l = p.sum(-1, keepdims=True)
            p /= l
            oc = p @ v64
            lc = (m + np.log(l))[:, 0]
            if backward:
                gc = g64[sl]
                dv = p.T @ gc
                dp = gc @ v64.T
                ds = p * (dp - (gc * oc).sum(-1, keepdims=True))
                dq = (ds @ kr) * scale
                dk = ds.T @ qs
        else:
            # forward: log2 domain, log2(e) folded into the query scale (attention_stream.hip, attention_x3_body.h)
            q2 = qr[sl] * F32(F32(scale) * F32(1.44269504088896340736))
            s = _x3(split_parts(q2, split), kp)
            m = s.max(-1, keepdims=True)
            p32 = np.exp2(s - m).astype(F32)                   # unnormalised, rounded to float32 before its split
            l = p32.sum(-1, keepdims=True, dtype=np.float64)
            oc = (_x3(split_parts(p32, split), vtp) / l).astype(F32)
            lc = ((m + np.log2(l))[:, 0] * math.log(2.0)).astype(F32)
            if backward:
                # backward: natural domain, q pre-scaled, P = exp(S - lse), D = rowsum(dO * O) in float32 (attention_bwd_stream.hip)
                gc = g[sl]
                qs = qr[sl] * F32(scale)
                qsp, gp = split_parts(qs, split), split_parts(gc, split)
                s = _x3(qsp, kp)
                p32 = np.exp(s - lc.astype(np.float64)[:, None]).astype(F32)
                dsum = (gc.astype(np.float64) * oc.astype(np.float64)).sum(-1, keepdims=True).astype(F32).astype(np.float64)
                dp = _x3(gp, vp)
                ds32 = (p32 * (dp - dsum)).astype(F32)
                dsp = split_parts(ds32, split)
                dq = _x3(dsp, ktp) * scale
                dk = _x3(_t(dsp), _t(qsp))
                dv = _x3(_t(split_parts(p32, split)), _t(gp))
        return oc, lc, dq, dk, dv

    parts = _pmap(rows, range(0, T, chunk))
    o = np.concatenate([p[0] for p in parts]).astype(np.float64)
    lse = np.concatenate([p[1] for p in parts]).astype(np.float64)
    if not backward:
        return o, lse, None, None, None
    dq = np.concatenate([p[2] for p in parts])
    dk, dv = sum(p[3] for p in parts), sum(p[4] for p in parts)
    return o, lse, _rot(dq, cos, sin, inverse=True), _rot(dk, cos, sin, inverse=True), dv


def _pair32(q, k, v, g, cos, sin, backward, chunk):
    """the reference's own arithmetic in float32 (torch, CPU): q * scale @ k^T, softmax, @ v; autograd for the backward"""
    T, hd = q.shape
    scale = hd ** -0.5
    ct, st = torch.from_numpy(cos), torch.from_numpy(sin)
    r = 2 * cos.shape[1]

    def rot(x, c, s):
        a, b = x[:, 0:r:2], x[:, 1:r:2]
        return torch.cat((torch.stack((a * c - b * s, b * c + a * s), dim=-1).reshape(x.shape[0], r), x[:, r:]), dim=-1)
    qt, kt, vt, gt = (None if a is None else torch.from_numpy(np.ascontiguousarray(a)) for a in (q, k, v, g))

    def rows(r0):
        with torch.set_grad_enabled(backward):
            qc, kc, vc = (x.clone().requires_grad_(backward) for x in (qt[r0:r0 + chunk], kt, vt))
            attn = (rot(qc, ct[r0:r0 + chunk], st[r0:r0 + chunk]) * scale) @ rot(kc, ct, st).transpose(-2, -1)
            oc = attn.softmax(dim=-1) @ vc
            lc = torch.logsumexp(attn.detach(), dim=-1)
            grads = torch.autograd.grad((oc * gt[r0:r0 + chunk]).sum(), (qc, kc, vc)) if backward else (None, None, None)
        return (oc.detach(), lc) + tuple(grads)

    parts = _pmap(rows, range(0, T, chunk))
    o, lse = torch.cat([p[0] for p in parts]).numpy(), torch.cat([p[1] for p in parts]).numpy()
    if not backward:
        return o, lse, None, None, None
    return o, lse, torch.cat([p[2] for p in parts]).numpy(), sum(p[3] for p in parts).numpy(), sum(p[4] for p in parts).numpy()


def _run(pair_fn, qkv, d_o, N, T, heads, hd, backward):
    D = heads * hd
    cos, sin = rotary_tables(hd, T)
    r = qkv.reshape(N, T, 3, heads, hd)
    g = None if d_o is None else d_o.reshape(N, T, heads, hd)
    o = np.empty((N, T, heads, hd), np.float64)
    lse = np.empty((N, heads, T), np.float64)
    dqkv = np.empty((N, T, 3, heads, hd), np.float64) if backward else None

    def one(nh):
        n, h = divmod(nh, heads)
        q, k, v = (np.ascontiguousarray(r[n, :, i, h]) for i in range(3))
        res = pair_fn(q, k, v, np.ascontiguousarray(g[n, :, h]) if backward else None, cos, sin, backward)
        o[n, :, h], lse[n, h] = res[0], res[1]
        if backward:
            for i in range(3):
                dqkv[n, :, i, h] = res[2 + i]
    _pmap(one, range(N * heads))
    out = {"o": o.reshape(N * T, D), "lse": lse}
    if backward:
        out["dqkv"] = dqkv.reshape(N * T, 3 * D)
    return out


def ref64(qkv, d_o, N, T, heads, hd, backward=True, chunk=512):
    return _run(lambda q, k, v, g, c, s, b: _pair(q, k, v, g, c, s, None, b, chunk), qkv, d_o, N, T, heads, hd, backward)


def ref32(qkv, d_o, N, T, heads, hd, backward=True, chunk=512):
    return _run(lambda q, k, v, g, c, s, b: _pair32(q, k, v, g, c, s, b, chunk), qkv, d_o, N, T, heads, hd, backward)


def twin(precision, qkv, d_o, N, T, heads, hd, backward=True, split=torch.bfloat16, chunk=512):
    if precision == "fp32":
        return ref32(qkv, d_o, N, T, heads, hd, backward, chunk)
    assert precision in ("bf16x3", "bf16x3_presplit"), precision
    return _run(lambda q, k, v, g, c, s, b: _pair(q, k, v, g, c, s, split, b, chunk), qkv, d_o, N, T, heads, hd, backward)


def arith(precision):
    """the two bf16x3 modes share one twin"""
    return "fp32" if precision == "fp32" else "bf16x3"


# ------------------------------------------------------------------------------------------------ the measure
def block_err(a, b, N, T, heads, hd):
    """o (N*T, D) -> (N, 1, heads), d(qkv) (N*T, 3*D) -> (N, 3, heads): max_{t,d} |a - b| / max_{t,d} |b| of every block.
    NaN or inf anywhere in a block of `a` gives that block inf."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    comp = a.size // (N * T * heads * hd)
    a, b = a.reshape(N, T, comp, heads, hd), b.reshape(N, T, comp, heads, hd)
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b).max(axis=(1, 4))
    d = np.where(np.isfinite(d), d, np.inf)
    return d / np.abs(b).max(axis=(1, 4))


def lse_err(a, b):
    """(N, heads, T) -> (N, heads): max_t |a - b| / max(1, max_t |b|)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b).max(axis=-1)
    d = np.where(np.isfinite(d), d, np.inf)
    return d / np.maximum(1.0, np.abs(b).max(axis=-1))


def rel(a, b):
    """the suite's norm-wise measure (gpu_util.rel), for the comparisons with it"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def tolerances():
    """TOL_p of both directions: the constants of the existing kernel tests, imported (never copied)"""
    import test_gpu_guided_long
    import test_gpu_long
    return {"fwd": test_gpu_long.ATTN_TOL, "bwd": test_gpu_guided_long.ATTN_TOL}


# ------------------------------------------------------------------------------------------------ cases, cached references, the bound
RESIDENT_SHAPES = [(2, 256, 16, 72), (3, 200, 16, 72), (2, 288, 6, 64), (2, 257, 6, 64), (1, 37, 6, 64)]
STREAM_SHAPES = [(1, 512, 4, 72), (1, 1000, 4, 72), (1, 2080, 4, 72), (2, 300, 6, 64), (1, 1025, 6, 64)]
LONG_SHAPES = [(1, 8192, 2, 72), (1, 6001, 2, 64)]
LONG_FAMILIES = ("ramp_up", "lastkey", "peaked3")
PAIR_SHAPES = [(48, 128, 16, 72), (48, 129, 6, 64)]
PAIR_FAMILIES = ("peaked3", "headscale")
JUMP_SHAPES = [(1, 300, 6, 64), (1, 1000, 4, 72), (1, 6001, 2, 64), (1, 8192, 2, 72)]
JUMP_STREAM_SHAPES = [(2, 257, 6, 64)]
KEYCOUNT_SHAPES = [(1, 37, 6, 64), (2, 257, 6, 64), (2, 300, 6, 64), (1, 6001, 2, 64), (1, 8192, 2, 72)]


def shape_id(shape):
    return "x".join(map(str, shape))


def case_seed(shape):
    """one seed per shape: every family of a shape starts from the same `base`, so `randn` calibrates the very draw the others modify"""
    N, T, heads, hd = shape
    return 7000 + 13 * T + hd + N


def has_backward(fam):
    return fam not in FORWARD_ONLY and fam not in ("randn15", "zeroq")


_CACHE = {}


def inputs(fam, shape):
    return family(fam, *shape, case_seed(shape))


def reference(fam, shape):
    """ref64 of a case (o, lse, and d(qkv) where the family has a backward), cached"""
    key = ("ref64", fam, shape)
    if key not in _CACHE:
        qkv, d_o = inputs(fam, shape)
        _CACHE[key] = ref64(qkv, d_o, *shape, backward=has_backward(fam))
    return _CACHE[key]


def errors(result, fam, shape):
    """every block of a result (any of 'o', 'lse', 'dqkv') against ref64: {'o': (N, 1, heads), 'lse': (N, heads), 'dqkv': (N, 3, heads)}"""
    ref = reference(fam, shape)
    return {qn: lse_err(np.reshape(v, ref["lse"].shape), ref["lse"]) if qn == "lse" else block_err(v, ref[qn], *shape)
            for qn, v in result.items() if qn in ("o", "lse", "dqkv")}


def twin_errors(precision, fam, shape, split=torch.bfloat16):
    """block errors of the twin of `precision` on a case, cached (only the errors are kept, not the twin's tensors)"""
    key = ("twin", arith(precision), str(split), fam, shape)
    if key not in _CACHE:
        qkv, d_o = inputs(fam, shape)
        _CACHE[key] = errors(twin(arith(precision), qkv, d_o, *shape, backward=has_backward(fam), split=split), fam, shape)
    return _CACHE[key]


def headroom(precision, direction, shape, split=torch.bfloat16):
    """R_p = max(1, TOL_p / worst block of the twin on the suite's own input at this shape: `randn` x 1.5 for the forward, `randn` for the
    backward): how far above its arithmetic's model the suite already lets a kernel sit.  From o for the forward (lse uses it too: from
    lse alone it would be above 10 and check nothing), from d(qkv) for the backward.  -> (R_p, the twin's worst block)"""
    tol = tolerances()[direction][precision]
    worst = float(twin_errors(precision, "randn15", shape, split)["o"].max() if direction == "fwd"
                  else twin_errors(precision, "randn", shape, split)["dqkv"].max())
    return max(1.0, tol / worst), worst


def bound(precision, quantity, fam, shape, split=torch.bfloat16):
    """max(TOL_p, 2 * R_p * worst block of the twin on this family), the maximum taken per component: o -> (1,), lse -> (), d(qkv) -> (3,).
    The factor 2 covers where the twin places its roundings, not their draw; it is not to be raised."""
    direction = "bwd" if quantity == "dqkv" else "fwd"
    tol = tolerances()[direction][precision]
    R, _ = headroom(precision, direction, shape, split)
    e = twin_errors(precision, fam, shape, split)[quantity]
    worst = e.max() if quantity == "lse" else e.max(axis=(0, 2))
    return np.maximum(tol, 2.0 * R * worst)


def within(err, bnd):
    """every block of err (N, comp, heads) / (N, heads) within its component's bound; NaN fails"""
    if np.ndim(bnd) == 1:
        bnd = np.asarray(bnd)[None, :, None]
    return bool(np.all(err <= bnd))


# ------------------------------------------------------------------------------------------------ float64 flash forward + its mutants
def blocked64(qkv, N, T, heads, hd, mutant=None):
    """ref64's forward restated the way the streaming kernel walks it: key blocks of KEY_BLOCK, running maximum, one rescale of the
    accumulators per block.  mutant None reproduces ref64; the others are deliberately wrong variants for the sensitivity tests:
      'no_final_rescale'  the output accumulators are not rescaled when the maximum grows in the final key block
      'extra_key'         one masked key past T is counted, with score 0 (its V row is zero)"""
    D = heads * hd
    cos, sin = rotary_tables(hd, T)
    r = qkv.reshape(N, T, 3, heads, hd)
    o = np.empty((N, T, heads, hd), np.float64)
    lse = np.empty((N, heads, T), np.float64)
    nb = (T + KEY_BLOCK - 1) // KEY_BLOCK
    for n in range(N):
        for h in range(heads):
            q = _rot(r[n, :, 0, h].astype(np.float64), cos, sin) * hd ** -0.5
            k = _rot(r[n, :, 1, h].astype(np.float64), cos, sin)
            v = r[n, :, 2, h].astype(np.float64)
            m = np.full((T, 1), -np.inf)
            l = np.zeros((T, 1))
            acc = np.zeros((T, hd))
            for b in range(nb):
                ks = slice(b * KEY_BLOCK, min(T, (b + 1) * KEY_BLOCK))
                s = q @ k[ks].T
                vb = v[ks]
                if mutant == "extra_key" and b == nb - 1:
                    s = np.concatenate((s, np.zeros((T, 1))), axis=1)
                    vb = np.concatenate((vb, np.zeros((1, hd))), axis=0)
                m_new = np.maximum(m, s.max(-1, keepdims=True))
                alpha = np.exp(m - m_new)
                p = np.exp(s - m_new)
                l = l * alpha + p.sum(-1, keepdims=True)
                if not (mutant == "no_final_rescale" and b == nb - 1 and nb > 1):
                    acc *= alpha
                acc += p @ vb
                m = m_new
            o[n, :, h] = acc / l
            lse[n, h] = (m + np.log(l))[:, 0]
    return {"o": o.reshape(N * T, D), "lse": lse}


def scaled_scores(qkv, N, T, heads, hd, n=0, h=0):
    """float64 scaled scores (T, T) of one (sample, head)"""
    cos, sin = rotary_tables(hd, T)
    r = qkv.reshape(N, T, 3, heads, hd)
    q = _rot(r[n, :, 0, h].astype(np.float64), cos, sin) * hd ** -0.5
    k = _rot(r[n, :, 1, h].astype(np.float64), cos, sin)
    return q @ k.T


# ------------------------------------------------------------------------------------------------ model level: peaked synthetic weights
def peak_qk(sd, gain):
    """rgm.synth weights with the q and k rows of every attn.qkv.weight / .bias multiplied by `gain`: scores grow by gain^2, a trained
    network's peaked softmax on synthetic weights (tests/golden/make_golden_peaked.py)"""
    out = dict(sd)
    for name, w in sd.items():
        if name.endswith("attn.qkv.weight") or name.endswith("attn.qkv.bias"):
            w = np.array(w, copy=True)
            w[:2 * (w.shape[0] // 3)] *= np.asarray(gain, w.dtype)
            out[name] = w
    return out


def model_max_scores(sd, heads, forward):
    """max |scaled score| of every attention of one oracle forward: forward() runs oracle.dit_np with `sd`; -> list, one per block"""
    from oracle import dit_np as odit
    seen = []
    inner = odit.attention

    def spy(m, sd_, pre, heads_, cos, sin, cache=None):
        n, T, D = m.shape
        hd = D // heads_
        qkv = odit.linear(m, sd_[pre + "qkv.weight"], sd_[pre + "qkv.bias"]).reshape(n, T, 3, heads_, hd)
        q, k = (odit.apply_rotary(qkv[:, :, i].transpose(0, 2, 1, 3), cos, sin).astype(np.float64) for i in range(2))
        seen.append(max(float(np.abs(q[i, h] @ k[i, h].T).max()) * hd ** -0.5 for i in range(n) for h in range(heads_)))
        return inner(m, sd_, pre, heads_, cos, sin, cache)
    odit.attention = spy
    try:
        forward()
    finally:
        odit.attention = inner
    return seen
