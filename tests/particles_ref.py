"""Yardsticks of the particle rule guidance tests: a float64 numpy restatement of one weighting-and-resampling step
(rgm_particle_resample) and of the whole particle loop on dpmpp_ref.GaussianModel, and the builder of the kernel's test cases.
Written from the definition in docs/rounds/particles.md, not from the package or the kernel.

The step, per group of n particles (columns of (n, B) arrays):
    r      = reward, NaN and +inf counted as -inf
    l      = logw + lam (r - r_prev); -inf where r or logw is -inf, or where l came out NaN / +inf.  r_prev <- r where r is finite.
    w      = exp(l - max l) / sum, ESS = 1 / sum w^2; every sum runs in ascending k (numpy.cumsum)
    resample iff ESS < ess n (ess <= 0 never, ess > 1 always); every weight 0: nothing, logw <- 0, flag -1, ESS reported 0
    systematic: c_j = w_0 + .. + w_j, c_j counted as +inf from the last particle of non-zero weight on,
                anc_k = min{j : c_j > (k + u) / n}; then logw <- 0, r_prev <- r_prev[anc]
    otherwise anc_k = k, logw <- l - max - log(sum) + log(n)
"""
import numpy as np

import dpmpp_ref as R

NS = (1, 2, 3, 63, 64, 65, 256, 1024)
BS = (1, 3, 257)
U_TOP = 1.0 - 2.0 ** -53
MARGIN = 1e-9


def resample(reward, logw, r_prev, lam, ess, u):
    """reward (n, B) float32, logw (n, B) float64, r_prev (n, B) float32, u (B,) float64 -> dict of anc (n, B) int32, logw, r_prev,
    ess (B,), resampled (B,) int32, and the two margins the exact comparisons rest on: margin_c (B,): the least distance of a threshold
    from a finite c_j where the group resampled (inf elsewhere), margin_ess (B,): |ESS - ess n| / n where 0 < ess <= 1 decides."""
    reward = np.asarray(reward, np.float32)
    n, B = reward.shape
    r = reward.astype(np.float64)
    r[~(reward < np.inf)] = -np.inf
    rp = np.asarray(r_prev, np.float32)
    lw = np.asarray(logw, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        l = lw + lam * (r - rp.astype(np.float64))
    l[(r == -np.inf) | (lw == -np.inf) | ~(l < np.inf)] = -np.inf
    rp_new = np.where(r == -np.inf, rp, reward).astype(np.float32)
    m = l.max(axis=0)
    out_anc = np.tile(np.arange(n, dtype=np.int32)[:, None], (1, B))
    out_lw, out_rp = np.zeros((n, B)), rp_new.copy()
    out_ess, flag = np.zeros(B), np.full(B, -1, dtype=np.int32)
    margin_c, margin_ess = np.full(B, np.inf), np.full(B, np.inf)
    live = np.flatnonzero(m > -np.inf)
    if live.size == 0:
        return dict(anc=out_anc, logw=out_lw, r_prev=out_rp, ess=out_ess, resampled=flag, margin_c=margin_c, margin_ess=margin_ess)
    e = np.exp(l[:, live] - m[live])
    s = np.cumsum(e, axis=0)[-1]
    w = e / s
    ssq = np.cumsum(w * w, axis=0)[-1]
    c = np.cumsum(w, axis=0)
    ESS = 1.0 / ssq
    out_ess[live] = ESS
    if ess > 1:
        go = np.ones(live.size, dtype=bool)
    elif ess > 0:
        go = ESS < ess * n
        margin_ess[live] = np.abs(ESS - ess * n) / n
    else:
        go = np.zeros(live.size, dtype=bool)
    flag[live] = go.astype(np.int32)
    with np.errstate(divide="ignore"):
        stay = l[:, live] - m[live] - np.log(s) + np.log(float(n))
    out_lw[:, live] = np.where(go[None, :], 0.0, stay)
    ks = np.arange(n, dtype=np.float64)
    for col in np.flatnonzero(go):
        b = live[col]
        last = int(np.flatnonzero(w[:, col] > 0)[-1])
        thr = (ks + u[b]) / n
        cc = c[:last, col]                                        # the finite part: c_j counts as +inf from `last` on
        anc = np.searchsorted(cc, thr, side="right")              # min{j : c_j > thr}
        out_anc[:, b] = anc
        out_rp[:, b] = rp_new[anc, b]
        if last > 0:
            at = np.searchsorted(cc, thr)
            near = np.minimum(np.abs(cc[np.clip(at, 0, last - 1)] - thr), np.abs(cc[np.clip(at - 1, 0, last - 1)] - thr))
            margin_c[b] = near.min()
    return dict(anc=out_anc, logw=out_lw, r_prev=out_rp, ess=out_ess, resampled=flag, margin_c=margin_c, margin_ess=margin_ess)


# ------------------------------------------------------------------------------------ the kernel's cases
# (name, reward kind, u kind, ess, incoming state): every reward case of the definition, u = 0 and u = 1 - 2^-53 on seeded rewards with
# a non-zero incoming state, ess in {0, 0.5, 2}
CASES = [("uniform", "uniform", "rand", e, False) for e in (0.0, 0.5, 2.0)] + \
        [("dominant", "dominant", "rand", 0.5, False), ("dominant.in", "dominant", "rand", 2.0, True)] + \
        [("ties", "ties", "rand", e, False) for e in (0.5, 2.0)] + \
        [("one_dead", "one_dead", "rand", e, True) for e in (0.5, 2.0)] + \
        [("some_nan", "some_nan", "rand", 2.0, False), ("some_nan.in", "some_nan", "rand", 0.5, True)] + \
        [("all_dead", "all_dead", "rand", 2.0, True)] + \
        [("u0", "normal", "zero", e, True) for e in (0.0, 0.5, 2.0)] + \
        [("utop", "normal", "top", e, True) for e in (0.0, 0.5, 2.0)]


def _rewards(kind, n, B, rng):
    if kind == "uniform":
        return np.tile(rng.uniform(-3, 3, size=(1, B)), (n, 1)).astype(np.float32)
    if kind == "ties":
        return rng.randint(0, 3, size=(n, B)).astype(np.float32)
    r = (2.0 * rng.randn(n, B)).astype(np.float32)
    cols = np.arange(B)
    if kind == "dominant":
        r = (0.5 * rng.randn(n, B)).astype(np.float32)
        r[rng.randint(0, n, size=B), cols] += np.float32(50.0)
    elif kind == "one_dead":
        r[rng.randint(0, n, size=B), cols] = -np.inf
    elif kind == "some_nan":
        r[rng.rand(n, B) < 0.25] = np.nan
        r[rng.randint(0, n, size=B), cols] = np.inf
    elif kind == "all_dead":
        r[:] = -np.inf
        r[rng.rand(n, B) < 0.3] = np.nan
    return r


def build_case(n, B, case, lam=0.7):
    """-> dict(inputs..., ref=resample(...)) with every margin asserted: a seed whose thresholds or ESS come too close is replaced"""
    name, kind, ukind, ess, incoming = case
    if ess * n == 1.0:
        ess = 0.75              # n = 2: an ESS of 1 (one live particle) is the least there is and equals 0.5 n -- no margin; the threshold moves up
    base = (n * 1009 + B * 17 + sum(map(ord, name)) + int(ess * 10)) % (2 ** 31)
    for attempt in range(200):
        rng = np.random.RandomState((base + 7919 * attempt) % (2 ** 31))
        reward = _rewards(kind, n, B, rng)
        if incoming:
            logw = 0.8 * rng.randn(n, B)
            logw -= np.log(np.exp(logw).mean(axis=0))
            r_prev = rng.randn(n, B).astype(np.float32)
        else:
            logw, r_prev = np.zeros((n, B)), np.zeros((n, B), dtype=np.float32)
        u = {"rand": rng.uniform(0.01, 0.99, size=B), "zero": np.zeros(B), "top": np.full(B, U_TOP)}[ukind]
        ref = resample(reward, logw, r_prev, lam, ess, u)
        if ref["margin_c"].min() >= MARGIN and ref["margin_ess"].min() >= MARGIN:
            break
    assert ref["margin_c"].min() >= MARGIN and ref["margin_ess"].min() >= MARGIN, (n, B, case, ref["margin_c"].min(), ref["margin_ess"].min())
    return dict(name=name, n=n, B=B, lam=lam, ess=ess, reward=reward, logw=logw, r_prev=r_prev, u=u, ref=ref)


_BUILT = {}


def cases(n, B):
    """every case at (n, B), computed once and shared"""
    if (n, B) not in _BUILT:
        _BUILT[(n, B)] = [build_case(n, B, c) for c in CASES]
    return _BUILT[(n, B)]


def tolerance(n):
    """two ulp per exp plus an n-term non-negative sum, in units of 2^-52"""
    return (n + 8) * 2.0 ** -52


def philox_u(seed, counter, B):
    """u_b = (w0 + 0.5) 2^-32, w0 the first word of Philox4x32-10 (Salmon et al. 2011) at counter (counter + b, 0) under key `seed`"""
    ctr = (np.uint64(counter) + np.arange(B, dtype=np.uint64))
    M = np.uint64(0xFFFFFFFF)
    c = [ctr & M, ctr >> np.uint64(32), np.zeros(B, dtype=np.uint64), np.zeros(B, dtype=np.uint64)]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return (c[0].astype(np.float64) + 0.5) * 2.0 ** -32


def ladder_rewards(n, B, rungs):
    """rewards (lam = 1, zero state) whose weights put `rungs` equal steps of c inside [0, 1 / n): the ancestor of particle 0 is
    floor(u rungs) -- it reads the group's u back to 1 / rungs"""
    w = np.full(n, (1.0 - 1.0 / n) / (n - rungs))
    w[:rungs] = 1.0 / (n * rungs)
    return np.tile(np.log(w)[:, None], (1, B)).astype(np.float32)


# ------------------------------------------------------------------------------------ the whole loop on the Gaussian model
def weights(logw):
    """(n, B) log-weights -> normalised weights per group"""
    w = np.exp(logw - logw.max(axis=0))
    return w / w.sum(axis=0)


def particle_chain(ac, gm, x_T, n, B, reward, lam=1.0, ess=0.5, every=1, noise=None, u=None, solver="ddim", dtype=np.float64):
    """The particle loop on a GaussianModel: x_T (n B, E), particle k of group b at row k B + b.  reward(x0_rows) -> (n B,);
    noise(i, shape) -> z of the step at index i; u(i, B) -> the resampling offsets of the scored step at index i.
    Returns (x (n B, E), logw (n, B), final reward (n, B), resampling count (B,))."""
    T = len(ac)
    x, prev = x_T.astype(dtype), None
    logw, r_prev = np.zeros((n, B)), np.zeros((n, B), dtype=np.float32)
    count = np.zeros(B, dtype=np.int64)
    c1, c2 = np.sqrt(1.0 / ac), np.sqrt(1.0 / ac - 1)
    for i in range(T - 1, -1, -1):
        t = np.full(x.shape[0], i, dtype=np.int64)
        eps = gm.eps(ac[i], x.astype(np.float64))
        if (T - 1 - i) % every == 0:
            x0 = c1[i] * x.astype(np.float64) - c2[i] * eps
            res = resample(np.asarray(reward(x0), np.float32).reshape(n, B), logw, r_prev, lam, ess, u(i, B))
            logw, r_prev = res["logw"], res["r_prev"]
            count += res["resampled"] == 1
            rows = (res["anc"].astype(np.int64) * B + np.arange(B)[None, :]).reshape(-1)
            x, eps = x[rows], eps[rows]
            prev = None if prev is None else prev[rows]
        z = noise(i, x.shape)
        if solver == "ddim":
            x, prev, _ = R.ddim_step(ac, x, eps, t, noise=z, eta=1.0, dtype=dtype)
        else:
            x, prev, _ = R.step(ac, x, eps, t, x0_prev=prev, noise=z, order=2, sde=True, dtype=dtype)
    final = np.asarray(reward(x.astype(np.float64)), np.float32).reshape(n, B)
    res = resample(final, logw, r_prev, lam, 0.0, np.zeros(B))
    return x, res["logw"], final, count


def tilted_gaussian(mu, s, target, tau, lam):
    """mean and variance of N(mu, s^2) exp(-lam (x - target)^2 / (2 tau^2)), normalised"""
    prec = 1.0 / s ** 2 + lam / tau ** 2
    return (mu / s ** 2 + lam * target / tau ** 2) / prec, 1.0 / prec
