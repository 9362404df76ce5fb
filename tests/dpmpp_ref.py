"""Yardsticks of the DPM-Solver++(2M) tests: a numpy restatement of the step and of whole chains, evaluated in float64 (the
reference) or in float32 (whose deviation d32 from float64 sizes the tolerance), the float64 DDIM step, and a Gaussian data model
whose eps and probability-flow ODE solution are closed forms.  Written from the formulas of the paper (Lu et al. 2022, Alg. 2 and
its SDE variant), not from the package: it shares no code with guided_diffusion.gaussian_diffusion.dpmpp_tables."""
import numpy as np


def linear_alphas_cumprod(T=1000):
    k = 1000 / T
    return np.cumprod(1.0 - np.linspace(k * 0.0001, k * 0.02, T, dtype=np.float64))


def chain_alphas_cumprod(kept, base=None):
    """alphas_cumprod of the chain that keeps the timesteps `kept` of the base schedule"""
    base = linear_alphas_cumprod() if base is None else base
    return base[np.array(sorted(kept), dtype=np.int64)]


def logsnr_steps(ac, count):
    """the "logsnrN" rule: nearest timestep to each of `count` logSNR-uniform targets, lower t on a tie, both ends kept"""
    lam = 0.5 * np.log(ac / (1.0 - ac))
    kept = {0, len(ac) - 1}
    for target in np.linspace(lam[0], lam[-1], count):
        d = np.abs(lam - target)
        kept.add(int(np.flatnonzero(d == d.min())[0]))
    return kept


_TABLES = {}


def tables(ac, sde):
    """float64 (cx, cd, w1, cn) per chain index; entry 0 is the final step (h = inf), written down"""
    key = (np.asarray(ac, np.float64).tobytes(), bool(sde))
    if key not in _TABLES:
        _TABLES[key] = _tables(ac, sde)
    return _TABLES[key]


def _tables(ac, sde):
    T = len(ac)
    lam = 0.5 * np.log(ac / (1.0 - ac))
    cx, cd, w1, cn = np.zeros(T), np.zeros(T), np.zeros(T), np.zeros(T)
    cd[0] = 1.0
    for i in range(1, T):
        h = lam[i - 1] - lam[i]
        a_s, s_s, s_t = np.sqrt(ac[i - 1]), np.sqrt(1.0 - ac[i - 1]), np.sqrt(1.0 - ac[i])
        if sde:
            cx[i] = s_s / s_t * np.exp(-h)
            cd[i] = a_s * -np.expm1(-2 * h)
            cn[i] = s_s * np.sqrt(-np.expm1(-2 * h))
        else:
            cx[i] = s_s / s_t
            cd[i] = a_s * -np.expm1(-h)
        if i < T - 1:
            w1[i] = 0.5 * h / (lam[i] - lam[i + 1])
    return cx, cd, w1, cn


def step(ac, x, eps, t, grad=None, x0_prev=None, noise=None, order=2, sde=False, clip=False, t_end=0, dtype=np.float64):
    """One step for rows at chain indices t (N,), x (N, E).  The tables are float64 cast to `dtype` (what the kernel is handed in
    float32); the arithmetic runs in `dtype`.  Returns (sample, pred_xstart, g)."""
    f = dtype
    T = len(ac)
    cx, cd, w1, cn = (a.astype(f)[t][:, None] for a in tables(ac, sde))
    c1 = np.sqrt(1.0 / ac).astype(f)[t][:, None]
    c2 = np.sqrt(1.0 / ac - 1).astype(f)[t][:, None]
    acf = ac.astype(f)[t][:, None]
    x, eps = x.astype(f), eps.astype(f)
    x0 = c1 * x - c2 * eps
    if clip:
        x0 = np.clip(x0, f(-1), f(1))
    if grad is not None:
        e = (c1 * x - x0) / c2
        e = e - np.sqrt(f(1) - acf) * grad.astype(f)
        x0 = c1 * x - c2 * e
    D = x0
    if x0_prev is not None and order == 2:
        second = ((t > 0) & (t < T - 1))[:, None]
        D = np.where(second, x0 + w1 * (x0 - x0_prev.astype(f)), x0)
    s = cx * x + cd * D
    if noise is not None:
        s = s + (t != t_end).astype(f)[:, None] * cn * noise.astype(f)
    s = np.where((t == 0)[:, None], D, s)
    assert s.dtype == f and x0.dtype == f
    return s, x0, cn[:, 0]


def ddim_step(ac, x, eps, t, grad=None, noise=None, eta=0.0, clip=False, t_end=0, dtype=np.float64):
    """The DDIM step of the reference (ddim_sample with condition_score), restated"""
    f = dtype
    acp = np.append(1.0, ac[:-1])
    c1 = np.sqrt(1.0 / ac).astype(f)[t][:, None]
    c2 = np.sqrt(1.0 / ac - 1).astype(f)[t][:, None]
    ab, abp = ac.astype(f)[t][:, None], acp.astype(f)[t][:, None]
    x, eps = x.astype(f), eps.astype(f)
    x0 = c1 * x - c2 * eps
    if clip:
        x0 = np.clip(x0, f(-1), f(1))
    if grad is not None:
        e = (c1 * x - x0) / c2
        e = e - np.sqrt(f(1) - ab) * grad.astype(f)
        x0 = c1 * x - c2 * e
    e2 = (c1 * x - x0) / c2
    sigma = f(eta) * np.sqrt((f(1) - abp) / (f(1) - ab)) * np.sqrt(f(1) - ab / abp)
    s = x0 * np.sqrt(abp) + np.sqrt(f(1) - abp - sigma * sigma) * e2
    if noise is not None:
        s = s + (t != t_end).astype(f)[:, None] * sigma * noise.astype(f)
    return s, x0, sigma[:, 0]


class GaussianModel:
    """Data x0 ~ N(mu, s^2) per element: eps(x_t, t) and the probability-flow ODE solution are closed forms."""

    def __init__(self, E, seed=0):
        rng = np.random.RandomState(seed)
        self.mu = rng.uniform(-0.6, 0.6, size=E)
        self.s = rng.uniform(0.3, 0.6, size=E)

    def eps(self, ac_t, x):
        """ac_t scalar or (N, 1): E[eps | x_t] = sigma (x_t - alpha mu) / (alpha^2 s^2 + sigma^2)"""
        a = np.sqrt(ac_t)
        return np.sqrt(1.0 - ac_t) * (x - a * self.mu) / (ac_t * self.s ** 2 + 1.0 - ac_t)

    def exact(self, ac_T, x_T):
        """the ODE keeps (x_t - alpha_t mu) / sqrt(alpha_t^2 s^2 + sigma_t^2) constant; at abar = 1 that is (x - mu) / s"""
        return self.mu + self.s * (x_T - np.sqrt(ac_T) * self.mu) / np.sqrt(ac_T * self.s ** 2 + 1.0 - ac_T)

    def standardised(self, x):
        return (x - self.mu) / self.s


def chain(ac, model, x_T, order=2, sde=False, noise=None, dtype=np.float64, solver="dpmpp", eta=0.0):
    """The whole chain from the top index down.  noise: callable(i, shape) -> z of the step at index i (SDE / eta > 0)."""
    T = len(ac)
    x, prev = x_T.astype(dtype), None
    for i in range(T - 1, -1, -1):
        t = np.full(x.shape[0], i, dtype=np.int64)
        eps = model.eps(ac[i], x.astype(np.float64))
        z = noise(i, x.shape) if noise is not None else None
        if solver == "ddim":
            x, prev, _ = ddim_step(ac, x, eps, t, noise=z, eta=eta, dtype=dtype)
        else:
            x, prev, _ = step(ac, x, eps, t, x0_prev=prev, noise=z, order=order, sde=sde, dtype=dtype)
    return x


def rel_rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - b) ** 2)) / np.sqrt(np.mean(np.asarray(b, np.float64) ** 2)))


def bound(ref64, ref32, floor=1e-6):
    """(d32, tolerance): d32 = deviation of the float32 restatement from the float64 one, relative to the largest magnitude;
    the tolerance max(4 d32, floor) never comes from a kernel"""
    scale = float(np.abs(ref64).max())
    d32 = float(np.abs(ref32.astype(np.float64) - ref64).max()) / scale
    return d32, max(4.0 * d32, floor)


def rel_err(out, ref64):
    return float(np.abs(np.asarray(out, np.float64) - ref64).max() / np.abs(ref64).max())
