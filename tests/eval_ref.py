"""fp64 numpy restatement of the inversion / bits-per-dim terms (reference gaussian_diffusion.py :366-374, :978-1014, :1145-1178,
:1255-1272, :1297-1318; losses.py :12-77), shared by tests/test_eval_fixtures.py (CPU, against the reference's fp64 results) and
tests/test_gpu_eval.py (the kernels against it at sizes no fixture holds).

The schedule tables enter as the reference's _extract_into_tensor hands them over: the float64 table entry cast to float32.  Everything
else is float64."""
import numpy as np

F64 = np.float64
VAR_TYPES = ("fixed_large", "fixed_small", "learned", "learned_range")


def diffusion(rs, var_type="fixed_large", mean_type="EPSILON"):
    """this project's (host-side, numpy) schedule object for a re-spaced linear 1000-step chain"""
    from guided_diffusion import gaussian_diffusion as gd
    from guided_diffusion.respace import SpacedDiffusion, space_timesteps
    vt = {"fixed_large": gd.ModelVarType.FIXED_LARGE, "fixed_small": gd.ModelVarType.FIXED_SMALL, "learned": gd.ModelVarType.LEARNED,
          "learned_range": gd.ModelVarType.LEARNED_RANGE}[var_type]
    return SpacedDiffusion(use_timesteps=space_timesteps(1000, rs), betas=gd.get_named_beta_schedule("linear", 1000),
                           model_mean_type=getattr(gd.ModelMeanType, mean_type), model_var_type=vt, loss_type=gd.LossType.MSE,
                           rescale_timesteps=False)


def tab(arr, t, like):
    """_extract_into_tensor: float32-cast table entries, broadcast over the sample's elements, as float64"""
    v = np.asarray(arr, dtype=F64)[np.asarray(t)].astype(np.float32).astype(F64)
    return v.reshape((-1,) + (1,) * (np.ndim(like) - 1))


def mean_flat(a):
    return a.reshape(a.shape[0], -1).mean(axis=1)


def normal_kl(mean1, logvar1, mean2, logvar2):
    return 0.5 * (-1.0 + logvar2 - logvar1 + np.exp(logvar1 - logvar2) + (mean1 - mean2) ** 2 * np.exp(-logvar2))


def approx_cdf(x):
    return 0.5 * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))


def discretized_gaussian_log_likelihood(x, means, log_scales):
    c = x - means
    inv = np.exp(-log_scales)
    cdf_plus, cdf_min = approx_cdf(inv * (c + 1.0 / 255.0)), approx_cdf(inv * (c - 1.0 / 255.0))
    return np.where(x < -0.999, np.log(np.maximum(cdf_plus, 1e-12)),
                    np.where(x > 0.999, np.log(np.maximum(1.0 - cdf_min, 1e-12)), np.log(np.maximum(cdf_plus - cdf_min, 1e-12))))


def pred_xstart(d, x_t, eps, t, clip):
    x0 = tab(d.sqrt_recip_alphas_cumprod, t, x_t) * x_t.astype(F64) - tab(d.sqrt_recipm1_alphas_cumprod, t, x_t) * eps.astype(F64)
    return np.clip(x0, -1, 1) if clip else x0


def model_log_variance(d, var_type, t, like, var_values):
    if var_type == "learned":
        return var_values.astype(F64)
    if var_type == "learned_range":
        frac = (var_values.astype(F64) + 1) / 2
        return frac * tab(np.log(d.betas), t, like) + (1 - frac) * tab(d.posterior_log_variance_clipped, t, like)
    if var_type == "fixed_small":
        return tab(d.posterior_log_variance_clipped, t, like) * np.ones(like.shape)
    return tab(np.log(np.append(d.posterior_variance[1], d.betas[1:])), t, like) * np.ones(like.shape)


def vb_terms(d, var_type, x_start, x_t, eps, noise, t, clip, var_values=None, model_mean=None, model_xstart=None):
    """-> {'vb', 'xstart_mse', 'mse' (N,), 'pred_xstart'}: _vb_terms_bpd's output and calc_bpd_loop's two errors of one step"""
    t = np.asarray(t)
    xs, xt = x_start.astype(F64), x_t.astype(F64)
    if model_xstart is not None:
        x0 = np.clip(model_xstart.astype(F64), -1, 1) if clip else model_xstart.astype(F64)
    else:
        x0 = pred_xstart(d, x_t, eps, t, clip)
    c1, c2 = tab(d.posterior_mean_coef1, t, xt), tab(d.posterior_mean_coef2, t, xt)
    mean = c1 * x0 + c2 * xt if model_mean is None else model_mean.astype(F64)
    lv = model_log_variance(d, var_type, t, xt, var_values)
    kl = mean_flat(normal_kl(c1 * xs + c2 * xt, tab(d.posterior_log_variance_clipped, t, xt), mean, lv)) / np.log(2.0)
    nll = mean_flat(-discretized_gaussian_log_likelihood(xs, mean, 0.5 * lv)) / np.log(2.0)
    out = {"vb": np.where(t == 0, nll, kl), "xstart_mse": mean_flat((x0 - xs) ** 2), "pred_xstart": x0}
    if noise is not None:
        e = (tab(d.sqrt_recip_alphas_cumprod, t, xt) * xt - x0) / tab(d.sqrt_recipm1_alphas_cumprod, t, xt)
        out["mse"] = mean_flat((e - noise.astype(F64)) ** 2)
    return out


def prior_bpd(d, x_start):
    T = np.full((x_start.shape[0],), d.num_timesteps - 1)
    xs = x_start.astype(F64)
    return mean_flat(normal_kl(tab(d.sqrt_alphas_cumprod, T, xs) * xs, tab(d.log_one_minus_alphas_cumprod, T, xs), 0.0, 0.0)) / np.log(2.0)


def xstart_from_xprev(d, x_t, t, xprev):
    return (tab(1.0 / d.posterior_mean_coef1, t, x_t) * xprev.astype(F64)
            - tab(d.posterior_mean_coef2 / d.posterior_mean_coef1, t, x_t) * x_t.astype(F64))


def ddim_reverse(d, x, eps, t, clip):
    """-> (sample, pred_xstart) of ddim_reverse_sample"""
    t = np.asarray(t)
    xv = x.astype(F64)
    x0 = pred_xstart(d, x, eps, t, clip)
    e = (tab(d.sqrt_recip_alphas_cumprod, t, xv) * xv - x0) / tab(d.sqrt_recipm1_alphas_cumprod, t, xv)
    abn = tab(d.alphas_cumprod_next, t, xv)
    return x0 * np.sqrt(abn) + np.sqrt(1 - abn) * e, x0


def bound(d_ref):
    """the issue's bound: at most four times as far from the fp64 truth as the reference's own fp32 result, floor 1e-6"""
    return max(4.0 * float(np.asarray(d_ref).reshape(-1)[0]), 1e-6)


def rel_to_max(a, b):
    a, b = np.asarray(a, dtype=F64), np.asarray(b, dtype=F64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))
