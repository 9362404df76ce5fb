"""CPU: the inversion / bits-per-dim fixtures (tests/golden/make_golden_eval.py: the reference's ddim_reverse_sample, _vb_terms_bpd,
_prior_bpd, calc_bpd_loop in fp64) against the fp64 numpy restatement of tests/eval_ref.py, the public surface against the
reference's recorded signatures, and the fixtures' seeds against the generator's own table."""
import ast
import glob
import inspect
import json
import os

import numpy as np
import pytest

import eval_ref as er
from conftest import GOLDEN, load_golden

TIGHT = 1e-12
# calc_bpd_loop: 8 steps, and numpy's exp / tanh / log are not torch's to the last bit -- the decoder term's difference of two CDF values
# amplifies an ulp of tanh by 1 / (cdf_plus - cdf_min)
LOOP = 1e-10


def _eval_seeds():
    src = open(os.path.join(GOLDEN, "make_golden_eval.py")).read()
    node = next(n for n in ast.parse(src).body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "EVAL_SEEDS")
    return ast.literal_eval(node.value)


def test_eval_fixtures_carry_the_seeds_the_generator_pins():
    table = _eval_seeds()
    seen = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, "eval_*.npz"))):
        g = np.load(path)
        keys = [k for k in g.files if k.endswith("seed")]
        assert all(g[k].shape == (1,) for k in keys), path       # never 0-d: make_golden.py's FIXTURE_SEEDS covers those
        seen[os.path.basename(path)[:-4]] = {k: int(g[k][0]) for k in keys}
        assert os.path.getsize(path) < 1024 * 1024
    assert seen == table


def test_public_surface_has_the_reference_signatures():
    """the five methods exist on GaussianDiffusion with the reference's parameter names, in its order (fails before the feature)"""
    from guided_diffusion.gaussian_diffusion import GaussianDiffusion
    api = json.load(open(os.path.join(GOLDEN, "eval_api.json")))
    assert set(api) == {"ddim_reverse_sample", "_predict_xstart_from_xprev", "_vb_terms_bpd", "_prior_bpd", "calc_bpd_loop"}
    for name, params in api.items():
        assert list(inspect.signature(getattr(GaussianDiffusion, name)).parameters) == params, name
    loop = inspect.signature(GaussianDiffusion.ddim_reverse_sample_loop)
    assert list(loop.parameters) == ["self", "model", "x_start", "num_steps", "clip_denoised", "denoised_fn", "model_kwargs", "progress"]
    sig = inspect.signature(GaussianDiffusion.ddim_reverse_sample).parameters
    assert sig["clip_denoised"].default is True and sig["eta"].default == 0.0


@pytest.mark.parametrize("var_type", er.VAR_TYPES)
def test_restatement_reproduces_the_fp64_terms(var_type):
    g = load_golden("eval_terms")
    d = er.diffusion("8", var_type)
    vv = {"learned": g["var_log"], "learned_range": g["var_values"]}.get(var_type)
    for si, ts in enumerate(g["t_sets"]):
        for clip in (0, 1):
            r = er.vb_terms(d, var_type, g["x_start"], g["x_t"], g["eps"], g["noise"], ts, bool(clip), var_values=vv)
            tag = f"{var_type}.s{si}.c{clip}"
            for k in ("vb", "xstart_mse", "mse"):
                assert er.rel_to_max(r[k], g[f"{tag}.{k}"]) < TIGHT, (tag, k)
            assert er.rel_to_max(r["pred_xstart"], g[f"s{si}.c{clip}.pred_xstart"]) < TIGHT


def test_terms_fixture_covers_the_edge_bins():
    g = load_golden("eval_terms")
    xs = g["x_start"]
    for v in (-1.0, 1.0, -0.9995, 0.9995, -0.9985, 0.9985):
        assert (xs == np.float32(v)).sum() >= 2
    ts = g["t_sets"]
    assert {0, 1, 4, 7} == set(ts.reshape(-1).tolist()) and any(a == b for a, b in ts) and any(a != b for a, b in ts)


def test_restatement_reproduces_the_fp64_steps_and_prior():
    g, s = load_golden("eval_terms"), load_golden("eval_steps")
    d = er.diffusion("8")
    assert er.rel_to_max(er.prior_bpd(d, g["x_start"]), g["prior_bpd"]) < TIGHT
    for si, ts in enumerate(s["t_sets"]):
        assert er.rel_to_max(er.xstart_from_xprev(d, g["x_t"], ts, g["xprev"]), s[f"s{si}.xstart_from_xprev"]) < TIGHT
        for clip in (0, 1):
            sample, _ = er.ddim_reverse(d, g["x_t"], g["eps"], ts, bool(clip))
            assert er.rel_to_max(sample, s[f"s{si}.c{clip}.sample"]) < TIGHT


@pytest.mark.parametrize("prefix,var_type", [("", "fixed_large"), ("ls.", "learned_range")])
def test_restatement_reproduces_the_fp64_bpd_loop(prefix, var_type):
    """calc_bpd_loop rebuilt from the restated terms and the stored model outputs: columns in the reference's order (column 0 = the
    last timestep), total = sum of the columns + prior"""
    g = load_golden("eval_bpd")
    d = er.diffusion("8", var_type)
    xs = g[prefix + "x_start"]
    T = d.num_timesteps
    assert T == 8 and g[prefix + "model_out"].shape[0] == 8
    cols = {"vb": [], "xstart_mse": [], "mse": []}
    for j, i in enumerate(range(T)[::-1]):
        t = np.full((xs.shape[0],), i)
        nz = g[prefix + "noise"][j].astype(np.float64)
        x_t = er.tab(d.sqrt_alphas_cumprod, t, xs) * xs.astype(np.float64) + er.tab(d.sqrt_one_minus_alphas_cumprod, t, xs) * nz
        out = g[prefix + "model_out"][j]
        r = er.vb_terms(d, var_type, xs, x_t, out[:, :4], nz, t, True, var_values=out[:, 4:] if var_type == "learned_range" else None)
        for k in cols:
            cols[k].append(r[k])
    cols = {k: np.stack(v, axis=1) for k, v in cols.items()}
    for k in cols:
        assert cols[k].shape == g[f"{prefix}f64.{k}"].shape == (2, 8)
        assert er.rel_to_max(cols[k], g[f"{prefix}f64.{k}"]) < LOOP, (prefix, k)
    prior = er.prior_bpd(d, xs)
    assert er.rel_to_max(prior, g[prefix + "f64.prior_bpd"]) < TIGHT
    assert er.rel_to_max(cols["vb"].sum(axis=1) + prior, g[prefix + "f64.total_bpd"]) < LOOP
    if prefix:
        assert np.abs(g["ls.f64.vb"]).max() < 1e3 and g["ls.final_std"].shape == (1,)
