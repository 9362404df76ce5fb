"""CPU: the float64 restatement of particle rule guidance (tests/particles_ref.py) against the properties the definition promises --
systematic resampling's invariants, the prior at lambda = 0 and the closed-form tilted mean at lambda = 1 on the Gaussian data model --
and the host side of the feature: the CLI flags and the combinations particle_sample_loop refuses by name without a device."""
import importlib.util
import os
from types import SimpleNamespace

import numpy as np
import pytest

import dpmpp_ref as R
import particles_ref as P
from conftest import PKG


def test_case_builder_covers_the_definition_and_keeps_its_margins():
    names = {c[0].split(".")[0] for c in P.CASES}
    assert names == {"uniform", "dominant", "ties", "one_dead", "some_nan", "all_dead", "u0", "utop"}
    assert {c[3] for c in P.CASES} == {0.0, 0.5, 2.0}
    for n, B in ((1, 1), (3, 3), (65, 3), (256, 1)):
        for c in P.cases(n, B):
            ref = c["ref"]
            assert ref["margin_c"].min() >= P.MARGIN and ref["margin_ess"].min() >= P.MARGIN
            if c["name"] == "all_dead":
                assert (ref["resampled"] == -1).all() and (ref["logw"] == 0).all()
                assert np.array_equal(ref["anc"], np.tile(np.arange(n, dtype=np.int32)[:, None], (1, B)))
            if c["ess"] == 0.0:
                assert (ref["resampled"] <= 0).all()
            if c["ess"] == 2.0:                                         # always, unless the group has no live particle (n = 1: its only one)
                assert np.array_equal(ref["resampled"] == 1, ref["ess"] > 0) and np.array_equal(ref["resampled"] == -1, ref["ess"] == 0)


@pytest.mark.parametrize("n", [2, 3, 64, 65, 1024])
def test_systematic_resampling_invariants(n):
    """ancestors never decrease in k, a particle of weight zero is never chosen, and every count lies within 1 of n w"""
    B = 3
    seen = 0
    for c in P.cases(n, B):
        ref = c["ref"]
        r = c["reward"].astype(np.float64)
        r[~(c["reward"] < np.inf)] = -np.inf
        with np.errstate(invalid="ignore"):
            l = c["logw"] + c["lam"] * (r - c["r_prev"])
        l[(r == -np.inf) | ~(l < np.inf)] = -np.inf
        for b in np.flatnonzero(ref["resampled"] == 1):
            w = np.exp(l[:, b] - l[:, b].max())
            w /= w.sum()
            anc = ref["anc"][:, b]
            assert (np.diff(anc) >= 0).all()
            assert (w[anc] > 0).all(), c["name"]
            counts = np.bincount(anc, minlength=n)
            assert (np.abs(counts - n * w) <= 1 + 1e-9).all(), c["name"]
            assert (ref["logw"][:, b] == 0).all()
            assert np.array_equal(ref["r_prev"][:, b], np.where(r[:, b] == -np.inf, c["r_prev"][:, b], c["reward"][:, b])[anc])
            seen += 1
        for b in np.flatnonzero(ref["resampled"] == 0):                  # kept: the weights are unchanged and average to 1
            assert np.array_equal(ref["anc"][:, b], np.arange(n))
            assert abs(np.exp(ref["logw"][:, b]).mean() - 1) < 1e-12
    assert seen >= 10


# ------------------------------------------------------------------------------------ the Gaussian data model
E, N_PART, GROUPS = 2, 16, 4096
TARGET, TAU = -0.4, 0.35


def _gauss_run(lam, steps, seed):
    gm = R.GaussianModel(E, 0)
    ac = R.chain_alphas_cumprod(range(0, 1000, 1000 // steps))
    rng = np.random.RandomState(seed)
    reward = lambda x0: -(x0[:, 0] - TARGET) ** 2 / (2 * TAU ** 2)
    x, logw, final, count = P.particle_chain(ac, gm, rng.randn(N_PART * GROUPS, E), N_PART, GROUPS, reward, lam=lam, ess=0.5,
                                             noise=lambda i, s: rng.randn(*s), u=lambda i, B: rng.rand(B))
    w = P.weights(logw)
    xs = x.reshape(N_PART, GROUPS, E)
    return gm, xs, w, count


def test_lambda_zero_returns_the_prior():
    gm, xs, w, count = _gauss_run(0.0, 1000, 3)
    assert (count == 0).all() and np.allclose(w, 1.0 / N_PART)
    z = gm.standardised(xs.reshape(-1, E))
    N = z.shape[0]
    for e in range(E):
        # the full chain: the stochastic DDIM step's own variance shortfall (13 % at 100 steps, falling like 1 / steps) must sit
        # inside the sampling error of 65536 draws
        assert abs(z[:, e].mean()) <= 5 / np.sqrt(N), z[:, e].mean()
        assert abs(z[:, e].var() - 1) <= 5 * np.sqrt(2.0 / N), z[:, e].var()


def test_lambda_one_lands_on_the_closed_form_tilted_mean():
    """500 DDIM (eta = 1) steps: the weighted mean of the rewarded element within 5 % of the prior-to-tilted shift of the closed form
    (measured with this seed: 2.77 %, -0.2329 against -0.2412; docs/rounds/particles.md)"""
    gm, xs, w, count = _gauss_run(1.0, 500, 4)
    mean_t, _ = P.tilted_gaussian(gm.mu[0], gm.s[0], TARGET, TAU, 1.0)
    shift = mean_t - gm.mu[0]
    got = float((w * xs[:, :, 0]).sum(axis=0).mean())
    best = float(xs[np.argmax(-(xs[:, :, 0] - TARGET) ** 2, axis=0), np.arange(GROUPS), 0].mean())
    print(f"[particles gaussian] prior mean {gm.mu[0]:.4f}, tilted mean {mean_t:.4f}, weighted particle mean {got:.4f} "
          f"({100 * abs(got - mean_t) / abs(shift):.2f} % of the shift), best-of-{N_PART} mean {best:.4f}, target {TARGET}; "
          f"resampling steps per group {count.mean():.1f}")
    assert abs(got - mean_t) <= 0.05 * abs(shift), (got, mean_t, shift)
    assert count.sum() > 0 and count.max() < 500                    # resampling happened, and not on every step
    # the unrewarded element keeps its prior
    other = float((w * xs[:, :, 1]).sum(axis=0).mean())
    assert abs(other - gm.mu[1]) <= 5 * gm.s[1] / np.sqrt(GROUPS)


# ------------------------------------------------------------------------------------ flags and refusals
def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_cli_particles", os.path.join(PKG, "scripts", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_particle_flags_parse_and_stay_out_of_the_reference_flags():
    cli = _load("sample_rule")
    before = {a.dest for a in cli.create_argparser()._actions}
    assert not {d for d in before if d.startswith("particle")}
    full = cli.add_particle_arguments(cli.add_note_stats_arguments(cli.add_sampler_arguments(cli.create_argparser())))
    a = full.parse_args([])
    assert (a.particles, a.particle_lambda, a.particle_ess, a.particle_every, a.particle_keep) == (0, 1.0, 0.5, 1, "best")
    a = full.parse_args(["--particles", "8", "--particle_lambda", "2.5", "--particle_ess", "0.25", "--particle_every", "2",
                         "--particle_keep", "all"])
    assert (a.particles, a.particle_lambda, a.particle_ess, a.particle_every, a.particle_keep) == (8, 2.5, 0.25, 2, "all")
    with pytest.raises(SystemExit):
        full.parse_args(["--particle_keep", "some"])
    assert {a.dest for a in cli.create_argparser()._actions} == before
    assert cli.particle_metadata(full.parse_args([])) is None
    assert cli.particle_metadata(a) == {"num_particles": 8, "lambda": 2.5, "ess": 0.25, "every": 2, "keep": "all"}


def _diffusion(rs="ddim50", learn_sigma=False):
    from guided_diffusion.script_util import create_diffusion
    return create_diffusion(learn_sigma=learn_sigma, diffusion_steps=1000, noise_schedule="linear", timestep_respacing=rs,
                            use_kl=False, predict_xstart=False, rescale_timesteps=False, rescale_learned_sigmas=False)


def test_unsupported_combinations_raise_by_name_without_a_device():
    from guided_diffusion import gaussian_diffusion as gd
    d = _diffusion()

    def model(*a, **k):
        raise AssertionError("the model was called")
    shape = (2, 4, 128, 16)
    kw = dict(reward_fn=lambda x, t: x.sum(), device="cpu")
    with pytest.raises(NotImplementedError, match="edit_kwargs"):
        d.particle_sample_loop(model, shape, 4, edit_kwargs={"gt": None}, **kw)
    with pytest.raises(NotImplementedError, match="segment mode"):
        d.particle_sample_loop(model, shape, 4, guidance_kwargs=SimpleNamespace(method="no_guidance", dc=SimpleNamespace(base=128)), **kw)
    with pytest.raises(NotImplementedError, match="DPS"):
        d.particle_sample_loop(model, shape, 4, cond_fn=model, guidance_kwargs=SimpleNamespace(method="dps", schedule=False), **kw)
    with pytest.raises(ValueError, match="scg_kwargs"):
        d.particle_sample_loop(model, shape, 4, scg_kwargs={"num_samples": 4}, **kw)
    for eta in (0.0, 0.5):
        with pytest.raises(ValueError, match="eta"):
            d.particle_sample_loop(model, shape, 4, sampler="dpmpp", eta=eta, **kw)
    with pytest.raises(ValueError, match="num_particles"):
        d.particle_sample_loop(model, shape, 1025, **kw)
    with pytest.raises(ValueError, match="num_particles"):
        d.particle_sample_loop(model, shape, 0, **kw)
    with pytest.raises(ValueError, match="sampler"):
        d.particle_sample_loop(model, shape, 4, sampler="heun", **kw)
    with pytest.raises(ValueError, match="nothing to score"):
        d.particle_sample_loop(model, shape, 4, device="cpu")
    with pytest.raises(NotImplementedError, match="learned-variance"):
        _diffusion(learn_sigma=True).particle_sample_loop(model, shape, 4, **kw)
    d.model_mean_type = gd.ModelMeanType.PREVIOUS_X
    with pytest.raises(NotImplementedError, match="PREVIOUS_X"):
        d.particle_sample_loop(model, shape, 4, **kw)
    with pytest.raises(NotImplementedError, match="PREVIOUS_X"):
        next(d.particle_sample_loop_progressive(model, shape, 4, **kw))
