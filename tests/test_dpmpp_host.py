"""CPU: the logSNR spacing, the coefficient tables and the float64 restatement of DPM-Solver++(2M) (tests/dpmpp_ref.py) on the
Gaussian data model -- the figures the sampler was proposed on (docs/rounds/dpmpp.md), reproduced within 10 %."""
import numpy as np
import pytest

import dpmpp_ref as R


def _kept(rs, T=1000, betas=None):
    from guided_diffusion.respace import space_timesteps
    return space_timesteps(T, rs) if betas is None else space_timesteps(T, rs, betas=betas)


@pytest.mark.parametrize("n,length", [(20, 20), (40, 39), (50, 49), (100, 94)])
def test_logsnr_spacing_lengths_and_ends(n, length):
    kept = _kept(f"logsnr{n}")
    assert len(kept) == length and 0 in kept and 999 in kept
    assert kept == R.logsnr_steps(R.linear_alphas_cumprod(), n)


def test_logsnr_spacing_other_schedules_and_errors():
    from guided_diffusion import gaussian_diffusion as gd
    from guided_diffusion.script_util import create_gaussian_diffusion
    betas = gd.get_named_beta_schedule("cosine", 1000)
    kept = _kept("logsnr20", betas=betas)
    assert kept == R.logsnr_steps(np.cumprod(1 - betas), 20) and kept != _kept("logsnr20")
    d = create_gaussian_diffusion(steps=1000, noise_schedule="cosine", timestep_respacing="logsnr20")
    assert d.timestep_map == sorted(kept)
    np.testing.assert_allclose(d.alphas_cumprod, np.cumprod(1 - betas)[sorted(kept)], rtol=1e-12)
    with pytest.raises(ValueError):
        _kept("logsnr1")
    with pytest.raises(ValueError):
        _kept("logsnr2000")


def test_existing_respacing_strings_keep_their_meaning():
    assert _kept("ddim50") == set(range(0, 1000, 20))
    assert sorted(_kept("250"))[-3:] == [991, 995, 999]
    assert len(_kept("8")) == 8 and _kept([1000]) == set(range(1000))


@pytest.mark.parametrize("schedule", ["linear", "cosine"])
@pytest.mark.parametrize("rs", ["", "ddim50", "logsnr20", "8"])
def test_tables_finite_and_equal_to_the_restatement(schedule, rs):
    from guided_diffusion import gaussian_diffusion as gd
    from guided_diffusion.script_util import create_gaussian_diffusion
    d = create_gaussian_diffusion(steps=1000, noise_schedule=schedule, timestep_respacing=rs)
    tabs = gd.dpmpp_tables(d.alphas_cumprod)
    for mode in ("ode", "sde"):
        ref = R.tables(d.alphas_cumprod, mode == "sde")
        for name, a, b in zip("cx cd w1 cn".split(), tabs[mode], ref):
            assert a.dtype == np.float64 and a.shape == (d.num_timesteps,)
            assert np.isfinite(a).all() and np.isfinite(a.astype(np.float32)).all(), (mode, name)
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=0, err_msg=f"{mode} {name}")
        cx, cd, w1, cn = tabs[mode]
        assert (cx[0], cd[0], w1[0], cn[0]) == (0.0, 1.0, 0.0, 0.0) and w1[-1] == 0.0     # the final step is written down
        assert (cn == 0).all() if mode == "ode" else (cn[1:] > 0).all()


def test_first_order_is_ddim():
    """order 1: the ODE step is DDIM's eta = 0 step, the SDE step DDIM's eta = 1 step (mean and noise scale)"""
    ac = R.chain_alphas_cumprod(_kept("logsnr20"))
    rng = np.random.RandomState(0)
    x, eps, z = rng.randn(20, 64), rng.randn(20, 64), rng.randn(20, 64)
    t = np.arange(20)
    for sde in (False, True):
        a = R.step(ac, x, eps, t, noise=z, order=1, sde=sde)
        b = R.ddim_step(ac, x, eps, t, noise=z, eta=float(sde))
        for u, v in zip(a, b):
            np.testing.assert_allclose(u, v, rtol=0, atol=1e-12)


# relative RMS error of the final sample against the exact ODE solution: (first order, 2M), as proposed
TABLE = {"ddim20": (1.1e-1, 1.9e-1), "ddim100": (2.4e-2, 1.3e-2), "logsnr20": (9.5e-2, 1.16e-2), "logsnr50": (3.8e-2, 1.7e-3)}


@pytest.fixture(scope="module")
def ode_errors():
    E = 1 << 14
    m = R.GaussianModel(E, 0)
    xT = np.random.RandomState(1).randn(4, E)
    out = {}
    for rs in TABLE:
        ac = R.chain_alphas_cumprod(_kept(rs))
        exact = m.exact(ac[-1], xT)
        out[rs] = (R.rel_rms(R.chain(ac, m, xT, order=1), exact), R.rel_rms(R.chain(ac, m, xT, order=2), exact))
    return out


@pytest.mark.parametrize("rs", list(TABLE))
def test_ode_errors_reproduce_the_proposal(ode_errors, rs):
    e1, e2 = ode_errors[rs]
    print(f"{rs}: first order {e1:.3e}, 2M {e2:.3e}")
    assert abs(e1 / TABLE[rs][0] - 1) < 0.10 and abs(e2 / TABLE[rs][1] - 1) < 0.10


def test_2m_on_logsnr20_beats_first_order_fourfold_and_ddim100(ode_errors):
    e1, e2 = ode_errors["logsnr20"]
    print(f"logsnr20: first order / 2M = {e1 / e2:.2f}")
    assert e1 / e2 >= 4.0
    assert e2 < ode_errors["ddim100"][0]                    # 20 steps of 2M beat 100 first-order steps
    assert ode_errors["ddim20"][1] > ode_errors["ddim20"][0]  # ... and on the time-uniform spacing 2M loses: the spacing is part of it


def test_sde_variance():
    """standardised output variance over 2^20 elements: 2M SDE ~ 1, first order (DDIM eta = 1) badly under-dispersed"""
    E = 1 << 20
    m = R.GaussianModel(E, 0)
    xT = np.random.RandomState(1).randn(1, E)
    want = {10: (0.41, 1.04), 20: (0.63, 1.08), 50: (0.82, 1.01)}
    for n, (w1, w2) in want.items():
        ac = R.chain_alphas_cumprod(_kept(f"logsnr{n}"))
        rng = np.random.RandomState(2)
        v2 = m.standardised(R.chain(ac, m, xT, order=2, sde=True, noise=lambda i, s: rng.randn(*s))).var()
        v1 = m.standardised(R.chain(ac, m, xT, order=1, sde=True, noise=lambda i, s: rng.randn(*s))).var()
        print(f"logsnr{n}: first order {v1:.3f}, 2M SDE {v2:.3f}")
        assert abs(v1 / w1 - 1) < 0.10 and abs(v2 / w2 - 1) < 0.10
        if n == 20:
            assert 0.95 <= v2 <= 1.15


def test_api_surface_and_errors_without_a_device():
    """the raising cases raise before any tensor is touched"""
    import torch
    from guided_diffusion import gaussian_diffusion as gd
    from guided_diffusion.script_util import create_gaussian_diffusion
    d = create_gaussian_diffusion(steps=1000, timestep_respacing="logsnr20")
    for name in ("dpmpp_sample", "dpmpp_sample_loop", "dpmpp_sample_loop_progressive"):
        assert callable(getattr(d, name))
    x, t = torch.zeros(1, 4, 8, 8), torch.zeros(1, dtype=torch.long)

    def boom(*a, **k):
        raise AssertionError("the model was called")
    with pytest.raises(ValueError, match="eta"):
        d.dpmpp_sample(boom, x, t, eta=0.5)
    with pytest.raises(ValueError, match="order"):
        d.dpmpp_sample(boom, x, t, order=3)
    with pytest.raises(ValueError, match="SCG"):
        d.dpmpp_sample(boom, x, t, eta=0.0, scg_kwargs={"num_samples": 4})

    class G:
        method, schedule = "dps", False
    with pytest.raises(NotImplementedError, match="DPS"):
        d.dpmpp_sample(boom, x, t, eta=1.0, cond_fn=boom, guidance_kwargs=G())
    d.model_mean_type = gd.ModelMeanType.PREVIOUS_X
    with pytest.raises(NotImplementedError, match="PREVIOUS_X"):
        d.dpmpp_sample(boom, x, t)
