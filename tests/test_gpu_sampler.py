"""-m gpu: scheduler steps, VAE decoder, rule kernels and the SCG step against the reference's goldens
(teacher-forced: the recorded noise of the golden run is injected through diffusion.noise_fn)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from rgm import synth

pytestmark = pytest.mark.gpu
F32 = np.float32
SM = dict(depth=2, hidden=384, heads=6, patch=8, in_ch=4, out_ch=4, num_classes=3)
VAE_DECODE_TOL = {"fp32": 5e-5, "bf16x3": 5e-5, "bf16x3_presplit": 5e-5}      # decoded roll against the reference, norm-wise (tests/vae_cases.py imports it)


def _dit(arch, seed, final_std=None, device_gen=False):
    from gpu_util import load_module
    from guided_diffusion.dit import DiTRotary
    m = DiTRotary(input_size=[128, 16], patch_size=8, in_channels=4, hidden_size=arch["hidden"], depth=arch["depth"],
                  num_heads=arch["heads"], num_classes=arch["num_classes"], learn_sigma=False)
    return load_module(m, synth.dit_state_dict(seed, final_std=final_std, device="cuda" if device_gen else None, **arch))


def _vae(seed=2):
    from gpu_util import load_module
    from taming.models.klvae_pedal import AutoencoderKL
    return load_module(AutoencoderKL(), synth.vae_state_dict(seed, encoder=True))


def _diffusion(rs):
    from guided_diffusion.script_util import create_diffusion
    return create_diffusion(learn_sigma=False, diffusion_steps=1000, noise_schedule="linear", timestep_respacing=rs,
                            use_kl=False, predict_xstart=False, rescale_timesteps=False, rescale_learned_sigmas=False)


def _model_fn(m):
    from functools import partial
    from guided_diffusion.condition_functions import model_fn
    return partial(model_fn, model=m, num_classes=3, class_cond=True, cfg=False, w=0.)


def _inject(d, *arrays):
    q = [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays]

    def fn(shape, device):
        z = q.pop(0)
        assert tuple(z.shape) == tuple(shape), (z.shape, shape)
        return z.to(device)
    d.noise_fn = fn


def test_philox_randn_is_counter_based_and_normal():
    from guided_diffusion.gaussian_diffusion import PhiloxNoise
    a = PhiloxNoise(seed=1234)
    full = a.fill((4096, 64), "cuda")
    part = PhiloxNoise(seed=1234).fill((1000,), "cuda", offset=777)
    assert torch.equal(full.view(-1)[777:1777], part)                  # any slice regenerates from (seed, offset)
    z = full.double()
    assert abs(z.mean().item()) < 0.01 and abs(z.std().item() - 1) < 0.01
    assert abs((z ** 4).mean().item() - 3) < 0.1 and z.abs().max().item() < 6.5
    assert not torch.equal(full, PhiloxNoise(seed=1235).fill((4096, 64), "cuda"))


@pytest.mark.parametrize("tag,rs,ddim", [("ddpm", "", False), ("ddim", "ddim50", True), ("ddpm250", "250", False)])
def test_teacher_forced_step_matches_reference(tag, rs, ddim, precision):
    from gpu_util import dev, rel
    g = load_golden("steps")
    m = _dit(SM, 11)
    d = _diffusion(rs)
    d.t_end = 0
    _inject(d, g[f"{tag}.noise"])
    kw = dict(clip_denoised=False, model_kwargs={"y": dev(g["y"])})
    x, t = dev(g["x"]), dev(g[f"{tag}.t"])
    out = d.ddim_sample(_model_fn(m), x, t, eta=1.0, **kw) if ddim else d.p_sample(_model_fn(m), x, t, **kw)
    assert rel(out["sample"].cpu().numpy(), g[f"{tag}.sample"]) < 2e-4
    assert rel(out["pred_xstart"].cpu().numpy(), g[f"{tag}.pred_xstart"]) < 2e-4


def test_vae_decoder_matches_reference_and_uint8_roll(precision):
    from gpu_util import dev, rel
    from guided_diffusion.midi_util import decode_sample_for_midi
    from guided_diffusion.gaussian_diffusion import _decode
    g = load_golden("vae_decoder")
    vae = _vae(int(g["seed"]))
    out = vae.decode(dev(g["z"]))
    assert rel(out.cpu().numpy(), g["out"]) < VAE_DECODE_TOL[precision]
    u8 = decode_sample_for_midi(dev(g["lat"]), embed_model=vae, scale_factor=1.2465, threshold=-0.95)
    assert u8.shape == (1, 128, 256, 3) and u8.dtype == torch.uint8
    # the integer stage itself is bit-exact: quantise the float roll with the oracle's quantiser
    from gpu_util import u8_flip_report
    from oracle import vae_np
    from rgm import native as R
    with R.gemm_precision_scope("fp32"):                 # the final decode's own arithmetic (midi_util.FINAL_DECODE_EXACT)
        roll = _decode(dev(g["lat"]), vae, scale_factor=1.2465)
    # every entry that differs from the reference's uint8 roll sits on a quantisation boundary (fp32 re-association; the numpy
    # oracle itself: 5 of 98304), by one grey level or the background snap -- anything else would be a bug
    # (tolerance = the float agreement of the two rolls: decoder output rel. err 5e-6 in fp32, 2.5e-5 with the bf16x3 split)
    n_bad, n_unexplained, dist = u8_flip_report(u8.cpu().numpy(), g["u8"], roll.cpu().numpy(), tol=2e-5)
    print(f"[decoder {precision}] uint8 mismatches {n_bad} / {g['u8'].size}, max boundary distance {dist:.1e}")
    assert n_unexplained == 0 and n_bad <= 16, (n_bad, n_unexplained, dist)
    # the decode in the loop's own arithmetic (what SCG's inner decodes run) stays within its round-1 bound
    u8_loop = decode_sample_for_midi(dev(g["lat"]), embed_model=vae, scale_factor=1.2465, threshold=-0.95, exact=False)
    assert int((u8_loop.cpu().numpy() != g["u8"]).sum()) <= (16 if precision == 'fp32' else 96)
    assert np.array_equal(vae_np.quantise_roll(roll.cpu().numpy()), u8.cpu().numpy())
    # fused latent path == generic tile path
    lat = dev(g["lat"])
    tiles = torch.cat(torch.chunk((lat / 1.2465).permute(0, 1, 3, 2), 2, dim=-1), dim=0).contiguous()
    dec = vae.decode(tiles)
    roll_loop = _decode(lat, vae, scale_factor=1.2465)                # both in the loop's arithmetic
    assert rel(torch.cat(torch.chunk(dec, 2, dim=0), dim=-1).cpu().numpy(), roll_loop.cpu().numpy()) < 1e-6


def _sparse_roll(rng, n, T):
    r = -1 + 0.08 * rng.rand(n, 3, 128, T).astype(F32)
    for b in range(n):
        for _ in range(60 * T // 1024 + 5):
            p = rng.randint(0, 128)
            s = rng.randint(0, T - 8)
            L = rng.randint(4, 120)
            r[b, 0, p, s:s + L] = rng.uniform(-0.5, 1.0)
            r[b, 1, p, s] = 1.0
    return r.astype(F32)


def test_rule_kernels_bit_exact_counts_and_side_effects():
    from gpu_util import dev, rel
    from music_rule_guidance.rule_maps import FUNC_DICT, LOSS_DICT
    from oracle import rules_np
    g = load_golden("rules")
    roll = _sparse_roll(np.random.RandomState(400), 3, 1024)
    for name in ("note_density", "note_density_hr_1", "note_density_hr_2", "note_density_class", "note_density_pixel"):
        r = dev(roll)
        out = FUNC_DICT[name](r)
        assert np.array_equal(out.cpu().numpy(), g[name]), name
        ro = roll.copy()
        rules_np.FUNC_DICT[name](ro)
        assert np.array_equal(r.cpu().numpy(), ro), f"{name}: in-place writes differ from the reference semantics"
    r = dev(roll)
    assert rel(FUNC_DICT["pitch_hist"](r).cpu().numpy(), g["pitch_hist"]) < 1e-6
    ro = roll.copy()
    rules_np.pitch_hist(ro)
    assert np.array_equal(r.cpu().numpy(), ro)
    r = dev(roll)
    FUNC_DICT["note_density"](r)
    assert rel(FUNC_DICT["pitch_hist"](r).cpu().numpy(), g["pitch_hist_after_nd"]) < 1e-6
    loss = LOSS_DICT["note_density"](dev(g["note_density"]), dev(g["mse_target"]))
    assert rel(loss.cpu().numpy(), g["mse_loss"]) < 1e-6
    assert FUNC_DICT["pitch_hist"](dev(roll[:1])).shape == (12,) and FUNC_DICT["note_density"](dev(roll[:1])).shape == (16,)
    # CPU tensors are staged through the device and get the in-place writes back
    rc = torch.from_numpy(roll.copy())
    out = FUNC_DICT["note_density"](rc)
    assert not out.is_cuda and np.array_equal(out.numpy(), g["note_density"])
    ro = roll.copy()
    rules_np.note_density(ro)
    assert np.array_equal(rc.numpy(), ro)
    # size-independent property at full roll length: counts are integers / interval
    big = dev(_sparse_roll(np.random.RandomState(7), 2, 4096))
    nd = FUNC_DICT["note_density"](big).cpu().numpy()
    assert nd.shape == (2, 64) and np.allclose(nd[:, :32] * 128, np.round(nd[:, :32] * 128)) and np.allclose(nd[:, 32:] * 5, np.round(nd[:, 32:] * 5))


def test_scg_step_selects_the_same_candidates_as_the_reference(precision):
    from types import SimpleNamespace
    from gpu_util import dev, rel
    g = load_golden("steps")
    m, vae = _dit(SM, 11), _vae(2)
    d = _diffusion("")
    d.t_end = 0
    _inject(d, g["scg.noise"])
    tgt = {"pitch_hist": dev(g["scg.target.pitch_hist"]), "note_density": dev(g["scg.target.note_density"])}
    guid = SimpleNamespace(schedule=True, t_start=750, t_end=0, interval=1, method="no_guidance")
    out = d.p_sample(_model_fn(m), dev(g["x"]), dev(g["scg.t"]), clip_denoised=False,
                     model_kwargs={"y": dev(g["y"]), "rule": tgt}, embed_model=vae, scale_factor=1.2465,
                     guidance_kwargs=guid, scg_kwargs={"num_samples": 4, "pitch_hist": 40., "note_density": 1.})
    assert np.array_equal(d.last_scg["max_ind"].cpu().numpy(), g["scg.max_ind"])
    assert rel(d.last_scg["total_log_prob"].cpu().numpy(), g["scg.total_log_prob"]) < 1e-4
    assert rel(out["sample"].cpu().numpy(), g["scg.sample"]) < 2e-4


def test_scg_select_first_max_tie_break_and_nan():
    from rgm import native as R
    n, B, E = 5, 3, 64
    cand = torch.arange(n * B * E, dtype=torch.float32, device="cuda").view(n * B, E)
    total = torch.tensor([[1., 7., 0.], [3., 7., float("nan")], [3., 2., 5.], [0., 7., 9.], [3., 1., 1.]], device="cuda")
    out = torch.empty(B, E, device="cuda")
    idx = torch.empty(B, dtype=torch.int64, device="cuda")
    R.check(R.lib.rgm_scg_select(R.ptr(cand), R.ptr(total), R.ptr(out), R.ptr(idx), n, B, E, R.current_stream()))
    torch.cuda.synchronize()
    assert idx.tolist() == [1, 0, 1]                                   # first maximum; NaN counts as maximal (torch.argmax)
    assert torch.equal(out, cand.view(n, B, E)[idx, torch.arange(B, device="cuda")])


@pytest.mark.parametrize("tag,arch,seed", [("sm", SM, 11), ("xl28", dict(depth=28, hidden=1152, heads=16, patch=8, in_ch=4, out_ch=4, num_classes=3), 1)])
def test_end_to_end_ddim50_latents_and_uint8_roll(tag, arch, seed, precision):
    """BASELINE config 1 on the GPU: 50 DDIM steps (eta=1), B=2, injected noise; latents within the north
    star's 1e-3, decoded uint8 piano roll equal up to re-association flips (oracle itself: ~70/786432)."""
    from gpu_util import dev, rel
    from guided_diffusion.midi_util import decode_sample_for_midi
    g = load_golden(f"e2e_ddim50_{tag}")
    m = _dit(arch, seed, final_std=0.3 / arch["hidden"] ** 0.5, device_gen=True)
    d = _diffusion("ddim50")
    rng = np.random.RandomState(700 + seed)
    xT = rng.randn(2, 4, 128, 16).astype(F32)
    nz = [rng.randn(2, 4, 128, 16).astype(F32) for _ in range(50)]
    _inject(d, xT, *nz)
    lat = d.ddim_sample_loop(_model_fn(m), (2, 4, 128, 16), clip_denoised=False, model_kwargs={"y": dev(g["y"])},
                             device="cuda", eta=1.0)
    assert rel(lat.cpu().numpy(), g["latent"]) < 1e-3
    from gpu_util import u8_flip_report
    from guided_diffusion.gaussian_diffusion import _decode
    vae = _vae(2)
    # the final decode runs in exact fp32 whatever the loop's arithmetic (midi_util.FINAL_DECODE_EXACT): the float roll the boundary
    # check needs comes from the same arithmetic
    from rgm import native as R
    u8 = decode_sample_for_midi(lat, embed_model=vae, scale_factor=1.2465, threshold=-0.95).cpu().numpy()
    with R.gemm_precision_scope("fp32"):
        roll = _decode(lat, vae, scale_factor=1.2465).cpu().numpy()
    assert R.lib.rgm_get_gemm_precision() == R.PRECISIONS[precision]          # the scope restored the loop's arithmetic
    u8_loop = decode_sample_for_midi(lat, embed_model=vae, scale_factor=1.2465, threshold=-0.95, exact=False).cpu().numpy()
    print(f"[{tag} {precision}] uint8 mismatches with the decode in the loop's arithmetic: {int((u8_loop != g['u8']).sum())}")
    # "integer piano-roll decode bit-exact under fixed seed": the integer stage is (tested above); end to end, the entries that
    # differ from the reference's roll must ALL sit on a quantisation boundary of the float roll (two fp32 summation orders of
    # the same 50-step chain disagree there: numpy oracle vs torch reference ~70 of 786432) -- by one grey level or the
    # background snap, within the float agreement of the two rolls.  Count bound = 2x the measured figures of round 1.
    n_bad, n_unexplained, dist = u8_flip_report(u8, g["u8"], roll, tol=1e-4)
    print(f"[{tag} {precision}] latent rel err {rel(lat.cpu().numpy(), g['latent']):.2e}; uint8 mismatches {n_bad} / {u8.size} "
          f"({n_unexplained} not boundary-adjacent, max boundary distance {dist:.1e})")
    assert n_unexplained == 0, (n_bad, n_unexplained, dist)
    assert n_bad / u8.size <= 1.5e-4, n_bad          # every arithmetic: the integer output comes from the exact-fp32 decoder


def test_sharded_scg_rank_sees_same_winner_and_rebuilds_it(monkeypatch):
    """The multi-GPU SCG protocol on one GPU: run the step unsharded, then replay it as 'rank 1 of 2' (candidates
    8..15 only, the other rank's log-probs supplied by a stand-in all-gather).  Same (n,B) table, same first-argmax,
    and the winner -- even when it belongs to the other rank -- is rebuilt bit-exactly from the Philox counters."""
    from types import SimpleNamespace
    from gpu_util import dev
    from rgm import scg_shard
    from guided_diffusion.gaussian_diffusion import PhiloxNoise
    g = load_golden("steps")
    m, vae = _dit(SM, 11), _vae(2)
    tgt = {"pitch_hist": dev(g["scg.target.pitch_hist"]), "note_density": dev(g["scg.target.note_density"])}
    guid = SimpleNamespace(schedule=True, t_start=750, t_end=0, interval=1, method="no_guidance")
    scg = {"num_samples": 16, "pitch_hist": 40., "note_density": 1.}

    def run(d):
        d.t_end = 0
        d.noise = PhiloxNoise(seed=99)
        out = d.p_sample(_model_fn(m), dev(g["x"]), dev(g["scg.t"]), clip_denoised=False,
                         model_kwargs={"y": dev(g["y"]), "rule": tgt}, embed_model=vae, scale_factor=1.2465,
                         guidance_kwargs=guid, scg_kwargs=scg)
        return out["sample"], d.last_scg["total_log_prob"].clone(), d.last_scg["max_ind"].clone()

    ref_sample, ref_total, ref_idx = run(_diffusion(""))
    for rank in (0, 1):
        monkeypatch.setattr(scg_shard, "partition", lambda n, r=rank: (r * n // 2, n // 2, True))

        def fake_gather(local, r=rank):
            assert torch.equal(local, ref_total[r * 8:(r + 1) * 8])            # this rank's scores == the unsharded ones
            parts = [ref_total[:8], ref_total[8:]]
            parts[r] = local
            return torch.cat(parts, dim=0)
        monkeypatch.setattr(scg_shard, "gather_totals", fake_gather)
        s, total, idx = run(_diffusion(""))
        assert torch.equal(idx, ref_idx) and torch.equal(total, ref_total)
        assert torch.equal(s, ref_sample), f"rank {rank}: rebuilt winner differs"
    assert len(set(ref_idx.tolist())) >= 1


@pytest.mark.parametrize("world", [2, 4])
def test_search_step_forward_rows_are_shared_out_over_the_ranks(monkeypatch, world):
    """SURVEY 8e, the x_t forward of an SCG search step: replayed as 'rank r of R' on one GPU the step runs the eps-network on this
    rank's rows only (R = 2: one row of the batch of 2; R = 4 > B: one row each, ranks 2 and 3 repeat rows 0 and 1), the stand-in
    all-gather supplies the other rows as the owning rank computes them, and the step ends on the unsharded winners and a latent
    equal to the unsharded one up to the batch-size dependence of the GEMM tiles (rows computed in a batch of 1 instead of 2)."""
    from types import SimpleNamespace
    from gpu_util import dev, rel
    from rgm import batch_shard
    from guided_diffusion.gaussian_diffusion import PhiloxNoise
    g = load_golden("steps")
    m, vae = _dit(SM, 11), _vae(2)
    tgt = {"pitch_hist": dev(g["scg.target.pitch_hist"]), "note_density": dev(g["scg.target.note_density"])}
    guid = SimpleNamespace(schedule=True, t_start=750, t_end=0, interval=1, method="no_guidance")
    scg = {"num_samples": 16, "pitch_hist": 40., "note_density": 1.}
    x, t, y = dev(g["x"]), dev(g["scg.t"]), dev(g["y"])
    B = x.shape[0]
    mf = _model_fn(m)

    def run(d):
        d.t_end = 0
        d.noise = PhiloxNoise(seed=99)
        out = d.p_sample(mf, x, t, clip_denoised=False, model_kwargs={"y": y, "rule": tgt}, embed_model=vae, scale_factor=1.2465,
                         guidance_kwargs=guid, scg_kwargs=scg)
        return out["sample"], d.last_scg["max_ind"].clone()

    ref_sample, ref_idx = run(_diffusion(""))
    dd = _diffusion("")
    calls = []
    for rank in range(world):
        part = batch_shard._orig_partition_rows(B, world, rank)
        assert part == ((rank * B // world, B // world) if B % world == 0 else (rank % B, 1))
        monkeypatch.setattr(batch_shard, "partition_rows", lambda b, ws=None, r=None, part=part: part)

        def fake_gather(tensors, rank=rank):                       # every rank's rows, each computed in that rank's own small batch
            out = []
            for tns in tensors:
                rows = []
                for r in range(world):
                    b0, nb = batch_shard._orig_partition_rows(B, world, r)
                    if r == rank:
                        rows.append(tns)
                    else:
                        with torch.no_grad():
                            tr = t[b0:b0 + nb].contiguous()
                            rows.append(dd._wrap_model(mf)(x[b0:b0 + nb].contiguous(), dd._scale_timesteps(tr), y=y[b0:b0 + nb],
                                                           rule={k: v[b0:b0 + nb] for k, v in tgt.items()}).float())
                out.append(torch.cat(rows, dim=0))
            calls.append((rank, tensors[0].shape[0]))
            return out
        monkeypatch.setattr(batch_shard, "gather_rows", fake_gather)
        s, idx = run(_diffusion(""))
        assert torch.equal(idx, ref_idx), f"rank {rank} of {world}: other winners"
        assert rel(s.cpu().numpy(), ref_sample.cpu().numpy()) < 2e-5, rank
    assert calls == [(r, max(1, B // world)) for r in range(world)]


def test_search_step_eps_and_gradient_rows_go_to_different_ranks_when_there_are_twice_as_many(monkeypatch):
    """R >= 2 B with classifier guidance (C4 on 8 GPUs: B = 4): batch_shard.partition_roles gives rank b the eps-network forward of
    row b and rank B + b its guidance gradient -- the two do not depend on each other (condition_functions.py:58-64) -- and ONE
    all-gather of (eps | gradient) slots completes both.  Replayed as 'rank r of 4' for B = 2 on one GPU with a stand-in all-gather
    that computes the other ranks' slots the way those ranks would: every rank ends on the unsharded winners and latent."""
    from functools import partial
    from types import SimpleNamespace
    from gpu_util import dev, rel
    from rgm import batch_shard
    from guided_diffusion.condition_functions import composite_nn_zt
    from guided_diffusion.gaussian_diffusion import PhiloxNoise
    from test_gpu_pins2 import _cls
    g = load_golden("steps")
    m, vae, cm = _dit(SM, 11), _vae(2), _cls()
    tgt = {"pitch_hist": dev(g["scg.target.pitch_hist"]), "note_density": dev(g["scg.target.note_density"])}
    cond = partial(composite_nn_zt, fns=["grad_nn_zt_mse"], classifier_scales=[10.], classifiers=[cm], rule_names=["note_density"])
    guid = SimpleNamespace(schedule=True, t_start=750, t_end=0, interval=1, method="classifier_guidance")
    scg = {"num_samples": 8, "pitch_hist": 40., "note_density": 1.}
    x, t, y = dev(g["x"]), dev(g["scg.t"]), dev(g["y"])
    B, world = x.shape[0], 4
    assert B == 2
    mf = _model_fn(m)

    def run(d):
        d.t_end = 0
        d.noise = PhiloxNoise(seed=7)
        out = d.p_sample(mf, x, t, clip_denoised=False, cond_fn=cond, model_kwargs={"y": y, "rule": tgt}, embed_model=vae,
                         scale_factor=1.2465, guidance_kwargs=guid, scg_kwargs=scg)
        return out["sample"], d.last_scg["max_ind"].clone()

    assert [batch_shard.partition_roles(B, world, r) for r in range(world)] == [(0, 0), (1, 0), (0, 1), (1, 1)]
    assert batch_shard.partition_roles(4, 8, 6) == (2, 1) and batch_shard.partition_roles(4, 4, 1) is None and batch_shard.partition_roles(3, 8, 0) is None
    ref_sample, ref_idx = run(_diffusion(""))
    dd = _diffusion("")
    seen = []
    for rank in range(world):
        monkeypatch.setattr(batch_shard, "partition_rows", lambda b, ws=None, r=None, rank=rank: batch_shard._orig_partition_rows(b, world, rank))
        monkeypatch.setattr(batch_shard, "partition_roles", lambda b, ws=None, r=None, rank=rank: batch_shard._orig_partition_roles(b, world, rank))

        def fake_gather(tensors, rank=rank):
            assert len(tensors) == 2 and tensors[0].shape[0] == 1
            slots = [[], []]
            for r in range(world):
                row, role = batch_shard._orig_partition_roles(B, world, r)
                if r == rank:
                    mine = [tensors[0], tensors[1]]
                else:
                    xr, tr = x[row:row + 1].contiguous(), t[row:row + 1].contiguous()
                    kw = {"y": y[row:row + 1], "rule": {k: v[row:row + 1] for k, v in tgt.items()}}
                    with torch.no_grad():
                        val = (dd._wrap_model(mf)(xr, dd._scale_timesteps(tr), **kw) if role == 0 else dd._wrap_model(cond)(xr, dd._scale_timesteps(tr), **kw)).float()
                    mine = [val if role == 0 else torch.zeros_like(val), val if role == 1 else torch.zeros_like(val)]
                slots[0].append(mine[0])
                slots[1].append(mine[1])
            my_row, my_role = batch_shard._orig_partition_roles(B, world, rank)
            assert float(tensors[1 - my_role].abs().max()) == 0.0 and float(tensors[my_role].abs().max()) > 0.0
            seen.append((rank, my_role))
            return [torch.cat(slots[0], dim=0), torch.cat(slots[1], dim=0)]
        monkeypatch.setattr(batch_shard, "gather_rows", fake_gather)
        s, idx = run(_diffusion(""))
        assert torch.equal(idx, ref_idx), f"rank {rank} of {world}: other winners"
        assert rel(s.cpu().numpy(), ref_sample.cpu().numpy()) < 2e-5, rank
    assert seen == [(0, 0), (1, 0), (2, 1), (3, 1)]


def test_sharded_segmentwise_scg_matches_unsharded(monkeypatch):
    """dc.base > 0 (per-segment winners, reference :562-592) under candidate sharding: rank r scores its half of the
    candidates on every segment, the stand-in all-gather completes the (n, S, B) table, every rank picks the same
    per-segment winners and rebuilds them -- local or not -- from the Philox counters: bit-identical to one GPU."""
    from types import SimpleNamespace
    from gpu_util import dev
    from rgm import scg_shard
    from guided_diffusion.gaussian_diffusion import PhiloxNoise
    g = load_golden("steps")
    m, vae = _dit(SM, 11), _vae(2)
    tgt = {"pitch_hist": dev(g["scg.target.pitch_hist"]), "note_density": dev(g["scg.target.note_density"])}
    guid = SimpleNamespace(schedule=True, t_start=750, t_end=0, interval=1, method="no_guidance", dc=SimpleNamespace(base=64))
    scg = {"num_samples": 8, "pitch_hist": 40., "note_density": 1.}

    def run(d):
        d.t_end = 0
        d.noise = PhiloxNoise(seed=321)
        out = d.p_sample(_model_fn(m), dev(g["x"]), dev(g["scg.t"]), clip_denoised=False,
                         model_kwargs={"y": dev(g["y"]), "rule": tgt}, embed_model=vae, scale_factor=1.2465,
                         guidance_kwargs=guid, scg_kwargs=scg)
        return out["sample"], d.last_scg["total_log_prob"].clone(), d.last_scg["max_ind"].clone()

    ref_sample, ref_total, ref_idx = run(_diffusion(""))
    assert ref_total.shape == (8, 2, 2) and ref_idx.shape == (2, 2)               # (n, segments, B), (segments, B)
    for rank in (0, 1):
        monkeypatch.setattr(scg_shard, "partition", lambda n, r=rank: (r * n // 2, n // 2, True))

        def fake_gather(local, r=rank):
            mine = ref_total[r * 4:(r + 1) * 4].reshape(4, -1)
            assert torch.equal(local, mine)
            parts = [ref_total[:4].reshape(4, -1), ref_total[4:].reshape(4, -1)]
            parts[r] = local
            return torch.cat(parts, dim=0)
        monkeypatch.setattr(scg_shard, "gather_totals", fake_gather)
        s, total, idx = run(_diffusion(""))
        assert torch.equal(idx, ref_idx) and torch.equal(total, ref_total)
        assert torch.equal(s, ref_sample), f"rank {rank}: rebuilt segment winners differ"


def test_full_size_batch_is_row_independent_of_the_small_pinned_batches(precision):
    """BASELINE config 2 runs B = 16 (and SCG decodes hundreds of squares at once); the goldens pin B = 2.  Size-independent
    property that carries the parity over: every sample of the big batch equals the same sample computed in a batch of 2
    (tile shapes, grids and kernels differ with the batch size; the per-row arithmetic must not)."""
    from gpu_util import dev, rel
    arch = dict(depth=28, hidden=1152, heads=16, patch=8, in_ch=4, out_ch=4, num_classes=3)
    m = _dit(arch, 1, final_std=0.3 / 1152 ** 0.5, device_gen=True)
    rng = np.random.RandomState(77)
    x = dev(rng.randn(16, 4, 128, 16).astype(F32))
    t = dev(rng.randint(0, 1000, size=16).astype(np.int64))
    y = dev(rng.randint(0, 3, size=16).astype(np.int64))
    big = m(x, t, y)
    for i in (0, 6, 14):
        small = m(x[i:i + 2].contiguous(), t[i:i + 2].contiguous(), y[i:i + 2].contiguous())
        # presplit mode: the batch-of-2 GEMMs with K = 4608 run split-K (a different, still deterministic, summation order)
        assert rel(big[i:i + 2].cpu().numpy(), small.cpu().numpy()) < (3e-5 if precision == "bf16x3_presplit" else 2e-6), i
    vae = _vae(2)
    z = dev(rng.randn(64, 4, 16, 16).astype(F32))
    dec = vae.decode(z)
    # pre-split mode: the big batch's 3x3 convs run the one-wave-per-SIMD kernels with channel-block-major K (gemm2.hip ALOAD 2), the
    # batch of 2 the 128-row kernels with tap-major K -- the same bf16x3 products in another fp32 summation order (measured 5e-6)
    vtol = 2e-5 if precision == "bf16x3_presplit" else 2e-6
    for i in (0, 31, 62):
        assert rel(dec[i:i + 2].cpu().numpy(), vae.decode(z[i:i + 2].contiguous()).cpu().numpy()) < vtol, i


def test_chord_rule_device_preamble_and_host_plugin():
    """a11: the roll arithmetic of get_chords (mask, background snap, 0..127 quantisation) is a kernel, bit-exact with the reference
    incl. the writes into the caller's roll; the symbolic analysis is the registered host function, called once per excerpt with
    the reference's piano_roll_to_chords signature, in this process or in the spawn-context worker pool -- same answers."""
    from conftest import chord_test_roll
    from gpu_util import dev, fake_chord_backend
    from guided_diffusion.gaussian_diffusion import _extract_rule
    from guided_diffusion.midi_util import eval_rule_loss
    from music_rule_guidance import music_rules
    g = load_golden("chord_quantise")
    roll = dev(chord_test_roll(int(g["seed"])))
    q = music_rules.chord_quantise(roll)
    assert q.dtype == torch.uint8 and np.array_equal(q.cpu().numpy(), g["q"])
    after = roll.cpu().numpy()
    assert float(after.astype(np.float64).sum()) == float(g["after_sum"]) and int((after == -1).sum()) == int(g["after_minus1"])
    assert np.array_equal(after[:, 0, 60], g["after_ch0_row60"])
    with pytest.raises(ImportError):
        music_rules.register_chord_backend(None)
        music_rules.get_chords(roll)
    expect = [fake_chord_backend(g["q"][i].astype(np.intc), return_key=True) for i in range(3)]
    try:
        for workers in (0, 2):
            music_rules.register_chord_backend(fake_chord_backend, workers=workers)
            fresh = dev(chord_test_roll(int(g["seed"])))
            chords, keys, corr = music_rules.get_chords(fresh, return_key=True)
            assert chords.shape == (3, 2) and chords.dtype == torch.long
            assert torch.equal(chords, torch.stack([e["chords"] for e in expect]))
            assert keys == [e["key"] for e in expect] and corr == [e["correlationCoefficient"] for e in expect]
            assert music_rules.get_chords(dev(chord_test_roll(int(g["seed"]))[:1])).shape == (2,)       # N == 1 squeezes
        # the sampler evaluates chord rules on a copy (the reference's .cpu() chunks): the caller's roll keeps its values
        keep = dev(chord_test_roll(int(g["seed"])))
        before = keep.clone()
        out = _extract_rule("chord_progression", keep)
        assert torch.equal(keep, before) and out.shape == (3, 2) and out.device == keep.device
        # the report path: key indices become key names
        df = eval_rule_loss(dev(chord_test_roll(int(g["seed"]))), {"chord_progression": torch.zeros(3, 2, dtype=torch.long)})
        assert list(df["chord_progression.key_str"]) == [music_rules.IND2KEY[e["key"]] for e in expect]
    finally:
        music_rules.register_chord_backend(None)


def test_full_size_guidance_and_scg_decode_are_row_independent(precision):
    """The shapes the bench runs but the goldens cannot hold: BASELINE config 3's classifier value-and-
    gradient at B = 32 (DiTRotary-S/8-cls, depth 12) and config 4's SCG decode of 512 latent squares (B = 4, n = 16) at once.
    Size-independent property: every row of the big call equals the same row computed in a batch of 2 (other tiles, grids and
    kernels -- same per-row arithmetic), which the goldens pin."""
    from gpu_util import dev, load_module, rel
    from guided_diffusion.dit import DiTRotaryClassifier
    arch = dict(depth=12, hidden=384, heads=6, patch=8, in_ch=4, classifier=True, cls_classes=16)
    clf = load_module(DiTRotaryClassifier(input_size=[128, 16], patch_size=8, in_channels=4, hidden_size=384, depth=12, num_heads=6,
                                          num_classes=16), synth.dit_state_dict(3, **arch))
    rng = np.random.RandomState(91)
    x = dev(rng.randn(32, 4, 128, 16).astype(F32))
    t = dev(rng.randint(0, 1000, size=32).astype(np.int64))
    tgt = dev((rng.rand(32, 16) * 4).astype(F32))
    logits, grad = clf.value_and_grad(x, t, tgt, "mse", 10.0)
    tol = 2e-6 if precision == "fp32" else 3e-5
    for i in (0, 14, 30):
        l2, g2 = clf.value_and_grad(x[i:i + 2].contiguous(), t[i:i + 2].contiguous(), tgt[i:i + 2].contiguous(), "mse", 10.0)
        assert rel(logits[i:i + 2].cpu().numpy(), l2.cpu().numpy()) < tol, i
        assert rel(grad[i:i + 2].cpu().numpy(), g2.cpu().numpy()) < 10 * tol, i
    vae = _vae(2)
    z = dev(rng.randn(512, 4, 16, 16).astype(F32))
    dec = vae.decode(z)
    assert dec.shape == (512, 3, 128, 128)
    vtol = 2e-5 if precision == "bf16x3_presplit" else 2e-6          # other K order of the big batch's convs (see the test above)
    for i in (0, 255, 510):
        assert rel(dec[i:i + 2].cpu().numpy(), vae.decode(z[i:i + 2].contiguous()).cpu().numpy()) < vtol, i
    # and the latent-shaped path SCG uses (64 candidates x 8 squares, segment-major gather inside the kernel)
    from guided_diffusion.gaussian_diffusion import _decode
    lat = dev(rng.randn(64, 4, 128, 16).astype(F32))
    roll = _decode(lat, vae, scale_factor=1.2465)
    assert roll.shape == (64, 3, 128, 1024)
    for i in (0, 33, 62):
        assert rel(roll[i:i + 2].cpu().numpy(), _decode(lat[i:i + 2].contiguous(), vae, scale_factor=1.2465).cpu().numpy()) < vtol, i


@pytest.mark.parametrize("kind", ["ddpm_cls", "ddim", "dps"])
def test_batch_sharded_step_reproduces_the_unsharded_rows(kind, monkeypatch):
    """SURVEY 8e for the steps outside SCG's search: the step replayed as 'rank r of 2' (this rank's rows only, the other rank's
    rows supplied by a stand-in all-gather) gives the unsharded step's rows bit for bit -- same kernels per row, and the Philox
    draw of a row does not depend on which rank materialises it."""
    from functools import partial
    from types import SimpleNamespace
    from gpu_util import dev, load_module
    from rgm import batch_shard
    from guided_diffusion.condition_functions import composite_nn_zt
    from guided_diffusion.dit import DiTRotaryClassifier
    from guided_diffusion.gaussian_diffusion import PhiloxNoise
    g = load_golden("steps")
    m = _dit(SM, 11)
    carch = dict(depth=2, hidden=384, heads=6, patch=8, in_ch=4, classifier=True, cls_classes=16)
    cm = load_module(DiTRotaryClassifier(input_size=[128, 16], patch_size=8, in_channels=4, hidden_size=384, depth=2, num_heads=6,
                                         num_classes=16), synth.dit_state_dict(4, **carch))
    rng = np.random.RandomState(3)
    x = dev(np.concatenate([g["x"], rng.randn(2, 4, 128, 16).astype(F32)]))          # B = 4
    y = dev(np.array([1, 2, 0, 1], dtype=np.int64))
    rule = {"note_density": dev((rng.rand(4, 16) * 4).astype(F32))}

    def run(d):
        d.t_end = 0
        d.noise = PhiloxNoise(seed=5)
        kw = dict(clip_denoised=False, model_kwargs={"y": y, "rule": rule})
        if kind == "ddim":
            return d.ddim_sample(_model_fn(m), x, dev(np.full(4, 30, dtype=np.int64)), eta=1.0, **kw)
        fn = "grad_nn_zt_mse" if kind == "ddpm_cls" else "nn_z0_mse_dummy"
        cond = partial(composite_nn_zt, fns=[fn], classifier_scales=[10. if kind == "ddpm_cls" else 1.], classifiers=[cm],
                       rule_names=["note_density"])
        gk = SimpleNamespace(schedule=False, method="classifier_guidance" if kind == "ddpm_cls" else "dps", step_size=1.5, nn=True, vae=False)
        return d.p_sample(_model_fn(m), x, dev(np.full(4, 120, dtype=np.int64)), cond_fn=cond, guidance_kwargs=gk, **kw)

    chain = "ddim50" if kind == "ddim" else "250"
    ref = run(_diffusion(chain))
    for rank in (0, 1):
        monkeypatch.setattr(batch_shard, "partition", lambda B, r=rank: (r * B // 2, B // 2, True))

        def fake_gather(tensors, r=rank):
            out = []
            for mine, full in zip(tensors, (ref["sample"], ref["pred_xstart"])):
                assert mine.shape[0] == 2
                parts = [full[:2].clone(), full[2:].clone()]
                parts[r] = mine
                out.append(torch.cat(parts, dim=0))
            return out
        monkeypatch.setattr(batch_shard, "gather_rows", fake_gather)
        got = run(_diffusion(chain))
        assert torch.equal(got["sample"], ref["sample"]), f"rank {rank}: rows differ from the unsharded step"
        assert torch.equal(got["pred_xstart"], ref["pred_xstart"])
