"""-m gpu: the VAE kernels (csrc/vae.hip, the implicit-GEMM 3x3 convs and the GroupNorm epilogue of csrc/gemm2_body.h) on offset, peaked,
dead-group and edge inputs (tests/vae_cases.py): decoder, encoder and the decoder's input gradient, every block on its own -- roll
(square, channel), moments (tile, channel), d(latent) (sample, channel, square) -- against the reference's float64 results stored in
tests/golden/vae_inputs.npz, under a bound derived from the existing tolerances and the stored errors of the float32 reference and of the
bf16x3 twin (vae_cases.bound); plus checks whose expected value is known exactly: the GroupNorm routes agree bit for bit on stressed
inputs, nothing leaks between squares, the integer stage is exact.  Nothing here provokes anything: NaN latents are data, the tests read
and compare.

Set RGM_VAE_REPORT to a file name to get one JSON line per (family, quantity, shape, route, precision): tools/vae_inputs_table.py turns
them into the table of docs/rounds/vae_inputs.md."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import vae_cases as V

pytestmark = pytest.mark.gpu
F32 = np.float32


def _vae(family):
    from gpu_util import load_module
    from taming.models.klvae_pedal import AutoencoderKL
    return load_module(AutoencoderKL(), V.weights(family))


def _routes(precision):
    """the heuristic tiles; in the pre-split arithmetic also the 256x256 / 512x128 conv kernels (rgm_set_big_tiles(1, 1)), the only
    arithmetic that has them"""
    return ("auto", "big") if precision == "bf16x3_presplit" else ("auto",)


class _Route:
    def __init__(self, route):
        self.route = route

    def __enter__(self):
        from rgm import native as R
        if self.route == "big":
            R.check(R.lib.rgm_set_big_tiles(1, 1))
        return self

    def __exit__(self, *exc):
        from rgm import native as R
        R.check(R.lib.rgm_set_big_tiles(1, 256))
        return False


def _report(**rec):
    path = os.environ.get("RGM_VAE_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")


def _check(failures, precision, route, family, quantity, got, H=16):
    """every block of one result within the bound of its case; the figures are printed before anything is asserted"""
    err = V.block_err(got, V.reference(family, quantity, H), quantity)
    bnd = V.bound(precision, family, quantity, H)
    R_p, base_worst = V.headroom(precision, quantity, H)
    comp = float(V.comparator_errors(precision, family, quantity, H).max())
    ref32 = float(V.comparator_errors("fp32", family, quantity, H).max())
    norm = V.rel(got, V.reference(family, quantity, H))
    print(f"{family} {quantity} H={H} {route} {precision}: kernel worst block {err.max():.2e} (norm-wise {norm:.2e}), comparator {comp:.2e}, "
          f"ref32 {ref32:.2e}, R_p {R_p:.2f}, bound {bnd:.2e}")
    _report(family=family, quantity=quantity, H=H, route=route, precision=precision, kernel=float(err.max()), norm=norm, comparator=comp,
            ref32=ref32, R=R_p, bound=bnd)
    if not V.within(err, bnd):
        failures.append((family, quantity, H, route, precision, float(err.max()), bnd, np.argwhere(~(err <= bnd)).tolist()[:4]))


# ------------------------------------------------------------------------------------------------ against the float64 reference
@pytest.mark.parametrize("family", V.DECODE_FAMILIES)
def test_decoder_on_stressed_inputs_block_by_block(family, precision):
    """vae.decode of one square for every family, decode_latent of two squares (N = 1, H = 32) for `offset` and `impulse`"""
    from gpu_util import dev
    from rgm import native as R
    from test_gpu_fullsize import _Recorded
    vae = _vae(family)
    failures = []
    try:
        for route in _routes(precision):
            with _Route(route):
                with _Recorded() as rec:
                    roll = vae.decode(dev(V.tiles_of(V.latent(family)))).cpu().numpy()
                big = rec.n[121] + rec.n[122]
                assert (big > 0) == (route == "big"), (route, big)         # the route really is the one it is named after
                _check(failures, precision, route, family, "roll", roll)
                if family in V.TWO_SQUARE_FAMILIES:
                    roll2 = vae.decode_latent(dev(V.latent(family, 32))).cpu().numpy()
                    _check(failures, precision, route, family, "roll", roll2, 32)
    finally:
        R.check(R.lib.rgm_set_big_tiles(1, 256))
        R.set_gemm_precision("fp32")
    assert not failures, failures


@pytest.mark.parametrize("family", V.DECODE_FAMILIES)
def test_decoder_input_gradient_on_stressed_inputs_block_by_block(family, precision):
    """decode_latent_save + decode_latent_vjp with a seeded cotangent: d(latent) of every (sample, channel, square)"""
    from gpu_util import dev
    from rgm import native as R
    vae = _vae(family)
    failures = []
    try:
        for route in _routes(precision):
            with _Route(route):
                for H in (16, 32) if family in V.TWO_SQUARE_FAMILIES else (16,):
                    roll = vae.decode_latent_save(dev(V.latent(family, H)))
                    dl = vae.decode_latent_vjp(dev(V.cotangent(H))).cpu().numpy()
                    _check(failures, precision, route, family, "roll", roll.cpu().numpy(), H)
                    _check(failures, precision, route, family, "dlat", dl, H)
    finally:
        R.check(R.lib.rgm_set_big_tiles(1, 256))
        R.set_gemm_precision("fp32")
    assert not failures, failures


@pytest.mark.parametrize("family", V.ENCODE_WEIGHTS)
def test_encoder_on_silence_corners_and_sparse_rolls_block_by_block(family, precision):
    """encode_save of the three roll families (silence; notes at the four corners of the tile: the one-sided padding of the stride-2 convs;
    a sparse roll) under base, offset and gain weights"""
    from gpu_util import dev
    from rgm import native as R
    vae = _vae(family)
    failures = []
    try:
        for route in _routes(precision):
            with _Route(route):
                mom = vae.encode_save(dev(V.rolls())).cpu().numpy()
                _check(failures, precision, route, family, "moments", mom)
    finally:
        R.check(R.lib.rgm_set_big_tiles(1, 256))
        R.set_gemm_precision("fp32")
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ exact checks, no reference
def _eight_squares(seed=81):
    return np.random.RandomState(seed).randn(1, 4, 128, 16).astype(F32)


@pytest.mark.parametrize("family", ["offset", "gain", "dead"])
def test_groupnorm_routes_agree_bit_for_bit_on_stressed_weights(family):
    """rgm_set_gn_fuse 0 / 1 / 2 (separate pass, GroupNorm inside the conv launch, its raw-row fallback) on eight squares, the smallest
    size at which every level qualifies for the in-launch GroupNorm: large group means, wide gains and a zero-variance group (rstd = 1000)
    go through the epilogue statistics, gn_finalize_tiles and gn_fixup -- the rolls must be identical."""
    from gpu_util import dev
    from rgm import native as R
    R.set_gemm_precision("bf16x3_presplit")
    prev = C.c_int(0)
    R.check(R.lib.rgm_set_gn_fuse(0, C.byref(prev)))
    try:
        assert prev.value == 1
        vae = _vae(family)
        z = dev(_eight_squares())
        n0 = R.lib.rgm_gn_fused_launches()
        apart = vae.decode_latent(z).clone()
        assert R.lib.rgm_gn_fused_launches() == n0
        R.check(R.lib.rgm_set_gn_fuse(1, None))
        R.lib.rgm_gn_fallback_tiles(1)
        fused = [vae.decode_latent(z).clone() for _ in range(2)]
        launches = R.lib.rgm_gn_fused_launches() - n0
        assert R.lib.rgm_gn_fallback_tiles(1) == 0               # an idle device: no tile ever gives up its wait
        R.check(R.lib.rgm_set_gn_fuse(2, None))
        fallback = vae.decode_latent(z).clone()
        assert R.lib.rgm_gn_fallback_tiles(1) > 0                # forced: every tile of every fused launch is counted
    finally:
        R.check(R.lib.rgm_set_gn_fuse(prev.value, None))
        R.set_gemm_precision("fp32")
    print(f"{family}: {launches} fused GroupNorm launches in two decodes of eight squares")
    assert launches >= 2
    assert bool(torch.isfinite(fused[0]).all())
    assert torch.equal(fused[0], fused[1])
    assert torch.equal(fused[0], apart), float((fused[0] - apart).abs().max())
    assert torch.equal(fallback, apart), float((fallback - apart).abs().max())


def test_a_nan_square_leaves_the_other_squares_alone(precision):
    """eight squares, the latent of one of them all NaN against all zero: every other square's roll is finite and the same bits in both
    runs (statistics, counters and scratch are per image).  In the pre-split arithmetic with the in-launch GroupNorm off and on."""
    from gpu_util import dev
    from rgm import native as R
    vae = _vae("base")
    sq = 5
    prev = C.c_int(0)
    R.check(R.lib.rgm_set_gn_fuse(1, C.byref(prev)))
    try:
        for fuse in (0, 1) if precision == "bf16x3_presplit" else (prev.value,):
            R.check(R.lib.rgm_set_gn_fuse(fuse, None))
            rolls = []
            for fill in (0.0, float("nan")):
                z = _eight_squares()
                z[:, :, 16 * sq:16 * (sq + 1)] = fill
                rolls.append(vae.decode_latent(dev(z)).cpu().numpy())
            others = np.ones(8 * 128, bool)
            others[128 * sq:128 * (sq + 1)] = False
            assert np.isfinite(rolls[1][..., others]).all(), (precision, fuse)
            assert np.array_equal(rolls[0][..., others], rolls[1][..., others]), (precision, fuse)
    finally:
        R.check(R.lib.rgm_set_gn_fuse(prev.value, None))
        R.set_gemm_precision("fp32")


def test_a_silent_cotangent_gives_exact_zeros_and_leaves_the_loud_square_alone(precision):
    """cotangent zero on all squares but one: d(latent) of the silent squares is exactly 0.0 and the loud square's d(latent) has the bits
    of the run in which every square is loud"""
    from gpu_util import dev
    vae = _vae("base")
    sq = 2
    z = dev(_eight_squares())
    cot = np.random.RandomState(82).randn(1, 3, 128, 1024).astype(F32)
    one = np.zeros_like(cot)
    one[..., 128 * sq:128 * (sq + 1)] = cot[..., 128 * sq:128 * (sq + 1)]
    vae.decode_latent_save(z)
    loud = vae.decode_latent_vjp(dev(cot)).cpu().numpy()
    lone = vae.decode_latent_vjp(dev(one)).cpu().numpy()
    rows = np.zeros(128, bool)
    rows[16 * sq:16 * (sq + 1)] = True
    assert np.isfinite(loud).all() and np.abs(loud[:, :, ~rows]).max() > 0
    assert (lone[:, :, ~rows] == 0.0).all(), float(np.abs(lone[:, :, ~rows]).max())
    assert np.array_equal(lone[:, :, rows], loud[:, :, rows]), float(np.abs(lone[:, :, rows] - loud[:, :, rows]).max())


def test_integer_stage_on_a_roll_that_leaves_the_unit_range(precision):
    """`gain` weights: the decoded roll reaches several times [-1, 1], so the clamp of the quantiser works on both sides.  The uint8 roll
    of decode_sample_for_midi equals the oracle's quantiser applied to this implementation's own float roll exactly, and every difference
    from the reference's uint8 roll sits on a quantisation boundary (gpu_util.u8_flip_report with its own tolerance)."""
    from gpu_util import dev, u8_flip_report
    from guided_diffusion.gaussian_diffusion import _decode
    from guided_diffusion.midi_util import decode_sample_for_midi
    from oracle import vae_np
    from rgm import native as R
    vae = _vae("gain")
    lat = dev(V.latent("gain", 32))
    u8 = decode_sample_for_midi(lat, embed_model=vae, scale_factor=1.0, threshold=-0.95).cpu().numpy()
    with R.gemm_precision_scope("fp32"):                 # the final decode's own arithmetic (midi_util.FINAL_DECODE_EXACT)
        roll = _decode(lat, vae, scale_factor=1.0).cpu().numpy()
    assert np.abs(roll).max() >= 3.0 and (u8 == 127).any() and (u8 == 0).any()
    assert np.array_equal(vae_np.quantise_roll(roll), u8)
    ref = V.fixtures()["gain.h32.u8"]
    n_bad, n_unexplained, dist = u8_flip_report(u8, ref, roll)
    print(f"[gain {precision}] uint8 mismatches {n_bad} / {ref.size}, unexplained {n_unexplained}, max boundary distance {dist:.1e}")
    assert n_unexplained == 0, (n_bad, n_unexplained, dist)


def test_a_square_latent_is_decoded_untransposed_like_the_reference(precision):
    """midi_util.decode_sample_for_midi transposes a latent only when it is longer than wide; a 16 x 16 latent goes to the decoder as it
    is (the one shape where it differs from _decode).  Against the reference's uint8 roll of the `base` latent."""
    from gpu_util import dev, u8_flip_report
    from guided_diffusion.midi_util import decode_sample_for_midi
    from oracle import vae_np
    vae = _vae("base")
    lat = dev(V.latent("base"))
    u8 = decode_sample_for_midi(lat, embed_model=vae, scale_factor=1.0, threshold=-0.95).cpu().numpy()
    roll = vae.decode(lat).cpu().numpy()
    assert np.array_equal(vae_np.quantise_roll(roll), u8)
    ref = V.fixtures()["base.u8"]
    n_bad, n_unexplained, dist = u8_flip_report(u8, ref, roll)
    print(f"[square {precision}] uint8 mismatches {n_bad} / {ref.size}, unexplained {n_unexplained}, max boundary distance {dist:.1e}")
    assert n_unexplained == 0, (n_bad, n_unexplained, dist)
