"""The forward-only pieces of the reference's guided_diffusion/train_util.py: the latent input of a classifier (get_kl_input), the
per-quartile loss log and the checkpoint-name parser.  TrainLoop, optimisers, EMA and weight gradients are out of scope
(docs/rounds/augment.md)."""
import re

import torch as th

from rgm import native as _rgm

_KV = {}                                                   # key -> [sum, count]: the running means of log_loss_dict


def get_kl_input(batch, microbatch=-1, model=None, scale_factor=1., recombine=True, shift_size=4):
    """Piano rolls (B, 3, 128, S) in [-1, 1] -> latents * scale_factor, the reference's get_kl_input: the S / 128 tiles of `microbatch` rolls
    at a time go through model.encode_save(range_fix=False) stacked tile-major, and one rgm_latent_windows launch takes the posterior
    mode, re-assembles it along time and, with recombine, cuts windows of 128 latent rows 16 * shift_size apart:
    (B W, 4, 128, 16) with W = (16 S / 128 - 128) // (16 shift_size) + 1, or (B, 4, 16 S / 128, 16) without.  Fewer than 8 tiles with
    recombine raise ValueError (the reference's unfold raises there)."""
    _rgm.require_cuda(batch)
    if batch.dim() != 4 or batch.shape[1] != 3 or batch.shape[2] != 128 or batch.shape[3] % 128 or batch.shape[3] < 128:
        raise ValueError(f"get_kl_input takes rolls (B, 3, 128, 128 n), got {tuple(batch.shape)}")
    if microbatch < 0:
        microbatch = batch.shape[0]
    tiles = batch.shape[-1] // batch.shape[-2]
    shift = int(shift_size) if recombine else 0
    if recombine and shift < 1:
        raise ValueError(f"recombine needs shift_size >= 1, got {shift_size}")
    W = int(_rgm.lib.rgm_latent_windows_count(tiles, shift))
    if W < 1:
        raise ValueError(f"recombine with {tiles} tiles and shift_size {shift_size}: a window is 128 latent rows (8 tiles)")
    full_z = []
    for i in range(0, batch.shape[0], microbatch):
        micro = batch[i:i + microbatch]
        n = micro.shape[0]
        moments = tile_moments(micro, model)
        z0 = th.empty((n * W, 4, 128 if shift else 16 * tiles, 16), dtype=th.float32, device=moments.device)
        with th.cuda.device(moments.device):
            _rgm.check(_rgm.lib.rgm_latent_windows(_rgm.ptr(moments), n, tiles, shift, float(scale_factor), _rgm.ptr(z0), None, None, None, 0,
                                                   None, 0, 0, None, _rgm.current_stream()))
        full_z.append(z0)
    return full_z[0] if len(full_z) == 1 else th.concat(full_z, dim=0)


def tile_moments(batch, model):
    """Rolls (n, 3, 128, 128 tiles) -> the encoder's moments (tiles n, 8, 16, 16), tile s of sample b in row s n + b."""
    tiles = batch.shape[-1] // batch.shape[-2]
    stacked = th.concat(th.chunk(batch, tiles, dim=-1), dim=0)
    return model.encode_save(stacked, range_fix=False).float().contiguous()


def get_noised_kl_input(batch, t, diffusion, model=None, scale_factor=1., noise=None, seed=None, offset=0):
    """get_kl_input(recombine=False) followed by diffusion.q_sample(z0, t, noise), the latter fused into the window launch
    (GaussianDiffusion.noised_latents): (z0, x_t), both (B, 4, 16 S / 128, 16)."""
    _rgm.require_cuda(batch)
    return diffusion.noised_latents(tile_moments(batch, model), t, batch.shape[0], scale_factor=scale_factor, shift_size=0, noise=noise,
                                    seed=seed, offset=offset)


def parse_resume_step_from_filename(filename):
    """path/to/modelNNNNNN.pt -> NNNNNN; 0 where the name holds no such number."""
    m = re.search(r"^(\d+)(\.|$)", filename.split("model")[-1]) if "model" in filename else None
    return int(m.group(1)) if m else 0


def log_loss_dict(diffusion, ts, losses, sink=None):
    """Running means of every loss under its key and under key_q<quartile of its timestep> -- the reference's logger.logkv_mean calls.
    sink: the dict the means are kept in (default: this module's, read by logged_means)."""
    kv = _KV if sink is None else sink
    t_host = ts.detach().cpu().numpy()
    for key, values in losses.items():
        v_host = values.detach().float().cpu().numpy()
        _mean(kv, key, float(values.float().mean().item()))
        for sub_t, sub_loss in zip(t_host, v_host):
            _mean(kv, f"{key}_q{int(4 * sub_t / diffusion.num_timesteps)}", float(sub_loss))


def _mean(kv, key, value):
    s = kv.setdefault(key, [0.0, 0])
    s[0] += value
    s[1] += 1


def logged_means(sink=None):
    return {k: s / n for k, (s, n) in (_KV if sink is None else sink).items()}
