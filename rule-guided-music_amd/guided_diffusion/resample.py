"""Schedule samplers -- the reference's guided_diffusion/resample.py as far as the forward-only paths need it: the uniform sampler.
The loss-aware sampler reweights by training losses, which are out of scope (GaussianDiffusion.training_losses raises)."""
import numpy as np
import torch as th


def create_named_schedule_sampler(name, diffusion):
    if name == "uniform":
        return UniformSampler(diffusion)
    if name == "loss-second-moment":
        raise NotImplementedError("schedule sampler 'loss-second-moment' resamples by training losses, which are out of scope here")
    raise NotImplementedError(f"unknown schedule sampler: {name}")


class ScheduleSampler:
    """A distribution over the timesteps of a diffusion process.  `rng` (numpy.random.Generator or RandomState) replaces numpy's global
    stream, which the reference draws from."""

    rng = None

    def weights(self):
        raise NotImplementedError

    def sample(self, batch_size, device):
        """(timesteps int64 (batch_size), weights float32 (batch_size)) on `device`, drawn on the host as in the reference."""
        w = np.asarray(self.weights(), dtype=np.float64)
        p = w / w.sum()
        rng = self.rng if self.rng is not None else np.random
        picks = np.asarray(rng.choice(p.size, size=(batch_size,), p=p))
        scale = 1.0 / (p.size * p[picks])
        return th.from_numpy(picks).long().to(device), th.from_numpy(scale).float().to(device)


class UniformSampler(ScheduleSampler):
    def __init__(self, diffusion, rng=None):
        self.diffusion = diffusion
        self._weights = np.ones([diffusion.num_timesteps])
        self.rng = rng

    def weights(self):
        return self._weights


def fold_high_noise(t, num_timesteps=1000, bound=750):
    """--no_high_noise of the classifier scripts: t > 750 -> 1000 - t (the decoder cannot decode noisier latents).  In place, returned."""
    hi = t > bound
    t[hi] = num_timesteps - t[hi]
    return t
