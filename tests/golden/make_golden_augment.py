#!/usr/bin/env python3
"""Generate tests/golden/augment.npz by IMPORTING the reference:  `python tests/golden/make_golden_augment.py`.

Runs only in the build container, like the other generators; no test imports this file or the reference.  It pins the data path of
docs/rounds/augment.md to the reference's own code:

  * guided_diffusion/pr_datasets_all.py ImageDataset.__getitem__ on uint8 excerpts written to a temporary directory, with the three draws
    injected: np.random.uniform and np.random.randint are replaced around the call (and restored), uniform answers (pr_len + 0.5) / S so
    that int(u * S) is the wanted pr_len, randint answers the start and then k;
  * key_shift on a random batch, k of both signs;
  * guided_diffusion/train_util.py get_kl_input on an identity stand-in encoder whose moments hold their own flat index, so that only the
    chunk / concat / permute / unfold order is pinned;
  * music_rule_guidance's note_density and pitch_hist of the augmented rolls.

    augment.npz
        gen                         what the excerpts' generator was started from (tests do not rebuild them: they are stored)
        u8.<S>                      (3, 3, 128, T) uint8 excerpts for S in 128, 256; T = 166, 333
        cases                       (n, 8) int32 rows: S, excerpt, pr_len, start, k, time_stretch, pitch_shift, deterministic
        roll.<i>                    the reference's item of case i, float32 (3, 128, S)
        nd.<i>, ph.<i>              its note_density / pitch_hist labels (computed on a copy, the roll is stored as __getitem__ returned it)
        ks.in, ks.k, ks.out.<j>     key_shift's input batch, the shifts and its outputs
        kl.cfg                      (m, 4) int32 rows: tiles, shift_size, recombine, B
        kl.<j>                      flat index into the moments (tiles B, 8, 16, 16) of every output element, int32; kl.raises.<j> = 1 and no
                                    map where the reference raises (a window of 128 latent rows does not fit 16 tiles' worth of rows)
The file regenerates bit for bit."""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shims  # noqa: E402

GEN = 20240611
SIZES = {128: 166, 256: 333}                             # image_size -> columns of its excerpts (about 1.3 S)


def excerpt(rng, T):
    """(3, 128, T) uint8 [velocity | onset | pedal]: held notes on about 15 % of the cells, some outside the piano range, an onset mark at
    every note's first column -- also in column 0 and in the last column --, a stepped pedal row on pitches 21 .. 108."""
    u = np.zeros((3, 128, T), dtype=np.uint8)
    while (u[0] > 0).mean() < 0.15:
        p = int(rng.randint(15, 115))
        s = int(rng.randint(0, T))
        e = min(T, s + int(rng.randint(1, 24)))
        u[0, p, s:e] = rng.randint(1, 128)
        u[1, p, s] = 127
    for p in (30, 60, 61):                               # notes that start in column 0 and in the last column, neighbours in time
        u[0, p, 0:3] = 90
        u[1, p, 0] = 127
        u[0, p, T - 1] = 77
        u[1, p, T - 1] = 127
    u[0, 64, 40:44] = 50
    u[1, 64, 40] = 127
    u[0, 64, 44:50] = 80                                  # two onsets in adjacent source columns
    u[1, 64, 41] = 127
    c = 0
    while c < T:
        w = int(rng.randint(8, 40))
        u[2, 21:109, c:c + w] = min(int(rng.randint(0, 8)) * 16 + 8, 127) if rng.rand() < 0.7 else 0
        c += w
    return u


class Draws:
    """np.random.uniform / randint answer the queued draws while active."""

    def __init__(self, S, pr_len, start, k):
        self.S, self.pr_len, self.queue = S, pr_len, [start, k]

    def uniform(self, lo, hi):
        u = (self.pr_len + 0.5) / self.S
        assert (lo, hi) == (0.95, 1.05) and int(u * self.S) == self.pr_len
        return u

    def randint(self, *a):
        return self.queue.pop(0)

    def __enter__(self):
        self.saved = (np.random.uniform, np.random.randint)
        np.random.uniform, np.random.randint = self.uniform, self.randint
        return self

    def __exit__(self, *exc):
        np.random.uniform, np.random.randint = self.saved
        return False


def cases():
    rows = []
    for S in SIZES:
        lo, hi = int(0.95 * S), int(1.05 * S)
        T = SIZES[S]
        rows += [(S, 0, lo, 0, -6, 1, 1, 0),              # stretch, the window at the excerpt's start
                 (S, 1, hi, T - hi - 1, -1, 1, 1, 0),     # compress, the last start randint can give
                 (S, 2, S, 7, 0, 1, 1, 0),                # equal
                 (S, 0, S - 3, 11, 3, 1, 1, 0),           # stretch
                 (S, 1, S + 4, 5, 0, 1, 1, 0),            # compress without a shift
                 (S, 2, S, 0, 0, 0, 0, 1)]                # deterministic=True: both augmentations off
    return np.array(rows, dtype=np.int32)


def main():
    ref_shims.install()
    from guided_diffusion import pr_datasets_all as ref
    from guided_diffusion import train_util as ref_tu
    from music_rule_guidance.rule_maps import FUNC_DICT

    rng = np.random.RandomState(GEN)
    out = {"gen": np.array([GEN], dtype=np.int64)}
    for S, T in SIZES.items():
        out[f"u8.{S}"] = np.stack([excerpt(rng, T) for _ in range(3)])
    rows = cases()
    out["cases"] = rows
    with tempfile.TemporaryDirectory() as tmp:
        for i, (S, e, pr_len, start, k, ts, ps, det) in enumerate(rows.tolist()):
            path = os.path.join(tmp, f"e_{S}_{e}.npy")
            np.save(path, out[f"u8.{S}"][e])
            ds = ref.ImageDataset([path], image_size=S, pitch_shift=bool(ps), time_stretch=bool(ts))
            with Draws(S, pr_len, start, k) as d:
                arr, _ = ds[0]
            assert len(d.queue) == (0 if ts and ps else 2), d.queue
            roll = arr.numpy().astype(np.float32)
            assert roll.shape == (3, 128, S)
            out[f"roll.{i}"] = roll
            out[f"nd.{i}"] = FUNC_DICT["note_density"](arr[None].clone()).numpy().astype(np.float32)
            out[f"ph.{i}"] = FUNC_DICT["pitch_hist"](arr[None].clone()).numpy().astype(np.float32)

    x = torch.from_numpy((rng.rand(2, 3, 128, 24) * 2 - 1).astype(np.float32))
    ks = np.array([-6, -1, 0, 3, 127, -127], dtype=np.int32)
    out["ks.in"], out["ks.k"] = x.numpy().copy(), ks
    for j, k in enumerate(ks.tolist()):
        out[f"ks.out.{j}"] = ref.key_shift(x.clone(), k).numpy()

    cfg = np.array([(1, 4, 1, 2), (9, 1, 1, 2), (12, 4, 1, 2), (2, 4, 0, 2)], dtype=np.int32)
    out["kl.cfg"] = cfg
    for j, (tiles, shift, rec, B) in enumerate(cfg.tolist()):
        class Identity:
            def encode_save(self, micro, range_fix=False):
                assert micro.shape == (tiles * B, 3, 128, 128) and range_fix is False
                return torch.arange(tiles * B * 8 * 256, dtype=torch.float32).reshape(tiles * B, 8, 16, 16)
        batch = torch.zeros(B, 3, 128, 128 * tiles)
        try:
            z = ref_tu.get_kl_input(batch, model=Identity(), scale_factor=1., recombine=bool(rec), shift_size=shift).cpu()
        except RuntimeError as e:
            print(f"get_kl_input{(tiles, shift, rec)} raises: {str(e).splitlines()[0]}")
            out[f"kl.raises.{j}"] = np.array([1], dtype=np.int32)
            continue
        out[f"kl.{j}"] = z.numpy().astype(np.int32)

    path = os.path.join(HERE, "augment.npz")
    np.savez_compressed(path, **out)                      # numpy stamps every member 1980-01-01: the file regenerates bit for bit
    size = os.path.getsize(path)
    print(f"wrote {path}: {size} bytes, {len(out)} arrays")
    assert size < (1 << 20)


if __name__ == "__main__":
    main()
