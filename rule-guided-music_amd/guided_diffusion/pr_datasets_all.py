"""Augmented piano-roll batches -- the reference's guided_diffusion/pr_datasets_all.py (load_data, ImageDataset, key_shift) with the
batch built on the device (docs/rounds/augment.md).

The reference augments item by item in DataLoader workers: scale, a random window, F.interpolate with an onset repair, key_shift,
piano_like, the rule label.  Here the uint8 excerpts of a shard are packed into one device blob and csrc/augment.hip writes the whole
float32 batch in one launch from three integers per item (pr_len, start, k) drawn on the host.

  augment_excerpt   the numpy host partner of the kernel: a closed-form restatement of ImageDataset.__getitem__, equal to it bit for bit
  ImageDataset      host, numpy: the reference's constructor, draws from an injectable numpy.random.Generator
  pack_rolls, augment_rolls, load_data: the device path

Quirk kept: key_shift's k < 0 branch slices with -k, so a negative k moves the rows the same way as a positive one
(new[p] = old[(p + |k|) mod 128]); what wraps round lands outside the piano range and is erased by piano_like."""
import csv

import numpy as np
import torch

from music_rule_guidance import music_rules
from music_rule_guidance.rule_maps import FUNC_DICT
from rgm import native as _rgm

MIN_PIANO, MAX_PIANO = 21, 108
MAX_IMAGE_SIZE = 16384
FLAG_STRETCH, FLAG_SHIFT = 1, 2
AUGMENT_STATUS = {0: "accepted", 1: "file index out of range, or the excerpt lies outside the blob", 2: "window outside the excerpt",
                  3: "pr_len < 1 or beyond the kernel's capacity", 4: "|k| > 127"}


def augment_capacity(image_size):
    """Source columns a row may ask for: 1.0625 image_size rounded up to 16, plus 16 (0 outside 1 .. MAX_IMAGE_SIZE)."""
    return int(_rgm.lib.rgm_roll_augment_capacity(int(image_size)))


def key_shift(x, k):
    """(batch, 3, pitch, time): pitch rows of the velocity and onset channels rolled by |k| (the reference's k < 0 branch slices with -k),
    the pedal left alone, then piano_like -- in place on the concatenated copy, like the reference."""
    shifted = torch.roll(x[:, :2, :, :], -abs(int(k)), dims=2) if k != 0 else x[:, :2, :, :]
    return music_rules.piano_like(torch.cat((shifted, x[:, 2:, :, :]), dim=1))


def nearest_map(image_size, pr_len):
    """torch's `nearest` source column of every output column: min(int(floorf(j * (float(pr_len) / float(S)))), pr_len - 1), float32."""
    scale = np.float32(pr_len) / np.float32(image_size)
    src = np.floor(np.arange(image_size, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(src, pr_len - 1)


def onset_map(image_size, pr_len):
    """(arange(S) / S * pr_len).int() of the reference's stretch branch, float32."""
    return ((np.arange(image_size, dtype=np.float32) / np.float32(image_size)) * np.float32(pr_len)).astype(np.int32)


def first_columns(image_size, pr_len):
    """Output columns that take a source onset column under stretch: column 0 and every column whose onset_map differs from its left
    neighbour's.  Column number r of them takes source column r."""
    a = onset_map(image_size, pr_len)
    return np.concatenate(([0], np.nonzero(np.diff(a))[0] + 1))


def augment_excerpt(u8, image_size, pr_len, start, k, time_stretch=True, pitch_shift=True):
    """One uint8 excerpt (3, 128, T) [velocity | onset | pedal] -> float32 (3, 128, image_size): steps 1-7 of docs/rounds/augment.md, the
    reference's ImageDataset.__getitem__ with its three draws given."""
    u8 = np.asarray(u8)
    if u8.ndim != 3 or u8.shape[:2] != (3, 128):
        raise ValueError(f"an excerpt is (3, 128, T), got {u8.shape}")
    S, T = int(image_size), u8.shape[-1]
    x = u8.astype(np.float32) / np.float32(63.5) - np.float32(1)
    if time_stretch:
        if not (pr_len >= 1 and 0 <= start and start + pr_len <= T):
            raise ValueError(f"window [{start}, {start} + {pr_len}) outside an excerpt of {T} columns")
        x = x[:, :, start:start + pr_len]
        if pr_len < S:
            src, ind = nearest_map(S, pr_len), first_columns(S, pr_len)
            assert len(ind) == pr_len, f"{len(ind)} first columns for pr_len = {pr_len}, image_size = {S}"
            onset = np.full((128, S), -1, dtype=np.float32)
            onset[:, ind] = x[1]
            x = np.stack((x[0][:, src], onset, x[2][:, src]))
        elif pr_len > S:
            x = x[:, :, nearest_map(S, pr_len)]
            rise = np.zeros((128, S), dtype=bool)
            rise[:, 1:] = x[0][:, 1:] > x[0][:, :-1]
            x[1][rise] = 1
    else:
        if S > T:
            raise ValueError(f"an excerpt of {T} columns is shorter than image_size = {S}")
        x = x[:, :, :S]
    x = np.ascontiguousarray(x, dtype=np.float32).copy()
    if pitch_shift and k != 0:
        x[:2] = np.roll(x[:2], -(abs(int(k)) % 128), axis=1)
    x[:, :MIN_PIANO, :] = -1
    x[:, MAX_PIANO + 1:, :] = -1
    return x


def draw_augment(rng, T, image_size):
    """The reference's three draws from a numpy.random.Generator: pr_len = int(U(0.95, 1.05) image_size), start uniform in [0, T - pr_len),
    k uniform in -6 .. 6.  T <= pr_len raises ValueError, as numpy's randint does in the reference."""
    pr_len = int(rng.uniform(0.95, 1.05) * image_size)
    if T - pr_len <= 0:
        raise ValueError(f"an excerpt of {T} columns cannot hold a window of {pr_len} (randint needs T > pr_len)")
    start = int(rng.integers(0, T - pr_len))
    k = int(rng.integers(-6, 7))
    return pr_len, start, k


def _label(rule, batch, out_dict):
    if rule is None:
        return
    if "chord" in rule:                                   # chord and key jointly
        chord, key, _ = FUNC_DICT[rule](batch, return_key=True)
        out_dict["chord"] = chord
        out_dict["key"] = torch.as_tensor(np.array(key, dtype=np.int64))
    else:
        out_dict[rule] = FUNC_DICT[rule](batch)


class ImageDataset:
    """The reference's dataset on the host in numpy: item idx -> (float32 (3, 128, image_size), out_dict).  Draws come from `rng`
    (numpy.random.Generator).  The rule label is FUNC_DICT[rule] of the one-item batch, so it needs what that rule needs."""

    def __init__(self, image_paths, classes=None, rule=None, shard=0, num_shards=1, image_size=1024, pitch_shift=True, time_stretch=True,
                 rng=None):
        self.local_images = image_paths[shard:][::num_shards]
        self.local_classes = None if classes is None else classes[shard:][::num_shards]
        self.rule = rule
        self.pitch_shift = pitch_shift
        self.time_stretch = time_stretch
        self.image_size = image_size
        self.rng = rng if rng is not None else np.random.default_rng()

    def __len__(self):
        return len(self.local_images)

    def draw(self, T):
        """(pr_len, start, k) in the reference's draw order; a switched-off augmentation draws nothing."""
        pr_len, start, k = self.image_size, 0, 0
        if self.time_stretch:
            pr_len = int(self.rng.uniform(0.95, 1.05) * self.image_size)
            if T - pr_len <= 0:
                raise ValueError(f"an excerpt of {T} columns cannot hold a window of {pr_len} (randint needs T > pr_len)")
            start = int(self.rng.integers(0, T - pr_len))
        if self.pitch_shift:
            k = int(self.rng.integers(-6, 7))
        return pr_len, start, k

    def __getitem__(self, idx):
        item = self.local_images[idx]
        u8 = np.load(item) if isinstance(item, (str, bytes)) or hasattr(item, "__fspath__") else np.asarray(item)
        pr_len, start, k = self.draw(u8.shape[-1])
        arr = augment_excerpt(u8, self.image_size, pr_len, start, k, self.time_stretch, self.pitch_shift)
        out_dict = {}
        if self.rule is not None:
            batch = torch.from_numpy(arr)[None]
            _label(self.rule, batch, out_dict)
            arr = batch[0].numpy()                        # the rule's in-place writes reach the item, as in the reference
        if self.local_classes is not None:
            out_dict["y"] = np.array(self.local_classes[idx], dtype=np.int64)
        return arr, out_dict


def pack_rolls_host(paths_or_arrays):
    """uint8 excerpts (3, 128, T_i), as .npy paths or arrays -> (blob, offsets, lengths) on the host: the excerpts back to back in a uint8
    array padded with zeros to a multiple of 16 plus 16 (the rule of midi_util.pack_midi_files), N + 1 int64 byte offsets, N int32
    column counts."""
    arrs = []
    for a in paths_or_arrays:
        a = np.load(a) if isinstance(a, (str, bytes)) or hasattr(a, "__fspath__") else np.asarray(a)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[:2] != (3, 128) or a.shape[2] < 1:
            raise ValueError(f"an excerpt is a uint8 array (3, 128, T), got {a.dtype} {a.shape}")
        arrs.append(np.ascontiguousarray(a))
    if not arrs:
        raise ValueError("no excerpts to pack")
    lengths = np.array([a.shape[2] for a in arrs], dtype=np.int32)
    offsets = np.zeros(len(arrs) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(384 * lengths.astype(np.int64))
    total = int(offsets[-1])
    blob = np.zeros((total + 15) // 16 * 16 + 16, dtype=np.uint8)
    for a, o in zip(arrs, offsets[:-1]):
        blob[o:o + a.size] = a.reshape(-1)
    return blob, offsets, lengths


def pack_rolls(paths_or_arrays, device=None):
    """pack_rolls_host, uploaded: (blob uint8, offsets int64 (N + 1), lengths int32 (N)) on the device.  One copy each."""
    return _upload(*pack_rolls_host(paths_or_arrays), device)


def augment_rolls(blob, offsets, lengths, params, image_size, strict=True):
    """One rgm_roll_augment launch: params (B, 5) int32 rows (file, start, pr_len, k, flags; flags = FLAG_STRETCH | FLAG_SHIFT) ->
    (batch (B, 3, 128, image_size) float32, status (B) int32), both on the blob's device.  A refused row (AUGMENT_STATUS) is -1 throughout;
    strict reads the status back and raises ValueError naming the first refused row."""
    _rgm.require_cuda(blob, offsets, lengths)
    if blob.dtype != torch.uint8 or offsets.dtype != torch.int64 or lengths.dtype != torch.int32:
        raise ValueError("augment_rolls takes what pack_rolls returns: a uint8 blob, int64 offsets, int32 lengths")
    dev = blob.device
    params = torch.as_tensor(params, dtype=torch.int32).to(dev).contiguous()
    if params.dim() != 2 or params.shape[1] != 5 or params.shape[0] < 1:
        raise ValueError(f"params are (B, 5) rows (file, start, pr_len, k, flags), got {tuple(params.shape)}")
    B, N, S = params.shape[0], lengths.shape[0], int(image_size)
    if offsets.shape[0] != N + 1:
        raise ValueError(f"{N} lengths need {N + 1} offsets, got {offsets.shape[0]}")
    out = torch.empty((B, 3, 128, S), dtype=torch.float32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _rgm.check(_rgm.lib.rgm_roll_augment(_rgm.ptr(blob), blob.numel(), _rgm.ptr(offsets), _rgm.ptr(lengths), N, _rgm.ptr(params), B, S,
                                             _rgm.ptr(out), _rgm.ptr(status), _rgm.current_stream()))
    if strict:
        bad = torch.nonzero(status).flatten().cpu().numpy()
        if len(bad):
            code = int(status[int(bad[0])])
            raise ValueError(f"row {int(bad[0])}: refused by the augmentation kernel, status {code} ({AUGMENT_STATUS.get(code, '?')})")
    return out, status


def _shard():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def load_data(*, data_dir, batch_size, class_cond=False, deterministic=False, image_size=1024, rule=None, device=None, rng=None,
              resident=True):
    """The reference's generator of (batch, out_dict) over the csv `data_dir` (columns midi_filename, and classes with class_cond).

    The rank's shard (files[rank::world] of torch.distributed when initialised) is packed on the device once (resident=False: only the
    files of each batch); every batch is one rgm_roll_augment launch plus the rule call, with no host read.  An epoch visits the shard in
    a fresh permutation drawn from `rng` (numpy.random.Generator), the last partial batch is dropped; deterministic=True visits the files in
    order with both augmentations off.  out_dict: the rule's label under its name (`chord` and `key` for a chord rule), `y` with class_cond.
    batch is (batch_size, 3, 128, image_size) float32 on the device, after the rule's in-place writes."""
    with open(data_dir, newline="") as f:
        rows = list(csv.DictReader(f))
    all_files = [r["midi_filename"] for r in rows]
    classes = [int(r["classes"]) for r in rows] if class_cond else None
    rank, world = _shard()
    files = all_files[rank:][::world]
    classes = None if classes is None else classes[rank:][::world]
    S = int(image_size)
    if not 1 <= S <= MAX_IMAGE_SIZE:
        raise ValueError(f"image_size = {S}: the augmentation kernel serves 1 .. {MAX_IMAGE_SIZE}")
    if batch_size < 1 or len(files) < batch_size:
        raise ValueError(f"a shard of {len(files)} files gives no batch of {batch_size}")
    rng = rng if rng is not None else np.random.default_rng()
    drawer = ImageDataset(files, image_size=S, pitch_shift=not deterministic, time_stretch=not deterministic, rng=rng)
    flags = 0 if deterministic else FLAG_STRETCH | FLAG_SHIFT
    packed = lengths_h = None
    if resident:
        blob_h, offsets_h, lengths_h = pack_rolls_host(files)
        packed = _upload(blob_h, offsets_h, lengths_h, device)
    y_all = None if classes is None else np.asarray(classes, dtype=np.int64)
    while True:
        order = np.arange(len(files)) if deterministic else rng.permutation(len(files))
        for b0 in range(0, len(files) - batch_size + 1, batch_size):
            idx = order[b0:b0 + batch_size]
            if resident:
                local, lens, dev_arrays = idx, lengths_h[idx], packed
            else:
                blob_h, offsets_h, lens = pack_rolls_host([files[i] for i in idx])
                local, dev_arrays = np.arange(batch_size), _upload(blob_h, offsets_h, lens, device)
            params = np.zeros((batch_size, 5), dtype=np.int32)
            for r in range(batch_size):
                T = int(lens[r])
                if deterministic and T < S:
                    raise ValueError(f"{files[idx[r]]}: {T} columns, shorter than image_size = {S}")
                pr_len, start, k = drawer.draw(T)
                params[r] = (local[r], start, pr_len, k, flags)
            batch, _ = augment_rolls(*dev_arrays, params, S, strict=False)     # the draws were checked against T on the host
            out_dict = {}
            _label(rule, batch, out_dict)
            if y_all is not None:
                out_dict["y"] = torch.from_numpy(y_all[idx]).to(batch.device)
            yield batch, out_dict


def _upload(blob_h, offsets_h, lengths_h, device):
    if not torch.cuda.is_available():
        raise _rgm.RgmError("excerpts are packed for, and batches built on, a HIP device (no CPU fallback in the product path)")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    return torch.from_numpy(blob_h).to(dev), torch.from_numpy(offsets_h).to(dev), torch.from_numpy(lengths_h).to(dev)
