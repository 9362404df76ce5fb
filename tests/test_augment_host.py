"""CPU: the host side of the augmented training batches (docs/rounds/augment.md) -- the numpy host partner against the reference's rolls
(tests/golden/augment.npz), the two index maps against torch, the draws, the loader's order / sharding / dropped batch with a CPU stand-in
for the device call, the schedule sampler, the quartile log, the ABI entries and the flag sets.  The kernels: tests/test_gpu_augment.py."""
import csv
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT, load_golden


@pytest.fixture(scope="module")
def g():
    return load_golden("augment")


def _script(path):
    spec = importlib.util.spec_from_file_location(os.path.basename(path)[:-3] + "_cli", os.path.join(PKG, path))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_the_host_partner_equals_every_reference_roll(g):
    from guided_diffusion import pr_datasets_all as prd
    cases = g["cases"].tolist()
    assert len(cases) == 12
    kinds = set()
    for i, (S, e, pr_len, start, k, ts, ps, det) in enumerate(cases):
        got = prd.augment_excerpt(g[f"u8.{S}"][e], S, pr_len, start, k, bool(ts), bool(ps))
        assert got.dtype == np.float32 and np.array_equal(got, g[f"roll.{i}"]), i
        kinds.add("off" if not ts else ("stretch" if pr_len < S else "compress" if pr_len > S else "equal"))
    assert kinds == {"off", "stretch", "compress", "equal"} and {c[4] for c in cases} == {-6, -1, 0, 3}


def test_key_shift_equals_the_reference_for_both_signs(g):
    from guided_diffusion.pr_datasets_all import key_shift
    x = torch.from_numpy(g["ks.in"])
    ks = g["ks.k"].tolist()
    assert min(ks) < 0 < max(ks)
    for j, k in enumerate(ks):
        assert torch.equal(key_shift(x.clone(), k), torch.from_numpy(g[f"ks.out.{j}"])), k
    assert torch.equal(key_shift(x.clone(), -3), key_shift(x.clone(), 3))          # the reference's sign quirk


@pytest.mark.parametrize("S", [100, 128, 256])
def test_the_index_maps_are_torchs_and_every_source_onset_is_kept_once(S):
    import torch.nn.functional as F
    from guided_diffusion import pr_datasets_all as prd
    for pr_len in range(int(0.95 * S), int(1.05 * S) + 1):
        src = F.interpolate(torch.arange(pr_len, dtype=torch.float32).reshape(1, 1, 1, pr_len), size=(1, S), mode="nearest").reshape(-1)
        assert np.array_equal(prd.nearest_map(S, pr_len), src.numpy().astype(np.int64)), pr_len
        a = (torch.arange(S) / S * pr_len).int().numpy()
        assert np.array_equal(prd.onset_map(S, pr_len), a), pr_len
        if pr_len < S:
            first = prd.first_columns(S, pr_len)
            assert len(first) == pr_len and first[0] == 0 and (np.diff(first) > 0).all(), pr_len


def test_a_window_that_does_not_fit_raises():
    from guided_diffusion import pr_datasets_all as prd
    rng = np.random.default_rng(0)
    with pytest.raises(ValueError):
        prd.draw_augment(rng, int(0.95 * 128), 128)                             # T <= the smallest pr_len
    u8 = np.zeros((3, 128, 130), dtype=np.uint8)
    with pytest.raises(ValueError):
        prd.augment_excerpt(u8, 128, 131, 0, 0)
    with pytest.raises(ValueError):
        prd.augment_excerpt(u8, 128, 120, 11, 0)
    with pytest.raises(ValueError):
        prd.augment_excerpt(u8[:, :, :100], 128, 128, 0, 0, time_stretch=False)
    ds = prd.ImageDataset([u8[:, :, :121]], image_size=128, rng=np.random.default_rng(1))
    with pytest.raises(ValueError):
        ds[0]


def test_draws_stay_in_range_and_hit_both_ends():
    from guided_diffusion import pr_datasets_all as prd
    rng = np.random.default_rng(5)
    S, T = 128, 140
    d = np.array([prd.draw_augment(rng, T, S) for _ in range(10000)])
    lo, hi = int(0.95 * S), int(1.05 * S)
    assert d[:, 0].min() == lo and d[:, 0].max() == hi
    assert (d[:, 1] >= 0).all() and (d[:, 1] + d[:, 0] < T).all()                # randint's upper end is exclusive: start + pr_len <= T - 1
    assert (d[:, 1] == 0).any() and (d[:, 1] + d[:, 0] == T - 1).any()
    assert d[:, 2].min() == -6 and d[:, 2].max() == 6


def _dataset(tmp_path, n, T=140):
    rng = np.random.RandomState(3)
    files = []
    for i in range(n):
        u8 = np.zeros((3, 128, T), dtype=np.uint8)
        u8[0, 30 + i, 5:60] = 40 + i
        u8[1, 30 + i, 5] = 127
        u8[2, 21:109, 20:90] = rng.randint(0, 8) * 16 + 8
        path = tmp_path / f"x_{i}.npy"
        np.save(path, u8)
        files.append(str(path))
    with open(tmp_path / "data.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["midi_filename", "classes"])
        for i, p in enumerate(files):
            w.writerow([p, i % 3])
    return files, str(tmp_path / "data.csv")


def _cpu_stand_in(monkeypatch, launches):
    """load_data's two device calls on the host: the upload keeps CPU tensors, the launch is the host partner row by row."""
    from guided_diffusion import pr_datasets_all as prd

    def upload(blob, offsets, lengths, device):
        return torch.from_numpy(blob), torch.from_numpy(offsets), torch.from_numpy(lengths)

    def augment(blob, offsets, lengths, params, image_size, strict=True):
        rows = []
        for f, start, pr_len, k, flags in np.asarray(params).tolist():
            T = int(lengths[f])
            u8 = blob[int(offsets[f]):int(offsets[f]) + 384 * T].numpy().reshape(3, 128, T)
            rows.append(prd.augment_excerpt(u8, image_size, pr_len, start, k, bool(flags & prd.FLAG_STRETCH), bool(flags & prd.FLAG_SHIFT)))
        launches.append(np.asarray(params).copy())
        return torch.from_numpy(np.stack(rows)), torch.zeros(len(rows), dtype=torch.int32)

    monkeypatch.setattr(prd, "_upload", upload)
    monkeypatch.setattr(prd, "augment_rolls", augment)
    return prd


def test_load_data_deterministic_yields_the_files_in_order_and_drops_the_partial_batch(tmp_path, monkeypatch):
    files, path = _dataset(tmp_path, 7)
    launches = []
    prd = _cpu_stand_in(monkeypatch, launches)
    data = prd.load_data(data_dir=path, batch_size=3, class_cond=True, deterministic=True, image_size=128)
    seen = []
    for _ in range(4):                                                          # two epochs of two batches: file 6 never appears
        batch, out = next(data)
        assert batch.shape == (3, 3, 128, 128) and batch.dtype == torch.float32
        idx = launches[-1][:, 0].tolist()
        assert launches[-1][:, 1:].tolist() == [[0, 128, 0, 0]] * 3             # both augmentations off
        assert out["y"].tolist() == [i % 3 for i in idx] and out["y"].dtype == torch.int64
        for r, i in enumerate(idx):
            want = prd.augment_excerpt(np.load(files[i]), 128, 128, 0, 0, False, False)
            assert np.array_equal(batch[r].numpy(), want)
        seen += idx
    assert seen == [0, 1, 2, 3, 4, 5, 0, 1, 2, 3, 4, 5]


def test_load_data_shards_by_rank_and_shuffles_without_replacement(tmp_path, monkeypatch):
    files, path = _dataset(tmp_path, 9)
    launches = []
    prd = _cpu_stand_in(monkeypatch, launches)
    monkeypatch.setattr(prd, "_shard", lambda: (1, 2))
    data = prd.load_data(data_dir=path, batch_size=2, deterministic=True, image_size=128)
    got = torch.cat([next(data)[0], next(data)[0]])
    shard = files[1::2]                                                         # files 1, 3, 5, 7
    assert [int(i) for l in launches for i in l[:, 0]] == [0, 1, 2, 3] and len(shard) == 4
    for r, path_r in enumerate(shard):
        assert np.array_equal(got[r].numpy(), prd.augment_excerpt(np.load(path_r), 128, 128, 0, 0, False, False))
    with pytest.raises(ValueError):
        next(prd.load_data(data_dir=path, batch_size=5, deterministic=True, image_size=128))      # the shard holds 4 files
    launches.clear()
    monkeypatch.setattr(prd, "_shard", lambda: (0, 1))
    data = prd.load_data(data_dir=path, batch_size=4, image_size=128, rng=np.random.default_rng(2))
    for _ in range(4):
        batch, out = next(data)
        assert out == {} and batch.shape == (4, 3, 128, 128)
    epochs = [sorted(int(i) for l in launches[2 * e:2 * e + 2] for i in l[:, 0]) for e in range(2)]
    assert all(len(set(e)) == 8 and set(e) <= set(range(9)) for e in epochs)    # 8 of the 9 files, none twice
    p = np.concatenate(launches)
    assert (p[:, 4] == prd.FLAG_STRETCH | prd.FLAG_SHIFT).all() and (p[:, 1] + p[:, 2] < 140).all() and (np.abs(p[:, 3]) <= 6).all()
    assert len({tuple(r) for r in p[:, 1:4].tolist()}) > 8                     # fresh draws for every item


def test_packing_follows_the_midi_blob_rules():
    from guided_diffusion import pr_datasets_all as prd
    a = np.arange(3 * 128 * 5, dtype=np.uint8).reshape(3, 128, 5)
    b = np.full((3, 128, 3), 7, dtype=np.uint8)
    blob, offsets, lengths = prd.pack_rolls_host([a, b])
    assert offsets.dtype == np.int64 and offsets.tolist() == [0, 1920, 3072] and lengths.dtype == np.int32 and lengths.tolist() == [5, 3]
    assert blob.dtype == np.uint8 and len(blob) % 16 == 0 and 3072 + 16 <= len(blob) < 3072 + 48 and not blob[3072:].any()
    assert blob[:1920].tobytes() == a.tobytes() and blob[1920:3072].tobytes() == b.tobytes()
    for bad in ([], [a.astype(np.float32)], [a[:2]], [a[:, :, :0]]):
        with pytest.raises(ValueError):
            prd.pack_rolls_host(bad)
    assert set(prd.AUGMENT_STATUS) == set(range(5))
    for S in (1, 19, 20, 100, 128, 1024, 16384):
        assert prd.augment_capacity(S) >= int(1.05 * S) + 1 and prd.augment_capacity(S) % 16 == 0


def test_uniform_sampler_and_the_high_noise_fold():
    from guided_diffusion.resample import UniformSampler, create_named_schedule_sampler, fold_high_noise
    from guided_diffusion.script_util import create_gaussian_diffusion
    diffusion = create_gaussian_diffusion(steps=1000)
    s = create_named_schedule_sampler("uniform", diffusion)
    assert isinstance(s, UniformSampler)
    s.rng = np.random.default_rng(0)
    t, w = s.sample(4096, "cpu")
    assert t.dtype == torch.int64 and t.min() >= 0 and t.max() <= 999 and t.max() > 990 and t.min() < 10
    assert w.dtype == torch.float32 and torch.equal(w, torch.ones(4096))
    u = fold_high_noise(t.clone(), 1000)
    hi = t > 750
    assert hi.any() and torch.equal(u[hi], 1000 - t[hi]) and torch.equal(u[~hi], t[~hi]) and u.max() <= 750
    assert fold_high_noise(torch.tensor([750, 751, 999, 0])).tolist() == [750, 249, 1, 0]
    with pytest.raises(NotImplementedError, match="loss-second-moment"):
        create_named_schedule_sampler("loss-second-moment", diffusion)
    with pytest.raises(NotImplementedError):
        create_named_schedule_sampler("other", diffusion)


def test_log_loss_dict_writes_the_quartile_keys():
    from guided_diffusion import train_util
    from guided_diffusion.script_util import create_gaussian_diffusion
    diffusion = create_gaussian_diffusion(steps=1000)
    sink = {}
    ts = torch.tensor([0, 249, 250, 600, 999])
    train_util.log_loss_dict(diffusion, ts, {"val_loss": torch.tensor([1., 3., 5., 7., 9.])}, sink=sink)
    train_util.log_loss_dict(diffusion, torch.tensor([800]), {"val_loss": torch.tensor([1.])}, sink=sink)
    m = train_util.logged_means(sink)
    assert set(m) == {"val_loss", "val_loss_q0", "val_loss_q1", "val_loss_q2", "val_loss_q3"}
    assert m == {"val_loss": 3.0, "val_loss_q0": 2.0, "val_loss_q1": 5.0, "val_loss_q2": 7.0, "val_loss_q3": 5.0}
    assert train_util.parse_resume_step_from_filename("a/b/model012345.pt") == 12345
    assert train_util.parse_resume_step_from_filename("a/b/ema_0.9999_000100.pt") == 0
    assert train_util.parse_resume_step_from_filename("a/modelx.pt") == 0


def test_training_stays_out_of_scope():
    from guided_diffusion.script_util import create_gaussian_diffusion
    with pytest.raises(NotImplementedError):
        create_gaussian_diffusion(steps=1000).training_losses(None, None, None)


def test_the_header_declares_the_augment_entries_and_the_bindings_know_them():
    src = open(os.path.join(ROOT, "include", "rgm.h")).read()
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "augment.hip" in mk
    from rgm import native
    for name in ("rgm_roll_augment", "rgm_latent_windows", "rgm_latent_std", "rgm_roll_augment_capacity", "rgm_latent_windows_count",
                 "rgm_latent_std_workspace"):
        assert name + "(" in src
        assert hasattr(native.lib, name) and getattr(native.lib, name).argtypes is not None
    for S in (1, 100, 128, 16384):
        assert native.lib.rgm_roll_augment_capacity(S) == ((S + S // 16 + 15) & ~15) + 16
    assert native.lib.rgm_roll_augment_capacity(0) == 0 and native.lib.rgm_roll_augment_capacity(16385) == 0
    assert [native.lib.rgm_latent_windows_count(*c) for c in ((1, 4), (9, 1), (12, 4), (2, 0), (8, 4), (7, 1))] == [0, 2, 2, 1, 1, 0]


def test_the_new_clis_parse_their_flags_and_the_old_ones_keep_theirs():
    val = _script("scripts/classifier_val.py")
    a = val.create_argparser().parse_args([])
    for name in ("data_dir", "model", "in_channels", "noised", "no_high_noise", "batch_size", "encode_rep", "get_KL", "scale_factor",
                 "pr_image_size", "rule", "num_classes", "embed_model_name", "embed_model_ckpt", "model_path", "iterations",
                 "synthetic_weights", "gemm_precision", "seed"):
        assert hasattr(a, name), name
    assert (a.noised, a.no_high_noise, a.get_KL, a.encode_rep, a.pr_image_size, a.num_classes, a.rule) == (True, False, True, 1, 1024, 9, None)
    b = val.create_argparser().parse_args(["--rule", "note_density", "--no_high_noise", "True", "--pr_image_size", "128", "--seed", "3"])
    assert (b.rule, b.no_high_noise, b.pr_image_size, b.seed) == ("note_density", True, 128, 3)
    std = _script("compute_std.py")
    c = std.create_argparser().parse_args(["--data_dir", "x.csv"])
    assert set(vars(c)) >= {"data_dir", "image_size", "batch_size", "total_batch", "vae", "vae_path", "synthetic_weights"}
    assert (c.image_size, c.batch_size, c.total_batch, c.vae) == (1024, 32, 256, "kl/f8-all-onset")
    with pytest.raises(SystemExit):
        std.create_argparser().parse_args([])
    counts = {"sample_rule": None, "edit": None, "cfg_sample": None}
    for name in counts:
        counts[name] = vars(_script(f"scripts/{name}.py").create_argparser().parse_args([]))
        assert "pr_image_size" not in counts[name] and "encode_rep" not in counts[name]
    assert counts["sample_rule"]["gemm_precision"] == "bf16x3_presplit" and counts["sample_rule"]["synthetic_weights"] is False
