"""GPU: csrc/augment.hip (docs/rounds/augment.md) -- rgm_roll_augment against the numpy host partner (itself pinned to the reference by
tests/test_augment_host.py) and the reference's rolls, exactly; rgm_latent_windows against the reference's index map, a torch
restatement and q_sample, exactly; rgm_latent_std against numpy float64 within the bound of a float64 sum of n terms; the loader and the
two CLIs end to end."""
import csv
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import PKG, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def g():
    return load_golden("augment")


@pytest.fixture(scope="module")
def prd():
    from guided_diffusion import pr_datasets_all
    return pr_datasets_all


def _script(path):
    spec = importlib.util.spec_from_file_location(os.path.basename(path)[:-3] + "_cli", os.path.join(PKG, path))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def excerpt(seed, T, lo=21, hi=109):
    """(3, 128, T) uint8: held notes with onset marks on pitches lo .. hi - 1, onsets in the first and last column, a stepped pedal."""
    rng = np.random.RandomState(seed)
    u = np.zeros((3, 128, T), dtype=np.uint8)
    for _ in range(max(8, T // 2)):
        p, s = int(rng.randint(lo, hi)), int(rng.randint(0, T))
        e = min(T, s + int(rng.randint(1, 20)))
        u[0, p, s:e] = rng.randint(1, 256)
        u[1, p, s] = 127
    u[0, 60, 0] = u[0, 61, T - 1] = 99
    u[1, 60, 0] = u[1, 61, T - 1] = 127
    c = 0
    while c < T:
        w = int(rng.randint(5, 30))
        u[2, 21:109, c:c + w] = rng.randint(0, 256)
        c += w
    return u


def launch(prd, excerpts, params, S):
    """One launch over `excerpts` packed back to back -> (batch, status) as numpy, plus the blob check: it is only read."""
    blob, offsets, lengths = prd.pack_rolls(excerpts, DEV)
    before = blob.clone()
    out, status = prd.augment_rolls(blob, offsets, lengths, np.asarray(params, dtype=np.int32), S, strict=False)
    torch.cuda.synchronize()
    assert torch.equal(blob, before)
    return out.cpu().numpy(), status.cpu().numpy()


def host_rows(prd, excerpts, params, S):
    return np.stack([prd.augment_excerpt(excerpts[f], S, L, st, k, bool(fl & 1), bool(fl & 2)) for f, st, L, k, fl in params])


def test_the_reference_rolls_of_the_fixture(g, prd):
    cases = g["cases"].tolist()
    for S in (128, 256):
        rows = [(i, c) for i, c in enumerate(cases) if c[0] == S]
        params = [(c[1], c[3], c[2], c[4], (1 if c[5] else 0) | (2 if c[6] else 0)) for _, c in rows]
        out, status = launch(prd, list(g[f"u8.{S}"]), params, S)
        assert not status.any()
        for r, (i, _) in enumerate(rows):
            assert np.array_equal(out[r], g[f"roll.{i}"]), (S, i)


@pytest.mark.parametrize("S", [128, 100, 7])
def test_every_window_length_in_range(prd, S):
    """S = 100 and 7 take the 4-byte stores and the tail group; every pr_len the draw can give, a start and a shift that vary with it."""
    lo, hi = int(0.95 * S), int(1.05 * S)
    T = hi + 9
    ex = [excerpt(10 + S, T), excerpt(11 + S, T + 3)]
    params = []
    for L in range(max(1, lo - 2), hi + 3):
        f = L % 2
        room = ex[f].shape[2] - L
        params += [(f, (L * 7) % (room + 1), L, (L % 13) - 6, 3), (f, room, L, 0, 1)]
    out, status = launch(prd, ex, params, S)
    assert not status.any()
    assert np.array_equal(out, host_rows(prd, ex, params, S))


@pytest.mark.parametrize("B", [1, 3, 17])
def test_mixed_rows_in_one_launch(prd, B):
    S = 256
    ex = [excerpt(20, 300), excerpt(21, 333), excerpt(22, 275)]
    kinds = [(243, 3), (268, 3), (256, 3), (256, 0), (250, 1), (260, 2), (256, 2)]        # stretch, compress, equal, off, no shift, no stretch
    params = []
    for r in range(B):
        L, fl = kinds[r % len(kinds)]
        f = r % 3
        params.append((f, (r * 5) % (ex[f].shape[2] - 268), L, (r % 13) - 6, fl))
    out, status = launch(prd, ex, params, S)
    assert not status.any() and out.shape == (B, 3, 128, S)
    assert np.array_equal(out, host_rows(prd, ex, params, S))
    for r in range(B):                                                          # without the stretch flag start and pr_len are not read
        if not params[r][4] & 1:
            assert np.array_equal(out[r], prd.augment_excerpt(ex[params[r][0]], S, S, 0, params[r][3], False, bool(params[r][4] & 2)))


def test_every_shift_and_the_wrap_into_the_erased_rows(prd):
    """Notes in rows 15 .. 26 and 103 .. 114: what a shift wraps round or moves out of the piano range is erased, what it moves in appears."""
    S, T = 128, 140
    ex = [excerpt(30, T, 15, 27), excerpt(31, T, 103, 115)]
    ex[0][0, 0, :] = 200                                                        # row 0 wraps to row 127 for k = 1 and into the piano for |k| >= 20
    ex[0][1, 0, 3] = 127
    params = [(abs(k) % 2, 4, 125 if k % 3 else 131, k, 3) for k in range(-127, 128)]
    out, status = launch(prd, ex, params, S)
    assert not status.any()
    want = host_rows(prd, ex, params, S)
    assert np.array_equal(out, want)
    assert (out[:, :, :21] == -1).all() and (out[:, :, 109:] == -1).all()
    assert params[127 + 5][:3] == params[127 - 5][:3] and np.array_equal(out[127 + 5], out[127 - 5])      # k = 5 and k = -5 move the same way
    assert ex[1][0, 109:114, 4:129].any() and (out[127 + 5, 0, 104:109] > -1).any()      # rows outside the piano moved into it
    assert (out[127 + 40, 0, 88] > 1).any()                                      # row 0 of the source at pitch 128 - 40


def test_odd_byte_offsets_and_windows_that_touch_both_ends(prd):
    """Excerpts placed by hand at odd byte offsets; T = pr_len + 1 with the start at both ends; the last excerpt ends with the blob's data."""
    S = 128
    ex = [excerpt(40, 123), excerpt(41, 135), excerpt(42, 129)]
    offs, at = [], 1
    for e in ex:
        offs.append(at)
        at += e.size + 3
    total = offs[-1] + ex[-1].size
    blob = np.full((total + 15) // 16 * 16 + 16, 255, dtype=np.uint8)             # 255 around the excerpts: a read outside one shows
    blob[total:] = 0
    for e, o in zip(ex, offs):
        blob[o:o + e.size] = e.reshape(-1)
    params = [(0, 0, 122, 2, 3), (0, 1, 122, -3, 3), (1, 0, 134, 0, 3), (1, 1, 134, 5, 3), (2, 0, 128, 0, 3), (2, 1, 128, 1, 3), (2, 0, 128, 0, 0)]
    b = torch.from_numpy(blob).to(DEV)
    out, status = prd.augment_rolls(b, torch.tensor(offs + [total], dtype=torch.int64, device=DEV),
                                    torch.tensor([e.shape[2] for e in ex], dtype=torch.int32, device=DEV), np.array(params, dtype=np.int32), S,
                                    strict=False)
    assert not status.cpu().numpy().any()
    assert np.array_equal(out.cpu().numpy(), host_rows(prd, ex, params, S))
    assert torch.equal(b.cpu(), torch.from_numpy(blob))


def test_onsets_at_the_ends_and_in_adjacent_columns(prd):
    S, T = 128, 150
    u = np.zeros((3, 128, T), dtype=np.uint8)
    u[0, 50, 0:4] = 60                                                          # an onset in the first source column
    u[1, 50, 0] = 127
    u[0, 54, :] = 80                                                            # sounds in every column, no onset mark anywhere
    for L in (121, 134):                                                        # an onset in the last column of the windows that start at 5
        u[0, 52, 5 + L - 1] = 70
        u[1, 52, 5 + L - 1] = 127
    dropped = np.setdiff1d(np.arange(134), prd.nearest_map(S, 134))             # source columns the compression skips
    dropped = [int(d) for d in dropped if 2 <= d <= 128]
    assert len(dropped) >= 4
    for start, row in ((0, 70), (5, 72)):                                       # a short quiet note, then a louder one whose onset column is skipped
        for d in dropped:
            c = start + d
            u[0, row, c - 1] = 40
            u[0, row, c:c + 3] = 90
            u[1, row, c - 1:c + 1] = 127                                        # two onsets in adjacent source columns
    params = [(0, 0, 121, 0, 3), (0, 5, 121, 0, 3), (0, 0, 134, 0, 3), (0, 5, 134, 0, 3)]
    out, status = launch(prd, [u], params, S)
    assert not status.any() and np.array_equal(out, host_rows(prd, [u], params, S))
    assert (out[:, 1, 54] == -1).all()                                          # column 0 is compared with itself: never an onset
    for r, (_, start, L, _, _) in enumerate(params):
        assert out[r, 1, 50, 0] == (1 if start == 0 else -1)
        if L < S:                                                               # stretch: every source onset once, none doubled
            assert int((out[r, 1] == 1).sum()) == int((u[1, :, start:start + L] == 127).sum())
            assert out[r, 1, 52, S - 1] == (1 if start == 5 else -1)            # the last source column lands in the last output column
        else:
            row = 70 if start == 0 else 72
            src = prd.nearest_map(S, L)
            for d in dropped:
                j = int(np.searchsorted(src, d))                                # the first output column behind the skipped one
                assert src[j - 1] == d - 1 and src[j] == d + 1 and u[1, row, start + d + 1] == 0
                assert out[r, 1, row, j - 1] == 1 and out[r, 1, row, j] == 1 and out[r, 0, row, j] > out[r, 0, row, j - 1]      # the repair


def test_every_status_code_between_good_rows(prd):
    S = 128
    ex = [excerpt(50, 170), excerpt(51, 100)]
    cap = prd.augment_capacity(S)
    good = [(0, 3, 125, 2, 3), (0, 7, 133, -1, 3), (0, 0, 128, 0, 0)]
    bad = [((2, 0, 125, 0, 3), 1), ((-1, 0, 125, 0, 3), 1), ((0, 46, 125, 0, 3), 2), ((0, -1, 125, 0, 3), 2), ((1, 0, 128, 0, 0), 2),
           ((0, 0, 0, 0, 3), 3), ((0, 0, -5, 0, 3), 3), ((0, 0, cap + 1, 0, 3), 3), ((0, 0, 2 ** 31 - 1, 0, 3), 3),
           ((0, 2 ** 31 - 1, 125, 0, 3), 2), ((0, 0, 125, 128, 3), 4), ((0, 0, 125, -128, 3), 4), ((0, 0, 125, -2 ** 31, 3), 4)]
    params, want_status = [], []
    for i, (row, code) in enumerate(bad):
        params += [good[i % 3], row]
        want_status += [0, code]
    params.append(good[0])
    want_status.append(0)
    out, status = launch(prd, ex, params, S)
    assert status.tolist() == want_status
    alone = {r: launch(prd, ex, [r], S)[0][0] for r in good}
    for r, code in zip(range(len(params)), want_status):
        if code:
            assert (out[r] == -1).all()
        else:
            assert np.array_equal(out[r], alone[params[r]]) and np.array_equal(out[r], host_rows(prd, ex, [params[r]], S)[0])
    assert launch(prd, ex, [(0, 0, 125, 128, 1)], S)[1].tolist() == [0]         # without the shift flag k is not read
    assert launch(prd, ex, [(0, 0, cap, 0, 3)], S)[1].tolist() == [0]           # the capacity itself is served
    blob, offsets, lengths = prd.pack_rolls(ex, DEV)
    with pytest.raises(ValueError, match="row 1"):
        prd.augment_rolls(blob, offsets, lengths, np.array([good[0], bad[2][0], bad[5][0]], dtype=np.int32), S)
    lengths2 = lengths.clone()
    lengths2[1] = 10 ** 6                                                       # a length that leaves the blob: refused, nothing read
    out2, st2 = prd.augment_rolls(blob, offsets, lengths2, np.array([(1, 0, 125, 0, 3)], dtype=np.int32), S, strict=False)
    assert st2.tolist() == [1] and (out2 == -1).all()


def test_launches_repeat_and_a_row_does_not_depend_on_its_batch(prd):
    S = 256
    ex = [excerpt(60, 300), excerpt(61, 290)]
    params = [(r % 2, (r * 3) % 20, 243 + (r * 5) % 26, (r % 13) - 6, 3) for r in range(17)]
    blob, offsets, lengths = prd.pack_rolls(ex, DEV)
    p = np.array(params, dtype=np.int32)
    first, _ = prd.augment_rolls(blob, offsets, lengths, p, S)
    for _ in range(19):
        again, _ = prd.augment_rolls(blob, offsets, lengths, p, S)
        assert torch.equal(first, again)
    for r in (0, 8, 16):
        alone, _ = prd.augment_rolls(blob, offsets, lengths, p[r:r + 1], S)
        assert torch.equal(alone[0], first[r])


def test_the_largest_size(prd):
    """S = 16384: the LDS layout at its largest, 64 columns per thread in the rank scan, the longest windows the capacity holds."""
    S = 16384
    cap = prd.augment_capacity(S)
    ex = [excerpt(70, cap + 5)]
    params = [(0, 5, int(0.95 * S), -6, 3), (0, 0, int(1.05 * S), 3, 3), (0, 4, cap, 0, 3), (0, 1, S, 1, 3)]
    out, status = launch(prd, ex, params, S)
    assert not status.any() and np.array_equal(out, host_rows(prd, ex, params, S))


def test_size_and_pointer_errors_write_nothing(prd):
    from rgm import native as R
    S, B = 128, 2
    ex = [excerpt(80, 150)]
    blob, offsets, lengths = prd.pack_rolls(ex, DEV)
    params = torch.tensor([(0, 0, 125, 0, 3)] * B, dtype=torch.int32, device=DEV)
    out = torch.full((B, 3, 128, S), 7.0, device=DEV)
    status = torch.full((B,), 9, dtype=torch.int32, device=DEV)
    ok = dict(blob=R.ptr(blob), nbytes=blob.numel(), offsets=R.ptr(offsets), lengths=R.ptr(lengths), N=1, params=R.ptr(params), B=B, S=S,
              out=R.ptr(out), status=R.ptr(status))
    import ctypes as C
    for change in (dict(B=0), dict(B=-1), dict(S=0), dict(S=16385), dict(N=0), dict(nbytes=blob.numel() - 1), dict(nbytes=0), dict(blob=None),
                   dict(offsets=None), dict(lengths=None), dict(params=None), dict(out=None), dict(status=None),
                   dict(blob=C.c_void_p(blob.data_ptr() + 1)), dict(out=C.c_void_p(out.data_ptr() + 2))):
        a = dict(ok, **change)
        rc = R.lib.rgm_roll_augment(a["blob"], a["nbytes"], a["offsets"], a["lengths"], a["N"], a["params"], a["B"], a["S"], a["out"], a["status"],
                                    R.current_stream())
        assert rc != 0 and R.lib.rgm_last_error(), change
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (status == 9).all()
    R.check(R.lib.rgm_roll_augment(ok["blob"], ok["nbytes"], ok["offsets"], ok["lengths"], 1, ok["params"], B, S, ok["out"], ok["status"],
                                   R.current_stream()))
    assert (status == 0).all() and np.array_equal(out[1].cpu().numpy(), prd.augment_excerpt(ex[0], S, 125, 0, 0))
    mom, z0 = torch.zeros((2, 8, 16, 16), device=DEV), torch.full((2, 4, 16, 16), 7.0, device=DEV)
    for tiles, shift in ((1, 4), (0, 0), (1, -1), (7, 1)):
        assert R.lib.rgm_latent_windows(R.ptr(mom), 2, tiles, shift, 1.0, R.ptr(z0), None, None, None, 0, None, 0, 0, None, R.current_stream()) != 0
    assert R.lib.rgm_latent_windows(R.ptr(mom), 2, 1, 0, 1.0, R.ptr(z0), None, None, None, 0, None, 0, 0, R.ptr(z0), R.current_stream()) != 0
    assert R.lib.rgm_latent_std(R.ptr(mom), 16, R.ptr(z0), None, 0, R.current_stream()) != 0
    torch.cuda.synchronize()
    assert (z0 == 7.0).all()


# ---- latent windows ------------------------------------------------------------------------------------------------------------------------------
def restated_windows(moments, B, tiles, shift, recombine):
    """Step 10 of docs/rounds/augment.md in torch index arithmetic."""
    mean = moments[:, :4].reshape(tiles, B, 4, 16, 16)                          # [s, b, c, i, j]
    z = mean.permute(1, 2, 0, 4, 3).reshape(B, 4, 16 * tiles, 16)               # [b, c, 16 s + j, i]
    if not recombine:
        return z
    W = (16 * tiles - 128) // (16 * shift) + 1
    return torch.stack([z[:, :, 16 * shift * w:16 * shift * w + 128] for w in range(W)], dim=1).reshape(B * W, 4, 128, 16)


@pytest.fixture(scope="module")
def diffusion():
    from guided_diffusion.script_util import create_gaussian_diffusion
    return create_gaussian_diffusion(steps=1000)


def test_latent_windows_follow_the_reference_index_map(g, diffusion):
    rng = np.random.RandomState(0)
    for j, (tiles, shift, rec, B) in enumerate(g["kl.cfg"].tolist()):
        moments = torch.from_numpy(rng.randn(tiles * B, 8, 16, 16).astype(np.float32)).to(DEV)
        if f"kl.raises.{j}" in g:                                               # the reference's unfold raises: refused here too
            with pytest.raises(ValueError):
                diffusion.noised_latents(moments, None, B, shift_size=shift if rec else 0)
            continue
        z0, x_t = diffusion.noised_latents(moments, None, B, shift_size=shift if rec else 0)
        assert x_t is None
        idx = torch.from_numpy(g[f"kl.{j}"].astype(np.int64)).to(DEV)
        assert z0.shape == idx.shape and torch.equal(z0, moments.flatten()[idx])
        assert torch.equal(z0, restated_windows(moments, B, tiles, shift, bool(rec)))
        zs, _ = diffusion.noised_latents(moments, None, B, scale_factor=0.37, shift_size=shift if rec else 0)
        assert torch.equal(zs, z0 * 0.37)


def test_noised_latents_equal_q_sample_bit_for_bit(diffusion):
    from rgm import native as R
    rng = np.random.RandomState(1)
    for tiles, shift, B in ((9, 1, 2), (2, 0, 3), (1, 0, 1)):
        moments = torch.from_numpy(rng.randn(tiles * B, 8, 16, 16).astype(np.float32)).to(DEV)
        z0, _ = diffusion.noised_latents(moments, None, B, scale_factor=1.7, shift_size=shift)
        rows = z0.shape[0]
        t = torch.from_numpy(rng.randint(0, 1000, size=rows)).to(DEV)
        t[0], t[-1] = 999, 0
        noise = torch.from_numpy(rng.randn(*z0.shape).astype(np.float32)).to(DEV)
        z1, x_t = diffusion.noised_latents(moments, t, B, scale_factor=1.7, shift_size=shift, noise=noise)
        assert torch.equal(z1, z0) and torch.equal(x_t, diffusion.q_sample(z0, t, noise=noise))
        seed, offset = 1234567, 5                                               # an offset that is no multiple of 4: blocks straddle
        drawn = torch.empty_like(z0)
        R.check(R.lib.rgm_randn(R.ptr(drawn), drawn.numel(), seed, offset, R.current_stream()))
        _, x_p = diffusion.noised_latents(moments, t, B, scale_factor=1.7, shift_size=shift, seed=seed, offset=offset)
        _, x_i = diffusion.noised_latents(moments, t, B, scale_factor=1.7, shift_size=shift, noise=drawn)
        assert torch.equal(x_p, x_i) and not torch.equal(x_p, x_t)


@pytest.fixture(scope="module")
def vae():
    from load_utils import load_model
    from rgm import synth
    m = load_model("kl/f8-all-onset", None)
    m.load_state_dict(synth.vae_state_dict(2, device=DEV, encoder=True))
    return m.to(DEV).eval()


def test_get_kl_input_equals_encode(prd, vae):
    from guided_diffusion.gaussian_diffusion import _encode
    from guided_diffusion.train_util import get_kl_input
    ex = [excerpt(90, 300), excerpt(91, 300)]
    batch, _ = prd.augment_rolls(*prd.pack_rolls(ex, DEV), np.array([(0, 3, 250, 2, 3), (1, 0, 262, -1, 3)], dtype=np.int32), 256)
    for s in (1.0, 0.8125, 1.37):
        z = get_kl_input(batch, model=vae, scale_factor=s, recombine=False)
        assert z.shape == (2, 4, 32, 16) and torch.equal(z, _encode(batch, vae, s).contiguous())
    assert torch.equal(get_kl_input(batch, microbatch=1, model=vae, scale_factor=1.37, recombine=False), z)
    with pytest.raises(ValueError):
        get_kl_input(batch, model=vae)                                          # 2 tiles cannot hold a window of 128 latent rows


# ---- latent scale ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1024, 131072, 131073])
def test_latent_std_against_numpy_float64(n):
    std_cli = _script("compute_std.py")
    x = (np.random.RandomState(n).randn(n) * 1.3 + 0.4).astype(np.float32)
    x64 = x.astype(np.float64)
    want = (x64.mean(), x64.std(ddof=1), 1.0 / x64.std(ddof=1))
    assert abs(want[0]) <= want[1]
    xd = torch.from_numpy(x).to(DEV)
    got = std_cli.latent_std(xd)
    bound = n * 2.0 ** -52                                                      # a float64 sum of n terms
    for a, b in zip(got, want):
        print(f"n = {n}: {a!r} against {b!r}, relative error {abs(a - b) / abs(b):.3e}, bound {bound:.3e}")
        assert abs(a - b) <= bound * abs(b)
    for _ in range(19):
        assert std_cli.latent_std(xd) == got
    assert abs(got[1] - float(torch.from_numpy(x64).std())) <= bound * got[1]


def test_latent_std_of_one_value_is_nan():
    std_cli = _script("compute_std.py")
    mean, std, inv = std_cli.latent_std(torch.tensor([2.5], device=DEV))
    assert mean == 2.5 and np.isnan(std) and np.isnan(inv)


# ---- the loader and the CLIs ----------------------------------------------------------------------------------------------------------------
def _dataset(tmp_path, n, T):
    files = []
    for i in range(n):
        path = tmp_path / f"x_{i}.npy"
        u = excerpt(100 + i, T)
        u[0, 40, 10:60] = 2                                                     # a note below the rules' -0.95 threshold, in every window
        np.save(path, u)
        files.append(str(path))
    with open(tmp_path / "data.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["midi_filename", "classes"])
        for i, p in enumerate(files):
            w.writerow([p, i % 3])
    return files, str(tmp_path / "data.csv")


def test_load_data_labels_the_batch_it_returns(prd, tmp_path, monkeypatch):
    from music_rule_guidance.rule_maps import FUNC_DICT
    files, path = _dataset(tmp_path, 5, 170)
    seen = []
    real = prd.augment_rolls

    def recording(blob, offsets, lengths, params, image_size, strict=True):
        seen.append(np.asarray(params).copy())
        return real(blob, offsets, lengths, params, image_size, strict)

    monkeypatch.setattr(prd, "augment_rolls", recording)
    data = prd.load_data(data_dir=path, batch_size=2, class_cond=True, image_size=128, rule="note_density", rng=np.random.default_rng(4))
    for _ in range(3):
        batch, out = next(data)
        p = seen[-1]
        assert batch.is_cuda and batch.shape == (2, 3, 128, 128) and set(out) == {"note_density", "y"}
        host = torch.from_numpy(host_rows(prd, [np.load(f) for f in files], p.tolist(), 128)).to(DEV)
        raw = host.clone()
        label = FUNC_DICT["note_density"](host)                                 # thresholds channel 0 of `host` in place
        assert torch.equal(out["note_density"], label) and torch.equal(batch, host)
        assert not torch.equal(raw, host)                                       # the batch carries the rule's in-place threshold
        assert out["y"].tolist() == [int(i) % 3 for i in p[:, 0]]
    other = prd.load_data(data_dir=path, batch_size=2, image_size=128, rng=np.random.default_rng(4), resident=False)
    n0 = len(seen)
    b2, o2 = next(other)
    assert o2 == {} and seen[n0][:, 0].tolist() == [0, 1] and seen[n0][:, 1:].tolist() == seen[0][:, 1:].tolist()


def test_classifier_val_reproduces_its_loss(prd, tmp_path):
    from guided_diffusion import train_util
    from guided_diffusion.resample import create_named_schedule_sampler
    cli = _script("scripts/classifier_val.py")
    files, path = _dataset(tmp_path, 6, 170)
    argv = ["--data_dir", path, "--model", "DiTRotary-XS/8-cls", "--rule", "note_density", "--num_classes", "2", "--pr_image_size", "128",
            "--batch_size", "2", "--iterations", "2", "--synthetic_weights", "True", "--gemm_precision", "fp32", "--seed", "11",
            "--scale_factor", "1.25"]
    cli.main(argv + ["--outdir", str(tmp_path / "a")])
    cli.main(argv + ["--outdir", str(tmp_path / "b")])
    text = open(tmp_path / "a" / "val_results.csv").read()
    assert text == open(tmp_path / "b" / "val_results.csv").read()              # a second run is identical
    rows = list(csv.DictReader(open(tmp_path / "a" / "val_results.csv")))
    assert len(rows) == 2 and all(np.isfinite(float(r["val_loss"])) for r in rows)
    args = cli.create_argparser().parse_args(argv)
    torch.manual_seed(11)
    model, diffusion, vae_ = cli.build(args, torch.device(DEV, torch.cuda.current_device()))
    sampler = create_named_schedule_sampler("uniform", diffusion)
    sampler.rng = np.random.default_rng([11, 1])
    data = prd.load_data(data_dir=path, batch_size=2, image_size=128, rule="note_density", rng=np.random.default_rng([11, 0]))
    with torch.no_grad():
        for r in rows:
            batch, extra = next(data)
            z = train_util.get_kl_input(batch, model=vae_, scale_factor=1.25, recombine=False)
            t, _ = sampler.sample(2, DEV)
            assert r["t"] == " ".join(str(int(v)) for v in t.cpu())
            x = diffusion.q_sample(z, t)
            logits = model(x, t)
            loss = torch.nn.functional.mse_loss(logits, extra["note_density"], reduction="none").mean(dim=-1)
            assert float(r["val_loss"]) == float(loss.mean().item())
    import json
    meta = json.load(open(tmp_path / "a" / "run_metadata.json"))
    assert "val_loss" in meta["means"] and any(k.startswith("val_loss_q") for k in meta["means"])


def test_compute_std_prints_the_reciprocal_of_the_latents_std(tmp_path, capsys):
    cli = _script("compute_std.py")
    files, path = _dataset(tmp_path, 4, 170)
    argv = ["--data_dir", path, "--image_size", "128", "--batch_size", "2", "--total_batch", "2", "--synthetic_weights", "True", "--seed", "3",
            "--outdir", str(tmp_path / "o")]
    meta = cli.main(argv)
    printed = [l for l in capsys.readouterr().out.splitlines() if l.startswith("scale_factor: ")]
    assert len(printed) == 1 and float(printed[0].split()[1]) == meta["scale_factor"]
    latents = cli.collect_latents(cli.create_argparser().parse_args(argv), torch.device(DEV, torch.cuda.current_device()))
    x64 = latents.cpu().numpy().astype(np.float64).reshape(-1)
    n = x64.size
    assert n == 2 * 2 * 4 * 16 * 16 == meta["elements"]
    want = 1.0 / x64.std(ddof=1)
    assert abs(meta["scale_factor"] - want) <= n * 2.0 ** -52 * want
    import json
    assert json.load(open(tmp_path / "o" / "run_metadata.json"))["scale_factor"] == meta["scale_factor"]
