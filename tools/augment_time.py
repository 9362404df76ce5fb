"""What building augmented batches on the device costs (docs/rounds/augment.md): rgm_roll_augment alone by HIP events (warm, the minimum of
5 rounds of 10 calls) for (B, S) = (16, 128), (16, 1024), (64, 1024), (16, 2560) with random draws, next to the bytes the launch must
move (12 * 128 * S * B written, at most 3 * 128 * 1.05 * S * B read) and the GB/s that makes; the whole next(load_data(...)) with the
note_density rule by the wall clock against the host partner -- ImageDataset item by item plus the same rule call -- IN THE SAME PROCESS;
and get_kl_input at (16, 1024) next to the bare encode_save of the same tiles, with the window launch alone by events.  The device batch
is compared with the host partner's while at it.  The figures are reported, not asserted.  Writes profiles/augment_time.json and prints
it as one line.

    python tools/augment_time.py [--out profiles/augment_time.json]"""
import argparse
import csv
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rule-guided-music_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = ((16, 128), (16, 1024), (64, 1024), (16, 2560))


def events_us(fn, iters=10, rounds=5, warmup=3):
    for _ in range(warmup):
        fn()
    best = float("inf")
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / iters * 1e3)
    return round(best, 2)


def wall_ms(fn, rounds=5, warmup=1):
    for _ in range(warmup):
        fn()
    best = float("inf")
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return round(best, 3)


def excerpt(rng, T):
    u = np.zeros((3, 128, T), dtype=np.uint8)
    while (u[0] > 0).mean() < 0.15:
        p, s = int(rng.integers(21, 109)), int(rng.integers(0, T))
        e = min(T, s + int(rng.integers(4, 60)))
        u[0, p, s:e] = rng.integers(1, 128)
        u[1, p, s] = 127
    c = 0
    while c < T:
        w = int(rng.integers(20, 120))
        u[2, 21:109, c:c + w] = int(rng.integers(0, 8)) * 16 + 8
        c += w
    return u


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_time.json"))
    args = ap.parse_args()
    from guided_diffusion import pr_datasets_all as prd
    from guided_diffusion import train_util
    from load_utils import load_model
    from music_rule_guidance.rule_maps import FUNC_DICT
    from rgm import native as R
    from rgm import synth
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"device": torch.cuda.get_device_name(0), "kernel": [], "loader": [], "latents": {}}
    rng = np.random.default_rng(0)
    for B, S in SHAPES:
        T = int(1.3 * S)
        ex = [excerpt(rng, T) for _ in range(min(B, 16))]
        blob, offsets, lengths = prd.pack_rolls(ex, dev)
        params = np.array([(r % len(ex),) + tuple(np.array(prd.draw_augment(rng, T, S))[[1, 0, 2]]) + (3,) for r in range(B)], dtype=np.int32)
        p = torch.from_numpy(params).to(dev)
        out = torch.empty((B, 3, 128, S), dtype=torch.float32, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)

        def call():
            R.check(R.lib.rgm_roll_augment(R.ptr(blob), blob.numel(), R.ptr(offsets), R.ptr(lengths), len(ex), R.ptr(p), B, S, R.ptr(out),
                                           R.ptr(status), R.current_stream()))
        us = events_us(call)
        want = np.stack([prd.augment_excerpt(ex[f], S, L, st, k) for f, st, L, k, _ in params.tolist()])
        written, read = 12 * 128 * S * B, int(params[:, 2].sum()) * 3 * 88
        res["kernel"].append({"B": B, "S": S, "us": us, "bytes_written": written, "bytes_read": read,
                              "GBps": round((written + read) / us / 1e3, 1), "equal_to_host_partner": bool(np.array_equal(out.cpu().numpy(), want)),
                              "status_ok": not bool(status.any())})

    with tempfile.TemporaryDirectory() as tmp:
        for B, S in ((16, 1024), (16, 2560)):
            T = int(1.3 * S)
            files = []
            for i in range(2 * B):
                files.append(os.path.join(tmp, f"e_{S}_{i}.npy"))
                np.save(files[-1], excerpt(rng, T))
            path = os.path.join(tmp, f"d_{S}.csv")
            with open(path, "w", newline="") as f:
                w = csv.writer(f)
                w.writerow(["midi_filename", "classes"])
                w.writerows([(p_, 0) for p_ in files])
            data = prd.load_data(data_dir=path, batch_size=B, image_size=S, rule="note_density", device=dev, rng=np.random.default_rng(1))
            ds = prd.ImageDataset(files, image_size=S, rng=np.random.default_rng(1))

            def host_batch():
                rolls = torch.from_numpy(np.stack([ds[i % len(files)][0] for i in range(B)])).to(dev)
                return rolls, FUNC_DICT["note_density"](rolls)
            res["loader"].append({"B": B, "S": S, "device_ms": wall_ms(lambda: next(data)), "host_partner_ms": wall_ms(host_batch, rounds=3)})

    vae = load_model("kl/f8-all-onset", None)
    vae.load_state_dict(synth.vae_state_dict(2, device=dev, encoder=True))
    vae.to(dev).eval()
    B, S = 16, 1024
    ex = [excerpt(rng, int(1.3 * S)) for _ in range(B)]
    params = np.array([(r,) + tuple(np.array(prd.draw_augment(rng, int(1.3 * S), S))[[1, 0, 2]]) + (3,) for r in range(B)], dtype=np.int32)
    batch, _ = prd.augment_rolls(*prd.pack_rolls(ex, dev), params, S)
    tiles = torch.concat(torch.chunk(batch, S // 128, dim=-1), dim=0).contiguous()
    for name in ("fp32", "bf16x3_presplit"):
        R.set_gemm_precision(name)
        with torch.no_grad():
            res["latents"][name] = {"B": B, "S": S, "encode_save_ms": wall_ms(lambda: vae.encode_save(tiles, range_fix=False)),
                                    "get_kl_input_ms": wall_ms(lambda: train_util.get_kl_input(batch, model=vae, recombine=False)),
                                    "get_kl_input_recombined_ms": wall_ms(lambda: train_util.get_kl_input(batch, model=vae, recombine=True))}
    R.set_gemm_precision("fp32")
    from guided_diffusion.script_util import create_gaussian_diffusion
    diffusion = create_gaussian_diffusion(steps=1000)
    moments = vae.encode_save(tiles, range_fix=False)
    t = torch.randint(0, 1000, (B,), device=dev)
    res["latents"]["window_launch_us"] = events_us(lambda: diffusion.noised_latents(moments, None, B))
    res["latents"]["window_and_noise_launch_us"] = events_us(lambda: diffusion.noised_latents(moments, t, B, seed=1, offset=0))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
