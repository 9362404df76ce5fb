"""What writing MIDI files on the device costs (docs/rounds/midi.md): rgm_midi_measure and rgm_midi_emit at (N, T) = (16, 384), (128, 384)
and (16, 4096) by HIP events around the launches alone (warm, the minimum of 5 rounds), the whole midi_util.rolls_to_midi_bytes call (two
entries, the host read of the sizes between them, the copy of the files to the host) by the wall clock, and the host path --
piano_roll_to_pretty_midi(...).write per sample, as save_piano_roll_midi runs it -- on the same rolls IN THE SAME PROCESS.  Two kinds of
rolls: a batch decoded from noise by the synthetic VAE weights (what a --synthetic_weights run writes) and a dense synthetic roll (runs of
~30 columns in a third of the piano rows, onsets and pedal throughout).  The two paths' files are compared byte for byte while at it.
The figures are reported, not asserted.  Writes profiles/midi_time.json and prints it as one line.

    python tools/midi_time.py [--out profiles/midi_time.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rule-guided-music_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rgm import native as R, synth  # noqa: E402

SHAPES = ((16, 384), (128, 384), (16, 4096))


def events_us(fn, iters=20, rounds=5, warmup=5):
    """microseconds per call: events around `iters` back-to-back calls, the minimum of `rounds`"""
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


def wall_ms(fn, rounds):
    best = float("inf")
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return round(best, 3)


def decoded_rolls(vae, N, T):
    """(N, 128, T, 3) uint8 on the device: latents of unit noise through the synthetic decoder, as decode_sample_for_midi returns them"""
    from guided_diffusion import midi_util
    g = torch.Generator(device="cuda").manual_seed(N * 100003 + T)
    parts = []
    for lo in range(0, N, 16):                            # decoder batches of 16 excerpts
        z = torch.randn((min(16, N - lo), 4, T // 8, 16), device="cuda", generator=g)
        parts.append(midi_util.decode_sample_for_midi(z, embed_model=vae, scale_factor=1.2465, threshold=-0.95))
    return torch.cat(parts, 0).contiguous()


def dense_rolls(N, T):
    rng = np.random.default_rng(N * 7 + T)
    state = rng.random((N, 128)) < 0.3
    on = np.zeros((N, 128, T), dtype=bool)
    for t in range(T):
        state = np.where(state, rng.random((N, 128)) < 0.97, rng.random((N, 128)) < 0.015)
        on[:, :, t] = state
    roll = np.zeros((N, 128, T, 3), dtype=np.uint8)
    roll[..., 0] = on * rng.integers(20, 128, (N, 128, T))
    roll[:, :21, :, 0] = 0
    roll[..., 1] = rng.choice(np.array([0, 127], dtype=np.uint8), (N, 128, T), p=[0.9, 0.1])
    roll[..., 2] = rng.integers(0, 128, (N, 1, T))
    return torch.from_numpy(roll).cuda()


def host_path(arr, fs, tmp):
    """save_piano_roll_midi's loop body on (N, 3, 128, T) uint8 numpy rolls -> the files' bytes"""
    from music_rule_guidance.piano_roll_to_chord import piano_roll_to_pretty_midi
    out = []
    for i in range(arr.shape[0]):
        cur = np.array(arr[i])
        cur[1, np.nonzero(cur[0, :, 0])[0], 0] = 127
        path = os.path.join(tmp, f"{i}.midi")
        piano_roll_to_pretty_midi(cur.astype(np.float32), fs=fs).write(path)
        out.append(path)
    return out


def measure(rolls, fs=100):
    from guided_diffusion import midi_util
    N, _, T, _ = rolls.shape
    s = rolls.stride()
    strides = (s[0], s[3], s[1], s[2])
    ticks = midi_util.midi_tick_table(T, fs)
    counts = torch.empty((N, 4), dtype=torch.int64, device="cuda")
    ws = torch.empty((R.lib.rgm_midi_workspace(N, T) + 7) // 8, dtype=torch.int64, device="cuda")
    st = R.current_stream()

    def first():
        R.check(R.lib.rgm_midi_measure(C.c_void_p(rolls.data_ptr()), *strides, N, 3, T, 1, C.c_void_p(ticks.ctypes.data), R.ptr(counts), R.ptr(ws),
                                       ws.numel() * 8, st))
    first()
    sizes = counts.cpu().numpy()
    off = (torch.cumsum(counts, 0) - counts).t().contiguous()
    notes = torch.empty((int(sizes[:, 0].sum()), 4), dtype=torch.int32, device="cuda")
    ccs = torch.empty((int(sizes[:, 1].sum()), 2), dtype=torch.int32, device="cuda")
    blob = torch.empty(int(sizes[:, 3].sum()), dtype=torch.uint8, device="cuda")

    def second():
        R.check(R.lib.rgm_midi_emit(N, T, 0, R.ptr(off[0]), R.ptr(off[1]), R.ptr(off[3]), R.ptr(notes) if notes.numel() else None, notes.shape[0],
                                    R.ptr(ccs) if ccs.numel() else None, ccs.shape[0], R.ptr(blob), blob.numel(), R.ptr(ws), ws.numel() * 8, st))
    out = {"notes": int(sizes[:, 0].sum()), "ccs": int(sizes[:, 1].sum()), "messages": int(sizes[:, 2].sum()), "file_bytes": int(sizes[:, 3].sum()),
           "workspace_bytes": int(ws.numel() * 8), "measure_us": events_us(first), "emit_us": events_us(second)}
    files = midi_util.rolls_to_midi_bytes(rolls, fs=fs)
    out["rolls_to_midi_bytes_ms"] = wall_ms(lambda: midi_util.rolls_to_midi_bytes(rolls, fs=fs), 5)
    arr = rolls.cpu().numpy().transpose(0, 3, 1, 2)
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        paths = host_path(arr, fs, tmp)
        once = (time.perf_counter() - t0) * 1e3
        out["host_path_ms"] = round(min([once] + [wall_ms(lambda: host_path(arr, fs, tmp), 1) for _ in range(4 if once < 500 else 0)]), 3)
        out["files_equal"] = all(open(p, "rb").read() == f for p, f in zip(paths, files))
    with tempfile.TemporaryDirectory() as tmp:           # what the device path still does on the host: writing the bytes
        def dump():
            for i, f in enumerate(files):
                with open(os.path.join(tmp, f"{i}.midi"), "wb") as fh:
                    fh.write(f)
        out["write_given_bytes_ms"] = wall_ms(dump, 5)
    out["host_over_device"] = round(out["host_path_ms"] / (out["rolls_to_midi_bytes_ms"] + out["write_given_bytes_ms"]), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "midi_time.json"))
    a = ap.parse_args()
    from taming.models.klvae_pedal import AutoencoderKL
    vae = AutoencoderKL()
    vae.load_state_dict(synth.vae_state_dict(2, device="cuda", encoder=True))
    vae = vae.to("cuda").eval()
    R.set_gemm_precision("bf16x3_presplit")
    out = {"fs": 100, "channels": 3, "first_column_onsets": True, "shapes": {}}
    for N, T in SHAPES:
        out["shapes"][f"N{N}_T{T}"] = {"decoded": measure(decoded_rolls(vae, N, T)), "dense": measure(dense_rolls(N, T))}
    out["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
