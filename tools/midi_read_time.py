"""What reading MIDI files on the device costs (docs/rounds/midi_read.md): rgm_midi_read_scan and rgm_midi_read_rolls for N = 16 and 128 files
of about 16 KB and for one file of about 1 MB, by HIP events around the entries alone (warm, the minimum of 5 rounds), the whole
midi_util.midi_files_to_rolls call (packing, the upload of the blob, both entries, the host read of the sizes) by the wall clock, and the
host reader -- SimpleMIDI followed by midi_to_full_piano_roll, file after file -- on the same files IN THE SAME PROCESS.  The files are the
device writer's files of dense synthetic rolls (runs of ~30 columns in a third of the piano rows, onsets and pedal throughout).  The two
paths' rolls are compared cell for cell while at it.  The figures are reported, not asserted.  Writes profiles/midi_read_time.json and prints
it as one line.

    python tools/midi_read_time.py [--out profiles/midi_read_time.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rule-guided-music_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rgm import native as R  # noqa: E402

SHAPES = (("N16_16KB", 16, 480), ("N128_16KB", 128, 480), ("N1_1MB", 1, 30000))


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


def wall_ms(fn, rounds):
    best = float("inf")
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return round(best, 3)


def dense_files(N, T):
    """N files: the device writer's bytes of dense (3, 128, T) rolls"""
    from guided_diffusion import midi_util
    rng = np.random.default_rng(N * 7 + T)
    state = rng.random((N, 128)) < 0.3
    on = np.zeros((N, 128, T), dtype=bool)
    for t in range(T):
        state = np.where(state, rng.random((N, 128)) < 0.97, rng.random((N, 128)) < 0.015)
        on[:, :, t] = state
    roll = np.zeros((N, 3, 128, T), dtype=np.uint8)
    roll[:, 0] = on * rng.integers(20, 128, (N, 128, T))
    roll[:, 0, :21] = 0
    roll[:, 1] = rng.choice(np.array([0, 127], dtype=np.uint8), (N, 128, T), p=[0.9, 0.1])
    roll[:, 2] = rng.integers(0, 128, (N, 1, T))
    return midi_util.rolls_to_midi_bytes(torch.from_numpy(roll).cuda())


def host_rolls(paths, fs):
    from guided_diffusion import midi_util
    return [midi_util.read_midi_piano_roll(p, fs) for p in paths]


def measure(files, fs=100):
    from guided_diffusion import midi_util
    blob_h, off_h, tracks = midi_util.pack_midi_files(files)
    N, total = len(files), int(off_h[-1])
    blob, off = torch.from_numpy(blob_h).cuda(), torch.from_numpy(off_h).cuda()
    status = torch.empty(N, dtype=torch.int32, device="cuda")
    counts = torch.empty((N, 4), dtype=torch.int64, device="cuda")
    columns = torch.empty(N, dtype=torch.int64, device="cuda")
    nbytes = R.lib.rgm_midi_read_workspace(N, total, tracks)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")
    st = R.current_stream()

    def scan():
        R.check(R.lib.rgm_midi_read_scan(R.ptr(blob), R.ptr(off), N, total, tracks, float(fs), R.ptr(status), R.ptr(counts), R.ptr(columns), None, None,
                                         None, 0, None, 0, R.ptr(ws), nbytes, st))
    scan()
    T = int(columns.max())
    out_u8 = torch.empty((N, 3, 128, T), dtype=torch.uint8, device="cuda")
    over = torch.empty(N, dtype=torch.int64, device="cuda")

    def rolls():
        R.check(R.lib.rgm_midi_read_rolls(N, total, tracks, float(fs), 0, T, 1, R.ptr(out_u8), R.ptr(over), R.ptr(ws), nbytes, st))
    sizes = counts.cpu().numpy()
    out = {"files": N, "bytes": total, "tracks": tracks, "notes": int(sizes[:, 0].sum()), "ccs": int(sizes[:, 1].sum()), "columns": T,
           "accepted": int((status == 0).sum()), "workspace_bytes": int(nbytes), "scan_us": events_us(scan), "rolls_us": events_us(rolls)}
    whole = midi_util.midi_files_to_rolls(files, fs=fs, dtype=torch.float32)
    out["midi_files_to_rolls_ms"] = wall_ms(lambda: midi_util.midi_files_to_rolls(files, fs=fs), 5)
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for i, f in enumerate(files):
            paths.append(os.path.join(tmp, f"{i}.mid"))
            with open(paths[-1], "wb") as fh:
                fh.write(f)
        t0 = time.perf_counter()
        host = host_rolls(paths, fs)
        once = (time.perf_counter() - t0) * 1e3
        out["host_reader_ms"] = round(min([once] + [wall_ms(lambda: host_rolls(paths, fs), 1) for _ in range(2 if once < 2000 else 0)]), 3)
        out["midi_files_to_rolls_from_paths_ms"] = wall_ms(lambda: midi_util.midi_files_to_rolls(paths, fs=fs), 5)
    got = whole["roll"].cpu().numpy()
    out["rolls_equal"] = all(np.array_equal(got[i, :, :, :h.shape[2]], h) and not got[i, :, :, h.shape[2]:].any() for i, h in enumerate(host))
    out["host_over_device"] = round(out["host_reader_ms"] / out["midi_files_to_rolls_from_paths_ms"], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "midi_read_time.json"))
    a = ap.parse_args()
    out = {"fs": 100, "shapes": {}}
    for name, N, T in SHAPES:
        out["shapes"][name] = measure(dense_files(N, T))
    out["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
