"""What rendering audio on the device costs (docs/rounds/synth.md): rgm_synth_render at (N, T, audio_fs) = (16, 1024, 44100) and
(128, 1024, 16000) by HIP events around the entry alone (its four small table copies and two launches; warm, the minimum of 3 rounds of 5
calls), rgm_synth_pcm the same way, the whole midi_util.rolls_to_wav_bytes call (the MIDI measure and emit entries with their host read of
the sizes, render, pcm, the copy of the files to the host, the slicing) by the wall clock, and the host partner -- synthesize_roll and
wav_bytes per roll -- on the first rolls of the same batch IN THE SAME PROCESS, scaled to the batch.  Two kinds of rolls, those of
tools/midi_time.py: a batch decoded from noise by the synthetic VAE weights and a dense synthetic roll.  The two paths' files are compared
while at it: the share of int16 samples that are equal and the largest difference (sin and exp come from two libraries, so a sample
within their error of a rounding boundary may differ by one).  The figures are reported, not asserted.  Writes profiles/synth_time.json
and prints it as one line.

    python tools/synth_time.py [--out profiles/synth_time.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rule-guided-music_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from midi_time import decoded_rolls, dense_rolls, events_us, wall_ms  # noqa: E402  (tools/midi_time.py)
from rgm import native as R, synth  # noqa: E402

SHAPES = ((16, 1024, 44100), (128, 1024, 16000))
HOST_ROLLS = 4                                           # rolls the host partner is timed on


def measure(rolls, audio_fs, fs=100):
    from guided_diffusion import midi_util
    from music_rule_guidance import music_rules
    from music_rule_guidance.piano_roll_to_chord import synthesize_roll, wav_bytes
    N, _, T, _ = rolls.shape
    ev = music_rules.midi_events_raw(rolls, fs=fs, first_column_onsets=True)
    samp, length, omega, fade = midi_util.synth_host_tables(T, fs, audio_fs)
    cap = (int(length[T]) + 7) // 8 * 8
    wave = torch.empty((N, cap), dtype=torch.float64, device="cuda")
    lengths = torch.empty(N, dtype=torch.int64, device="cuda")
    peak = torch.empty(N, dtype=torch.float64, device="cuda")
    silent = torch.empty(N, dtype=torch.int32, device="cuda")
    ws = torch.empty((R.lib.rgm_synth_workspace(N, T, cap) + 15) // 16 * 2, dtype=torch.int64, device="cuda")
    pcm = torch.empty(N * (44 + 2 * cap), dtype=torch.uint8, device="cuda")
    st = R.current_stream()
    notes, ccs = ev["notes"], ev["ccs"]

    def render():
        R.check(R.lib.rgm_synth_render(N, T, R.ptr(notes) if notes.numel() else None, notes.shape[0], R.ptr(ev["note_offsets"]),
                                       R.ptr(ccs) if ccs.numel() else None, ccs.shape[0], R.ptr(ev["cc_offsets"]), R.ptr(ev["counts"]),
                                       float(audio_fs), samp.ctypes.data, length.ctypes.data, omega.ctypes.data, fade.ctypes.data, len(fade),
                                       R.ptr(wave), cap, R.ptr(lengths), R.ptr(peak), R.ptr(silent), R.ptr(ws), ws.numel() * 8, st))

    def quantise():
        R.check(R.lib.rgm_synth_pcm(N, R.ptr(wave), R.ptr(lengths), R.ptr(peak), cap, 1, int(audio_fs), R.ptr(pcm), st))
    out = {"notes": int(notes.shape[0]), "ccs": int(ccs.shape[0]), "cap": cap, "workspace_bytes": int(ws.numel() * 8),
           "render_us": events_us(render, iters=5, rounds=3, warmup=2), "pcm_us": events_us(quantise, iters=5, rounds=3, warmup=2)}
    lens = lengths.cpu().numpy()
    m = np.zeros((N, cap), dtype=np.int32)                # notes sounding per audio sample: the number of sin + exp pairs formed
    rows, offs, cnt = notes.cpu().numpy(), ev["note_offsets"].cpu().numpy(), ev["counts"].cpu().numpy()[:, 0]
    for n in range(N):
        for p, v, a, b in rows[offs[n]:offs[n] + cnt[n]]:
            m[n, samp[a]:samp[b]] += 1
    out["audio_samples"] = int(lens.sum())
    out["terms"] = int(m.sum())
    out["render_ps_per_term"] = round(out["render_us"] * 1e6 / out["terms"], 2) if out["terms"] else None
    out["silent"] = int(silent.sum())
    files = midi_util.rolls_to_wav_bytes(rolls, fs=fs, audio_fs=audio_fs)
    out["rolls_to_wav_bytes_ms"] = wall_ms(lambda: midi_util.rolls_to_wav_bytes(rolls, fs=fs, audio_fs=audio_fs), 3)
    out["wav_bytes"] = int(sum(len(f) for f in files))
    arr = rolls.cpu().numpy().transpose(0, 3, 1, 2)
    k = min(N, HOST_ROLLS)
    t0 = time.perf_counter()
    host = []
    for i in range(k):
        cur = np.array(arr[i])
        cur[1, np.nonzero(cur[0, :, 0])[0], 0] = 127
        host.append(wav_bytes(synthesize_roll(cur.astype(np.float32), fs=fs, audio_fs=audio_fs), audio_fs))
    out["host_rolls_timed"] = k
    out["host_partner_ms_per_roll"] = round((time.perf_counter() - t0) * 1e3 / k, 3)
    out["host_partner_ms_scaled_to_batch"] = round(out["host_partner_ms_per_roll"] * N, 1)
    out["host_over_device"] = round(out["host_partner_ms_scaled_to_batch"] / out["rolls_to_wav_bytes_ms"], 1)
    same, total, worst = 0, 0, 0
    for h, d in zip(host, files):
        out["lengths_equal"] = out.get("lengths_equal", True) and len(h) == len(d) and h[:44] == d[:44]
        if len(h) == len(d):
            a, b = np.frombuffer(h[44:], dtype="<i2").astype(np.int32), np.frombuffer(d[44:], dtype="<i2").astype(np.int32)
            same, total, worst = same + int((a == b).sum()), total + a.size, max(worst, int(np.abs(a - b).max()) if a.size else 0)
    out["int16_equal_share"] = round(same / max(1, total), 8)
    out["int16_largest_difference"] = worst
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "synth_time.json"))
    a = ap.parse_args()
    from taming.models.klvae_pedal import AutoencoderKL
    vae = AutoencoderKL()
    vae.load_state_dict(synth.vae_state_dict(2, device="cuda", encoder=True))
    vae = vae.to("cuda").eval()
    R.set_gemm_precision("bf16x3_presplit")
    out = {"fs": 100, "channels": 3, "first_column_onsets": True, "shapes": {}}
    for N, T, rate in SHAPES:
        out["shapes"][f"N{N}_T{T}_fs{rate}"] = {"decoded": measure(decoded_rolls(vae, N, T), rate), "dense": measure(dense_rolls(N, T), rate)}
    out["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
