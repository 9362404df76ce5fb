"""A directory of uint8 .npy piano rolls -> .wav files: the counterpart of the reference's music_evaluation/convert_to_wav.py with the sine
voice of its pretty_midi fork in place of fluidsynth and a sound font (docs/rounds/synth.md).

    python scripts/rolls_to_wav.py --roll_dir DIR --outdir DIR [--fs 100] [--wav_fs 44100] [--batch 16]

Every *.npy file holding a uint8 roll (3, 128, T) [velocity | onset | pedal], (2, 128, T) [velocity | pedal] or (128, T) -- what the
samplers save beside their .midi files and what scripts/midi_to_rolls.py writes -- becomes <stem>.wav (mono, 16 bit): the notes
piano_roll_to_pretty_midi finds, with save_piano_roll_midi's forced onsets in column 0 so that the audio holds the notes of the .midi file
of the same roll, each one sine under exp(-t), the sum normalised to its peak.  Rolls of one shape are rendered together by csrc/synth.hip,
--batch at a time.  A file that holds something else is named on stderr and skipped.  rolls_to_wav.json lists what was written."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def create_argparser():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--roll_dir", required=True, type=str, help="directory of uint8 .npy rolls")
    p.add_argument("--outdir", required=True, type=str, help="where the .wav files and rolls_to_wav.json go")
    p.add_argument("--fs", type=float, default=100, help="columns per second of the rolls")
    p.add_argument("--wav_fs", type=int, default=44100, help="audio samples per second")
    p.add_argument("--batch", type=int, default=16, help="rolls per device call")
    return p


def load_roll(path):
    """-> (C, 128, T) uint8, or None with the reason"""
    try:
        a = np.load(path, allow_pickle=False)
    except Exception as e:                               # not an array file
        return None, f"{type(e).__name__}: {e}"
    if a.dtype != np.uint8:
        return None, f"dtype {a.dtype}, not uint8"
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[0] not in (1, 2, 3) or a.shape[1] != 128 or a.shape[2] < 1:
        return None, f"shape {a.shape}, not (C, 128, T) with C in 1 .. 3"
    return a, None


def main(argv=None):
    args = create_argparser().parse_args(argv)
    if args.batch < 1 or not args.fs > 0 or args.wav_fs < 1:
        raise ValueError("rolls_to_wav: batch >= 1, fs > 0 and wav_fs >= 1 are needed")
    import torch
    from guided_diffusion import midi_util
    names = sorted(f for f in os.listdir(args.roll_dir) if f.endswith(".npy"))
    os.makedirs(args.outdir, exist_ok=True)
    meta = {"roll_dir": args.roll_dir, "fs": args.fs, "wav_fs": args.wav_fs, "files": len(names), "written": 0, "silent": [], "skipped": []}
    by_shape = {}
    for name in names:
        roll, reason = load_roll(os.path.join(args.roll_dir, name))
        if roll is None:
            print(f"rolls_to_wav: {name} skipped: {reason}", file=sys.stderr)
            meta["skipped"].append({"file": name, "reason": reason})
            continue
        by_shape.setdefault(roll.shape, []).append((name, roll))
    fs = int(args.fs) if float(args.fs).is_integer() else args.fs
    for shape in sorted(by_shape):
        group = by_shape[shape]
        for b in range(0, len(group), args.batch):
            part = group[b:b + args.batch]
            rolls = torch.from_numpy(np.stack([r for _, r in part])).cuda()
            files = midi_util.rolls_to_wav_bytes(rolls, fs=fs, audio_fs=args.wav_fs, first_column_onsets=True)
            for (name, _), data in zip(part, files):
                with open(os.path.join(args.outdir, name[:-4] + ".wav"), "wb") as f:
                    f.write(data)
                meta["written"] += 1
                if not any(data[44:]):
                    meta["silent"].append(name)
    with open(os.path.join(args.outdir, "rolls_to_wav.json"), "w") as f:
        json.dump(meta, f, indent=1)
    return meta


if __name__ == "__main__":
    main()
