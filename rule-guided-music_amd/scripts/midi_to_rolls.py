"""A directory of MIDI files -> the uint8 .npy piano-roll excerpts the samplers, edit.py and eval_sets.py consume: the counterpart of the
reference's datasets/piano_roll_all.py (docs/rounds/midi_read.md).

    python scripts/midi_to_rolls.py --midi_dir DIR --outdir DIR [--fs 100] [--image_size 128] [--overlap False] [--batch_size 64]
                                    [--midi_reader device]

Every *.mid / *.midi file's (3, 128, T) [velocity | onset | pedal] roll is cut at multiples of image_size, the last piece zero-padded; pieces
whose maximum is 0 are skipped; each piece is saved as uint8 (3, 128, image_size) under <stem>_<k>.npy, and with --overlap True the
half-shifted pieces under shift_<stem>_<k>.npy with k = j // image_size, as the reference names them.  Velocity sums above 255 saturate
(the reference's cast wraps) and are counted.  A file the reader refuses is named on stderr and skipped.  run_metadata.json lists counts,
refusals and overflow.  --midi_reader device (the default here) builds whole batches with csrc/midi_read.hip; host runs SimpleMIDI and
midi_to_full_piano_roll file by file."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def str2bool(v):
    if isinstance(v, bool):
        return v
    if v.lower() in ("yes", "true", "t", "y", "1"):
        return True
    if v.lower() in ("no", "false", "f", "n", "0"):
        return False
    raise argparse.ArgumentTypeError("boolean value expected")


def create_argparser():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--midi_dir", required=True, type=str, help="directory of .mid / .midi files")
    p.add_argument("--outdir", required=True, type=str, help="where the .npy pieces and run_metadata.json go")
    p.add_argument("--fs", type=float, default=100, help="columns per second")
    p.add_argument("--image_size", type=int, default=128, help="columns per piece")
    p.add_argument("--overlap", type=str2bool, default=False, help="also save the pieces shifted by image_size // 2")
    p.add_argument("--batch_size", type=int, default=64, help="files per device call")
    p.add_argument("--midi_reader", default="device", choices=["host", "device"], help="who builds the rolls")
    return p


def host_reader(paths, fs):
    """[(float32 (3,128,T) roll, or None when refused; the reason)] from the host reader, one file after the other."""
    from guided_diffusion import midi_util
    out = []
    for p in paths:
        try:
            out.append((midi_util.read_midi_piano_roll(p, fs), None))
        except Exception as e:                           # the host reader raises ValueError, IndexError, struct.error ... on a bad file
            out.append((None, f"{type(e).__name__}: {e}"))
    return out


def device_reader(paths, fs):
    """The same list from one device call: float32 rolls, exact, trimmed to every file's own length on the host."""
    import torch
    from guided_diffusion import midi_util
    r = midi_util.midi_files_to_rolls(paths, fs=fs, dtype=torch.float32, strict=False)
    rolls, cols, status = r["roll"].cpu().numpy(), r["columns"].cpu().numpy(), r["status"].cpu().numpy()
    return [(rolls[i, :, :, :int(cols[i])], None) if status[i] == 0 else
            (None, f"status {int(status[i])} ({midi_util.MIDI_READ_STATUS[int(status[i])]})") for i in range(len(paths))]


def save_pieces(roll, stem, outdir, image_size, overlap):
    """The reference's two loops (datasets/piano_roll_all.py:90-123) -> (names written, saturated cells)."""
    names, T = [], roll.shape[-1]
    over = int((roll > 255).sum())
    roll = np.minimum(roll, 255)
    for first, prefix in ((0, ""), (image_size // 2, "shift_")) if overlap else ((0, ""),):
        for j in range(first, T, image_size):
            piece = np.zeros((3, 128, image_size), dtype=np.uint8)
            piece[:, :, :min(image_size, T - j)] = roll[:, :, j:j + image_size].astype(np.uint8)
            if piece.max() == 0:
                continue
            names.append(f"{prefix}{stem}_{j // image_size}.npy")
            np.save(os.path.join(outdir, names[-1]), piece)
    return names, over


def main(argv=None, reader_fn=None):
    args = create_argparser().parse_args(argv)
    if args.image_size < 2 or args.batch_size < 1 or not args.fs > 0:
        raise ValueError("midi_to_rolls: image_size >= 2, batch_size >= 1 and fs > 0 are needed")
    if reader_fn is None:
        reader_fn = device_reader if args.midi_reader == "device" else host_reader
    paths = sorted(os.path.join(args.midi_dir, f) for f in os.listdir(args.midi_dir) if f.lower().endswith((".mid", ".midi")))
    os.makedirs(args.outdir, exist_ok=True)
    meta = {"midi_dir": args.midi_dir, "fs": args.fs, "image_size": args.image_size, "overlap": bool(args.overlap),
            "midi_reader": args.midi_reader, "files": len(paths), "converted": 0, "pieces": 0, "refused": [], "overflow_cells": 0,
            "overflow_files": []}
    for b in range(0, len(paths), args.batch_size):
        batch = paths[b:b + args.batch_size]
        for path, (roll, reason) in zip(batch, reader_fn(batch, args.fs)):
            name = os.path.basename(path)
            if roll is None:
                print(f"midi_to_rolls: {path} refused: {reason}", file=sys.stderr)
                meta["refused"].append({"file": name, "reason": reason})
                continue
            names, over = save_pieces(np.asarray(roll), name[:name.lower().rfind(".mid")], args.outdir, args.image_size, args.overlap)
            meta["converted"] += 1
            meta["pieces"] += len(names)
            if over:
                meta["overflow_cells"] += over
                meta["overflow_files"].append(name)
    with open(os.path.join(args.outdir, "run_metadata.json"), "w") as f:
        json.dump(meta, f, indent=1)
    return meta


if __name__ == "__main__":
    main()
