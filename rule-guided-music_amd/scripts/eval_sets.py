"""Set-level objective evaluation of two directories of saved rolls, on the device: the counterpart of the reference's
music_evaluation/music_evaluator.py (docs/rounds/sets.md).

    python scripts/eval_sets.py --set1dir DIR --set2dir DIR --outdir DIR [--savename NAME] [--num_sample N] [--num_runs 1] [--seed 0]

Reads the .npy rolls that save_piano_roll_midi writes next to every .midi, runs music_rules.note_stats(..., first_column_onsets=True) on
them in batches (rolls of different lengths in groups of equal T), draws the reference's random subsets per run (set 2 once, set 1 per
run; seeded here, the reference's are not), and writes <savename>_mean.csv / <savename>_std.csv -- or <set1>.<set2>.mean.csv / .std.csv --
with the reference's columns attribute,KL,OA and its `avg` row, plus run_metadata.json.  A metric that is constant over a set (the
reference raises LinAlgError) is written as nan, named on stderr and left out of `avg`.  The statistics are those of the in-memory
rolls, not of the MIDI files read back (docs/rounds/notes.md)."""
import argparse
import csv
import glob
import json
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from music_evaluation.set_eval import DEFAULT_METRICS, KL_POINTS, OA_PANELS  # noqa: E402


def create_argparser():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--set1dir", required=True, type=str, help="directory of the first set's .npy rolls")
    p.add_argument("--set2dir", required=True, type=str, help="directory of the second (baseline) set's .npy rolls")
    p.add_argument("--outdir", required=True, type=str, help="where the two CSV files and run_metadata.json go")
    p.add_argument("--savename", type=str, default=None, help="stem of the output CSV files")
    p.add_argument("--num_sample", type=int, default=None, help="samples per set and run (default: all)")
    p.add_argument("--num_runs", type=int, default=1, help="runs over which mean and std are taken")
    p.add_argument("--seed", type=int, default=0, help="seed of the random subsets")
    p.add_argument("--batch_size", type=int, default=64, help="rolls per note_stats call")
    return p


def device_note_stats(rolls):
    """(N, C, 128, T) uint8 numpy -> music_rules.note_stats on the device"""
    import torch
    from music_rule_guidance import music_rules
    return music_rules.note_stats(torch.from_numpy(np.ascontiguousarray(rolls)).cuda(), first_column_onsets=True)


def device_evaluate(stats1, stats2, metrics):
    from music_evaluation.set_eval import evaluate_sets
    return evaluate_sets(stats1, stats2, metrics)


def _cat(parts):
    if isinstance(parts[0], np.ndarray):
        return np.concatenate(parts)
    import torch
    return torch.cat(parts)


def _take(x, idx):
    if isinstance(x, np.ndarray):
        return x[np.asarray(idx, dtype=np.int64)]
    import torch
    return x[torch.as_tensor(idx, dtype=torch.long, device=x.device)]


def list_rolls(directory):
    files = sorted(glob.glob(os.path.join(directory, "*.npy")))
    if not files:
        raise SystemExit(f"no .npy rolls in {directory}")
    return files


def stats_of_files(files, note_stats_fn, batch_size):
    """the statistics of every file, in the order of `files`: rolls are grouped by shape, sent through note_stats_fn in batches and put
    back in file order"""
    groups = {}
    for i, f in enumerate(files):
        roll = np.load(f)
        if roll.ndim == 2:
            roll = roll[None]
        if roll.ndim != 3 or roll.shape[1] != 128 or roll.dtype != np.uint8:
            raise SystemExit(f"{f}: expected a uint8 roll (C, 128, T), got {roll.dtype} {roll.shape}")
        groups.setdefault(roll.shape, []).append((i, roll))
    order, parts = [], []
    for shape in sorted(groups):
        members = groups[shape]
        for k in range(0, len(members), batch_size):
            chunk = members[k:k + batch_size]
            order += [i for i, _ in chunk]
            parts.append(note_stats_fn(np.stack([r for _, r in chunk])))
    back = np.argsort(np.asarray(order))
    return {key: _take(_cat([p[key] for p in parts]), back) for key in parts[0]}


def _number(v):
    return float(v.item()) if hasattr(v, "item") else float(v)


def main(argv=None, note_stats_fn=None, evaluate_fn=None):
    args = create_argparser().parse_args(argv)
    note_stats_fn = note_stats_fn or device_note_stats
    evaluate_fn = evaluate_fn or device_evaluate
    metrics = list(DEFAULT_METRICS)
    files1, files2 = list_rolls(args.set1dir), list_rolls(args.set2dir)
    stats1, stats2 = stats_of_files(files1, note_stats_fn, args.batch_size), stats_of_files(files2, note_stats_fn, args.batch_size)
    rng = random.Random(args.seed)
    want = args.num_sample if args.num_sample else max(len(files1), len(files2))
    pick2 = rng.sample(range(len(files2)), min(want, len(files2)))              # the baseline subset is drawn once
    runs, degenerate, used = [], [], []
    for run in range(args.num_runs):
        pick1 = rng.sample(range(len(files1)), min(want, len(files1)))
        n = min(len(pick1), len(pick2))
        if n < 2:
            raise SystemExit(f"set evaluation needs at least two samples per set, got {len(pick1)} and {len(pick2)}")
        s1 = {k: _take(v, pick1[:n]) for k, v in stats1.items()}
        s2 = {k: _take(v, pick2[:n]) for k, v in stats2.items()}
        res = evaluate_fn(s1, s2, metrics)
        rows = [(m, _number(res[m]["KL"]), _number(res[m]["OA"])) for m in metrics]
        bad = [m for m in metrics if bool(_number(res[m]["degenerate"]))]
        for m in bad:
            print(f"run {run}: {m} is constant over a set (the reference raises LinAlgError): written as nan, left out of avg", file=sys.stderr)
        rows.append(("avg", _number(res["avg"]["KL"]), _number(res["avg"]["OA"])))
        runs.append(rows)
        degenerate.append(bad)
        used.append(n)
    kl = np.array([[r[1] for r in rows] for rows in runs])                      # (runs, attributes)
    oa = np.array([[r[2] for r in rows] for rows in runs])
    os.makedirs(args.outdir, exist_ok=True)
    if args.savename is None:
        stem = f"{os.path.basename(os.path.normpath(args.set1dir))}.{os.path.basename(os.path.normpath(args.set2dir))}"
        mean_csv, std_csv = os.path.join(args.outdir, stem + ".mean.csv"), os.path.join(args.outdir, stem + ".std.csv")
    else:
        mean_csv, std_csv = os.path.join(args.outdir, args.savename + "_mean.csv"), os.path.join(args.outdir, args.savename + "_std.csv")
    attributes = metrics + ["avg"]
    for path, fold in ((mean_csv, np.mean), (std_csv, np.std)):
        with open(path, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["attribute", "KL", "OA"])
            for j, a in enumerate(attributes):
                w.writerow([a, repr(float(fold(kl[:, j]))), repr(float(fold(oa[:, j])))])
    meta = {"set1dir": args.set1dir, "set2dir": args.set2dir, "files": [len(files1), len(files2)], "num_sample": args.num_sample,
            "num_runs": args.num_runs, "seed": args.seed, "samples_in_use": used, "metrics": metrics, "kl_points": KL_POINTS,
            "oa_panels": OA_PANELS, "degenerate": degenerate, "first_column_onsets": True, "mean_csv": mean_csv, "std_csv": std_csv}
    with open(os.path.join(args.outdir, "run_metadata.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(f"saved {mean_csv} and {std_csv}")
    return {"attributes": attributes, "KL": kl, "OA": oa, "mean_csv": mean_csv, "std_csv": std_csv, "degenerate": degenerate}


if __name__ == "__main__":
    main()
