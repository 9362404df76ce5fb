"""What the set-level evaluation costs.  (1) rgm_set_kl_oa alone (1000 KL points, 16384 Simpson panels) on the intra / inter distances of
N = 200, 500 and 1000 samples of a one-dimensional statistic: HIP events behind a warm-up, the minimum over repeated calls.  (2)
evaluate_sets for the seven metrics at those N.  (3) The host partner kl_oa_np on one core at the N of --host_sizes.  (4) The
reference's own times, quoted from the measurement on the build container's CPU that motivated the work (mgeval/utils.py on synthetic
distance vectors), not re-measured here.  Writes profiles/sets_time.json and prints it as one line.

    python tools/sets_time.py [--out profiles/sets_time.json] [--repeats 5] [--host_only | --device_only] [--host_sizes 200,500,1000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rule-guided-music_amd"), os.path.join(ROOT, "tests")]

SIZES = (200, 500, 1000)
REFERENCE = {"provenance": "the reference's mgeval/utils.py kl_dist / overlap_area on synthetic distance vectors, one CPU core of the build container",
             "N200_n40000": {"kl_dist_s": 1.5, "overlap_area_s": 2.3}, "N500_n250000": {"kl_dist_s": 5.8, "overlap_area_s": 11.2}}


def min_ms(fn, repeats, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def stats_like(N, seed):
    """seven statistics of N samples with the shapes and rough ranges of note_stats' values"""
    rng = np.random.RandomState(seed)
    return {"total_used_pitch": rng.randint(10, 40, size=N).astype(np.float64), "pitch_range": rng.randint(20, 70, size=N).astype(np.float64),
            "avg_IOI": rng.gamma(3.0, 0.05, size=N), "total_pitch_class_histogram": rng.dirichlet(np.full(12, 0.7), size=N),
            "mean_note_velocity": rng.randint(40, 100, size=N).astype(np.float64), "mean_note_duration": rng.gamma(2.0, 0.2, size=N),
            "note_density_mgeval": rng.gamma(4.0, 2.0, size=N)}


def device(repeats):
    import torch
    from music_evaluation import set_eval
    out = {}
    for N in SIZES:
        s1, s2 = stats_like(N, 1), stats_like(N, 2)
        d1 = {k: torch.from_numpy(v).cuda() for k, v in s1.items()}
        d2 = {k: torch.from_numpy(v).cuda() for k, v in s2.items()}
        intra, _, inter = set_eval.set_distances(d1["mean_note_duration"], d2["mean_note_duration"])
        points = set_eval.KL_POINTS + set_eval.OA_PANELS + 1
        call = min_ms(lambda: set_eval.kl_oa(intra, inter), repeats)
        dist = min_ms(lambda: set_eval.set_distances(d1["total_pitch_class_histogram"], d2["total_pitch_class_histogram"]), repeats)
        whole = min_ms(lambda: set_eval.evaluate_sets(d1, d2), repeats)
        pairs = points * (intra.numel() + inter.numel())
        out[f"N{N}"] = {"n_intra": intra.numel(), "n_inter": inter.numel(), "points_per_density": points, "rgm_set_kl_oa_ms": round(call, 3),
                        "exp_per_ns": round(pairs / (call * 1e6), 2), "set_distances_d12_three_vectors_ms": round(dist, 3),
                        "evaluate_sets_seven_metrics_ms": round(whole, 3)}
    out["device"] = torch.cuda.get_device_name(0)
    return out


def host(sizes):
    from music_evaluation import set_eval
    out = {}
    for N in sizes:
        s1, s2 = stats_like(N, 1), stats_like(N, 2)
        intra, _, inter = set_eval.set_distances_np(s1["mean_note_duration"][:, None], s2["mean_note_duration"][:, None])
        t0 = time.perf_counter()
        set_eval.kl_oa_np(intra, inter)
        out[f"N{N}"] = {"kl_oa_np_s": round(time.perf_counter() - t0, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sets_time.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host_only", action="store_true")
    ap.add_argument("--device_only", action="store_true")
    ap.add_argument("--host_sizes", default="200", help="comma-separated N for the host partner (1000 takes ten minutes on one core)")
    args = ap.parse_args()
    res = json.load(open(args.out)) if os.path.exists(args.out) else {}       # the two halves may be measured in two runs
    res.update({"kl_points": 1000, "oa_panels": 16384, "reference_quoted": REFERENCE})
    if not args.device_only:
        res.setdefault("host_partner", {}).update(host([int(n) for n in args.host_sizes.split(",")]))
    if not args.host_only:
        res["device"] = device(args.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
