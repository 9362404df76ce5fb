#!/usr/bin/env python3
"""Generate tests/golden/step_inputs.npz by IMPORTING the reference:  `python tests/golden/make_golden_step_inputs.py`.

Runs only in the build container, like the other make_golden_*.py scripts, whose shims it installs.  No GPU test imports this file or the
reference.  Inputs are rebuilt from tests/step_cases.py (seeded, named); only what the reference returns is stored:

    <family>.n<N>c<C>t<T>.<rule>.out      FUNC_DICT[rule] of the reference on the family's roll (squeezed at N = 1 as the reference does);
                                          rule in note_density, note_density_hr_1, note_density_hr_2, note_density_pixel, note_density_class
                                          (N > 1 only: the reference indexes a batch axis there) and pitch_hist
    <family>.n<N>c<C>t<T>.<rule>.after    channel 0 of the roll after the call (the in-place mask and snap); the other channels are asserted
                                          untouched here
    <family>.n<N>c<C>t<T>.chord.q/.after  the integer roll get_chords hands its analyser (a recorder stands in for it) and channel 0 after
    split.n<n>ov<ov>.wins                 w_img.split_wimg of a seeded (3, 4, 1, W) image
    merge.n<n>ov<ov>.avg / .sum           w_img.avg_merge_wimg(is_avg = True / False) of seeded windows at B = 3
    seed.*                                every seed the inputs are rebuilt from

Asserted here: oracle/rules_np.py and oracle/collage_np.py give the same arrays bit for bit (NaN by position; pitch_hist, a float sum in
another order, to 1e-6 with the same roll afterwards)."""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import step_cases as sc  # noqa: E402  (tests/step_cases.py)
import ref_shims  # noqa: E402

ref_shims.install()
from music_rule_guidance import music_rules as rmr, rule_maps as rrm  # noqa: E402
from diff_collage import w_img as rwi  # noqa: E402
from oracle import rules_np as orl, collage_np as ocl  # noqa: E402

assert rmr.__file__.startswith(ref_shims.REF_ROOT), rmr.__file__
LIMIT = 1024 * 1024
RULES = tuple(sc.ND_RULES) + ("note_density_class", "pitch_hist")


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def save(path, arrs):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:   # np.savez_compressed's layout with a fixed time stamp
        for k, v in arrs.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())
    assert os.path.getsize(path) < LIMIT, f"{path}: {os.path.getsize(path)} bytes"
    print(f"  wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB, {len(arrs)} arrays)")


def main():
    out = {"seed.rule": np.array([sc.RULE_SEED], np.int64), "seed.collage": np.array([sc.COLLAGE_SEED], np.int64)}
    for fam, shape in sc.rule_cases():
        key = sc.case_key(fam, shape)
        src = sc.roll(fam, shape)
        for rule in RULES:
            if rule == "note_density_class" and shape[0] == 1:
                continue
            t = torch.from_numpy(src.copy())
            res = rrm.FUNC_DICT[rule](t).numpy()
            after = t.numpy()
            assert same(after[:, 1:], src[:, 1:]), (key, rule)
            mine = src.copy()
            own = orl.FUNC_DICT[rule](mine)
            assert same(mine, after), (key, rule, "oracle/rules_np.py leaves another roll than the reference")
            if rule == "pitch_hist":                                    # a float sum: the order differs, the places of the NaN do not
                assert same(np.isnan(own), np.isnan(res)) and np.allclose(own, res, rtol=0, atol=1e-6, equal_nan=True), (key, rule)
            else:
                assert same(own, res), (key, rule, "oracle/rules_np.py differs from the reference")
            out[f"{key}.{rule}.out"], out[f"{key}.{rule}.after"] = res, after[:, 0]
        print(f"  [{key}] {len(RULES)} rules", flush=True)
    seen = []

    def recorder(pr, given_key=None, fs=100, window_size=1.28, return_key=False):
        seen.append(np.array(pr))
        return {"chords": torch.zeros(int(pr.shape[-1] / fs / window_size), dtype=torch.long)}
    old, rmr.piano_roll_to_chords = rmr.piano_roll_to_chords, recorder
    try:
        for fam, shape in sc.rule_cases(sc.CHORD_SHAPES):
            key = sc.case_key(fam, shape)
            src = sc.roll(fam, shape)
            t = torch.from_numpy(src.copy())
            del seen[:]
            rmr.get_chords(t)
            q = np.stack(seen)
            assert q.min() >= 0 and q.max() <= 127 and q.shape == (shape[0], 128, shape[2])
            mine = src.copy()
            assert same(orl.chord_quantise(mine), q) and same(mine, t.numpy()), (key, "chord")
            assert same(t.numpy()[:, 1:], src[:, 1:])
            out[f"{key}.chord.q"], out[f"{key}.chord.after"] = q.astype(np.uint8), t.numpy()[:, 0]
    finally:
        rmr.piano_roll_to_chords = old
    for n in sc.COLLAGE_N:
        for ov in sc.COLLAGE_OV:
            img, wins = sc.golden_image(n, ov), sc.golden_windows(n, ov)
            xs, got_ov = rwi.split_wimg(torch.from_numpy(img), n)
            assert got_ov == ov and same(ocl.split_wimg(img, n)[0], xs.numpy())
            out[f"split.n{n}ov{ov}.wins"] = xs.numpy()
            for tag, avg in (("avg", True), ("sum", False)):
                m = rwi.avg_merge_wimg(torch.from_numpy(wins), ov, n=n, is_avg=avg).numpy()
                if ov <= 64:                                            # at most two terms per element: the order cannot matter
                    assert same(ocl.merge_wimg(wins, ov, n, avg), m), (n, ov, tag)
                out[f"merge.n{n}ov{ov}.{tag}"] = m
    save(os.path.join(HERE, "step_inputs.npz"), out)


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
