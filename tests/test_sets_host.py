"""CPU: the numpy host partner of the set-level evaluation (music_evaluation/set_eval.py: set_distances_np, kde_pdf_np, kl_oa_np,
evaluate_sets_np) against the reference's answers and the 80-bit evaluation in tests/golden/sets.npz, under the comparison rules of
docs/rounds/sets.md (sets_cases.check_distances / check_kl_oa): distances exact at d = 1 and within (d + 2) 2^-53 beyond, bandwidths
within 8 2^-53, densities no worse than the reference's own error against the 80-bit values, KL within eps (S + 2), OA within quad's
tolerance of the reference and within (eps + 32 2^-53) OA of the 80-bit Simpson value.  Plus the API, the ABI's new symbols and the
command line with the host partner injected."""
import csv
import importlib.util
import json
import os

import numpy as np
import pytest

import notes_cases as nc
import sets_cases as sc
from conftest import PKG, load_golden


@pytest.fixture(scope="module")
def gold():
    return load_golden("sets")


@pytest.fixture(scope="module")
def cases():
    return sc.cases(load_golden("notes"))


def test_fixture_names_and_what_the_reference_raises(gold, cases):
    assert [str(n) for n in gold["names"]] == list(cases) and int(gold["seed"][0]) == sc.SEED
    assert [str(f) for f in gold["scalar_fields"]] == list(sc.SCALARS)
    raises = dict(zip(cases, (str(r) for r in gold["raises"])))
    assert raises["constant.n12"] == raises["constant.n40"] == "LinAlgError"
    assert all(not r for n, r in raises.items() if not n.startswith("constant."))
    for name, (x1, x2) in cases.items():
        n = x1.shape[0]
        assert gold[f"{name}.intra1"].shape == (n * (n - 1),) and gold[f"{name}.inter"].shape == (n * n,)
    assert gold["ints.n96.intra1"].size == 9120 and gold["ints.n96.inter"].size == 9216
    assert np.isnan(cases["nan20.n40"][0]).any() and (gold["nan20.n40.inter"] == 0).sum() >= 40
    assert set(np.unique(gold["two_valued.n40.inter"])) == {0.0, 64.0}
    assert sc.scalar(gold, "two_valued.n40", "KL") < 1e-2               # a relative rule would be meaningless here


def test_host_distances_match_the_reference(gold, cases):
    from music_evaluation.set_eval import set_distances_np
    for name, (x1, x2) in cases.items():
        worst = sc.check_distances(set_distances_np(x1, x2), gold, name, x1.shape[1])
        if x1.shape[1] > 1:
            print(f"{name}: distances off by at most {worst:.2e} relative (bound {(x1.shape[1] + 2) * sc.U:.2e})")


def test_host_partner_matches_the_reference_and_the_80_bit_values_on_every_case(gold, cases):
    from music_evaluation.set_eval import kde_pdf_np, kl_oa_np
    for name in cases:
        A, B = gold[f"{name}.intra1"], gold[f"{name}.inter"]
        out = kl_oa_np(A, B)
        sA, sB = sc.kl_points(gold, name)
        sc.check_kl_oa(out, kde_pdf_np(A, sA), kde_pdf_np(B, sB), gold, name, "host")


def test_small_sets_and_the_degenerate_flag():
    from music_evaluation.set_eval import evaluate_sets_np, kde_pdf_np, kl_oa_np, set_distances_np
    x1, x2 = np.array([[1.0], [4.0]]), np.array([[2.0], [7.0]])
    intra1, intra2, inter = set_distances_np(x1, x2)
    assert intra1.tolist() == [3.0, 3.0] and intra2.tolist() == [5.0, 5.0] and inter.tolist() == [1.0, 6.0, 2.0, 3.0]
    out = kl_oa_np(intra1, inter)                                       # N = 2: the two intra distances are equal
    assert out[7] == 1.0 and np.isnan(out[:3]).all() and out[3] == 0.0 and out[5] == 1.0 and out[6] == 6.0
    assert np.isnan(kde_pdf_np([2.0, 2.0, 2.0], [1.0, 2.0])).all() and np.isnan(kde_pdf_np([2.0], [1.0])).all()
    three = evaluate_sets_np({"m": np.array([1.0, 4.0, 9.0])}, {"m": np.array([2.0, 7.0, 8.0, 100.0])}, metrics=("m",))
    assert not three["m"]["degenerate"] and 0 < three["m"]["OA"] < 1 and np.isfinite(three["m"]["KL"])      # cut to N = 3
    assert three["m"]["mean"].tolist() == [14.0 / 3.0] and three["avg"]["KL"] == three["m"]["KL"]
    with pytest.raises(ValueError):
        evaluate_sets_np({"m": np.array([1.0])}, {"m": np.array([2.0, 3.0])}, metrics=("m",))
    # NaN and inf distances are written as 0, in every dimension
    a = np.array([[np.nan, 1.0], [2.0, 3.0], [np.inf, 0.0]])
    intra, _, _ = set_distances_np(a, a)
    assert intra.tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]


def test_evaluate_sets_np_shapes_metrics_and_the_avg_row(gold):
    from music_evaluation.set_eval import DEFAULT_METRICS, evaluate_sets_np
    notes = load_golden("notes")
    s1, s2 = sc.notes_stats(notes, 384), sc.notes_stats(notes, 1064)
    assert DEFAULT_METRICS == sc.REAL_METRICS
    res = evaluate_sets_np(s1, s2, kl_points=200, oa_panels=512)
    assert list(res) == list(DEFAULT_METRICS) + ["avg"]
    for m in DEFAULT_METRICS:
        assert set(res[m]) == {"KL", "OA", "OA_err", "degenerate", "mean", "std"} and not res[m]["degenerate"]
        assert res[m]["mean"].shape == res[m]["std"].shape == ((12,) if m == "total_pitch_class_histogram" else (1,))
    assert res["avg"]["KL"] == np.mean([res[m]["KL"] for m in DEFAULT_METRICS])
    assert res["note_density"]["mean"][0] == s1["note_density_mgeval"].mean()
    # a constant statistic: flagged, NaN, left out of avg; the transition matrix is taken when asked for
    s1c = dict(s1, total_used_pitch=np.full(20, 9))
    res = evaluate_sets_np(s1c, s2, metrics=("total_used_pitch", "pitch_range", "pitch_class_transition_matrix"), kl_points=200, oa_panels=512)
    assert res["total_used_pitch"]["degenerate"] and np.isnan(res["total_used_pitch"]["KL"])
    assert res["avg"]["OA"] == np.mean([res["pitch_range"]["OA"], res["pitch_class_transition_matrix"]["OA"]])
    assert res["pitch_class_transition_matrix"]["mean"].shape == (144,)
    with pytest.raises(KeyError):
        evaluate_sets_np(s1, s2, metrics=("bar_pitch_class_histogram",))
    # the full-size answer for one metric is the fixture's case
    one = evaluate_sets_np(s1, s2, metrics=("pitch_range",))
    assert abs(one["pitch_range"]["OA"] - sc.scalar(gold, "real.pitch_range", "OA")) <= max(sc.scalar(gold, "real.pitch_range", "quad_abserr"), 1.49e-8)


def test_the_library_exports_and_binds_the_new_entry_points():
    import __graft_entry__ as ge
    ge.build()
    from rgm import native as R
    for name in ("rgm_set_distances", "rgm_kde_pdf", "rgm_kde_pdf_workspace", "rgm_set_kl_oa", "rgm_set_kl_oa_workspace"):
        assert getattr(R.lib, name).argtypes is not None
    ws = R.lib.rgm_set_kl_oa_workspace
    assert ws(132, 144, 1000, 16384) == 128 + 16 * 2 * 17385 and ws(9120, 16385, 1000, 16384) == 128 + 16 * 3 * 17385
    assert ws(1, 144, 1000, 16384) == 0 and ws(132, 2 ** 24 + 1, 1000, 16384) == 0 and ws(132, 144, 4097, 16384) == 0
    assert ws(132, 144, 1000, 16383) == 0 and ws(132, 144, 1000, 65538) == 0 and ws(2, 2, 2, 2) > 0
    assert R.lib.rgm_kde_pdf_workspace(65, 4097) == 64 + 8 * 4097 and R.lib.rgm_kde_pdf_workspace(0, 5) == 0


def test_device_surface_refuses_host_tensors_and_other_modes():
    import torch
    from music_evaluation import set_eval
    from music_evaluation.mgeval import utils
    from rgm.native import RgmError
    with pytest.raises(NotImplementedError):
        utils.c_dist(torch.zeros(1, 3), torch.zeros(4, 3), mode="EMD")
    with pytest.raises(NotImplementedError):
        utils.c_dist(torch.zeros(1, 3), torch.zeros(4, 3), mode="KL", normalize=1)
    with pytest.raises(RgmError):
        utils.kl_dist(torch.zeros(5, dtype=torch.float64), torch.ones(5, dtype=torch.float64))
    with pytest.raises(RgmError):
        set_eval.set_distances(torch.zeros(3, 1), torch.zeros(3, 1))
    with pytest.raises(RgmError):
        set_eval.evaluate_sets({"m": torch.zeros(3, dtype=torch.float64)}, {"m": torch.ones(3, dtype=torch.float64)}, metrics=("m",))


def _host_note_stats(rolls):
    from music_rule_guidance.piano_roll_to_chord import piano_roll_note_stats
    rows = [piano_roll_note_stats(r, first_column_onsets=True) for r in rolls]
    return {k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0]}


def _host_evaluate(s1, s2, metrics):
    from music_evaluation.set_eval import evaluate_sets_np
    return evaluate_sets_np(s1, s2, metrics, kl_points=100, oa_panels=256)


def _cli():
    spec = importlib.util.spec_from_file_location("eval_sets_cli", os.path.join(PKG, "scripts", "eval_sets.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def save_rolls(directory, T, count, seed):
    os.makedirs(directory, exist_ok=True)
    rolls = []
    for i in range(count):
        rolls.append(nc.random_roll(seed + i, 3, T))
        np.save(os.path.join(directory, f"sample_{i}_y_1.npy"), rolls[-1])
    return rolls


def read_csv(path):
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    return rows[0], {r[0]: (float(r[1]), float(r[2])) for r in rows[1:]}, [r[0] for r in rows[1:]]


def test_cli_writes_the_reference_layout_and_the_seed_repeats(tmp_path, capsys):
    from music_evaluation.set_eval import DEFAULT_METRICS
    cli = _cli()
    d1, d2 = str(tmp_path / "gen"), str(tmp_path / "base")
    rolls1 = save_rolls(d1, 64, 5, 100) + [nc.random_roll(300, 3, 96)]
    np.save(os.path.join(d1, "sample_5_y_1.npy"), rolls1[-1])                   # another length: its own group
    rolls2 = save_rolls(d2, 64, 7, 200)
    argv = ["--set1dir", d1, "--set2dir", d2, "--outdir", str(tmp_path / "out"), "--num_sample", "5", "--num_runs", "3"]
    res = cli.main(argv + ["--seed", "4"], note_stats_fn=_host_note_stats, evaluate_fn=_host_evaluate)
    header, mean, order = read_csv(str(tmp_path / "out" / "gen.base.mean.csv"))
    assert header == ["attribute", "KL", "OA"] and order == list(DEFAULT_METRICS) + ["avg"]
    _, std, order_std = read_csv(str(tmp_path / "out" / "gen.base.std.csv"))
    assert order_std == order
    assert res["KL"].shape == (3, 8)
    for j, a in enumerate(order):
        assert mean[a] == (float(np.mean(res["KL"][:, j])), float(np.mean(res["OA"][:, j])))
        assert std[a] == (float(np.std(res["KL"][:, j])), float(np.std(res["OA"][:, j])))
    ok = [j for j in range(7) if not np.isnan(res["KL"][0, j])]
    assert ok and res["KL"][0, 7] == np.mean(res["KL"][0, ok]) and res["OA"][0, 7] == np.mean(res["OA"][0, ok])
    assert np.unique(res["OA"][:, :7], axis=0).shape[0] > 1                    # the runs draw different subsets of set 1
    meta = json.load(open(str(tmp_path / "out" / "run_metadata.json")))
    assert meta["seed"] == 4 and meta["num_runs"] == 3 and meta["files"] == [6, 7] and meta["samples_in_use"] == [5, 5, 5]
    again = cli.main(argv + ["--seed", "4", "--savename", "x"], note_stats_fn=_host_note_stats, evaluate_fn=_host_evaluate)
    assert np.array_equal(res["KL"], again["KL"], equal_nan=True) and np.array_equal(res["OA"], again["OA"], equal_nan=True)
    assert os.path.exists(str(tmp_path / "out" / "x_mean.csv")) and os.path.exists(str(tmp_path / "out" / "x_std.csv"))
    other = cli.main(argv + ["--seed", "5"], note_stats_fn=_host_note_stats, evaluate_fn=_host_evaluate)
    assert not np.array_equal(res["OA"], other["OA"], equal_nan=True)
    # all files, one run: the statistics reach the evaluation in file order, whatever their lengths
    got = {}

    def spy(s1, s2, metrics):
        got["s1"], got["s2"] = s1, s2
        return _host_evaluate(s1, s2, metrics)
    cli.main(["--set1dir", d1, "--set2dir", d2, "--outdir", str(tmp_path / "out2")], note_stats_fn=_host_note_stats, evaluate_fn=spy)
    want1, want2 = _host_note_stats(rolls1[:5]), _host_note_stats(rolls2)
    last = _host_note_stats(rolls1[5:])
    # every file once, under one permutation for all statistics (one run over all files: 6 of set 1 against 6 of the 7 of set 2)
    for key in ("mean_note_duration", "n_notes"):
        pool = [tuple(np.ravel(v)) for v in want1[key]] + [tuple(np.ravel(v)) for v in last[key]]
        assert sorted(tuple(np.ravel(v)) for v in got["s1"][key]) == sorted(pool)
    rows1 = list(zip(got["s1"]["n_notes"].tolist(), got["s1"]["mean_note_duration"].tolist()))
    assert sorted(rows1) == sorted(zip(want1["n_notes"].tolist() + last["n_notes"].tolist(),
                                       want1["mean_note_duration"].tolist() + last["mean_note_duration"].tolist()))
    assert len(got["s2"]["n_notes"]) == 6 and set(got["s2"]["n_notes"].tolist()) <= set(want2["n_notes"].tolist())
    # a constant statistic: nan in the file, named on stderr, left out of avg
    capsys.readouterr()

    def constant(rolls):
        s = _host_note_stats(rolls)
        s["pitch_range"] = np.full_like(s["pitch_range"], 40)
        return s
    res = cli.main(argv + ["--savename", "c"], note_stats_fn=constant, evaluate_fn=_host_evaluate)
    assert "pitch_range" in capsys.readouterr().err and res["degenerate"][0] == ["pitch_range"]
    _, mean, _ = read_csv(str(tmp_path / "out" / "c_mean.csv"))
    assert np.isnan(mean["pitch_range"][0]) and np.isnan(mean["pitch_range"][1]) and np.isfinite(mean["avg"][0])
