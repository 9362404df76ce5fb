"""-m gpu: the set-level mgeval evaluation on the device (csrc/sets.hip: rgm_set_distances, rgm_kde_pdf, rgm_set_kl_oa) against the
reference's answers and the 80-bit evaluation in tests/golden/sets.npz, through the ABI, through music_evaluation.set_eval and
music_evaluation.mgeval.utils, from note_stats without a host copy, and from scripts/eval_sets.py.  Comparison rules
(docs/rounds/sets.md, sets_cases.check_distances / check_kl_oa): distances exact at d = 1 and within (d + 2) 2^-53 beyond, zeros exact,
bandwidths within 8 2^-53, densities no worse than the reference's own error against the 80-bit values, KL within eps (S + 2), OA
within quad's tolerance of the reference and within (eps + 32 2^-53) OA of the 80-bit Simpson value.

The file name puts these tests behind the test_gpu_* files, like tests/test_rule_notes_gpu.py."""
import numpy as np
import pytest
import torch

import notes_cases as nc
import sets_cases as sc
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return load_golden("sets")


@pytest.fixture(scope="module")
def notes_gold():
    return load_golden("notes")


@pytest.fixture(scope="module")
def cases(notes_gold):
    return sc.cases(notes_gold)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).cuda()


def _abi_distances(a, b, skip):
    from rgm import native as R
    ta, tb = dev(a), dev(b)
    out = torch.full((a.shape[0] * (b.shape[0] - 1 if skip else b.shape[0]),), -1.0, dtype=torch.float64, device="cuda")
    R.check(R.lib.rgm_set_distances(R.ptr(ta), a.shape[0], R.ptr(tb), b.shape[0], a.shape[1], int(skip), R.ptr(out), R.current_stream()))
    return out.cpu().numpy()


def _abi_kl_oa(A, B, kl_points=sc.KL_POINTS, panels=sc.OA_PANELS):
    from rgm import native as R
    ta, tb = dev(A), dev(B)
    nbytes = R.lib.rgm_set_kl_oa_workspace(ta.numel(), tb.numel(), kl_points, panels)
    assert nbytes > 0
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")
    out = torch.full((8,), -1.0, dtype=torch.float64, device="cuda")
    R.check(R.lib.rgm_set_kl_oa(R.ptr(ta), ta.numel(), R.ptr(tb), tb.numel(), kl_points, panels, R.ptr(out), R.ptr(ws), nbytes, R.current_stream()))
    return out.cpu().numpy()


def test_every_case_through_the_abi(gold, cases):
    """distances from the feature matrices, then densities, KL and OA from the FIXTURE's distance vectors, so that every rule is checked
    against the reference's inputs"""
    from music_evaluation.set_eval import kde_pdf
    for name, (x1, x2) in cases.items():
        got = (_abi_distances(x1, x1, True), _abi_distances(x2, x2, True), _abi_distances(x1, x2, False))
        worst = sc.check_distances(got, gold, name, x1.shape[1])
        if x1.shape[1] > 1:
            print(f"{name}: distances off by at most {worst:.2e} relative (bound {(x1.shape[1] + 2) * sc.U:.2e})")
        A, B = gold[f"{name}.intra1"], gold[f"{name}.inter"]
        sA, sB = sc.kl_points(gold, name)
        sc.check_kl_oa(_abi_kl_oa(A, B), kde_pdf(dev(A), dev(sA)).cpu().numpy(), kde_pdf(dev(B), dev(sB)).cpu().numpy(), gold, name, "kernel")


def test_every_case_through_evaluate_sets_and_the_reference_names(gold, cases):
    from music_evaluation.mgeval import utils
    from music_evaluation.set_eval import evaluate_sets, set_distances
    names = list(cases)
    for name, (x1, x2) in cases.items():
        res = evaluate_sets({"m": dev(x1)}, {"m": dev(x2)}, metrics=("m",))
        r = res["m"]
        assert all(r[k].is_cuda for k in r) and r["KL"].dim() == 0 and r["KL"].dtype == torch.float64 and r["mean"].shape == (x1.shape[1],)
        s = {f: sc.scalar(gold, name, f) for f in sc.SCALARS}
        if str(gold["raises"][names.index(name)]):
            assert bool(r["degenerate"]) and torch.isnan(r["KL"]) and torch.isnan(r["OA"]) and torch.isnan(res["avg"]["KL"])
            continue
        assert not bool(r["degenerate"])
        eps = sc.reference_density_error(gold, name)
        print(f"evaluate_sets {name}: KL off by {abs(float(r['KL']) - s['KL80']):.2e} (bound {eps * (s['S80'] + 2):.2e}), OA off quad by "
              f"{abs(float(r['OA']) - s['OA']):.2e} (bound {max(s['quad_abserr'], 1.49e-8):.2e}), OA_err {float(r['OA_err']):.2e}")
        assert abs(float(r["KL"]) - s["KL80"]) <= eps * (s["S80"] + 2)
        assert abs(float(r["OA"]) - s["OA"]) <= max(s["quad_abserr"], 1.49e-8)
        assert float(res["avg"]["KL"]) == float(r["KL"]) and float(res["avg"]["OA"]) == float(r["OA"])
        with np.errstate(invalid="ignore"):
            assert np.allclose(r["mean"].cpu().numpy(), x1.mean(axis=0), rtol=1e-14, atol=0, equal_nan=True)
            assert np.allclose(r["std"].cpu().numpy(), x1.std(axis=0), rtol=1e-12, equal_nan=True)
    # the reference's three names
    x1, x2 = cases["dirichlet.n12"]
    intra1, intra2, inter = (t.cpu().numpy() for t in set_distances(dev(x1), dev(x2)))
    sc.check_distances((intra1, intra2, inter), gold, "dirichlet.n12", 12)
    row = utils.c_dist(dev(x1[[3]]), dev(x2))
    assert row.shape == (12,) and row.dtype == torch.float64 and np.array_equal(row.cpu().numpy(), inter[36:48])
    A, B = dev(gold["gamma.n40.intra1"]), dev(gold["gamma.n40.inter"])
    kl, oa = utils.kl_dist(A, B), utils.overlap_area(A, B)
    ref = _abi_kl_oa(gold["gamma.n40.intra1"], gold["gamma.n40.inter"])
    assert kl.dim() == 0 and float(kl) == ref[0] and float(oa) == ref[1]
    assert float(utils.kl_dist(A, B, num_sample=77)) != ref[0]


def test_kde_pdf_at_the_wave_and_tile_edges_against_the_host_partner():
    """n = 2, 3, 63, 64, 65 data values at m = 1, 1000, 4097 points within [min - h, max + h].  Kernel and host partner form the same
    t = (x - y) / h in IEEE arithmetic from bandwidths within 4 2^-53 of the exact one each, so a term differs by (1 + t^2) 8 2^-53 from
    h, by 2 2^-53 from the two exp (1 ulp each), and the sum (compensated here, pairwise there: 1 + log2 n roundings) and the
    scaling add at most 12 2^-53: the bound is (14 + 8 (1 + t_max^2)) 2^-53 relative"""
    from music_evaluation.set_eval import bandwidth_np, kde_pdf, kde_pdf_np
    rng = np.random.RandomState(4100)
    for n in (2, 3, 63, 64, 65):
        y = rng.gamma(2.0, 1.5, size=n)
        h, bad = bandwidth_np(y)
        assert not bad
        for m in (1, 1000, 4097):
            x = rng.uniform(y.min() - h, y.max() + h, size=m)
            got = kde_pdf(dev(y), dev(x)).cpu().numpy()
            want = kde_pdf_np(y, x)
            tmax = (y.max() - y.min() + h) / h
            bound = (14 + 8 * (1 + tmax * tmax)) * sc.U
            rel = float((np.abs(got - want) / want).max())
            print(f"kde_pdf n = {n}, m = {m}: off the host partner by {rel:.2e} relative (bound {bound:.2e})")
            assert got.shape == (m,) and rel <= bound
    assert torch.isnan(kde_pdf(dev([2.0, 2.0, 2.0]), dev([1.0, 2.0, 3.0]))).all()      # zero variance
    assert torch.isnan(kde_pdf(dev([2.0]), dev([1.0, 2.0]))).all()                     # n < 2


def test_a_density_does_not_depend_on_the_tile_shape_of_its_launch():
    """700 points over 20000 data values (two chunks) run in one-wave workgroups of 64 points; the same points repeated 800 times make a
    grid large enough for the 512-point workgroups: every copy has the bits of the small launch, and the small launch is the host
    partner's density within sets_cases.partner_density_bound"""
    from music_evaluation.set_eval import kde_pdf, kde_pdf_np
    rng = np.random.RandomState(4200)
    yn, xn = rng.gamma(2.0, 1.5, size=20000), rng.uniform(0.0, 12.0, size=700)
    y, x = dev(yn), dev(xn)
    small = kde_pdf(y, x)
    big = kde_pdf(y, x.repeat(800)).reshape(800, 700)
    assert torch.isfinite(small).all() and (small > 0).all()
    assert torch.equal(big, small[None].expand(800, 700))
    want, bound = kde_pdf_np(yn, xn), sc.partner_density_bound(yn, xn)
    rel = np.abs(small.cpu().numpy() - want) / want
    print(f"two chunks, 700 points: off the host partner by {rel.max():.2e} relative (bound {bound.min():.2e} .. {bound.max():.2e})")
    assert (rel <= bound).all()


def _grid_values(rng, n, p):
    """n values on a grid of 40 (0.25 k, k binomial): as many as a few hundred samples per set give, at a host cost that does not grow
    with n, because the host partner takes equal values together"""
    return 0.25 * rng.binomial(39, p, size=n).astype(np.float64)


def test_several_ragged_chunks_of_different_counts_against_the_host_partner():
    """Sizes the fixture does not hold.  A has 40000 values (3 chunks of 16384, the last 7232), B 70000 (5 chunks, the last 4464): the
    two densities of rgm_set_kl_oa have different chunk counts, and with 4096 KL points and 65536 panels the grid (137 tiles x 8
    chunks) takes the 512-point workgroups.  rgm_kde_pdf on B at 110000 points (215 tiles x 5 chunks) takes them too.  Yardstick: the
    host partner.  Densities within partner_density_bound (d); KL within d (S + 2) and OA within (d + 32 2^-53) OA, the forms of the
    fixture's rules with the partner's bound in place of eps; bandwidths within 32 2^-53"""
    from music_evaluation.set_eval import kde_pdf, kde_pdf_np, kl_oa_np, rel_entr_np
    rng = np.random.RandomState(4300)
    A, B = _grid_values(rng, 40000, 0.4), _grid_values(rng, 70000, 0.55)
    want = kl_oa_np(A, B, 4096, 65536)
    h = want[4]
    x = rng.uniform(B.min() - h, B.max() + h, size=110000)
    pdf, pdf_want, bound = kde_pdf(dev(B), dev(x)).cpu().numpy(), kde_pdf_np(B, x), sc.partner_density_bound(B, x)
    rel = np.abs(pdf - pdf_want) / pdf_want
    print(f"kde_pdf n = 70000, m = 110000: off the host partner by {rel.max():.2e} relative (bound {bound.min():.2e} .. {bound.max():.2e})")
    assert (pdf_want > 0).all() and (rel <= bound).all()
    got = _abi_kl_oa(A, B, 4096, 65536)
    sA, sB = np.linspace(A.min(), A.max(), 4096), np.linspace(B.min(), B.max(), 4096)
    grid = np.linspace(want[5], want[6], 65537)
    d_kl = max(sc.partner_density_bound(A, sA).max(), sc.partner_density_bound(B, sB).max())
    d_oa = max(sc.partner_density_bound(A, grid).max(), sc.partner_density_bound(B, grid).max())
    p, q = kde_pdf_np(A, sA), kde_pdf_np(B, sB)
    S = float(np.abs(rel_entr_np(p / p.sum(), q / q.sum())).sum())
    print(f"kl_oa n = 40000 / 70000: KL {got[0]!r} off the host partner by {abs(got[0] - want[0]):.2e} (bound {d_kl * (S + 2):.2e}), OA {got[1]!r} "
          f"off by {abs(got[1] - want[1]):.2e} (bound {(d_oa + 32 * sc.U) * want[1]:.2e}), OA_err {got[2]:.2e} (host {want[2]:.2e}), "
          f"h off by {abs(got[3] / want[3] - 1):.2e} and {abs(got[4] / want[4] - 1):.2e}")
    assert got[7] == 0.0 and want[7] == 0.0 and np.isfinite(want[:3]).all() and 0.01 < want[1] < 0.99
    assert abs(got[3] / want[3] - 1) <= 32 * sc.U and abs(got[4] / want[4] - 1) <= 32 * sc.U
    assert got[5] == want[5] and got[6] == want[6]
    assert abs(got[0] - want[0]) <= d_kl * (S + 2)
    assert abs(got[1] - want[1]) <= (d_oa + 32 * sc.U) * want[1]


def test_three_samples_through_the_whole_chain_and_two_raise_the_flag():
    from music_evaluation.set_eval import evaluate_sets, evaluate_sets_np, kl_oa
    s1, s2 = {"m": np.array([1.0, 4.0, 9.0])}, {"m": np.array([2.0, 7.0, 8.0, 100.0])}
    want = evaluate_sets_np(s1, s2, metrics=("m",))["m"]
    got = evaluate_sets({"m": dev(s1["m"])}, {"m": dev(s2["m"])}, metrics=("m",))["m"]
    print(f"N = 3: KL {float(got['KL'])!r} (host {want['KL']!r}), OA {float(got['OA'])!r} (host {want['OA']!r})")
    # 6 and 9 distances, both sides the same formula in float64: 64 ulp of slack on values of order one
    assert not bool(got["degenerate"]) and abs(float(got["KL"]) - want["KL"]) <= 64 * sc.U * (1 + abs(want["KL"]))
    assert abs(float(got["OA"]) - want["OA"]) <= 64 * sc.U
    assert abs(float(got["mean"][0]) - want["mean"][0]) <= 4 * sc.U * want["mean"][0]      # torch's mean of three: a sum and a scaling
    two = evaluate_sets({"m": dev([1.0, 4.0])}, {"m": dev([2.0, 7.0])}, metrics=("m",))
    assert bool(two["m"]["degenerate"]) and torch.isnan(two["m"]["KL"]) and torch.isnan(two["m"]["OA"]) and torch.isnan(two["avg"]["OA"])
    out = kl_oa(dev([3.0, 3.0]), dev([1.0, 6.0, 2.0, 3.0])).cpu().numpy()
    assert out[7] == 1.0 and np.isnan(out[:3]).all() and out[3] == 0.0 and out[4] > 0 and out[5] == 1.0 and out[6] == 6.0


def test_twenty_launches_repeat_bit_for_bit(gold):
    A, B = gold["ints.n96.intra1"], gold["ints.n96.inter"]
    first = _abi_kl_oa(A, B)
    assert first[7] == 0.0 and np.isfinite(first).all()
    for _ in range(19):
        assert _abi_kl_oa(A, B).tobytes() == first.tobytes()


def test_a_metric_does_not_depend_on_the_metrics_it_shares_a_call_with(notes_gold):
    from music_evaluation.set_eval import DEFAULT_METRICS, evaluate_sets
    s1 = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in sc.notes_stats(notes_gold, 384).items()}
    s2 = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in sc.notes_stats(notes_gold, 1064).items()}
    every = evaluate_sets(s1, s2)
    assert list(every) == list(DEFAULT_METRICS) + ["avg"]
    alone = evaluate_sets(s1, s2, metrics=("mean_note_duration",))
    pair = evaluate_sets(s1, s2, metrics=("pitch_class_transition_matrix", "mean_note_duration"))
    for k in ("KL", "OA", "OA_err", "mean", "std"):
        a = every["mean_note_duration"][k].cpu().numpy().tobytes()
        assert a == alone["mean_note_duration"][k].cpu().numpy().tobytes() == pair["mean_note_duration"][k].cpu().numpy().tobytes()
    assert pair["pitch_class_transition_matrix"]["mean"].shape == (144,) and torch.isfinite(pair["pitch_class_transition_matrix"]["OA"])
    assert float(every["avg"]["KL"]) == pytest.approx(float(np.mean([float(every[m]["KL"]) for m in DEFAULT_METRICS])), rel=1e-14)


def test_arguments_are_checked_before_any_launch():
    from music_evaluation import set_eval
    from rgm import native as R
    a = torch.zeros((4, 3), dtype=torch.float64, device="cuda")
    out = torch.full((16,), -1.0, dtype=torch.float64, device="cuda")
    ws = torch.zeros(1 << 16, dtype=torch.int64, device="cuda")
    s = R.current_stream()
    assert R.lib.rgm_set_distances(R.ptr(a), 4, R.ptr(a), 4, 145, 0, R.ptr(out), s) != 0 and b"d = 145" in R.lib.rgm_last_error()
    assert R.lib.rgm_set_distances(R.ptr(a), 4, R.ptr(a), 4, 0, 0, R.ptr(out), s) != 0
    assert R.lib.rgm_set_distances(R.ptr(a), 4, R.ptr(a), 3, 3, 1, R.ptr(out), s) != 0 and b"diagonal" in R.lib.rgm_last_error()
    assert R.lib.rgm_set_distances(R.ptr(a), 0, R.ptr(a), 4, 3, 0, R.ptr(out), s) != 0
    assert R.lib.rgm_set_distances(None, 4, R.ptr(a), 4, 3, 0, R.ptr(out), s) != 0
    v = torch.arange(12, dtype=torch.float64, device="cuda")
    for nA, nB, kl, panels, nbytes in ((1, 12, 100, 64, 1 << 19), (12, 12, 1, 64, 1 << 19), (12, 12, 4097, 64, 1 << 19), (12, 12, 100, 63, 1 << 19),
                                       (12, 12, 100, 65538, 1 << 19), (12, 12, 100, 0, 1 << 19), (12, 12, 100, 64, 64)):
        assert R.lib.rgm_set_kl_oa(R.ptr(v), nA, R.ptr(v), nB, kl, panels, R.ptr(out), R.ptr(ws), nbytes, s) != 0, (nA, nB, kl, panels, nbytes)
    assert b"workspace" in R.lib.rgm_last_error()
    assert R.lib.rgm_kde_pdf(R.ptr(v), 12, R.ptr(v), 12, R.ptr(out), R.ptr(ws), 8, s) != 0 and b"workspace" in R.lib.rgm_last_error()
    assert R.lib.rgm_kde_pdf(R.ptr(v), 0, R.ptr(v), 12, R.ptr(out), R.ptr(ws), 1 << 19, s) != 0
    assert R.lib.rgm_kde_pdf(R.ptr(v), 12, R.ptr(v), 0, R.ptr(out), R.ptr(ws), 1 << 19, s) != 0
    torch.cuda.synchronize()
    assert (out == -1.0).all()                                                  # nothing was launched
    with pytest.raises(ValueError):
        set_eval.kl_oa(v, v, oa_panels=7)
    with pytest.raises(ValueError):
        set_eval.set_distances(v[:1].reshape(1, 1), v[:3].reshape(3, 1))
    with pytest.raises(ValueError):
        set_eval.evaluate_sets({"m": v[:1]}, {"m": v}, metrics=("m",))
    # oa_panels even but no multiple of 4: the rule at half the panels does not exist, OA does
    r = set_eval.kl_oa(v, v * 1.5, kl_points=50, oa_panels=66).cpu().numpy()
    assert np.isnan(r[2]) and 0 < r[1] <= 1 and r[7] == 0


def _rolls(T):
    return np.stack([nc.random_roll(nc.SEED + 20 * (3 * nc.RANDOM_T.index(T) + 2) + i, 3, T) for i in range(20)])


def test_note_stats_to_evaluate_sets_stays_on_the_device(gold, notes_gold):
    """the real case: the twenty T = 384 and twenty T = 1064 three-channel rolls of the note-statistics fixture through note_stats and
    evaluate_sets; between the two nothing synchronises with the host (torch's sync debug mode raises where something does)"""
    from music_evaluation.set_eval import DEFAULT_METRICS, evaluate_sets
    from music_rule_guidance import music_rules
    cases = nc.cases()
    for T in (384, 1064):
        assert np.array_equal(_rolls(T)[7], cases[f"random.t{T}.c3.s7"])
    r1, r2 = torch.from_numpy(_rolls(384)).cuda(), torch.from_numpy(_rolls(1064)).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        s1 = music_rules.note_stats(r1, first_column_onsets=True)
        s2 = music_rules.note_stats(r2, first_column_onsets=True)
        res = evaluate_sets(s1, s2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for m in DEFAULT_METRICS:
        name = "real." + m
        s = {f: sc.scalar(gold, name, f) for f in sc.SCALARS}
        eps = sc.reference_density_error(gold, name)
        kl, oa = float(res[m]["KL"]), float(res[m]["OA"])
        print(f"{name}: KL {kl:.6g} off by {abs(kl - s['KL80']):.2e} (bound {eps * (s['S80'] + 2):.2e}), OA {oa:.9f} off quad by "
              f"{abs(oa - s['OA']):.2e} (bound {max(s['quad_abserr'], 1.49e-8):.2e})")
        assert not bool(res[m]["degenerate"]) and abs(kl - s["KL80"]) <= eps * (s["S80"] + 2)
        assert abs(oa - s["OA"]) <= max(s["quad_abserr"], 1.49e-8)


def test_eval_sets_cli_end_to_end_against_the_host_partner(tmp_path):
    from test_sets_host import _cli, _host_note_stats, read_csv, save_rolls
    from music_evaluation.set_eval import DEFAULT_METRICS, evaluate_sets_np
    cli = _cli()
    d1, d2 = str(tmp_path / "gen"), str(tmp_path / "base")
    save_rolls(d1, 64, 6, 100)
    np.save(d1 + "/sample_6_y_1.npy", nc.random_roll(300, 3, 96))
    save_rolls(d2, 64, 8, 200)
    argv = ["--set1dir", d1, "--set2dir", d2, "--num_sample", "6", "--num_runs", "2", "--seed", "3", "--savename", "t", "--batch_size", "4"]
    device = cli.main(argv + ["--outdir", str(tmp_path / "device")])
    host = cli.main(argv + ["--outdir", str(tmp_path / "host")], note_stats_fn=_host_note_stats,
                    evaluate_fn=lambda a, b, metrics: evaluate_sets_np(a, b, metrics))
    header, mean, order = read_csv(str(tmp_path / "device" / "t_mean.csv"))
    assert header == ["attribute", "KL", "OA"] and order == list(DEFAULT_METRICS) + ["avg"]
    assert np.array_equal(np.isnan(device["KL"]), np.isnan(host["KL"])) and device["degenerate"] == host["degenerate"]
    ok = ~np.isnan(host["KL"])
    print(f"CLI: KL off the host partner by {np.abs(device['KL'] - host['KL'])[ok].max():.2e}, OA by {np.abs(device['OA'] - host['OA'])[ok].max():.2e}")
    # 30 and 36 distances per metric; the same formulas in float64 on both sides, KL of order one and OA <= 1
    assert np.abs(device["KL"] - host["KL"])[ok].max() <= 1e-12 and np.abs(device["OA"] - host["OA"])[ok].max() <= 1e-12
    for j, a in enumerate(order):
        assert np.isnan(mean[a][0]) or mean[a] == (float(np.mean(device["KL"][:, j])), float(np.mean(device["OA"][:, j])))
