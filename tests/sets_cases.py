"""Inputs of the set-evaluation tests (docs/rounds/sets.md), shared by tests/golden/make_golden_sets.py, which asks the reference, and by
tests/test_sets_host.py / tests/test_rule_sets_gpu.py, which compare the host partner and the kernels with its answers.

cases(notes_gold) -> {name: (x1, x2)}, two (N, d) float64 feature matrices per case, in a fixed order: synthetic statistics rebuilt from
their seeds, and the seven statistics of the twenty T = 384 (set 1) and twenty T = 1064 (set 2) three-channel rolls of
tests/golden/notes.npz with first-column onsets, as the reference answered them there.  Only the seed and the reference's answers are
stored in tests/golden/sets.npz."""
import numpy as np

SEED = 8200
KINDS = ("ints", "gamma", "dirichlet", "nan20", "two_valued", "constant")
SIZES = (12, 40)
REAL_METRICS = ("total_used_pitch", "pitch_range", "avg_IOI", "total_pitch_class_histogram", "mean_note_velocity", "mean_note_duration",
                "note_density")
SCALARS = ("h_A", "h_B", "KL", "OA", "quad_abserr", "quad_neval", "KL80", "S80", "OA80", "eps")
KL_POINTS = 1000
OA_PANELS = 16384
# Draws replaced under the generator's rule (a case on which the host partner's Simpson value misses quad's tolerance is replaced, the
# bound is never widened): on the first gamma.n12 draw quad answers 1.3e-7 away from the 80-bit Simpson value while estimating its own
# error at 1.1e-8 (the integrand has kinks where the two densities cross); the rule at 16384 and at 8192 panels agrees to 3.7e-9 there.
RESEED = {"gamma.n12": 1000, "counts144.n12": 1000}


def _one(rng, kind, N):
    if kind == "ints":                                   # integers in 10 .. 39, like total_used_pitch: many tied distances
        return rng.randint(10, 40, size=(N, 1)).astype(np.float64)
    if kind == "gamma":
        return rng.gamma(2.0, 0.35, size=(N, 1))
    if kind == "dirichlet":                              # pitch-class histograms
        return rng.dirichlet(np.full(12, 0.7), size=N)
    if kind == "nan20":                                  # avg_IOI of samples with fewer than two notes
        x = rng.gamma(3.0, 0.2, size=(N, 1))
        x[rng.rand(N) < 0.2, 0] = np.nan
        return x
    if kind == "two_valued":                             # two clusters of distances, 0 and 64
        return rng.choice([32.0, 96.0], size=(N, 1))
    if kind == "constant":
        return np.full((N, 1), 57.0)
    if kind == "counts144":                              # transition matrices
        return rng.poisson(1.5, size=(N, 144)).astype(np.float64)
    raise KeyError(kind)


def synthetic():
    out = {}
    k = 0
    for N in SIZES:
        for kind in KINDS:
            rng = np.random.RandomState(SEED + k + RESEED.get(f"{kind}.n{N}", 0))
            k += 1
            x1 = _one(rng, kind, N)
            x2 = _one(rng, "ints" if kind == "constant" else kind, N)      # a constant set 1 against a varying set 2
            if kind == "nan20":
                x1[0, 0], x2[1, 0] = np.nan, np.nan      # at least one NaN on either side whatever the draw
            out[f"{kind}.n{N}"] = (x1, x2)
    rng = np.random.RandomState(SEED + 100 + RESEED.get("counts144.n12", 0))
    out["counts144.n12"] = (_one(rng, "counts144", 12), _one(rng, "counts144", 12))
    rng = np.random.RandomState(SEED + 101)                                   # 9120 and 9216 distances: ragged data chunks and point tiles
    out["ints.n96"] = (_one(rng, "ints", 96), _one(rng, "ints", 96))
    return out


def notes_stats(notes_gold, T, first_column_onsets=1):
    """the statistics of the twenty three-channel rolls of T columns in tests/golden/notes.npz, as a dict of numpy arrays under the keys of
    music_rules.note_stats"""
    names = [str(n) for n in notes_gold["names"]]
    idx = [names.index(f"random.t{T}.c3.s{i}") for i in range(20)]
    ints, real = notes_gold["ints"][idx, first_column_onsets], notes_gold["real"][idx, first_column_onsets]
    return {"n_notes": ints[:, 0], "total_used_pitch": ints[:, 1], "pitch_range": ints[:, 2], "mean_note_velocity": ints[:, 3],
            "end_time": real[:, 0], "avg_IOI": real[:, 1], "mean_note_duration": real[:, 2], "note_density_mgeval": real[:, 3],
            "total_pitch_class_histogram": real[:, 4:16], "pitch_class_transition_matrix": ints[:, 4:148].reshape(-1, 12, 12)}


def real(notes_gold):
    s1, s2 = notes_stats(notes_gold, 384), notes_stats(notes_gold, 1064)
    out = {}
    for m in REAL_METRICS:
        key = "note_density_mgeval" if m == "note_density" else m
        out[f"real.{m}"] = (np.asarray(s1[key], dtype=np.float64).reshape(20, -1), np.asarray(s2[key], dtype=np.float64).reshape(20, -1))
    return out


def cases(notes_gold):
    out = synthetic()
    out.update(real(notes_gold))
    return out


def reference_pdf(gold, name, which):
    """the reference's 1000-point density of case `name` (which: "A" or "B"), stored as its relative deviation from the 80-bit values"""
    x80 = gold[f"{name}.pdf80_{which}"]
    return x80 * (1.0 + gold[f"{name}.ref_dev_{which}"].astype(np.float64))


# ---- the comparison rules of docs/rounds/sets.md; each yardstick is the reference or the 80-bit evaluation, never the code under test
U = 2.0 ** -53


def index(gold, name):
    return [str(n) for n in gold["names"]].index(name)


def scalar(gold, name, field):
    return float(gold["scalars"][index(gold, name), SCALARS.index(field)])


def check_distances(got, gold, name, d):
    """d = 1: exact (sqrt(fl(x^2)) = |x|); d > 1: within (d + 2) 2^-53 relative; the zeros (NaN and inf are written as 0) exact"""
    worst = 0.0
    for key, g in zip(("intra1", "intra2", "inter"), got):
        ref = gold[f"{name}.{key}"]
        assert g.shape == ref.shape and g.dtype == np.float64, f"{name}.{key}: {g.dtype} {g.shape} != {ref.shape}"
        assert np.array_equal(g == 0, ref == 0), f"{name}.{key}: {int(((g == 0) != (ref == 0)).sum())} zeros differ"
        if d == 1:
            assert np.array_equal(g, ref), f"{name}.{key}: {int((g != ref).sum())} of {ref.size} distances differ, by up to {np.abs(g - ref).max():.3e}"
        else:
            rel = float((np.abs(g - ref) / np.maximum(ref, 1e-300)).max())
            worst = max(worst, rel)
            assert rel <= (d + 2) * U, f"{name}.{key}: off by {rel:.3e} relative, bound {(d + 2) * U:.3e}"
    return worst


def density_error(pdf, gold, name, which):
    """the worst relative error of a 1000-point density against the 80-bit values (as stored: rounded to float64, which is also the
    yardstick of the reference's own error below)"""
    x80 = gold[f"{name}.pdf80_{which}"]
    return float((np.abs(np.asarray(pdf, dtype=np.float64) - x80) / x80).max())


def reference_density_error(gold, name):
    """eps of the rules: the reference's worst relative density error against the 80-bit values, the float64 the generator stored (the
    float32 deviation arrays beside it are a record of where the error sits, not the bound)"""
    return scalar(gold, name, "eps")


def partner_density_bound(y, x):
    """Per point of x, how far rgm_kde_pdf may lie from kde_pdf_np, relative.  Both form the same t = (x - y) / h in IEEE arithmetic but
    from their own bandwidths.  The kernel's h carries about 4 roundings (compensated sums, sqrt, pow, product); numpy's pairwise sums
    of up to 2^17 values carry at most 16 + log2(n / 128) + 8 < 36 in the variance, half of that after the square root, plus pow and the
    product: the two bandwidths differ by less than 32 2^-53 relative (asserted where both are at hand).  A bandwidth off by d moves the
    term exp(-t^2 / 2) / h by (1 + t^2) d, hence the sum by the terms' weighted mean of it: (1 + G(x)) d with
    G = sum t^2 exp(-t^2 / 2) / sum exp(-t^2 / 2), evaluated here.  Two exp of 1 ulp each, the count product, the sums (compensated
    there, pairwise over the distinct values here) and the two scalings add at most 14 roundings.  -> (14 + 32 (1 + G)) 2^-53"""
    y, x = np.asarray(y, dtype=np.float64).reshape(-1), np.asarray(x, dtype=np.float64).reshape(-1)
    n = y.size
    h = np.sqrt(((y - y.mean()) ** 2).sum() / (n - 1)) * float(n) ** -0.2
    u, count = np.unique(y, return_counts=True)
    G = np.zeros(x.size)
    for i in range(0, x.size, 256):
        t2 = ((x[i:i + 256, None] - u[None, :]) / h) ** 2
        w = count * np.exp(-0.5 * t2)
        G[i:i + 256] = (w * t2).sum(axis=1) / w.sum(axis=1)
    return (14 + 32 * (1 + G)) * U


def check_kl_oa(out8, pdf_A, pdf_B, gold, name, what):
    """out8: the 8 doubles of rgm_set_kl_oa / kl_oa_np at 1000 points and 16384 panels; pdf_A, pdf_B: the two densities at the KL points.
    Prints every figure, then asserts the rules.  -> the figures"""
    out8 = np.asarray(out8, dtype=np.float64)
    if str(gold["raises"][index(gold, name)]):
        print(f"{what} {name}: flag {out8[7]}, KL {out8[0]}, OA {out8[1]} (the reference raises {gold['raises'][index(gold, name)]})")
        assert out8[7] == 1.0 and np.isnan(out8[0]) and np.isnan(out8[1]) and np.isnan(out8[2]), f"{name}: {out8}"
        return {}
    s = {f: scalar(gold, name, f) for f in SCALARS}
    eps = reference_density_error(gold, name)
    fig = {"h": max(abs(out8[3] / s["h_A"] - 1), abs(out8[4] / s["h_B"] - 1)),
           "density": max(density_error(pdf_A, gold, name, "A"), density_error(pdf_B, gold, name, "B")), "eps": eps,
           "KL": abs(out8[0] - s["KL80"]), "KL_bound": eps * (s["S80"] + 2),
           "OA_quad": abs(out8[1] - s["OA"]), "OA_quad_bound": max(s["quad_abserr"], 1.49e-8),
           "OA_arith": abs(out8[1] - s["OA80"]), "OA_arith_bound": (eps + 32 * U) * s["OA80"]}
    print(f"{what} {name}: h off by {fig['h']:.2e} (bound {8 * U:.2e}); density error {fig['density']:.2e} (the reference's {eps:.2e}); "
          f"KL off by {fig['KL']:.2e} (bound {fig['KL_bound']:.2e}); OA off quad by {fig['OA_quad']:.2e} (bound {fig['OA_quad_bound']:.2e}), "
          f"off the 80-bit Simpson by {fig['OA_arith']:.2e} (bound {fig['OA_arith_bound']:.2e}); OA_err {out8[2]:.2e}")
    assert out8[7] == 0.0, f"{name}: flag {out8[7]}"
    assert fig["h"] <= 8 * U, f"{name}: bandwidth off by {fig['h']:.3e} relative"
    assert fig["density"] <= eps, f"{name}: density error {fig['density']:.3e} above the reference's own {eps:.3e}"
    assert fig["KL"] <= fig["KL_bound"], f"{name}: KL {out8[0]!r} vs {s['KL80']!r}, bound {fig['KL_bound']:.3e}"
    assert fig["OA_quad"] <= fig["OA_quad_bound"], f"{name}: OA {out8[1]!r} vs quad {s['OA']!r} +- {s['quad_abserr']:.2e}"
    assert fig["OA_arith"] <= fig["OA_arith_bound"], f"{name}: OA {out8[1]!r} vs the 80-bit Simpson {s['OA80']!r}, bound {fig['OA_arith_bound']:.3e}"
    assert out8[5] == min(gold[f"{name}.intra1"].min(), gold[f"{name}.inter"].min()) and out8[6] == max(gold[f"{name}.intra1"].max(), gold[f"{name}.inter"].max())
    return fig


def kl_points(gold, name):
    A, B = gold[f"{name}.intra1"], gold[f"{name}.inter"]
    return np.linspace(A.min(), A.max(), KL_POINTS), np.linspace(B.min(), B.max(), KL_POINTS)
