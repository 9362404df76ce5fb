"""The set-level half of mgeval on the device (csrc/sets.hip; docs/rounds/sets.md): what the reference's music_evaluation/music_evaluator.py
computes from two sets of per-sample statistics -- leave-one-out intra-set and inter-set Euclidean distances per statistic, then the KL
divergence and the overlap area of the Gaussian-KDE densities of the set-1 intra distances and the inter distances -- without leaving
the device, plus a numpy host partner of the whole chain written from the same definition (the A/B partner of the tests; no scipy).

    evaluate_sets(stats1, stats2)       two note_stats dicts (or {metric: (N, d) tensor}) -> KL / OA per metric and their `avg` row
    set_distances(x1, x2)               (intra1, intra2, inter), flattened, NaN and inf already 0
    kde_pdf(data, x), kl_oa(A, B)       the two kernels' entry points on tensors
    set_distances_np, kde_pdf_np, kl_oa_np, evaluate_sets_np      the host partner

Differences from the reference: the overlap area is a composite Simpson rule on 16384 panels in place of QUADPACK's adaptive rule (its
own error estimate |OA(16384) - OA(8192)| is returned as OA_err); a statistic that is constant over a set makes the reference raise
LinAlgError and is reported here as degenerate with KL = OA = NaN; the statistics are those of the in-memory rolls, not of MIDI files
read back (docs/rounds/notes.md)."""
import math

import numpy as np

DEFAULT_METRICS = ("total_used_pitch", "pitch_range", "avg_IOI", "total_pitch_class_histogram", "mean_note_velocity",
                   "mean_note_duration", "note_density")
KL_POINTS = 1000
OA_PANELS = 16384
SQRT_2PI = 2.5066282746310002
OUT_FIELDS = ("KL", "OA", "OA_err", "h_A", "h_B", "lo", "hi", "degenerate")


def _key(stats, metric):
    """the reference's `note_density` is mgeval's notes per second, which note_stats returns as note_density_mgeval"""
    if metric == "note_density" and "note_density_mgeval" in stats:
        return "note_density_mgeval"
    if metric not in stats:
        raise KeyError(f"statistic {metric!r} is not in the set ({sorted(stats)})")
    return metric


# ---------------------------------------------------------------------------------------------------------------- host partner (numpy)
def _feature_np(stats, metric):
    v = np.asarray(stats[_key(stats, metric)], dtype=np.float64)
    return v.reshape(v.shape[0], -1)


def _distances_np(a, b, skip_diagonal):
    s = np.zeros((a.shape[0], b.shape[0]))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(a.shape[1]):                     # summed in k order, as the kernel does
            x = a[:, None, k] - b[None, :, k]
            s += x * x
        r = np.sqrt(s)
    r[~np.isfinite(r)] = 0.0                            # music_evaluator.delete_nan
    if skip_diagonal:
        r = r[~np.eye(a.shape[0], dtype=bool)].reshape(a.shape[0], a.shape[0] - 1)
    return r.reshape(-1)


def set_distances_np(x1, x2):
    """(N, d) and (N, d) float64 -> (intra1 N (N - 1), intra2 N (N - 1), inter N N): row i of an intra vector holds the distances to the
    samples j != i in ascending j, the layout of the reference's leave-one-out loop after its transpose and reshape"""
    x1, x2 = np.asarray(x1, dtype=np.float64), np.asarray(x2, dtype=np.float64)
    x1, x2 = x1.reshape(x1.shape[0], -1), x2.reshape(x2.shape[0], -1)
    return _distances_np(x1, x1, True), _distances_np(x2, x2, True), _distances_np(x1, x2, False)


def bandwidth_np(y):
    """-> (h, degenerate): Scott's bandwidth sqrt(sum (y - mean)^2 / (n - 1)) n^(-1/5)"""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n = y.size
    if n < 2:
        return float("nan"), True
    mean = y.sum() / n
    var = ((y - mean) ** 2).sum() / (n - 1)
    h = math.sqrt(var) * float(n) ** -0.2 if var >= 0 else float("nan")
    return h, not (var > 0 and math.isfinite(var) and h > 0)


def kde_pdf_np(data, x, rows=256):
    """scipy.stats.gaussian_kde(data)(x) for one-dimensional data, with (x - y) / h formed per pair; NaN everywhere for n < 2 or a zero
    variance.  Equal data values are taken together (count * exp): distances of integer statistics have a few dozen distinct values
    whatever n is"""
    y = np.asarray(data, dtype=np.float64).reshape(-1)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    h, bad = bandwidth_np(y)
    out = np.full(x.shape, np.nan)
    if bad:
        return out
    den = y.size * h * SQRT_2PI
    u, count = np.unique(y, return_counts=True)
    count = count.astype(np.float64)
    for i in range(0, x.size, rows):
        t = (x[i:i + rows, None] - u[None, :]) / h
        out[i:i + rows] = (count * np.exp(-0.5 * t * t)).sum(axis=1) / den
    return out


def rel_entr_np(p, q):
    """scipy.special.rel_entr"""
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where((p > 0) & (q > 0), p * np.log(p / q), np.where((p == 0) & (q >= 0), 0.0, np.inf))
    return np.where(np.isnan(p) | np.isnan(q), np.nan, out)


def simpson_np(m, lo, hi):
    """composite Simpson rule of the samples m on len(m) - 1 (even) panels over [lo, hi]"""
    step = (hi - lo) / (m.size - 1)
    return step / 3.0 * ((m[0] + m[-1]) + 4.0 * m[1:-1:2].sum() + 2.0 * m[2:-1:2].sum())


def kl_oa_np(A, B, kl_points=KL_POINTS, oa_panels=OA_PANELS):
    """-> the 8 doubles of rgm_set_kl_oa: KL, OA, OA_err, h_A, h_B, lo, hi, flag"""
    A, B = np.asarray(A, dtype=np.float64).reshape(-1), np.asarray(B, dtype=np.float64).reshape(-1)
    if A.size < 2 or B.size < 2 or kl_points < 2 or oa_panels < 2 or oa_panels % 2:
        raise ValueError("kl_oa needs two vectors of at least two values, at least two KL points and an even number of panels")
    (hA, badA), (hB, badB) = bandwidth_np(A), bandwidth_np(B)
    lo, hi = min(A.min(), B.min()), max(A.max(), B.max())
    if badA or badB:
        return np.array([np.nan, np.nan, np.nan, hA, hB, lo, hi, 1.0])
    p = kde_pdf_np(A, np.linspace(A.min(), A.max(), kl_points))
    q = kde_pdf_np(B, np.linspace(B.min(), B.max(), kl_points))
    kl = rel_entr_np(p / p.sum(), q / q.sum()).sum()
    grid = np.linspace(lo, hi, oa_panels + 1)
    m = np.minimum(kde_pdf_np(A, grid), kde_pdf_np(B, grid))
    oa = simpson_np(m, lo, hi)
    err = abs(oa - simpson_np(m[::2], lo, hi)) if oa_panels % 4 == 0 else np.nan
    return np.array([kl, oa, err, hA, hB, lo, hi, 0.0])


def evaluate_sets_np(stats1, stats2, metrics=DEFAULT_METRICS, kl_points=KL_POINTS, oa_panels=OA_PANELS):
    """the host partner of evaluate_sets on numpy values: the same dict with Python floats / numpy arrays"""
    out = {}
    for metric in metrics:
        x1, x2 = _feature_np(stats1, metric), _feature_np(stats2, metric)
        n = min(x1.shape[0], x2.shape[0])
        if n < 2:
            raise ValueError(f"set evaluation needs at least two samples per set, got {x1.shape[0]} and {x2.shape[0]}")
        x1, x2 = x1[:n], x2[:n]
        intra1, _, inter = set_distances_np(x1, x2)
        r = kl_oa_np(intra1, inter, kl_points, oa_panels)
        out[metric] = {"KL": float(r[0]), "OA": float(r[1]), "OA_err": float(r[2]), "degenerate": bool(r[7]),
                       "mean": x1.mean(axis=0), "std": x1.std(axis=0)}
    ok = [m for m in metrics if not out[m]["degenerate"]]
    out["avg"] = {"KL": float(np.mean([out[m]["KL"] for m in ok])) if ok else float("nan"),
                  "OA": float(np.mean([out[m]["OA"] for m in ok])) if ok else float("nan")}
    return out


# ---------------------------------------------------------------------------------------------------------------------------- device
def _f64(t):
    import torch
    from rgm import native as R
    R.require_cuda(t)
    return t.detach().to(torch.float64).contiguous()


def _distances(a, b, skip_diagonal):
    import torch
    from rgm import native as R
    Na, d = a.shape
    Nb = b.shape[0]
    if b.shape[1] != d:
        raise ValueError(f"the two sets have {d} and {b.shape[1]} values per sample")
    out = torch.empty(Na * (Nb - 1 if skip_diagonal else Nb), dtype=torch.float64, device=a.device)
    with torch.cuda.device(a.device):
        R.check(R.lib.rgm_set_distances(R.ptr(a), Na, R.ptr(b), Nb, d, int(skip_diagonal), R.ptr(out), R.current_stream()))
    return out


def set_distances(x1, x2):
    """device tensors (N, d) and (N, d) -> (intra1, intra2, inter) float64 device vectors as set_distances_np lays them out, NaN and
    inf already replaced by 0; no host sync"""
    a = _f64(x1)
    b = _f64(x2)
    a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    if a.shape[0] < 2 or b.shape[0] < 2:
        raise ValueError(f"set distances need at least two samples per set, got {a.shape[0]} and {b.shape[0]}")
    return _distances(a, a, True), _distances(b, b, True), _distances(a, b, False)


def kde_pdf(data, x):
    """scipy.stats.gaussian_kde(data)(x) on the device: 1-d float64 tensors -> the density at x (NaN everywhere for n < 2 or a zero variance)"""
    import torch
    from rgm import native as R
    y = _f64(data)
    pts = _f64(x)
    y, pts = y.reshape(-1), pts.reshape(-1)
    out = torch.empty_like(pts)
    with torch.cuda.device(y.device):
        nbytes = R.lib.rgm_kde_pdf_workspace(y.numel(), pts.numel())
        if nbytes == 0:
            raise ValueError(f"kde_pdf takes 1 .. 2^24 data values and 1 .. 2^20 points, got {y.numel()} and {pts.numel()}")
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=y.device)
        R.check(R.lib.rgm_kde_pdf(R.ptr(y), y.numel(), R.ptr(pts), pts.numel(), R.ptr(out), R.ptr(ws), ws.numel() * 8, R.current_stream()))
    return out


def kl_oa(A, B, kl_points=KL_POINTS, oa_panels=OA_PANELS):
    """kl_dist(A, B, kl_points) and overlap_area(A, B) in one call -> (8,) float64 device tensor in the order of OUT_FIELDS; no host sync"""
    import torch
    from rgm import native as R
    a = _f64(A)
    b = _f64(B)
    a, b = a.reshape(-1), b.reshape(-1)
    out = torch.empty(8, dtype=torch.float64, device=a.device)
    with torch.cuda.device(a.device):
        nbytes = R.lib.rgm_set_kl_oa_workspace(a.numel(), b.numel(), int(kl_points), int(oa_panels))
        if nbytes == 0:
            raise ValueError(f"kl_oa takes 2 .. 2^24 values per vector, 2 .. 4096 KL points and an even 2 .. 65536 panels, got "
                             f"{a.numel()}, {b.numel()}, {kl_points}, {oa_panels}")
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=a.device)
        R.check(R.lib.rgm_set_kl_oa(R.ptr(a), a.numel(), R.ptr(b), b.numel(), int(kl_points), int(oa_panels), R.ptr(out), R.ptr(ws),
                                    ws.numel() * 8, R.current_stream()))
    return out


def evaluate_sets(stats1, stats2, metrics=DEFAULT_METRICS, kl_points=KL_POINTS, oa_panels=OA_PANELS):
    """stats1, stats2: two dicts as music_rules.note_stats returns them, or {metric: (N, d) device tensor}.  Both sets are cut to the
    smaller N, as the reference does.  -> {metric: {"KL", "OA", "OA_err", "degenerate", "mean", "std"}, "avg": {"KL", "OA"}} of
    device tensors: KL and OA of the set-1 intra distances against the inter distances (music_evaluator.py:174-175), mean and
    (population) std of set 1's statistic, and the mean of KL and of OA over the metrics that are not degenerate.  Nothing is copied to
    the host.  pitch_class_transition_matrix (d = 144) is accepted when asked for."""
    import torch
    from rgm import native as R
    out = {}
    for metric in metrics:
        x1 = stats1[_key(stats1, metric)]
        x2 = stats2[_key(stats2, metric)]
        R.require_cuda(x1, x2)
        x1, x2 = x1.reshape(x1.shape[0], -1), x2.reshape(x2.shape[0], -1)
        n = min(x1.shape[0], x2.shape[0])
        if n < 2:
            raise ValueError(f"set evaluation needs at least two samples per set, got {x1.shape[0]} and {x2.shape[0]}")
        x1, x2 = x1[:n].to(torch.float64), x2[:n].to(torch.float64)
        a, b = x1.contiguous(), x2.contiguous()
        r = kl_oa(_distances(a, a, True), _distances(a, b, False), kl_points, oa_panels)
        out[metric] = {"KL": r[0], "OA": r[1], "OA_err": r[2], "degenerate": r[7] != 0, "mean": x1.mean(dim=0), "std": x1.std(dim=0, unbiased=False)}
    kl = torch.stack([out[m]["KL"] for m in metrics])
    oa = torch.stack([out[m]["OA"] for m in metrics])
    out["avg"] = {"KL": torch.nanmean(kl), "OA": torch.nanmean(oa)}
    return out
