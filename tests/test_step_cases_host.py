"""CPU: the references, restatements, measures and cases of tests/step_cases.py -- what tests/test_gpu_step_inputs.py holds the sampler, SCG,
rule and collage kernels to (docs/rounds/step_inputs.md).  Nothing here runs a kernel; RGM_STEP_HOST lines carry the document's figures."""
import json

import numpy as np
import pytest
import torch

import step_cases as sc
from conftest import load_golden
from oracle import collage_np, diffusion_np, rules_np

F32 = np.float32
DRIFT = 1.5            # another numpy's float32 libm may move a restatement's worst ratio; beyond this the recorded figure is stale


def _report(**kw):
    print("RGM_STEP_HOST " + json.dumps(kw))


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _holds(name, worst):
    _report(kind="restatement", name=name, worst=worst, recorded=sc.MEASURED[name], bound=sc.bound(name))
    assert np.isfinite(worst) and worst < 64, (name, worst)
    assert worst <= DRIFT * sc.MEASURED[name], (name, worst, "re-measure step_cases.MEASURED")
    assert sc.bound(name) >= sc.FACTOR * sc.MEASURED[name]


# ------------------------------------------------------------------------------------ 1. Philox
def test_philox_known_answers():
    for ctr, key, out in sc.KAT:
        got = sc.philox4x32_10([np.array([c], np.uint64) for c in ctr], key)
        assert [int(w[0]) for w in got] == list(out)


def test_stream_layout_and_the_2_34_boundary():
    seed = sc.SEEDS[2]
    ra, rb, sine = sc.stream_words(seed, 4, 8)                          # blocks 1 and 2, lanes 0..3
    w = sc.philox4x32_10([np.array([1, 2], np.uint64), np.zeros(2, np.uint64), np.zeros(2, np.uint64), np.zeros(2, np.uint64)],
                         (seed & 0xFFFFFFFF, seed >> 32))
    assert ra.tolist() == [int(w[0][0]), int(w[0][0]), int(w[2][0]), int(w[2][0]), int(w[0][1]), int(w[0][1]), int(w[2][1]), int(w[2][1])]
    assert rb.tolist() == [int(w[1][0]), int(w[1][0]), int(w[3][0]), int(w[3][0]), int(w[1][1]), int(w[1][1]), int(w[3][1]), int(w[3][1])]
    assert sine.tolist() == [False, True] * 4
    # across position 2^34 the block counter passes 2^32: the second counter word is 1, the first starts again at 0
    a = sc.stream_words(seed, sc.P34, 1)[0]
    hi = sc.philox4x32_10([np.zeros(1, np.uint64), np.ones(1, np.uint64), np.zeros(1, np.uint64), np.zeros(1, np.uint64)], (seed & 0xFFFFFFFF, seed >> 32))
    lo = sc.philox4x32_10([np.zeros(1, np.uint64)] * 4, (seed & 0xFFFFFFFF, seed >> 32))
    assert int(a[0]) == int(hi[0][0]) != int(lo[0][0])
    z, _ = sc.normals64(seed, sc.P34 - 513, 1027)
    for off, n in ((0, 7), (510, 9), (513, 1), (1000, 27)):
        assert np.array_equal(sc.normals64(seed, sc.P34 - 513 + off, n)[0], z[off:off + n])
    assert not np.array_equal(sc.normals64(sc.SEEDS[2], 0, 16)[0], sc.normals64(12345, 0, 16)[0])       # the seed's high word matters


def test_normals_are_standard_and_the_restatement_sets_the_bound():
    z, rad = sc.normals64(1, 0, 1 << 16)
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1) < 0.02 and np.isfinite(z).all() and rad.max() < 5.8      # sqrt(-2 ln 2^-24) = 5.77
    assert {(off % 4) for _, off, _ in sc.RANDN_CASES} == {0, 1, 2, 3} and {n for _, _, n in sc.RANDN_CASES} >= {1, 2, 3, 5, 1027}
    assert any(off < sc.P34 < off + n for _, off, n in sc.RANDN_CASES)
    worst = max(sc.randn_ratio(sc.normals32(s, off, n), s, off) for s, off, n in sc.RANDN_CASES)
    _holds("randn", worst)
    assert sc.RANDN_K == sc.FACTOR * sc.MEASURED["randn"]


# ------------------------------------------------------------------------------------ 2. SCG
def test_argmax_rule_is_torchs():
    cases = sc.select_cases()
    assert {"all_equal", "all_neg_inf", "inf_then_nan", "n1"} <= set(cases)
    for name, tot in cases.items():
        assert sc.argmax_first_nan(tot).tolist() == torch.argmax(torch.from_numpy(tot), dim=0).tolist(), name
    assert sc.argmax_first_nan(cases["inf_then_nan"]).tolist() == [2, 1, 0]


# ------------------------------------------------------------------------------------ 3. steps
def _walk(resp, s):
    tb, inp = sc.tables(resp), sc.step_inputs(resp, s)
    for kern, kw in sc.ddpm_cases():
        kw = dict(kw, t_end=sc.resolve_t_end(kw["t_end"], inp))
        if "vv" in kw:
            kw["vv"] = sc.vv_array(kw["vv"])
        yield kern, ("sample", "pred_xstart", "g"), sc.ddpm_step(tb, inp, F32, **kw), sc.ddpm_step(tb, inp, np.float64, **kw)
    for kw in sc.ddim_cases():
        kw = dict(kw, t_end=sc.resolve_t_end(kw["t_end"], inp))
        yield "ddim", ("sample", "pred_xstart", "g"), sc.ddim_step(tb, inp, F32, **kw), sc.ddim_step(tb, inp, np.float64, **kw)
    for scale in (1.0, sc.OUT_SCALE):
        yield "xstart", ("out",), sc.xstart_from_eps(tb, inp, F32, scale), sc.xstart_from_eps(tb, inp, np.float64, scale)
    for clip in (0, 1):
        for m in sc.MASKS + ("mixed",):
            mk = sc.mask_array(m)
            yield "edit", ("out",), sc.edit_replace_eps(tb, inp, F32, clip, mk), sc.edit_replace_eps(tb, inp, np.float64, clip, mk)


def test_step_restatements_set_the_bounds():
    worst = {}
    for resp in sc.SCHEDULES:
        for s in (1, 1e3):
            for kern, outs, a, b in _walk(resp, s):
                for o in outs:
                    assert a[o].dtype == F32 and b[o].dtype == np.float64, (kern, o)
                    worst[f"{kern}.{o}"] = max(worst.get(f"{kern}.{o}", 0.0), sc.ratio(a[o], b[o], b[o + ".A"]))
    assert set(worst) == {k for k in sc.MEASURED if k.split(".")[0] in ("ddpm", "learned", "ddim", "xstart", "edit")}
    for name, w in worst.items():
        _holds(name, w)


@pytest.mark.parametrize("resp", sc.SCHEDULES)
def test_step_cases_are_hard(resp):
    tb = sc.tables(resp)
    assert tb["T"] == {"": 1000, "250": 250, "ddim50": 50}[resp] and all(t.dtype == F32 and len(t) == tb["T"] for t in tb["tabs"])
    for s in (1, 1e3):
        inp = sc.step_inputs(resp, s)
        assert inp["t"].tolist() == [0, 1, tb["T"] - 1, tb["T"] // 2] and inp["x"].shape == (4, 321) and 321 % 256
        r = sc.ddpm_step(tb, inp, np.float64, clip=1)
        x0, A = r["x0_64"], np.abs(tb["tabs"][0][inp["t"]][:, None] * inp["x"]) + np.abs(tb["tabs"][1][inp["t"]][:, None] * inp["eps"])
        assert 0.25 < (np.abs(x0) > 1).mean() < 0.42                               # a third saturates
        assert np.median(A[2] / np.maximum(np.abs(x0[2]), 1e-3)) > 50 * s          # t = T' - 1: the difference cancels
        assert r["sat"].mean() > (0.3 if s == 1 else 0.2)                          # ... and most of those beyond the rounding margin
        plain = 3 * sc.U * A <= 1e-3                                                # per element: the issue's margin wherever rounding stays below it
        assert np.array_equal(sc.clip_margin(A.astype(np.float64))[plain], np.full(int(plain.sum()), 1e-3)) and np.array_equal(r["sat"][plain], (np.abs(x0) > 1 + 1e-3)[plain])
        assert plain.all() if s == 1 else (plain[0].mean() > 0.5 > plain[2].mean())  # s = 1e3: most of t = 0 keeps it, 157 x 1e3 at T' - 1 cannot
        _report(kind="step_case", schedule=resp, s=s, saturated=float((np.abs(x0) > 1).mean()), exact=float(r["sat"].mean()),
                cancel=float(np.median(A[2] / np.maximum(np.abs(x0[2]), 1e-3))))
    assert 1 / float(tb["tabs"][1][0]) > 50                                         # edit at t = 0: the division by c2 amplifies


@pytest.mark.parametrize("resp", sc.SCHEDULES)
def test_step_reference_is_the_oracles(resp):
    """what oracle/diffusion_np.py covers of these kernels: xstart_from_eps, eps_from_xstart after the edit replacement, p_mean_variance
    (mean, pred_xstart, fixed variance) with and without clip, p_sample (the condition-mean gradient and the t > t_end noise gate) and
    ddim_sample (condition_score behind the clip, sigma, sqrt(1 - abp - sigma^2) and the t != t_end gate) -- the float32 restatement is
    the oracle bit for bit, the float64 reference within the restatement's own bound.  The oracle has no learned variances."""
    S = diffusion_np.Schedule(1000, "linear", resp if resp else "")
    tb = sc.tables(resp)
    for mine, name in zip(tb["tabs"], ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2",
                                       "model_variance", "model_log_variance", "alphas_cumprod", "alphas_cumprod_prev")):
        assert np.allclose(mine, getattr(S, name).astype(F32), rtol=2.0 ** -23, atol=0), name
    tbo = dict(tb, tabs=[getattr(S, n).astype(F32) for n in ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1",
                                                              "posterior_mean_coef2", "model_variance", "model_log_variance", "alphas_cumprod",
                                                              "alphas_cumprod_prev")])
    for s in (1, 1e3):
        inp = sc.step_inputs(resp, s)
        x, eps, t = inp["x"].reshape(4, 1, 1, 321), inp["eps"].reshape(4, 1, 1, 321), inp["t"]
        assert _same(diffusion_np.xstart_from_eps(S, x, t, eps).reshape(4, 321), sc.xstart_from_eps(tbo, inp, F32, 1.0)["out"])
        for clip in (0, 1):
            pm = diffusion_np.p_mean_variance(S, lambda xx, tt: eps, x, t, bool(clip), {})
            a, b = sc.ddpm_step(tbo, inp, F32, clip=clip), sc.ddpm_step(tbo, inp, np.float64, clip=clip)
            assert _same(pm["mean"].reshape(4, 321), a["sample"]) and _same(pm["pred_xstart"].reshape(4, 321), a["pred_xstart"])
            assert _same(np.exp(F32(0.5) * pm["log_variance"].reshape(4, 321)).astype(F32), a["g"].astype(F32))
            assert sc.ratio(pm["mean"].reshape(4, 321), b["sample"], b["sample.A"]) <= sc.bound("ddpm.sample")
            shape4 = x.shape
            cond = dict(cond_fn=lambda xx, tt: inp["grad"].reshape(shape4), guidance=dict(schedule=False))
            for grad in (False, True):
                for te in sc.t_ends(inp):
                    kw = dict(clip=clip, grad=grad, noise=True, t_end=te)
                    extra = cond if grad else {}
                    ps = diffusion_np.p_sample(S, lambda xx, tt: eps, x, t, inp["noise"].reshape(shape4), clip_denoised=bool(clip), t_end=te, **extra)
                    a, b = sc.ddpm_step(tbo, inp, F32, **kw), sc.ddpm_step(tbo, inp, np.float64, **kw)
                    assert _same(ps["sample"].reshape(4, 321), a["sample"]) and _same(ps["mean"].reshape(4, 321), a["mean"]), ("p_sample", s, kw)
                    assert _same(ps["pred_xstart"].reshape(4, 321), a["pred_xstart"])
                    assert sc.ratio(ps["sample"].reshape(4, 321), b["sample"], b["sample.A"]) <= sc.bound("ddpm.sample")
                    ds = diffusion_np.ddim_sample(S, lambda xx, tt: eps, x, t, inp["noise"].reshape(shape4), eta=1.0, clip_denoised=bool(clip), t_end=te,
                                                  return_aux=True, **extra)
                    a, b = sc.ddim_step(tbo, inp, F32, **kw), sc.ddim_step(tbo, inp, np.float64, **kw)
                    assert _same(ds["sample"].reshape(4, 321), a["sample"]) and _same(ds["pred_xstart"].reshape(4, 321), a["pred_xstart"]), ("ddim_sample", s, kw)
                    assert _same(ds["aux"]["mean_pred"].reshape(4, 321), a["mean"]) and _same(ds["aux"]["sigma"].reshape(4), a["g"][:, 0])
                    for o in ("sample", "pred_xstart"):
                        assert sc.ratio(ds[o].reshape(4, 321), b[o], b[o + ".A"]) <= sc.bound("ddim." + o)
                    assert sc.ratio(np.broadcast_to(ds["aux"]["sigma"].reshape(4, 1), (4, 321)), b["g"], b["g.A"]) <= sc.bound("ddim.g")
            for m in sc.MASKS + ("mixed",):
                mk = sc.mask_array(m)
                edit = dict(mask=mk.reshape(x.shape), gt=inp["gt"].reshape(x.shape))
                x0e = diffusion_np.xstart_from_eps(S, x, t, eps)
                x0e = np.clip(x0e, -1, 1) if clip else x0e
                want = diffusion_np.eps_from_xstart(S, x, t, edit["mask"] * edit["gt"] + (1 - edit["mask"]) * x0e).astype(F32)
                e32, e64 = sc.edit_replace_eps(tbo, inp, F32, clip, mk), sc.edit_replace_eps(tbo, inp, np.float64, clip, mk)
                assert _same(want.reshape(4, 321), e32["out"])
                assert sc.ratio(want.reshape(4, 321), e64["out"], e64["out.A"]) <= sc.bound("edit.out")


# ------------------------------------------------------------------------------------ 4. rules
@pytest.fixture(scope="module")
def gold():
    return load_golden("step_inputs")


def test_fixture_names_its_seeds_and_stays_small(gold):
    import os
    from conftest import GOLDEN
    assert int(gold["seed.rule"][0]) == sc.RULE_SEED and int(gold["seed.collage"][0]) == sc.COLLAGE_SEED
    assert os.path.getsize(os.path.join(GOLDEN, "step_inputs.npz")) < 1024 * 1024
    assert all(v.dtype.kind in "fiu" for v in gold.values())


def test_roll_families_hold_what_they_are_named_for():
    shapes = [s for f in sc.RULE_SHAPES for s in sc.RULE_SHAPES[f]]
    assert {s[0] for s in shapes} == {1, 3} and {s[1] for s in shapes} == {1, 3} and {s[2] for s in shapes} == {128, 384}
    for fam, shape in sc.rule_cases() + sc.rule_cases(sc.CHORD_SHAPES):
        r = sc.roll(fam, shape)
        assert r.shape == (shape[0], shape[1], 128, shape[2]) and r.dtype == F32 and (r[:, 1:] == sc.MARKER).all()
    th = sc.roll("threshold", (3, 3, 384))[:, 0, sc.MIN_PIANO:sc.MAX_PIANO + 1]
    assert all((th.view(np.uint32) == v.view(np.uint32)).any() for v in sc.THRESHOLD_VALUES)
    assert sc.THRESHOLD_VALUES[1] < sc.TH < sc.THRESHOLD_VALUES[2] and sc.THRESHOLD_VALUES[4] < -1
    e = sc.roll("edges", (3, 3, 384))[:, 0]
    assert (e[:, 60, 0] > 0).all() and (e[:, 62, -1] > 0).all() and all((e[:, p, 30] > 0).all() for p in (20, 21, 108, 109))
    assert e[0, 64, 255] > 0 and e[0, 64, 256] > 0 and e[0, 66, 256] == -1          # active across the block boundary: no onset at 256
    assert e[1, 66, 256] > 0 and e[1, 66, 255] == -1 and e[1, 64, 255] == -1        # onset exactly at 256
    assert (sc.roll("silent", (1, 3, 128))[:, 0] == -1).all() and (sc.roll("full", (3, 1, 128))[:, 0] == 1).all()
    for shape in sc.RULE_SHAPES["nonfinite"]:
        a = sc.roll("nonfinite", shape)[:, 0]
        w = 128 if shape[2] == 384 else 16
        for n in range(min(shape[0], 2)):
            cols = [int(np.argwhere(m[n])[0][1]) for m in (np.isnan(a), a == np.inf, a == -np.inf)]
            assert [int(m[n].sum()) for m in (np.isnan(a), a == np.inf, a == -np.inf)] == [1, 1, 1] and len({c // w for c in cols}) == 3
    lv = sc.roll("levels", (1, 1, 128))[0, 0]
    for k in sc.LEVEL_KS:
        v = F32(2.0 * k / 127.0 - 1.0)
        assert all((lv == x).any() for x in (v, np.nextafter(v, F32(-2)), np.nextafter(v, F32(2))))


@pytest.mark.parametrize("fam,shape", sc.rule_cases(), ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_rule_references_agree(gold, fam, shape):
    """the reference's outputs and rolls (the fixture), oracle/rules_np.py and the float64 definitions of step_cases agree"""
    key, src = sc.case_key(fam, shape), sc.roll(fam, shape)
    N, _, T = shape
    b = sc.binarise(src[:, 0])
    for rule, kw in sc.ND_RULES.items():
        mine = src.copy()
        with np.errstate(invalid="ignore"):
            out = rules_np.FUNC_DICT[rule](mine)
        assert _same(out, gold[f"{key}.{rule}.out"]) and _same(mine[:, 0], gold[f"{key}.{rule}.after"]) and _same(mine[:, 1:], src[:, 1:])
        iv = kw["interval"]
        vert = b.sum(1).reshape(N, -1, iv).mean(-1)
        d = np.diff(np.pad(b, ((0, 0), (0, 0), (1, 0))), axis=-1)
        with np.errstate(invalid="ignore"):
            on = (np.where(d < 0, 0, d).sum(1) != 0).astype(np.float64)                    # NaN != 0
        hor = on.reshape(N, -1, iv).sum(-1) / kw["horizontal_scale"]
        want = np.concatenate((vert, hor), -1).astype(F32)
        assert _same(want.squeeze() if N == 1 else want, gold[f"{key}.{rule}.out"]), rule
    if N > 1:
        mine = src.copy()
        with np.errstate(invalid="ignore"):
            cls = rules_np.note_density_class(mine)
        assert _same(cls, gold[f"{key}.note_density_class.out"]) and _same(mine[:, 0], gold[f"{key}.note_density_class.after"])
        if fam == "nonfinite":
            assert (cls[np.isnan(gold[f"{key}.note_density_hr_1.out"])] == 7).all()        # torch.bucketize: NaN above every bound
    h64, _, _ = sc.pitch_hist64(src)
    ref = gold[f"{key}.pitch_hist.out"].reshape(N, 12)
    assert np.array_equal(np.isnan(h64), np.isnan(ref)) and np.allclose(h64, ref, rtol=0, atol=1e-6, equal_nan=True)
    after = gold[f"{key}.pitch_hist.after"]
    assert (after[:, :sc.MIN_PIANO] == -1).all() and (after[:, sc.MAX_PIANO + 1:] == -1).all()
    assert _same(after[:, sc.MIN_PIANO:sc.MAX_PIANO + 1], src[:, 0, sc.MIN_PIANO:sc.MAX_PIANO + 1])
    if fam == "silent":
        assert (h64 == 0).all() and (sc.pitch_hist32(src) == 0).all()


def test_pitch_restatements_set_the_bounds():
    worst = {"pitch.hist": 0.0, "vag.logp": 0.0, "vag.hist": 0.0, "vag.dh": 0.0}
    for fam, shape in sc.rule_cases():
        src = sc.roll(fam, shape)
        h64, h32 = sc.pitch_hist64(src)[0], sc.pitch_hist32(src)
        assert np.array_equal(np.isnan(h64), np.isnan(h32))
        fin = ~np.isnan(h64)
        worst["pitch.hist"] = max(worst["pitch.hist"], float(np.abs(h32.astype(np.float64) - h64)[fin].max() / sc.U) if fin.any() else 0.0)
        if fam not in sc.FINITE:
            continue
        tg = sc.vag_target(shape[0])
        for scale in (1.0, 37.5):
            l64, hh, dh64, unit = sc.vag64(src, tg, scale)
            l32, h32b, dh32 = sc.vag32(src, tg, scale)
            worst["vag.logp"] = max(worst["vag.logp"], float((np.abs(l32 - l64) / np.abs(l64)).max() / sc.U))
            worst["vag.hist"] = max(worst["vag.hist"], float(np.abs(h32b - hh).max() / sc.U))
            worst["vag.dh"] = max(worst["vag.dh"], float((np.abs(dh32 - dh64) / unit).max() / sc.U))
            lo, go = rules_np.pitch_hist_logp_grad(src.copy(), tg, scale)                     # the closed form already in the oracle
            assert np.allclose(lo, l64, rtol=1e-6) and np.allclose(go[:, 0, 60, 0], 0.5 * dh64[:, 0], rtol=1e-6)
            assert (go[:, 1:] == 0).all() and (go[:, 0, :sc.MIN_PIANO] == 0).all() and (go[:, 0, sc.MAX_PIANO + 1:] == 0).all()
            if fam == "silent":
                assert np.abs(dh64).max() > 1e10 * scale                                      # u / 1e-12
    for name, w in worst.items():
        _holds(name, w)


def test_bucketize_and_row_loss_cases():
    for bounds in (rules_np.VERTICAL_ND_BOUNDS, rules_np.HORIZONTAL_ND_BOUNDS, [1.8, 2.6, 3.2]):
        b = np.asarray(bounds, F32)
        v = sc.bucketize_values(b)
        assert np.isnan(v).sum() == 1 and np.isinf(v).sum() == 2 and all((v == x).any() for x in b)
        want = torch.bucketize(torch.from_numpy(v), torch.from_numpy(b)).numpy()
        assert want[np.isnan(v)][0] == len(b) and want[v == np.inf][0] == len(b) and want[v == -np.inf][0] == 0
        assert np.array_equal(want, np.searchsorted(b, v, side="left"))
    assert torch.bucketize(torch.tensor([float("nan"), float("inf"), float("-inf"), 1.8]), torch.tensor([1.8, 2.6, 3.2])).tolist() == [3, 3, 0, 0]
    for K in (1, 12, 16):
        a, b = sc.row_loss_case(K)
        mse, _ = sc.row_loss64(a, b, 0)
        zo, _ = sc.row_loss64(a, b, 1)
        assert np.isnan(mse[5]) and mse[9] == np.inf and mse[3] == 0 and zo[3] == 0 and zo[5] > 0
        assert np.allclose(rules_np.mse_loss_mean(a, b), mse, rtol=1e-5, equal_nan=True) and np.array_equal(rules_np.zero_one_loss_mean(a, b), zo.astype(F32))


# ------------------------------------------------------------------------------------ 5. collage
def test_collage_references_agree(gold):
    assert [c for c in ((n, ov) for n in sc.COLLAGE_N for ov in sc.COLLAGE_OV) if not sc.collage_valid(*c, 1)] == [(2, 96)]
    cfg = sc.collage_configs()
    assert {c[0] for c in cfg} == {1, 3} and {c[1] for c in cfg} == {1, 16} and {(c[2], c[3]) for c in cfg} == {(n, o) for n in sc.COLLAGE_N for o in sc.COLLAGE_OV}
    for n in sc.COLLAGE_N:
        for ov in sc.COLLAGE_OV:
            img, wins = sc.golden_image(n, ov), sc.golden_windows(n, ov)
            assert _same(sc.split_ref(img, n, ov, 0)[0], gold[f"split.n{n}ov{ov}.wins"])          # the reference's (b n) row order at B = 3
            for tag, avg in (("avg", 1), ("sum", 0)):
                v32, _, _ = sc.merge_ref(wins, None, n, ov, 0, avg, torch.float32)
                v64, A, terms = sc.merge_ref(wins, None, n, ov, 0, avg, torch.float64)
                assert _same(v32, gold[f"merge.n{n}ov{ov}.{tag}"])
                assert terms.max() == (1 if ov == 0 or n == 1 else (2 if ov <= 64 else min(n, 4)))
                assert (np.abs(v32 - v64) <= terms * sc.U * A).all()
    for B, h, n, ov in cfg:
        if ov == 0:
            continue
        full, half = sc.collage_arrays(B, h, n, ov)
        for circle in (0, 1):
            if not sc.collage_valid(n, ov, circle):
                continue
            W = n * (sc.BASE - ov) + (0 if circle else ov)
            calls = []

            def eps_fn(x, t, y=None):
                calls.append(x.shape)
                return full if x.shape[-1] == sc.BASE else half
            want = collage_np.condind_eps(np.zeros((B, sc.COLLAGE_C, h, W), F32), np.zeros(B, np.int64), eps_fn, n, ov, circle=bool(circle))
            got, _, _ = sc.merge_ref(full, half, n, ov, circle, 0, torch.float32)
            assert got.shape == want.shape == (B, sc.COLLAGE_C, h, W)
            if ov <= 64:
                assert _same(got, want)
            else:
                v64, A, terms = sc.merge_ref(full, half, n, ov, circle, 0, torch.float64)
                assert (np.abs(want - v64) <= terms * sc.U * A).all() and (np.abs(got - v64) <= terms * sc.U * A).all()
    idx = sc.index_windows(3, 1, 3)
    m, _, _ = sc.merge_ref(idx, None, 3, 64, 0, 1, torch.float32)
    assert m[1, 0, 0, 0] == 4 and m[1, 0, 0, 64] == 4.5 and m[2, 0, 0, -1] == 9                  # sample b reads windows b n .. b n + n - 1
