"""-m gpu: the sampler and SCG kernels (csrc/sampler.hip), the rule kernels (csrc/rules.hip) and the DiffCollage kernels (csrc/collage.hip)
element by element on edge inputs (tests/step_cases.py, docs/rounds/step_inputs.md), through the C ABI.

Every float result is held per element to 4 x the worst ratio of a float32 restatement against float64, measured on the CPU
(step_cases.MEASURED) -- never to a figure of a kernel; gathers, gates, saturation, integer counts, in-place writes and the two SCG routes
are compared bit for bit.  Every output buffer is fenced with NaN on both sides.  One RGM_STEP_REPORT line per kernel and measure."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import step_cases as sc
from conftest import load_golden
from oracle import rules_np

pytestmark = pytest.mark.gpu
F32 = np.float32
PAD = 8
U64 = C.c_uint64


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"


@pytest.fixture(scope="module")
def R():
    from rgm import native
    return native


@pytest.fixture(scope="module")
def gold():
    return load_golden("step_inputs")


def _report(**kw):
    print("RGM_STEP_REPORT " + json.dumps(kw))


_KEEP = []


@pytest.fixture(autouse=True)
def _keep_inputs_alive():
    """an input made inside a call's argument list would be freed, and its memory handed to the next input, before the launch"""
    yield
    torch.cuda.synchronize()
    del _KEEP[:]


def dev(a):
    if a is None:
        return None
    _KEEP.append(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    return _KEEP[-1]


class Fenced:
    """an output of `shape` with PAD NaN (or 0xAB bytes / -1 for integers) on both sides, which have to survive"""

    def __init__(self, shape, dtype=torch.float32):
        self.n = int(np.prod(shape))
        self.shape = shape
        self.fill = float("nan") if dtype.is_floating_point else (171 if dtype == torch.uint8 else -1)
        self.buf = torch.full((self.n + 2 * PAD,), self.fill, dtype=dtype, device="cuda")
        self.view = self.buf[PAD:PAD + self.n]

    def ptr(self):
        return C.c_void_p(self.view.data_ptr())

    def get(self):
        torch.cuda.synchronize()
        b = self.buf.cpu()
        edge = torch.cat((b[:PAD], b[PAD + self.n:]))
        assert (torch.isnan(edge).all() if b.dtype.is_floating_point else (edge == self.fill).all()), "a write outside the output"
        return b[PAD:PAD + self.n].reshape(self.shape).numpy()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def bits(a, b):
    """bit for bit, the sign of zero and the payload of a NaN included"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ==================================================================================== 1. Philox normals
def randn(R, seed, offset, n):
    out = Fenced((n,))
    R.check(R.lib.rgm_randn(out.ptr(), n, U64(seed), U64(offset), R.current_stream()))
    return out.get()


@pytest.mark.parametrize("seed", sc.SEEDS)
def test_randn_against_float64(R, seed):
    worst = 0.0
    for s, off, n in sc.RANDN_CASES:
        if s != seed:
            continue
        z = randn(R, s, off, n)
        assert np.isfinite(z).all()
        r = sc.randn_ratio(z, s, off)
        worst = max(worst, r)
        assert r <= sc.RANDN_K, (s, off, n, r)
    _report(kernel="randn", measure="|z - z64| / (2^-24 (1 + rad))", seed=seed, worst=worst, bound=sc.RANDN_K)


def test_randn_slices_regenerate_bit_for_bit(R):
    for seed in sc.SEEDS:
        base = sc.P34 - 513
        z = randn(R, seed, base, 1027)
        for off, n in ((0, 7), (1, 6), (2, 5), (3, 4), (510, 9), (511, 3), (513, 1), (1000, 27)):
            assert bits(randn(R, seed, base + off, n), z[off:off + n]), (seed, off, n)
    assert not bits(randn(R, sc.SEEDS[2], 0, 64), randn(R, 12345, 0, 64))                       # the seed's high word
    assert not bits(randn(R, 0, sc.P34, 64), randn(R, 0, 0, 64))                                 # the counter's high word


# ==================================================================================== 2. SCG
def candidates(R, mean, g, noise, n, B, E):
    out = Fenced((n, B, E))
    R.check(R.lib.rgm_scg_candidates(R.ptr(mean), R.ptr(g), R.ptr(noise), out.ptr(), n, B, E, R.current_stream()))
    return out


def test_scg_candidates_against_float64(R):
    n, B, E = 3, 2, 320
    rng = np.random.RandomState(4200)
    mean, g, z = (rng.randn(B, E) * 3).astype(F32), np.array([0.7, 1e-3], F32), rng.randn(n, B, E).astype(F32)
    got = candidates(R, dev(mean), dev(g), dev(z), n, B, E).get()
    ref, A = sc.scg_candidates64(mean, g, z)
    r = float((np.abs(got - ref) / (sc.U * A)).max())
    _report(kernel="scg_candidates", measure="|c - c64| / (2^-24 (|mean| + |g z|))", worst=r, bound=2.0)
    assert r <= 2.0


def select(R, cand, total, n, B, E):
    """-> (idx (B,), out (B, E) or None)"""
    idx = Fenced((B,), torch.int64)
    out = None if cand is None else Fenced((B, E))
    R.check(R.lib.rgm_scg_select(R.ptr(cand), R.ptr(total), None if out is None else out.ptr(), idx.ptr(), n, B, E, R.current_stream()))
    return idx.get(), None if out is None else out.get()


@pytest.mark.parametrize("E", [320, 70000])
def test_scg_select_indices_and_rows(R, E):
    rng = np.random.RandomState(4300 + E)
    for name, tot in sc.select_cases().items():
        n, B = tot.shape
        want = sc.argmax_first_nan(tot)
        cand = rng.randn(n, B, E).astype(F32)
        cand[0, 0, :4] = (np.nan, -0.0, np.inf, 1e-45)                 # a copy keeps every bit
        idx, out = select(R, dev(cand), dev(tot), n, B, E)
        assert idx.tolist() == want.tolist(), name
        assert bits(out, cand[want, np.arange(B)]), name
        idx2, _ = select(R, None, dev(tot), n, B, E)                    # index only
        assert idx2.tolist() == want.tolist(), name


REBUILD_GEOMETRY = [((4, 32, 4), 32), ((4, 32, 4), 16), ((4, 32, 4), 8), ((1, 1, 320), 1)]
REBUILD_BASES = [1, 2, 3, 2 ** 32 - 1500 + 1, 2 ** 34 - 1500 + 2, 2 ** 34 + 7]


@pytest.mark.parametrize("per_elem", [0, 1], ids=["g_per_sample", "g_per_element"])
@pytest.mark.parametrize("geom,seg_rows", REBUILD_GEOMETRY, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"rows{v}")
def test_scg_rebuild_is_the_three_kernel_path(R, geom, seg_rows, per_elem):
    """rgm_scg_rebuild[_g] against rgm_scg_select over rgm_scg_candidates over rgm_randn at the same stream positions, bit for bit, and
    against mean + g z64 of the float64 normals"""
    (Cc, H, W), n, B = geom, 3, 2
    E, S = Cc * H * W, H // seg_rows
    seg_of = (np.arange(E) // W) % H // seg_rows
    worst = 0.0
    for ci, base in enumerate(REBUILD_BASES):
        seed = sc.SEEDS[ci % 3]
        rng = np.random.RandomState(4400 + ci)
        mean = rng.randn(B, E).astype(F32)
        g = (rng.rand(B, E) + 0.1).astype(F32) if per_elem else np.array([0.8, 0.05], F32)
        win = rng.randint(0, n, size=(S, B))
        win[0, 0], win[-1, -1] = 0, n - 1                                # the first and the last candidate both win somewhere
        if base % 4 == 3:
            win[0, 0] = n - 1
        md, gd, wd = dev(mean), dev(g), dev(win.astype(np.int64))
        out = Fenced((B, E))
        fn = R.lib.rgm_scg_rebuild_g if per_elem else R.lib.rgm_scg_rebuild
        R.check(fn(R.ptr(md), R.ptr(gd), R.ptr(wd), U64(seed), U64(base), out.ptr(), B, E, H, W, seg_rows, R.current_stream()))
        got = out.get()
        # the three-kernel path, one selection per segment
        nz = Fenced((n * B * E,))
        R.check(R.lib.rgm_randn(nz.ptr(), n * B * E, U64(seed), U64(base), R.current_stream()))
        z = nz.get()
        if per_elem:                                                     # (n, B E, 1): the per-sample scale of B E one-element samples
            cand = candidates(R, md, gd, dev(z), n, B * E, 1)
        else:
            cand = candidates(R, md, gd, dev(z), n, B, E)
        cand_host = cand.get().reshape(n, B, E)
        want = np.empty((B, E), F32)
        for s in range(S):
            tot = np.zeros((n, B), F32)
            tot[win[s], np.arange(B)] = 1.0
            idx, rows = select(R, dev(cand_host), dev(tot), n, B, E)
            assert idx.tolist() == win[s].tolist()
            want[:, seg_of == s] = rows[:, seg_of == s]
        assert bits(got, want), (base, seg_rows, per_elem)
        # float64: the winner's normals at base + (k B + b) E + e
        for b in range(B):
            for s in range(S):
                cols = np.flatnonzero(seg_of == s)
                k = int(win[s, b])
                z64, rad = sc.normals64(seed, base + (k * B + b) * E, E)
                gg = (g[b] if per_elem else np.full(E, g[b])).astype(np.float64)
                ref = mean[b].astype(np.float64) + gg * z64
                tol = sc.U * (sc.RANDN_K * gg * (1 + rad) + 2.0 * (np.abs(mean[b]) + np.abs(gg * z64)))
                r = (np.abs(got[b] - ref) / tol)[cols].max()
                worst = max(worst, float(r))
                assert r <= 1.0, (base, b, s, r)
    _report(kernel="scg_rebuild_g" if per_elem else "scg_rebuild", measure="|x - x64| / (2^-24 (k |g| (1 + rad) + 2 (|mean| + |g z|)))",
            geometry=list(geom), seg_rows=seg_rows, worst=worst, bound=1.0)


# ==================================================================================== 3. step kernels
class Tabs:
    def __init__(self, tb):
        self.t = [dev(a) for a in tb["tabs"]]
        self.ptrs = (C.c_void_p * 8)(*[t.data_ptr() for t in self.t])
        self.min_log, self.max_log = dev(tb["min_log"]), dev(tb["max_log"])


@pytest.fixture(scope="module")
def tabs():
    return {r: Tabs(sc.tables(r)) for r in sc.SCHEDULES}


def run_ddpm(R, T, inp, d, clip=0, t_end=-1, grad=False, noise=False, vv=None, mode="fixed", with_g=True):
    """-> dict of host arrays: sample, pred_xstart, g ((N, E) broadcast of g_out, or g_elem)"""
    N, E = inp["x"].shape
    sample, pred = Fenced((N, E)), Fenced((N, E))
    idle = Fenced((N,))                                                  # a g_out the call is not given: it has to stay NaN
    gr, nz = (d["grad"] if grad else None), (d["noise"] if noise else None)
    st = R.current_stream()
    if mode == "fixed":
        g = Fenced((N,)) if with_g else None
        R.check(R.lib.rgm_ddpm_step(R.ptr(d["x"]), R.ptr(d["eps"]), R.ptr(gr), R.ptr(nz), R.ptr(d["t"]), T.ptrs, clip, t_end, sample.ptr(),
                                    pred.ptr(), None if g is None else g.ptr(), N, E, st))
        gv = None if g is None else np.broadcast_to(g.get()[:, None], (N, E))
    else:
        mn, mx = (T.min_log, T.max_log) if mode == "range" else (None, None)
        vd = dev(vv)
        if with_g:
            g = Fenced((N, E))
            R.check(R.lib.rgm_ddpm_step_learned_g(R.ptr(d["x"]), R.ptr(d["eps"]), R.ptr(vd), R.ptr(mn), R.ptr(mx), R.ptr(gr), R.ptr(nz),
                                                  R.ptr(d["t"]), T.ptrs, clip, t_end, sample.ptr(), pred.ptr(), g.ptr(), N, E, st))
            gv = g.get()
        else:
            R.check(R.lib.rgm_ddpm_step_learned(R.ptr(d["x"]), R.ptr(d["eps"]), R.ptr(vd), R.ptr(mn), R.ptr(mx), R.ptr(gr), R.ptr(nz),
                                                R.ptr(d["t"]), T.ptrs, clip, t_end, sample.ptr(), pred.ptr(), N, E, st))
            gv = None
    if mode != "fixed" or not with_g:                                    # the learned entries take no g_out; the fixed one was passed NULL
        assert np.isnan(idle.get()).all()
    return dict(sample=sample.get(), pred_xstart=pred.get(), g=gv)


def run_ddim(R, T, inp, d, clip=0, t_end=-1, grad=False, noise=False, eta=1.0):
    N, E = inp["x"].shape
    sample, pred, g = Fenced((N, E)), Fenced((N, E)), Fenced((N,))
    R.check(R.lib.rgm_ddim_step(R.ptr(d["x"]), R.ptr(d["eps"]), R.ptr(d["grad"] if grad else None), R.ptr(d["noise"] if noise else None),
                                R.ptr(d["t"]), T.ptrs, clip, t_end, eta, sample.ptr(), pred.ptr(), g.ptr(), N, E, R.current_stream()))
    return dict(sample=sample.get(), pred_xstart=pred.get(), g=np.broadcast_to(g.get()[:, None], (N, E)))


def check_step(kern, got, ref, worst, tag):
    for o in ("sample", "pred_xstart", "g"):
        if got[o] is None:
            continue
        assert np.isfinite(got[o]).all(), (kern, o, tag)
        r = sc.ratio(got[o], ref[o], ref[o + ".A"])
        worst[f"{kern}.{o}"] = max(worst.get(f"{kern}.{o}", 0.0), r)
        assert r <= sc.bound(f"{kern}.{o}"), (kern, o, tag, r, sc.bound(f"{kern}.{o}"))
    sat = ref["sat"]
    if sat.any():                                                       # beyond the margin the clipped x0 is exactly +-1
        assert bits(got["pred_xstart"][sat], np.sign(ref["x0_64"][sat]).astype(F32)), (kern, tag)


def device_inputs(inp):
    return {k: dev(inp[k]) for k in ("x", "eps", "grad", "noise", "gt", "t")}


@pytest.mark.parametrize("s", [1, 1e3], ids=["s1", "s1e3"])
@pytest.mark.parametrize("resp", sc.SCHEDULES, ids=["full", "250", "ddim50"])
def test_ddpm_steps_per_element(R, tabs, resp, s):
    tb, T, inp = sc.tables(resp), tabs[resp], sc.step_inputs(resp, s)
    d, worst = device_inputs(inp), {}
    for kern, kw in sc.ddpm_cases():
        kw = dict(kw, t_end=sc.resolve_t_end(kw["t_end"], inp))
        if "vv" in kw:
            kw["vv"] = sc.vv_array(kw["vv"])
        ref = sc.ddpm_step(tb, inp, np.float64, **kw)
        got = run_ddpm(R, T, inp, d, **kw)
        check_step(kern, got, ref, worst, (resp, s, kw.get("mode"), kw["clip"], kw["grad"], kw["noise"], kw["t_end"]))
        if kw["noise"]:
            # the gate is exact: where ti <= t_end the sample is the mean of the same call without noise, bit for bit; elsewhere it moved
            mean = run_ddpm(R, T, inp, d, **dict(kw, noise=False), with_g=False)
            assert bits(mean["pred_xstart"], got["pred_xstart"])
            closed = inp["t"] <= kw["t_end"]
            assert bits(got["sample"][closed], mean["sample"][closed]), (kern, kw["t_end"])
            assert closed.tolist() == {-1: [0, 0, 0, 0], 0: [1, 0, 0, 0], inp["mid"]: [1, 1, 0, 1], inp["T"]: [1, 1, 1, 1]}[kw["t_end"]]
            moved = np.abs(got["sample"][~closed] - mean["sample"][~closed]) > 0
            assert not (~closed).any() or moved.mean() > 0.5              # exp(-15) of the LEARNED case is below half an ulp of x = 1e3
            if kern == "learned":                                       # the entry without g_elem computes the same
                assert bits(run_ddpm(R, T, inp, d, **kw, with_g=False)["sample"], got["sample"])
    for k, w in worst.items():
        _report(kernel=k, schedule=resp, s=s, measure="|out - ref64| / (2^-24 A)", worst=w, bound=sc.bound(k))


@pytest.mark.parametrize("s", [1, 1e3], ids=["s1", "s1e3"])
@pytest.mark.parametrize("resp", sc.SCHEDULES, ids=["full", "250", "ddim50"])
def test_ddim_step_grad_clip_and_gate(R, tabs, resp, s):
    tb, T, inp = sc.tables(resp), tabs[resp], sc.step_inputs(resp, s)
    d, worst = device_inputs(inp), {}
    for kw in sc.ddim_cases():
        kw = dict(kw, t_end=sc.resolve_t_end(kw["t_end"], inp))
        ref = sc.ddim_step(tb, inp, np.float64, **kw)
        got = run_ddim(R, T, inp, d, **kw)
        check_step("ddim", got, ref, worst, (resp, s, kw))
        mean = run_ddim(R, T, inp, d, **dict(kw, noise=False))
        closed = inp["t"] == kw["t_end"]                                # ti != t_end gates the noise; t = 0 has sigma = 0 besides
        assert bits(got["sample"][closed], mean["sample"][closed]), kw
        open_rows = ~closed & (inp["t"] > 0)
        assert (np.abs(got["sample"][open_rows] - mean["sample"][open_rows]) > 0).mean() > 0.9
        assert bits(got["sample"][inp["t"] == 0], mean["sample"][inp["t"] == 0])
    for k, w in worst.items():
        _report(kernel=k, schedule=resp, s=s, measure="|out - ref64| / (2^-24 A)", worst=w, bound=sc.bound(k))


@pytest.mark.parametrize("resp", sc.SCHEDULES, ids=["full", "250", "ddim50"])
def test_xstart_and_edit_replace_per_element(R, tabs, resp):
    tb, T = sc.tables(resp), tabs[resp]
    worst = {"xstart.out": 0.0, "edit.out": 0.0}
    for s in (1, 1e3):
        inp = sc.step_inputs(resp, s)
        d = device_inputs(inp)
        N, E = inp["x"].shape
        for scale in (1.0, sc.OUT_SCALE):
            out = Fenced((N, E))
            R.check(R.lib.rgm_xstart_from_eps(R.ptr(d["x"]), R.ptr(d["eps"]), R.ptr(d["t"]), T.ptrs, float(scale), out.ptr(), N, E, R.current_stream()))
            ref = sc.xstart_from_eps(tb, inp, np.float64, scale)
            r = sc.ratio(out.get(), ref["out"], ref["out.A"])
            worst["xstart.out"] = max(worst["xstart.out"], r)
            assert r <= sc.bound("xstart.out"), (resp, s, scale, r)
        for clip in (0, 1):
            for m in sc.MASKS + ("mixed",):
                mk = sc.mask_array(m)
                out = Fenced((N, E))
                R.check(R.lib.rgm_edit_replace_eps(R.ptr(d["x"]), R.ptr(d["eps"]), R.ptr(d["gt"]), R.ptr(dev(mk)), R.ptr(d["t"]), T.ptrs, clip,
                                                   out.ptr(), N, E, R.current_stream()))
                ref = sc.edit_replace_eps(tb, inp, np.float64, clip, mk)
                got = out.get()
                r = sc.ratio(got, ref["out"], ref["out.A"])
                worst["edit.out"] = max(worst["edit.out"], r)
                assert r <= sc.bound("edit.out"), (resp, s, clip, m, r)
    for k, w in worst.items():
        _report(kernel=k, schedule=resp, measure="|out - ref64| / (2^-24 A)", worst=w, bound=sc.bound(k))


# ==================================================================================== 4. rules
RULE_IDS = [sc.case_key(f, s) for f, s in sc.rule_cases()]


@pytest.mark.parametrize("fam,shape", sc.rule_cases(), ids=RULE_IDS)
def test_note_density_rules_bit_equal(R, gold, fam, shape):
    """FUNC_DICT's five note-density entries: outputs and the whole roll afterwards against the reference's fixture and oracle/rules_np.py"""
    from music_rule_guidance.rule_maps import FUNC_DICT
    key, src = sc.case_key(fam, shape), sc.roll(fam, shape)
    for rule in tuple(sc.ND_RULES) + ("note_density_class",):
        if rule == "note_density_class" and shape[0] == 1:
            continue                                                    # the reference indexes a batch axis there: N > 1 only
        t = dev(src)
        out = FUNC_DICT[rule](t)
        torch.cuda.synchronize()
        out, after = out.cpu().numpy(), t.cpu().numpy()
        mine = src.copy()
        with np.errstate(invalid="ignore"):
            own = rules_np.FUNC_DICT[rule](mine)
        assert same(out, gold[f"{key}.{rule}.out"]) and same(out, own), (key, rule)
        assert bits(after[:, 0], gold[f"{key}.{rule}.after"]) and bits(after, mine), (key, rule)
        assert (after[:, 1:] == sc.MARKER).all()
    if fam == "nonfinite":
        assert np.isnan(gold[f"{key}.note_density_pixel.out"]).sum() == min(shape[0], 2)


@pytest.mark.parametrize("fam,shape", sc.rule_cases(), ids=RULE_IDS)
def test_pitch_hist_per_class(R, gold, fam, shape):
    key, src = sc.case_key(fam, shape), sc.roll(fam, shape)
    N, Cc, T = shape
    t, out, scratch = dev(src), Fenced((N, 12)), Fenced((N, 128))
    R.check(R.lib.rgm_rule_pitch_hist(R.ptr(t), out.ptr(), scratch.ptr(), N, Cc, T, R.current_stream()))
    got, after = out.get(), t.cpu().numpy()
    scratch.get()
    h64 = sc.pitch_hist64(src)[0]
    assert np.array_equal(np.isnan(got), np.isnan(h64)), key
    fin = ~np.isnan(h64)
    err = np.abs(got.astype(np.float64) - h64)[fin] / sc.U
    _report(kernel="pitch_hist", case=key, measure="per-class |hist - hist64| / 2^-24", worst=float(err.max()) if err.size else 0.0,
            bound=sc.bound("pitch.hist"))
    assert (err <= sc.bound("pitch.hist")).all(), (key, err.max())
    if fam == "silent":
        assert bits(got, np.zeros((N, 12), F32))
    assert bits(after[:, 0], gold[f"{key}.pitch_hist.after"]) and (after[:, 1:] == sc.MARKER).all()


@pytest.mark.parametrize("fam,shape", [c for c in sc.rule_cases() if c[0] in sc.FINITE], ids=[k for k in RULE_IDS if k.split(".")[0] in sc.FINITE])
def test_pitch_hist_value_and_gradient(R, gold, fam, shape):
    key, src = sc.case_key(fam, shape), sc.roll(fam, shape)
    N, Cc, T = shape
    tg = sc.vag_target(N)
    for scale in (1.0, 37.5):
        t = dev(src)
        hist, logp, droll, scratch = Fenced((N, 12)), Fenced((N,)), Fenced((N, Cc, 128, T)), Fenced((N * 140,))
        R.check(R.lib.rgm_rule_pitch_hist_vag(R.ptr(t), R.ptr(dev(tg)), float(scale), hist.ptr(), logp.ptr(), droll.ptr(), scratch.ptr(), N, Cc, T,
                                              R.current_stream()))
        h, lp, dr, after = hist.get(), logp.get(), droll.get(), t.cpu().numpy()
        scratch.get()
        l64, h64, dh64, unit = sc.vag64(src, tg, scale)
        e_l = float((np.abs(lp - l64) / np.abs(l64)).max() / sc.U)
        e_h = float(np.abs(h - h64).max() / sc.U)
        pr = np.arange(sc.MIN_PIANO, sc.MAX_PIANO + 1)
        want = 0.5 * dh64[:, pr % 12][:, :, None]                       # (N, 88, 1)
        e_d = float((np.abs(dr[:, 0, pr, :] - want) / (0.5 * unit[:, :, None])).max() / sc.U)
        for name, e in (("vag.logp", e_l), ("vag.hist", e_h), ("vag.dh", e_d)):
            _report(kernel=name, case=key, scale=scale, worst=e, bound=sc.bound(name))
            assert e <= sc.bound(name), (key, scale, name, e)
        assert np.isfinite(dr).all() and (dr[:, 1:] == 0).all() and (dr[:, 0, :sc.MIN_PIANO] == 0).all() and (dr[:, 0, sc.MAX_PIANO + 1:] == 0).all()
        assert (dr[:, 0, pr, :] == dr[:, 0, pr, :1]).all()              # one value per row
        if fam == "silent":
            assert np.abs(dr).max() > 1e10 * scale and bits(h, np.zeros((N, 12), F32))
        assert bits(after[:, 0], gold[f"{key}.pitch_hist.after"]) and (after[:, 1:] == sc.MARKER).all()


def test_bucketize_is_torchs(R):
    for bounds in (rules_np.VERTICAL_ND_BOUNDS, rules_np.HORIZONTAL_ND_BOUNDS, [1.8, 2.6, 3.2], [0.5]):
        b = np.asarray(bounds, F32)
        v = sc.bucketize_values(b)
        out = Fenced((len(v),), torch.int64)
        R.check(R.lib.rgm_bucketize(R.ptr(dev(v)), R.ptr(dev(b)), len(b), out.ptr(), len(v), R.current_stream()))
        want = torch.bucketize(torch.from_numpy(v), torch.from_numpy(b)).numpy()
        assert out.get().tolist() == want.tolist(), (bounds, v[out.get() != want])


@pytest.mark.parametrize("K", [1, 12, 16])
def test_row_loss(R, K):
    a, b = sc.row_loss_case(K)
    rows = a.shape[0]
    for zero_one in (0, 1):
        out = Fenced((rows,))
        R.check(R.lib.rgm_row_loss(R.ptr(dev(a)), R.ptr(dev(b)), out.ptr(), rows, K, zero_one, R.current_stream()))
        got = out.get()
        ref, scale = sc.row_loss64(a, b, zero_one)
        if zero_one:
            assert bits(got, (ref * K).astype(F32) / F32(K))
            continue
        fin = np.isfinite(ref)
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got == np.inf, ref == np.inf) and not fin[5] and not fin[9]
        assert (got[ref == 0] == 0).all()
        e = np.abs(got[fin] - ref[fin]) / (sc.U * np.maximum(scale[fin], 1e-300))
        _report(kernel="row_loss", K=K, measure="|out - ref64| / (2^-24 sum d^2 / K)", worst=float(e.max()), bound=float(K))
        assert (e <= K).all()


@pytest.mark.parametrize("fam,shape", sc.rule_cases(sc.CHORD_SHAPES), ids=[sc.case_key(f, s) for f, s in sc.rule_cases(sc.CHORD_SHAPES)])
def test_chord_quantise_bit_equal(R, gold, fam, shape):
    key, src = sc.case_key(fam, shape), sc.roll(fam, shape)
    N, Cc, T = shape
    t, q = dev(src), Fenced((N, 128, T), torch.uint8)
    R.check(R.lib.rgm_rule_chord_quantise(R.ptr(t), q.ptr(), N, Cc, T, R.current_stream()))
    got, after = q.get(), t.cpu().numpy()
    mine = src.copy()
    own = rules_np.chord_quantise(mine)
    assert same(got, gold[f"{key}.chord.q"]) and np.array_equal(got, own)
    assert bits(after[:, 0], gold[f"{key}.chord.after"]) and bits(after, mine)


# ==================================================================================== 5. collage
def split(R, img, B, h, W, n, ov, want_halves):
    wins = Fenced((B * n, sc.COLLAGE_C, h, sc.BASE))
    halves = Fenced((B * n, sc.COLLAGE_C, h, ov)) if want_halves and ov > 0 else None
    R.check(R.lib.rgm_collage_split(R.ptr(dev(img)), wins.ptr(), None if halves is None else halves.ptr(), B, sc.COLLAGE_C, h, W, n, ov,
                                    R.current_stream()))
    return wins.get(), None if halves is None else halves.get()


def merge(R, full, half, B, h, n, ov, circle, is_avg):
    Wl = n * sc.BASE - (n - 1) * ov
    out = Fenced((B, sc.COLLAGE_C, h, Wl - ov if circle else Wl))
    R.check(R.lib.rgm_collage_merge(R.ptr(dev(full)), R.ptr(dev(half)), out.ptr(), B, sc.COLLAGE_C, h, n, ov, circle, is_avg, R.current_stream()))
    return out.get()


@pytest.mark.parametrize("B,h,n,ov", sc.collage_configs(), ids=lambda v: str(v))
def test_collage_split_is_a_gather(R, B, h, n, ov):
    for circle in (0, 1):
        W = n * (sc.BASE - ov) + (0 if circle else ov)
        img = np.random.RandomState(8300 + B + h + n + ov + circle).randn(B, sc.COLLAGE_C, h, W).astype(F32)
        if not sc.collage_valid(n, ov, circle):
            with pytest.raises(R.RgmError):                             # the extension is wider than the image: refused before any launch
                split(R, img, B, h, W, n, ov, False)
            continue
        want_w, want_h = sc.split_ref(img, n, ov, circle)
        for halves in (False, True):
            w, hv = split(R, img, B, h, W, n, ov, halves)
            assert bits(w, want_w), (circle, halves)
            if hv is not None:
                assert bits(hv, want_h), circle


def test_collage_split_is_the_references_at_three_samples(R, gold):
    for n in sc.COLLAGE_N:
        for ov in sc.COLLAGE_OV:
            img = sc.golden_image(n, ov)
            assert bits(split(R, img, 3, 1, img.shape[-1], n, ov, True)[0], gold[f"split.n{n}ov{ov}.wins"]), (n, ov)
            wins = sc.golden_windows(n, ov)
            for tag, avg in (("avg", 1), ("sum", 0)):
                got, ref = merge(R, wins, None, 3, 1, n, ov, 0, avg), gold[f"merge.n{n}ov{ov}.{tag}"]
                if ov <= 64 and not avg:
                    assert bits(got, ref), (n, ov, tag)
                else:
                    v64, A, terms = sc.merge_ref(wins, None, n, ov, 0, avg, torch.float64)
                    assert (np.abs(got - v64) <= np.maximum(terms, 2) * sc.U * A).all() and (np.abs(ref - v64) <= np.maximum(terms, 2) * sc.U * A).all()


@pytest.mark.parametrize("B,h,n,ov", sc.collage_configs(), ids=lambda v: str(v))
def test_collage_merge_per_element(R, B, h, n, ov):
    full, half = sc.collage_arrays(B, h, n, ov)
    worst = 0.0
    for circle in (0, 1):
        if not sc.collage_valid(n, ov, circle):
            with pytest.raises(R.RgmError):                             # refused like the split of the same shape, before any launch
                merge(R, full, half, B, h, n, ov, circle, 0)
            continue
        for is_avg in (0, 1):
            for hf in (None, half):
                if hf is not None and ov == 0:
                    continue
                got = merge(R, full, hf, B, h, n, ov, circle, is_avg)
                v32, _, _ = sc.merge_ref(full, hf, n, ov, circle, is_avg, torch.float32)
                v64, A, terms = sc.merge_ref(full, hf, n, ov, circle, is_avg, torch.float64)
                assert got.shape == v64.shape
                if ov <= 64 and not sc.merge_divides(n, ov, circle, is_avg):
                    assert bits(got, v32), (circle, is_avg, hf is not None)          # at most two terms: the float32 fold, bit for bit
                    continue
                k = 2.0 if ov <= 64 else terms                                       # a division: 2 x 2^-24; four windows: cnt x 2^-24
                with np.errstate(divide="ignore", invalid="ignore"):
                    r = np.where(A > 0, np.abs(got - v64) / (k * sc.U * A), np.where(got == v64, 0.0, np.inf))
                worst = max(worst, float(r.max()))
                assert r.max() <= 1.0, (circle, is_avg, hf is not None, float(r.max()))
    _report(kernel="collage_merge", B=B, h=h, n=n, overlap=ov, measure="|out - ref64| / (k 2^-24 sum |terms|), k = 2 or the window count",
            worst=worst, bound=1.0)


@pytest.mark.parametrize("n,ov", [(2, 64), (3, 32), (7, 96), (3, 0)])
def test_collage_windows_land_in_their_sample(R, n, ov):
    """window (b, i) filled with b n + i + 1: the averages of small integers are exact, a swapped (b n) order is not"""
    B, h = 3, 1
    idx = sc.index_windows(B, h, n)
    for circle in (0, 1):
        got = merge(R, idx, None, B, h, n, ov, circle, 1)
        v64, _, _ = sc.merge_ref(idx, None, n, ov, circle, 1, torch.float64)
        assert np.abs(got - v64).max() <= 2 * sc.U * (B * n), (n, ov, circle)
        if not circle:                                                  # the first and the last column belong to one window each
            assert bits(got[:, 0, 0, 0], (np.arange(B) * n + 1).astype(F32)) and bits(got[:, 0, 0, -1], (np.arange(B) * n + n).astype(F32))
