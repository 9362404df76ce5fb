"""-m gpu: the native chord and key analyser on the device (csrc/chords.hip, rgm_rule_chords) against the restatement
tests/chords_ref.py, through the ABI, through FUNC_DICT, inside an SCG search step and from the CLI.  Comparison rules
(docs/rounds/chords.md): chords, roots, key and the "no key" cases equal exactly, every input with a gap >= 1e-9 between the best and
second-best key correlation in the restatement (asserted, never skipped), the coefficient within 1e-12 absolute.

The file name puts these tests behind the test_gpu_* files: the search steps and the CLI run build models (each with a side stream of
its own) and start the analyser's driver thread, and the suite's wall-clock tests of the two-stream forward (test_gpu_fullsize.py) are
sensitive to what the process has created before them."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import chords_ref as ref
from conftest import load_golden

pytestmark = pytest.mark.gpu
MIN_GAP, COEF_TOL = 1e-9, 1e-12


@pytest.fixture
def native():
    from music_rule_guidance import music_rules
    music_rules.register_chord_backend("native")
    yield music_rules
    music_rules.register_chord_backend(None)


def _run(q, wc, profile="krumhansl", given_tonic=None, analyse_key=True):
    from music_rule_guidance import music_rules
    t = torch.from_numpy(np.ascontiguousarray(q if q.ndim == 3 else q[None])).cuda()
    chords, roots, key, coef = music_rules.chords_native(t, wc, profile, given_tonic, analyse_key)
    assert chords.dtype == torch.int64 and roots.dtype == torch.int32 and key.dtype == torch.int32 and coef.dtype == torch.float64
    assert chords.is_cuda and chords.shape == roots.shape == (t.shape[0], t.shape[2] // wc)
    return chords.cpu().numpy(), roots.cpu().numpy(), key.cpu().numpy(), coef.cpu().numpy()


def _check(q, wc, profile="krumhansl"):
    """batch q (N,128,T) through the kernel against the restatement, row by row"""
    chords, roots, key, coef = _run(q, wc, profile)
    for i in range(q.shape[0]):
        want = ref.analyse(q[i], wc, profile)
        assert want["gap"] >= MIN_GAP, (i, want["gap"])
        assert chords[i].tolist() == want["chords"], i
        assert roots[i].tolist() == want["roots"], i
        assert int(key[i]) == want["key"], i
        assert abs(float(coef[i]) - want["coef"]) <= COEF_TOL, (i, float(coef[i]), want["coef"])


@pytest.mark.parametrize("N,T,wc", [(1, 128, 128), (3, 1024, 128), (5, 1064, 128), (3, 128, 16), (2, 2048, 100), (1, 1024, 1024)])
def test_kernel_matches_the_restatement_on_random_rolls(N, T, wc):
    q = np.stack([ref.random_roll(i, T) for i in range(N)])
    for profile in ("krumhansl", "aarden"):
        _check(q, wc, profile)
    # a given tonic with the key analysed, and without key analysis (key -1, coefficient 0 are written)
    chords, _, key, _ = _run(q, wc, given_tonic=5)
    chords2, roots2, key2, coef2 = _run(q, wc, given_tonic=5, analyse_key=False)
    for i in range(N):
        assert chords[i].tolist() == ref.analyse(q[i], wc, given_tonic=5)["chords"] and int(key[i]) == ref.analyse(q[i], wc)["key"]
        assert chords2[i].tolist() == ref.analyse(q[i], wc, given_tonic=5, analyse_key=False)["chords"]
    assert (key2 == -1).all() and (coef2 == 0.0).all()


def test_hand_built_rolls():
    """slices one pitch apart at 21 / 108 / in the second mask word, a slice across the window boundary, equal lengths, long silence, a
    velocity change, the last column alone, root ties, the widest window -- junk in rows 0..20 and 109..127 of every roll, handed
    straight to the ABI"""
    for name, q, wc, roots in ref.hand_cases():
        assert (q[:21] > 0).any() and (q[109:] > 0).any()
        got = _run(q, wc)
        assert got[1][0].tolist() == roots, (name, got[1][0].tolist())
        _check(q[None], wc)


def test_no_key_cases_and_short_rolls():
    z = np.zeros((128, 1024), dtype=np.uint8)
    z[:21], z[109:] = 99, 99
    flat = np.zeros((128, 1024), dtype=np.uint8)
    flat[60:72, :512] = 64
    chords, roots, key, coef = _run(np.stack([z, flat]), 128, given_tonic=3)
    assert (chords == 0).all() and (key == -1).all() and (coef == 0.0).all()
    assert roots[0].tolist() == [-1] * 8 and roots[1].tolist() == [0] * 4 + [-1] * 4
    # no key analysis: the given tonic still gives degrees (E- as tonic: C is its sixth)
    chords, _, _, _ = _run(np.stack([z, flat]), 128, given_tonic=3, analyse_key=False)
    assert chords[0].tolist() == [0] * 8 and chords[1].tolist() == [6] * 4 + [0] * 4
    # shorter than one window: no chords, the key from the columns there are
    q = ref.random_roll(3, 100)
    chords, roots, key, coef = _run(q, 128)
    want = ref.analyse(q, 128)
    assert chords.shape == (1, 0) and want["gap"] >= MIN_GAP and int(key[0]) == want["key"] and abs(float(coef[0]) - want["coef"]) <= COEF_TOL


def test_arguments_are_checked_before_any_launch(native):
    from rgm.native import RgmError
    q = torch.zeros((1, 128, 128), dtype=torch.uint8, device="cuda")
    for wc in (0, 1025, -1):
        with pytest.raises(ValueError):
            native.chords_native(q, wc)
    with pytest.raises(ValueError):
        native.chords_native(q, 128, "temperley")
    with pytest.raises(ValueError):
        native.chords_native(q, 128, analyse_key=False)
    with pytest.raises(ValueError):
        native.chords_native(q.float(), 128)
    with pytest.raises(RgmError):
        native.chords_native(q.cpu(), 128)
    x = torch.from_numpy(ref.float_roll(np.zeros((128, 128), dtype=np.uint8))).cuda()
    keep = x.clone()
    for kw in (dict(fs=100, window_size=1.285), dict(fs=100, window_size=10.25), dict(given_key="H major")):
        with pytest.raises(ValueError):
            native.get_chords(x, **kw)
        with pytest.raises(ValueError):
            native.get_chords_async(x, **kw)
    assert torch.equal(x, keep)                                   # refused before the preamble wrote anything


@pytest.mark.parametrize("rule,T,wc", [("chord_progression", 1024, 128), ("chord_progression_pixel", 128, 16)])
def test_func_dict_on_float_device_rolls(native, rule, T, wc):
    """the 24 keys in one batch through FUNC_DICT: known degrees and keys, the preamble's writes in the caller's roll, the N == 1 squeeze"""
    from music_rule_guidance.rule_maps import FUNC_DICT
    built = [ref.progression_roll(k % 12, k // 12, T=T, wc=wc, seed=k) for k in range(24)]
    q = np.stack([b[0] for b in built])
    degs = [b[1] for b in built]
    for profile in ("krumhansl", "aarden"):
        native.register_chord_backend("native", profile=profile)
        for k in range(24):
            want = ref.analyse(q[k], wc, profile)
            assert want["gap"] >= MIN_GAP and want["key"] == k and want["chords"] == degs[k]
        x = torch.from_numpy(ref.float_roll(q, seed=1)).cuda()
        twin = x.clone()
        chords, keys, coefs = FUNC_DICT[rule](x, return_key=True)
        assert chords.is_cuda and chords.dtype == torch.int64 and chords.tolist() == degs
        assert isinstance(keys, list) and keys == [native.KEY_DICT[native.CHORD_KEY_NAMES[k]] for k in range(24)]
        assert [native.IND2KEY[c] for c in keys] == [ref.key_name(k) for k in range(24)]
        assert isinstance(coefs, list) and all(abs(c - ref.analyse(q[k], wc, profile)["coef"]) <= COEF_TOL for k, c in enumerate(coefs))
        native.chord_quantise(twin)
        assert torch.equal(x, twin) and not torch.equal(x, torch.from_numpy(ref.float_roll(q, seed=1)).cuda())
        assert torch.equal(FUNC_DICT[rule](x.clone()), chords)                     # without return_key: the chords alone
        # a given key: degrees relative to it, nothing read back
        given = FUNC_DICT[rule](x.clone(), given_key="E- major")
        assert given.tolist() == [ref.analyse(q[k], wc, given_tonic=3, analyse_key=False)["chords"] for k in range(24)]
        # N == 1 squeezes, through the future too; a CPU roll is staged and answered on the CPU
        one = FUNC_DICT[rule](x[5:6].clone())
        assert one.shape == (T // wc,) and one.tolist() == degs[5]
        kw = {} if rule == "chord_progression" else dict(fs=12.5)
        fut = native.get_chords_async(x[5:6].clone(), return_key=True, **kw)
        assert fut.done() and fut.result()[0].shape == (T // wc,) and fut.result()[0].is_cuda and fut.result()[1] == [keys[5]]
        cpu = FUNC_DICT[rule](x[:3].cpu())
        assert not cpu.is_cuda and cpu.tolist() == degs[:3]


def test_launches_repeat_bitwise_and_rows_do_not_depend_on_the_batch():
    q = np.stack([ref.random_roll(10 + i, 1064) for i in range(5)])
    first = _run(q, 100)
    for _ in range(19):
        again = _run(q, 100)
        for a, b in zip(first, again):
            assert a.tobytes() == b.tobytes()
    alone = _run(q[3], 100)
    for a, b in zip(first, alone):
        assert a[3].tobytes() == b[0].tobytes()


def _scg_setup(n=4):
    from gpu_util import dev
    from guided_diffusion.gaussian_diffusion import PhiloxNoise
    from test_gpu_sampler import SM, _diffusion, _dit, _model_fn, _vae
    g = load_golden("steps")
    m, vae = _dit(SM, 11), _vae(2)
    rules = {"note_density": dev(g["scg.target.note_density"]),
             "chord_progression": torch.tensor([[1, 4, 5, 1, 6, 2, 5, 1]] * 2, dtype=torch.long, device="cuda")}
    scg = dict(num_samples=n, note_density=1., chord_progression=2.)

    def run(base):
        guid = SimpleNamespace(schedule=True, t_start=750, t_end=0, interval=1, method="no_guidance", dc=SimpleNamespace(base=base))
        d = _diffusion("")
        d.t_end = 0
        d.noise = PhiloxNoise(seed=99)
        out = d.p_sample(_model_fn(m), dev(g["x"]), dev(g["scg.t"]), clip_denoised=False, model_kwargs={"y": dev(g["y"]), "rule": rules},
                         embed_model=vae, scale_factor=1.2465, guidance_kwargs=guid, scg_kwargs=scg)
        return out["sample"].clone(), d.last_scg["total_log_prob"].clone(), d.last_scg["max_ind"].clone()
    return run


def test_search_step_is_the_same_under_the_device_and_the_host_analyser(monkeypatch):
    """one SCG step (B = 2, n = 4; chord rule + note density) of the synthetic eps-network and decoder: the chord rule scored on the
    device against the host partner piano_roll_to_chords_native through the existing host path -- log-probability table, winners and
    sample bit for bit, with the analyser beside the GPU (RGM_CHORD_ASYNC 1), in the blocking order (0) and per segment (dc.base)."""
    import guided_diffusion.gaussian_diffusion as gd
    from music_rule_guidance import music_rules
    from music_rule_guidance.piano_roll_to_chord import piano_roll_to_chords_native
    run = _scg_setup()
    try:
        for base in (0, 64):
            results = {}
            for asyn in (True, False):
                monkeypatch.setattr(gd, "CHORD_ASYNC", asyn)
                for backend in ("native", piano_roll_to_chords_native):
                    music_rules.register_chord_backend(backend, workers=0)
                    assert gd._async_chord_rules({"note_density": None, "chord_progression": None}) == (["chord_progression"] if asyn else [])
                    results[(asyn, backend == "native")] = run(base)
            for asyn in (True, False):
                device, host = results[(asyn, True)], results[(asyn, False)]
                assert device[1].shape == ((4, 2, 2) if base else (4, 2)) and torch.isfinite(device[1]).all()
                for a, b in zip(device, host):
                    assert torch.equal(a, b), (base, asyn)
    finally:
        music_rules.register_chord_backend(None)


def test_sample_rule_cli_with_the_native_backend(tmp_path, monkeypatch):
    """scripts/sample_rule.py --chord_backend native on a shipped chord config, two solver steps: it runs, nothing is dropped, the
    metadata names the backend and the report carries the chord columns"""
    import pandas as pd
    from music_rule_guidance import music_rules
    from test_gpu_cli import CFG, COMMON, _cli
    monkeypatch.chdir(tmp_path)
    cli = _cli()
    cfg = os.path.join(CFG, "cond_table/single/scg/chord.yml")
    try:
        res = cli.main(["--config_path", cfg, "--batch_size", "2", "--num_samples", "2", "--diffusion_steps", "24", "--sampler", "dpmpp",
                        "--dpmpp_steps", "2", "--chord_backend", "native", "--chord_profile", "aarden"] + COMMON)
        assert music_rules.native_chord_backend()
    finally:
        music_rules.register_chord_backend(None)
    out_dir = os.path.join("loggings", cli.output_dir_for(cfg, 1))
    meta = json.load(open(os.path.join(out_dir, "run_metadata.json")))
    assert meta["chord_backend"] == "native" and meta["chord_profile"] == "aarden" and not meta["dropped_rules"]
    df = pd.read_csv(os.path.join(out_dir, "results.csv"))
    assert len(df) == 2 and len(res) == 2
    cols = {"chord_progression." + c for c in ("target_rule", "gen_rule", "loss", "key_str", "key_corr")}
    assert cols <= set(df.columns), df.columns
    assert np.isfinite(df["chord_progression.loss"]).all() and all(len(json.loads(g)) == 8 for g in df["chord_progression.gen_rule"])
    assert all(k in music_rules.KEY_DICT for k in df["chord_progression.key_str"])
