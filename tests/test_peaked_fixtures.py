"""CPU: the peaked-softmax model fixture (tests/golden/make_golden_peaked.py: rgm.synth weights with the q and k rows of every qkv layer
multiplied by one gain, so that the attention scores reach 30 to 60) against the numpy oracle, its seeds and its gain against the
generator's own table, and the property it exists for: the score scale."""
import ast
import glob
import os

import numpy as np
import pytest

import attn_cases as A
from conftest import GOLDEN, load_golden, rel_err
from oracle import dit_np as odit
from rgm import synth

XL2 = dict(depth=2, hidden=1152, heads=16, patch=8, in_ch=4, out_ch=4, num_classes=3)
CLS2 = dict(depth=2, hidden=384, heads=6, patch=8, in_ch=4, classifier=True, cls_classes=16)


def _generator(name):
    src = open(os.path.join(GOLDEN, "make_golden_peaked.py")).read()
    node = next(n for n in ast.parse(src).body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == name)
    return ast.literal_eval(node.value)


def _randn(seed, *shape):
    return np.random.RandomState(int(seed)).randn(*shape).astype(np.float32)


def _weights(g, tag, arch):
    return A.peak_qk(synth.dit_state_dict(int(g[f"{tag}.seed"][0]), **arch), float(g["qk_gain"][0]))


def test_peaked_fixture_carries_the_seeds_and_the_gain_the_generator_pins():
    table = _generator("PEAKED_SEEDS")["peaked"]
    paths = sorted(glob.glob(os.path.join(GOLDEN, "peaked*.npz")))
    assert [os.path.basename(p) for p in paths][0] == "peaked.npz"
    for path in paths:
        g = np.load(path)
        keys = [k for k in g.files if k.endswith("seed")]
        assert os.path.getsize(path) < 1024 * 1024, path
        if ".part" in os.path.basename(path):
            assert not keys and "qk_gain" not in g.files, path
            continue
        assert all(g[k].shape == (1,) for k in keys), path
        assert {k: int(g[k][0]) for k in keys} == table
        assert g["qk_gain"].shape == (1,) and float(g["qk_gain"][0]) == _generator("QK_GAIN")
    g = load_golden("peaked")
    assert not any(k.endswith(".x128") or k.endswith(".x256") or ".c" in k for k in g)          # inputs are rebuilt from their seeds
    for k in g:
        if k.endswith("_64"):
            assert g[k].dtype == np.float64 and g[k[:-2] + "32"].dtype == np.float32 and g[k].shape == g[k[:-2] + "32"].shape, k


@pytest.mark.parametrize("H", [128, 256])
def test_peaked_eps_network_oracle_and_score_scale(H):
    g = load_golden("peaked")
    sd = _weights(g, "xl2", XL2)
    x = _randn(g[f"xl2.x{H}_seed"][0], 1, 4, H, 16)
    out = {}
    scores = A.model_max_scores(sd, 16, lambda: out.update(eps=odit.dit_forward(sd, x, g[f"xl2.t{H}"], g[f"xl2.y{H}"], depth=2, heads=16)))
    lo, hi = _generator("SCORE_RANGE")
    assert len(scores) == 2 and all(lo <= s <= hi for s in scores), scores
    plain = synth.dit_state_dict(int(g["xl2.seed"][0]), **XL2)
    flat = A.model_max_scores(plain, 16, lambda: odit.dit_forward(plain, x, g[f"xl2.t{H}"], g[f"xl2.y{H}"], depth=2, heads=16))
    assert max(flat) < 8, flat                                   # what every other model-level fixture runs: a nearly flat softmax
    # the float32 oracle against the reference in both precisions, and the reference against itself (a quarter of the GPU tolerances)
    assert rel_err(out["eps"], g[f"xl2.eps{H}_32"]) < 1e-4 and rel_err(out["eps"], g[f"xl2.eps{H}_64"]) < 1e-4
    assert rel_err(g[f"xl2.eps{H}_32"], g[f"xl2.eps{H}_64"]) <= 2e-4 / 4
    assert rel_err(g[f"xl2.grad{H}_32"], g[f"xl2.grad{H}_64"]) <= 5e-4 / 4
    assert np.isfinite(g[f"xl2.grad{H}_64"]).all() and g[f"xl2.grad{H}_64"].shape == x.shape


@pytest.mark.parametrize("H", [128, 256])
def test_peaked_classifier_oracle_backward_and_score_scale(H):
    g = load_golden("peaked")
    sd = _weights(g, "cls", CLS2)
    x = _randn(g[f"cls.x{H}_seed"][0], 2, 4, H, 16)
    out = {}
    scores = A.model_max_scores(sd, 6, lambda: out.update(r=odit.grad_nn_zt_mse(sd, x, g[f"cls.t{H}"], g[f"cls.rule{H}"], 10., depth=2, heads=6)))
    lo, hi = _generator("SCORE_RANGE")
    assert len(scores) == 2 and all(lo <= s <= hi for s in scores), scores
    grad, logits = out["r"]
    assert rel_err(logits, g[f"cls.logits{H}_32"]) < 1e-4 and rel_err(logits, g[f"cls.logits{H}_64"]) < 1e-4
    assert rel_err(grad, g[f"cls.grad{H}_32"]) < 2e-4 and rel_err(grad, g[f"cls.grad{H}_64"]) < 2e-4
    assert rel_err(g[f"cls.logits{H}_32"], g[f"cls.logits{H}_64"]) <= 2e-4 / 4
    assert rel_err(g[f"cls.grad{H}_32"], g[f"cls.grad{H}_64"]) <= 5e-4 / 4
