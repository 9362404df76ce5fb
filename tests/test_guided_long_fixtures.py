"""CPU: the guided long-excerpt fixtures (tests/golden/make_golden_guided_long.py: the reference's autograd beyond 256 tokens) against
the numpy / torch-CPU oracle, and their seeds against the generator's own table."""
import ast
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden, rel_err
from oracle import dit_np as odit
from rgm import synth

XL2 = dict(depth=2, hidden=1152, heads=16, patch=8, in_ch=4, out_ch=4, num_classes=3)
CLS2 = dict(depth=2, hidden=384, heads=6, patch=8, in_ch=4, classifier=True, cls_classes=16)
CLS12 = dict(CLS2, depth=12)
CHD = dict(depth=2, hidden=384, heads=6, patch=8, in_ch=4, classifier=True, cls_classes=8, chord=True)


def _table():
    src = open(os.path.join(GOLDEN, "make_golden_guided_long.py")).read()
    node = next(n for n in ast.parse(src).body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "GUIDED_LONG_SEEDS")
    return ast.literal_eval(node.value)


def _randn(seed, *shape):
    return np.random.RandomState(int(seed)).randn(*shape).astype(np.float32)


def test_guided_long_fixtures_carry_the_seeds_the_generator_pins():
    """every guidedlong_* fixture holds exactly the seeds of its GUIDED_LONG_SEEDS entry, as one-element arrays (never 0-d: those belong
    to make_golden.py's FIXTURE_SEEDS); continuation parts hold no seed; every entry has its fixture; no file reaches 1 MiB"""
    table = _table()
    seen = {}
    paths = sorted(glob.glob(os.path.join(GOLDEN, "guidedlong_*.npz")))
    for path in paths:
        g = np.load(path)
        keys = [k for k in g.files if k.endswith("seed")]
        assert all(g[k].shape == (1,) for k in keys), path
        assert os.path.getsize(path) < 1024 * 1024, path
        name = os.path.basename(path)[:-4]
        if ".part" in name:
            assert not keys, path
            continue
        seen[name] = {k: int(g[k][0]) for k in keys}
    assert seen == table
    steps = load_golden("guidedlong_steps")
    assert not any(k in steps for k in ("x", "noise", "gt"))      # inputs are rebuilt from their seeds, never stored
    assert "must match the size" in str(steps["edit.reference_raises"]) and "editfull.sample" in steps


@pytest.mark.parametrize("tag,arch,H,B", [("s8d2", CLS2, 256, 2), ("s8", CLS12, 256, 2), ("s8d2", CLS2, 512, 1)])
def test_oracle_backward_matches_reference_autograd_mse(tag, arch, H, B):
    """the hand-written numpy backward reproduces the reference's autograd at T = 513 / 1025 tokens (cls token included)"""
    g = load_golden("guidedlong_cls")
    sd = synth.dit_state_dict(int(g[f"{tag}.seed"][0]), **arch)
    x = _randn(g[f"{tag}.x{H}_seed"][0], B, 4, H, 16)
    grad, logits = odit.grad_nn_zt_mse(sd, x, g[f"{tag}.t{H}"], g[f"{tag}.rule{H}"], 10., depth=arch["depth"], heads=arch["heads"])
    assert grad.shape == x.shape
    assert rel_err(logits, g[f"{tag}.logits{H}"]) < 1e-4
    assert rel_err(grad, g[f"{tag}.grad{H}"]) < 1e-4


def test_oracle_backward_matches_reference_autograd_chord():
    g = load_golden("guidedlong_cls")
    sd = synth.dit_state_dict(int(g["chord.seed"][0]), **CHD)
    x = _randn(g["chord.x256_seed"][0], 2, 4, 256, 16)
    grad, (key, ch) = odit.grad_nn_zt_chord(sd, x, g["chord.t256"], g["chord.rule256"], 10., depth=2, heads=6)
    assert rel_err(key, g["chord.key256"]) < 1e-4 and rel_err(ch, g["chord.logits256"]) < 1e-4
    assert rel_err(grad, g["chord.grad256"]) < 1e-4


@pytest.mark.parametrize("H", [136, 256, 512])
def test_torch_oracle_forward_matches_the_eps_of_the_vjp_fixture(H):
    """oracle/dit_torch.py: dit_forward runs under torch.no_grad() as written, so it is not differentiable: its FORWARD is held to the
    eps the reference computed beside the input gradient at T = 272 / 512 / 1024 tokens (the gradient itself is checked on the GPU)"""
    import torch
    from oracle import dit_torch as odt
    g = load_golden("guidedlong_vjp")
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.dit_state_dict(int(g["xl2.seed"][0]), **XL2).items()}
    x = torch.from_numpy(_randn(g[f"xl2.x{H}_seed"][0], 1, 4, H, 16))
    eps = odt.dit_forward(sd, x, torch.from_numpy(g[f"xl2.t{H}"]), torch.from_numpy(g[f"xl2.y{H}"]), depth=2, heads=16)
    assert g[f"xl2.grad{H}"].shape == tuple(x.shape) and np.isfinite(g[f"xl2.grad{H}"]).all()
    assert rel_err(np.asarray(eps), g[f"xl2.eps{H}"]) < 1e-4
