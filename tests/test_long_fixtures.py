"""CPU: the long-excerpt fixtures (tests/golden/make_golden_long.py: the reference's DiTRotary beyond 256 tokens) against the numpy
oracle, and their seeds against the generator's own table."""
import ast
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden, rel_err
from oracle import dit_np as odit
from rgm import synth

XL2 = dict(depth=2, hidden=1152, heads=16, patch=8, in_ch=4, out_ch=4, num_classes=3)


def _long_seeds():
    src = open(os.path.join(GOLDEN, "make_golden_long.py")).read()
    node = next(n for n in ast.parse(src).body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "LONG_SEEDS")
    return ast.literal_eval(node.value)


def test_long_fixtures_carry_the_seeds_the_generator_pins():
    """make_golden_long.py keeps its own seed table (LONG_SEEDS) and stores every seed as a one-element array; every long_* fixture
    holds exactly the seeds of its entry, and every entry has its fixture."""
    table = _long_seeds()
    seen = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, "long_*.npz"))):
        g = np.load(path)
        keys = [k for k in g.files if k.endswith("seed")]
        assert all(g[k].shape == (1,) for k in keys), path       # never 0-d: make_golden.py's FIXTURE_SEEDS covers those
        seen[os.path.basename(path)[:-4]] = {k: int(g[k][0]) for k in keys}
    assert seen == table
    for path in glob.glob(os.path.join(GOLDEN, "long_*.npz")):
        assert os.path.getsize(path) < 1024 * 1024


@pytest.mark.parametrize("H", [136, 256, 512])
def test_oracle_matches_long_reference_forward(H):
    """the numpy oracle (unchanged) reproduces the reference's DiTRotary at T = 2H = 272 / 512 / 1024 tokens: the same model code
    serves any length, rotary positions included"""
    g = load_golden("long_dit_xl2")
    sd = synth.dit_state_dict(int(g["seed"][0]), **XL2)
    x, t, y = g[f"x{H}"], g[f"t{H}"], g[f"y{H}"]
    out = odit.dit_forward(sd, x, t, y, depth=2, heads=16)
    assert out.shape == x.shape
    assert rel_err(out, g[f"out{H}"]) < 1e-4


@pytest.mark.parametrize("H", [1040, 4096])
def test_oracle_matches_long_reference_forward_at_the_edges(H):
    """the numpy oracle reproduces the reference at T = 2080 (partial last query tile and key block of the streaming kernel) and at
    its ceiling T = 8192: the stored slices (the first and last 64 latent rows, every 16th between) of an input rebuilt from its seed"""
    g = load_golden("long_dit_xl2_edge")
    sd = synth.dit_state_dict(int(g["seed"][0]), **XL2)
    t, y, rows = g[f"t{H}"], g[f"y{H}"], g[f"rows{H}"]
    x = np.random.RandomState(int(g[f"x{H}_seed"][0])).randn(len(t), 4, H, 16).astype(np.float32)
    assert rows[0] == 0 and rows[-1] == H - 1 and np.array_equal(rows[:64], np.arange(64))
    out = odit.dit_forward(sd, x, t, y, depth=2, heads=16)
    assert out.shape == x.shape
    assert rel_err(out[:, :, rows], g[f"out{H}"]) < 1e-4
