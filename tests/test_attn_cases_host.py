"""Keeps the attention input families honest without a GPU (tests/attn_cases.py, used on the kernels by test_gpu_attn_inputs.py):
every family at every shape up to T = 2080 is well conditioned (the float32 reference stays within 1e-3 of float64 in every block) and has
the property it is built for; the headroom R_p of every shape is printed; and three deliberately wrong variants of the float64 reference
(mutants of the reference arithmetic on the CPU -- nothing runs on a GPU) exceed the new bound where the old norm-wise checks let them pass."""
import math

import numpy as np
import pytest

import attn_cases as A

SHAPES = A.RESIDENT_SHAPES + A.STREAM_SHAPES
CASES = ([(f, s) for s in SHAPES for f in A.FAMILIES + A.FORWARD_ONLY] + [(f, s) for s in A.PAIR_SHAPES for f in A.PAIR_FAMILIES]
         + [("zeroq", s) for s in A.KEYCOUNT_SHAPES if s[1] <= 2080])


def _ids(case):
    return f"{case[0]}-{A.shape_id(case[1])}"


def _scores(fam, shape):
    """scaled float64 scores of every (sample, head) of a case, one at a time"""
    N, T, heads, hd = shape
    qkv, _ = A.inputs(fam, shape)
    pairs = [(n, h) for n in range(N) for h in range(heads)]
    if N > 3:                                                    # the many-pair shapes: a sample of the pairs
        pairs = pairs[::37]
    for n, h in pairs:
        yield A.scaled_scores(qkv, *shape, n=n, h=h)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_family_is_well_conditioned_and_does_what_it_says(case):
    fam, shape = case
    N, T, heads, hd = shape
    qkv, d_o = A.inputs(fam, shape)
    r32 = A.ref32(qkv, d_o, *shape, backward=A.has_backward(fam))
    assert all(np.isfinite(v).all() for v in r32.values()), case
    err = A.errors(r32, fam, shape)
    print(f"{fam} {A.shape_id(shape)}: ref32 vs ref64 worst block " + ", ".join(f"{k} {v.max():.2e}" for k, v in err.items()))
    for quantity, e in err.items():
        assert e.max() < 1e-3, (case, quantity, e.max())         # no degenerate block: a relative error means something in each
    ref = A.reference(fam, shape)
    if fam in A.MAX_SCORE:
        mx = max(np.abs(s).max() for s in _scores(fam, shape))
        assert A.MAX_SCORE[fam] / 1.5 <= mx <= A.MAX_SCORE[fam] * 1.5, (case, mx)
    if fam == "ramp_up":
        # the running maximum still grows in the final key block: in every (sample, head) there are rows whose maximum sits there, and no
        # row has it in the first half of the keys.  (Where the final block is a lone key -- T = 257, 1025 -- that is a minority of the rows.)
        last = ((T + A.KEY_BLOCK - 1) // A.KEY_BLOCK - 1) * A.KEY_BLOCK
        for s in _scores(fam, shape):
            am = s.argmax(-1)
            assert (am >= last).any() and (am >= T // 2).all(), (case, float((am >= last).mean()), int(am.min()))
    if fam == "ramp_down":
        for s in _scores(fam, shape):                            # the maximum settles in the first half and never grows after it
            assert (s.argmax(-1) < T // 2).all(), case
    if fam in ("lastkey", "firstkey", "jump"):
        key = 0 if fam == "firstkey" else T - 1
        for s in _scores(fam, shape):
            assert (s.argmax(-1) == key).all(), case             # the largest probability of every row is on the chosen key
    if fam == "jump":
        v_last = qkv.reshape(N, T, 3, heads, hd)[:, T - 1, 2].astype(np.float64)            # (N, heads, hd)
        for r in (ref, r32):                                     # o is v[T-1] exactly, in float64 and in the float32 reference
            assert np.array_equal(np.asarray(r["o"], np.float64).reshape(N, T, heads, hd), np.broadcast_to(v_last[:, None], (N, T, heads, hd)))
        assert 150 < ref["lse"].min() and ref["lse"].max() < 200
    if fam == "zeroq":
        v = qkv.reshape(N, T, 3, heads, hd)[:, :, 2].astype(np.float64)
        assert np.abs(ref["lse"] - math.log(T)).max() < 1e-12
        assert np.abs(ref["o"].reshape(N, T, heads, hd) - v.mean(axis=1, keepdims=True)).max() < 1e-12
    if fam == "headscale":
        scale = np.abs(ref["dqkv"].reshape(N, T, 3, heads, hd)).max(axis=(1, 4))             # (N, 3, heads)
        assert scale[:, 2].max() / scale[:, 2].min() > 500 and scale[:, 0].max() / scale[:, 0].min() > 2e5, scale


@pytest.mark.parametrize("shape", SHAPES + A.PAIR_SHAPES, ids=A.shape_id)
def test_headroom_of_every_shape(shape):
    """R_p of both directions and both arithmetics (the table of docs/rounds/attn_inputs.md); by its definition never below 1"""
    for precision in ("fp32", "bf16x3"):
        for direction in ("fwd", "bwd"):
            R, worst = A.headroom(precision, direction, shape)
            print(f"R_p {A.shape_id(shape)} {precision} {direction}: {R:.2f} (twin's worst block on randn {worst:.2e}, "
                  f"TOL {A.tolerances()[direction][precision]:.0e})")
            assert R >= 1.0 and np.isfinite(R)


# ------------------------------------------------------------------------------------------------ sensitivity: mutants of the reference
def _forward_exceeds(mutant, fam, shape):
    qkv, _ = A.inputs(fam, shape)
    err = A.errors(A.blocked64(qkv, *shape, mutant=mutant), fam, shape)
    bo, bl = A.bound("fp32", "o", fam, shape), A.bound("fp32", "lse", fam, shape)
    print(f"mutant {mutant} on {fam} {A.shape_id(shape)}: o {err['o'].max():.2e} (bound {bo.max():.2e}), lse {err['lse'].max():.2e} (bound {bl:.2e})")
    return not (A.within(err["o"], bo) and A.within(err["lse"], bl))


@pytest.mark.parametrize("shape", [(2, 257, 6, 64), (2, 300, 6, 64), (1, 1000, 4, 72)], ids=A.shape_id)
def test_blocked_restatement_is_the_reference(shape):
    """the flash-style float64 walk the mutants are made from reproduces ref64 far inside the fp32 bound"""
    for fam in ("ramp_up", "rowshift", "jump"):
        qkv, _ = A.inputs(fam, shape)
        err = A.errors(A.blocked64(qkv, *shape), fam, shape)
        assert err["o"].max() < 1e-9 and err["lse"].max() < 1e-12, (fam, shape, err["o"].max(), err["lse"].max())


@pytest.mark.parametrize("shape", [(2, 257, 6, 64), (2, 300, 6, 64), (1, 1000, 4, 72)], ids=A.shape_id)
def test_missing_rescale_in_the_final_block_is_caught(shape):
    caught = [fam for fam in ("ramp_up", "lastkey", "jump", "randn") if _forward_exceeds("no_final_rescale", fam, shape)]
    assert "ramp_up" in caught and "lastkey" in caught and "jump" in caught, caught


@pytest.mark.parametrize("shape", [(1, 37, 6, 64), (2, 257, 6, 64), (2, 300, 6, 64), (1, 1000, 4, 72)], ids=A.shape_id)
def test_a_masked_key_counted_with_score_zero_is_caught(shape):
    caught = [fam for fam in ("ramp_down", "rowshift", "peaked3", "randn") if _forward_exceeds("extra_key", fam, shape)]
    assert "rowshift" in caught, caught


def test_a_masked_key_at_8192_passes_the_old_lse_check_and_fails_the_key_count():
    """The gap the key-count check closes: with q = 0 one key too many at T = 8192 moves lse by 1.2e-4, norm-wise 1.4e-5 of a value near 9
    -- inside the suite's bf16x3 lse tolerance (2e-5), 12 times the key-count tolerance."""
    shape = (1, 8192, 1, 64)
    qkv, _ = A.family("zeroq", *shape, 3)
    lse = A.blocked64(qkv, *shape, mutant="extra_key")["lse"]
    ref = np.full_like(lse, math.log(8192))
    old = A.rel(lse, ref)
    print(f"extra key at T = 8192: lse off by {np.abs(lse - ref).max():.3e}, norm-wise {old:.3e}")
    assert old < A.tolerances()["fwd"]["bf16x3"]
    assert np.abs(lse - ref).max() > 1e-5


def test_a_quiet_head_off_by_1e_3_is_caught_where_the_norm_wise_measure_is_blind():
    shape = (1, 1000, 4, 72)
    N, T, heads, hd = shape
    ref = A.reference("headscale", shape)
    wrong = ref["dqkv"].reshape(N, T, 3, heads, hd).copy()
    scale = np.abs(wrong).max(axis=(1, 4))
    quiet = int(scale[0, 0].argmin())
    wrong[:, :, 0, quiet] *= 1.0 + 1e-3                          # dq of the quietest head
    wrong = wrong.reshape(ref["dqkv"].shape)
    old = A.rel(wrong, ref["dqkv"])
    err = A.block_err(wrong, ref["dqkv"], *shape)
    bnd = A.bound("fp32", "dqkv", "headscale", shape)
    print(f"quiet head {quiet}: norm-wise {old:.3e} (old tolerance {A.tolerances()['bwd']['fp32']:.0e}), its block {err[0, 0, quiet]:.3e} "
          f"(bound {bnd[0]:.3e})")
    assert old < A.tolerances()["bwd"]["fp32"]                   # today's check passes it
    assert abs(err[0, 0, quiet] - 1e-3) < 1e-5 and not A.within(err, bnd)
    for precision in ("bf16x3", "bf16x3_presplit"):              # and the looser bf16x3 bound still catches it
        assert not A.within(err, A.bound(precision, "dqkv", "headscale", shape))


def test_block_err_reports_non_finite_and_single_blocks():
    shape = (2, 5, 3, 64)
    b = np.random.RandomState(0).randn(10, 3 * 3 * 64)
    a = b.copy()
    a.reshape(2, 5, 3, 3, 64)[1, 2, 1, 2, 7] += 0.5
    e = A.block_err(a, b, *shape)
    assert e.shape == (2, 3, 3) and e[1, 1, 2] > 0 and (np.delete(e.ravel(), np.ravel_multi_index((1, 1, 2), e.shape)) == 0).all()
    a.reshape(2, 5, 3, 3, 64)[0, 0, 0, 0, 0] = np.nan
    assert np.isinf(A.block_err(a, b, *shape)[0, 0, 0]) and not A.within(A.block_err(a, b, *shape), np.full(3, 1e30))
    lse = np.zeros((2, 3, 5))
    assert A.lse_err(lse + 1e-3, lse).max() == pytest.approx(1e-3)


def test_the_split_is_the_documented_one():
    """hi = bf16(x) round to nearest even, lo = bf16(x - hi): against torch's own conversion; x - hi - lo stays below 2^-16 |x|"""
    import torch
    x = (np.random.RandomState(1).randn(20000) * 10.0 ** np.random.RandomState(2).uniform(-6, 3, 20000)).astype(np.float32)
    hi, lo = A.split_parts(x)
    t = torch.from_numpy(x)
    th = t.to(torch.bfloat16).float()
    assert np.array_equal(hi, th.numpy().astype(np.float64))
    assert np.array_equal(lo, (t - th).to(torch.bfloat16).float().numpy().astype(np.float64))
    assert (np.abs(x - hi - lo) <= 2.0 ** -16 * np.abs(x)).all()
    h16, l16 = A.split_parts(x[np.abs(x) < 6e4], torch.float16)
    assert np.array_equal(h16, x[np.abs(x) < 6e4].astype(np.float16).astype(np.float64))
