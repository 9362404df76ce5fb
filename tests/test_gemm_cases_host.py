"""CPU: the inputs, comparators, bound and mutants of tests/gemm_cases.py -- what tests/test_gpu_gemm_inputs.py holds the GEMM and LayerNorm
kernels to (docs/rounds/gemm_inputs.md).  Nothing here runs a kernel; RGM_GEMM_HOST lines carry the figures of the document's tables."""
import json

import numpy as np
import pytest

import gemm_cases as gc

ALL_SHAPES = gc.HOST_SHAPES + gc.SHAPES + gc.SHAPES_144 + [gc.SPLITK_SHAPE]
BENIGN = ("offset", "outlier", "wide")


def _report(**kw):
    print("RGM_GEMM_HOST " + json.dumps(kw))


def test_block_err_measures_every_block_on_its_own():
    rng = np.random.RandomState(0)
    ref = rng.randn(40, 50)
    got = ref.copy()
    got[17, 33] += 1e-3                                              # block (1, 2)
    e = gc.block_err(got, ref)
    assert e.shape == (3, 4)
    assert e[1, 2] > 0 and np.count_nonzero(e) == 1
    assert np.isclose(e[1, 2], 1e-3 / np.linalg.norm(ref[16:32, 32:48]))
    got[39, 49] = np.nan                                             # the partial corner block (8 x 2)
    assert gc.block_err(got, ref)[2, 3] == np.inf and not gc.within(gc.block_err(got, ref), 1.0)
    zero = np.zeros((16, 16))
    assert gc.block_err(zero, zero)[0, 0] == 0.0 and gc.block_err(zero + 1e-30, zero)[0, 0] == np.inf
    assert gc.worst(e) == (e[1, 2], (1, 2))
    assert np.allclose(gc.row_err(got[:17], ref[:17])[:16], 0) and gc.row_err(got, ref)[39] == np.inf


@pytest.mark.parametrize("shape", gc.HOST_SHAPES, ids=gc.shape_id)
def test_families_have_the_properties_they_are_built_for(shape):
    M, N, K = shape
    p = {f: gc.properties(f, shape) for f in gc.FAMILIES}
    _report(kind="family", shape=gc.shape_id(shape), **{f: {k: v for k, v in p[f].items() if k != "nonzero_tiles"} for f in gc.FAMILIES})
    assert p["randn"]["offset_ratio"] < 0.02 and 45 < p["offset"]["offset_ratio"] < 55          # DC part 50 standard deviations out
    assert p["outlier"]["top2_share"] > 0.3 and p["randn"]["top2_share"] < 2.5 * 2 / K * 1.2 + 0.02   # two channels carry a third or more of sum |a||b|
    assert p["outlier"]["top_tile_share"] > 5 * p["randn"]["top_tile_share"] or p["outlier"]["top_tile_share"] > 0.9
    assert p["wide"]["dyn_range"] > p["randn"]["dyn_range"] + 10                                # lo halves 2^-10 and more below the row's scale
    assert p["cancel"]["cancel_ratio"] < 3e-4 < 0.02 < p["randn"]["cancel_ratio"]               # result ~1e-4 of sum |a||b|
    for f in gc.KT_FAMILIES:
        assert p[f]["nonzero_tiles"] == [gc.ktile_index(f, K)]
    assert len(p["randn"]["nonzero_tiles"]) == K // gc.KTILE
    A, B = gc.family("cancel", M, N, K, gc.case_seed(shape))
    assert np.array_equal(B[:, K // 2:], -B[:, :K // 2])
    bias = gc.bias_of("tails", N, gc.case_seed(shape))
    assert set(np.unique(bias)) <= set(gc.TAIL_BIASES) and (N < 64 or len(np.unique(bias)) == len(gc.TAIL_BIASES))
    assert not gc.bias_of("cancel", N, 0).any()
    for f in gc.FAMILIES:                                                                       # deterministic in (name, M, N, K, seed)
        assert all(np.array_equal(a, b) for a, b in zip(gc.family(f, M, N, K, 5), gc.family(f, M, N, K, 5)))


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=gc.shape_id)
def test_comparators_against_float64_and_the_headroom(shape):
    """the twin sits in bf16x3's band and the float32 product in fp32's on `randn`, `offset`, `outlier` and `wide`; `cancel` is the family
    whose bound has to come from the comparator; R >= 1 is what the suite's norm-wise tolerances leave above either"""
    out = {}
    for prec, lo, hi in (("fp32", 2e-8, 1.5e-6), ("bf16x3", 1.5e-6, 1.5e-5)):
        R, w = gc.headroom(prec, shape)
        fam = {f: float(gc.comparator_errors(prec, f, shape).max()) for f in gc.FAMILIES}
        out[prec] = dict(R=R, **fam)
        assert R >= 1.0 and lo < w < hi, (prec, w)
        for f in BENIGN:
            assert lo < fam[f] < 2 * hi, (prec, f, fam[f])
        if shape[2] >= 64:
            assert fam["cancel"] > 20 * w, (prec, fam["cancel"], w)
        for f in gc.FAMILIES:
            assert gc.bound(prec, f, shape) >= gc.tolerances(False)[prec]
            assert gc.bound(prec, f, shape) == max(gc.tolerances(False)[prec], 2 * R * fam[f])
    _report(kind="comparators", shape=gc.shape_id(shape), **out)


@pytest.mark.parametrize("shape", gc.HOST_SHAPES + gc.SHAPES[1:4], ids=gc.shape_id)
def test_no_family_needs_more_than_the_bound_on_the_comparator_alone(shape):
    """the comparator in ANOTHER summation order -- one product per K-tile, added in K order in a float32 accumulator, as an MFMA kernel
    walks K -- stays inside the bound of every family and epilogue: the factor 2 R is enough for what the comparator does not share
    with a kernel, and a family that needed more would have to change"""
    for epi in (gc.PLAIN, (2, 0.7, 37, True)):
        for f in gc.FAMILIES:
            op = gc.operands(f, shape, epi)
            kw = gc._epi_kwargs(op)
            ref = gc.reference(f, shape, epi)
            for prec, alt in (("fp32", gc.ref32_tiles), ("bf16x3", gc.twin_tiles)):
                e = gc.block_err(alt(op["A"], op["B"], **kw), ref)
                assert gc.within(e, gc.bound(prec, f, shape, epi)), (f, prec, epi, gc.worst(e), gc.bound(prec, f, shape, epi))


# mutant -> (epilogue, the families it is run on; the first is the one it has to be caught on)
GEMM_MUTANTS = {"drop_lo_hi": (gc.PLAIN, ("randn", "cancel", "outlier", "tails")), "ring_shift": (gc.PLAIN, ("randn", "offset", "outlier")),
                "gate_late": ((0, 0.7, 37, True), ("randn", "tails")), "bias_prev": (gc.PLAIN, ("tails", "randn", "offset"))}


@pytest.mark.parametrize("name", list(GEMM_MUTANTS))
@pytest.mark.parametrize("shape", [(300, 296, 416), (513, 1160, 1152)], ids=gc.shape_id)
def test_gemm_mutants_are_caught_block_by_block(name, shape):
    """the float64 twin with one operation swapped: the block check has to catch each on the first family of its list; what the
    suite's norm-wise assertion (gpu_util.rel < TOL) says about the same result is recorded beside it"""
    epi, fams = GEMM_MUTANTS[name]
    tol = gc.tolerances(gc.is_epilogue(epi))["bf16x3"]
    for i, f in enumerate(fams):
        got, (rs, cs) = gc.mutant_gemm(name, gc.operands(f, shape, epi))
        ref = gc.reference(f, shape, epi)
        e = gc.block_err(got, ref)
        bnd = gc.bound("bf16x3", f, shape, epi)
        w, loc = gc.worst(e)
        _report(kind="mutant", mutant=name, shape=gc.shape_id(shape), family=f, worst=w, bound=bnd, caught=bool(w > bnd),
                rel=gc.rel(got, ref), old_check_fails=bool(gc.rel(got, ref) >= tol))
        if i == 0:
            assert w > bnd, (name, f, w, bnd)
            assert rs.start // gc.BLOCK <= loc[0] <= (rs.stop - 1) // gc.BLOCK and cs.start // gc.BLOCK <= loc[1] <= (cs.stop - 1) // gc.BLOCK
        outside = e.copy()                                           # and only where the defect is: every other block stays the twin's
        outside[rs.start // gc.BLOCK:(rs.stop - 1) // gc.BLOCK + 1, cs.start // gc.BLOCK:(cs.stop - 1) // gc.BLOCK + 1] = 0
        assert gc.within(outside, bnd)


@pytest.mark.parametrize("D", [516, 1152, 1284, 2048])
def test_layernorm_mutants_are_caught_row_by_row(D):
    """variance as E[x^2] - mean^2 in float32: invisible on `randn` (any check passes it), caught once the mean is 1e3 standard deviations
    out; statistics without the last chunk of four columns: caught on `randn` and on `outlier`"""
    tol = gc.ln_tolerance()
    for mut, fams in (("var32", ("offset", "randn")), ("short", ("randn", "outlier", "ramp"))):
        for i, f in enumerate(fams):
            c = gc.ln_case(f, D, "mod")
            ref = gc.ln_ref(c)
            with np.errstate(invalid="ignore"):
                got = gc.ln_ref(c, mutant=mut)
            w, bnd = float(gc.row_err(got, ref).max()), gc.ln_bound(f, D, "mod")
            _report(kind="ln_mutant", mutant=mut, D=D, family=f, worst=w, bound=bnd, caught=bool(w > bnd), rel=gc.rel(got, ref),
                    old_check_fails=bool(not gc.rel(got, ref) < tol))
            if i == 0:
                assert w > bnd, (mut, f, w, bnd)
    c = gc.ln_case("randn", D, "mod")
    assert gc.row_err(gc.ln_ref(c, mutant="var32"), gc.ln_ref(c)).max() < tol          # the benign input hides it


@pytest.mark.parametrize("D", gc.LN_DIMS)
def test_layernorm_comparator_headroom_and_the_const_rows(D):
    out = {}
    for form in gc.LN_FORMS:
        R, w = gc.ln_headroom(D, form)
        out[form] = dict(R=R, **{f: float(gc.ln_comparator_errors(f, D, form).max()) for f in gc.LN_FAMILIES})
        assert R >= 1.0 and w < gc.ln_tolerance()
        # `const`: variance exactly 0, the normalised row exactly 0 -- on the float64 oracle the output IS the shift / the affine bias
        c = gc.ln_case("const", D, form)
        assert (c["x"] == c["x"][:, :1]).all() and len(np.unique(c["x"][:, 0])) == 25
        want = gc.ln_const_expectation(c)
        if want is not None:
            assert np.array_equal(gc.ln_ref(c), want.astype(np.float64))
            assert np.array_equal(gc.ln_ref(c, dtype=np.float32), want)
        else:
            s = np.arange(c["x"].shape[0]) // c["rps"]
            assert np.array_equal(gc.ln_ref(c), c["b"].astype(np.float64) * (1 + c["mod"][s, 2 * D:3 * D].astype(np.float64)) + c["mod"][s, D:2 * D])
    _report(kind="ln", D=D, **out)
    x = gc.ln_rows("offset", 64, D, 1)
    assert abs(x.mean() - 1e3) < 1 and 0.8 < x.std(-1).mean() < 1.2 or D < 16
    x = gc.ln_rows("ramp", 48, D, 1)
    assert np.allclose(np.log2(np.abs(x[1]).mean() / np.abs(x[0]).mean()), 1, atol=1.5 if D < 64 else 0.3)
    _, _, mod = gc.ln_params(D, 1)
    assert set(np.unique(np.abs(mod[:, D:2 * D]))) == {20.0} and (mod[:, 2 * D:3 * D] > -1).all() and mod[:, 2 * D:3 * D].max() < np.e ** 2
