"""-m gpu: the dense GEMM kernels (csrc/gemm.hip, gemm2.hip + gemm2_body.h, gemm144.hip) and the LayerNorm row bodies (csrc/ln_body.h)
block by block on offset, outlier, wide-range, cancelling, one-K-tile and tail inputs (tests/gemm_cases.py, docs/rounds/gemm_inputs.md).

Every 16 x 16 block of every result is held to max(TOL, 2 R x the comparator's worst block on that family, shape and epilogue): the
float32 product for the fp32 kernels, the float64 twin of the three-term split for both bf16x3 modes -- never a figure of a kernel.  The
exact checks (isolation, padding, power-of-two scaling, row permutation, one K-tile) have no tolerance.  One RGM_GEMM_REPORT line per case
(tools/gemm_inputs_table.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gemm_cases as gc

pytestmark = pytest.mark.gpu
F32 = np.float32

# tile -> (rows, columns) of its output tile: every id gemm2_launch dispatches, but 48 / 49 (whole rounds of 512 tiles only); 0 = heuristic
PRESPLIT_TILES = {0: (128, 64), 1: (128, 128), 2: (128, 64), 3: (64, 64), 5: (256, 128), 21: (128, 128), 22: (128, 64), 43: (128, 128),
                  44: (128, 64), 45: (256, 128), 46: (64, 64), 51: (128, 128), 52: (128, 64), 53: (128, 64), 54: (128, 128), 55: (128, 128),
                  56: (128, 64), 57: (64, 64), 58: (64, 64), 71: (256, 256), 72: (512, 128), 73: (128, 256), 74: (256, 288), 81: (128, 144)}
OPERAND_TILES = {0: (128, 64), 1: (128, 128), 2: (128, 64), 3: (64, 64), 4: (32, 128)}       # rgm_gemm_tile, fp32 and bf16x3
GATE_PERIODS = (32, 33, 37, 129, 257)
# tiles whose rows are NOT bit-identical under a permutation of the rows of A on the parent commit (none: measured on one MI355X)
PERMUTATION_VARIANT_TILES = set()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    from rgm import native as R
    R.set_gemm_precision("fp32")
    yield
    R.set_gemm_precision("fp32")


def _report(**kw):
    line = json.dumps(kw)
    print("RGM_GEMM_REPORT " + line)
    path = os.environ.get("RGM_GEMM_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _kernels(shape, gated=False, tiles=None):
    """[(precision, tile)] that take the shape: 81 needs N % 144 == 0 and K >= 64, 74 N % 8 == 0 and the plain epilogue"""
    M, N, K = shape
    out = []
    for t in (PRESPLIT_TILES if tiles is None else tiles):
        if t == 81 and (N % 144 or K < 64):
            continue
        if t == 74 and (N % 8 or gated):
            continue
        out.append(("bf16x3_presplit", t))
    return out


# ------------------------------------------------------------------------------------------------ launches
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _padded(x, ld, fill):
    """(rows, K) float32 -> device (rows, ld) with the pad columns at `fill`"""
    if ld == x.shape[1]:
        return _dev(x)
    out = torch.full((x.shape[0], ld), fill, device="cuda")
    out[:, :x.shape[1]] = _dev(x)
    return out


def _split(x, ld=None, fill=float("nan")):
    """(rows, K) float32 -> the split-row image on the device, rows of `ld` elements, pad columns at `fill`"""
    from rgm import native as R
    rows, K = x.shape
    ld = ld or K
    out = torch.full((rows, ld), fill, device="cuda")
    xd = _dev(x)
    R.check(R.lib.rgm_split_rows_ld(R.ptr(xd), K, R.ptr(out), ld, rows, K, R.current_stream()))
    torch.cuda.synchronize()
    return out


def _unsplit(t, N):
    """split-row device tensor (rows, ldc) -> float64 hi + lo of its first N columns: lines of [32 hi | 32 lo] (csrc/common.h)"""
    from gpu_util import split_torch_dtype
    rows, ld = t.shape
    raw = t.contiguous().view(split_torch_dtype()).view(rows, ld // 32, 2, 32).double().cpu().numpy()
    return (raw[:, :, 0, :] + raw[:, :, 1, :]).reshape(rows, ld)[:, :N]


class Case:
    """the operands of one case on the device, plain and split, launched through any kernel"""

    def __init__(self, op, lda=None, ldb=None, gate_pad=64):
        self.op = op
        self.A, self.B = op["A"], op["B"]
        self.M, self.K = self.A.shape
        self.N = self.B.shape[0]
        self.lda, self.ldb = lda or self.K, ldb or self.K
        self.bias = _dev(op["bias"]) if op["bias"] is not None else None
        self.gate_ld = self.N + gate_pad                              # gate rows strided like the modulation buffer's
        self.gate = _padded(op["gate"], self.gate_ld, 3.0) if op["gate"] is not None else None
        self._plain = self._splits = None

    def plain(self):
        if self._plain is None:
            nan = float("nan")
            self._plain = (_padded(self.A, self.lda, nan), _padded(self.B, self.ldb, nan))
        return self._plain

    def splits(self):
        if self._splits is None:
            self._splits = (_split(self.A, self.lda), _split(self.B, self.ldb))
        return self._splits

    def out(self, ldc, fill, in_place):
        c = torch.full((self.M, ldc), fill, device="cuda")
        if in_place:
            c[:, :self.N] = _dev(self.op["res"])                      # the residual is read from and written to C
        return c

    def run(self, precision, tile, out_split=0, ldc=None, fill=float("nan"), ws=None, raw=False):
        """-> the result's first N columns as numpy (float64 from a split-row output), or the whole device tensor with raw=True"""
        from rgm import native as R
        op, M, N, K = self.op, self.M, self.N, self.K
        ldc = ldc or N
        # fp32 output: the residual is C itself (res == C, the proj / fc2 epilogue); split-row output: a buffer of its own (a split line
        # does not keep its values where the fp32 line had them)
        in_place = op["res"] is not None and not out_split
        c = self.out(ldc, fill, in_place)
        res = None if op["res"] is None else (c if in_place else _dev(op["res"]))
        ldres = ldc if in_place else N
        st = R.current_stream()
        gated = op["gate"] is not None or op["res"] is not None or op["alpha"] != 1.0
        if precision == "bf16x3_presplit":
            As, Bs = self.splits()
            R.check(R.lib.rgm_gemm_split_epi(R.ptr(As), self.lda, R.ptr(Bs), self.ldb, R.ptr(c), ldc, M, N, K, R.ptr(self.bias), op["act"],
                                             op["alpha"], R.ptr(self.gate), self.gate_ld if self.gate is not None else 0, op["rpg"],
                                             R.ptr(res), ldres, tile, out_split,
                                             R.ptr(ws) if ws is not None else None, ws.numel() if ws is not None else 0, st))
        else:
            Ad, Bd = self.plain()
            assert not out_split
            if gated:                                                 # the full epilogue has no explicit-tile entry: the heuristic's kernel
                assert tile == 0
                R.set_gemm_precision(precision)
                try:
                    R.check(R.lib.rgm_gemm(R.ptr(Ad), self.lda, R.ptr(Bd), self.ldb, R.ptr(c), ldc, M, N, K, R.ptr(self.bias), op["act"], op["alpha"],
                                           R.ptr(self.gate), self.gate_ld if self.gate is not None else 0, op["rpg"],
                                           R.ptr(res), ldres, st))
                finally:
                    R.set_gemm_precision("fp32")
            else:
                R.check(R.lib.rgm_gemm_tile(R.ptr(Ad), self.lda, R.ptr(Bd), self.ldb, R.ptr(c), ldc, M, N, K, R.ptr(self.bias), op["act"],
                                            tile | ((R.PRECISIONS[precision] + 1) << 4), st))
        torch.cuda.synchronize()
        if raw:
            return c
        return _unsplit(c, N) if out_split else c[:, :N].cpu().numpy()


def _all_kernels(shape, gated=False):
    """the operand-staging kernels (fp32, bf16x3: every explicit tile for the plain epilogue, the heuristic's for the full one) + the pre-split tiles"""
    ops = [(p, t) for p in ("fp32", "bf16x3") for t in ((0,) if gated else OPERAND_TILES)]
    return ops + _kernels(shape, gated)


def _check_blocks(case, fam, shape, epi, kernels, split_too=True):
    """every block of every kernel's result inside the bound of the case; one report line per kernel -> the list of failures"""
    ref = gc.reference(fam, shape, epi)
    bad = []
    for prec, tile in kernels:
        bnd = gc.bound(prec, fam, shape, epi)
        R_, _ = gc.headroom(prec, shape, epi)
        cmp_worst = float(gc.comparator_errors(prec, fam, shape, epi).max())
        for out_split in ((0, 1) if split_too and prec == "bf16x3_presplit" and shape[1] % 32 == 0 else (0,)):
            e = gc.block_err(case.run(prec, tile, out_split), ref)
            w, loc = gc.worst(e)
            bm, bn = (PRESPLIT_TILES if prec == "bf16x3_presplit" else OPERAND_TILES)[tile]
            _report(family=fam, shape=gc.shape_id(shape), epilogue=list(epi), precision=prec, tile=tile, out_split=out_split, kernel=w,
                    row_tile=loc[0] * gc.BLOCK // bm, col_tile=loc[1] * gc.BLOCK // bn, comparator=cmp_worst, bound=bnd, R=R_)
            if not gc.within(e, bnd):
                bad.append((prec, tile, out_split, w, loc, bnd))
    return bad


# ------------------------------------------------------------------------------------------------ the block bound
@pytest.mark.parametrize("fam", gc.FAMILIES)
@pytest.mark.parametrize("shape", gc.SHAPES + gc.SHAPES_144, ids=gc.shape_id)
def test_every_block_of_every_kernel_is_inside_the_comparator_bound(shape, fam):
    """plain output (bias, no activation) of every kernel, and the split-row output of the pre-split kernels where N % 32 == 0"""
    case = Case(gc.operands(fam, shape))
    kernels = _all_kernels(shape) if shape in gc.SHAPES else [("fp32", 0), ("bf16x3", 0)] + _kernels(shape, tiles=(0, 81))
    bad = _check_blocks(case, fam, shape, gc.PLAIN, kernels)
    assert not bad, bad


@pytest.mark.parametrize("rpg", GATE_PERIODS)
@pytest.mark.parametrize("act", [0, 1, 2])
def test_epilogues_under_tails_with_gate_periods_that_cut_through_slabs_and_tiles(act, rpg):
    """bias from {-30 .. 30} (SiLU / GELU at both tails: silu_f, gelu_tanh_f, gelu_tanh_fast_f), alpha 0.7, a per-sample gate whose switch
    lands inside 32-row slabs and inside the partial row tile, residual read from and written to C: the 128-row kernels, tile 81, the
    big tiles 71 - 73 and the operand-staging kernels; fp32 and split-row output; and the activation alone through tile 74"""
    shape = (300, 288, 416)
    epi = (act, 0.7, rpg, True)
    bad = _check_blocks(Case(gc.operands("tails", shape, epi)), "tails", shape, epi, _all_kernels(shape, gated=True))
    if rpg == GATE_PERIODS[0]:
        epi = (act, 1.0, 0, False)
        bad += _check_blocks(Case(gc.operands("tails", shape, epi)), "tails", shape, epi, _all_kernels(shape))
    assert not bad, bad


@pytest.mark.parametrize("fam", ["outlier", "cancel"])
def test_split_k_route_block_by_block_and_bit_identical_on_dirty_scratch(fam):
    """rgm_gemm_split_epi with a workspace, tile 0, at the smallest shape splitk_factor slices (72 K-tiles, 10 tiles of 128 x 64): the launch
    records show the K slices as ONE batched 128 x 64 launch (id 84) and no unsliced launch; plain and gated epilogue through the reduce
    kernel; the same bits from scratch pre-filled with 0xAB twice"""
    import test_gpu_fullsize as full
    from rgm import native as R
    shape = gc.SPLITK_SHAPE
    M, N, K = shape
    need = int(R.lib.rgm_gemm_scratch_bytes(M, N))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    bad = []
    for epi in (gc.PLAIN, (0, 0.7, 37, True), (2, 1.0, 0, False)):
        case = Case(gc.operands(fam, shape, epi))
        ref = gc.reference(fam, shape, epi)
        bnd = gc.bound("bf16x3_presplit", fam, shape, epi)
        outs = []
        for rep in range(2):
            ws.fill_(0xAB)
            R.check(R.lib.rgm_prof_reset())
            R.check(R.lib.rgm_prof_enable(1))
            try:
                outs.append(case.run("bf16x3_presplit", 0, ws=ws))
            finally:
                R.check(R.lib.rgm_prof_enable(0))
            n = full._launches([84, 97, 96, 135])
            R.check(R.lib.rgm_prof_reset())
            assert n[84] == 1 and n[97] == 0 and n[96] == 0 and n[135] == 0, n
        assert np.array_equal(outs[0], outs[1])
        e = gc.block_err(outs[0], ref)
        w, loc = gc.worst(e)
        _report(family=fam, shape=gc.shape_id(shape), epilogue=list(epi), precision="bf16x3_presplit", tile="splitk", out_split=0, kernel=w,
                row_tile=loc[0] * gc.BLOCK // 128, col_tile=loc[1] * gc.BLOCK // 64,
                comparator=float(gc.comparator_errors("bf16x3", fam, shape, epi).max()), bound=bnd, R=gc.headroom("bf16x3", shape, epi)[0])
        if not gc.within(e, bnd):
            bad.append((epi, w, loc, bnd))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ exact checks
def _poison_rows(M, bm):
    """the last row of a full tile, the first row of the partial tile, row M - 1"""
    rows = {M - 1}
    if M >= bm:
        rows.add(bm - 1)
    if M % bm and M > bm:
        rows.add(M - M % bm)
    return sorted(rows)


@pytest.mark.parametrize("variant", ["plain", "split", "gated", "gated-split"])
def test_a_nan_row_of_an_operand_stays_in_its_own_row_or_column(variant):
    """rows of A all NaN -> exactly those rows of C are NaN; rows of B all NaN -> exactly those columns; every other entry has the bits of
    the run in which the poisoned rows are zero.  Every tile, each with the rows its own tile height and width make the edges."""
    gated, out_split = variant.startswith("gated"), int(variant.endswith("split"))
    epi = (0, 0.7, 37, True) if gated else gc.PLAIN
    bad = []
    for shape in ((552, 608, 64), (300, 576, 64)):
        M, N, K = shape
        kernels = _kernels(shape, gated, None if shape[1] == 608 else (81,))
        if not out_split and shape[1] == 608:
            kernels = [(p, t) for p in ("fp32", "bf16x3") for t in ((0,) if gated else OPERAND_TILES)] + kernels
        op = gc.operands("randn", shape, epi)
        cache = {}
        for prec, tile in kernels:
            bm, bn = (PRESPLIT_TILES if prec == "bf16x3_presplit" else OPERAND_TILES)[tile]
            rows, cols = _poison_rows(M, bm), _poison_rows(N, bn)
            key = (tuple(rows), tuple(cols))
            if key not in cache:
                ops = []
                for v in (0.0, np.nan):
                    A, B = op["A"].copy(), op["B"].copy()
                    A[rows], B[cols] = v, v
                    ops.append(Case(dict(op, A=A, B=B)))
                cache[key] = ops
            zero, nan = (c.run(prec, tile, out_split) for c in cache[key])
            hit = np.zeros((M, N), bool)
            hit[rows], hit[:, cols] = True, True
            if not (np.isnan(nan[hit]).all() and np.array_equal(nan[~hit], zero[~hit]) and np.isfinite(zero).all()):
                bad.append((shape, prec, tile, int(np.isnan(nan[~hit]).sum()), int((nan[~hit] != zero[~hit]).sum())))
    assert not bad, bad


def test_nan_padding_of_the_operands_is_never_read_and_the_output_padding_never_written():
    """lda, ldb > K with NaN in the pad columns, ldc > N pre-filled with 7.0: finite, the bits of the tightly packed run, padding still 7.0
    -- every tile (74 and 81 included), plain and split-row output, and the operand-staging kernels"""
    bad = []
    for shape in ((333, 160, 192), (300, 576, 96)):
        M, N, K = shape
        lda, ldb, ldc = K + 32, K + 64, N + 32
        op = gc.operands("randn", shape)
        tight, padded = Case(op), Case(op, lda=lda, ldb=ldb)
        kernels = _kernels(shape, tiles=None if N == 160 else (0, 81))
        if N == 160:
            kernels = [(p, t) for p in ("fp32", "bf16x3") for t in OPERAND_TILES] + kernels
        for prec, tile in kernels:
            for out_split in ((0, 1) if prec == "bf16x3_presplit" else (0,)):
                want = tight.run(prec, tile, out_split)
                c = padded.run(prec, tile, out_split, ldc=ldc, fill=7.0, raw=True)
                got = _unsplit(c, N) if out_split else c[:, :N].cpu().numpy()
                ok = np.isfinite(got).all() and np.array_equal(got, want) and bool((c[:, N:] == 7.0).all())
                if not ok:
                    bad.append((shape, prec, tile, out_split))
    assert not bad, bad


@pytest.mark.parametrize("ea,eb", [(-40, -20), (40, 20)])
def test_power_of_two_scaling_of_the_operands_scales_the_result_bit_for_bit(ea, eb):
    """no activation, no bias: A 2^ea, B 2^eb -> C 2^(ea + eb) exactly -- no absolute epsilon, no lo half flushed; fp32, bf16x3, every pre-split tile"""
    bad = []
    for shape in ((300, 288, 416), (300, 432, 416)):
        op = dict(gc.operands("randn", shape), bias=None)
        base = Case(op)
        scaled = Case(dict(op, A=op["A"] * F32(2.0 ** ea), B=op["B"] * F32(2.0 ** eb)))
        kernels = _all_kernels(shape) if shape[1] == 288 else _kernels(shape, tiles=(81,))
        for prec, tile in kernels:
            want = base.run(prec, tile).astype(np.float64) * 2.0 ** (ea + eb)
            got = scaled.run(prec, tile).astype(np.float64)
            if not (np.isfinite(got).all() and np.array_equal(got, want)):
                bad.append((shape, prec, tile, int((got != want).sum())))
    assert not bad, bad


def test_permuting_the_rows_of_a_permutes_the_rows_of_c_bit_for_bit():
    """within one kernel a row's result does not depend on where in the tile it sits (the MFMA accumulation order is that of K alone)"""
    variant = set()
    for shape in ((552, 608, 224), (300, 432, 96)):
        op = gc.operands("wide", shape)
        perm = np.random.RandomState(4).permutation(shape[0])
        base, moved = Case(op), Case(dict(op, A=op["A"][perm]))
        for prec, tile in (_all_kernels(shape) if shape[1] == 608 else _kernels(shape, tiles=(81,))):
            if not np.array_equal(base.run(prec, tile)[perm], moved.run(prec, tile)):
                variant.add((prec, tile))
    assert {t for _, t in variant} == PERMUTATION_VARIANT_TILES, sorted(variant)


@pytest.mark.parametrize("fam", gc.KT_FAMILIES)
def test_one_nonzero_k_tile_gives_the_bits_of_that_tile_alone(fam):
    """K = 416 with only K-tile j non-zero against the same kernel on that tile alone (K = 32; 64 with a zero tile behind it for tile 81,
    which takes K >= 64): a K-tile skipped, doubled or read from the wrong ring stage cannot agree"""
    bad = []
    for shape in ((300, 288, 416), (300, 432, 416)):
        M, N, K = shape
        op = gc.operands(fam, shape)
        j = gc.ktile_index(fam, K)
        s = slice(j * gc.KTILE, (j + 1) * gc.KTILE)
        z = np.zeros((1, gc.KTILE), F32)
        long_, one = Case(op), Case(dict(op, A=op["A"][:, s].copy(), B=op["B"][:, s].copy()))
        two = Case(dict(op, A=np.hstack((op["A"][:, s], z.repeat(M, 0))), B=np.hstack((op["B"][:, s], z.repeat(N, 0)))))
        for prec, tile in (_all_kernels(shape) if N == 288 else _kernels(shape, tiles=(81,))):
            got, want = long_.run(prec, tile), (two if tile == 81 else one).run(prec, tile)
            if not (np.array_equal(got, want) and np.abs(want).max() > 0.1):
                bad.append((shape, prec, tile, int((got != want).sum())))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ LayerNorm
def _layernorm(c, rows=None):
    """rgm_layernorm_modulate on the first `rows` rows of a case (views into a strided modulation buffer, like the DiT's) -> numpy"""
    from rgm import native as R
    D = c["D"]
    x = c["x"] if rows is None else c["x"][:rows]
    xd, od = _dev(x), torch.full((x.shape[0], D), float("nan"), device="cuda")
    wd, bd = (None, None) if c["w"] is None else (_dev(c["w"]), _dev(c["b"]))
    md = None if c["mod"] is None else _dev(c["mod"])
    R.check(R.lib.rgm_layernorm_modulate(R.ptr(xd), R.ptr(od), x.shape[0], D, gc.LN_EPS, R.ptr(wd), R.ptr(bd),
                                         md.data_ptr() + 4 * D if md is not None else None, md.data_ptr() + 8 * D if md is not None else None,
                                         6 * D, c["rps"], R.current_stream()))
    torch.cuda.synchronize()
    return od.cpu().numpy()


@pytest.mark.parametrize("form", gc.LN_FORMS)
@pytest.mark.parametrize("D", gc.LN_DIMS)
def test_layernorm_rows_inside_the_comparator_bound_and_const_rows_exact(D, form):
    """all three MAXV instantiations of ln_mod_kernel, both sides of each switch (D = 512 / 516, 1280 / 1284), a partial last chunk in each;
    3 samples of 37 rows, and M = 1 / 5 (a partial workgroup of 4 waves).  A `const` row gives the shift / the affine bias exactly."""
    bad = []
    for fam in gc.LN_FAMILIES:
        c = gc.ln_case(fam, D, form)
        ref = gc.ln_ref(c)
        bnd = gc.ln_bound(fam, D, form)
        got = _layernorm(c)
        e = gc.row_err(got, ref)
        _report(family=fam, shape=f"ln{D}", epilogue=[form], precision="fp32", tile="ln", out_split=0, kernel=float(e.max()),
                row_tile=int(e.argmax()), col_tile=0, comparator=float(gc.ln_comparator_errors(fam, D, form).max()), bound=bnd,
                R=gc.ln_headroom(D, form)[0])
        if not gc.within(e, bnd):
            bad.append((fam, float(e.max()), bnd))
        for rows in (1, 5):
            if not np.array_equal(_layernorm(c, rows), got[:rows]):
                bad.append((fam, "rows", rows))
        want = gc.ln_const_expectation(c) if fam == "const" else None
        if want is not None and not np.array_equal(got, want):
            bad.append((fam, "exact", int((got != want).sum())))
    assert not bad, bad


def _layernorm_all():
    """every modulated case (the only form RGM_LN_PRELOAD touches) -> {name: result}"""
    return {f"{fam}.{D}": _layernorm(gc.ln_case(fam, D, "mod")) for D in gc.LN_DIMS for fam in gc.LN_FAMILIES}


_LN_CHILD = """
import sys
sys.path[:0] = {paths!r}
import numpy as np
import test_gpu_gemm_inputs as t
np.savez(sys.argv[1], **t._layernorm_all())
"""


def test_layernorm_preload_of_the_modulation_row_changes_no_bit(tmp_path):
    """RGM_LN_PRELOAD (read once per process): 1, the default -- the sample's shift / scale requested with the row -- in this process, 0 in
    a fresh child; identical bits for every D and family"""
    assert os.environ.get("RGM_LN_PRELOAD", "1") == "1"
    here = _layernorm_all()
    out = tmp_path / "ln_preload0.npz"
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    script = _LN_CHILD.format(paths=[tests, root, os.path.join(root, "rule-guided-music_amd")])
    r = subprocess.run([sys.executable, "-c", script, str(out)], env=dict(os.environ, RGM_LN_PRELOAD="0"), timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    there = np.load(out)
    assert sorted(there.files) == sorted(here)
    assert not [k for k in here if not np.array_equal(here[k], there[k])]


# ------------------------------------------------------------------------------------------------ the split-row LayerNorm, through the model
@pytest.mark.parametrize("fam", ["offset", "outlier"])
@pytest.mark.parametrize("hidden,heads,depth", [(384, 6, 1), (1152, 16, 1), (1152, 16, 2)])
def test_fused_reduce_layernorm_equals_the_separate_launch_on_offset_and_outlier_rows(hidden, heads, depth, fam):
    """the split-row output of the LayerNorm has no entry of its own: a forward in bf16x3_presplit at B = 4, T = 256 whose residual stream
    carries the family (the embedder's output bias: + 50 on every channel / 300 on two) -- at 1152 proj runs as K slices whose reduce
    writes the block's second LayerNorm, and with a second block fc2's reduce writes that block's first; identical bits with
    rgm_set_fuse_reduce_ln 0 and 1, and the counter shows the route (hidden 384 has no K-sliced GEMM: the counter must not move)"""
    from gpu_util import load_module
    from guided_diffusion.dit import DiTRotary
    from rgm import native as R, synth
    arch = dict(depth=depth, hidden=hidden, heads=heads, patch=8, in_ch=4, out_ch=4, num_classes=3)
    sd = synth.dit_state_dict(3, final_std=0.3 / hidden ** 0.5, device="cuda", **arch)
    b = sd["x_embedder.MLP.2.bias"].clone()
    if fam == "offset":
        b += 50.0
    else:
        b[np.random.RandomState(hidden).choice(hidden, 2, replace=False)] = 300.0
    sd["x_embedder.MLP.2.bias"] = b
    m = load_module(DiTRotary(input_size=[128, 16], patch_size=8, in_channels=4, hidden_size=hidden, depth=depth, num_heads=heads,
                              num_classes=3, learn_sigma=False), sd)
    rng = np.random.RandomState(hidden + depth)
    B = 4
    x = _dev(rng.randn(B, 4, 128, 16).astype(F32))
    t = _dev(rng.randint(0, 1000, size=B).astype(np.int64))
    y = _dev(rng.randint(0, 3, size=B).astype(np.int64))
    R.set_gemm_precision("bf16x3_presplit")
    try:
        R.check(R.lib.rgm_set_fuse_reduce_ln(0))
        n0 = R.lib.rgm_fused_reduce_ln_launches()
        apart = m(x, t, y).clone()
        assert R.lib.rgm_fused_reduce_ln_launches() == n0
        R.check(R.lib.rgm_set_fuse_reduce_ln(1))
        fused = m(x, t, y).clone()
        n1 = R.lib.rgm_fused_reduce_ln_launches() - n0
    finally:
        R.check(R.lib.rgm_set_fuse_reduce_ln(1))
        R.set_gemm_precision("fp32")
    assert n1 == (0 if hidden == 384 else depth + (depth - 1)), n1   # proj of every block + fc2 of every block but the last
    assert bool(torch.isfinite(fused).all())
    assert torch.equal(fused, apart), float((fused - apart).abs().max())
