"""-m gpu: the two epilogues of the 128 x 144 pre-split GEMM tile (csrc/gemm144.hip, tile 81; rgm_set_gemm144_epilogue): 0 straight from
the accumulators, 1 the tile staged in the idle operand ring and moved as whole 576-byte rows by all eight waves.

Mode 1 must give the BITS of mode 0 (torch.equal on the whole output buffer, pad columns and their sentinel included) on the smallest
shapes at which it can go wrong: one row, a partial and a just-over-one row tile, two column tiles (the second starts in the middle of a
128-byte line), several row and column tiles; rows_per_gate that cuts through a wave's 16 rows (33, 37), one that spans them (129) and
short ones (5: the per-chunk gate row without a division); ldc = ldres = N + 32; K slices.  Against the float64 twin of the three-term
split every 16 x 16 block is held as tests/test_gpu_gemm_inputs.py holds tile 81: gemm_cases.bound, a figure of the comparator alone.

Split-row output needs N % 32 == 0 (gemm2_launch refuses it otherwise), which of the shapes only N = 288 meets: the split format runs on
(128, 288, 64) and on (129, 288, 64), added for a partial row tile in that format."""
import ctypes as C

import pytest
import torch

import gemm_cases as gc
from test_gpu_gemm_inputs import Case

pytestmark = pytest.mark.gpu
TILE = 81
SHAPES = [(1, 144, 64), (127, 144, 64), (129, 144, 96), (128, 288, 64), (129, 288, 64), (272, 432, 128)]
SENTINEL = 7.0
# (name, epilogue without the activation: alpha, rows_per_gate or 0, residual; bias on)
EPILOGUES = [("plain", (1.0, 0, False), False), ("bias", (1.0, 0, False), True),
             ("gated33", (0.7, 33, True), True), ("gated37", (0.7, 37, True), True), ("gated129", (0.7, 129, True), True),
             ("gated5", (0.7, 5, True), True)]


@pytest.fixture(scope="module", autouse=True)
def _mode():
    """every test leaves the library in the mode it found"""
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    from rgm import native as R
    prev = C.c_int(-1)
    R.check(R.lib.rgm_set_gemm144_epilogue(0, C.byref(prev)))
    R.check(R.lib.rgm_set_gemm144_epilogue(prev.value, None))
    yield
    R.check(R.lib.rgm_set_gemm144_epilogue(prev.value, None))


def _set(mode):
    from rgm import native as R
    R.check(R.lib.rgm_set_gemm144_epilogue(mode, None))


def _case(shape, act, epi, bias, fam="tails"):
    alpha, rpg, res = epi
    op = gc.operands(fam, shape, (act, alpha, rpg, res))
    return Case(op if bias else dict(op, bias=None))


def _both(case, **kw):
    """the whole output buffer in mode 0 and in mode 1"""
    out = []
    for mode in (0, 1):
        _set(mode)
        out.append(case.run("bf16x3_presplit", TILE, raw=True, fill=SENTINEL, **kw))
    return out


@pytest.mark.parametrize("name,epi,bias", EPILOGUES, ids=[e[0] for e in EPILOGUES])
@pytest.mark.parametrize("shape", SHAPES, ids=gc.shape_id)
def test_whole_row_epilogue_gives_the_bits_of_the_accumulator_epilogue(shape, name, epi, bias):
    """every activation, fp32 rows (residual in place: res == C) and split rows (N % 32 == 0), tight and with ldc = ldres = N + 32: the
    same bits, the sentinel untouched in the pad columns"""
    M, N, K = shape
    bad = []
    for act in (0, 1, 2):
        case = _case(shape, act, epi, bias)
        for out_split in ((0, 1) if N % 32 == 0 else (0,)):
            for ldc in (N, N + 32):
                old, new = _both(case, out_split=out_split, ldc=ldc)
                pad_ok = bool((new[:, N:] == SENTINEL).all()) and bool((old[:, N:] == SENTINEL).all())
                # a split row holds N / 2 floats of bf16 pairs per half: finite as raw bits is not meaningful, compare bits only
                fin = True if out_split else bool(torch.isfinite(new[:, :N]).all())
                if not (torch.equal(old, new) and pad_ok and fin):
                    bad.append((act, out_split, ldc, int((old != new).sum()), pad_ok, fin))
    assert not bad, bad


def test_k_slices_give_the_same_bits_in_both_modes():
    """(256, 144, 256) through rgm_gemm_split_epi with a workspace, tile 81 and the heuristic's choice; and the shape at which the heuristic
    does cut K on these tiles (24 tiles x 8 slices of 18 K-tiles: blockIdx.z > 0, partial sums at stride sC in the workspace, then the
    reduce kernel), gated and in place"""
    from rgm import native as R
    bad = []
    for shape, tile in (((256, 144, 256), TILE), ((256, 144, 256), 0), ((256, 1728, 4608), 0)):
        M, N, K = shape
        ws = torch.empty(int(R.lib.rgm_gemm_scratch_bytes(M, N)), dtype=torch.uint8, device="cuda")
        case = Case(gc.operands("randn", shape, (0, 0.7, 37, True)))
        outs = []
        for mode in (0, 1):
            _set(mode)
            ws.fill_(0xAB)
            outs.append(case.run("bf16x3_presplit", tile, raw=True, ws=ws))
        if not (torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[1]).all())):
            bad.append((shape, tile, int((outs[0] != outs[1]).sum())))
    assert not bad, bad


@pytest.mark.parametrize("shape", SHAPES, ids=gc.shape_id)
def test_every_block_of_the_whole_row_epilogue_is_inside_the_comparator_bound(shape):
    """mode 1, gated epilogue (alpha 0.7, rows_per_gate 37, residual in place): every 16 x 16 block within gemm_cases.bound -- max(TOL,
    2 R x the float64 twin's worst block on this case), the measure and margin test_gpu_gemm_inputs.py holds tile 81 to"""
    epi = (0, 0.7, 37, True)
    fam = "randn"
    case = Case(gc.operands(fam, shape, epi))
    ref = gc.reference(fam, shape, epi)
    bnd = gc.bound("bf16x3_presplit", fam, shape, epi)
    _set(1)
    e = gc.block_err(case.run("bf16x3_presplit", TILE), ref)
    w, loc = gc.worst(e)
    print(f"RGM_G144_EPI_REPORT shape={gc.shape_id(shape)} kernel={w:.3e} at block {loc} "
          f"comparator={float(gc.comparator_errors('bf16x3_presplit', fam, shape, epi).max()):.3e} bound={bnd:.3e}")
    assert gc.within(e, bnd), (w, loc, bnd)


def test_setter_returns_the_previous_mode_and_refuses_other_modes():
    from rgm import native as R
    prev = C.c_int(-1)
    R.check(R.lib.rgm_set_gemm144_epilogue(1, None))
    R.check(R.lib.rgm_set_gemm144_epilogue(0, C.byref(prev)))
    assert prev.value == 1
    R.check(R.lib.rgm_set_gemm144_epilogue(1, C.byref(prev)))
    assert prev.value == 0
    for mode in (-1, 2, 7):
        prev = C.c_int(-5)
        assert R.lib.rgm_set_gemm144_epilogue(mode, C.byref(prev)) != 0
        assert prev.value == -5                                        # nothing reported ...
        R.check(R.lib.rgm_set_gemm144_epilogue(1, C.byref(prev)))
        assert prev.value == 1                                         # ... and nothing changed


def test_twenty_launches_on_fresh_copies_of_one_input_agree():
    """(272, 432, 128), gated, in place, mode 1: a race on the staged image -- a wave reading rows another has not written yet, a piece of
    the last K-tile landing in it -- shows as a difference between runs"""
    case = Case(gc.operands("randn", (272, 432, 128), (2, 0.7, 37, True)))
    _set(1)
    first = case.run("bf16x3_presplit", TILE, raw=True)
    assert bool(torch.isfinite(first).all())
    diff = [i for i in range(1, 20) if not torch.equal(case.run("bf16x3_presplit", TILE, raw=True), first)]
    assert not diff, diff
