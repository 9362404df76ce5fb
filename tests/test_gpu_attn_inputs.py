"""-m gpu: the attention kernels on peaked, shifted and uneven-scale inputs (tests/attn_cases.py): resident fp32 / bf16x3 / key-blocked /
per-tile forward, resident backward with its per-tile and lone-token paths, streaming forward, streaming dq / dkv -- every (sample,
component, head) block on its own against the float64 reference, under a bound derived from the existing tolerances and from CPU
references computed here (attn_cases.bound); plus checks whose expected value is known exactly (key count, underflowing rescale, silent
heads, NaN neighbours).  Nothing here provokes anything: NaN arithmetic faults nothing, the tests read and compare.

Set RGM_ATTN_REPORT to a file name to get one JSON line per (family, shape, mode, precision, quantity): the table of
docs/rounds/attn_inputs.md."""
import json
import math
import os

import numpy as np
import pytest
import torch

import attn_cases as A

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the kernels through the C ABI
def _tables(T, hd):
    from gpu_util import dev
    cos, sin = A.rotary_tables(hd, T)
    return dev(cos), dev(sin)


def _forward(qd, shape, with_lse=True):
    """qd: device tensor whose first N*T rows are the qkv rows.  -> o (N*T, D), lse (N*heads*T) device tensors, pre-filled with NaN"""
    from rgm import native as R
    N, T, heads, hd = shape
    cd, sd_ = _tables(T, hd)
    od = torch.full((N * T, heads * hd), float("nan"), device="cuda")
    ld = torch.full((N * heads * T,), float("nan"), device="cuda") if with_lse else None
    if with_lse:
        R.check(R.lib.rgm_rotary_attention_lse(R.ptr(qd), R.ptr(od), R.ptr(ld), R.ptr(cd), R.ptr(sd_), N, T, heads, hd, hd // 4, R.current_stream()))
    else:
        R.check(R.lib.rgm_rotary_attention(R.ptr(qd), R.ptr(od), R.ptr(cd), R.ptr(sd_), N, T, heads, hd, hd // 4, R.current_stream()))
    torch.cuda.synchronize()
    return od, ld


def _backward(qd, od, gd, ld, shape):
    """d(qkv) (N*T, 3*D) from the o and lse the forward kernel produced; output pre-filled with NaN"""
    from rgm import native as R
    N, T, heads, hd = shape
    cd, sd_ = _tables(T, hd)
    out = torch.full((N * T, 3 * heads * hd), float("nan"), device="cuda")
    R.check(R.lib.rgm_rotary_attention_bwd(R.ptr(qd), R.ptr(od), R.ptr(gd), R.ptr(ld), R.ptr(out), R.ptr(cd), R.ptr(sd_),
                                           N, T, heads, hd, hd // 4, R.current_stream()))
    torch.cuda.synchronize()
    return out


class _Mode:
    """auto: the library's own choice.  split0 / split1: rgm_set_attn_split pinned (per-head with the lone-token path / per-tile).
    stream: every length on the streaming forward and backward.  Everything is restored on exit."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from rgm import native as R
        self.restore = []
        if self.mode in ("split0", "split1"):
            R.lib.rgm_set_attn_split(int(self.mode[-1]))
            self.restore.append(lambda: R.lib.rgm_set_attn_split(-1))
        elif self.mode == "stream":
            pf, pb = R.lib.rgm_set_attn_stream(1), R.lib.rgm_set_attn_bwd_stream(1)
            self.restore += [lambda: R.lib.rgm_set_attn_stream(pf), lambda: R.lib.rgm_set_attn_bwd_stream(pb)]
        else:
            assert self.mode == "auto", self.mode
        return self

    def __exit__(self, *exc):
        for fn in self.restore:
            fn()
        return False


def _kernels(fam, shape, mode, backward):
    """forward (o, lse; and o of the entry without lse) and backward of one case in one mode -> numpy"""
    from gpu_util import dev
    qkv, d_o = A.inputs(fam, shape)
    qd = dev(qkv)
    with _Mode(mode):
        od, ld = _forward(qd, shape)
        o2, _ = _forward(qd, shape, with_lse=False)
        out = {"o": od.cpu().numpy(), "lse": ld.cpu().numpy().reshape(shape[0], shape[2], shape[1]), "o_nolse": o2.cpu().numpy()}
        if backward:
            out["dqkv"] = _backward(qd, od, dev(d_o), ld, shape).cpu().numpy()
    return out


def _split():
    from gpu_util import split_torch_dtype
    return split_torch_dtype()


def _report(**rec):
    path = os.environ.get("RGM_ATTN_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")


def _check(fam, shape, mode, precision, got, quantities, against=None):
    """every block of every quantity within its component's bound (attn_cases.bound); every figure printed before anything is asserted.
    against: the resident kernels' result -- the forced streaming kernels also stay within twice the bound of it."""
    split = _split()
    err = A.errors({k: got[k] for k in quantities}, fam, shape)
    r32 = A.twin_errors("fp32", fam, shape)
    failures = []
    for qn in quantities:
        bnd = A.bound(precision, qn, fam, shape, split)
        tw = A.twin_errors(precision, fam, shape, split)[qn]
        R, _ = A.headroom(precision, "bwd" if qn == "dqkv" else "fwd", shape, split)
        comp = (lambda e: [float(e.max())]) if qn == "lse" else (lambda e: [float(x) for x in e.max(axis=(0, 2))])
        print(f"{fam} {A.shape_id(shape)} {mode} {precision} {qn}: kernel {comp(err[qn])} twin {comp(tw)} ref32 {comp(r32[qn])} "
              f"R_p {R:.2f} bound {np.atleast_1d(bnd).tolist()}")
        _report(family=fam, shape=A.shape_id(shape), mode=mode, precision=precision, quantity=qn, kernel=comp(err[qn]), twin=comp(tw),
                ref32=comp(r32[qn]), R=R, bound=np.atleast_1d(bnd).tolist())
        if not A.within(err[qn], bnd):
            failures.append((qn, comp(err[qn]), np.atleast_1d(bnd).tolist()))
        if against is not None:
            d = A.lse_err(got["lse"], against["lse"]) if qn == "lse" else A.block_err(got[qn], against[qn], *shape)
            print(f"    vs the resident kernels: {comp(d)}")
            if not A.within(d, 2.0 * bnd):
                failures.append((qn + " vs resident", comp(d), (2.0 * np.atleast_1d(bnd)).tolist()))
    assert not failures, (fam, shape, mode, precision, failures)


def _run_case(fam, shape, mode, precision):
    backward = A.has_backward(fam)
    got = _kernels(fam, shape, mode, backward)
    assert np.array_equal(got["o"], got["o_nolse"], equal_nan=True), (fam, shape, mode)      # writing lse changes nothing else
    against = _kernels(fam, shape, "auto", backward) if mode == "stream" else None
    _check(fam, shape, mode, precision, got, ("o", "lse") + (("dqkv",) if backward else ()), against)


ALL = A.FAMILIES + ("randn15",)                                  # randn15: the forward on the suite's own x 1.5 input
RESIDENT = [(s, m) for s in A.RESIDENT_SHAPES for m in (("auto", "split0", "split1") if s[1] in (256, 257) else ("auto",))]


def _sid(v):
    return A.shape_id(v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("fam", ALL)
@pytest.mark.parametrize("shape,mode", RESIDENT, ids=_sid)
def test_resident_kernels(shape, mode, fam, precision):
    _run_case(fam, shape, mode, precision)


@pytest.mark.parametrize("fam", ALL)
@pytest.mark.parametrize("shape", A.RESIDENT_SHAPES, ids=_sid)
def test_resident_shapes_on_the_streaming_kernels(shape, fam, precision):
    from rgm import native as R
    before = R.lib.rgm_attn_bwd_stream_launches()
    _run_case(fam, shape, "stream", precision)
    assert R.lib.rgm_attn_bwd_stream_launches() == before + (1 if A.has_backward(fam) else 0)
    assert R.lib.rgm_set_attn_stream(0) == 0 and R.lib.rgm_set_attn_bwd_stream(0) == 0       # both switches restored


@pytest.mark.parametrize("fam", ALL)
@pytest.mark.parametrize("shape", A.STREAM_SHAPES, ids=_sid)
def test_streaming_kernels(shape, fam, precision):
    _run_case(fam, shape, "auto", precision)


@pytest.mark.parametrize("fam", A.LONG_FAMILIES)
@pytest.mark.parametrize("shape", A.LONG_SHAPES, ids=_sid)
def test_streaming_kernels_at_the_ceiling_and_a_ragged_length(shape, fam, precision):
    _run_case(fam, shape, "auto", precision)


@pytest.mark.parametrize("fam", A.PAIR_FAMILIES)
@pytest.mark.parametrize("shape", A.PAIR_SHAPES, ids=_sid)
def test_many_pair_short_sequence_launchers(shape, fam, precision):
    _run_case(fam, shape, "auto", precision)


# ------------------------------------------------------------------------------------------------ expected values known exactly
@pytest.mark.parametrize("shape", A.KEYCOUNT_SHAPES, ids=_sid)
def test_key_count(shape, precision):
    """q = 0: every score is exactly 0, so lse = ln T and o = the column mean of v.  One key too many or too few at T = 8192 moves lse by
    1.2e-4 -- inside the norm-wise bf16x3 tolerance of the other tests (2e-5 x 9), 12 times the 1e-5 asked here."""
    N, T, heads, hd = shape
    got = _kernels("zeroq", shape, "auto", backward=False)
    dl = float(np.abs(got["lse"].astype(np.float64) - math.log(T)).max())
    print(f"key count {A.shape_id(shape)} {precision}: |lse - ln T| {dl:.3e}")
    _check("zeroq", shape, "auto", precision, got, ("o",))
    assert dl <= 1e-5, (shape, precision, dl)


@pytest.mark.parametrize("shape,mode", [(s, "auto") for s in A.JUMP_SHAPES] + [(s, "stream") for s in A.JUMP_STREAM_SHAPES], ids=_sid)
def test_underflowing_rescale(shape, mode, precision):
    """`jump`: the last key's score is about 176 above all others, the rescale factor of the final block underflows to 0 and every row of o
    is v[T-1] of its head (exactly in float64 and in the float32 reference; the bf16x3 modes carry v as hi + lo)."""
    got = _kernels("jump", shape, mode, backward=False)
    assert np.isfinite(got["o"]).all() and np.isfinite(got["lse"]).all(), (shape, mode, precision)
    tol = A.tolerances()["fwd"][precision]
    eo = A.errors({"o": got["o"], "lse": got["lse"]}, "jump", shape)["o"]                     # the reference's o IS v[T-1], broadcast
    print(f"jump {A.shape_id(shape)} {mode} {precision}: o vs v[T-1] worst block {eo.max():.3e} (TOL {tol:.0e})")
    _check("jump", shape, mode, precision, got, ("lse",))
    assert eo.max() <= tol, (shape, mode, precision, float(eo.max()))


SILENT = [((2, 256, 16, 72), "split0"), ((2, 256, 16, 72), "split1"), ((2, 257, 6, 64), "split0"), ((2, 257, 6, 64), "split1"),
          ((2, 257, 6, 64), "stream"), ((2, 256, 16, 72), "stream"), ((1, 1000, 4, 72), "auto"), ((2, 300, 6, 64), "auto")]


@pytest.mark.parametrize("shape,mode", SILENT, ids=_sid)
def test_silent_heads(shape, mode, precision):
    """d_o zero for all heads but one: the d(qkv) blocks of the silent heads are exactly 0.0, and the loud head's block equals, bit for bit,
    its block from the run with every head loud."""
    from gpu_util import dev
    N, T, heads, hd = shape
    qkv, d_o = A.inputs("randn", shape)
    loud = heads // 2
    quiet_do = np.zeros_like(d_o).reshape(N, T, heads, hd)
    quiet_do[:, :, loud] = d_o.reshape(N, T, heads, hd)[:, :, loud]
    qd = dev(qkv)
    with _Mode(mode):
        od, ld = _forward(qd, shape)
        full = _backward(qd, od, dev(d_o), ld, shape).cpu().numpy().reshape(N, T, 3, heads, hd)
        one = _backward(qd, od, dev(quiet_do.reshape(d_o.shape)), ld, shape).cpu().numpy().reshape(N, T, 3, heads, hd)
    silent = np.delete(one, loud, axis=3)
    assert np.isfinite(one).all() and (silent == 0.0).all(), (shape, mode, int((silent != 0).sum()))
    assert np.array_equal(one[:, :, :, loud].view(np.int32), full[:, :, :, loud].view(np.int32)), (shape, mode)


NEIGHBOURS = [(37, 6, 64, "split0"), (37, 6, 64, "split1"), (200, 16, 72, "split0"), (200, 16, 72, "split1"), (257, 6, 64, "split0"),
              (257, 6, 64, "split1"), (300, 6, 64, "split0"), (1000, 4, 72, "split0"), (257, 6, 64, "stream"), (200, 16, 72, "stream")]


@pytest.mark.parametrize("T,heads,hd,mode", NEIGHBOURS, ids=_sid)
def test_neighbours(T, heads, hd, mode, precision):
    """N = 2 with every input row of sample 1 NaN, and a guard of 64 NaN rows behind the last sample inside the same allocation (the
    kernels get views of it: no read leaves the allocation).  A masked key still multiplies its V row and 0 x NaN is NaN, so whatever a
    kernel reads behind a sample's last tile shows: o, lse and d(qkv) of sample 0 must be finite and bit-identical to the N = 1 run.
    rgm_set_attn_split is pinned for both runs (the automatic choice depends on N, and the two modes sum in different orders)."""
    D = heads * hd
    GUARD = 64
    qkv, d_o = A.inputs("randn", (1, T, heads, hd))

    def run(N):
        shape = (N, T, heads, hd)
        rows = N * T + GUARD
        qd = torch.full((rows, 3 * D), float("nan"), device="cuda")
        gd = torch.full((rows, D), float("nan"), device="cuda")
        qd[:T] = torch.from_numpy(qkv).cuda()
        gd[:T] = torch.from_numpy(d_o).cuda()
        with _Mode(mode):
            od, ld = _forward(qd, shape)
            # the backward reads o and lse as the forward left them (sample 1: NaN), again with NaN rows behind them
            og = torch.full((rows, D), float("nan"), device="cuda")
            lg = torch.full((N * heads * T + GUARD,), float("nan"), device="cuda")
            og[:N * T] = od
            lg[:N * heads * T] = ld
            dd = _backward(qd, og, gd, lg, shape)
        return od[:T].cpu().numpy(), ld[:heads * T].cpu().numpy(), dd[:T].cpu().numpy()
    one, two = run(1), run(2)
    for name, a, b in zip(("o", "lse", "dqkv"), one, two):
        assert np.isfinite(a).all(), (name, "N = 1", T, mode, int((~np.isfinite(a)).sum()))
        assert np.isfinite(b).all(), (name, "N = 2", T, mode, int((~np.isfinite(b)).sum()))
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), (name, T, mode, int((a != b).sum()))


# ------------------------------------------------------------------------------------------------ the models on peaked weights
from test_gpu_guided_long import GRAD_TOL, TOL  # noqa: E402  (outputs 2e-4, gradients 5e-4: the fp32 bounds of test_gpu_dit.py, imported)
CONTRACT = 1e-3                                                  # the project's stated contract, what the bf16x3 modes are held to here
XL2 = dict(depth=2, hidden=1152, heads=16, patch=8, in_ch=4, out_ch=4, num_classes=3)
CLS2 = dict(depth=2, hidden=384, heads=6, patch=8, in_ch=4, classifier=True, cls_classes=16)


def _randn(seed, *shape):
    return np.random.RandomState(int(seed)).randn(*shape).astype(np.float32)


@pytest.fixture
def long_on():
    from guided_diffusion import dit
    dit.set_long_backward(True)
    yield
    dit.set_long_backward(None)


def _peaked_weights(g, tag, arch):
    from rgm import synth
    return A.peak_qk(synth.dit_state_dict(int(g[f"{tag}.seed"][0]), **arch), float(g["qk_gain"][0]))


def _model_bounds(precision):
    return (TOL, GRAD_TOL) if precision == "fp32" else (CONTRACT, CONTRACT)


@pytest.mark.parametrize("H", [128, 256])
def test_peaked_eps_network_and_its_input_gradient(H, precision, long_on):
    """XL-2 on weights whose scores reach 30 to 60 (tests/golden/make_golden_peaked.py), against the reference module run in float64:
    T = 256 on the resident kernels, T = 512 on the streaming pair.  fp32 within the bounds of test_gpu_dit.py; the bf16x3 modes within
    the project's contract of 1e-3, the measured value printed (docs/rounds/attn_inputs.md)."""
    from conftest import load_golden
    from gpu_util import dev, load_module, rel
    from guided_diffusion.dit import DiTRotary
    g = load_golden("peaked")
    m = load_module(DiTRotary(input_size=[128, 16], patch_size=8, in_channels=4, hidden_size=1152, depth=2, num_heads=16, num_classes=3,
                              learn_sigma=False), _peaked_weights(g, "xl2", XL2))
    s = int(g[f"xl2.x{H}_seed"][0])
    eps, grad = m.vjp(dev(_randn(s, 1, 4, H, 16)), dev(g[f"xl2.t{H}"]), dev(g[f"xl2.y{H}"]), dev(_randn(s + 1000, 1, 4, H, 16)))
    ee, eg = rel(eps.cpu().numpy(), g[f"xl2.eps{H}_64"]), rel(grad.cpu().numpy(), g[f"xl2.grad{H}_64"])
    re_, rg = rel(g[f"xl2.eps{H}_32"], g[f"xl2.eps{H}_64"]), rel(g[f"xl2.grad{H}_32"], g[f"xl2.grad{H}_64"])
    print(f"peaked xl2 H={H} {precision}: eps {ee:.3e}, grad {eg:.3e} against float64 (the reference's own float32: {re_:.3e}, {rg:.3e})")
    _report(family="peaked_xl2", shape=f"H{H}", mode="model", precision=precision, quantity="eps,grad", kernel=[ee, eg], ref32=[re_, rg])
    bo, bg = _model_bounds(precision)
    assert ee <= bo and eg <= bg, (H, precision, ee, eg)


@pytest.mark.parametrize("H", [128, 256])
def test_peaked_classifier_logits_and_mse_gradient(H, precision, long_on):
    """the depth-2 S/8 classifier on peaked weights at T = 257 (resident backward, lone-token / per-tile paths) and T = 513 (streaming)"""
    from conftest import load_golden
    from gpu_util import dev, load_module, rel
    from guided_diffusion.condition_functions import grad_nn_zt_mse
    from guided_diffusion.dit import DiTRotaryClassifier
    g = load_golden("peaked")
    m = load_module(DiTRotaryClassifier(input_size=[128, 16], patch_size=8, in_channels=4, hidden_size=384, depth=2, num_heads=6,
                                        num_classes=16, chord=False), _peaked_weights(g, "cls", CLS2))
    x, t, rule = dev(_randn(g[f"cls.x{H}_seed"][0], 2, 4, H, 16)), dev(g[f"cls.t{H}"]), dev(g[f"cls.rule{H}"])
    logits, grad = m.value_and_grad(x, t, rule, "mse", 10.0)
    el, eg = rel(logits.cpu().numpy(), g[f"cls.logits{H}_64"]), rel(grad.cpu().numpy(), g[f"cls.grad{H}_64"])
    rl, rg = rel(g[f"cls.logits{H}_32"], g[f"cls.logits{H}_64"]), rel(g[f"cls.grad{H}_32"], g[f"cls.grad{H}_64"])
    print(f"peaked cls H={H} {precision}: logits {el:.3e}, grad {eg:.3e} against float64 (the reference's own float32: {rl:.3e}, {rg:.3e})")
    _report(family="peaked_cls", shape=f"H{H}", mode="model", precision=precision, quantity="logits,grad", kernel=[el, eg], ref32=[rl, rg])
    bo, bg = _model_bounds(precision)
    assert el <= bo and eg <= bg, (H, precision, el, eg)
    assert torch.equal(grad_nn_zt_mse(x, t, rule=rule, classifier_scale=10., classifier=m), grad)
