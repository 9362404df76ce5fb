"""Inputs, CPU references, the error measure and the bound of the GEMM and LayerNorm tests on offset, outlier, wide-range, cancelling,
one-K-tile and tail inputs (test_gemm_cases_host.py, test_gpu_gemm_inputs.py).  A plain helper module: no fixtures, nothing here touches a GPU.

Layout: A (M, K), B (N, K) float32, C = epi(alpha * A . B^T + bias) (* gate[row // rows_per_gate]) (+ res) like rgm_gemm; LayerNorm rows
x (rows, D) with per-sample modulation rows (samples, D).

References: ref64 (numpy float64 throughout); ref32 (torch CPU float32 of the same expression: the comparator of the fp32 kernels); twin
(the hi*hi + hi*lo + lo*hi product of csrc/common.h in float64 through attn_cases.split_parts / _x3, epilogue in float64: the comparator of
both bf16x3 modes).  It restates the documented arithmetic, not the kernels."""
import numpy as np
import torch

import attn_cases

F32 = np.float32
BLOCK = 16                                  # a common divisor of every tile, slab and MFMA shape of csrc/gemm*.hip
KTILE = 32                                  # values per K-tile (one 128-byte split line)
KT_FAMILIES = ("ktile_first", "ktile_mid", "ktile_last")
FAMILIES = ("randn", "offset", "outlier", "wide", "cancel") + KT_FAMILIES + ("tails",)
TAIL_BIASES = (-30.0, -12.0, -6.0, 0.0, 6.0, 12.0, 30.0)
OFFSET, OUTLIER_GAIN, CANCEL_EPS = 50.0, 300.0, 1e-3

SHAPES = [(1, 32, 32), (40, 584, 96), (300, 288, 416), (552, 608, 224), (257, 1152, 1152)]
SHAPES_144 = [(129, 144, 96), (300, 432, 416)]               # tile 81: N % 144 == 0, K >= 64
SPLITK_SHAPE = (200, 288, 2304)
HOST_SHAPES = [(200, 96, 64), (333, 288, 1152)]              # where the families were first characterised


def shape_id(shape):
    return "x".join(map(str, shape))


def case_seed(shape):
    """one seed per shape: every family of a shape edits the same draw, so `randn` calibrates the very draw the others modify"""
    M, N, K = shape
    return 9000 + 7 * M + 3 * N + K


# ------------------------------------------------------------------------------------------------ operands
def ktile_index(name, K):
    kt = K // KTILE
    return {"ktile_first": 0, "ktile_mid": kt // 2, "ktile_last": kt - 1}[name]


def family(name, M, N, K, seed):
    """(A (M, K), B (N, K)) float32, rebuilt from the seed"""
    rng = np.random.RandomState(seed)
    A = rng.randn(M, K)
    B = rng.randn(N, K) * (1 + np.arange(N)[:, None] / N) / np.sqrt(K)          # rows of B differ in scale: catches transposes
    extra = np.random.RandomState(seed + 1)
    if name in ("randn", "tails"):
        pass
    elif name == "offset":
        A = A + OFFSET
    elif name == "outlier":
        A[:, extra.choice(K, 2, replace=False)] *= OUTLIER_GAIN
    elif name == "wide":
        A = A * np.exp(3.0 * extra.randn(M, K))
    elif name == "cancel":
        h = K // 2
        B[:, h:] = -B[:, :h]
        A[:, h:] = A[:, :h].astype(F32) + CANCEL_EPS * extra.randn(M, h)
    elif name in KT_FAMILIES:
        j = ktile_index(name, K)
        keep = np.zeros(K, bool)
        keep[j * KTILE:(j + 1) * KTILE] = True
        A[:, ~keep] = 0
        B[:, ~keep] = 0
    else:
        raise KeyError(name)
    A, B = A.astype(F32), B.astype(F32)
    if name == "cancel":
        B[:, K // 2:] = -B[:, :K // 2]                                          # exact after the rounding to float32 as well
    return A, B


def bias_of(name, N, seed):
    """`tails`: a value of TAIL_BIASES per column (every activation evaluated at both tails); `cancel`: zero (any bias would bury the
    1e-3 that is left of the product); the others: 0.1 randn"""
    rng = np.random.RandomState(seed + 2)
    if name == "tails":
        return np.asarray(TAIL_BIASES, F32)[rng.randint(0, len(TAIL_BIASES), size=N)]
    return ((0.0 if name == "cancel" else 0.1) * rng.randn(N)).astype(F32)


def gate_res(M, N, rpg, seed):
    """gate ((M + rpg - 1) // rpg, N) and residual (M, N) of the proj / fc2 epilogue"""
    rng = np.random.RandomState(seed + 3)
    return rng.randn((M + rpg - 1) // rpg, N).astype(F32), rng.randn(M, N).astype(F32)


# ------------------------------------------------------------------------------------------------ references
def epilogue64(y, bias=None, act=0, alpha=1.0, gate=None, rpg=1, res=None):
    y = alpha * y
    if bias is not None:
        y = y + np.asarray(bias, np.float64)
    if act == 1:
        with np.errstate(over="ignore"):
            y = y / (1 + np.exp(-y))
    elif act == 2:
        y = 0.5 * y * (1 + np.tanh(np.sqrt(2 / np.pi) * (y + 0.044715 * y ** 3)))
    if gate is not None:
        y = y * np.asarray(gate, np.float64)[np.arange(y.shape[0]) // rpg]
    if res is not None:
        y = y + np.asarray(res, np.float64)
    return y


def ref64(A, B, **epi):
    return epilogue64(A.astype(np.float64) @ B.astype(np.float64).T, **epi)


def _t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32))


def ref32(A, B, **epi):
    """torch CPU float32 of the same expression"""
    return _epilogue32(_t32(A) @ _t32(B).T, **epi)


def ref32_tiles(A, B, **epi):
    """the same in another summation order: one float32 product per K-tile, added in float32 in K order (for the bound's factor 2)"""
    acc = torch.zeros(A.shape[0], B.shape[0])
    for k0 in range(0, A.shape[1], KTILE):
        acc = acc + _t32(A[:, k0:k0 + KTILE]) @ _t32(B[:, k0:k0 + KTILE]).T
    return _epilogue32(acc, **epi)


def _epilogue32(y, bias=None, act=0, alpha=1.0, gate=None, rpg=1, res=None):
    t = _t32
    y = F32(alpha) * y
    if bias is not None:
        y = y + t(bias)
    if act == 1:
        y = torch.nn.functional.silu(y)
    elif act == 2:
        y = torch.nn.functional.gelu(y, approximate="tanh")
    if gate is not None:
        y = y * t(gate)[torch.arange(y.shape[0]) // rpg]
    if res is not None:
        y = y + t(res)
    return y.numpy()


def twin_product(A, B):
    """A . B^T as the bf16x3 modes form it: hi*hi + hi*lo + lo*hi of the two-term splits, wide accumulation"""
    return attn_cases._x3(attn_cases.split_parts(A), attn_cases.split_parts(B))


def twin(A, B, **epi):
    return epilogue64(twin_product(A, B), **epi)


def twin_tiles(A, B, **epi):
    """the twin with a float32 accumulator: the three-term product of every K-tile added in K order and rounded to float32 each time"""
    (ah, al), (bh, bl) = attn_cases.split_parts(A), attn_cases.split_parts(B)
    acc = np.zeros((A.shape[0], B.shape[0]), F32)
    for k0 in range(0, A.shape[1], KTILE):
        s = slice(k0, k0 + KTILE)
        acc = (acc + (ah[:, s] @ (bh[:, s] + bl[:, s]).T + al[:, s] @ bh[:, s].T)).astype(F32)
    return epilogue64(acc.astype(np.float64), **epi)


def arith(precision):
    """the two bf16x3 modes share one twin"""
    return "fp32" if precision == "fp32" else "bf16x3"


def comparator(precision, A, B, **epi):
    return ref32(A, B, **epi) if arith(precision) == "fp32" else twin(A, B, **epi)


# ------------------------------------------------------------------------------------------------ the measure
def block_err(got, ref, b=BLOCK):
    """||got - ref||_2 / ||ref||_2 of every b x b block (the last row / column of blocks may be partial) -> (ceil(M / b), ceil(N / b)).
    NaN or inf in a block of `got` gives inf; a block whose reference is all zero passes only when `got` is all zero there."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and got.ndim == 2, (got.shape, ref.shape)
    ri, ci = np.arange(0, ref.shape[0], b), np.arange(0, ref.shape[1], b)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = np.add.reduceat(np.add.reduceat((got - ref) ** 2, ri, axis=0), ci, axis=1)
        s = np.add.reduceat(np.add.reduceat(ref ** 2, ri, axis=0), ci, axis=1)
        d = np.where(np.isfinite(d), d, np.inf)
        return np.where(s > 0, np.sqrt(d / s), np.where(d == 0, 0.0, np.inf))


def row_err(got, ref):
    """||got - ref||_2 / ||ref||_2 of every row (LayerNorm); NaN or inf gives inf"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = ((got - ref) ** 2).sum(-1)
        s = (ref ** 2).sum(-1)
        d = np.where(np.isfinite(d), d, np.inf)
        return np.where(s > 0, np.sqrt(d / s), np.where(d == 0, 0.0, np.inf))


def worst(err):
    """(value, (block row, block column)) of the largest entry"""
    err = np.asarray(err)
    i = np.unravel_index(int(np.argmax(np.where(np.isnan(err), np.inf, err))), err.shape)
    return float(err[i]), tuple(int(v) for v in i)


def rel(a, b):
    """the suite's norm-wise measure (gpu_util.rel), for the comparisons with it"""
    return attn_cases.rel(a, b)


def tolerances(epilogue):
    """TOL per arithmetic: the constants of the existing kernel tests, imported (never copied).  `epilogue`: alpha / gate / residual /
    activation in play (test_gemm_fused_epilogues' figure for fp32), else the plain product + bias"""
    import test_gpu_ops
    return {"fp32": test_gpu_ops.GEMM_EPI_TOL if epilogue else test_gpu_ops.GEMM_TOL, "bf16x3": test_gpu_ops.GEMM_X3_TOL}


def ln_tolerance():
    import test_gpu_ops
    return test_gpu_ops.LN_TOL


# ------------------------------------------------------------------------------------------------ cases, cached references, the bound
PLAIN = (0, 1.0, 0, False)                  # an epilogue is (act, alpha, rows_per_gate or 0 for no gate, residual); the bias is always on
_CACHE = {}


def is_epilogue(epi):
    return tuple(epi) != PLAIN


def operands(fam, shape, epi=PLAIN):
    """{'A', 'B', 'bias', 'act', 'alpha', 'gate', 'rpg', 'res'} of a case"""
    act, alpha, rpg, has_res = epi
    M, N, K = shape
    seed = case_seed(shape)
    A, B = family(fam, M, N, K, seed)
    gate, res = gate_res(M, N, rpg or M, seed)
    return dict(A=A, B=B, bias=bias_of(fam, N, seed), act=act, alpha=alpha, gate=gate if rpg else None, rpg=max(rpg, 1),
                res=res if has_res else None)


def _epi_kwargs(op):
    return {k: op[k] for k in ("bias", "act", "alpha", "gate", "rpg", "res")}


def reference(fam, shape, epi=PLAIN):
    key = ("ref64", fam, shape, tuple(epi))
    if key not in _CACHE:
        op = operands(fam, shape, epi)
        _CACHE[key] = ref64(op["A"], op["B"], **_epi_kwargs(op))
    return _CACHE[key]


def comparator_errors(precision, fam, shape, epi=PLAIN):
    """block errors against float64 of the comparator of `precision` on a case, cached (only the errors are kept)"""
    key = ("cmp", arith(precision), fam, shape, tuple(epi))
    if key not in _CACHE:
        op = operands(fam, shape, epi)
        _CACHE[key] = block_err(comparator(precision, op["A"], op["B"], **_epi_kwargs(op)), reference(fam, shape, epi))
    return _CACHE[key]


def headroom(precision, shape, epi=PLAIN):
    """R = max(1, TOL / worst block of the comparator on `randn` at this shape and epilogue): how far above its arithmetic's model the
    suite already lets a kernel sit -> (R, the comparator's worst block)"""
    w = float(comparator_errors(precision, "randn", shape, epi).max())
    return max(1.0, tolerances(is_epilogue(epi))[arith(precision)] / w) if w > 0 else 1.0, w


def bound(precision, fam, shape, epi=PLAIN):
    """max(TOL, 2 R x worst block of the comparator on this family, shape and epilogue): one number for every block of the case.  The
    factor 2 covers the summation order the comparator does not share with a kernel, not its draw; it is not to be raised."""
    R, _ = headroom(precision, shape, epi)
    return max(tolerances(is_epilogue(epi))[arith(precision)], 2.0 * R * float(comparator_errors(precision, fam, shape, epi).max()))


def within(err, bnd):
    """every block within the bound; NaN fails"""
    return bool(np.all(np.asarray(err) <= bnd))


# ------------------------------------------------------------------------------------------------ family properties
def properties(fam, shape):
    """numbers the family table is asserted on"""
    M, N, K = shape
    A, B = family(fam, M, N, K, case_seed(shape))
    a, b = A.astype(np.float64), B.astype(np.float64)
    mass = np.abs(a) @ np.abs(b).T                                              # sum_k |a||b| per output
    out = {"offset_ratio": float(np.abs(a.mean()) / a.std()),
           "cancel_ratio": float(np.abs(a @ b.T).mean() / mass.mean()),
           "dyn_range": float(np.log2(np.abs(a).max() / np.abs(a)[a != 0].min())) if (a != 0).any() else 0.0}
    col_mass = np.abs(a).sum(0) * np.abs(b).sum(0)
    out["top2_share"] = float(np.sort(col_mass)[-2:].sum() / col_mass.sum())
    tile_mass = col_mass.reshape(-1, KTILE).sum(1)
    out["top_tile_share"] = float(tile_mass.max() / tile_mass.sum())
    out["nonzero_tiles"] = [int(i) for i in np.nonzero(tile_mass)[0]]
    return out


# ------------------------------------------------------------------------------------------------ mutants of the twin (CPU only)
def _tile_products(A, B, lo_hi=True):
    """per-K-tile twin products (KT, M, N): hi*hi + hi*lo (+ lo*hi)"""
    (ah, al), (bh, bl) = attn_cases.split_parts(A), attn_cases.split_parts(B)
    kt = A.shape[1] // KTILE
    out = np.empty((kt, A.shape[0], B.shape[0]))
    for j in range(kt):
        s = slice(j * KTILE, (j + 1) * KTILE)
        out[j] = ah[:, s] @ (bh[:, s] + bl[:, s]).T + (al[:, s] @ bh[:, s].T if lo_hi else 0.0)
    return out


def mutant_gemm(name, op, location=None):
    """the twin of a case with one operation swapped -> (result, the blocks (16 x 16) the defect touches as (row slice, column slice)):
      'drop_lo_hi'   one 32 x 32 block drops a_lo . b_hi of one K-tile
      'ring_shift'   one 16-row band of one 128-column tile takes its K-tiles one ring stage late: the last counted twice, the first dropped
      'gate_late'    the gate row switches one row late at a sample boundary (needs a gate)
      'bias_prev'    the bias of the last, partial group of 32 columns is taken from the group before it"""
    A, B = op["A"], op["B"]
    M, N = A.shape[0], B.shape[0]
    kt = A.shape[1] // KTILE
    epi = _epi_kwargs(op)
    if name == "drop_lo_hi":
        r0, c0 = location or (32 * ((M // 32) // 2), 32 * ((N // 32) // 2))
        rs, cs = slice(r0, min(M, r0 + 32)), slice(c0, min(N, c0 + 32))
        j = kt // 2
        s = slice(j * KTILE, (j + 1) * KTILE)
        al, bh = attn_cases.split_parts(A)[1], attn_cases.split_parts(B)[0]
        y = twin_product(A, B)
        y[rs, cs] -= al[rs, s] @ bh[cs, s].T
        return epilogue64(y, **epi), (rs, cs)
    if name == "ring_shift":
        r0, c0 = location or (16 * ((M // 16) // 2), 128 * ((N // 128) // 2))
        rs, cs = slice(r0, min(M, r0 + 16)), slice(c0, min(N, c0 + 128))
        y = twin_product(A, B)
        if kt > 1:
            first = _tile_products(A[rs, :KTILE], B[cs, :KTILE])[0]
            last = _tile_products(A[rs, -KTILE:], B[cs, -KTILE:])[0]
            y[rs, cs] += last - first
        return epilogue64(y, **epi), (rs, cs)
    if name == "gate_late":
        assert op["gate"] is not None
        rpg = op["rpg"]
        y = epilogue64(twin_product(A, B), **dict(epi, gate=None, res=None))
        rows = np.arange(M)
        g = rows // rpg
        b = rpg * max(1, (M // rpg) // 2)                                        # one boundary row: it keeps the gate row of the sample before
        if b < M:
            g[b] -= 1
        y = y * op["gate"].astype(np.float64)[g]
        if op["res"] is not None:
            y = y + op["res"]
        return y, (slice(b, b + 1), slice(0, N))
    if name == "bias_prev":
        c0 = N - (N % 32 or 32)
        bias = np.array(op["bias"], np.float64)
        if c0 >= 32:
            bias[c0:] = bias[c0 - 32:c0 - 32 + (N - c0)]
        return epilogue64(twin_product(A, B), **dict(epi, bias=bias)), (slice(0, M), slice(c0, N))
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ LayerNorm rows
LN_FAMILIES = ("randn", "offset", "outlier", "const", "ramp")
LN_DIMS = (4, 8, 252, 256, 512, 516, 1152, 1280, 1284, 2048)
LN_FORMS = ("mod", "affine", "both")
LN_SAMPLES, LN_ROWS = 3, 37
LN_EPS = 1e-6


def ln_rows(name, rows, D, seed):
    """x (rows, D) float32"""
    rng = np.random.RandomState(seed)
    x = rng.randn(rows, D)
    if name == "randn":
        x = x * 3 + 1
    elif name == "offset":
        x = x + 1e3
    elif name == "outlier":
        x[:, rng.randint(D)] = 1e4
    elif name == "const":
        # every entry of a row equal, and a value of few bits (k / 2, |k| <= 12): every partial sum of a row is exact in float32 in any
        # order, so mean == the value, every x - mean == 0 and the variance is exactly 0 whatever the kernel's reduction tree
        x = np.repeat(((np.arange(rows) % 25) - 12)[:, None] * 0.5, D, axis=1)
    elif name == "ramp":
        x = x * (2.0 ** ((np.arange(rows) % 24) - 12))[:, None]
    else:
        raise KeyError(name)
    return x.astype(F32)


def ln_params(D, seed, samples=LN_SAMPLES):
    """weight, bias (D) and a strided modulation buffer (samples, 6 D) like the DiT's: shift = cols D..2D, scale = cols 2D..3D"""
    rng = np.random.RandomState(seed + 5)
    w, b = (1 + 0.1 * rng.randn(D)).astype(F32), rng.randn(D).astype(F32)
    mod = rng.randn(samples, 6 * D).astype(F32)
    mod[:, D:2 * D] = np.where(rng.rand(samples, D) < 0.5, -20.0, 20.0)
    mod[:, 2 * D:3 * D] = np.exp(rng.uniform(-2.0, 2.0, size=(samples, D))) - 1.0
    return w, b, mod


def ln_case(fam, D, form, rows_per_sample=LN_ROWS, samples=LN_SAMPLES):
    seed = 500 + D
    x = ln_rows(fam, samples * rows_per_sample, D, seed + LN_FAMILIES.index(fam))
    w, b, mod = ln_params(D, seed, samples)
    return dict(x=x, w=w if form in ("affine", "both") else None, b=b if form in ("affine", "both") else None,
                mod=mod if form in ("mod", "both") else None, rps=rows_per_sample, D=D)


def ln_ref(c, dtype=np.float64, mutant=None):
    """LayerNorm (+ affine) (+ modulation) of a case in numpy at `dtype`.  mutants: 'var32' the variance as E[x^2] - mean^2 in float32;
    'short' the statistics over D - 4 columns (the last chunk of four missing)"""
    x = c["x"].astype(dtype)
    D = c["D"]
    if mutant == "var32":
        x32 = c["x"].astype(F32)
        mu = x32.mean(-1, keepdims=True, dtype=F32)
        var = ((x32 * x32).mean(-1, keepdims=True, dtype=F32) - mu * mu).astype(dtype)
        mu = mu.astype(dtype)
    else:
        xs = x[:, :D - 4] if mutant == "short" and D > 4 else x
        mu = xs.mean(-1, keepdims=True)
        var = ((xs - mu) ** 2).mean(-1, keepdims=True)
    y = (x - mu) / np.sqrt(var + dtype(LN_EPS))
    if c["w"] is not None:
        y = y * c["w"].astype(dtype) + c["b"].astype(dtype)
    if c["mod"] is not None:
        s = np.arange(x.shape[0]) // c["rps"]
        y = y * (1 + c["mod"][s, 2 * D:3 * D].astype(dtype)) + c["mod"][s, D:2 * D].astype(dtype)
    return y


def ln_ref32(c):
    """the comparator: torch CPU float32 layer_norm followed by the modulation"""
    D = c["D"]
    x = torch.from_numpy(c["x"])
    y = torch.nn.functional.layer_norm(x, (D,), None if c["w"] is None else torch.from_numpy(c["w"]),
                                       None if c["b"] is None else torch.from_numpy(c["b"]), LN_EPS)
    if c["mod"] is not None:
        s = torch.arange(x.shape[0]) // c["rps"]
        mod = torch.from_numpy(c["mod"])
        y = y * (1 + mod[s, 2 * D:3 * D]) + mod[s, D:2 * D]
    return y.numpy()


def ln_const_expectation(c):
    """what a `const` row must give exactly: the normalised row is 0, so the sample's shift under a modulation alone, the affine bias
    under the affine form alone.  With both, bias * (1 + scale) + shift may or may not be one fused multiply-add: None, the bound only."""
    D = c["D"]
    rows = c["x"].shape[0]
    if c["mod"] is not None and c["b"] is not None:
        return None
    if c["mod"] is not None:
        return np.ascontiguousarray(c["mod"][np.arange(rows) // c["rps"], D:2 * D])
    return np.ascontiguousarray(np.broadcast_to(c["b"], (rows, D)))


def ln_comparator_errors(fam, D, form):
    key = ("ln", fam, D, form)
    if key not in _CACHE:
        c = ln_case(fam, D, form)
        _CACHE[key] = row_err(ln_ref32(c), ln_ref(c))
    return _CACHE[key]


def ln_headroom(D, form):
    w = float(ln_comparator_errors("randn", D, form).max())
    return (max(1.0, ln_tolerance() / w) if w > 0 else 1.0), w


def ln_bound(fam, D, form):
    R, _ = ln_headroom(D, form)
    return max(ln_tolerance(), 2.0 * R * float(ln_comparator_errors(fam, D, form).max()))
