"""Per-op parity of the decode linear kernels against a float64 reference, through the fm_op_* hooks
(each runs ONE production launcher on caller operands): launch_linear (the 16-row MFMA tile kernel),
launch_gemv (R <= 8), launch_rowgemv (one row), launch_bstream (bsacc_kernel / bstream_kernel, 8 < R <=
32), launch_finalize_norm and launch_prompt_skinny.  Run on the MI355X box: pytest -m gpu.

Inputs: seeded standard_normal x, weights scaled by 1 / sqrt(K), every row distinct; in bf16 runs all
inputs are rounded to bf16 first (round_bf16), so the float64 reference sees exactly what the kernel sees.

Reference and bound, per element.  Every case carries three float64 arrays through the rounding chain the
headers document (fm_kernels.h; linear_epi: round(acc + bias), round(res + round(acc + bias)),
round(silu(round(g))) * round(u); int8: round(round(acc) * scale); FIN: round(res + round(W x + bias))):
t the exact value with NO rounding, e a bound on |kernel's value - t|, and r the "restatement" (the same
chain with each rounding applied to the float64 value).  |got - t| <= e is asserted for EVERY element; the
share of elements with got == r is printed and asserted from below (summation order legitimately moves
last bits, so it is not 100 %).  With u8 = 2^-8 (half a bf16 ulp, relative) and u24 = 2^-24:

  accumulation   any fp32 summation order of K products: |acc - exact| <= K u24 (|x| . |w|); asserted with
                 the factor 2 (the MFMA's internal ordering, the split-K partial adds):
                 E = 2 K u24 (|x| @ |w|.T), evaluated in float64.  bf16 products are exact in fp32.
  fp32 add/mul   of a value t~ (|t~ - t| <= e) with an exact operand: e + u24 (|t| + e).
  bf16 rounding  of t~: e + u8 (|t| + e).  fp32 mode has no such term.
  silu           Lipschitz constant <= 1.1, plus 4 u24 |silu| for expf / add / divide in fp32.
  product        |a| e_b + |b| e_a + e_a e_b, then one fp32 rounding (the up-projection multiplies).
  raw fp32       EPI_F32 carries one rounding; EPI_SLAB partials and the skinny GEMM's slabs carry none: the
                 sum of the parts is held to E alone -- the sharpest checks here.
  int8 row GEMV  the kernel sums (q + 128) x and takes 128 sum(x) off at the end (fm_rowgemv.hip), so its
                 accumulation bound is 2 K u24 (|x| . |q + 128| + 128 sum |x|).
  norm prologue  X' = round(round(x rs) w).  rs = 1 / sqrt(mean(x^2) + eps) in fp32: the sum of K positive
                 terms is within (K + 1) u24 relative in any order, sqrt / divide / the fp32 product add
                 <= 10 u24, so rs is within band = ((K + 1) / 2 + 10) u24 of the float64 value.  X' is
                 monotone in rs, so the kernel's X' lies between the chain evaluated at rs (1 - band) and at
                 rs (1 + band): the matmul bound gets dX' @ |w|.T on top of E (dX' is zero for most elements
                 in bf16: only values next to a rounding boundary can move).  The X' values themselves are
                 held to 1 bf16 ulp / 4 fp32 ulp by test_gpu_ops.py.
  finalize_norm  the K parts are added in order in fp32, which numpy float32 restates exactly; outputs are
                 held to 1 bf16 ulp / 4 fp32 ulp (the form of test_gpu_ops._check).

Every case also asserts: the sentinel (columns N .. ld - 1 and rows >= R of every output array, pre-filled
with a finite bf16-exact value, come back bit-unchanged); reps = 3 gives the bits of reps = 1 and leaves no
ticket / counter word non-zero (finalize_norm: err == 0); and knob variants that only reschedule (same
summation order: gemv_u, gemv_nt, gemv_dummy, bs_dummy, bs_xfirst, bs_vec_epi, linear_u32, prompt_unroll, fin8,
row_qkv_rp) give the default's bits, while gemv_wpb 8 (another partition of the k-steps among waves) is held to
the bound on its own.

EPI_SLABFIN and EPI_SWIGLU8 work on whole 16-row tiles (the hooks refuse other N), so those epilogues run at
N in {16, 48, 1008} where the others run at {16, 40, 1000}.  bstream_kernel (fm_tune bstream_acc 0) is what
fp32 batched frames run.  In bf16, production reaches it only for shapes bsacc_plan declines: more than 6
tiles per block (N > 24576 at 256 CUs) or more than 80 k-steps per K part (a whole-K epilogue at K > 2560);
no S2-Pro linear is such a shape, so there the bf16 form is reachable through the knob alone.

Measured on MI355X, per family (kernel / epilogue / precision): the smallest share of elements bit-equal to
the restatement over the family's cases, and the largest |got - t| / e (finalize: |d| / ulp; its fp32 norm
output reaches the 4-ulp bar at d = 2560 and 8192).  The floors asserted are these shares minus 0.02.  fp32
shares are low because the restatement rounds the float64 sum once while the kernel rounds every add; the
raw-slab families compare the fp32 sum of the parts.
  bsacc/f32/bf16               0.9994     0.956         gemv/prenorm/f32/fp32        0.0446    0.0394
  bsacc/slab/bf16              0.2419   0.00036         gemv/prenorm/store/bf16      0.9998     0.969
  bsacc/slabfin/bf16           1.0000      0.81         gemv/prenorm/store/fp32      0.0446    0.0394
  bsacc/store/bf16             0.9994     0.973         gemv/prenorm/swiglu/bf16     0.9999     0.623
  bsacc/swiglu8/bf16           0.9997     0.699         gemv/prenorm/swiglu/fp32     0.0375    0.0244
  bsacc_prenorm/store/bf16     0.9999     0.915         gemv/prenorm/swiglu8/bf16    0.9998     0.568
  bsacc_prenorm/swiglu8/bf16   0.9999     0.616         gemv/prenorm/swiglu8/fp32    0.0000    0.0149
  bstream/f32/bf16             0.9997     0.766         linear/f32/bf16              0.9993     0.977
  bstream/f32/fp32             0.2531  0.000246         linear/f32/fp32              0.0919    0.0399
  bstream/slab/bf16            0.2558  5.22e-05         linear/resid/bf16            1.0000     0.968
  bstream/slab/fp32            0.1145  0.000112         linear/resid/fp32            0.2125     0.045
  bstream/store/bf16           0.9999     0.917         linear/store/bf16            0.9998     0.973
  bstream/store/fp32           0.3272   0.00213         linear/store/fp32            0.1202    0.0351
  bstream/swiglu8/bf16         1.0000     0.571         linear/swiglu/bf16           0.9999     0.688
  finalize/x/bf16              1.0000         0         linear/swiglu/fp32           0.0662     0.016
  finalize/x/fp32              1.0000         0         linear_split/f32/bf16        0.9994     0.723
  finalize/xn/bf16             1.0000         0         linear_split/f32/fp32        0.1648  0.000264
  finalize/xn/fp32             0.1000         4         linear_split/resid/bf16      1.0000     0.803
  gemv/norm/f32/bf16           0.9998     0.969         linear_split/resid/fp32      0.2758  0.000272
  gemv/norm/f32/fp32           0.0446    0.0449         linear_split/store/bf16      0.9998     0.823
  gemv/norm/store/bf16         0.9998     0.969         linear_split/store/fp32      0.2778  0.000287
  gemv/norm/store/fp32         0.0446    0.0449         linear_split/swiglu/bf16     0.9994     0.568
  gemv/norm/swiglu/bf16        0.9999     0.623         linear_split/swiglu/fp32     0.1100  0.000222
  gemv/norm/swiglu/fp32        0.0375    0.0244         rowgemv/fin                  1.0000     0.796
  gemv/plain/f32/bf16          0.9998      0.96         rowgemv/norm_f32             1.0000      0.62
  gemv/plain/f32/fp32          0.0250    0.0452         rowgemv/norm_store           1.0000     0.746
  gemv/plain/slab/bf16         0.2517    0.0207         rowgemv/norm_swiglu          1.0000      0.18
  gemv/plain/slab/fp32         0.0250    0.0452         rowgemv_q8/fin               1.0000     0.367
  gemv/plain/slabfin/bf16      1.0000      0.93         rowgemv_q8/norm_f32          1.0000    0.0615
  gemv/plain/slabfin/fp32      0.1250    0.0434         rowgemv_q8/norm_store        1.0000    0.0615
  gemv/plain/store/bf16        0.9998      0.96         rowgemv_q8/norm_swiglu       1.0000     0.126
  gemv/plain/store/fp32        0.0250    0.0452         skinny/act                   0.9962     0.636
  gemv/prenorm/f32/bf16        0.9998     0.969         skinny/slab                  0.0987   0.00304
"""
import numpy as np
import pytest

from fishmi import ops
from fishmi.synth import round_bf16
from linear_ref import (U24, mk as _mk, norm_ref, rb as _rb, rd as _rd, v_acc, v_add, v_mul, v_q8, v_rnd, v_silu,
                        v_swiglu, v_swiglu8)
from parity_util import knob, tuned  # noqa: F401  (knob: fixture)

pytestmark = pytest.mark.gpu

SENT = np.float32(-24576.0)  # -1.5 * 2^14: finite, bf16-exact, far outside every output
PRECS = ["bf16", "fp32"]

# measured share of bit-exact elements per family (see the docstring); asserted at this minus 0.02
MEASURED = {
    "bsacc/f32/bf16": 0.9994, "bsacc/slab/bf16": 0.2419, "bsacc/slabfin/bf16": 1.0000, "bsacc/store/bf16": 0.9994,
    "bsacc/swiglu8/bf16": 0.9997, "bsacc_prenorm/store/bf16": 0.9999, "bsacc_prenorm/swiglu8/bf16": 0.9999,
    "bstream/f32/bf16": 0.9997, "bstream/f32/fp32": 0.2531, "bstream/slab/bf16": 0.2558, "bstream/slab/fp32": 0.1145,
    "bstream/store/bf16": 0.9999, "bstream/store/fp32": 0.3272, "bstream/swiglu8/bf16": 1.0000,
    "finalize/x/bf16": 1.0000, "finalize/x/fp32": 1.0000, "finalize/xn/bf16": 1.0000, "finalize/xn/fp32": 0.1000,
    "gemv/norm/f32/bf16": 0.9998, "gemv/norm/f32/fp32": 0.0446, "gemv/norm/store/bf16": 0.9998,
    "gemv/norm/store/fp32": 0.0446, "gemv/norm/swiglu/bf16": 0.9999, "gemv/norm/swiglu/fp32": 0.0375,
    "gemv/plain/f32/bf16": 0.9998, "gemv/plain/f32/fp32": 0.0250, "gemv/plain/slab/bf16": 0.2517,
    "gemv/plain/slab/fp32": 0.0250, "gemv/plain/slabfin/bf16": 1.0000, "gemv/plain/slabfin/fp32": 0.1250,
    "gemv/plain/store/bf16": 0.9998, "gemv/plain/store/fp32": 0.0250, "gemv/prenorm/f32/bf16": 0.9998,
    "gemv/prenorm/f32/fp32": 0.0446, "gemv/prenorm/store/bf16": 0.9998, "gemv/prenorm/store/fp32": 0.0446,
    "gemv/prenorm/swiglu/bf16": 0.9999, "gemv/prenorm/swiglu/fp32": 0.0375, "gemv/prenorm/swiglu8/bf16": 0.9998,
    "gemv/prenorm/swiglu8/fp32": 0.0000, "linear/f32/bf16": 0.9993, "linear/f32/fp32": 0.0919,
    "linear/resid/bf16": 1.0000, "linear/resid/fp32": 0.2125, "linear/store/bf16": 0.9998,
    "linear/store/fp32": 0.1202, "linear/swiglu/bf16": 0.9999, "linear/swiglu/fp32": 0.0662,
    "linear_split/f32/bf16": 0.9994, "linear_split/f32/fp32": 0.1648, "linear_split/resid/bf16": 1.0000,
    "linear_split/resid/fp32": 0.2758, "linear_split/store/bf16": 0.9998, "linear_split/store/fp32": 0.2778,
    "linear_split/swiglu/bf16": 0.9994, "linear_split/swiglu/fp32": 0.1100, "rowgemv/fin": 1.0000,
    "rowgemv/norm_f32": 1.0000, "rowgemv/norm_store": 1.0000, "rowgemv/norm_swiglu": 1.0000, "rowgemv_q8/fin": 1.0000,
    "rowgemv_q8/norm_f32": 1.0000, "rowgemv_q8/norm_store": 1.0000, "rowgemv_q8/norm_swiglu": 1.0000,
    "skinny/act": 0.9962, "skinny/slab": 0.0987,
}
_seen = {}


def _floor(family):
    return MEASURED.get(family, 0.02) - 0.02


# ---------------------------------------------------------------------------------- the common assertions
def _buf(rows, ld):
    return np.full((rows, ld), SENT, np.float32)


def _check(tag, family, got, v):
    """every element within its bound; the bit-exact share against the restatement printed and held"""
    got64 = np.asarray(got, np.float64)
    assert got64.shape == v.t.shape, (tag, got64.shape, v.t.shape)
    assert np.isfinite(got64).all(), tag
    err = np.abs(got64 - v.t)
    tiny = 1e-300
    ratio = float((err / (v.e + tiny)).max())
    share = float((got64 == v.r).mean())
    lo, hi, n = _seen.get(family, (1.0, 0.0, 0))
    _seen[family] = (min(lo, share), max(hi, ratio), n + 1)
    print(f"{family} | {tag}: {share * 100:.2f}% bit-exact, max |got - t| / e {ratio:.3g}")
    bad = err > v.e
    assert not bad.any(), (tag, int(bad.sum()), np.argwhere(bad)[:4].tolist(), ratio)
    assert share >= _floor(family), (tag, share)
    return share


def _sentinel(tag, buf, rows, cols):
    m = np.ones(buf.shape, bool)
    m[:rows, :cols] = False
    hit = m & (buf.view(np.uint32) != SENT.view(np.uint32))
    assert not hit.any(), (tag, "sentinel overwritten", np.argwhere(hit)[:4].tolist())


def _sum_parts(parts):
    """raw fp32 K-part slabs summed in part order in fp32, as their consumers do (finalize_norm, the split-K
    epilogue): the parts - 1 extra adds are inside E's factor 2"""
    acc = parts[0].astype(np.float32)
    for q in range(1, len(parts)):
        acc = acc + parts[q].astype(np.float32)
    return acc.astype(np.float64)


def _same(tag, a, b):
    assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32)), (tag, "bits differ")


def _run(fn, shape, reps=(1, 3)):
    """fn(buf, reps) -> info; runs it on fresh sentinel-filled buffers for each reps value"""
    outs = []
    for rp in reps:
        buf = _buf(*shape)
        outs.append((buf, fn(buf, rp)))
    return outs


@pytest.fixture(scope="module", autouse=True)
def _family_summary():
    """after the module's tests: the per-family minimum share / maximum ratio of this run (the docstring's table)"""
    yield
    for fam, (lo, hi, n) in sorted(_seen.items()):
        print(f"\n  {fam:28s} min bit-exact {lo:.4f}  max ratio {hi:.3g}  ({n} checks)", end="")


# ---------------------------------------------------------------------------------- launch_linear (tile kernel)
TILE_SHAPES = [(1, 16, 32), (15, 24, 96), (16, 200, 544), (17, 16, 1056), (32, 24, 32), (33, 200, 96),
               (64, 24, 544), (65, 16, 1056), (100, 200, 544)]
LIN_EPIS = {"store": ops.EPI_STORE, "resid": ops.EPI_RESID, "swiglu": ops.EPI_SWIGLU, "f32": ops.EPI_F32}


def _linear_ref(epi, x, w, w2, bias, res, prec):
    a = v_add(v_acc(x, w), None if bias is None else bias[None, :].astype(np.float64))
    if epi == ops.EPI_STORE or epi == ops.EPI_F32:
        return v_rnd(a, prec)
    if epi == ops.EPI_RESID:
        return v_rnd(v_add(v_rnd(a, prec), res.astype(np.float64)), prec)
    u = v_acc(x, w2)
    return v_rnd(v_mul(v_rnd(v_silu(v_rnd(a, prec)), prec), v_rnd(u, prec)), prec)


def _linear_case(tag, fam, prec, R, N, K, epi_name, with_bias, seed, split=False, want_ksb=None):
    rng = np.random.default_rng(seed)
    epi = LIN_EPIS[epi_name]
    ldx, ldy, ldr = K + 8, N + 5, N + 3
    x = _mk(rng, (R, ldx), prec)
    w = _mk(rng, (N, K), prec, K ** -0.5)
    w2 = _mk(rng, (N, K), prec, K ** -0.5) if epi == ops.EPI_SWIGLU else None
    bias = _mk(rng, N, prec) if with_bias else None
    res = _mk(rng, (R, ldr), prec) if epi == ops.EPI_RESID else None
    v = _linear_ref(epi, x[:, :K], w, w2, bias, None if res is None else res[:, :N], prec)
    outs = _run(lambda buf, rp: ops.linear(w, x, buf, epi, w2=w2, bias=bias, res=res, precision=prec, split=split,
                                            reps=rp), (R + 2, ldy))
    (y1, (ksb, d1)), (y3, (_, d3)) = outs
    if want_ksb is not None:
        assert ksb == want_ksb, (tag, ksb)
    _check(tag, fam, y1[:R, :N], v)
    _sentinel(tag, y1, R, N)
    _same(tag, y1, y3)
    assert d1 == 0 and d3 == 0, (tag, d1, d3)
    return y1


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("R,N,K", TILE_SHAPES)
def test_linear_tile(prec, R, N, K):
    """R crosses the 1 / 2 / 4 column-group kernels and the c0 loop (65, 100); N 24 and 200 end in a part
    tile; K 32 / 96 give fewer k-steps than waves, 544 / 1056 leave a remainder after the unrolled loop;
    ldx = K + 8.  Every epilogue, bias on and off."""
    for i, epi in enumerate(LIN_EPIS):
        for with_bias in (False, True):
            tag = f"linear {prec} R={R} N={N} K={K} {epi} bias={int(with_bias)}"
            _linear_case(tag, f"linear/{epi}/{prec}", prec, R, N, K, epi, with_bias, 100 * R + N + K + i)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("R", [9, 33, 64])
def test_linear_tile_split_k(prec, R, knob):
    """split-K over part / tickets (8 < R <= 64): fm_tune linear_fill forces ksb 2 and 4 at 13 tiles of
    33 k-steps; the last-arriving block's epilogue and the ticket reset."""
    N, K = 200, 1056
    for fill, want in ((26, 2), (52, 4)):
        knob("linear_fill", fill)
        for i, epi in enumerate(LIN_EPIS):
            tag = f"linear split {prec} R={R} ksb={want} {epi}"
            _linear_case(tag, f"linear_split/{epi}/{prec}", prec, R, N, K, epi, i % 2 == 0, 7 * R + i, split=True,
                         want_ksb=want)


def test_linear_tile_u32_variant(knob):
    """fm_tune linear_u32 4 / 8 (16 < R <= 32) only deepens the load ring: same bits"""
    outs = []
    for u in (4, 8):
        knob("linear_u32", u)
        outs.append(_linear_case(f"linear u32={u}", "linear/store/bf16", "bf16", 32, 200, 1056, "store", True, 5))
    _same("linear_u32", outs[0], outs[1])


# ---------------------------------------------------------------------------------- launch_gemv
GEMV_COMBOS = [  # (prologue, epilogue) pairs launch_gemv dispatches (PRO_FATT aside)
    ("plain", "store"), ("plain", "f32"), ("plain", "slab"), ("plain", "slabfin"),
    ("norm", "store"), ("norm", "swiglu"), ("norm", "f32"),
    ("prenorm", "store"), ("prenorm", "swiglu"), ("prenorm", "f32"), ("prenorm", "swiglu8"),
]
PROS = {"plain": ops.PRO_PLAIN, "norm": ops.PRO_NORM, "prenorm": ops.PRO_PRENORM}
EPIS = {"store": ops.EPI_STORE, "swiglu": ops.EPI_SWIGLU, "f32": ops.EPI_F32, "slab": ops.EPI_SLAB,
        "slabfin": ops.EPI_SLABFIN, "swiglu8": ops.EPI_SWIGLU8}
EPS = 1e-6


def _ss_check(tag, ss, xfin, layout):
    """per-16-column sums of squares of the finalised rows: 16 products and 15 adds in fp32, any order"""
    R, N = xfin.shape
    want = (xfin.astype(np.float64) ** 2).reshape(R, N // 16, 16).sum(-1)
    if layout == "tile_major":
        want = want.T
    assert ss.shape == want.shape, (tag, ss.shape)
    assert (np.abs(ss - want) <= 32 * U24 * want + 1e-37).all(), (tag, "ss_out")


def _gemv_case(tag, fam, prec, pro_name, epi_name, R, N, K, ksb, seed, gather=False, ss_gran=0, with_bias=True):
    rng = np.random.default_rng(seed)
    pro, epi = PROS[pro_name], EPIS[epi_name]
    ldx, ldy, ldr = K + 8, (N // 2 if epi_name == "swiglu8" else N) + 5, N + 3
    w = _mk(rng, (N, K), prec, K ** -0.5)
    w2 = _mk(rng, (N, K), prec, K ** -0.5) if epi_name == "swiglu" else None
    bias = _mk(rng, N, prec) if with_bias and epi_name not in ("swiglu8",) else None
    nw = _rb(prec)((1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)) if pro_name != "plain" else None
    idx = None
    T = 5
    # in range, the last row, one past the table (reads the last row), negative (reads row 0)
    raw_idx = np.array([2, T - 1, T + 2, -3, 0, 1, 3, 4], np.int32)[:R]
    clamped = np.clip(raw_idx, 0, T - 1)
    xrows = T if (gather and pro_name == "norm") else R
    x = _mk(rng, (xrows, ldx), prec)
    res = None
    if epi_name == "slabfin":
        res = _mk(rng, (T if gather else R, ldr), prec)
    if gather:
        idx = np.full((R, 3), 1, np.int32)
        idx[:, 1] = raw_idx
    xr = x[clamped] if (gather and pro_name == "norm") else x
    xk = xr[:, :K]
    if pro_name == "plain":
        a = v_acc(xk, w)
        a2 = None
    else:
        c, dx = norm_ref(xk, nw, EPS, prec)
        a = v_acc(c, w, dx=dx)
        a2 = v_acc(c, w2, dx=dx) if w2 is not None else None
    b64 = None if bias is None else bias[None, :].astype(np.float64)
    rows, cols = R, N
    if epi_name in ("store", "f32"):
        v = v_rnd(v_add(a, b64), prec)
    elif epi_name == "swiglu":
        v = v_rnd(v_mul(v_rnd(v_silu(v_rnd(v_add(a, b64), prec)), prec), v_rnd(a2, prec)), prec)
    elif epi_name == "swiglu8":
        v = v_swiglu8(a, prec)
        cols = N // 2
    elif epi_name == "slab":
        v = v_add(a, b64)  # the sum of the K slices: no rounding at all (the ksb - 1 adds are in E's factor 2)
        rows = ksb * R
    else:
        rr = res[clamped] if gather else res
        v = v_rnd(v_add(v_rnd(v_add(a, b64), prec), rr[:, :N].astype(np.float64)), prec)
    ss = np.full((N // 16, R), SENT, np.float32) if epi_name == "slabfin" else None

    def go(buf, rp):
        if ss is not None:
            ss[:] = SENT
        return ops.gemv(w, x, buf, pro, epi, ksb, R=R, w2=w2, bias=bias, nw=nw, eps=EPS, idx=idx, idx_col=1, res=res,
                        ss_gran=ss_gran, ss_out=ss, precision=prec, reps=rp)

    (y1, d1), (y3, d3) = _run(go, (rows + 2, ldy))
    got = y1[:rows, :cols]
    if epi_name == "slab":
        parts = got.reshape(ksb, R, N).astype(np.float64)
        if ksb > 1:
            assert all(np.any(parts[q] != 0) for q in range(ksb)), (tag, "an empty K slice")
        got = _sum_parts(parts)
    _check(tag, fam, got, v)
    _sentinel(tag, y1, rows, cols)
    _same(tag, y1, y3)
    assert d1 == 0 and d3 == 0, (tag, d1, d3)
    if ss is not None:
        _ss_check(tag, ss, y3[:R, :N], "tile_major")
    return y1


def _gemv_n(epi_name, n):
    return {16: 16, 40: 48, 1000: 1008}[n] if epi_name in ("slabfin", "swiglu8") else n


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("pro,epi", GEMV_COMBOS)
def test_gemv(prec, pro, epi):
    """every dispatched (prologue, epilogue) pair at R 1, 2, 3, 7, 8 and N 16, 40, 1000 (part tile, many
    blocks): the smallest K (32: one k-step, three idle waves), K = 1344 (42 k-steps: 10 / 11 per wave),
    and with K slices (slab epilogues) 21 k-steps per slice at ksb 2 and 5 at ksb 4 (K = 640)."""
    fam = f"gemv/{pro}/{epi}/{prec}"
    slabs = epi in ("slab", "slabfin")
    cases = [(1, 16, 32, 1), (2, 40, 1344, 1), (3, 1000, 32, 1), (7, 16, 1344, 1), (8, 40, 32, 1), (8, 1000, 1344, 1)]
    if slabs:
        cases += [(2, 40, 1344, 2), (7, 1000, 640, 2), (3, 16, 640, 4), (8, 40, 640, 4)]
    for i, (R, n, K, ksb) in enumerate(cases):
        N = _gemv_n(epi, n)
        tag = f"gemv {prec} {pro}/{epi} R={R} N={N} K={K} ksb={ksb}"
        _gemv_case(tag, fam, prec, pro, epi, R, N, K, ksb, 1000 + 37 * i + R + K, with_bias=i % 2 == 0)


@pytest.mark.parametrize("prec", PRECS)
def test_gemv_prenorm_limits(prec):
    """PRO_PRENORM at its K limit (4096 columns: 256 tile sums per row in the reduction buffer), R = 8 and
    R = 1, and with the statistic from the staged row (ss_gran 1: one row, K <= 6144 -> 4096 here)."""
    for R, epi, g in ((8, "store", 0), (1, "swiglu8", 0), (1, "store", 1), (1, "f32", 1), (1, "swiglu8", 1)):
        tag = f"gemv {prec} prenorm/{epi} R={R} K=4096 ss_gran={g}"
        _gemv_case(tag, f"gemv/prenorm/{epi}/{prec}", prec, "prenorm", epi, R, 48, 4096, 1, 4096 + R + g, ss_gran=g)


@pytest.mark.parametrize("prec", PRECS)
def test_gemv_gather(prec):
    """xidx (PRO_NORM) and residx (EPI_SLABFIN) row gathers from a 5-row table through column 1 of a 3-wide
    index array: in-range indices, the last row, one index past the table and one negative -- the last two
    must read the clamped rows."""
    for R in (4, 8):
        _gemv_case(f"gemv {prec} gather norm/store R={R}", f"gemv/norm/store/{prec}", prec, "norm", "store", R, 40, 96, 1,
                   R, gather=True)
        _gemv_case(f"gemv {prec} gather plain/slabfin R={R}", f"gemv/plain/slabfin/{prec}", prec, "plain", "slabfin", R,
                   48, 640, 2, 50 + R, gather=True)


def test_gemv_variants(knob):
    """ring depth (gemv_u), non-temporal loads (gemv_nt) and the tail slots' dummy fragment (gemv_dummy) keep
    each wave's k order: the default's bits.  gemv_wpb 8 partitions the k-steps over 8 waves: another
    summation order, held to the bound on its own (inside _gemv_case)."""
    for pro, epi, R, N, K, ksb in (("plain", "slabfin", 3, 48, 640, 2), ("prenorm", "swiglu8", 8, 1008, 1344, 1),
                                   ("norm", "f32", 7, 40, 1344, 1)):
        args = (f"gemv/{pro}/{epi}/bf16", "bf16", pro, epi, R, N, K, ksb, 99)
        base = _gemv_case(f"gemv variants {pro}/{epi} default", *args)
        for key, vals in (("gemv_u", (2, 4, 8)), ("gemv_nt", (0, 1)), ("gemv_dummy", (0, 1, 2))):
            for val in vals:
                with tuned(**{key: val}):
                    _same(f"{key}={val}", base, _gemv_case(f"gemv variants {pro}/{epi} {key}={val}", *args))
        for val in (4, 8):
            with tuned(gemv_wpb=val):
                _gemv_case(f"gemv variants {pro}/{epi} gemv_wpb={val}", *args)


# ---------------------------------------------------------------------------------- launch_rowgemv
ROW_KINDS = {"fin": ops.ROW_FIN, "norm_store": ops.ROW_NORM_STORE, "norm_swiglu": ops.ROW_NORM_SWIGLU,
             "norm_f32": ops.ROW_NORM_F32}


def _row_case(tag, fam, kind_name, N, K, seed, q8=False, gather=False, with_bias=True):
    prec = "bf16"
    rng = np.random.default_rng(seed)
    kind = ROW_KINDS[kind_name]
    fin = kind_name == "fin"
    ldx, ldr = K + 8, N + 8
    w = _mk(rng, (N, K), prec, K ** -0.5)
    bias = _mk(rng, N, prec) if with_bias and not q8 and kind_name != "norm_swiglu" else None
    nw = None if fin else round_bf16((1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32))
    T = 5
    idx = np.array([7, 3, -2, T + 4], np.int32) if gather else None  # column picked per call below
    results = []
    for col in ((1, 2, 3) if gather else (0,)):
        sel = int(np.clip(idx[col], 0, T - 1)) if gather else 0
        x = _mk(rng, (T if (gather and not fin) else 1, ldx), prec)
        res = _mk(rng, (T if gather else 1, ldr), prec) if fin else None
        xk = x[sel if not fin else 0, :K][None, :]
        y_len = (N // 2 if kind_name == "norm_swiglu" else N)
        out = {}

        def go(buf, rp):
            out["q"] = ops.rowgemv(w, x, buf, kind, q8=q8, bias=bias, nw=nw, eps=EPS, res=res, idx=idx, idx_col=col, reps=rp)

        (y1, _), (y3, _) = _run(go, (1, y_len + 5))
        if fin:
            c, dx = xk.astype(np.float64), None
        else:
            c, dx = norm_ref(xk, nw, EPS, prec)
        if q8:
            q, sc = out["q"]
            q64 = q.astype(np.float64)
            # the kernel's own sum: (q + 128) . x - 128 sum(x)
            a = v_acc(c, q64, dx=dx, extra=lambda ax: ax @ np.abs(q64 + 128).T + 128 * ax.sum(-1, keepdims=True))
            a = v_q8(a, sc.astype(np.float64)[None, :], prec)
        else:
            a = v_add(v_acc(c, w, dx=dx), None if bias is None else bias[None, :].astype(np.float64))
        if fin:
            v = v_rnd(v_add(v_rnd(a, prec), res[sel, :N][None, :].astype(np.float64)), prec)
        elif kind_name == "norm_swiglu":
            rows = np.arange(N).reshape(-1, 8)
            v = v_swiglu(a[:, rows[:, :4].ravel()], a[:, rows[:, 4:].ravel()], prec)
        else:
            v = v_rnd(a, prec)
        t = f"{tag} col={col}" if gather else tag
        _check(t, fam, y1[:, :y_len], v)
        _sentinel(t, y1, 1, y_len)
        _same(t, y1, y3)
        results.append(y1)
    return results[0]


@pytest.mark.parametrize("K", [256, 512, 2304, 2560, 6144, 9728])
def test_rowgemv_fin(K):
    """FIN (wo / w2, 2 rows per block) at chunk depths U = 2, 2, 3, 3, 6, 10 per wave; N 2 and 6 (one and three
    blocks), 8, 16; bias on and off"""
    for i, N in enumerate((2, 6, 8, 16)):
        _row_case(f"rowgemv fin N={N} K={K}", "rowgemv/fin", "fin", N, K, K + N, with_bias=i % 2 == 0)


@pytest.mark.parametrize("kind", ["norm_store", "norm_swiglu", "norm_f32"])
@pytest.mark.parametrize("K", [256, 512, 2304, 2560, 6144])
def test_rowgemv_norm(kind, K):
    """the norm kinds (K <= 8 * 4 * 256) at N 8 and 16"""
    for N in (8, 16):
        _row_case(f"rowgemv {kind} N={N} K={K}", f"rowgemv/{kind}", kind, N, K, K + N + len(kind))


@pytest.mark.parametrize("kind,K", [("fin", 9728), ("norm_store", 2560), ("norm_swiglu", 2560), ("norm_f32", 6144)])
def test_rowgemv_many_blocks(kind, K):
    """N = 2560: 1280 / 320 blocks"""
    _row_case(f"rowgemv {kind} N=2560 K={K}", f"rowgemv/{kind}", kind, 2560, K, K)


@pytest.mark.parametrize("kind,K", [("fin", 512), ("fin", 9728), ("norm_store", 2560), ("norm_swiglu", 512), ("norm_f32", 2560),
                                    ("fin", 2560)])
def test_rowgemv_int8(kind, K):
    """the int8 codes, quantised on the device (launch_quant_rows): round(round(acc) * scale)"""
    for N in (8, 16):
        _row_case(f"rowgemv int8 {kind} N={N} K={K}", f"rowgemv_q8/{kind}", kind, N, K, 3 * K + N, q8=True)


def test_rowgemv_gather():
    """gathered X (norm kinds) and the gathered residual (FIN) from 5-row tables: an in-range index, a negative
    one and one past the table, which read the clamped rows"""
    _row_case("rowgemv gather fin", "rowgemv/fin", "fin", 16, 512, 1, gather=True)
    _row_case("rowgemv gather norm_store", "rowgemv/norm_store", "norm_store", 16, 512, 2, gather=True)
    _row_case("rowgemv gather norm_swiglu", "rowgemv/norm_swiglu", "norm_swiglu", 16, 2304, 3, gather=True)
    _row_case("rowgemv gather int8 fin", "rowgemv_q8/fin", "fin", 8, 512, 4, q8=True, gather=True)


def test_rowgemv_qkv_rows_per_block(knob):
    """fm_tune row_qkv_rp 4 / 8 / 16 at N = 48 regroups rows into blocks; each row's sum keeps its order"""
    outs = []
    for rp in (4, 8, 16):
        knob("row_qkv_rp", rp)
        outs.append(_row_case(f"rowgemv norm_store rp={rp}", "rowgemv/norm_store", "norm_store", 48, 2560, 11))
    _same("row_qkv_rp 4 vs 8", outs[0], outs[1])
    _same("row_qkv_rp 16 vs 8", outs[2], outs[1])


# ---------------------------------------------------------------------------------- launch_bstream
ALL_BSACC = {(s, {2: 4, 5: 2, 10: 1}[s], n) for s in (2, 5, 10) for n in (2, 3, 5, 6)}
_bs_plans = {}


def _bs_case(tag, fam, prec, epi_name, R, N, K, seed, prenorm=False, with_bias=True, want_acc=1):
    rng = np.random.default_rng(seed)
    epi = EPIS[epi_name]
    half = epi_name == "swiglu8"
    # whole tiles and ldy % 4 == 0: the 4-row epilogue (bs_vec_epi); else the scalar one
    ldx, ldy, ldr = K + 8, (N // 2 if half else N) + (8 if N % 16 == 0 else 5), N + 3
    w = _mk(rng, (N, K), prec, K ** -0.5)
    x = _mk(rng, (R, ldx), prec)
    bias = _mk(rng, N, prec) if with_bias and epi_name in ("store", "f32", "slabfin") else None
    nw = round_bf16((1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)) if prenorm else None
    res = _mk(rng, (R, ldr), prec) if epi_name == "slabfin" else None
    tiles = (N + 15) // 16
    ss = np.full((R, tiles), SENT, np.float32) if epi_name == "slabfin" else None
    if prenorm:
        c, dx = norm_ref(x[:, :K], nw, EPS, prec)
        a = v_acc(c, w, dx=dx)
    else:
        a = v_acc(x[:, :K], w)
    b64 = None if bias is None else bias[None, :].astype(np.float64)
    cols = N // 2 if half else N
    if epi_name in ("store", "f32"):
        v = v_rnd(v_add(a, b64), prec)
    elif half:
        v = v_swiglu8(a, prec)
    elif epi_name == "slab":
        v = a
    else:
        v = v_rnd(v_add(v_rnd(v_add(a, b64), prec), res[:, :N].astype(np.float64)), prec)
    rows_buf = (8 * R if epi_name == "slab" else R) + 2

    def go(buf, rp):
        if ss is not None:
            ss[:] = SENT
        return ops.bstream(w, x, buf, ops.PRO_PRENORM if prenorm else ops.PRO_PLAIN, epi, bias=bias, nw=nw, eps=EPS,
                           res=res, ss_out=ss, precision=prec, reps=rp)

    (y1, (plan, d1)), (y3, (_, d3)) = _run(go, (rows_buf, ldy))
    assert plan["acc"] == want_acc, (tag, plan)
    rows = R
    got = y1[:R, :cols]
    if epi_name == "slab":
        kp = plan["kparts"]
        rows = kp * R
        parts = y1[:rows, :N].reshape(kp, R, N).astype(np.float64)
        assert all(np.any(parts[q] != 0) for q in range(kp)), (tag, "an empty K part")
        got = _sum_parts(parts)
    _check(f"{tag} plan={plan}", fam, got, v)
    _sentinel(tag, y1, rows, cols)
    _same(tag, y1, y3)
    assert d1 == 0 and d3 == 0, (tag, d1, d3)
    if ss is not None:
        xf = np.zeros((R, tiles * 16), np.float32)
        xf[:, :N] = y3[:R, :N]
        _ss_check(tag, ss, xf, "row_major")
    return y1, plan


# K picks spw (<= 512: 2, 544 .. 1280: 5, 1312 .. 2560: 10), N picks ntm at 256 CUs (<= 8192: 2, .. 12288: 3,
# .. 20480: 5, .. 24576: 6); every K and N the issue lists appears
BSACC_GRID = [(9, 200, 480), (16, 8208, 256), (17, 12304, 480), (31, 20496, 256),
              (32, 200, 1248), (9, 8208, 544), (16, 12304, 1248), (17, 20496, 544),
              (31, 200, 2528), (32, 8208, 2528), (9, 12304, 1312), (16, 20496, 1312)]


@pytest.mark.parametrize("R,N,K", BSACC_GRID)
def test_bsacc_every_instantiation(R, N, K):
    """EPI_STORE on each of the twelve bsacc_kernel<SPW, TPI, NTM> instantiations (N = 200: the part tile and
    the scalar epilogue; the others: whole tiles, the 4-row epilogue)"""
    _, plan = _bs_case(f"bsacc store R={R} N={N} K={K}", "bsacc/store/bf16", "bf16", "store", R, N, K, N + K + R)
    assert (plan["spw"], plan["tpi"], plan["ntm"]) == _bsacc_cell(N, K), plan
    _bs_plans[(R, N, K)] = (plan["spw"], plan["tpi"], plan["ntm"])


def _bsacc_cell(N, K):
    """the instantiation bsacc_plan picks at 256 CUs with one K part (the table above BSACC_GRID)"""
    spw = 2 if K <= 512 else (5 if K <= 1280 else 10)
    tiles = (N + 15) // 16
    per = (tiles + 255) // 256
    return spw, {2: 4, 5: 2, 10: 1}[spw], 2 if per <= 2 else (3 if per == 3 else (5 if per <= 5 else 6))


def test_bsacc_instantiations_all_covered():
    """the grid names all twelve instantiations, and (each case above having held the hook's plan to its cell)
    so do the plans the hook returned: a device with another CU count fails loudly instead of silently testing
    less.  The returned set is compared once the whole grid has run in this session."""
    assert {_bsacc_cell(N, K) for _, N, K in BSACC_GRID} == ALL_BSACC
    if len(_bs_plans) == len(BSACC_GRID):
        assert set(_bs_plans.values()) == ALL_BSACC, sorted(ALL_BSACC - set(_bs_plans.values()))


BS_SMALL = [("f32", 9, 200, 256), ("f32", 32, 208, 1312), ("slab", 17, 200, 512), ("slab", 31, 208, 2560),
            ("swiglu8", 16, 208, 544), ("swiglu8", 32, 8208 - 16, 256), ("slabfin", 9, 200, 512), ("slabfin", 32, 208, 2560),
            ("store", 17, 40, 32), ("store", 31, 24, 96)]


@pytest.mark.parametrize("epi,R,N,K", BS_SMALL)
def test_bsacc_epilogues(epi, R, N, K):
    """the other epilogues (fp32, raw K-part slabs, SwiGLU8, slabs + residual finalise with its sums of
    squares and ticket) and the shortest K (one and three k-steps: fewer than 8 waves); bias on and off"""
    for with_bias in (True, False):
        _bs_case(f"bsacc {epi} R={R} N={N} K={K} bias={int(with_bias)}", f"bsacc/{epi}/bf16", "bf16", epi, R, N, K,
                 N + K + R + with_bias, with_bias=with_bias)


@pytest.mark.parametrize("epi,R,N,K", [("store", 9, 200, 256), ("store", 32, 208, 2560), ("swiglu8", 17, 208, 544),
                                       ("swiglu8", 31, 4096, 2560), ("store", 16, 6144, 2560)])
def test_bsacc_prenorm(epi, R, N, K):
    """PRO_PRENORM (X' from the producer's sums of squares [R][K / 16]) with STORE and SWIGLU8"""
    _bs_case(f"bsacc prenorm {epi} R={R} N={N} K={K}", f"bsacc_prenorm/{epi}/bf16", "bf16", epi, R, N, K, N + K + R,
             prenorm=True)


@pytest.mark.parametrize("epi,R,N,K,kparts", [("store", 32, 6144, 2560, 1), ("slab", 17, 2560, 4096, 8),
                                              ("slab", 32, 2560, 9728, 8), ("swiglu8", 32, 4096, 2560, 1),
                                              ("slabfin", 32, 2560, 4096, 8)])
def test_bsacc_production_geometries(epi, R, N, K, kparts):
    """S2-Pro's wqkv, wo (8 K parts), w2 and w1 || w3 at 256 CUs"""
    _, plan = _bs_case(f"bsacc prod {epi} R={R} N={N} K={K}", f"bsacc/{epi}/bf16", "bf16", epi, R, N, K, N + K)
    assert plan["kparts"] == kparts, plan


def test_bsacc_variants(knob):
    """bs_dummy 0 / 1 / 2, bs_xfirst 0 / 1 and bs_vec_epi 0 / 1 keep the summation order: the default's bits"""
    for epi, R, N, K in (("store", 17, 8208, 544), ("swiglu8", 32, 208, 1312), ("slab", 31, 208, 2560), ("f32", 9, 200, 256)):
        args = (f"bsacc/{epi}/bf16", "bf16", epi, R, N, K, 77)
        base, _ = _bs_case(f"bsacc variants {epi} default", *args)
        for key, vals in (("bs_dummy", (0, 1, 2)), ("bs_xfirst", (0, 1)), ("bs_vec_epi", (0, 1))):
            for val in vals:
                with tuned(**{key: val}):
                    _same(f"{key}={val}", base, _bs_case(f"bsacc variants {epi} {key}={val}", *args)[0])


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("epi,R,N,K", [("store", 9, 200, 256), ("f32", 17, 208, 1312), ("slab", 32, 200, 2560),
                                       ("store", 31, 1000, 544), ("slab", 16, 208, 4096)])
def test_bstream_kernel(prec, epi, R, N, K, knob):
    """the older bstream_kernel (fm_tune bstream_acc 0; what fp32 batched frames and the shapes bsacc_plan
    declines run on): STORE / F32 / SLAB in both precisions"""
    knob("bstream_acc", 0)
    _bs_case(f"bstream {prec} {epi} R={R} N={N} K={K}", f"bstream/{epi}/{prec}", prec, epi, R, N, K, N + K + R, want_acc=0)


def test_bstream_kernelv_swiglu8(knob):
    knob("bstream_acc", 0)
    _bs_case("bstream bf16 swiglu8", "bstream/swiglu8/bf16", "bf16", "swiglu8", 17, 208, 544, 3, want_acc=0)


# ---------------------------------------------------------------------------------- launch_finalize_norm
def _ulp(v, prec):
    a = np.maximum(np.abs(v).astype(np.float32), np.float32(2.0 ** -126))
    return np.exp2(np.floor(np.log2(a)) - 7).astype(np.float64) if prec == "bf16" else np.spacing(a).astype(np.float64)


def _ulp_check(tag, fam, got, ref, prec):
    """the 1 bf16 ulp / 4 fp32 ulp form of test_gpu_ops._check, the bit-exact share printed and held"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    d = np.abs(got - ref)
    ulp = _ulp(np.maximum(np.abs(got), np.abs(ref)), prec)
    share = float((d == 0).mean())
    lo, hi, n = _seen.get(fam, (1.0, 0.0, 0))
    _seen[fam] = (min(lo, share), max(hi, float((d / ulp).max())), n + 1)
    print(f"{fam} | {tag}: {share * 100:.2f}% bit-exact, max |d| / ulp {float((d / ulp).max()):.3f}")
    assert (d <= (1 if prec == "bf16" else 4) * ulp).all(), (tag, float((d / ulp).max()))
    assert share >= _floor(fam), (tag, share)


def _fin_case(tag, prec, d, R, kparts, bias_on, ws_on, nw_on, seed):
    rng = np.random.default_rng(seed)
    lds, ldr, ldo = d + 4, d + 8, d + 3
    slab = (rng.standard_normal((kparts, R, lds)) * (40.0 if ws_on else 1.0)).astype(np.float32)
    res = _mk(rng, (R, ldr), prec)
    bias = _mk(rng, d, prec) if bias_on else None
    nw = _rb(prec)((1.0 + 0.1 * rng.standard_normal(d)).astype(np.float32)) if nw_on else None
    ws = _rb(prec)((0.01 + 0.02 * rng.random(d)).astype(np.float32)) if ws_on else None
    rb = _rb(prec)
    # the documented chain in fp32, K parts added in order (numpy float32 adds are the kernel's)
    y = np.zeros((R, d), np.float32)
    for q in range(kparts):
        y = y + slab[q, :, :d]
    if bias is not None:
        y = y + bias[None, :]
    if ws is not None:
        y = rb(rb(y) * ws[None, :])
    xref = rb(res[:, :d] + rb(y))
    xo = _buf(R + 2, ldo)
    xn = _buf(R + 1, ldo + 1) if nw_on else None
    outs = []
    for rp in (1, 3):
        a, b = xo.copy(), (None if xn is None else xn.copy())
        split, err, dirty = ops.finalize_norm(slab, res, a, d, bias=bias, nw=nw, wscale=ws, xn_out=b, eps=EPS, precision=prec,
                                              reps=rp)
        assert err == 0 and dirty == 0, (tag, err, dirty)
        outs.append((a, b, split))
    (a1, b1, split), (a3, b3, _) = outs
    _ulp_check(tag + " x", f"finalize/x/{prec}", a1[:R, :d], xref, prec)
    _sentinel(tag, a1, R, d)
    _same(tag, a1, a3)
    if nw_on:
        got_x = a1[:R, :d].astype(np.float64)
        rs = 1.0 / np.sqrt((got_x ** 2).mean(-1, keepdims=True) + EPS)
        t = got_x * rs
        xnref = _rd(_rd(t, prec) * nw.astype(np.float64), prec)
        _ulp_check(tag + " xn", f"finalize/xn/{prec}", b1[:R, :d], xnref, prec)
        _sentinel(tag, b1, R, d)
        _same(tag, b1, b3)
    return a1, b1, split


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ch", [0, 2, 5])
@pytest.mark.parametrize("d", [8, 128, 2560, 8192])
def test_finalize_norm(prec, ch, d, knob):
    """d 8 (one item), 128, 2560 and the widest row the launcher admits (8 * 512 * 2); R 1, 9, 32, 64; K parts
    1, 2, 4, 8; bias, int8 scales and the norm each on and off; one block per row and the split form
    (fm_tune fin_split = ch; 5 does not divide d / 8), which launch_finalize_norm takes when a chunk fits 64
    threads; fin8 0 / 1 give the same bits."""
    knob("fin_split", ch)
    fits = ch > 1 and (d // 8 + ch - 1) // ch <= 64
    for i, (R, kparts) in enumerate(((1, 1), (9, 2), (32, 4), (64, 8))):
        bias_on, ws_on, nw_on = bool(i & 1), i == 2, i != 1
        tag = f"finalize {prec} d={d} R={R} kparts={kparts} ch={ch} bias={int(bias_on)} ws={int(ws_on)} nw={int(nw_on)}"
        res = []
        for f8 in (1, 0):
            with tuned(fin8=f8):
                res.append(_fin_case(tag + f" fin8={f8}", prec, d, R, kparts, bias_on, ws_on, nw_on, d + R + ch))
        assert res[0][2] == (fits and R * ch <= 1024), (tag, res[0][2])
        _same(tag + " fin8", res[0][0], res[1][0])
        if nw_on:
            _same(tag + " fin8 xn", res[0][1], res[1][1])


# ---------------------------------------------------------------------------------- launch_prompt_skinny
# (K, target): slice depths of 16 / 20 / 40 / 80 k-steps (4 / 5 / 10 / 20 chunks: the unrolled forms), 24 (6
# chunks) and 8 (one slice of 8 k-steps: 2 chunks), and K = 2560 in 4 slices of 20
SKINNY_K = [(512, 1, 1), (640, 1, 1), (1280, 1, 1), (2560, 1, 1), (768, 1, 1), (256, 1, 1), (2560, 4, None)]


def _skinny_case(tag, R, N, K, target, act, seed):
    rng = np.random.default_rng(seed)
    prec = "bf16"
    ldx = K + 8
    w = _mk(rng, (N, K), prec, K ** -0.5)
    x = _mk(rng, (R, ldx), prec)
    ks = ops.prompt_skinny_ks(N, K, target)
    assert ks >= 1, (tag, ks)
    a = v_acc(x[:, :K], w)
    if act:
        assert ks == 1
        v, rows, cols, shape = v_swiglu8(a, prec), R, N // 2, (R + 2, N // 2 + 5)
    else:
        v, rows, cols, shape = a, ks * R, N, (ks * R + 2, N)
    (y1, k1), (y3, _) = _run(lambda buf, rp: ops.prompt_skinny(w, x, buf, target, act=act, reps=rp), shape)
    assert k1 == ks
    got = y1[:rows, :cols]
    if not act:
        parts = got.reshape(ks, R, N).astype(np.float64)
        assert all(np.any(parts[q] != 0) for q in range(ks)), (tag, "an empty K slice")
        got = _sum_parts(parts)
    _check(f"{tag} ks={ks}", "skinny/act" if act else "skinny/slab", got, v)
    _sentinel(tag, y1, rows, cols)
    _same(tag, y1, y3)
    return y1, ks


@pytest.mark.parametrize("K,target,want_ks", SKINNY_K)
def test_prompt_skinny(K, target, want_ks, knob):
    """raw slabs [ks][R][N] at R 33, 48, 49, 64 and N 16, 80 (the last 64-row group holds one tile), 2560;
    the unrolled form (prompt_unroll 1) and the loop give the same bits"""
    for R, N in ((33, 16), (48, 80), (49, 2560), (64, 80)):
        if target > 1 and N != 16:
            continue
        outs = []
        for un in (1, 0):
            with tuned(prompt_unroll=un):
                y, ks = _skinny_case(f"skinny R={R} N={N} K={K} unroll={un}", R, N, K, target, False, R + N + K)
                outs.append(y)
        if want_ks is not None:
            assert ks == want_ks
        else:
            assert ks == 4, ks
        _same("prompt_unroll", outs[0], outs[1])


@pytest.mark.parametrize("K", [256, 640, 768, 2560])
def test_prompt_skinny_direct_swiglu(K):
    """one slice, act set: the interleaved SwiGLU straight from the accumulators (swiglu_i8_kernel's roundings)"""
    for R, N in ((33, 16), (64, 80), (49, 2560)):
        outs = []
        for un in (1, 0):
            with tuned(prompt_unroll=un):
                outs.append(_skinny_case(f"skinny act R={R} N={N} K={K} unroll={un}", R, N, K, 1, True, R + N + K)[0])
        _same("prompt_unroll act", outs[0], outs[1])
