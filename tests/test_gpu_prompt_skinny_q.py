"""The skinny prompt GEMM's code-reading forms (prompt_skinny_kernel WM 1 / 2, fm_prompt.hip) through
fm_op_prompt_skinny_q: the hook quantises a bf16-valued weight on the device with the model's rule, packs the
bf16 fragments and the step-granular codes with the model's pack launchers, and runs launch_prompt_skinny once
per form on the same rows.  The code form rebuilds every bf16 fragment bit for bit and keeps mode 0's slices,
steps and accumulators, so the two outputs are compared with array_equal; the bf16 form's output is then held
to test_gpu_linear_ops.py's bounds (its docstring derives them) of the float64 product over the dequantised
codes the hook returns: the raw slabs' sum to the accumulation bound alone, the direct SwiGLU through its
rounding chain -- int8: gate and up are round(round(acc) * scale) first (v_q8), then v_swiglu8.  The bit-exact
shares against the restatement are printed, not held (no floor is recorded for these families).
Run on the MI355X box: pytest -m gpu; the slice-plan test needs no device."""
import numpy as np
import pytest

from fishmi import ops
from linear_ref import mk as _mk, v_acc, v_q8, v_swiglu8
from parity_util import tuned
from test_gpu_linear_ops import _buf, _check, _same, _sentinel, _sum_parts
from test_gpu_quant_compact import _dequant4

# (K, target, ks, k-steps per slice): 2 chunks in the loop form; 4 / 5 / 10 / 20 chunks (the unrolled forms); 6
# chunks (loop); K = 2560 in 4 slices of 20; K = 1152 in 2 slices of 18 (unrolled 5 with a partial last chunk: the
# second slice starts two steps into a 128-k unit) and in 4 slices of 9 (loop, 3 chunks: slices start 1, 2, 3
# steps into a unit) -- the smallest shapes at which the int4 unit selection can go wrong
PLANS = [(256, 1, 1, 8), (512, 1, 1, 16), (640, 1, 1, 20), (1280, 1, 1, 40), (2560, 1, 1, 80), (768, 1, 1, 24),
         (2560, 4, 4, 20), (1152, 2, 2, 18), (1152, 4, 4, 9)]
QUANTS = [("int8", 128), ("int4", 128), ("int4", 256)]
ROWS = (33, 48, 49, 64)
COLS = (16, 80, 2560)
# int4: the K that are whole groups (multiples of 128, and of 256 at gs 256)
SLAB_CASES = [(q, gs) + p for q, gs in QUANTS for p in PLANS if q == "int8" or p[0] % gs == 0]
ACT_CASES = [(q, gs, K) for q, gs in QUANTS for K in (256, 640, 768, 2560) if q == "int8" or K % gs == 0]


@pytest.mark.parametrize("K,target,ks,steps", PLANS)
def test_slice_plans(K, target, ks, steps):
    """prompt_skinny_ks gives the table's slices at N = 16 (the planner call needs no device)"""
    assert ops.prompt_skinny_ks(16, K, target) == ks and K // 32 // ks == steps
    if target == 1:
        for N in COLS:
            assert ops.prompt_skinny_ks(N, K, 1) == 1


def _weights(rng, N, K, quant):
    """seeded weights scaled by 1 / sqrt(K).  int8: rows 0 and 1 hold a dominant +- 127.5 * 2^e (about 8 sigma,
    bf16-exact), so their scale is 2^e exactly and the quotients are +- 127.5: code 127 (128 clamped) and code
    -128 (the tie rounds to even) occur whatever the draw.  int4: a group's minimum is code 0, its maximum 15."""
    w = _mk(rng, (N, K), "bf16", K ** -0.5)
    if quant == "int8":
        w[0, 3] = np.float32(127.5 * 2.0 ** (np.round(np.log2(K ** -0.5)) - 4))
        w[1, 5] = -w[0, 3]
    return w


def _dequant(quant, q, sc, zr):
    return q.astype(np.float32) if quant == "int8" else _dequant4(q, sc, zr)


def _case(quant, gs, R, N, K, target, act, want_ks=None):
    rng = np.random.default_rng(R + N + K + gs + 7 * target)
    ldx = K + 8
    w, x = _weights(rng, N, K, quant), _mk(rng, (R, ldx), "bf16")
    ks = ops.prompt_skinny_ks(N, K, target)
    assert ks >= 1 and (want_ks is None or ks == want_ks), ks
    rows, cols, shape = (R, N // 2, (R + 2, N // 2 + 5)) if act else (ks * R, N, (ks * R + 2, N))
    tag = f"skinny_q {quant} gs={gs} R={R} N={N} K={K} ks={ks} act={int(act)}"
    outs = []
    for unroll, reps in ((1, 1), (1, 3), (0, 1)):
        yq, yb = _buf(*shape), _buf(*shape)
        with tuned(prompt_unroll=unroll):
            k1, q, sc, zr = ops.prompt_skinny_q(w, x, yq, yb, quant, target, gs=gs, act=act, reps=reps)
        assert k1 == ks
        _same(f"{tag} unroll={unroll} reps={reps}: codes vs bf16 fragments", yq, yb)
        _sentinel(tag, yq, rows, cols)
        _sentinel(tag, yb, rows, cols)
        outs.append(yb)
    _same(tag + " reps 3 vs 1", outs[0], outs[1])
    _same(tag + " prompt_unroll 0 vs 1", outs[0], outs[2])
    lo, hi = (-128, 127) if quant == "int8" else (0, 15)
    assert q.min() == lo and q.max() == hi, (tag, int(q.min()), int(q.max()))
    a = v_acc(x[:, :K], _dequant(quant, q, sc, zr))
    got = outs[0][:rows, :cols]
    if act:
        if quant == "int8":
            a = v_q8(a, sc[None, :].astype(np.float64), "bf16")
        v = v_swiglu8(a, "bf16")
    else:
        parts = got.reshape(ks, R, N).astype(np.float64)
        assert all(np.any(parts[p] != 0) for p in range(ks)), (tag, "an empty K slice")
        got, v = _sum_parts(parts), a
    _check(tag, f"skinny_q/{quant}/{'act' if act else 'slab'}", got, v)


@pytest.mark.gpu
@pytest.mark.parametrize("quant,gs,K,target,ks,steps", SLAB_CASES)
def test_codes_equal_fragments_slabs(quant, gs, K, target, ks, steps):
    """raw slabs [ks][R][N]: R 33 / 48 / 49 / 64 x N 16 / 80 (the last 64-row group holds one tile) / 2560; the
    sliced plans at N = 16"""
    for R in ROWS:
        for N in COLS if target == 1 else (16,):
            _case(quant, gs, R, N, K, target, False, want_ks=ks)


@pytest.mark.gpu
@pytest.mark.parametrize("quant,gs,K", ACT_CASES)
def test_codes_equal_fragments_direct_swiglu(quant, gs, K):
    """one slice, act set: the interleaved SwiGLU straight from the accumulators, with the int8 row scales"""
    for R in ROWS:
        for N in COLS:
            _case(quant, gs, R, N, K, 1, True, want_ks=1)


def test_int4_refuses_other_groups():
    """FM_ERR_ARG for int4 unless the group size and K are multiples of 128 (refused before any device call)"""
    from fishmi import native

    rng = np.random.default_rng(1)
    for K, gs in ((256, 64), (288, 32), (320, 128)):
        w, x = _mk(rng, (16, K), "bf16"), _mk(rng, (33, K), "bf16")
        with pytest.raises(native.FishMIError) as e:
            ops.prompt_skinny_q(w, x, _buf(35, 16), _buf(35, 16), "int4", 1, gs=gs)
        assert e.value.code == -1
